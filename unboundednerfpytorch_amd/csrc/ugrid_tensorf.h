// The lookup leaves of a TensoRF (vector-matrix) grid, shared by csrc/ugrid_tensorf.hip (query, backward, TV, bake) and the fused
// sampling march of csrc/ugrid_sample.hip (k_train_march_tensorf): ONE definition of the factorised density.  Every translation unit
// of the library is built with -ffp-contract=off, so one source expression gives one result in every kernel that includes this.
#pragma once
#include "ugrid_common.h"

struct tf_ax { int i0, i1; float w0, w1; };      // the two vertices along one axis: clamped into range, weight 0 where outside

__device__ __forceinline__ tf_ax tf_axis(float u, int n) {
  const float ix = ((u + 1.f) / 2.f) * (float)(n - 1);
  const float f = floorf(ix);
  const float w0 = (f + 1.f) - ix, w1 = ix - f;
  const int i = (int)fminf(fmaxf(f, -2.f), (float)n);
  const bool in0 = i >= 0 && i < n, in1 = i + 1 >= 0 && i + 1 < n;
  tf_ax a;
  a.i0 = in0 ? i : (in1 ? i + 1 : 0);
  a.i1 = in1 ? i + 1 : a.i0;
  a.w0 = in0 ? w0 : 0.f;
  a.w1 = in1 ? w1 : 0.f;
  return a;
}

// the factors of one grid and its sizes; group g = 0: xy_plane [Rxy,X,Y] with z_vec, 1: xz_plane [R,X,Z] with y_vec, 2: yz_plane [R,Y,Z]
// with x_vec (the reference's pairing, grid.py:176-187)
struct tf_factors {
  const float *plane[3];
  const float *vec[3];
  int A[3], B[3], N[3], Rg[3];      // plane [Rg,A,B], vector [Rg,N]
};

static tf_factors tf_make(const float *xy, const float *xz, const float *yz, const float *xv, const float *yv, const float *zv, int X, int Y,
                          int Z, int R, int Rxy) {
  tf_factors f;
  f.plane[0] = xy; f.vec[0] = zv; f.A[0] = X; f.B[0] = Y; f.N[0] = Z; f.Rg[0] = Rxy;
  f.plane[1] = xz; f.vec[1] = yv; f.A[1] = X; f.B[1] = Z; f.N[1] = Y; f.Rg[1] = R;
  f.plane[2] = yz; f.vec[2] = xv; f.A[2] = Y; f.B[2] = Z; f.N[2] = X; f.Rg[2] = R;
  return f;
}

template <bool CL>
__device__ __forceinline__ int64_t tf_pidx(int Rg, int A, int B, int r, int a, int b) {
  return CL ? ((int64_t)a * B + b) * Rg + r : ((int64_t)r * A + a) * B + b;
}
template <bool CL>
__device__ __forceinline__ int64_t tf_vidx(int Rg, int N, int r, int k) {
  return CL ? (int64_t)k * Rg + r : (int64_t)r * N + k;
}

// group g's factors by uniform selects: the group loops run rolled (`#pragma unroll 1`), so that one group's sizes and pointers are
// live at a time -- unrolled, the three groups' kernel arguments and products overflowed the scalar registers
struct tf_group { const float *plane, *vec; int A, B, N, Rg; };
__device__ __forceinline__ tf_group tf_sel(const tf_factors &f, int g) {
  tf_group q;
  q.plane = g == 0 ? f.plane[0] : (g == 1 ? f.plane[1] : f.plane[2]);
  q.vec = g == 0 ? f.vec[0] : (g == 1 ? f.vec[1] : f.vec[2]);
  q.A = g == 0 ? f.A[0] : (g == 1 ? f.A[1] : f.A[2]);
  q.B = g == 0 ? f.B[0] : (g == 1 ? f.B[1] : f.B[2]);
  q.N = g == 0 ? f.N[0] : (g == 1 ? f.N[1] : f.N[2]);
  q.Rg = g == 0 ? f.Rg[0] : (g == 1 ? f.Rg[1] : f.Rg[2]);
  return q;
}

// the axis taps of group g from the three per-axis taps (x, y, z): plane rows, plane columns, vector
#define TF_GROUP_TAPS(g, ta, tb, tv)                          \
  const tf_ax &ta = (g) == 2 ? ay : ax;                       \
  const tf_ax &tb = (g) == 0 ? ay : az;                       \
  const tf_ax &tv = (g) == 0 ? az : ((g) == 1 ? ay : ax)

template <bool CL>
__device__ __forceinline__ float tf_plane_val(const float *__restrict__ p, int Rg, int A, int B, int r, const tf_ax &ta, const tf_ax &tb) {
  // grid_sample's corner order and weight products: (row 0, col 0), (row 0, col 1), (row 1, col 0), (row 1, col 1); weight = col * row
  const float v00 = p[tf_pidx<CL>(Rg, A, B, r, ta.i0, tb.i0)], v01 = p[tf_pidx<CL>(Rg, A, B, r, ta.i0, tb.i1)];
  const float v10 = p[tf_pidx<CL>(Rg, A, B, r, ta.i1, tb.i0)], v11 = p[tf_pidx<CL>(Rg, A, B, r, ta.i1, tb.i1)];
  float acc = v00 * (tb.w0 * ta.w0);
  acc += v01 * (tb.w1 * ta.w0);
  acc += v10 * (tb.w0 * ta.w1);
  acc += v11 * (tb.w1 * ta.w1);
  return acc;
}
template <bool CL>
__device__ __forceinline__ float tf_vec_val(const float *__restrict__ v, int Rg, int N, int r, const tf_ax &tv) {
  float acc = v[tf_vidx<CL>(Rg, N, r, tv.i0)] * tv.w0;
  acc += v[tf_vidx<CL>(Rg, N, r, tv.i1)] * tv.w1;
  return acc;
}

// the single-channel (density) value at the normalised coordinates (ux, uy, uz) in [-1, 1]: the sum of the feature rows, group by
// group, (s0 + s1) + s2 in the reference's association.  k_tensorf_query (C == 1) and k_train_march_tensorf both call this: the march
// stores the bits the stand-alone query gives.
template <bool CL>
__device__ __forceinline__ float tf_density(const tf_factors &f, float ux, float uy, float uz) {
  const tf_ax ax = tf_axis(ux, f.N[2]);
  const tf_ax ay = tf_axis(uy, f.N[1]);
  const tf_ax az = tf_axis(uz, f.N[0]);
  float total = 0.f;
#pragma unroll 1
  for (int g = 0; g < 3; ++g) {
    TF_GROUP_TAPS(g, ta, tb, tv);
    const tf_group q = tf_sel(f, g);
    float acc = 0.f;
    for (int r = 0; r < q.Rg; ++r)
      acc += tf_plane_val<CL>(q.plane, q.Rg, q.A, q.B, r, ta, tb) * tf_vec_val<CL>(q.vec, q.Rg, q.N, r, tv);
    total = g == 0 ? acc : total + acc;          // (s0 + s1) + s2, the reference's association
  }
  return total;
}
