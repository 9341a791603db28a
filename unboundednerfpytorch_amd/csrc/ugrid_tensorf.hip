// TensoRF (vector-matrix) grids of the reference's DirectVoxGO / DirectContractedVoxGO (grid.py:90-201): the factorised lookup, its
// backward into the six factors and f_vec, the total-variation gradient of the factors and the dense bake.
//
//   value(x,y,z)[c] = sum over rows of feat[row] * f_vec[row, c]        (C > 1;  C == 1: the plain sum of feat)
//   feat = [ xy_plane_r(x,y) * z_vec_r(z)  (Rxy rows) | xz_plane_r(x,z) * y_vec_r(y)  (R rows) | yz_plane_r(y,z) * x_vec_r(x)  (R rows) ]
// with every plane sampled bilinearly and every vector linearly, grid_sample(align_corners=True, zeros padding) arithmetic: index
// ((u + 1) / 2) * (n - 1), weights (floor + 1) - index and index - floor, a corner outside [0, n-1] contributes nothing.
//
// Layouts (`comp_last`): canonical = the reference's [1,R,A,B] planes and [1,R,N,1] vectors (component slowest); component-last =
// torch.channels_last of the same logical tensors, [A][B][R] and [N][R] (a texel's R components are one run).
//
// One lane per point (query, backward) / per voxel (bake) / per factor element (TV).  The backward recomputes the interpolants (no
// [n, rows] tensor is kept from the forward) and accumulates as DESIGN.md 4.6 sizes it: plane gradients with fp32 global atomics; the
// f_vec gradient as a per-workgroup [rows x points] . [points x C] product out of LDS, kept in LDS across the workgroup's tiles and
// flushed with one atomic per element per workgroup; the vector gradients in LDS per workgroup where the three vectors fit beside
// that, else with global atomics.
#include "ugrid_common.h"
#include "ugrid_tensorf.h"      // the lookup leaves and tf_density, shared with the sampling march

#define ST(s) ((hipStream_t)(s))
#define TF_CMAX 16          // channels of one grid (a lane keeps them in registers; the f_vec product gives 16 lanes to a row)
#define TF_ROWS 16          // feature rows staged per step of the f_vec product
#define TF_PAD 257          // LDS row pitch of the 256-point staging arrays (256 + 1: the 4 rows a wave reads sit in 4 banks)
#define TF_LDS_MAX 65536
#define TF_FVEC_MAX 3072      // floats of f_vec ((2R + Rxy) * C): it and its gradient sit in LDS beside the 32 KB of staging

struct tf_grads {
  float *plane[3];
  float *vec[3];
};
__device__ __forceinline__ float *tf_selp(float *const *p, int g) { return g == 0 ? p[0] : (g == 1 ? p[1] : p[2]); }

// ---------------------------------------------------------------------------------------------- forward
template <bool CL>
__global__ void __launch_bounds__(256) k_tensorf_query(tf_factors f, const float *__restrict__ f_vec, int C, const float *__restrict__ xyz,
                                                       const float *__restrict__ xyz_min, const float *__restrict__ xyz_max, int64_t n,
                                                       float *__restrict__ out) {
  extern __shared__ float tf_sm[];
  const int rows = f.Rg[0] + f.Rg[1] + f.Rg[2];
  if (C > 1) {
    for (int i = threadIdx.x; i < rows * C; i += blockDim.x) tf_sm[i] = f_vec[i];
    __syncthreads();
  }
  const float lo0 = xyz_min[0], lo1 = xyz_min[1], lo2 = xyz_min[2], hi0 = xyz_max[0], hi1 = xyz_max[1], hi2 = xyz_max[2];
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
    const float ux = ((xyz[3 * p] - lo0) / (hi0 - lo0)) * 2.f - 1.f, uy = ((xyz[3 * p + 1] - lo1) / (hi1 - lo1)) * 2.f - 1.f,
                uz = ((xyz[3 * p + 2] - lo2) / (hi2 - lo2)) * 2.f - 1.f;
    if (C == 1) {
      out[p] = tf_density<CL>(f, ux, uy, uz);          // (ugrid_tensorf.h: the sampling march calls the same function)
      continue;
    }
    const tf_ax ax = tf_axis(ux, f.N[2]);
    const tf_ax ay = tf_axis(uy, f.N[1]);
    const tf_ax az = tf_axis(uz, f.N[0]);
    float acc[TF_CMAX];
#pragma unroll
    for (int c = 0; c < TF_CMAX; ++c) acc[c] = 0.f;
    int row = 0;
#pragma unroll 1
    for (int g = 0; g < 3; ++g) {
      TF_GROUP_TAPS(g, ta, tb, tv);
      const tf_group q = tf_sel(f, g);
      for (int r = 0; r < q.Rg; ++r, ++row) {
        const float feat = tf_plane_val<CL>(q.plane, q.Rg, q.A, q.B, r, ta, tb) * tf_vec_val<CL>(q.vec, q.Rg, q.N, r, tv);
        const float *__restrict__ fr = tf_sm + row * C;
#pragma unroll
        for (int c = 0; c < TF_CMAX; ++c)
          if (c < C) acc[c] += feat * fr[c];
      }
    }
#pragma unroll
    for (int c = 0; c < TF_CMAX; ++c)
      if (c < C) out[p * C + c] = acc[c];
  }
}

// ---------------------------------------------------------------------------------------------- backward
// LDS (floats): C > 1: f_vec [rows*C] | its gradient [rows*C] | feat [TF_ROWS][TF_PAD] | grad_out [TF_CMAX][TF_PAD];  behind that
// DOUBLE accumulators (a workgroup's sum over its points carries no fp32 rounding; each element then gets one fp32 atomic per
// workgroup): ACC == 1: of the three vector gradients [Rg*N each] -- few rows, every point adds to them: the contended, slow case of
// global atomics;  ACC == 2 (small grids): of the planes too, planes first;  ACC == 0: nothing fits, global atomics only.
template <bool CL, int ACC>
__global__ void __launch_bounds__(256) k_tensorf_query_backward(tf_factors f, tf_grads gr, const float *__restrict__ f_vec, float *__restrict__ g_fvec, int C,
                                                                const float *__restrict__ grad_out, const float *__restrict__ xyz,
                                                                const float *__restrict__ xyz_min, const float *__restrict__ xyz_max, int64_t n) {
  extern __shared__ float tf_sm[];
  const int tid = threadIdx.x;
  const int rows = f.Rg[0] + f.Rg[1] + f.Rg[2];
  float *f_s = tf_sm, *facc = f_s + rows * C, *feat_s = facc + rows * C, *g_s = feat_s + TF_ROWS * TF_PAD;
  double *dacc = (double *)(C > 1 ? g_s + TF_CMAX * TF_PAD : tf_sm);          // (the float count before it is even)
  // element counts of the three vectors / planes (the planes' only where they fit in LDS, ACC == 2): formed where they are used, not
  // kept in scalar registers across the tile loop
#define TF_VN(g) (f.Rg[g] * f.N[g])
#define TF_PN(g) (f.Rg[g] * f.A[g] * f.B[g])
  if (C > 1)
    for (int i = tid; i < rows * C; i += 256) { f_s[i] = f_vec[i]; facc[i] = 0.f; }
  const int ptot = ACC == 2 ? TF_PN(0) + TF_PN(1) + TF_PN(2) : 0;
  if (ACC >= 1)
    for (int i = tid; i < ptot + TF_VN(0) + TF_VN(1) + TF_VN(2); i += 256) dacc[i] = 0.0;
  __syncthreads();
  float lo0 = xyz_min[0], lo1 = xyz_min[1], lo2 = xyz_min[2], hi0 = xyz_max[0], hi1 = xyz_max[1], hi2 = xyz_max[2];
  // the six bounds live in VECTOR registers (an empty asm with a "+v" constraint, no instruction): kept scalar across the tile loop
  // they pushed the canonical ACC == 1 instantiation four registers over the scalar file
  asm volatile("" : "+v"(lo0), "+v"(lo1), "+v"(lo2), "+v"(hi0), "+v"(hi1), "+v"(hi2));
  for (int64_t tile0 = (int64_t)blockIdx.x * 256; tile0 < n; tile0 += (int64_t)gridDim.x * 256) {
    const int64_t p = tile0 + tid;
    const bool valid = p < n;
    const int64_t pc = valid ? p : n - 1;          // (a lane past the end computes on the last point with a zero gradient: it adds nothing)
    const tf_ax ax = tf_axis(((xyz[3 * pc] - lo0) / (hi0 - lo0)) * 2.f - 1.f, f.N[2]);
    const tf_ax ay = tf_axis(((xyz[3 * pc + 1] - lo1) / (hi1 - lo1)) * 2.f - 1.f, f.N[1]);
    const tf_ax az = tf_axis(((xyz[3 * pc + 2] - lo2) / (hi2 - lo2)) * 2.f - 1.f, f.N[0]);
    float g1 = 0.f;
    if (C == 1) {
      g1 = valid ? grad_out[p] : 0.f;
    } else {
      for (int c = 0; c < C; ++c) g_s[c * TF_PAD + tid] = valid ? grad_out[p * C + c] : 0.f;      // (read back by this lane, and after the barrier by the product)
    }
    int rowbase = 0, vbase = 0, pbase = 0;
#pragma unroll 1
    for (int g = 0; g < 3; ++g) {
      TF_GROUP_TAPS(g, ta, tb, tv);
      const tf_group q = tf_sel(f, g);
      const int Rg = q.Rg, A = q.A, B = q.B, N = q.N;
      float *__restrict__ gp = tf_selp(gr.plane, g), *__restrict__ gv = tf_selp(gr.vec, g);
      for (int r0 = 0; r0 < Rg; r0 += TF_ROWS) {
        const int cnt = Rg - r0 < TF_ROWS ? Rg - r0 : TF_ROWS;
        for (int rr = 0; rr < cnt; ++rr) {
          const int r = r0 + rr;
          const float pv = tf_plane_val<CL>(q.plane, Rg, A, B, r, ta, tb), vv = tf_vec_val<CL>(q.vec, Rg, N, r, tv);
          float dfeat = g1;
          if (C > 1) {
            feat_s[rr * TF_PAD + tid] = pv * vv;
            const float *__restrict__ fr = f_s + (rowbase + r) * C;
            dfeat = 0.f;
            for (int c = 0; c < C; ++c) dfeat += g_s[c * TF_PAD + tid] * fr[c];
          }
          if (dfeat == 0.f) continue;                 // (no barrier inside this loop)
          const float dp = dfeat * vv, dv = dfeat * pv;
          const float w00 = tb.w0 * ta.w0, w01 = tb.w1 * ta.w0, w10 = tb.w0 * ta.w1, w11 = tb.w1 * ta.w1;
          if (ACC == 2) {
            double *__restrict__ dp_ = dacc + pbase;
            if (w00 != 0.f) atomicAdd(dp_ + (int)tf_pidx<CL>(Rg, A, B, r, ta.i0, tb.i0), (double)(dp * w00));
            if (w01 != 0.f) atomicAdd(dp_ + (int)tf_pidx<CL>(Rg, A, B, r, ta.i0, tb.i1), (double)(dp * w01));
            if (w10 != 0.f) atomicAdd(dp_ + (int)tf_pidx<CL>(Rg, A, B, r, ta.i1, tb.i0), (double)(dp * w10));
            if (w11 != 0.f) atomicAdd(dp_ + (int)tf_pidx<CL>(Rg, A, B, r, ta.i1, tb.i1), (double)(dp * w11));
          } else {
            if (w00 != 0.f) unsafeAtomicAdd(gp + tf_pidx<CL>(Rg, A, B, r, ta.i0, tb.i0), dp * w00);
            if (w01 != 0.f) unsafeAtomicAdd(gp + tf_pidx<CL>(Rg, A, B, r, ta.i0, tb.i1), dp * w01);
            if (w10 != 0.f) unsafeAtomicAdd(gp + tf_pidx<CL>(Rg, A, B, r, ta.i1, tb.i0), dp * w10);
            if (w11 != 0.f) unsafeAtomicAdd(gp + tf_pidx<CL>(Rg, A, B, r, ta.i1, tb.i1), dp * w11);
          }
          if (ACC >= 1) {
            double *__restrict__ dv_ = dacc + ptot + vbase;
            if (tv.w0 != 0.f) atomicAdd(dv_ + (int)tf_vidx<CL>(Rg, N, r, tv.i0), (double)(dv * tv.w0));
            if (tv.w1 != 0.f) atomicAdd(dv_ + (int)tf_vidx<CL>(Rg, N, r, tv.i1), (double)(dv * tv.w1));
          } else {
            if (tv.w0 != 0.f) unsafeAtomicAdd(gv + tf_vidx<CL>(Rg, N, r, tv.i0), dv * tv.w0);
            if (tv.w1 != 0.f) unsafeAtomicAdd(gv + tf_vidx<CL>(Rg, N, r, tv.i1), dv * tv.w1);
          }
        }
        if (C > 1) {
          // grad f_vec[row, c] += sum over the tile's points of feat[row, point] * grad_out[point, c]: lane (rr, c) owns one element
          __syncthreads();
          const int rr = tid >> 4, c = tid & 15;
          if (rr < cnt && c < C) {
            const float *__restrict__ fs = feat_s + rr * TF_PAD, *__restrict__ gs = g_s + c * TF_PAD;
            double s = 0.0;          // (the 256 products of a tile summed without fp32 rounding)
            for (int q = 0; q < 256; ++q) s += (double)(fs[q] * gs[q]);
            facc[(rowbase + r0 + rr) * C + c] += (float)s;
          }
          __syncthreads();
        }
      }
      rowbase += Rg;
      vbase += Rg * N;
      pbase += Rg * A * B;
    }
    if (C > 1) __syncthreads();        // the next tile overwrites g_s
  }
  __syncthreads();
  if (C > 1)
    for (int i = tid; i < rows * C; i += 256)
      if (facc[i] != 0.f) unsafeAtomicAdd(g_fvec + i, facc[i]);
  if (ACC >= 1) {
    int off = 0;
#define TF_FLUSH(dst, count)                                                                  \
  do {                                                                                        \
    const int cnt_ = (count);                                                                 \
    for (int i = tid; i < cnt_; i += 256)                                                     \
      if (dacc[off + i] != 0.0) unsafeAtomicAdd((dst) + i, (float)dacc[off + i]);             \
    off += cnt_;                                                                              \
  } while (0)
    if (ACC == 2) {
      TF_FLUSH(gr.plane[0], TF_PN(0));
      TF_FLUSH(gr.plane[1], TF_PN(1));
      TF_FLUSH(gr.plane[2], TF_PN(2));
    }
    TF_FLUSH(gr.vec[0], TF_VN(0));
    TF_FLUSH(gr.vec[1], TF_VN(1));
    TF_FLUSH(gr.vec[2], TF_VN(2));
#undef TF_FLUSH
  }
#undef TF_VN
#undef TF_PN
}

// ---------------------------------------------------------------------------------------------- total variation
// Gradient of the reference's TV loss (grid.py:142-154: smooth-L1, beta = 1, over every adjacent pair of every factor, the weight of
// the pair's axis, / 6) in the gather form: d/da_j = c * (clamp(a_j - a_(j-1)) - clamp(a_(j+1) - a_j)), clamp to [-1, 1].
__device__ __forceinline__ float tf_clamp1(float d) { return fminf(fmaxf(d, -1.f), 1.f); }
__device__ __forceinline__ float tf_tv_axis(float v, const float *__restrict__ t, int64_t prev, int64_t next, bool has_prev, bool has_next, float c) {
  float s = 0.f;
  if (has_prev) s += c * tf_clamp1(v - t[prev]);
  if (has_next) s -= c * tf_clamp1(t[next] - v);
  return s;
}
template <bool CL>
__global__ void __launch_bounds__(256) k_tensorf_tv(tf_factors f, tf_grads gr, float cx, float cy, float cz) {
  int64_t tot = 0;
#pragma unroll
  for (int g = 0; g < 3; ++g) tot += (int64_t)f.Rg[g] * f.A[g] * f.B[g] + (int64_t)f.Rg[g] * f.N[g];
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += (int64_t)gridDim.x * blockDim.x) {
    int64_t beg = 0;          // elements in the order: the three planes, then the three vectors
#pragma unroll 1
    for (int g = 0; g < 3; ++g) {
      const tf_group q = tf_sel(f, g);
      const int64_t sz = (int64_t)q.Rg * q.A * q.B;
      if (e >= beg && e < beg + sz) {                     // a plane element: its two axes
        const int Rg = q.Rg, A = q.A, B = q.B;
        int64_t i = e - beg;
        int r, a, b;
        if (CL) { r = (int)(i % Rg); i /= Rg; b = (int)(i % B); a = (int)(i / B); }
        else { b = (int)(i % B); i /= B; a = (int)(i % A); r = (int)(i / A); }
        const float *__restrict__ t = q.plane;
        const float v = t[e - beg];
        const float ca = g == 2 ? cy : cx, cb = g == 0 ? cy : cz;
        float s = tf_tv_axis(v, t, tf_pidx<CL>(Rg, A, B, r, a > 0 ? a - 1 : a, b), tf_pidx<CL>(Rg, A, B, r, a + 1 < A ? a + 1 : a, b), a > 0, a + 1 < A, ca);
        s += tf_tv_axis(v, t, tf_pidx<CL>(Rg, A, B, r, a, b > 0 ? b - 1 : b), tf_pidx<CL>(Rg, A, B, r, a, b + 1 < B ? b + 1 : b), b > 0, b + 1 < B, cb);
        tf_selp(gr.plane, g)[e - beg] += s;
      }
      beg += sz;
    }
#pragma unroll 1
    for (int g = 0; g < 3; ++g) {
      const tf_group q = tf_sel(f, g);
      const int64_t sz = (int64_t)q.Rg * q.N;
      if (e >= beg && e < beg + sz) {                     // a vector element: its one axis
        const int Rg = q.Rg, N = q.N;
        const int64_t i = e - beg;
        const int r = CL ? (int)(i % Rg) : (int)(i / N), k = CL ? (int)(i / Rg) : (int)(i % N);
        const float *__restrict__ t = q.vec;
        const float cv = g == 0 ? cz : (g == 1 ? cy : cx);
        tf_selp(gr.vec, g)[i] += tf_tv_axis(t[i], t, tf_vidx<CL>(Rg, N, r, k > 0 ? k - 1 : k), tf_vidx<CL>(Rg, N, r, k + 1 < N ? k + 1 : k), k > 0, k + 1 < N, cv);
      }
      beg += sz;
    }
  }
}

// ---------------------------------------------------------------------------------------------- bake
// dense[c][x][y][z] (OCL: [x][y][z][c]) = get_dense_grid (grid.py:156-169), one lane per voxel, no intermediate
template <bool CL, bool OCL>
__global__ void __launch_bounds__(256) k_tensorf_bake(tf_factors f, const float *__restrict__ f_vec, int C, int X, int Y, int Z, float *__restrict__ out) {
  extern __shared__ float tf_sm[];
  const int rows = f.Rg[0] + f.Rg[1] + f.Rg[2];
  if (C > 1) {
    for (int i = threadIdx.x; i < rows * C; i += blockDim.x) tf_sm[i] = f_vec[i];
    __syncthreads();
  }
  const int64_t vol = (int64_t)X * Y * Z;
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < vol; v += (int64_t)gridDim.x * blockDim.x) {
    const int z = (int)(v % Z), y = (int)((v / Z) % Y), x = (int)(v / ((int64_t)Z * Y));
    float acc[TF_CMAX];
#pragma unroll
    for (int c = 0; c < TF_CMAX; ++c) acc[c] = 0.f;
    float total = 0.f;
    int row = 0;
#pragma unroll 1
    for (int g = 0; g < 3; ++g) {
      const int a = g == 2 ? y : x, b = g == 0 ? y : z, k = g == 0 ? z : (g == 1 ? y : x);
      const tf_group q = tf_sel(f, g);
      float sg = 0.f;
      for (int r = 0; r < q.Rg; ++r, ++row) {
        const float feat = q.plane[tf_pidx<CL>(q.Rg, q.A, q.B, r, a, b)] * q.vec[tf_vidx<CL>(q.Rg, q.N, r, k)];
        if (C == 1) {
          sg += feat;
        } else {
          const float *__restrict__ fr = tf_sm + row * C;
#pragma unroll
          for (int c = 0; c < TF_CMAX; ++c)
            if (c < C) acc[c] += feat * fr[c];
        }
      }
      total = g == 0 ? sg : total + sg;
    }
    if (C == 1) {
      out[v] = total;
    } else {
#pragma unroll
      for (int c = 0; c < TF_CMAX; ++c)
        if (c < C) out[OCL ? v * C + c : (int64_t)c * vol + v] = acc[c];
    }
  }
}

// ---------------------------------------------------------------------------------------------- C ABI
static bool tf_shape_ok(int X, int Y, int Z, int R, int Rxy, int C) {
  return X >= 1 && Y >= 1 && Z >= 1 && R >= 1 && Rxy >= 1 && C >= 1 && C <= TF_CMAX && (int64_t)(2 * R + Rxy) * C <= TF_FVEC_MAX;
}
static unsigned tf_grid_dim(int64_t items) {
  const int64_t b = (items + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > 8192 ? 8192 : b));          // grid-stride kernels: at most 8192 workgroups (32 per CU)
}

extern "C" int ugrid_tensorf_query(const float *xy_plane, const float *xz_plane, const float *yz_plane, const float *x_vec, const float *y_vec,
                                   const float *z_vec, const float *f_vec, int X, int Y, int Z, int R, int Rxy, int C, int comp_last,
                                   const float *xyz, const float *xyz_min, const float *xyz_max, int64_t n, float *out, ugrid_stream_t s) {
  if (!tf_shape_ok(X, Y, Z, R, Rxy, C) || (C > 1 && !f_vec)) return (int)hipErrorInvalidValue;
  if (n <= 0) return 0;
  const tf_factors f = tf_make(xy_plane, xz_plane, yz_plane, x_vec, y_vec, z_vec, X, Y, Z, R, Rxy);
  const size_t lds = C > 1 ? (size_t)(2 * R + Rxy) * C * 4 : 0;
  if (comp_last)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tensorf_query<true>), dim3(tf_grid_dim(n)), dim3(256), lds, ST(s), f, f_vec, C, xyz, xyz_min, xyz_max, n, out);
  else
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tensorf_query<false>), dim3(tf_grid_dim(n)), dim3(256), lds, ST(s), f, f_vec, C, xyz, xyz_min, xyz_max, n, out);
  UG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ugrid_tensorf_query_backward(const float *grad_out, const float *xy_plane, const float *xz_plane, const float *yz_plane,
                                            const float *x_vec, const float *y_vec, const float *z_vec, const float *f_vec, int X, int Y, int Z,
                                            int R, int Rxy, int C, int comp_last, const float *xyz, const float *xyz_min, const float *xyz_max,
                                            int64_t n, float *g_xy_plane, float *g_xz_plane, float *g_yz_plane, float *g_x_vec, float *g_y_vec,
                                            float *g_z_vec, float *g_f_vec, ugrid_stream_t s) {
  if (!tf_shape_ok(X, Y, Z, R, Rxy, C) || (C > 1 && (!f_vec || !g_f_vec))) return (int)hipErrorInvalidValue;
  const tf_factors f = tf_make(xy_plane, xz_plane, yz_plane, x_vec, y_vec, z_vec, X, Y, Z, R, Rxy);
  tf_grads gr;
  gr.plane[0] = g_xy_plane; gr.vec[0] = g_z_vec;
  gr.plane[1] = g_xz_plane; gr.vec[1] = g_y_vec;
  gr.plane[2] = g_yz_plane; gr.vec[2] = g_x_vec;
  for (int g = 0; g < 3; ++g) {
    UG_HIP(hipMemsetAsync(gr.plane[g], 0, (size_t)f.Rg[g] * f.A[g] * f.B[g] * 4, ST(s)));
    UG_HIP(hipMemsetAsync(gr.vec[g], 0, (size_t)f.Rg[g] * f.N[g] * 4, ST(s)));
  }
  const int rows = 2 * R + Rxy;
  if (C > 1) UG_HIP(hipMemsetAsync(g_f_vec, 0, (size_t)rows * C * 4, ST(s)));
  if (n <= 0) return 0;
  const size_t base = C > 1 ? ((size_t)2 * rows * C + (TF_ROWS + TF_CMAX) * TF_PAD) * 4 : 0;
  const size_t vbytes = ((size_t)Rxy * Z + (size_t)R * Y + (size_t)R * X) * 4;
  const size_t pbytes = ((size_t)Rxy * X * Y + (size_t)R * X * Z + (size_t)R * Y * Z) * 4;
  const int acc = base + 2 * (pbytes + vbytes) <= TF_LDS_MAX ? 2 : (base + 2 * vbytes <= TF_LDS_MAX ? 1 : 0);
  const size_t lds = base + (acc == 2 ? 2 * (pbytes + vbytes) : acc == 1 ? 2 * vbytes : 0);
  // a workgroup walks several 256-point tiles, so that its LDS sums are flushed once for all of them: at most 4 workgroups per CU
  const int64_t tiles = (n + 255) / 256;
  const unsigned blocks = (unsigned)(tiles < 1024 ? tiles : 1024);
#define TF_BWD(CLv, VL)                                                                                                                  \
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tensorf_query_backward<CLv, VL>), dim3(blocks), dim3(256), lds, ST(s), f, gr, f_vec, g_f_vec, C, \
                     grad_out, xyz, xyz_min, xyz_max, n)
  if (comp_last) { if (acc == 2) TF_BWD(true, 2); else if (acc == 1) TF_BWD(true, 1); else TF_BWD(true, 0); }
  else { if (acc == 2) TF_BWD(false, 2); else if (acc == 1) TF_BWD(false, 1); else TF_BWD(false, 0); }
#undef TF_BWD
  UG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ugrid_tensorf_tv_add_grad(const float *xy_plane, const float *xz_plane, const float *yz_plane, const float *x_vec,
                                         const float *y_vec, const float *z_vec, float *g_xy_plane, float *g_xz_plane, float *g_yz_plane,
                                         float *g_x_vec, float *g_y_vec, float *g_z_vec, int X, int Y, int Z, int R, int Rxy, int comp_last,
                                         float wx, float wy, float wz, ugrid_stream_t s) {
  if (!tf_shape_ok(X, Y, Z, R, Rxy, 1)) return (int)hipErrorInvalidValue;
  const tf_factors f = tf_make(xy_plane, xz_plane, yz_plane, x_vec, y_vec, z_vec, X, Y, Z, R, Rxy);
  tf_grads gr;
  gr.plane[0] = g_xy_plane; gr.vec[0] = g_z_vec;
  gr.plane[1] = g_xz_plane; gr.vec[1] = g_y_vec;
  gr.plane[2] = g_yz_plane; gr.vec[2] = g_x_vec;
  int64_t tot = 0;
  for (int g = 0; g < 3; ++g) tot += (int64_t)f.Rg[g] * f.A[g] * f.B[g] + (int64_t)f.Rg[g] * f.N[g];
  // the coefficient autograd forms for `loss /= 6` of `w * smooth_l1(...)`: fl(fl(1/6) * w)
  const float sixth = 1.f / 6.f;
  if (comp_last)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tensorf_tv<true>), dim3(tf_grid_dim(tot)), dim3(256), 0, ST(s), f, gr, sixth * wx, sixth * wy, sixth * wz);
  else
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tensorf_tv<false>), dim3(tf_grid_dim(tot)), dim3(256), 0, ST(s), f, gr, sixth * wx, sixth * wy, sixth * wz);
  UG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ugrid_tensorf_bake(const float *xy_plane, const float *xz_plane, const float *yz_plane, const float *x_vec, const float *y_vec,
                                  const float *z_vec, const float *f_vec, int X, int Y, int Z, int R, int Rxy, int C, int comp_last,
                                  int out_channels_last, float *out, ugrid_stream_t s) {
  if (!tf_shape_ok(X, Y, Z, R, Rxy, C) || (C > 1 && !f_vec)) return (int)hipErrorInvalidValue;
  const tf_factors f = tf_make(xy_plane, xz_plane, yz_plane, x_vec, y_vec, z_vec, X, Y, Z, R, Rxy);
  const size_t lds = C > 1 ? (size_t)(2 * R + Rxy) * C * 4 : 0;
  const unsigned blocks = tf_grid_dim((int64_t)X * Y * Z);
#define TF_BAKE(CLv, OC) \
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tensorf_bake<CLv, OC>), dim3(blocks), dim3(256), lds, ST(s), f, f_vec, C, X, Y, Z, out)
  if (comp_last) { if (out_channels_last) TF_BAKE(true, true); else TF_BAKE(true, false); }
  else { if (out_channels_last) TF_BAKE(false, true); else TF_BAKE(false, false); }
#undef TF_BAKE
  UG_LAUNCH_CHECK();
  return 0;
}
