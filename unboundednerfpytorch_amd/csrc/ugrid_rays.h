// Ray / box / mask-cache leaves of the sample_pts_on_rays family, shared by the drop-in kernels of ugrid_ops.hip and the
// stage set-up kernels (ugrid_hit_coarse_geo there, ugrid_count_views_accumulate in ugrid_query.hip).  Every expression here is
// a bit-exactness contract with the reference kernels (render_utils_kernel.cu, pinned by tests/golden/native_ops.npz): a kernel
// that needs one of them calls it, none restates it.  Compiled with -ffp-contract=off like everything else (csrc/build.sh).
#pragma once
#include "ugrid_common.h"

// ----------------------------------------------------------------------------------------------
// Ray / AABB helpers (1 lane per ray; 12-byte AoS rays are read as 3 dwords, L1 absorbs the stride)
// ----------------------------------------------------------------------------------------------
struct ug_tmm { float tmin, tmax; };

__device__ __forceinline__ ug_tmm ug_t_minmax(const float *o, const float *d, const float *lo,
                                              const float *hi, float near, float far) {
  // a zero direction component is replaced by float(1e-6) (double literal narrowed)
  const float vx = (d[0] == 0.f) ? (float)1e-6 : d[0];
  const float vy = (d[1] == 0.f) ? (float)1e-6 : d[1];
  const float vz = (d[2] == 0.f) ? (float)1e-6 : d[2];
  const float ax = (hi[0] - o[0]) / vx, ay = (hi[1] - o[1]) / vy, az = (hi[2] - o[2]) / vz;
  const float bx = (lo[0] - o[0]) / vx, by = (lo[1] - o[1]) / vy, bz = (lo[2] - o[2]) / vz;
  ug_tmm r;
  r.tmin = fmaxf(fminf(fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fminf(az, bz)), far), near);
  r.tmax = fmaxf(fminf(fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz)), far), near);
  return r;
}

__device__ __forceinline__ float ug_norm3(const float *d) {
  return sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
}

__device__ __forceinline__ int64_t ug_n_samples(const float *d, float tmin, float tmax, float stepdist) {
  const double c = (double)ceilf((tmax - tmin) * ug_norm3(d) / stepdist);
  return (int64_t)(c > 1. ? c : 1.);
}

// sample `step` of a ray of sample_pts_on_rays: start + dir * dist per axis with start = o + d * t_min, dir = d / |d|,
// dist = stepdist * step (rn = ug_norm3(d)); returns mask_outbbox of the point
__device__ __forceinline__ bool ug_sample_point(const float *o, const float *d, float rn, float tm, float stepdist, int step,
                                                const float *lo, const float *hi, float *p) {
  const float dist = stepdist * (float)step;
  for (int c = 0; c < 3; ++c) {
    const float start = o[c] + d[c] * tm;
    const float dir = d[c] / rn;
    p[c] = start + dir * dist;
  }
  return (lo[0] > p[0]) | (lo[1] > p[1]) | (lo[2] > p[2]) | (hi[0] < p[0]) | (hi[1] < p[1]) | (hi[2] < p[2]);
}

// maskcache_lookup's voxel of a point: the flat index into world [sz_i,sz_j,sz_k], or -1 outside it
__device__ __forceinline__ int64_t ug_mask_index(const float *p, const float *scale, const float *shift, int64_t sz_i, int64_t sz_j,
                                                 int64_t sz_k) {
  float fi = roundf(p[0] * scale[0] + shift[0]);
  float fj = roundf(p[1] * scale[1] + shift[1]);
  float fk = roundf(p[2] * scale[2] + shift[2]);
  // the reference converts the rounded value with `const int i = round(...)` (render_utils_kernel.cu:385-387): the
  // hardware float->int conversion saturates and maps NaN to 0 (v_cvt_i32_f32, and cvt.rzi.s32.f32 on the
  // reference's own target), so a NaN coordinate indexes plane 0 of that axis -- pinned on the reference kernels
  // themselves (tests/golden/native_ops.npz); +-inf / huge values saturate out of range
  fi = (fi != fi) ? 0.f : fi; fj = (fj != fj) ? 0.f : fj; fk = (fk != fk) ? 0.f : fk;
  if (fi >= 0.f && fi < (float)sz_i && fj >= 0.f && fj < (float)sz_j && fk >= 0.f && fk < (float)sz_k)
    return (int64_t)fi * sz_j * sz_k + (int64_t)fj * sz_k + (int64_t)fk;
  return -1;
}
