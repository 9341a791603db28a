// libugrid_hip.so -- the grid lookup of the training path on the canonical layout: k_grid_query, its backward and the view counting
// of the coarse stage.  Built with -fno-slp-vectorize like the march these kernels were split from (csrc/build.sh).
#include "ugrid_render.h"
#include "ugrid_rays.h"
#include "ugrid_taps.h"

// ----------------------------------------------------------------------------------------------
// stand-alone grid query on the canonical layout (FourierGrid.forward / DenseGrid.forward).
// 1 lane per point; corner taps are z-pairs in the [.., Z] fastest dimension.
// ----------------------------------------------------------------------------------------------
// forward: 1 lane per point; per level the taps are set up once and reused by every channel; the per-channel sums
// over levels build up in the output row itself (level 0 first, like the reference's mean over the level axis).
// CL = channel-last storage [P][X][Y][Z][C] (torch channels_last_3d of the same logical [P,C,X,Y,Z] tensor: the C
// channels of a voxel are one contiguous run -- the training layout of multi-channel grids, section 4.4 of DESIGN.md);
// the arithmetic and its order are the same in both layouts.
template <bool CL>
__device__ __forceinline__ void ug_grid_query_one(int64_t tid, const float *__restrict__ grid, int P, int C, int X, int Y, int Z,
                                                  const float *__restrict__ xyz, const float *__restrict__ xyz_min,
                                                  const float *__restrict__ xyz_max, int F, int64_t n, float *__restrict__ out) {
  // canonical layout: one lane per point, levels and channels in loops.  channel-last: one lane per (point, channel),
  // channel fastest -- the C lanes of a point read one 4C-byte voxel record per corner; same per-channel operation order
  const int64_t p = CL ? tid / C : tid;
  if (p >= n) return;
  const float ux = ug_unorm(xyz[3 * p], xyz_min[0], xyz_max[0]);
  const float uy = ug_unorm(xyz[3 * p + 1], xyz_min[1], xyz_max[1]);
  const float uz = ug_unorm(xyz[3 * p + 2], xyz_min[2], xyz_max[2]);
  const int64_t vol = (int64_t)X * Y * Z;
  if (CL) {
    const int ch = (int)(tid - p * C);
    auto level = [&](int l, float cx, float cy, float cz) -> float {
      const ug_taps t = ug_tap_setup_ld(X, Y, Z, cx, cy, cz);
      const float *__restrict__ g = grid + (int64_t)l * vol * C + ch;
      float acc = 0.f;
#pragma unroll
      for (int c = 0; c < 8; ++c) acc += g[t.off[c] * C] * t.w[c];
      return acc;
    };
    // level 0, then the sin and the cos level of every frequency TOGETHER: one sin / cos evaluation serves both (ug_level_coords formed it
    // once per level) and their 16 corner loads are in flight at once; the level sums are added in level order as before: bit-identical
    float sum = level(0, ux, uy, uz);
    for (int k = 0; 2 * k + 2 < P; ++k) {
      const float f = (float)(1 << k);
      float sx, kx, sy, ky, sz, kz;
      ug_sincos(f * ux, &sx, &kx);
      ug_sincos(f * uy, &sy, &ky);
      ug_sincos(f * uz, &sz, &kz);
      const ug_taps ts = ug_tap_setup_ld(X, Y, Z, sx, sy, sz), tc = ug_tap_setup_ld(X, Y, Z, kx, ky, kz);
      const float *__restrict__ gs = grid + (int64_t)(2 * k + 1) * vol * C + ch, *__restrict__ gc = grid + (int64_t)(2 * k + 2) * vol * C + ch;
      float vs[8], vc[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) vs[c] = gs[ts.off[c] * C];
#pragma unroll
      for (int c = 0; c < 8; ++c) vc[c] = gc[tc.off[c] * C];
      float as = 0.f, ac = 0.f;
#pragma unroll
      for (int c = 0; c < 8; ++c) as += vs[c] * ts.w[c];
#pragma unroll
      for (int c = 0; c < 8; ++c) ac += vc[c] * tc.w[c];
      sum = sum + as;
      sum = sum + ac;
    }
    out[tid] = (F > 0) ? sum / (float)P : sum;
    return;
  }
  float *__restrict__ row = out + p * C;
  {
    const ug_taps t = ug_tap_setup_ld(X, Y, Z, ux, uy, uz);
    for (int ch = 0; ch < C; ++ch) {
      const float *__restrict__ g = grid + (int64_t)ch * vol;
      float acc = 0.f;
#pragma unroll
      for (int c = 0; c < 8; ++c) acc += g[t.off[c]] * t.w[c];
      row[ch] = acc;
    }
  }
  for (int k = 0; 2 * k + 2 < P; ++k) {          // the sin and the cos level of a frequency together (one sin / cos evaluation, 16 loads in flight)
    const float f = (float)(1 << k);
    float sx, kx, sy, ky, sz, kz;
    ug_sincos(f * ux, &sx, &kx);
    ug_sincos(f * uy, &sy, &ky);
    ug_sincos(f * uz, &sz, &kz);
#pragma unroll
    for (int half = 0; half < 2; ++half) {          // the sin level, then the cos level (one sin / cos evaluation serves both)
      const ug_taps t = half == 0 ? ug_tap_setup_ld(X, Y, Z, sx, sy, sz) : ug_tap_setup_ld(X, Y, Z, kx, ky, kz);
      for (int ch = 0; ch < C; ++ch) {
        const float *__restrict__ g = grid + ((int64_t)(2 * k + 1 + half) * C + ch) * vol;
        float acc = 0.f;
#pragma unroll
        for (int c = 0; c < 8; ++c) acc += g[t.off[c]] * t.w[c];
        row[ch] = row[ch] + acc;
      }
    }
  }
  if (F > 0)
    for (int ch = 0; ch < C; ++ch) row[ch] = row[ch] / (float)P;
}
// n_dev (may be null): the row count on the device (ug_devn, ugrid_common.h); grid-stride, so that a grid sized by a hint covers any count
template <bool CL>
__global__ void k_grid_query(const float *__restrict__ grid, int P, int C, int X, int Y, int Z,
                             const float *__restrict__ xyz, const float *__restrict__ xyz_min,
                             const float *__restrict__ xyz_max, int F, int64_t n, float *__restrict__ out,
                             const int64_t *__restrict__ n_dev) {
  UG_DEVN_CLAMP(n, n_dev);
  const int64_t total = CL ? n * C : n;
  for (int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; tid < total; tid += (int64_t)gridDim.x * blockDim.x)
    ug_grid_query_one<CL>(tid, grid, P, C, X, Y, Z, xyz, xyz_min, xyz_max, F, n, out);
}

// backward w.r.t. the grid: 1 lane per (point, level); grad_grid[l, ch, corner] += w * grad_out[p, ch] / P with
// hardware fp32 atomics (global_atomic_add_f32).  Like torch's grid_sample backward the accumulation order is
// not fixed, so sums agree to rounding, not bit for bit.  Canonical layout: the C atomics of a corner land in C
// different planes (32 MB apart at G = 200) -- every atomic its own 128-byte line; channel-last: one 4C-byte run.
// `touch` (channel-last only, may be null): one bit per 256-byte line (64 floats) of grad_grid, set for every line this
// launch adds to -- the masked TV / Adam passes then visit only those lines instead of scanning the whole gradient for
// non-zeros (ugrid_touch_words; the marking happens before the lane's own zero test, so that a record any channel of which
// receives a gradient is always marked).
template <bool CL>
__device__ __forceinline__ void ug_grid_query_backward_one(int64_t tid, const float *__restrict__ grad_out, int P, int C, int X, int Y, int Z,
                                                           const float *__restrict__ xyz, const float *__restrict__ xyz_min,
                                                           const float *__restrict__ xyz_max, int F, int64_t n,
                                                           float *__restrict__ grad_grid, uint32_t *__restrict__ touch) {
  // canonical layout: one lane per (point, level), channels in a loop (each channel is its own volume).
  // channel-last layout: one lane per (point, level, channel), channel fastest -- the C lanes of one (point, level) hit
  // C consecutive floats of one voxel record, so each atomic instruction touches ~64/C records instead of 64 lines.
  const int64_t q = CL ? tid / C : tid;
  const int chl = CL ? (int)(tid - q * C) : 0;
  if (q >= n * P) return;
  const int64_t p = q / P;
  const int l = (int)(q - p * P);
  const float ux = ug_unorm(xyz[3 * p], xyz_min[0], xyz_max[0]);
  const float uy = ug_unorm(xyz[3 * p + 1], xyz_min[1], xyz_max[1]);
  const float uz = ug_unorm(xyz[3 * p + 2], xyz_min[2], xyz_max[2]);
  float cx, cy, cz;
  ug_level_coords(l, ux, uy, uz, cx, cy, cz);
  const ug_taps t = ug_tap_setup(X, Y, Z, cx, cy, cz);
  const int64_t vol = (int64_t)X * Y * Z;
  if (CL) {
    if (touch) {
      // the two z-neighbours of a corner pair are adjacent records: one run of <= 2C floats, marked by one lane
      const int64_t e0 = (int64_t)l * vol * C;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if ((C >= 4 ? k : 0) != chl) continue;          // pair k is lane k's (a record with < 4 channels: all lane 0's)
        const int64_t lo = t.off[2 * k] >= 0 ? t.off[2 * k] : t.off[2 * k + 1];
        const int64_t hi = t.off[2 * k + 1] >= 0 ? t.off[2 * k + 1] : t.off[2 * k];
        if (lo < 0) continue;
        for (int64_t line = (e0 + lo * C) >> 6; line <= (e0 + hi * C + C - 1) >> 6; ++line) {
          const uint32_t bit = 1u << (line & 31);
          if (!(touch[line >> 5] & bit)) atomicOr(touch + (line >> 5), bit);
        }
      }
    }
    float g = grad_out[p * C + chl];
    if (F > 0) g = g / (float)P;
    if (g == 0.f) return;     // exact zeros stay exact zeros in the grid gradient (MaskedAdam keys on them)
    float *__restrict__ gl = grad_grid + (int64_t)l * vol * C + chl;
#pragma unroll
    for (int c = 0; c < 8; ++c)
      if (t.off[c] >= 0) unsafeAtomicAdd(gl + t.off[c] * C, g * t.w[c]);
    return;
  }
  for (int ch = 0; ch < C; ++ch) {
    float g = grad_out[p * C + ch];
    if (F > 0) g = g / (float)P;
    if (g == 0.f) continue;   // exact zeros stay exact zeros in the grid gradient (MaskedAdam keys on them)
    float *__restrict__ gg = grad_grid + ((int64_t)l * C + ch) * vol;
#pragma unroll
    for (int c = 0; c < 8; ++c)
      if (t.off[c] >= 0) unsafeAtomicAdd(gg + t.off[c], g * t.w[c]);
  }
}
template <bool CL>
__global__ void k_grid_query_backward(const float *__restrict__ grad_out, int P, int C, int X, int Y, int Z,
                                      const float *__restrict__ xyz, const float *__restrict__ xyz_min,
                                      const float *__restrict__ xyz_max, int F, int64_t n,
                                      float *__restrict__ grad_grid, uint32_t *__restrict__ touch, const int64_t *__restrict__ n_dev) {
  UG_DEVN_CLAMP(n, n_dev);
  const int64_t total = (CL ? n * C : n) * P;
  for (int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; tid < total; tid += (int64_t)gridDim.x * blockDim.x)
    ug_grid_query_backward_one<CL>(tid, grad_out, P, C, X, Y, Z, xyz, xyz_min, xyz_max, F, n, grad_grid, touch);
}

// ----------------------------------------------------------------------------------------------
// voxel_count_views (dvgo.py:250-276): per image, the trilinear footprint of every sample of every ray is added into a zero grid
// and a voxel counts as seen where it gathered more than 1.  The reference gets the footprint from the backward of a lookup on
// materialised points ([10000, n_samples, 3] per chunk, an autograd backward per chunk); here one lane walks one ray and adds the
// corner weights itself -- the point as that path forms it, o + d * (t_min + (stepdist * j) / |d|), the taps of the lookup's own
// backward (ug_unorm + ug_tap_setup, gradient 1), the same hardware atomics: the same sums in another order.
//   k_count_views_accumulate   one image's rays -> acc += footprint
//   k_count_views_commit       count += acc > 1; acc = 0 (ready for the next image)
// A ray stops where no later sample can reach the grid: zero padding gives a point up to ONE cell outside the box a weight on the
// face vertices, a point is monotone in j on every axis, so two cells beyond a face it is leaving (or not moving towards) is final.
// ----------------------------------------------------------------------------------------------
__global__ void k_count_views_accumulate(const float *__restrict__ rays_o, const float *__restrict__ rays_d, int64_t n_rays,
                                         const float *__restrict__ xyz_min, const float *__restrict__ xyz_max, float near, float far,
                                         float stepdist, int32_t n_samples, int X, int Y, int Z, float *__restrict__ acc) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rays) return;
  const float lo[3] = {xyz_min[0], xyz_min[1], xyz_min[2]}, hi[3] = {xyz_max[0], xyz_max[1], xyz_max[2]};
  const float o[3] = {rays_o[3 * r], rays_o[3 * r + 1], rays_o[3 * r + 2]}, d[3] = {rays_d[3 * r], rays_d[3 * r + 1], rays_d[3 * r + 2]};
  const float t_min = ug_t_minmax(o, d, lo, hi, near, far).tmin;
  const float rn = ug_norm3(d);
  const int dims[3] = {X, Y, Z};
  float below[3], above[3];                 // beyond these a point's eight corners are all outside the grid (two cells: one of slack)
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float two = 2.f * (hi[c] - lo[c]) / (float)(dims[c] - 1);
    below[c] = lo[c] - two;
    above[c] = hi[c] + two;
  }
  for (int32_t j = 0; j < n_samples; ++j) {
    const float t = t_min + (stepdist * (float)j) / rn;
    float p[3];
    bool gone = false;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      p[c] = o[c] + d[c] * t;
      gone |= (p[c] < below[c] && d[c] <= 0.f) || (p[c] > above[c] && d[c] >= 0.f);
    }
    if (gone) break;
    const ug_taps tp = ug_tap_setup(X, Y, Z, ug_unorm(p[0], lo[0], hi[0]), ug_unorm(p[1], lo[1], hi[1]), ug_unorm(p[2], lo[2], hi[2]));
#pragma unroll
    for (int c = 0; c < 8; ++c)
      if (tp.off[c] >= 0 && tp.w[c] != 0.f) unsafeAtomicAdd(acc + tp.off[c], tp.w[c]);      // (adding an exact zero changes nothing)
  }
}

__global__ void k_count_views_commit(float *__restrict__ acc, float *__restrict__ count, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    count[i] += acc[i] > 1.f ? 1.f : 0.f;
    acc[i] = 0.f;
  }
}

// ----------------------------------------------------------------------------------------------
// C ABI
// ----------------------------------------------------------------------------------------------
static int ug_grid_query_any(bool cl, const float *grid, int P, int C, int X, int Y, int Z, const float *xyz,
                             const float *xyz_min, const float *xyz_max, int freq_num, int64_t n, float *out, hipStream_t st) {
  if (n <= 0) return 0;
  if (P != (freq_num > 0 ? 2 * freq_num + 1 : 1)) return (int)hipErrorInvalidValue;
  const int64_t nl = ug_launch_rows(n);          // (a device count in force: the grid follows the hint, the kernel the count)
  if (cl)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_grid_query<true>), dim3(ug_blocks(nl * C, 256)), dim3(256), 0, st, grid, P, C, X, Y, Z, xyz,
                       xyz_min, xyz_max, freq_num, n, out, ug_tl_devn.ptr);
  else
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_grid_query<false>), dim3(ug_blocks(nl, 256)), dim3(256), 0, st, grid, P, C, X, Y, Z, xyz,
                       xyz_min, xyz_max, freq_num, n, out, ug_tl_devn.ptr);
  UG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ugrid_grid_query(const float *grid, int P, int C, int X, int Y, int Z, const float *xyz,
                                const float *xyz_min, const float *xyz_max, int freq_num, int64_t n,
                                float *out, ugrid_stream_t s) {
  return ug_grid_query_any(false, grid, P, C, X, Y, Z, xyz, xyz_min, xyz_max, freq_num, n, out, ST(s));
}

extern "C" int ugrid_grid_query_cl(const float *grid, int P, int C, int X, int Y, int Z, const float *xyz,
                                   const float *xyz_min, const float *xyz_max, int freq_num, int64_t n,
                                   float *out, ugrid_stream_t s) {
  return ug_grid_query_any(true, grid, P, C, X, Y, Z, xyz, xyz_min, xyz_max, freq_num, n, out, ST(s));
}

static int ug_grid_query_backward_any(bool cl, const float *grad_out, int P, int C, int X, int Y, int Z, const float *xyz,
                                      const float *xyz_min, const float *xyz_max, int freq_num, int64_t n,
                                      float *grad_grid, hipStream_t st, uint32_t *touch = nullptr) {
  if (n <= 0) return 0;
  if (P != (freq_num > 0 ? 2 * freq_num + 1 : 1)) return (int)hipErrorInvalidValue;
  const int64_t nl = ug_launch_rows(n);
  if (cl)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_grid_query_backward<true>), dim3(ug_blocks(nl * P * C, 256)), dim3(256), 0, st, grad_out, P, C,
                       X, Y, Z, xyz, xyz_min, xyz_max, freq_num, n, grad_grid, touch, ug_tl_devn.ptr);
  else
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_grid_query_backward<false>), dim3(ug_blocks(nl * P, 256)), dim3(256), 0, st, grad_out, P, C,
                       X, Y, Z, xyz, xyz_min, xyz_max, freq_num, n, grad_grid, (uint32_t *)nullptr, ug_tl_devn.ptr);
  UG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ugrid_grid_query_backward(const float *grad_out, int P, int C, int X, int Y, int Z, const float *xyz,
                                         const float *xyz_min, const float *xyz_max, int freq_num, int64_t n,
                                         float *grad_grid, ugrid_stream_t s) {
  return ug_grid_query_backward_any(false, grad_out, P, C, X, Y, Z, xyz, xyz_min, xyz_max, freq_num, n, grad_grid, ST(s));
}

extern "C" int ugrid_grid_query_backward_cl(const float *grad_out, int P, int C, int X, int Y, int Z, const float *xyz,
                                            const float *xyz_min, const float *xyz_max, int freq_num, int64_t n,
                                            float *grad_grid, ugrid_stream_t s) {
  return ug_grid_query_backward_any(true, grad_out, P, C, X, Y, Z, xyz, xyz_min, xyz_max, freq_num, n, grad_grid, ST(s));
}

extern "C" int ugrid_grid_query_backward_cl_touch(const float *grad_out, int P, int C, int X, int Y, int Z, const float *xyz,
                                                  const float *xyz_min, const float *xyz_max, int freq_num, int64_t n,
                                                  float *grad_grid, uint32_t *touch, ugrid_stream_t s) {
  return ug_grid_query_backward_any(true, grad_out, P, C, X, Y, Z, xyz, xyz_min, xyz_max, freq_num, n, grad_grid, ST(s), touch);
}

extern "C" int ugrid_count_views_accumulate(const float *rays_o, const float *rays_d, int64_t n_rays, const float *xyz_min,
                                            const float *xyz_max, float near, float far, float stepdist, int32_t n_samples, int X, int Y,
                                            int Z, float *acc, ugrid_stream_t s) {
  if (n_rays <= 0 || n_samples <= 0) return 0;
  if (!rays_o || !rays_d || !xyz_min || !xyz_max || !acc || X < 1 || Y < 1 || Z < 1) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_count_views_accumulate, dim3(ug_blocks(n_rays, 64)), dim3(64), 0, ST(s), rays_o, rays_d, n_rays, xyz_min, xyz_max,
                     near, far, stepdist, n_samples, X, Y, Z, acc);
  UG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ugrid_count_views_commit(float *acc, float *count, int64_t n, ugrid_stream_t s) {
  if (n <= 0) return 0;
  if (!acc || !count) return (int)hipErrorInvalidValue;
  const int64_t blocks = ug_blocks(n, 256);
  hipLaunchKernelGGL(k_count_views_commit, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, ST(s), acc, count, n);
  UG_LAUNCH_CHECK();
  return 0;
}
