// libugrid_hip.so -- drop-in kernels behind the reference's extension modules render_utils_cuda
// and ub360_utils_cuda (total_variation_cuda and adam_upd_cuda: ugrid_update.hip), written for
// gfx950 (MI355X): 64-lane waves, one wave per ray for the scans.  fp32 arithmetic follows the
// reference expression trees (compiled with -ffp-contract=off) so results are bit-identical to
// oracle/ref_ops.c except where libm transcendentals (exp/pow) are involved.
//
// Reference behaviour restated (never copied): FourierGrid/cuda/render_utils_kernel.cu,
// ub360_utils_kernel.cu -- per-function file:line citations are in include/ugrid_hip.h.
#include "ugrid_common.h"
#include "ugrid_rays.h"

extern "C" int ugrid_abi_version(void) { return 3; }  // 2: ugrid_render_params.mlp_mode, ugrid_pack_mlp(k0_absmax, best_mode); 3: ugrid_frame_metrics
extern "C" const char *ugrid_target_arch(void) { return "gfx950"; }

// Ray / AABB helpers (ug_t_minmax, ug_norm3, ug_n_samples, ug_sample_point, ug_mask_index): ugrid_rays.h

__global__ void k_infer_t_minmax(const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                                 const float *__restrict__ xyz_min, const float *__restrict__ xyz_max,
                                 float near, float far, int64_t n_rays, float *__restrict__ t_min,
                                 float *__restrict__ t_max) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rays) return;
  const float lo[3] = {xyz_min[0], xyz_min[1], xyz_min[2]}, hi[3] = {xyz_max[0], xyz_max[1], xyz_max[2]};
  const ug_tmm t = ug_t_minmax(rays_o + 3 * r, rays_d + 3 * r, lo, hi, near, far);
  t_min[r] = t.tmin;
  t_max[r] = t.tmax;
}

__global__ void k_infer_n_samples(const float *__restrict__ rays_d, const float *__restrict__ t_min,
                                  const float *__restrict__ t_max, float stepdist, int64_t n_rays,
                                  int64_t *__restrict__ n_samples) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rays) return;
  n_samples[r] = ug_n_samples(rays_d + 3 * r, t_min[r], t_max[r], stepdist);
}

__global__ void k_infer_ray_start_dir(const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                                      const float *__restrict__ t_min, int64_t n_rays,
                                      float *__restrict__ rays_start, float *__restrict__ rays_dir) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rays) return;
  const float *o = rays_o + 3 * r, *d = rays_d + 3 * r;
  const float rn = ug_norm3(d), tm = t_min[r];
  for (int c = 0; c < 3; ++c) {
    rays_start[3 * r + c] = o[c] + d[c] * tm;
    rays_dir[3 * r + c] = d[c] / rn;
  }
}

// fused first half of sample_pts_on_rays: t_min, t_max, N_steps in one pass over the rays
__global__ void k_sample_count(const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                               const float *__restrict__ xyz_min, const float *__restrict__ xyz_max,
                               float near, float far, float stepdist, int64_t n_rays,
                               float *__restrict__ t_min, float *__restrict__ t_max,
                               int64_t *__restrict__ n_steps) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rays) return;
  const float lo[3] = {xyz_min[0], xyz_min[1], xyz_min[2]}, hi[3] = {xyz_max[0], xyz_max[1], xyz_max[2]};
  const ug_tmm t = ug_t_minmax(rays_o + 3 * r, rays_d + 3 * r, lo, hi, near, far);
  t_min[r] = t.tmin;
  t_max[r] = t.tmax;
  n_steps[r] = ug_n_samples(rays_d + 3 * r, t.tmin, t.tmax, stepdist);
}

// ----------------------------------------------------------------------------------------------
// int64 inclusive scan (three short kernels; the ray counts involved are <= a few million)
// ----------------------------------------------------------------------------------------------
#define UG_SCAN_THREADS 256
#define UG_SCAN_ITEMS 4
#define UG_SCAN_TILE (UG_SCAN_THREADS * UG_SCAN_ITEMS)

__device__ __forceinline__ int64_t ug_block_exclusive_scan(int64_t v, int64_t *lds, int64_t *block_total) {
  // Hillis-Steele over 256 per-thread sums held in LDS
  const int t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
  for (int off = 1; off < UG_SCAN_THREADS; off <<= 1) {
    const int64_t add = (t >= off) ? lds[t - off] : 0;
    __syncthreads();
    lds[t] += add;
    __syncthreads();
  }
  *block_total = lds[UG_SCAN_THREADS - 1];
  return lds[t] - v;
}

__global__ void __launch_bounds__(UG_SCAN_THREADS)
k_scan_local(const int64_t *__restrict__ in, int64_t n, int64_t *__restrict__ out,
             int64_t *__restrict__ block_sums) {
  __shared__ int64_t lds[UG_SCAN_THREADS];
  const int64_t base = (int64_t)blockIdx.x * UG_SCAN_TILE + (int64_t)threadIdx.x * UG_SCAN_ITEMS;
  int64_t v[UG_SCAN_ITEMS], s = 0;
  for (int i = 0; i < UG_SCAN_ITEMS; ++i) {
    v[i] = (base + i < n) ? in[base + i] : 0;
    s += v[i];
  }
  int64_t total;
  int64_t run = ug_block_exclusive_scan(s, lds, &total);
  for (int i = 0; i < UG_SCAN_ITEMS; ++i) {
    run += v[i];
    if (base + i < n) out[base + i] = run;
  }
  if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

__global__ void __launch_bounds__(UG_SCAN_THREADS)
k_scan_block_sums(int64_t *__restrict__ block_sums, int64_t n_blocks, int64_t *__restrict__ total_out) {
  __shared__ int64_t lds[UG_SCAN_THREADS];
  int64_t carry = 0;
  for (int64_t base = 0; base < n_blocks; base += UG_SCAN_THREADS) {
    const int64_t i = base + threadIdx.x;
    const int64_t v = (i < n_blocks) ? block_sums[i] : 0;
    int64_t total;
    const int64_t ex = ug_block_exclusive_scan(v, lds, &total);
    if (i < n_blocks) block_sums[i] = carry + ex;
    carry += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) *total_out = carry;
}

__global__ void k_scan_add(int64_t *__restrict__ out, int64_t n, const int64_t *__restrict__ block_sums) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] += block_sums[i / UG_SCAN_TILE];
}

extern "C" int64_t ugrid_scan_ws_bytes(int64_t n) {
  return (int64_t)sizeof(int64_t) * ((n + UG_SCAN_TILE - 1) / UG_SCAN_TILE + 1);
}

static int ug_inclusive_scan(const int64_t *in, int64_t n, int64_t *out, int64_t *d_total, void *ws,
                             hipStream_t st) {
  if (n == 0) return (int)hipMemsetAsync(d_total, 0, sizeof(int64_t), st);
  const int64_t nb = (n + UG_SCAN_TILE - 1) / UG_SCAN_TILE;
  int64_t *bs = (int64_t *)ws;
  hipLaunchKernelGGL(k_scan_local, dim3((unsigned)nb), dim3(UG_SCAN_THREADS), 0, st, in, n, out, bs);
  hipLaunchKernelGGL(k_scan_block_sums, dim3(1), dim3(UG_SCAN_THREADS), 0, st, bs, nb, d_total);
  hipLaunchKernelGGL(k_scan_add, dim3(ug_blocks(n, 256)), dim3(256), 0, st, out, n, bs);
  UG_LAUNCH_CHECK();
  return 0;
}

// second half of sample_pts_on_rays: 1 lane per sample, owner ray by binary search in the
// inclusive prefix sum (replaces the reference's "1 at segment start + cumsum" construction).
__global__ void k_sample_fill(const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                              const float *__restrict__ xyz_min, const float *__restrict__ xyz_max,
                              const float *__restrict__ t_min, const int64_t *__restrict__ cumsum,
                              float stepdist, int64_t n_rays, int64_t total,
                              float *__restrict__ rays_pts, uint8_t *__restrict__ mask_outbbox,
                              int64_t *__restrict__ ray_id, int64_t *__restrict__ step_id) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  int64_t lo = 0, hi = n_rays - 1;  // first r with cumsum[r] > idx
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (cumsum[mid] > idx) hi = mid; else lo = mid + 1;
  }
  const int64_t r = lo;
  const int64_t s = idx - (r ? cumsum[r - 1] : 0);
  const float lo_[3] = {xyz_min[0], xyz_min[1], xyz_min[2]}, hi_[3] = {xyz_max[0], xyz_max[1], xyz_max[2]};
  float p[3];
  const bool out = ug_sample_point(rays_o + 3 * r, rays_d + 3 * r, ug_norm3(rays_d + 3 * r), t_min[r], stepdist, (int)s, lo_, hi_, p);
  for (int c = 0; c < 3; ++c) rays_pts[3 * idx + c] = p[c];
  mask_outbbox[idx] = (uint8_t)out;
  ray_id[idx] = r;
  step_id[idx] = s;
}

__global__ void k_sample_ndc(const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                             const float *__restrict__ xyz_min, const float *__restrict__ xyz_max,
                             int n_samples, int64_t total, float *__restrict__ rays_pts,
                             uint8_t *__restrict__ mask_outbbox) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int64_t r = idx / n_samples;
  const int s = (int)(idx - r * n_samples);
  const float dist = ((float)s) / (float)(n_samples - 1);
  float p[3];
  for (int c = 0; c < 3; ++c) {
    p[c] = rays_o[3 * r + c] + rays_d[3 * r + c] * dist;
    rays_pts[3 * idx + c] = p[c];
  }
  mask_outbbox[idx] = (uint8_t)((xyz_min[0] > p[0]) | (xyz_min[1] > p[1]) | (xyz_min[2] > p[2]) |
                                (xyz_max[0] < p[0]) | (xyz_max[1] < p[1]) | (xyz_max[2] < p[2]));
}

__global__ void k_sample_bg(const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                            const float *__restrict__ t_max, float bg_preserve, int n_samples,
                            int64_t total, float *__restrict__ rays_pts) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int64_t r = idx / n_samples;
  const int s = (int)(idx - r * n_samples);
  const float frac = ((float)s) / (float)n_samples;
  const float t_out = (float)((double)t_max[r] - 1. + 1. / (1. - (double)frac));
  const float x = rays_o[3 * r] + rays_d[3 * r] * t_out;
  const float y = rays_o[3 * r + 1] + rays_d[3 * r + 1] * t_out;
  const float z = rays_o[3 * r + 2] + rays_d[3 * r + 2] * t_out;
  const float tn = sqrtf(x * x + y * y + z * z);
  const float m = fmaxf(fabsf(x), fmaxf(fabsf(y), fabsf(z)));
  const float Ro = tn / m;
  const float q = (float)((double)(Ro * Ro / (tn * tn)) * (1. - (double)bg_preserve) +
                          (double)(Ro / tn * bg_preserve));
  rays_pts[3 * idx] = x * q;
  rays_pts[3 * idx + 1] = y * q;
  rays_pts[3 * idx + 2] = z * q;
}

__global__ void k_maskcache(const uint8_t *__restrict__ world, const float *__restrict__ xyz,
                            const float *__restrict__ scale, const float *__restrict__ shift,
                            int64_t sz_i, int64_t sz_j, int64_t sz_k, int64_t n,
                            uint8_t *__restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const int64_t at = ug_mask_index(xyz + 3 * p, scale, shift, sz_i, sz_j, sz_k);      // (-1: outside the mask grid)
  out[p] = at >= 0 ? world[at] : (uint8_t)0;
}

// hit_coarse_geo (dvgo.py:291-304) as ONE kernel, 1 lane per ray: the reference composes sample_pts_on_rays (points + ids of every
// sample of every ray: 29 B per sample and a host read of the total), a boolean index, maskcache_lookup and a scatter.  Here a ray
// walks its own samples -- the same t_min / step count / point / out-of-box test / mask voxel, through the same device functions as
// k_sample_count, k_sample_fill and k_maskcache -- and stops at the first occupied cell: the same bits, no sample ever stored.
__global__ void k_hit_coarse_geo(const float *__restrict__ rays_o, const float *__restrict__ rays_d, int64_t n_rays,
                                 const float *__restrict__ xyz_min, const float *__restrict__ xyz_max, float near, float far,
                                 float stepdist, const uint8_t *__restrict__ world, int64_t sz_i, int64_t sz_j, int64_t sz_k,
                                 const float *__restrict__ scale, const float *__restrict__ shift, uint8_t *__restrict__ hit) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rays) return;
  const float lo[3] = {xyz_min[0], xyz_min[1], xyz_min[2]}, hi[3] = {xyz_max[0], xyz_max[1], xyz_max[2]};
  const float sc[3] = {scale[0], scale[1], scale[2]}, sh[3] = {shift[0], shift[1], shift[2]};
  const float o[3] = {rays_o[3 * r], rays_o[3 * r + 1], rays_o[3 * r + 2]}, d[3] = {rays_d[3 * r], rays_d[3 * r + 1], rays_d[3 * r + 2]};
  const ug_tmm t = ug_t_minmax(o, d, lo, hi, near, far);
  int64_t n = ug_n_samples(d, t.tmin, t.tmax, stepdist);
  // a finite ray's samples span at most the box diagonal (t_min .. t_max lie on the box): like the sampling march's slots, a bound that
  // never binds on them -- it keeps a ray of non-finite numbers, whose count saturates, from walking forever
  const float ext[3] = {hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]};
  const float diag_steps = ceilf(ug_norm3(ext) / stepdist);
  const int64_t cap = (diag_steps < 2e9f ? (int64_t)diag_steps : 0) + 3;      // (a box that is not finite either: three samples)
  if (!(n <= cap)) n = cap;
  const float rn = ug_norm3(d);
  uint8_t h = 0;
  for (int64_t s = 0; s < n; ++s) {
    float p[3];
    if (ug_sample_point(o, d, rn, t.tmin, stepdist, (int)s, lo, hi, p)) continue;
    const int64_t at = ug_mask_index(p, sc, sh, sz_i, sz_j, sz_k);
    if (at >= 0 && world[at]) { h = 1; break; }
  }
  hit[r] = h;
}

// ----------------------------------------------------------------------------------------------
// raw -> alpha  (12 B/point stream)
// ----------------------------------------------------------------------------------------------
__global__ void k_raw2alpha(const float *__restrict__ density, float shift, float interval,
                            const float *__restrict__ interval_arr, int64_t n,
                            float *__restrict__ exp_d, float *__restrict__ alpha) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float itv = interval_arr ? interval_arr[i] : interval;
  const float e = expf(density[i] + shift);
  exp_d[i] = e;
  alpha[i] = 1 - powf(1 + e, -itv);
}

__global__ void k_raw2alpha_bwd(const float *__restrict__ exp_d, const float *__restrict__ grad_back,
                                float interval, const float *__restrict__ interval_arr, int64_t n,
                                float *__restrict__ grad) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float itv = interval_arr ? interval_arr[i] : interval;
  const float ef = exp_d[i];
  const double e = (double)ef;
  const double em = e < 1e10 ? e : 1e10;
  const float pw = powf(1 + ef, -itv - 1);
  grad[i] = (float)(em * (double)pw * (double)itv * (double)grad_back[i]);
}

// ----------------------------------------------------------------------------------------------
// alpha -> weights: one 64-lane wave per ray.  Samples are loaded 64 at a time (coalesced); the
// transmittance recurrence T <- float(double(T) * (1 - double(alpha))) is evaluated in sample order
// on a wave-uniform value (every lane runs the same chain, lane k keeps step k's T), so rounding is
// identical to the reference's serial scan while loads/stores stay coalesced.  The wave stops the
// chain as soon as T < 1e-3 and only streams default values (w=0, T=1) over the rest of the ray.
// ----------------------------------------------------------------------------------------------
__global__ void k_segments(const int64_t *__restrict__ ray_id, int64_t n, int64_t *__restrict__ i_start,
                           int64_t *__restrict__ i_end) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t r = ray_id[i];
  if (i > 0) {
    const int64_t rp = ray_id[i - 1];
    if (r != rp) {
      i_start[r] = i;
      i_end[rp] = i;
    }
  }
  if (i == n - 1) i_end[r] = n;
}

__global__ void __launch_bounds__(256)
k_alpha2weight(const float *__restrict__ alpha, int64_t n_rays, float *__restrict__ weight,
               float *__restrict__ T, float *__restrict__ alphainv_last,
               const int64_t *__restrict__ i_start, int64_t *__restrict__ i_end) {
  const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (r >= n_rays) return;
  const int lane = ug_lane();
  const int64_t i_s = i_start[r], i_e = i_end[r];
  float T_cum = 1.f;
  bool stopped = false;
  int64_t stop_at = i_e;
  for (int64_t base = i_s; base < i_e; base += UG_WAVE) {
    const int64_t i = base + lane;
    const int cnt = (int)((i_e - base) < UG_WAVE ? (i_e - base) : UG_WAVE);
    float myT = 1.f, myW = 0.f;
    if (!stopped) {
      const float a = (i < i_e) ? alpha[i] : 0.f;
      const double om = 1. - (double)a;
      for (int k = 0; k < cnt; ++k) {
        const float ak = ug_readlane_f(a, k);
        const double omk = ug_readlane_d(om, k);
        if (lane == k) {
          myT = T_cum;
          myW = T_cum * ak;
        }
        T_cum = (float)((double)T_cum * omk);
        if ((double)T_cum < 1e-3) {
          stopped = true;
          stop_at = base + k + 1;
          break;
        }
      }
      if (stopped && i >= stop_at) {
        myT = 1.f;
        myW = 0.f;
      }
    }
    if (i < i_e) {
      T[i] = myT;
      weight[i] = myW;
    }
  }
  if (lane == 0) {
    i_end[r] = stop_at;
    alphainv_last[r] = T_cum;
  }
}

// reverse pass: back_cum is a float running sum taken from the LAST kept sample backwards, so the
// chain again runs in order on a wave-uniform value; the per-sample double expression is lane-parallel.
__global__ void __launch_bounds__(256)
k_alpha2weight_bwd(const float *__restrict__ alpha, const float *__restrict__ weight,
                   const float *__restrict__ T, const float *__restrict__ alphainv_last,
                   const int64_t *__restrict__ i_start, const int64_t *__restrict__ i_end,
                   int64_t n_rays, const float *__restrict__ grad_weights,
                   const float *__restrict__ grad_last, float *__restrict__ grad) {
  const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (r >= n_rays) return;
  const int lane = ug_lane();
  const int64_t i_s = i_start[r], i_e = i_end[r];
  float back = grad_last[r] * alphainv_last[r];
  for (int64_t top = i_e; top > i_s; top -= UG_WAVE) {
    // lane k holds sample top-1-k (reverse order inside the chunk)
    const int64_t i = top - 1 - lane;
    const bool ok = i >= i_s;
    const float gw = ok ? grad_weights[i] : 0.f;
    const float prod = ok ? gw * weight[i] : 0.f;
    const int cnt = (int)((top - i_s) < UG_WAVE ? (top - i_s) : UG_WAVE);
    float my_back = 0.f;
    for (int k = 0; k < cnt; ++k) {
      if (lane == k) my_back = back;
      back += ug_readlane_f(prod, k);
    }
    if (ok) {
      const float a = alpha[i];
      grad[i] = (float)((double)(gw * T[i]) - (double)my_back / ((double)(1 - a) + 1e-10));
    }
  }
}

// ----------------------------------------------------------------------------------------------
// cumdist_thres: one wave per ray, 64 distances per coalesced load, serial float chain as above
// ----------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_cumdist(const float *__restrict__ dist, float thres, int64_t n_rays, int64_t n_pts,
          uint8_t *__restrict__ mask) {
  const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (r >= n_rays) return;
  const int lane = ug_lane();
  float cum = 0.f;
  for (int64_t base = 0; base < n_pts; base += UG_WAVE) {
    const int64_t i = base + lane;
    const float d = (i < n_pts) ? dist[r * n_pts + i] : 0.f;
    const int cnt = (int)((n_pts - base) < UG_WAVE ? (n_pts - base) : UG_WAVE);
    bool my_over = false;
    for (int k = 0; k < cnt; ++k) {
      cum += ug_readlane_f(d, k);
      const bool over = cum > thres;
      if (lane == k) my_over = over;
      cum *= over ? 0.f : 1.f;
    }
    if (i < n_pts) mask[r * n_pts + i] = (uint8_t)my_over;
  }
}

// ----------------------------------------------------------------------------------------------
// segment_cumsum (called by the reference's DistortionLoss, FourierGrid_model.py:684-708, never shipped by its
// ub360_utils.cpp): exclusive running sums of w and w*s inside each ray segment + per-ray totals.  One wave per
// ray, 64 samples per coalesced load, the two fp32 chains run in sample order on wave-uniform values.
// ----------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_segment_cumsum(const float *__restrict__ w, const float *__restrict__ s, int64_t n_rays,
                 const int64_t *__restrict__ i_start, const int64_t *__restrict__ i_end,
                 float *__restrict__ w_prefix, float *__restrict__ w_total, float *__restrict__ ws_prefix,
                 float *__restrict__ ws_total) {
  const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (r >= n_rays) return;
  const int lane = ug_lane();
  const int64_t i_s = i_start[r], i_e = i_end[r];
  float cw = 0.f, cws = 0.f;
  for (int64_t base = i_s; base < i_e; base += UG_WAVE) {
    const int64_t i = base + lane;
    const float wi = (i < i_e) ? w[i] : 0.f;
    const float wsi = (i < i_e) ? wi * s[i] : 0.f;
    const int cnt = (int)((i_e - base) < UG_WAVE ? (i_e - base) : UG_WAVE);
    float my_w = 0.f, my_ws = 0.f;
    for (int k = 0; k < cnt; ++k) {
      if (lane == k) { my_w = cw; my_ws = cws; }
      cw = cw + ug_readlane_f(wi, k);
      cws = cws + ug_readlane_f(wsi, k);
    }
    if (i < i_e) { w_prefix[i] = my_w; ws_prefix[i] = my_ws; }
  }
  if (lane == 0) { w_total[r] = cw; ws_total[r] = cws; }
}

// ----------------------------------------------------------------------------------------------
// get_rays_of_a_view (dvgo.py:493-521,554-559) as ONE kernel: pixel-centre pinhole rays,
// rays_d = dirs . c2w[:3,:3]^T, viewdirs = rays_d / |rays_d|, rays_o = c2w[:,3]; the torch chain it replaces is ~15
// launches per frame.  Operation order of the reference's elementwise chain (products, then ((p0 + p1) + p2); the norm as
// the fma chain of torch's vector_norm).  pix == nullptr: all H*W pixels in image order; else the listed flat indices.
// ----------------------------------------------------------------------------------------------
struct ug_cam { float fx, fy, cx, cy; int W, H, inverse_y, flip_x, flip_y, center; };

// world-space direction of flat pixel p (get_rays, dvgo.py:493-521)
__device__ __forceinline__ void ug_view_ray_dir(const ug_cam &c, const float *__restrict__ c2w, int64_t p, float (&r)[3]) {
  int j = (int)(p / c.W), i = (int)(p - (int64_t)j * c.W);
  if (c.flip_x) i = c.W - 1 - i;
  if (c.flip_y) j = c.H - 1 - j;
  float ii = (float)i, jj = (float)j;
  if (c.center) { ii = ii + 0.5f; jj = jj + 0.5f; }
  float dx, dy, dz;
  if (c.inverse_y) { dx = (ii - c.cx) / c.fx; dy = (jj - c.cy) / c.fy; dz = 1.0f; }
  else { dx = (ii - c.cx) / c.fx; dy = -(jj - c.cy) / c.fy; dz = -1.0f; }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float p0 = dx * c2w[4 * a], p1 = dy * c2w[4 * a + 1], p2 = dz * c2w[4 * a + 2];
    r[a] = (p0 + p1) + p2;
  }
}

// one ray of a view: o = c2w[:,3], d = the world direction of flat pixel p, v = d / |d|  (the per-ray body that
// k_rays_of_a_view and k_ray_batch share)
__device__ __forceinline__ void ug_view_ray(const ug_cam &c, const float *__restrict__ c2w, int64_t p, float (&o)[3], float (&d)[3],
                                            float (&v)[3]) {
  ug_view_ray_dir(c, c2w, p, d);
  const float nrm = sqrtf(fmaf(d[2], d[2], fmaf(d[1], d[1], d[0] * d[0])));
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    o[a] = c2w[4 * a + 3];
    v[a] = d[a] / nrm;
  }
}

__device__ __forceinline__ void ug_store3(float *__restrict__ dst, int64_t t, const float (&x)[3]) {
  dst[3 * t] = x[0];
  dst[3 * t + 1] = x[1];
  dst[3 * t + 2] = x[2];
}

__global__ void k_rays_of_a_view(ug_cam c, const float *__restrict__ c2w, const int64_t *__restrict__ pix, int64_t n,
                                 float *__restrict__ rays_o, float *__restrict__ rays_d, float *__restrict__ viewdirs) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  float o[3], d[3], v[3];
  ug_view_ray(c, c2w, pix ? pix[t] : t, o, d, v);
  ug_store3(rays_o, t, o);
  ug_store3(rays_d, t, d);
  ug_store3(viewdirs, t, v);
}

// get_rays_of_a_view(ndc=True) (dvgo.py:534-559): viewdirs from the WORLD direction, then ndc_rays(H, W, K[0][0], near, o, d)
// in the order of its torch chain: t = -(o_z + near) / d_z; o' = o + t * d; 2 * near / o'_z as reciprocal(o'_z) * (2 near)
// (Tensor.__rtruediv__); the Python constants -1 / (W / (2 focal)) etc. are formed in double on the host and rounded to fp32.
struct ug_ndc { float near, kx, ky, two_near, mtwo_near; };

// the NDC ray of flat pixel p (the per-ray body that k_rays_of_a_view_ndc and k_ray_batch share)
__device__ __forceinline__ void ug_view_ray_ndc(const ug_cam &c, const ug_ndc &q, const float *__restrict__ c2w, int64_t p,
                                                float (&o)[3], float (&d)[3], float (&v)[3]) {
  float r[3];
  ug_view_ray_dir(c, c2w, p, r);
  const float nrm = sqrtf(fmaf(r[2], r[2], fmaf(r[1], r[1], r[0] * r[0])));
#pragma unroll
  for (int a = 0; a < 3; ++a) v[a] = r[a] / nrm;
  const float wx = c2w[3], wy = c2w[7], wz = c2w[11];
  const float tt = -(wz + q.near) / r[2];
  const float ox = wx + tt * r[0], oy = wy + tt * r[1], oz = wz + tt * r[2];
  const float rz = 1.0f / oz;
  o[0] = q.kx * ox / oz;
  o[1] = q.ky * oy / oz;
  o[2] = 1.0f + rz * q.two_near;
  d[0] = q.kx * (r[0] / r[2] - ox / oz);
  d[1] = q.ky * (r[1] / r[2] - oy / oz);
  d[2] = rz * q.mtwo_near;
}

__global__ void k_rays_of_a_view_ndc(ug_cam c, ug_ndc q, const float *__restrict__ c2w, const int64_t *__restrict__ pix, int64_t n,
                                     float *__restrict__ rays_o, float *__restrict__ rays_d, float *__restrict__ viewdirs) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  float o[3], d[3], v[3];
  ug_view_ray_ndc(c, q, c2w, pix ? pix[t] : t, o, d, v);
  ug_store3(rays_o, t, o);
  ug_store3(rays_d, t, d);
  ug_store3(viewdirs, t, v);
}

// One iteration's ray batch from the pose table (train_rays.RayBatcher): a lane per batch row.  The row's global pixel index
// -> its view by binary search over the prefix of pixel counts (the LAST view whose start is <= the index, so that views
// without pixels are stepped over) -> the view's record -> the shared per-ray leaf; the colour comes from the flattened image
// store, float32 or 8-bit ((float)((double)u / 255.0): the value of the loaders' (img / 255.).astype(np.float32)).
// indexs (nullable): the view number as float in all three columns, like the reference's indexs_tr.
__global__ void k_ray_batch(const ugrid_ray_cam *__restrict__ cams, const int64_t *__restrict__ view_start, int n_views,
                            const int64_t *__restrict__ index, int64_t n, const void *__restrict__ images, int image_kind,
                            int inverse_y, int flip_x, int flip_y, int center, int ndc, float near, float two_near, float mtwo_near,
                            float *__restrict__ target, float *__restrict__ rays_o, float *__restrict__ rays_d,
                            float *__restrict__ viewdirs, float *__restrict__ indexs) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int64_t g = index[t];
  int lo = 0, hi = n_views;             // view_start[lo] <= g < view_start[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (view_start[mid] <= g) lo = mid; else hi = mid;
  }
  const ugrid_ray_cam *__restrict__ rec = cams + lo;
  ug_cam c;
  c.fx = rec->fx; c.fy = rec->fy; c.cx = rec->cx; c.cy = rec->cy;
  c.W = rec->W; c.H = rec->H; c.inverse_y = inverse_y; c.flip_x = flip_x; c.flip_y = flip_y; c.center = center;
  const int64_t p = g - view_start[lo];
  float o[3], d[3], v[3];
  if (ndc) {
    ug_ndc q;
    q.near = near; q.kx = rec->kx; q.ky = rec->ky; q.two_near = two_near; q.mtwo_near = mtwo_near;
    ug_view_ray_ndc(c, q, rec->c2w, p, o, d, v);
  } else {
    ug_view_ray(c, rec->c2w, p, o, d, v);
  }
  float rgb[3];
  if (image_kind == 1) {
    const uint8_t *__restrict__ im = (const uint8_t *)images + 3 * g;
#pragma unroll
    for (int a = 0; a < 3; ++a) rgb[a] = (float)((double)im[a] / 255.0);
  } else {
    const float *__restrict__ im = (const float *)images + 3 * g;
#pragma unroll
    for (int a = 0; a < 3; ++a) rgb[a] = im[a];
  }
  ug_store3(target, t, rgb);
  ug_store3(rays_o, t, o);
  ug_store3(rays_d, t, d);
  ug_store3(viewdirs, t, v);
  if (indexs) {
    const float f = (float)lo;
    const float fi[3] = {f, f, f};
    ug_store3(indexs, t, fi);
  }
}

// ----------------------------------------------------------------------------------------------
// C ABI
// ----------------------------------------------------------------------------------------------
#define ST(s) ((hipStream_t)(s))

extern "C" int ugrid_infer_t_minmax(const float *rays_o, const float *rays_d, const float *xyz_min,
                                    const float *xyz_max, float near, float far, int64_t n_rays,
                                    float *t_min, float *t_max, ugrid_stream_t s) {
  if (n_rays <= 0) return 0;
  hipLaunchKernelGGL(k_infer_t_minmax, dim3(ug_blocks(n_rays, 256)), dim3(256), 0, ST(s), rays_o, rays_d,
                     xyz_min, xyz_max, near, far, n_rays, t_min, t_max);
  UG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ugrid_infer_n_samples(const float *rays_d, const float *t_min, const float *t_max,
                                     float stepdist, int64_t n_rays, int64_t *n_samples, ugrid_stream_t s) {
  if (n_rays <= 0) return 0;
  hipLaunchKernelGGL(k_infer_n_samples, dim3(ug_blocks(n_rays, 256)), dim3(256), 0, ST(s), rays_d, t_min,
                     t_max, stepdist, n_rays, n_samples);
  UG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ugrid_infer_ray_start_dir(const float *rays_o, const float *rays_d, const float *t_min,
                                         int64_t n_rays, float *rays_start, float *rays_dir,
                                         ugrid_stream_t s) {
  if (n_rays <= 0) return 0;
  hipLaunchKernelGGL(k_infer_ray_start_dir, dim3(ug_blocks(n_rays, 256)), dim3(256), 0, ST(s), rays_o,
                     rays_d, t_min, n_rays, rays_start, rays_dir);
  UG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ugrid_sample_pts_on_rays_count(const float *rays_o, const float *rays_d,
                                              const float *xyz_min, const float *xyz_max, float near,
                                              float far, float stepdist, int64_t n_rays, float *t_min,
                                              float *t_max, int64_t *n_steps, int64_t *n_steps_cumsum,
                                              int64_t *d_total, void *scan_ws, ugrid_stream_t s) {
  if (n_rays <= 0) return (int)hipMemsetAsync(d_total, 0, sizeof(int64_t), ST(s));
  hipLaunchKernelGGL(k_sample_count, dim3(ug_blocks(n_rays, 256)), dim3(256), 0, ST(s), rays_o, rays_d,
                     xyz_min, xyz_max, near, far, stepdist, n_rays, t_min, t_max, n_steps);
  UG_LAUNCH_CHECK();
  return ug_inclusive_scan(n_steps, n_rays, n_steps_cumsum, d_total, scan_ws, ST(s));
}

extern "C" int ugrid_sample_pts_on_rays_fill(const float *rays_o, const float *rays_d,
                                             const float *xyz_min, const float *xyz_max,
                                             const float *t_min, const int64_t *n_steps_cumsum,
                                             float stepdist, int64_t n_rays, int64_t total_len,
                                             float *rays_pts, uint8_t *mask_outbbox, int64_t *ray_id,
                                             int64_t *step_id, ugrid_stream_t s) {
  if (total_len <= 0 || n_rays <= 0) return 0;
  hipLaunchKernelGGL(k_sample_fill, dim3(ug_blocks(total_len, 256)), dim3(256), 0, ST(s), rays_o, rays_d,
                     xyz_min, xyz_max, t_min, n_steps_cumsum, stepdist, n_rays, total_len, rays_pts,
                     mask_outbbox, ray_id, step_id);
  UG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ugrid_sample_ndc_pts_on_rays(const float *rays_o, const float *rays_d,
                                            const float *xyz_min, const float *xyz_max,
                                            int64_t n_samples, int64_t n_rays, float *rays_pts,
                                            uint8_t *mask_outbbox, ugrid_stream_t s) {
  const int64_t total = n_samples * n_rays;
  if (total <= 0) return 0;
  hipLaunchKernelGGL(k_sample_ndc, dim3(ug_blocks(total, 256)), dim3(256), 0, ST(s), rays_o, rays_d,
                     xyz_min, xyz_max, (int)n_samples, total, rays_pts, mask_outbbox);
  UG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ugrid_sample_bg_pts_on_rays(const float *rays_o, const float *rays_d, const float *t_max,
                                           float bg_preserve, int64_t n_samples, int64_t n_rays,
                                           float *rays_pts, ugrid_stream_t s) {
  const int64_t total = n_samples * n_rays;
  if (total <= 0) return 0;
  hipLaunchKernelGGL(k_sample_bg, dim3(ug_blocks(total, 256)), dim3(256), 0, ST(s), rays_o, rays_d, t_max,
                     bg_preserve, (int)n_samples, total, rays_pts);
  UG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ugrid_maskcache_lookup(const uint8_t *world, const float *xyz, const float *scale,
                                      const float *shift, int64_t sz_i, int64_t sz_j, int64_t sz_k,
                                      int64_t n_pts, uint8_t *out, ugrid_stream_t s) {
  if (n_pts <= 0) return 0;
  hipLaunchKernelGGL(k_maskcache, dim3(ug_blocks(n_pts, 256)), dim3(256), 0, ST(s), world, xyz, scale,
                     shift, sz_i, sz_j, sz_k, n_pts, out);
  UG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ugrid_hit_coarse_geo(const float *rays_o, const float *rays_d, int64_t n_rays, const float *xyz_min,
                                    const float *xyz_max, float near, float far, float stepdist, const uint8_t *mask, int64_t mi,
                                    int64_t mj, int64_t mk, const float *xyz2ijk_scale, const float *xyz2ijk_shift, uint8_t *hit,
                                    ugrid_stream_t s) {
  if (n_rays <= 0) return 0;
  if (!rays_o || !rays_d || !xyz_min || !xyz_max || !mask || !xyz2ijk_scale || !xyz2ijk_shift || !hit || mi < 1 || mj < 1 || mk < 1 ||
      !(stepdist > 0.f))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_hit_coarse_geo, dim3(ug_blocks(n_rays, 256)), dim3(256), 0, ST(s), rays_o, rays_d, n_rays, xyz_min, xyz_max, near, far,
                     stepdist, mask, mi, mj, mk, xyz2ijk_scale, xyz2ijk_shift, hit);
  UG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ugrid_raw2alpha(const float *density, float shift, float interval,
                               const float *interval_arr, int64_t n, float *exp_d, float *alpha,
                               ugrid_stream_t s) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_raw2alpha, dim3(ug_blocks(n, 256)), dim3(256), 0, ST(s), density, shift, interval,
                     interval_arr, n, exp_d, alpha);
  UG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ugrid_raw2alpha_backward(const float *exp_d, const float *grad_back, float interval,
                                        const float *interval_arr, int64_t n, float *grad,
                                        ugrid_stream_t s) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_raw2alpha_bwd, dim3(ug_blocks(n, 256)), dim3(256), 0, ST(s), exp_d, grad_back,
                     interval, interval_arr, n, grad);
  UG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ugrid_alpha2weight(const float *alpha, const int64_t *ray_id, int64_t n, int64_t n_rays,
                                  float *weight, float *T, float *alphainv_last, int64_t *i_start,
                                  int64_t *i_end, ugrid_stream_t s) {
  if (n_rays <= 0) return 0;
  UG_HIP(hipMemsetAsync(i_start, 0, sizeof(int64_t) * n_rays, ST(s)));
  UG_HIP(hipMemsetAsync(i_end, 0, sizeof(int64_t) * n_rays, ST(s)));
  if (n > 0)
    hipLaunchKernelGGL(k_segments, dim3(ug_blocks(n, 256)), dim3(256), 0, ST(s), ray_id, n, i_start, i_end);
  // 4 rays (waves) per 256-thread block; empty rays just write alphainv_last = 1
  hipLaunchKernelGGL(k_alpha2weight, dim3(ug_blocks(n_rays * UG_WAVE, 256)), dim3(256), 0, ST(s), alpha,
                     n_rays, weight, T, alphainv_last, i_start, i_end);
  UG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ugrid_alpha2weight_backward(const float *alpha, const float *weight, const float *T,
                                           const float *alphainv_last, const int64_t *i_start,
                                           const int64_t *i_end, int64_t n, int64_t n_rays,
                                           const float *grad_weights, const float *grad_last,
                                           float *grad, ugrid_stream_t s) {
  if (n > 0) UG_HIP(hipMemsetAsync(grad, 0, sizeof(float) * n, ST(s)));
  if (n_rays <= 0 || n <= 0) return 0;
  hipLaunchKernelGGL(k_alpha2weight_bwd, dim3(ug_blocks(n_rays * UG_WAVE, 256)), dim3(256), 0, ST(s),
                     alpha, weight, T, alphainv_last, i_start, i_end, n_rays, grad_weights, grad_last, grad);
  UG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ugrid_cumdist_thres(const float *dist, float thres, int64_t n_rays, int64_t n_pts,
                                   uint8_t *mask, ugrid_stream_t s) {
  if (n_rays <= 0 || n_pts <= 0) return 0;
  hipLaunchKernelGGL(k_cumdist, dim3(ug_blocks(n_rays * UG_WAVE, 256)), dim3(256), 0, ST(s), dist, thres,
                     n_rays, n_pts, mask);
  UG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ugrid_segment_cumsum(const float *w, const float *s_, const int64_t *ray_id, int64_t n, int64_t n_rays,
                                    float *w_prefix, float *w_total, float *ws_prefix, float *ws_total,
                                    int64_t *seg_scratch, ugrid_stream_t s) {
  if (n_rays <= 0) return 0;
  int64_t *i_start = seg_scratch, *i_end = seg_scratch + n_rays;   // zero = "ray without samples"
  UG_HIP(hipMemsetAsync(seg_scratch, 0, sizeof(int64_t) * 2 * n_rays, ST(s)));
  if (n > 0)
    hipLaunchKernelGGL(k_segments, dim3(ug_blocks(n, 256)), dim3(256), 0, ST(s), ray_id, n, i_start, i_end);
  hipLaunchKernelGGL(k_segment_cumsum, dim3(ug_blocks(n_rays * UG_WAVE, 256)), dim3(256), 0, ST(s), w, s_, n_rays,
                     i_start, i_end, w_prefix, w_total, ws_prefix, ws_total);
  UG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ugrid_rays_of_a_view(int32_t H, int32_t W, const float *h_K9, const float *c2w, int inverse_y, int flip_x,
                                    int flip_y, int mode_center, const int64_t *pixel_index, int64_t n, float *rays_o,
                                    float *rays_d, float *viewdirs, ugrid_stream_t s) {
  if (n <= 0) return 0;
  if (H <= 0 || W <= 0) return (int)hipErrorInvalidValue;
  ug_cam c;
  c.fx = h_K9[0]; c.fy = h_K9[4]; c.cx = h_K9[2]; c.cy = h_K9[5];
  c.W = W; c.H = H; c.inverse_y = inverse_y; c.flip_x = flip_x; c.flip_y = flip_y; c.center = mode_center;
  hipLaunchKernelGGL(k_rays_of_a_view, dim3(ug_blocks(n, 256)), dim3(256), 0, ST(s), c, c2w, pixel_index, n, rays_o, rays_d,
                     viewdirs);
  UG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ugrid_rays_of_a_view_ndc(int32_t H, int32_t W, const float *h_K9, const float *c2w, int inverse_y, int flip_x,
                                        int flip_y, int mode_center, const int64_t *pixel_index, int64_t n, float near,
                                        float *rays_o, float *rays_d, float *viewdirs, ugrid_stream_t s) {
  if (n <= 0) return 0;
  if (H <= 0 || W <= 0) return (int)hipErrorInvalidValue;
  ug_cam c;
  c.fx = h_K9[0]; c.fy = h_K9[4]; c.cx = h_K9[2]; c.cy = h_K9[5];
  c.W = W; c.H = H; c.inverse_y = inverse_y; c.flip_x = flip_x; c.flip_y = flip_y; c.center = mode_center;
  ug_ndc q;
  const double focal = (double)h_K9[0], nr = (double)near;
  q.near = near;
  q.kx = (float)(-1. / ((double)W / (2. * focal)));
  q.ky = (float)(-1. / ((double)H / (2. * focal)));
  q.two_near = (float)(2. * nr);
  q.mtwo_near = (float)(-2. * nr);
  hipLaunchKernelGGL(k_rays_of_a_view_ndc, dim3(ug_blocks(n, 256)), dim3(256), 0, ST(s), c, q, c2w, pixel_index, n, rays_o,
                     rays_d, viewdirs);
  UG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ugrid_ray_batch(const ugrid_ray_cam *cams, const int64_t *view_start, int32_t n_views, const int64_t *index,
                               int64_t n, const void *images, int image_kind, int inverse_y, int flip_x, int flip_y,
                               int mode_center, int ndc, float near, float *target, float *rays_o, float *rays_d, float *viewdirs,
                               float *indexs, ugrid_stream_t s) {
  if (n <= 0) return 0;
  if (n_views <= 0 || (image_kind != 0 && image_kind != 1)) return (int)hipErrorInvalidValue;
  const double nr = (double)near;
  hipLaunchKernelGGL(k_ray_batch, dim3(ug_blocks(n, 256)), dim3(256), 0, ST(s), cams, view_start, (int)n_views, index, n, images,
                     image_kind, inverse_y, flip_x, flip_y, mode_center, ndc, near, (float)(2. * nr), (float)(-2. * nr), target,
                     rays_o, rays_d, viewdirs, indexs);
  UG_LAUNCH_CHECK();
  return 0;
}
