// 8-bit video frames on the device: what the reference's render program forms on the host with numpy from the float stacks of
// render_viewpoints (FourierGrid/run_render.py), here from the packed frame [H*W,5] = rgb(3), depth, alphainv_last where it lies:
//   ugrid_frame_rgb8       utils.to8b(rgbs) (:261, :283, :307) behind render_video_flipy / render_video_rot90 (:93-103)
//   ugrid_depth8_max       utils.to8b(1 - depths / np.max(depths)) (:284)
//   ugrid_depthvis_select  the order statistics np.percentile(depths_vis[bgmaps < 0.1], q) interpolates between (:308-313)
//   ugrid_depth8_map       to8b(cmap(1 - clip((depths_vis - dmin) / (dmax - dmin), 0, 1))[..., :3]) (:314-315), the map as a table
//
// Arithmetic contract (the file is built with -ffp-contract=off, nothing here is fused; `/` is IEEE-rounded, hipcc's default):
//   to8b(x)    (uint8) trunc(255.0f * min(max(x, 0), 1)), the fp32 product numpy forms on a float32 array; NaN -> 0 (numpy's cast of
//              NaN is undefined: 0 is this library's rule);
//   depth max  1.0f - d / dmax in fp32; dmax == 0 -> 0 everywhere;
//   depth vis  v = d * (1 - b) + b, three fp32 roundings; t = ((double)v - dmin) / (dmax - dmin) clipped to [0,1] with NaN kept,
//              x = 1 - t, i = (int)(x * 256), 256 -> 255, colour = table[i]; NaN -> (0,0,0): fp64, as numpy >= 2 evaluates the line.
//
// One kernel template serves the three byte producers.  Output orientation np.rot90(np.flip(img, 0) if flipy else img, k): the
// source pixel of output pixel (i, j) is s0 + i*si + j*sj (ugrid_video_plan: five integers, no index table).
// Thread mapping, as k_frame_assemble: a lane owns 16 consecutive OUTPUT bytes counted from the 16-byte boundary at or below
// `out`, so a wave stores 1 KiB contiguous with global_store_dwordx4 whatever the pointer's alignment; the chunks that reach over
// the head or the tail of the frame (H'*W'*C is no multiple of 4 in general) store their bytes one by one.  A lane walks the 5-6
// pixels of its chunk incrementally (no division per byte); with k even they are neighbours in the source, 20 bytes apart, and
// the wave reads ~6.7 KB contiguous; with k odd a lane's pixels are W source pixels apart and it is the lanes of the waves of the
// 6 neighbouring output LINES that share a 128-byte source line (L2): the strided read is kept, see DESIGN.md 7.2 for the
// measured time of both orientations.
// The lane that owns a pixel's channel-0 byte also writes the pixel's (depth, alphainv_last) to db [H*W,2] in SOURCE order and
// feeds the running depth maximum: order-preserving uint32 keys, max over the wave by shuffles, over the workgroup in LDS, then at
// most ONE integer atomic max per workgroup -- independent of arrival order, so two runs leave the same word.  (The db pairs are
// stored per owned pixel, 8 bytes a lane and ~43 bytes apart within an instruction: partial-line writes, which cost more than the
// rest of the kernel at 1080p -- DESIGN.md 7.2 has the figures and the store shape that would avoid it.)
//
// ugrid_depthvis_select: radix select on the same keys, digits of 11 / 11 / 10 bits from the top.  k_select_hist counts the
// digit of every pixel that takes part and whose higher bits equal one of up to four prefixes (one per requested rank) in LDS
// histograms with integer adds, then adds every non-empty bin to the global counters with one integer atomic.  The HOST reads the
// counters between the passes (8 KB per prefix) and picks the bins: the call runs once per video, after the frame loop, and
// returns host values, so it synchronises the stream anyway; a one-wave device kernel choosing the bins would save nothing.
#include "ugrid_common.h"

#include <string.h>

#define UG_VD_THREADS 256
#define UG_VD_MAX_BLOCKS 4096
#define UG_VD_CHUNK 16
#define UG_SEL_BINS 2048
#define UG_SEL_MAXRANKS 4

enum { UG_VD_RGB = 0, UG_VD_DEPTHMAX = 1, UG_VD_DEPTHMAP = 2 };

struct ug_video_args {
  int total;        // output bytes H'*W'*C
  int mis;          // (uintptr_t)out & 15
  int Wo;           // output pixels per line
  int s0, si, sj;   // source pixel of output pixel (i, j) = s0 + i*si + j*sj
  int stride;       // floats per source pixel (UG_VD_RGB; the db modes read pairs)
  float dmax_f;     // UG_VD_DEPTHMAX
  double dmin, dmax;   // UG_VD_DEPTHMAP
};

// order-preserving key of an fp32 value: a < b (as floats, -0.0 below +0.0) <=> key(a) < key(b)
__device__ __forceinline__ uint32_t ug_f32_key(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ uint32_t ug_to8b(float x) {
  float c = x > 0.0f ? x : 0.0f;      // (NaN compares false: 0)
  c = c < 1.0f ? c : 1.0f;
  return (uint32_t)(255.0f * c);
}

__device__ __forceinline__ float ug_depth_vis(float d, float b) {
  const float t = 1.0f - b;
  const float u = d * t;
  return u + b;
}

// the bytes of source pixel p, channel c in bits 8c..8c+7
template <int MODE>
__device__ __forceinline__ uint32_t ug_video_pixel(unsigned p, const float *__restrict__ src, const uint8_t *__restrict__ table,
                                                   const ug_video_args &a) {
  if (MODE == UG_VD_RGB) {
    const float *px = src + p * (unsigned)a.stride;
    return ug_to8b(px[0]) | (ug_to8b(px[1]) << 8) | (ug_to8b(px[2]) << 16);
  }
  const float2 db = reinterpret_cast<const float2 *>(src)[p];
  if (MODE == UG_VD_DEPTHMAX) return a.dmax_f == 0.0f ? 0u : ug_to8b(1.0f - db.x / a.dmax_f);
  const double t = ((double)ug_depth_vis(db.x, db.y) - a.dmin) / (a.dmax - a.dmin);
  const double tc = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);      // (NaN stays NaN, as np.clip keeps it)
  const double x = 1.0 - tc;
  if (!(x == x)) return 0u;
  int i = (int)(x * 256.0);
  i = i > 255 ? 255 : i;
  const uint8_t *e = table + 3 * i;
  return (uint32_t)e[0] | ((uint32_t)e[1] << 8) | ((uint32_t)e[2] << 16);
}

template <int MODE>
__global__ __launch_bounds__(UG_VD_THREADS) void
k_video_bytes(const float *__restrict__ src, const uint8_t *__restrict__ table, ug_video_args a, uint8_t *__restrict__ out,
              float *__restrict__ db_out, uint32_t *__restrict__ dmax_key) {
  constexpr int C = MODE == UG_VD_DEPTHMAX ? 1 : 3;
  __shared__ uint32_t wave_max[UG_VD_THREADS / UG_WAVE];
  const int n_chunks = (a.total + a.mis + UG_VD_CHUNK - 1) / UG_VD_CHUNK;
  uint8_t *base = out - a.mis;               // 16-byte aligned; chunk g covers output bytes [16 g - mis, 16 g - mis + 16)
  uint32_t kmax = 0u;
  for (int g = (int)(blockIdx.x * UG_VD_THREADS + threadIdx.x); g < n_chunks; g += (int)(gridDim.x * UG_VD_THREADS)) {
    const int e0 = g * UG_VD_CHUNK - a.mis;
    const int first = e0 > 0 ? e0 : 0;
    const int op = first / C;
    int c = first - op * C;
    const int i = op / a.Wo;
    int j = op - i * a.Wo;
    int p = a.s0 + i * a.si + j * a.sj;
    uint32_t pix = 0u;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int t = 0; t < UG_VD_CHUNK; ++t) {
      const int e = e0 + t;
      if (e >= 0 && e < a.total) {
        if (e == first || c == 0) pix = ug_video_pixel<MODE>((unsigned)p, src, table, a);
        if (MODE == UG_VD_RGB && c == 0 && (db_out != nullptr || dmax_key != nullptr)) {      // this lane owns the pixel
          const float *px = src + (unsigned)p * (unsigned)a.stride;
          const float d = px[3], b = px[4];
          if (db_out != nullptr) reinterpret_cast<float2 *>(db_out)[(unsigned)p] = make_float2(d, b);
          const uint32_t key = ug_f32_key(d);
          kmax = key > kmax ? key : kmax;
        }
        w[t >> 2] |= ((pix >> (8 * c)) & 255u) << (8 * (t & 3));
        if (++c == C) {
          c = 0;
          p += a.sj;
          if (++j == a.Wo) {
            j = 0;
            p += a.si - a.Wo * a.sj;
          }
        }
      }
    }
    if (e0 >= 0 && e0 + UG_VD_CHUNK <= a.total) {
      *reinterpret_cast<uint4 *>(base + (size_t)g * UG_VD_CHUNK) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
      for (int t = 0; t < UG_VD_CHUNK; ++t)
        if (e0 + t >= 0 && e0 + t < a.total) out[e0 + t] = (uint8_t)(w[t >> 2] >> (8 * (t & 3)));
    }
  }
  if (MODE == UG_VD_RGB && dmax_key != nullptr) {      // (wave-uniform: a kernel argument)
#pragma unroll
    for (int s = UG_WAVE / 2; s > 0; s >>= 1) {
      const uint32_t o = (uint32_t)__shfl_xor((int)kmax, s, UG_WAVE);
      kmax = o > kmax ? o : kmax;
    }
    if (ug_lane() == 0) wave_max[threadIdx.x / UG_WAVE] = kmax;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t m = wave_max[0];
#pragma unroll
      for (int k = 1; k < UG_VD_THREADS / UG_WAVE; ++k) m = wave_max[k] > m ? wave_max[k] : m;
      // (the word only grows: a block whose maximum does not exceed what is already there has nothing to add, and skipping it
      // keeps the same-address atomics of a frame to the few blocks that raise the word instead of one per workgroup)
      if (m > __hip_atomic_load(dmax_key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(dmax_key, m);
    }
  }
}

struct ug_select_args {
  unsigned n;            // pixels
  float thres;
  int n_pre;             // prefixes (1..4); pass 1: one prefix that every key matches (pre_shift = 32)
  int pre_shift;         // a key matches prefix q when key >> pre_shift == pre[q] (32: always)
  int d_shift, d_bits;   // digit = (key >> d_shift) & ((1 << d_bits) - 1)
  uint32_t pre[UG_SEL_MAXRANKS];
};

__global__ __launch_bounds__(UG_VD_THREADS) void
k_select_hist(const float *__restrict__ db, ug_select_args a, uint32_t *__restrict__ counters) {
  __shared__ uint32_t hist[UG_SEL_MAXRANKS * UG_SEL_BINS];
  const int n_bins = a.n_pre * UG_SEL_BINS;
  for (int b = (int)threadIdx.x; b < n_bins; b += UG_VD_THREADS) hist[b] = 0u;
  __syncthreads();
  const uint32_t mask = (1u << a.d_bits) - 1u;
  for (unsigned p = blockIdx.x * UG_VD_THREADS + threadIdx.x; p < a.n; p += gridDim.x * UG_VD_THREADS) {
    const float2 v = reinterpret_cast<const float2 *>(db)[p];
    if (v.y < a.thres) {
      const uint32_t key = ug_f32_key(ug_depth_vis(v.x, v.y));
      const uint32_t hi = a.pre_shift >= 32 ? 0u : key >> a.pre_shift;
      const uint32_t digit = (key >> a.d_shift) & mask;
      for (int q = 0; q < a.n_pre; ++q)
        if (hi == a.pre[q]) atomicAdd(&hist[q * UG_SEL_BINS + digit], 1u);
    }
  }
  __syncthreads();
  for (int b = (int)threadIdx.x; b < n_bins; b += UG_VD_THREADS) {
    const uint32_t h = hist[b];
    if (h != 0u) atomicAdd(&counters[b], h);
  }
}

// np.rot90(np.flip(img, 0) if flipy else img, k, axes=(0,1)) of an H x W image as an affine source index
extern "C" int ugrid_video_plan(int64_t H, int64_t W, int32_t flipy, int32_t k, int64_t *plan) {
  if (H <= 0 || W <= 0 || H > INT32_MAX || W > INT32_MAX || !plan || H * W > INT32_MAX) return (int)hipErrorInvalidValue;
  const int q = ((k % 4) + 4) % 4;
  // rot90 of an Hm x Wm image m: k = 1: out[i][j] = m[j][Wm-1-i]; 2: m[Hm-1-i][Wm-1-j]; 3: m[Hm-1-j][i];  (y, x) = A (i, j) + c
  int64_t yi, yj, yc, xi, xj, xc;
  switch (q) {
    case 0: yi = 1, yj = 0, yc = 0, xi = 0, xj = 1, xc = 0; break;
    case 1: yi = 0, yj = 1, yc = 0, xi = -1, xj = 0, xc = W - 1; break;
    case 2: yi = -1, yj = 0, yc = H - 1, xi = 0, xj = -1, xc = W - 1; break;
    default: yi = 0, yj = -1, yc = H - 1, xi = 1, xj = 0, xc = 0; break;
  }
  if (flipy) yi = -yi, yj = -yj, yc = H - 1 - yc;      // m[y][x] = img[H-1-y][x]
  plan[0] = (q & 1) ? W : H;
  plan[1] = (q & 1) ? H : W;
  plan[2] = yc * W + xc;
  plan[3] = yi * W + xi;
  plan[4] = yj * W + xj;
  return 0;
}

template <int MODE>
static int ug_video_launch(const float *src, const uint8_t *table, int64_t H, int64_t W, int64_t stride, int32_t flipy, int32_t k,
                           ug_video_args a, uint8_t *out, float *db, uint32_t *dmax_key, ugrid_stream_t stream) {
  constexpr int C = MODE == UG_VD_DEPTHMAX ? 1 : 3;
  if (H <= 0 || W <= 0 || H > INT32_MAX || W > INT32_MAX || stride > INT32_MAX) return (int)hipErrorInvalidValue;
  if (H * W > INT32_MAX / stride || H * W * C > INT32_MAX - 2 * UG_VD_CHUNK) return (int)hipErrorInvalidValue;
  if (!src || !out) return (int)hipErrorInvalidValue;
  int64_t plan[5];
  const int err = ugrid_video_plan(H, W, flipy, k, plan);
  if (err) return err;
  a.total = (int)(H * W * C);
  a.mis = (int)((uintptr_t)out & (UG_VD_CHUNK - 1));
  a.Wo = (int)plan[1];
  a.s0 = (int)plan[2];
  a.si = (int)plan[3];
  a.sj = (int)plan[4];
  a.stride = (int)stride;
  const int64_t n_chunks = ((int64_t)a.total + a.mis + UG_VD_CHUNK - 1) / UG_VD_CHUNK;
  unsigned blocks = ug_blocks(n_chunks, UG_VD_THREADS);
  if (blocks > UG_VD_MAX_BLOCKS) blocks = UG_VD_MAX_BLOCKS;
  hipLaunchKernelGGL(k_video_bytes<MODE>, dim3(blocks), dim3(UG_VD_THREADS), 0, (hipStream_t)stream, src, table, a, out, db, dmax_key);
  UG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ugrid_frame_rgb8(const float *frame, int64_t stride, int64_t H, int64_t W, int32_t flipy, int32_t k, uint8_t *out,
                                float *db, uint32_t *dmax_key, ugrid_stream_t stream) {
  if (stride < 5) return (int)hipErrorInvalidValue;
  ug_video_args a = {};
  return ug_video_launch<UG_VD_RGB>(frame, nullptr, H, W, stride, flipy, k, a, out, db, dmax_key, stream);
}

extern "C" int ugrid_depth8_max(const float *db, int64_t H, int64_t W, int32_t flipy, int32_t k, float dmax, uint8_t *out,
                                ugrid_stream_t stream) {
  ug_video_args a = {};
  a.dmax_f = dmax;
  return ug_video_launch<UG_VD_DEPTHMAX>(db, nullptr, H, W, 2, flipy, k, a, out, nullptr, nullptr, stream);
}

extern "C" int ugrid_depth8_map(const float *db, int64_t H, int64_t W, int32_t flipy, int32_t k, double dmin, double dmax,
                                const uint8_t *table, uint8_t *out, ugrid_stream_t stream) {
  if (!table) return (int)hipErrorInvalidValue;
  ug_video_args a = {};
  a.dmin = dmin;
  a.dmax = dmax;
  return ug_video_launch<UG_VD_DEPTHMAP>(db, table, H, W, 2, flipy, k, a, out, nullptr, nullptr, stream);
}

extern "C" int64_t ugrid_depthvis_select_ws_bytes(void) { return (int64_t)UG_SEL_MAXRANKS * UG_SEL_BINS * sizeof(uint32_t); }

extern "C" int ugrid_depthvis_select(const float *db, int64_t n, float thres, int32_t m, const int64_t *ranks, int64_t *cnt,
                                     float *values, void *ws, ugrid_stream_t stream) {
  if (n < 0 || n > INT32_MAX || m < 0 || m > UG_SEL_MAXRANKS || !cnt) return (int)hipErrorInvalidValue;
  if (m > 0 && (!ranks || !values)) return (int)hipErrorInvalidValue;
  for (int r = 0; r < m; ++r)
    if (ranks[r] < 0 || (r > 0 && ranks[r] < ranks[r - 1])) return (int)hipErrorInvalidValue;
  if (n == 0) {
    if (m > 0) return (int)hipErrorInvalidValue;       // (every rank is >= the count)
    *cnt = 0;
    return 0;
  }
  if (!db || !ws) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  uint32_t *counters = (uint32_t *)ws;
  static thread_local uint32_t host[UG_SEL_MAXRANKS * UG_SEL_BINS];
  unsigned blocks = ug_blocks(n, UG_VD_THREADS * 8);      // (8 pixels per thread: the flush of a workgroup's bins is paid per 2048 pixels)
  if (blocks > 1024u) blocks = 1024u;
  int64_t rem[UG_SEL_MAXRANKS];      // rank of the wanted element among the keys that share its prefix
  uint32_t pre_of[UG_SEL_MAXRANKS];  // that prefix
  for (int r = 0; r < m; ++r) rem[r] = ranks[r], pre_of[r] = 0u;
  static const int d_shift[3] = {21, 10, 0}, d_bits[3] = {11, 11, 10};
  for (int pass = 0; pass < 3; ++pass) {
    ug_select_args a = {};
    a.n = (unsigned)n;
    a.thres = thres;
    a.pre_shift = d_shift[pass] + d_bits[pass];
    a.d_shift = d_shift[pass];
    a.d_bits = d_bits[pass];
    int slot_of[UG_SEL_MAXRANKS] = {0, 0, 0, 0};
    if (pass == 0) {
      a.n_pre = 1;
    } else {      // the distinct prefixes (ranks ascend, so equal prefixes are neighbours)
      for (int r = 0; r < m; ++r) {
        if (r == 0 || pre_of[r] != pre_of[r - 1]) a.pre[a.n_pre++] = pre_of[r];
        slot_of[r] = a.n_pre - 1;
      }
    }
    const size_t bytes = (size_t)a.n_pre * UG_SEL_BINS * sizeof(uint32_t);
    UG_HIP(hipMemsetAsync(counters, 0, bytes, st));
    hipLaunchKernelGGL(k_select_hist, dim3(blocks), dim3(UG_VD_THREADS), 0, st, db, a, counters);
    UG_LAUNCH_CHECK();
    UG_HIP(hipMemcpyAsync(host, counters, bytes, hipMemcpyDeviceToHost, st));
    UG_HIP(hipStreamSynchronize(st));
    if (pass == 0) {
      int64_t total = 0;
      for (int b = 0; b < UG_SEL_BINS; ++b) total += host[b];
      *cnt = total;
      for (int r = 0; r < m; ++r)
        if (ranks[r] >= total) return (int)hipErrorInvalidValue;
      if (m == 0) return 0;
    }
    for (int r = 0; r < m; ++r) {
      const uint32_t *h = host + slot_of[r] * UG_SEL_BINS;
      int64_t cum = 0;
      int b = 0;
      for (; b < (1 << d_bits[pass]) - 1; ++b) {
        if (rem[r] < cum + (int64_t)h[b]) break;
        cum += h[b];
      }
      rem[r] -= cum;
      pre_of[r] = (pre_of[r] << d_bits[pass]) | (uint32_t)b;
    }
  }
  for (int r = 0; r < m; ++r) {      // the full key: undo ug_f32_key
    const uint32_t key = pre_of[r], u = (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key;
    memcpy(&values[r], &u, 4);
  }
  return 0;
}
