// Image metrics of a rendered frame against its ground truth, on the device: the squared-error sum (PSNR) and the SSIM map of
// the reference's utils.rgb_ssim (FourierGrid/utils.py:79-125, after mip-NeRF's internal/math.py) in one pass over the frame.
//
// Arithmetic contract = what rgb_ssim does on float32 images: the products img0^2, img1^2, img0 img1 are formed in fp32 and
// widened; both passes of the separable 11-tap Gaussian ("valid" mode: the map is [(H-10),(W-10),3]), the variance clamps, the
// sign / min / sqrt clip of the covariance and the quotient run in fp64 (sqrt and / IEEE-rounded; the file is built with
// -ffp-contract=off, so the only fused operations are the blur's explicit fma()).  An fp32 map is off by up to 5.7e-4 on a nearly
// flat bright frame, where E[x^2] - mu^2 cancels against c2 = 9e-4: fp64 is the point of this kernel.
//
// k_frame_metrics: one workgroup of 256 threads per UG_MT_Y x UG_MT_X = 32 x 54 tile of the map, one colour channel at a time:
//   stage   the (32+10) x (54+10) = 42 x 64 input pixels of both images in LDS (loads from clamped addresses: whatever a clamped
//           pixel contributes only reaches map elements outside the image, which are masked out of the sum and never stored);
//           the same registers feed the squared-error sum of the pixels the tile owns (each pixel of the frame has one owner);
//           the next channel's loads are issued before the passes of this one;
//   pass 1  along the rows' axis, as the reference's convolve2d(z, filt[:, None]) comes first: a thread takes one of the 64 columns
//           and 8 consecutive output rows, reads 18 input rows, forms the five moments and keeps 5 x 8 fp64 accumulators;
//           result [5][32][64 (+1: the row stride of 65 doubles keeps pass 2's row-per-lane reads off one bank)] fp64 in LDS;
//   pass 2  along the columns' axis: a thread takes one row and 9 consecutive map columns (192 of the 256 threads), then evaluates
//           the pointwise formula and adds the 9 values to its partial sum.
// LDS: 2 x 42 x 64 x 4 + 5 x 32 x 65 x 8 = 104704 bytes, one workgroup per CU.
// Reduction: fixed-order tree per workgroup -> ws[tile] = {sq_err, ssim} (fp64); k_frame_metrics_sum adds the tiles' partials in a
// fixed order (one workgroup: strided sums, then a tree).  No floating-point atomics: two runs give the same bits.
#include "ugrid_common.h"

#include <math.h>

#define UG_MT_Y 32
#define UG_MT_X 54
#define UG_MHALO 10
#define UG_MIN_Y (UG_MT_Y + UG_MHALO)   // 42 staged rows
#define UG_MIN_X (UG_MT_X + UG_MHALO)   // 64 staged columns
#define UG_MV_STRIDE 65                 // doubles per row of the pass-1 result
#define UG_MTHREADS 256
#define UG_MLOADS ((UG_MIN_Y * UG_MIN_X + UG_MTHREADS - 1) / UG_MTHREADS)   // 11 staged pixels per thread (the last round is half full)
#define UG_M_LDS_BYTES (2 * UG_MIN_Y * UG_MIN_X * 4 + 5 * UG_MT_Y * UG_MV_STRIDE * 8)

struct ug_taps11 { double w[11]; };

static_assert(UG_MIN_X == 64, "pass 1 maps one wave lane to one staged column");
static_assert(UG_MT_Y % 8 == 0 && (UG_MT_Y / 8) * UG_MIN_X == UG_MTHREADS, "pass 1: 8 output rows per thread");
static_assert(UG_MT_X % 9 == 0 && (UG_MT_X / 9) * UG_MT_Y <= UG_MTHREADS, "pass 2: 9 map columns per thread");

__global__ __launch_bounds__(UG_MTHREADS) void
k_frame_metrics(const float *__restrict__ img, int64_t stride_img, const float *__restrict__ gt, int64_t stride_gt, int H, int W,
                ug_taps11 taps, double c1, double c2, double *__restrict__ partial, double *__restrict__ map) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  float *in0 = reinterpret_cast<float *>(lds_raw);                       // [42][64]
  float *in1 = in0 + UG_MIN_Y * UG_MIN_X;                                // [42][64]
  double *mid = reinterpret_cast<double *>(in1 + UG_MIN_Y * UG_MIN_X);   // [5][32][65]; re-used by the final reduction
  const int tid = (int)threadIdx.x;
  const int tx = (int)blockIdx.x, ty = (int)blockIdx.y;
  const int x0 = tx * UG_MT_X, y0 = ty * UG_MT_Y;
  const int mapH = H - UG_MHALO, mapW = W - UG_MHALO;
  const bool last_x = tx == (int)gridDim.x - 1, last_y = ty == (int)gridDim.y - 1;

  // staged pixel i of this thread: slot tid + 256 i of the 42 x 64 tile (the last round's upper half repeats slot 2687).
  // Bit i of `own`: the frame's pixel belongs to this tile -- the tile whose map rows / columns start at or below it; the last
  // tile of an axis also owns the 10 rows / columns beyond its map.  (Offsets are recomputed per channel: cheaper than 44 registers.)
  const int own_y = min(last_y ? UG_MIN_Y : UG_MT_Y, H - y0), own_x = min(last_x ? UG_MIN_X : UG_MT_X, W - x0);
  unsigned own = 0u;
#pragma unroll
  for (int i = 0; i < UG_MLOADS; ++i) {
    const int s = tid + UG_MTHREADS * i;       // (s >> 6 < own_y <= 42 implies s < 42 * 64)
    own |= ((s >> 6) < own_y && (s & 63) < own_x) ? 1u << i : 0u;
  }
  auto pixel = [&](int i) -> int64_t {
    const int s = tid + UG_MTHREADS * i;
    const int sc = s < UG_MIN_Y * UG_MIN_X ? s : UG_MIN_Y * UG_MIN_X - 1;
    const int y = y0 + (sc >> 6), x = x0 + (sc & 63);
    return (int64_t)(y < H ? y : H - 1) * W + (x < W ? x : W - 1);
  };
  float ra[UG_MLOADS], rb[UG_MLOADS];
#pragma unroll
  for (int i = 0; i < UG_MLOADS; ++i) {
    const int64_t p = pixel(i);
    ra[i] = img[p * stride_img];
    rb[i] = gt[p * stride_gt];
  }

  double sq_sum = 0.0, ssim_sum = 0.0;
  for (int c = 0; c < 3; ++c) {
    // (the empty asm keeps the per-pixel masks of `own` and `n_in` from being hoisted out of the channel loop as 20 wave masks
    // held in scalar registers, which spilled)
    unsigned own_c = own;
    asm volatile("" : "+v"(own_c));
#pragma unroll
    for (int i = 0; i < UG_MLOADS; ++i) {
      const int s = tid + UG_MTHREADS * i;
      const int sc = s < UG_MIN_Y * UG_MIN_X ? s : UG_MIN_Y * UG_MIN_X - 1;
      in0[sc] = ra[i];
      in1[sc] = rb[i];
      const float d = ra[i] - rb[i];           // numpy on float32 arrays: difference and square in fp32, the sum in fp64
      const float q = d * d;
      sq_sum += ((own_c >> i) & 1u) ? (double)q : 0.0;
    }
    __syncthreads();
    if (c < 2) {
#pragma unroll
      for (int i = 0; i < UG_MLOADS; ++i) {
        const int64_t p = pixel(i);
        ra[i] = img[p * stride_img + c + 1];
        rb[i] = gt[p * stride_gt + c + 1];
      }
    }
    // ---- pass 1: rows' axis
    {
      const int col = tid & 63, r0 = (tid >> 6) * 8;
      double acc[5][8];
#pragma unroll
      for (int m = 0; m < 5; ++m)
#pragma unroll
        for (int r = 0; r < 8; ++r) acc[m][r] = 0.0;
#pragma unroll
      for (int j = 0; j < 18; ++j) {
        const float a = in0[(r0 + j) * UG_MIN_X + col], b = in1[(r0 + j) * UG_MIN_X + col];
        const double v[5] = {(double)a, (double)b, (double)(a * a), (double)(b * b), (double)(a * b)};
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          const int k = j - r;
          if (k >= 0 && k <= 10) {
#pragma unroll
            for (int m = 0; m < 5; ++m) acc[m][r] = fma(taps.w[k], v[m], acc[m][r]);
          }
        }
      }
#pragma unroll
      for (int m = 0; m < 5; ++m)
#pragma unroll
        for (int r = 0; r < 8; ++r) mid[(m * UG_MT_Y + r0 + r) * UG_MV_STRIDE + col] = acc[m][r];
    }
    __syncthreads();
    // ---- pass 2: columns' axis, then the pointwise formula
    if (tid < UG_MT_Y * (UG_MT_X / 9)) {
      const int row = tid & (UG_MT_Y - 1), g0 = (tid / UG_MT_Y) * 9;
      double o[5][9];
#pragma unroll
      for (int m = 0; m < 5; ++m) {
        double v[19];
#pragma unroll
        for (int j = 0; j < 19; ++j) v[j] = mid[(m * UG_MT_Y + row) * UG_MV_STRIDE + g0 + j];
#pragma unroll
        for (int i = 0; i < 9; ++i) {
          double s = 0.0;
#pragma unroll
          for (int k = 0; k < 11; ++k) s = fma(taps.w[k], v[i + k], s);
          o[m][i] = s;
        }
      }
      const int y = y0 + row;
      int n_in = y < mapH ? mapW - (x0 + g0) : 0;       // map elements of this thread's 9 that lie inside the map: the first n_in
      asm volatile("" : "+v"(n_in));
#pragma unroll
      for (int i = 0; i < 9; ++i) {
        const double mu0 = o[0][i], mu1 = o[1][i];
        const double mu00 = mu0 * mu0, mu11 = mu1 * mu1, mu01 = mu0 * mu1;
        double s00 = o[2][i] - mu00, s11 = o[3][i] - mu11, s01 = o[4][i] - mu01;
        s00 = s00 > 0.0 ? s00 : 0.0;                       // np.maximum(0., sigma)
        s11 = s11 > 0.0 ? s11 : 0.0;
        const double lim = sqrt(s00 * s11), mag = fabs(s01);
        const double sgn = s01 > 0.0 ? 1.0 : (s01 < 0.0 ? -1.0 : 0.0);
        s01 = sgn * (lim < mag ? lim : mag);               // np.sign(s01) * np.minimum(sqrt(s00 s11), |s01|)
        const double numer = (2.0 * mu01 + c1) * (2.0 * s01 + c2);
        const double denom = (mu00 + mu11 + c1) * (s00 + s11 + c2);
        const double val = numer / denom;
        ssim_sum += i < n_in ? val : 0.0;
        o[0][i] = val;
      }
      if (map != nullptr) {
        double *dst = map + ((int64_t)y * mapW + x0 + g0) * 3 + c;
#pragma unroll
        for (int i = 0; i < 9; ++i)
          if (i < n_in) dst[3 * i] = o[0][i];
      }
    }
    // (no barrier here: the next channel's staging writes in0 / in1, last read before the barrier above; its pass 1 writes `mid`
    // only behind the next barrier, which every thread reaches after its pass 2)
  }

  // ---- the workgroup's two partial sums, fixed-order tree
  __syncthreads();
  double *red = mid;
  red[tid] = sq_sum;
  red[UG_MTHREADS + tid] = ssim_sum;
  __syncthreads();
  for (int n = UG_MTHREADS / 2; n > 0; n >>= 1) {
    if (tid < n) {
      red[tid] += red[tid + n];
      red[UG_MTHREADS + tid] += red[UG_MTHREADS + tid + n];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const int64_t t = (int64_t)ty * gridDim.x + tx;
    partial[2 * t] = red[0];
    partial[2 * t + 1] = red[UG_MTHREADS];
  }
}

// out[0] = sum of the tiles' squared-error partials, out[1] = sum of their SSIM partials: thread t adds tiles t, t + 256, ...
// in order, then the same tree as above.
__global__ __launch_bounds__(UG_MTHREADS) void
k_frame_metrics_sum(const double *__restrict__ partial, int64_t n_tiles, double *__restrict__ out) {
  __shared__ double red[2 * UG_MTHREADS];
  const int tid = (int)threadIdx.x;
  double a = 0.0, b = 0.0;
  for (int64_t t = tid; t < n_tiles; t += UG_MTHREADS) {
    a += partial[2 * t];
    b += partial[2 * t + 1];
  }
  red[tid] = a;
  red[UG_MTHREADS + tid] = b;
  __syncthreads();
  for (int n = UG_MTHREADS / 2; n > 0; n >>= 1) {
    if (tid < n) {
      red[tid] += red[tid + n];
      red[UG_MTHREADS + tid] += red[UG_MTHREADS + tid + n];
    }
    __syncthreads();
  }
  if (tid == 0) {
    out[0] = red[0];
    out[1] = red[UG_MTHREADS];
  }
}

static inline int64_t ug_metrics_tiles(int64_t H, int64_t W, int64_t *nty, int64_t *ntx) {
  *nty = (H - UG_MHALO + UG_MT_Y - 1) / UG_MT_Y;
  *ntx = (W - UG_MHALO + UG_MT_X - 1) / UG_MT_X;
  return *nty * *ntx;
}

extern "C" int64_t ugrid_frame_metrics_ws_bytes(int64_t H, int64_t W) {
  if (H < 11 || W < 11) return 0;
  int64_t nty, ntx;
  return ug_metrics_tiles(H, W, &nty, &ntx) * 16;
}

extern "C" int ugrid_frame_metrics(const float *img, int64_t img_stride, const float *gt, int64_t gt_stride, int64_t H, int64_t W,
                                   int32_t filter_size, double filter_sigma, double k1, double k2, double max_val, double *out,
                                   double *map, void *ws, ugrid_stream_t stream) {
  if (H < 11 || W < 11 || filter_size != 11) return (int)hipErrorInvalidValue;
  if (H > (1 << 24) || W > (1 << 24) || img_stride < 3 || gt_stride < 3 || !(filter_sigma > 0.0)) return (int)hipErrorInvalidValue;
  if (!img || !gt || !out || !ws) return (int)hipErrorInvalidValue;
  int64_t nty, ntx;
  const int64_t n_tiles = ug_metrics_tiles(H, W, &nty, &ntx);
  if (nty > 65535) return (int)hipErrorInvalidValue;
  ug_taps11 taps;
  double sum = 0.0;
  for (int i = 0; i < 11; ++i) {                 // utils.py:91-95 (hw = 5, shift = 0)
    const double t = (double)(i - 5) / filter_sigma;
    taps.w[i] = exp(-0.5 * (t * t));
    sum += taps.w[i];
  }
  for (int i = 0; i < 11; ++i) taps.w[i] /= sum;
  const double c1 = (k1 * max_val) * (k1 * max_val), c2 = (k2 * max_val) * (k2 * max_val);
  UG_SET_DYN_LDS(k_frame_metrics, UG_M_LDS_BYTES);
  hipStream_t st = (hipStream_t)stream;
  double *partial = (double *)ws;
  hipLaunchKernelGGL(k_frame_metrics, dim3((unsigned)ntx, (unsigned)nty), dim3(UG_MTHREADS), UG_M_LDS_BYTES, st, img, img_stride, gt,
                     gt_stride, (int)H, (int)W, taps, c1, c2, partial, map);
  UG_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_frame_metrics_sum, dim3(1), dim3(UG_MTHREADS), 0, st, (const double *)partial, n_tiles, out);
  UG_LAUNCH_CHECK();
  return 0;
}
