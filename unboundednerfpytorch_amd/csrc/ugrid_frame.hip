// Frame assembly of the multi-GPU render path (dist.FramePipeline): the packed frame [H*W,5] = rgb(3), depth, alphainv_last per
// pixel, in image order, put together in ONE pass from
//   source A  the all-gathered buffer [world*per,5] of the ranks' rendered tiles, or
//   source B  the three per-ray arrays rgb [R,3] / depth [R] / last [R] of a single-device render (no packing),
// and the send tile [per,5] of a rank (rows 0..n from the three arrays, rows n..per zero) by the same kernel.
//
// The source row of a pixel is COMPUTED, no index table is read (an int64 table is 8 of the 28 bytes a pixel would move):
//   ray position   q = y*W + x, or with tile8 the 8 x 8 pixel-block order of fourier_render.pixel_tile_order:
//                  q = ((y>>3)*(W>>3) + (x>>3))*64 + lane, lane bits y2 x2 y1 x1 y0 x0;
//   bands          rank = q / per, off = q % per, row = rank*per + off = q: the contiguous split needs no arithmetic at all;
//   dealt          (dist.tile_assignment, groups of `dg` 64-ray tiles dealt round-robin) t = q>>6, g = t/dg,
//                  row = (g % world)*per + (((g / world)*dg + t % dg)<<6) + (q & 63).
//
// Thread mapping: one lane per FOUR consecutive output words -- the stores of a wave are 1 KiB contiguous (global_store_dwordx4),
// the integer arithmetic (a division by 5, by W, by dg and by world) is paid once or twice per 16 bytes, and the four loads of a
// lane fall into one or two 20-byte source rows; the rows of eight neighbouring pixels lie in one 1280-byte source block, so
// every fetched line is used whole by the wave or by the waves of the neighbouring image lines (L2).  The other candidate, a lane
// per source row, reads contiguously but scatters 20-byte stores over eight image lines: partial-line writes cost more than
// partial-line reads that the cache completes.  No LDS, no barrier; words are moved as uint32, so every bit pattern survives.
#include "ugrid_common.h"

#define UG_FR_THREADS 256
#define UG_FR_MAX_BLOCKS 4096

struct ug_frame_map {
  unsigned n_pix;    // output rows (H*W, or `per` for the send tile)
  unsigned n_valid;  // source rows that exist: output rows whose source row is >= n_valid are written as zero (send tile only)
  unsigned W, Wb;    // image width, blocks per block row (W>>3)
  unsigned per, world, dg;   // dg = 0: bands
  unsigned tile8;
};

__device__ __forceinline__ unsigned ug_frame_row(unsigned p, const ug_frame_map &m) {
  unsigned q = p;
  if (m.tile8) {
    const unsigned y = p / m.W, x = p - y * m.W;
    const unsigned lane = ((y & 4u) << 3) | ((x & 4u) << 2) | ((y & 2u) << 2) | ((x & 2u) << 1) | ((y & 1u) << 1) | (x & 1u);
    q = (((y >> 3) * m.Wb + (x >> 3)) << 6) | lane;
  }
  if (m.dg == 0u) return q;
  const unsigned t = q >> 6, g = t / m.dg, j = t - g * m.dg;
  const unsigned k = g / m.world, rank = g - k * m.world;
  return rank * m.per + (((k * m.dg + j) << 6) | (q & 63u));
}

template <bool ARRAYS>
__device__ __forceinline__ uint32_t ug_frame_word(unsigned row, unsigned c, const uint32_t *__restrict__ gathered,
                                                  const uint32_t *__restrict__ rgb, const uint32_t *__restrict__ depth,
                                                  const uint32_t *__restrict__ last) {
  if (ARRAYS) return c < 3u ? rgb[row * 3u + c] : (c == 3u ? depth[row] : last[row]);
  return gathered[row * 5u + c];
}

template <bool ARRAYS>
__global__ __launch_bounds__(UG_FR_THREADS) void
k_frame_assemble(const uint32_t *__restrict__ gathered, const uint32_t *__restrict__ rgb, const uint32_t *__restrict__ depth,
                 const uint32_t *__restrict__ last, ug_frame_map m, int vec_store, uint32_t *__restrict__ out) {
  const unsigned total = m.n_pix * 5u, n_quads = (total + 3u) >> 2;
  for (unsigned i = blockIdx.x * UG_FR_THREADS + threadIdx.x; i < n_quads; i += gridDim.x * UG_FR_THREADS) {
    const unsigned e0 = i << 2, p0 = e0 / 5u, c0 = e0 - p0 * 5u;
    const unsigned r0 = ug_frame_row(p0, m);
    unsigned r1 = 0u;
    if (c0 >= 2u && p0 + 1u < m.n_pix) r1 = ug_frame_row(p0 + 1u, m);      // (c0 + 3 >= 5: the quad reaches into the next pixel)
    uint32_t w[4];
#pragma unroll
    for (unsigned k = 0; k < 4u; ++k) {
      const bool next = c0 + k >= 5u;
      const unsigned row = next ? r1 : r0, c = next ? c0 + k - 5u : c0 + k;
      w[k] = (e0 + k < total && row < m.n_valid) ? ug_frame_word<ARRAYS>(row, c, gathered, rgb, depth, last) : 0u;
    }
    if (vec_store && e0 + 3u < total) {
      *reinterpret_cast<uint4 *>(out + e0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
      for (unsigned k = 0; k < 4u; ++k)
        if (e0 + k < total) out[e0 + k] = w[k];
    }
  }
}

template <bool ARRAYS>
static int ug_frame_launch(const float *gathered, const float *rgb, const float *depth, const float *last, const ug_frame_map &m,
                           float *out, ugrid_stream_t stream) {
  const int64_t n_quads = ((int64_t)m.n_pix * 5 + 3) / 4;
  unsigned blocks = ug_blocks(n_quads, UG_FR_THREADS);
  if (blocks > UG_FR_MAX_BLOCKS) blocks = UG_FR_MAX_BLOCKS;
  const int vec_store = ((uintptr_t)out & 15u) == 0;
  hipLaunchKernelGGL(k_frame_assemble<ARRAYS>, dim3(blocks), dim3(UG_FR_THREADS), 0, (hipStream_t)stream,
                     (const uint32_t *)gathered, (const uint32_t *)rgb, (const uint32_t *)depth, (const uint32_t *)last, m, vec_store,
                     (uint32_t *)out);
  UG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ugrid_frame_pack(const float *rgb, const float *depth, const float *last, int64_t n, int64_t per, float *out,
                                ugrid_stream_t stream) {
  if (n < 0 || per < n || !out || 5 * per > INT32_MAX) return (int)hipErrorInvalidValue;
  if (n > 0 && (!rgb || !depth || !last)) return (int)hipErrorInvalidValue;
  if (per == 0) return 0;
  ug_frame_map m = {};
  m.n_pix = (unsigned)per;
  m.n_valid = (unsigned)n;
  m.W = (unsigned)per;
  m.world = 1u;
  m.per = (unsigned)per;
  return ug_frame_launch<true>(nullptr, rgb, depth, last, m, out, stream);
}

// rays of rank 0 (the largest share) when the R rays' 64-ray tiles are dealt in groups of dg: the rows every rank's block must hold
static int64_t ug_frame_dealt_share(int64_t R, int64_t world, int64_t dg) {
  const int64_t n_tiles = (R + 63) / 64, n_groups = (n_tiles + dg - 1) / dg, c0 = (n_groups + world - 1) / world;
  const int64_t g_last = (c0 - 1) * world, b = g_last * dg * 64, e = (g_last + 1) * dg * 64;
  return (c0 - 1) * dg * 64 + ((e < R ? e : R) - b);
}

extern "C" int ugrid_frame_assemble(const float *gathered, const float *rgb, const float *depth, const float *last, int32_t H,
                                    int32_t W, int32_t world, int64_t per, int32_t deal_group, int32_t tile8, float *out,
                                    ugrid_stream_t stream) {
  if (H <= 0 || W <= 0 || !out) return (int)hipErrorInvalidValue;
  const int64_t R = (int64_t)H * W;
  if (5 * R > INT32_MAX) return (int)hipErrorInvalidValue;
  if (tile8 && ((H & 7) || (W & 7))) return (int)hipErrorInvalidValue;
  ug_frame_map m = {};
  m.n_pix = (unsigned)R;
  m.W = (unsigned)W;
  m.Wb = (unsigned)(W >> 3);
  m.tile8 = tile8 ? 1u : 0u;
  m.world = 1u;
  m.per = (unsigned)R;
  if (!gathered) {      // source B: the three arrays of a single-device render, row = ray position
    if (!rgb || !depth || !last) return (int)hipErrorInvalidValue;
    m.n_valid = (unsigned)R;
    return ug_frame_launch<true>(nullptr, rgb, depth, last, m, out, stream);
  }
  if (world < 1 || per < 1 || deal_group < 0 || 5 * (int64_t)world * per > INT32_MAX) return (int)hipErrorInvalidValue;
  // every computed row must lie inside the buffer: bands need world*per >= R, a deal needs per >= the largest (rank 0's) share
  if (deal_group == 0 ? (int64_t)world * per < R : per < ug_frame_dealt_share(R, world, deal_group)) return (int)hipErrorInvalidValue;
  m.world = (unsigned)world;
  m.per = (unsigned)per;
  m.dg = (unsigned)deal_group;
  m.n_valid = (unsigned)((int64_t)world * per);
  return ug_frame_launch<false>(gathered, nullptr, nullptr, nullptr, m, out, stream);
}
