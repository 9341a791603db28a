// libugrid_hip.so -- march half of the fused render path: brick packing, the k_march* kernels and their entry points.
// Built with -fno-slp-vectorize (see ugrid_render.h header note and csrc/build.sh).  The grid lookup of the training path is
// ugrid_query.hip, its sampling march ugrid_sample.hip.
#include "ugrid_render.h"

// ----------------------------------------------------------------------------------------------
// brick packing: canonical [P,C,X,Y,Z] -> [P*(X-1)(Y-1)(Z-1)] cell records of [H halves][8][CH]
// coef=1 (density and feature bricks): the 8 entries of a cell are the coefficients of its trilinear
// polynomial  f(tx,ty,tz) = sum_{dx,dy,dz} c[4dx+2dy+dz] tx^dx ty^dy tz^dz  (t = fractional cell coordinates),
// computed in fp64 from the 8 corner values and rounded once: the kernels evaluate a cell with 7 FMAs per
// channel and need no corner weights.  coef=0 (rgbnet-less colour bricks): the 8 corner values themselves.
// ----------------------------------------------------------------------------------------------
__global__ void k_pack_bricks(const float *__restrict__ grid, int P, int C, int X, int Y, int Z, int H,
                              int CH, int coef, float *__restrict__ out, int64_t total) {
  for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < total;
       o += (int64_t)gridDim.x * blockDim.x) {
    int64_t q = o;
    int ch, c;
    if (H == 2) {   // feature half-bricks: [pair CH/2][entry 8][2 channels]
      const int qi = (int)(q % (8 * CH)); q /= (8 * CH);
      c = (qi >> 1) & 7;
      ch = (qi >> 4) * 2 + (qi & 1);
    } else {        // density / rgbnet-less colour bricks: [entry 8][CH]
      ch = (int)(q % CH); q /= CH;
      c = (int)(q % 8); q /= 8;
    }
    const int h = (int)(q % H); q /= H;
    const int k = (int)(q % (Z - 1)); q /= (Z - 1);
    const int j = (int)(q % (Y - 1)); q /= (Y - 1);
    const int i = (int)(q % (X - 1)); q /= (X - 1);
    const int l = (int)q;
    const int chan = h * CH + ch;
    float v = 0.f;
    if (chan < C) {
      const float *g = grid + ((int64_t)l * C + chan) * X * Y * Z;
      if (!coef) {
        const int ii = i + (c >> 2), jj = j + ((c >> 1) & 1), kk = k + (c & 1);
        v = g[((int64_t)ii * Y + jj) * Z + kk];
      } else {
        // inclusion-exclusion over the corners s that are sub-masks of c
        double acc = 0.0;
        for (int s = 0; s < 8; ++s) {
          if (s & ~c) continue;
          const int ii = i + (s >> 2), jj = j + ((s >> 1) & 1), kk = k + (s & 1);
          const double t = (double)g[((int64_t)ii * Y + jj) * Z + kk];
          acc += (__popc(c ^ s) & 1) ? -t : t;
        }
        v = (float)acc;
      }
    }
    out[o] = v;
  }
}

// quad layout of the C == 12 feature bricks (ugrid_render.h "quad k0 gather"): [cell][q 0..5][g 0..3][4 floats]; lane g
// of a quad owns channels 3g..3g+2, float4 q holds coefficients 4(q&1)..4(q&1)+3 of channel 3g + (q>>1)
__global__ void k_pack_quad(const float *__restrict__ grid, int P, int C, int X, int Y, int Z, float *__restrict__ out,
                            int64_t total) {
  for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (int64_t)gridDim.x * blockDim.x) {
    const int e = (int)(o & 3), g = (int)((o >> 2) & 3);
    int64_t r = o >> 4;
    const int q = (int)(r % 6); r /= 6;
    const int k = (int)(r % (Z - 1)); r /= (Z - 1);
    const int j = (int)(r % (Y - 1)); r /= (Y - 1);
    const int i = (int)(r % (X - 1)); r /= (X - 1);
    const int l = (int)r;
    const int chan = 3 * g + (q >> 1), c = 4 * (q & 1) + e;
    const float *gp = grid + ((int64_t)l * C + chan) * X * Y * Z;
    double acc = 0.0;   // inclusion-exclusion over the corners s that are sub-masks of c (as k_pack_bricks)
    for (int s = 0; s < 8; ++s) {
      if (s & ~c) continue;
      const int ii = i + (s >> 2), jj = j + ((s >> 1) & 1), kk = k + (s & 1);
      const double t = (double)gp[((int64_t)ii * Y + jj) * Z + kk];
      acc += (__popc(c ^ s) & 1) ? -t : t;
    }
    out[o] = (float)acc;
  }
}

// block -> tile of the four march kernels (256 threads = 4 waves = 4 consecutive tiles, blocks spread over the XCDs by
// ug_xcd_remap): a wave that has a tile runs march(tile, ent, slot) -> the tile's survivor count on it and records the count
template <class MarchTile>
__device__ __forceinline__ void ug_march_block(const ug_ws_view &ws, int64_t nblocks, MarchTile march) {
  const int64_t blk = ug_xcd_remap(blockIdx.x, nblocks);
  if (blk >= nblocks) return;
  const int64_t tile = blk * 4 + (threadIdx.x >> 6);
  if (tile >= ws.n_tiles) return;
  const int n = march(tile, ws.ent + tile * ws.cap, ws.slot + tile * ws.cap);
  if (ug_lane() == 0) ws.count[tile] = n;
}

// launch geometry of the four march kernels: the work-list view, 4 tiles per block, the grid rounded up to the 8 XCDs
struct ug_march_geom { ug_ws_view ws; int64_t nblocks; dim3 grid; };
static inline ug_march_geom ug_march_geometry(void *ws_mem, int64_t n_rays, int32_t S) {
  ug_march_geom g;
  g.ws = ug_ws_make(ws_mem, n_rays, S);
  g.nblocks = (g.ws.n_tiles + 3) / 4;
  g.grid = dim3((unsigned)(((g.nblocks + 7) / 8) * 8));  // room for the XCD remap
  return g;
}

// W = 4..6 waves per SIMD: the level sum with the brick loads left to the compiler (ug_density_level).  (The body is not shared with
// k_march_ring through a helper: passing the arguments on changes the register allocation of these kernels throughout.)
template <int F, bool L2, int W>
__global__ void __launch_bounds__(256, W)
k_march(ug_march_args a, const float *__restrict__ rays_o, const float *__restrict__ rays_d,
        const float *__restrict__ t_table, const float *__restrict__ s_table,
        const float *__restrict__ bricks, float *__restrict__ alphainv_last, float *__restrict__ depth,
        ug_ws_view ws, int64_t nblocks) {
  ug_march_block(ws, nblocks, [&](int64_t tile, float4 *ent, uint8_t *slot) {
    if constexpr (ug_march_ring<W>::value) {   // (A/B builds with the ring at 6 waves only: as k_march_ring below)
      tile = ug_wave_uniform(tile);
      ent = ws.ent + tile * ws.cap;
      slot = ws.slot + tile * ws.cap;
    }
    return ug_march_tile<F, L2, false, W>(a, rays_o, rays_d, t_table, s_table, bricks, alphainv_last, depth, tile, ent, slot);
  });
}

// W = 7 | 8: the same march with the level sum as a hand-pipelined ring of brick loads (ug_density_ring); a kernel of its own name,
// with its own register caps (72 / 64, no scratch: tests/test_march_ring_budget.py)
template <int F, bool L2, int W>
__global__ void __launch_bounds__(256, W)
k_march_ring(ug_march_args a, const float *__restrict__ rays_o, const float *__restrict__ rays_d,
             const float *__restrict__ t_table, const float *__restrict__ s_table,
             const float *__restrict__ bricks, float *__restrict__ alphainv_last, float *__restrict__ depth,
             ug_ws_view ws, int64_t nblocks) {
  static_assert(W == 7 || W == 8, "the ring is built for 7 and 8 waves per SIMD");
  ug_march_block(ws, nblocks, [&](int64_t tile, float4 *ent, uint8_t *slot) {
    // a wave owns a tile: say so, and the tile's list pointers (4 VGPRs) live in scalar registers
    tile = ug_wave_uniform(tile);
    ent = ws.ent + tile * ws.cap;
    slot = ws.slot + tile * ws.cap;
    return ug_march_tile<F, L2, false, W>(a, rays_o, rays_d, t_table, s_table, bricks, alphainv_last, depth, tile, ent, slot);
  });
}


// DirectContractedVoxGO march (single-level grids: F = 0): k_march + the cumdist_thres rule + the mask cache + wsum_mid
template <bool L2>
__global__ void __launch_bounds__(256, 5)
k_march_dcvgo(ug_march_args a, ug_dc_args dc, const float *__restrict__ rays_o, const float *__restrict__ rays_d,
              const float *__restrict__ t_table, const float *__restrict__ s_table, const float *__restrict__ bricks,
              float *__restrict__ alphainv_last, float *__restrict__ depth, float *__restrict__ wsum_mid, ug_ws_view ws,
              int64_t nblocks) {
  ug_march_block(ws, nblocks, [&](int64_t tile, float4 *ent, uint8_t *slot) {
    return ug_march_tile<0, L2, true>(a, rays_o, rays_d, t_table, s_table, bricks, alphainv_last, depth, tile, ent, slot, dc, wsum_mid);
  });
}

// bounded DirectVoxGO march (ug_march_tile_dvgo): variable-length rays clipped against the scene box
__global__ void __launch_bounds__(256, 6)
k_march_dvgo(ug_march_args a, ug_dv_args dv, const float *__restrict__ rays_o, const float *__restrict__ rays_d,
             const float *__restrict__ bricks, float *__restrict__ alphainv_last, float *__restrict__ depth, ug_ws_view ws,
             int64_t nblocks) {
  ug_march_block(ws, nblocks, [&](int64_t tile, float4 *ent, uint8_t *slot) {
    return ug_march_tile_dvgo(a, dv, rays_o, rays_d, bricks, alphainv_last, depth, tile, ent, slot, a.S);
  });
}

// forward-facing DirectMPIGO march (ug_march_tile_mpi): NDC rays, n samples each; act_shift [D <= 256] staged in LDS
__global__ void __launch_bounds__(256, 6)
k_march_mpi(ug_march_args a, ug_mpi_args mp, const float *__restrict__ rays_o, const float *__restrict__ rays_d,
            const float *__restrict__ bricks, const float *__restrict__ act_shift, float *__restrict__ alphainv_last,
            float *__restrict__ depth, ug_ws_view ws, int64_t nblocks) {
  __shared__ float shift[256];
  if ((int)threadIdx.x < mp.D) shift[threadIdx.x] = act_shift[threadIdx.x];
  __syncthreads();
  ug_march_block(ws, nblocks, [&](int64_t tile, float4 *ent, uint8_t *slot) {
    return ug_march_tile_mpi(a, mp, rays_o, rays_d, bricks, shift, alphainv_last, depth, tile, ent, slot);
  });
}

// ----------------------------------------------------------------------------------------------
// C ABI
// ----------------------------------------------------------------------------------------------
extern "C" int64_t ugrid_render_ws_bytes(int64_t n_rays, int32_t S) {
  const int64_t n_tiles = (n_rays + UG_WAVE - 1) / UG_WAVE, cap = (int64_t)UG_WAVE * S;
  return 256 + ug_align256(n_tiles * 4) + ug_align256(n_tiles * cap * 16) + ug_align256(n_tiles * cap);
}

static inline int ug_brick_ch(int C, int *H) {
  // density (C==1): 1 half x 1 channel; rgbnet-less k0 (C==3 handled by caller via halves=1, CH=4);
  // feature grids: 2 halves x ceil(C/2)
  if (C == 1) { *H = 1; return 1; }
  *H = 2;
  return UG_CH(C);
}

extern "C" int64_t ugrid_brick_bytes(int P, int C, int X, int Y, int Z, int direct) {
  int H, CH = ug_brick_ch(C, &H);
  if (direct) { H = 1; CH = 4; }
  return (int64_t)P * (X - 1) * (Y - 1) * (Z - 1) * H * 8 * CH * (int64_t)sizeof(float);
}

extern "C" int ugrid_pack_bricks(const float *grid, int P, int C, int X, int Y, int Z, int direct,
                                 float *bricks, ugrid_stream_t s) {
  if (X < 2 || Y < 2 || Z < 2 || P < 1 || C < 1) return (int)hipErrorInvalidValue;
  int H, CH = ug_brick_ch(C, &H);
  if (direct) { H = 1; CH = 4; }
  const int64_t total = (int64_t)P * (X - 1) * (Y - 1) * (Z - 1) * H * 8 * CH;
  int64_t blocks = (total + 255) / 256;
  if (blocks > 256 * 64) blocks = 256 * 64;
  if (C == 12 && !direct) {   // 384 B per cell in the quad layout (same size as two 192-byte halves)
    // multi-level grids are addressed with 32-bit byte offsets inside a level; a single-level grid (P == 1) with 64-bit ones
    if (P > 1 && (int64_t)(X - 1) * (Y - 1) * (Z - 1) * 384 >= ((int64_t)1 << 32)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pack_quad, dim3((unsigned)blocks), dim3(256), 0, ST(s), grid, P, C, X, Y, Z, bricks, total);
    UG_LAUNCH_CHECK();
    return 0;
  }
  int coef = direct ? 0 : 1;
  hipLaunchKernelGGL(k_pack_bricks, dim3((unsigned)blocks), dim3(256), 0, ST(s), grid, P, C, X, Y, Z, H, CH,
                     coef, bricks, total);
  UG_LAUNCH_CHECK();
  return 0;
}

// min waves/SIMD the march kernel is compiled for (register cap 512/W): 4..6 = the level sum as plain C++ loads (ug_density_level),
// 7 | 8 = ug_density_ring, three levels in flight behind hand-placed vmcnt waits; 0 = back to the default
#define UG_MARCH_WAVES_DEFAULT 8
static int g_march_waves = UG_MARCH_WAVES_DEFAULT;
extern "C" int ug_set_march_waves(int w) {
  if (w == 0) w = UG_MARCH_WAVES_DEFAULT;
  if (w < 4 || w > 8) return 1;
  g_march_waves = w;
  return 0;
}

template <int F, int W>
static int ug_march_launch_w(const ugrid_render_params *p, const ug_march_args &a, const float *rays_o,
                             const float *rays_d, const float *t_table, const float *s_table,
                             const float *bricks, float *alphainv_last, float *depth, const ug_march_geom &g,
                             hipStream_t st) {
  if constexpr (W >= 7) {
    if (p->norm_l2)
      hipLaunchKernelGGL(HIP_KERNEL_NAME(k_march_ring<F, true, W>), g.grid, dim3(256), 0, st, a, rays_o,
                         rays_d, t_table, s_table, bricks, alphainv_last, depth, g.ws, g.nblocks);
    else
      hipLaunchKernelGGL(HIP_KERNEL_NAME(k_march_ring<F, false, W>), g.grid, dim3(256), 0, st, a, rays_o,
                         rays_d, t_table, s_table, bricks, alphainv_last, depth, g.ws, g.nblocks);
  } else {
    if (p->norm_l2)
      hipLaunchKernelGGL(HIP_KERNEL_NAME(k_march<F, true, W>), g.grid, dim3(256), 0, st, a, rays_o,
                         rays_d, t_table, s_table, bricks, alphainv_last, depth, g.ws, g.nblocks);
    else
      hipLaunchKernelGGL(HIP_KERNEL_NAME(k_march<F, false, W>), g.grid, dim3(256), 0, st, a, rays_o,
                         rays_d, t_table, s_table, bricks, alphainv_last, depth, g.ws, g.nblocks);
  }
  UG_LAUNCH_CHECK();
  return 0;
}

template <int F>
static int ug_march_launch(const ugrid_render_params *p, const ug_march_args &a, const float *rays_o,
                           const float *rays_d, const float *t_table, const float *s_table,
                           const float *bricks, float *alphainv_last, float *depth, const ug_march_geom &g,
                           hipStream_t st) {
  switch (g_march_waves) {
    case 4: return ug_march_launch_w<F, 4>(p, a, rays_o, rays_d, t_table, s_table, bricks, alphainv_last, depth, g, st);
    case 6: return ug_march_launch_w<F, 6>(p, a, rays_o, rays_d, t_table, s_table, bricks, alphainv_last, depth, g, st);
    case 7: return ug_march_launch_w<F, 7>(p, a, rays_o, rays_d, t_table, s_table, bricks, alphainv_last, depth, g, st);
    case 8: return ug_march_launch_w<F, 8>(p, a, rays_o, rays_d, t_table, s_table, bricks, alphainv_last, depth, g, st);
    default: return ug_march_launch_w<F, 5>(p, a, rays_o, rays_d, t_table, s_table, bricks, alphainv_last, depth, g, st);
  }
}

extern "C" int ugrid_render_march(const ugrid_render_params *p, const float *rays_o, const float *rays_d,
                                  const float *t_table, const float *s_table, const float *density_bricks,
                                  float *alphainv_last, float *depth, void *ws_mem, ugrid_stream_t s) {
  if (p->n_rays <= 0) return 0;
  ug_march_args a;
  const int rc = ug_fill_march_args(p, a);
  if (rc) return rc;
  const ug_march_geom g = ug_march_geometry(ws_mem, p->n_rays, p->n_samples);
  switch (p->freq_num) {
    case 1: return ug_march_launch<1>(p, a, rays_o, rays_d, t_table, s_table, density_bricks, alphainv_last, depth, g, ST(s));
    case 2: return ug_march_launch<2>(p, a, rays_o, rays_d, t_table, s_table, density_bricks, alphainv_last, depth, g, ST(s));
    case 3: return ug_march_launch<3>(p, a, rays_o, rays_d, t_table, s_table, density_bricks, alphainv_last, depth, g, ST(s));
    case 4: return ug_march_launch<4>(p, a, rays_o, rays_d, t_table, s_table, density_bricks, alphainv_last, depth, g, ST(s));
    case 5: return ug_march_launch<5>(p, a, rays_o, rays_d, t_table, s_table, density_bricks, alphainv_last, depth, g, ST(s));
    default: return (int)hipErrorInvalidValue;
  }
}


extern "C" int ugrid_render_march_dcvgo(const ugrid_render_params *p, const ugrid_dcvgo_params *q, const float *rays_o,
                                        const float *rays_d, const float *t_table, const float *s_table,
                                        const float *density_bricks, float *alphainv_last, float *depth, float *wsum_mid,
                                        void *ws_mem, ugrid_stream_t s) {
  if (p->n_rays <= 0) return 0;
  if (p->freq_num != 0 || !q) return (int)hipErrorInvalidValue;
  ug_march_args a;
  ug_dc_args dc;
  int rc = ug_fill_mask_args(dc, q->mask, q->mask_x, q->mask_y, q->mask_z, q->xyz2ijk_scale, q->xyz2ijk_shift);
  if (!rc) rc = ug_fill_march_args(p, a);
  if (rc) return rc;
  dc.dist_thres = q->dist_thres;
  const ug_march_geom g = ug_march_geometry(ws_mem, p->n_rays, p->n_samples);
  if (p->norm_l2)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_march_dcvgo<true>), g.grid, dim3(256), 0, ST(s), a, dc, rays_o, rays_d, t_table,
                       s_table, density_bricks, alphainv_last, depth, wsum_mid, g.ws, g.nblocks);
  else
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_march_dcvgo<false>), g.grid, dim3(256), 0, ST(s), a, dc, rays_o, rays_d, t_table,
                       s_table, density_bricks, alphainv_last, depth, wsum_mid, g.ws, g.nblocks);
  UG_LAUNCH_CHECK();
  return 0;
}


extern "C" int ugrid_render_march_dvgo(const ugrid_render_params *p, const ugrid_dvgo_params *q, const float *rays_o,
                                       const float *rays_d, const float *density_bricks, float *alphainv_last, float *depth,
                                       void *ws_mem, ugrid_stream_t s) {
  if (p->n_rays <= 0) return 0;
  if (p->freq_num != 0 || !q || !(q->stepdist > 0.f)) return (int)hipErrorInvalidValue;
  ug_march_args a;
  ug_dv_args dv;
  int rc = ug_fill_mask_args(dv, q->mask, q->mask_x, q->mask_y, q->mask_z, q->xyz2ijk_scale, q->xyz2ijk_shift);
  if (!rc) rc = ug_fill_march_args(p, a);
  if (rc) return rc;
  dv.near = q->near_clip; dv.far = q->far_clip; dv.stepdist = q->stepdist;
  const ug_march_geom g = ug_march_geometry(ws_mem, p->n_rays, p->n_samples);
  hipLaunchKernelGGL(k_march_dvgo, g.grid, dim3(256), 0, ST(s), a, dv, rays_o, rays_d, density_bricks, alphainv_last,
                     depth, g.ws, g.nblocks);
  UG_LAUNCH_CHECK();
  return 0;
}



extern "C" int ugrid_render_march_mpi(const ugrid_render_params *p, const ugrid_mpi_params *q, const float *rays_o,
                                      const float *rays_d, const float *density_bricks, const float *act_shift, float *alphainv_last,
                                      float *depth, void *ws_mem, ugrid_stream_t s) {
  if (p->n_rays <= 0) return 0;
  if (p->freq_num != 0 || !q || !act_shift) return (int)hipErrorInvalidValue;
  // the LDS table holds 256 planes; a lane's samples fill at most n_samples entries of its tile's survivor list
  if (q->mpi_depth < 2 || q->mpi_depth > 256 || q->n_steps < 2 || q->n_steps > p->n_samples) return (int)hipErrorInvalidValue;
  ug_march_args a;
  ug_mpi_args mp;
  int rc = ug_fill_mask_args(mp, q->mask, q->mask_x, q->mask_y, q->mask_z, q->xyz2ijk_scale, q->xyz2ijk_shift);
  if (!rc) rc = ug_fill_march_args(p, a);
  if (rc) return rc;
  mp.D = q->mpi_depth; mp.n = q->n_steps;
  const ug_march_geom g = ug_march_geometry(ws_mem, p->n_rays, p->n_samples);
  hipLaunchKernelGGL(k_march_mpi, g.grid, dim3(256), 0, ST(s), a, mp, rays_o, rays_d, density_bricks, act_shift,
                     alphainv_last, depth, g.ws, g.nblocks);
  UG_LAUNCH_CHECK();
  return 0;
}
