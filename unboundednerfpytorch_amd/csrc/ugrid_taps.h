// ugrid_taps.h -- the trilinear corner taps and the Fourier level coordinates of a lookup on the CANONICAL grid layout (the parameter
// being trained, not the packed bricks of the render path): one definition for the grid query and its backward (ugrid_query.hip)
// and the training sampling march (ugrid_sample.hip), whose densities must be bit-identical to the query's.
#pragma once
#include "ugrid_common.h"
#include "ugrid_math.h"

// generic zero-padded trilinear tap at normalised (cx->X axis, cy->Y, cz->Z): the 8 corner offsets inside one
// [X,Y,Z] plane (-1 = outside the grid, zero padding) and their weights, in grid_sample's corner order
struct ug_taps { int64_t off[8]; float w[8]; };
__device__ __forceinline__ ug_taps ug_tap_setup(int X, int Y, int Z, float cx, float cy, float cz) {
  const float ix = ((cx + 1.f) / 2.f) * (float)(X - 1);
  const float iy = ((cy + 1.f) / 2.f) * (float)(Y - 1);
  const float iz = ((cz + 1.f) / 2.f) * (float)(Z - 1);
  const float fx = floorf(ix), fy = floorf(iy), fz = floorf(iz);
  const float wx0 = (fx + 1.f) - ix, wx1 = ix - fx;
  const float wy0 = (fy + 1.f) - iy, wy1 = iy - fy;
  const float wz0 = (fz + 1.f) - iz, wz1 = iz - fz;
  const int x0 = (int)fminf(fmaxf(fx, -2.f), (float)X), y0 = (int)fminf(fmaxf(fy, -2.f), (float)Y),
            z0 = (int)fminf(fmaxf(fz, -2.f), (float)Z);
  ug_taps t;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int xi = x0 + (c >> 2), yi = y0 + ((c >> 1) & 1), zi = z0 + (c & 1);
    const bool in = xi >= 0 && xi < X && yi >= 0 && yi < Y && zi >= 0 && zi < Z;
    t.off[c] = in ? ((int64_t)xi * Y + yi) * Z + zi : -1;
    t.w[c] = ((c & 1) ? wz1 : wz0) * (((c >> 1) & 1) ? wy1 : wy0) * ((c >> 2) ? wx1 : wx0);
  }
  return t;
}

// The same taps for kernels that LOAD the corners: every offset is valid (a corner outside the grid is clamped, per axis, onto the cell's
// in-range corner) and its weight is 0 -- `acc += g[off] * w` then runs without a branch and adds an exact zero where grid_sample pads.
// With `if (off >= 0) acc += g[off] * w` every load sat under its own exec branch and hipcc put s_waitcnt vmcnt(0) behind each: the eight
// corners of a level fetched ONE AFTER THE OTHER (round 6, visit P; S3's sampling march 0.64 ms).  Bit-identical: x + 0 = x, and the
// clamped corner is one the sample reads anyway (a NaN there reaches the result in both forms).
__device__ __forceinline__ ug_taps ug_tap_setup_ld(int X, int Y, int Z, float cx, float cy, float cz) {
  const float ix = ((cx + 1.f) / 2.f) * (float)(X - 1);
  const float iy = ((cy + 1.f) / 2.f) * (float)(Y - 1);
  const float iz = ((cz + 1.f) / 2.f) * (float)(Z - 1);
  const float fx = floorf(ix), fy = floorf(iy), fz = floorf(iz);
  const float wx0 = (fx + 1.f) - ix, wx1 = ix - fx;
  const float wy0 = (fy + 1.f) - iy, wy1 = iy - fy;
  const float wz0 = (fz + 1.f) - iz, wz1 = iz - fz;
  const int x0 = (int)fminf(fmaxf(fx, -2.f), (float)X), y0 = (int)fminf(fmaxf(fy, -2.f), (float)Y),
            z0 = (int)fminf(fmaxf(fz, -2.f), (float)Z);
  ug_taps t;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int xi = x0 + (c >> 2), yi = y0 + ((c >> 1) & 1), zi = z0 + (c & 1);
    const bool in = xi >= 0 && xi < X && yi >= 0 && yi < Y && zi >= 0 && zi < Z;
    const int xc = min(max(xi, 0), X - 1), yc = min(max(yi, 0), Y - 1), zc = min(max(zi, 0), Z - 1);
    t.off[c] = ((int64_t)xc * Y + yc) * Z + zc;
    const float w = ((c & 1) ? wz1 : wz0) * (((c >> 1) & 1) ? wy1 : wy0) * ((c >> 2) ? wx1 : wx0);
    t.w[c] = in ? w : 0.f;
  }
  return t;
}

// level coordinates of the Fourier grid: l = 0 plain, odd l = sin(2^k u), even l = cos(2^k u), k = (l-1)/2
__device__ __forceinline__ void ug_level_coords(int l, float ux, float uy, float uz, float &cx, float &cy, float &cz) {
  cx = ux; cy = uy; cz = uz;
  if (l > 0) {
    // ug_sincos (ugrid_math.h): 1.2e-7 max abs error for |x| <= 4, i.e. within an ulp of libm's results at a
    // seventh of the instructions of ocml sinf / cosf
    const float f = (float)(1 << ((l - 1) >> 1));
    float sx, kx, sy, ky, sz, kz;
    ug_sincos(f * ux, &sx, &kx);
    ug_sincos(f * uy, &sy, &ky);
    ug_sincos(f * uz, &sz, &kz);
    const bool is_cos = (l - 1) & 1;
    cx = is_cos ? kx : sx; cy = is_cos ? ky : sy; cz = is_cos ? kz : sz;
  }
}
