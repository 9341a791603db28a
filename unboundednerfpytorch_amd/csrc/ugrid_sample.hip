// libugrid_hip.so -- the sampling march of the training path: k_train_march (Fourier grids), k_train_march_vox / _tensorf (the three
// dense-grid models), the compactions, the backward of stage 2, and the ugrid_train_* entry points.
// Built with -fno-slp-vectorize like the march these kernels were split from (csrc/build.sh).
#include "ugrid_render.h"
#include "ugrid_taps.h"
#include "ugrid_tensorf.h"

// ----------------------------------------------------------------------------------------------
// Training forward, stage 1 (new entry points; replace the head of FourierGridModel.forward in training mode,
// FourierGrid_model.py:554-598: sample_ray -> [R,S,3] points, density lookup on all R*S points, Raw2Alpha, the
// `alpha > fast_color_thres` mask and seven boolean-index gathers with their host syncs).
//   k_train_march   one wave per ray, lane = sample (S/64 rounds): point, contraction, P-level density on the CANONICAL
//                   layout (the parameter being trained; same device functions and operation order as k_grid_query,
//                   so the densities are bit-identical to the composed path), alpha exactly as k_raw2alpha forms it,
//                   threshold, ballot + mbcnt compaction into the ray's private slot [r*S, r*S + count[r]) of a scratch
//   k_train_compact after a cumsum of the counts: one wave per ray copies its slot to the ray-major compact outputs
// The point arithmetic follows the torch elementwise chain of sample_ray (separate multiply / add, IEEE divisions).
// ----------------------------------------------------------------------------------------------
struct ug_train_args {
  int64_t n_rays;
  int32_t S, P, F, X, Y, Z, norm_l2;
  float cx, cy, cz, rx, ry, rz;
  float B, A;
  float shift, interval, thres;
};

// MODE 1 / 2 of k_train_march: the sampling rules of the reference's two non-Fourier models (single-level dense grids)
//   1 = DirectContractedVoxGO (dcvgo.py:228-310): the FourierGrid point rule + of the contracted samples only those whose running
//       inter-sample distance has just exceeded dist_thres (cumdist_thres, ub360_utils_kernel.cu:13-33: a serial recurrence
//       along the ray -- here a readlane loop over the wave's 64 samples with a wave-uniform carry) + the mask cache
//       (maskcache_lookup, render_utils_kernel.cu:374-392); the step id of a contracted sample is stored complemented
//       (inner_mask of dcvgo.py:262 travels in the sign)
//   2 = DirectVoxGO (dvgo.py:306-400): per-ray box clipping and step count (infer_t_minmax / infer_n_samples /
//       sample_pts_on_rays, render_utils_kernel.cu:16-57,100-260), mask_outbbox, the mask cache; a.S = slots per ray (>= the
//       longest possible ray: the host sizes it for the box diagonal), t_table unused
//   3 = DirectMPIGO (dmpigo.py:224-292): NDC rays, every ray takes the same a.S samples p = o + d * (j / (S-1)) with the direction NOT
//       normalised (sample_ndc_pts_on_rays, render_utils_kernel.cu:245-270; the arithmetic of ug_march_tile_mpi), mask_outbbox, the
//       mask cache; density = the grid lookup + the per-plane shift, a lerp along z of the D-entry table `plane_shift` (DEVICE memory:
//       the act_shift grid itself, no host copy), the two added in fp32 like `self.density(p) + self.act_shift(p)`.  s_dens keeps
//       the SUM and a.shift is 0, so the compaction and k_train_sample_bwd recompute the same exp; t_table unused
struct ug_train_vox : ug_mask_args {      // the mask cache: ug_mask_lookup (ugrid_render.h), shared with the render march
  float dist_thres;                 // mode 1
  float near, far, stepdist;        // mode 2
  const float *plane_shift;         // mode 3: [D]
  int32_t D;                        // mode 3: mpi_depth
};

// sample t of a normalised ray, contracted outside the unit cube / ball (dcvgo.py:251-262, the arithmetic of k_train_march);
// returns the norm before the contraction
__device__ __forceinline__ float ug_train_point(const ug_train_args &a, float ox, float oy, float oz, float dx, float dy, float dz,
                                                float t, float &px, float &py, float &pz) {
  px = ox + dx * t; py = oy + dy * t; pz = oz + dz * t;
  const float nrm = a.norm_l2 ? ug_norm3_torch(px, py, pz) : fmaxf(fabsf(px), fmaxf(fabsf(py), fabsf(pz)));
  if (!(nrm <= 1.0f)) {
    // `bg_len / norm` with a Python number on the left is torch's Tensor.__rtruediv__ = reciprocal(norm) * bg_len: two roundings
    const float sc = a.B - (1.0f / nrm) * a.A;
    px = px / nrm * sc; py = py / nrm * sc; pz = pz / nrm * sc;
  }
  return nrm;
}

// alpha of a raw density exactly as k_raw2alpha forms it (e = expf(density + shift) is what its backward keeps)
__device__ __forceinline__ float ug_train_alpha(float dens, float shift, float interval, float *e_out) {
  const float e = expf(dens + shift);
  *e_out = e;
  return 1 - powf(1 + e, -interval);
}

// W2 = true (ugrid_train_sample): ALSO stage 2 of the sampling -- the transmittance recurrence of Alphas2Weights over the
// kept samples, in order, exactly as k_alpha2weight runs it (T in float, the product in double, early stop below 1e-3),
// the weight threshold, alphainv_last -- and the march of a ray ENDS where its transmittance does (the reference looks up
// all S samples and throws the tail away: weight 0, gradient 0).  s_w / s_T: weight and transmittance per kept sample,
// count2: kept samples whose weight exceeds the threshold.
template <bool W2>
__global__ void __launch_bounds__(256)
k_train_march(ug_train_args a, const float *__restrict__ grid, const float *__restrict__ rays_o,
              const float *__restrict__ rays_d, const float *__restrict__ t_table, const float *__restrict__ xyz_min,
              const float *__restrict__ xyz_max, float *__restrict__ s_pts, float *__restrict__ s_dens,
              int32_t *__restrict__ s_step, int32_t *__restrict__ count, float *__restrict__ s_w, float *__restrict__ s_T,
              int32_t *__restrict__ count2, float *__restrict__ alphainv_last) {
  const int64_t ray = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (ray >= a.n_rays) return;
  const int lane = ug_lane();
  const float ox = (rays_o[3 * ray] - a.cx) / a.rx, oy = (rays_o[3 * ray + 1] - a.cy) / a.ry, oz = (rays_o[3 * ray + 2] - a.cz) / a.rz;
  const float rdx = rays_d[3 * ray], rdy = rays_d[3 * ray + 1], rdz = rays_d[3 * ray + 2];
  const float dn = ug_norm3_torch(rdx, rdy, rdz);
  const float dx = rdx / dn, dy = rdy / dn, dz = rdz / dn;
  const float lox = xyz_min[0], loy = xyz_min[1], loz = xyz_min[2], hix = xyz_max[0], hiy = xyz_max[1], hiz = xyz_max[2];
  const int64_t vol = (int64_t)a.X * a.Y * a.Z;
  const int64_t slot = ray * a.S;
  int kept = 0, kept2 = 0;   // wave-uniform
  float T_cum = 1.f;         // wave-uniform
  bool stopped = false;
  for (int j0 = 0; j0 < a.S && !stopped; j0 += UG_WAVE) {
    const int j = j0 + lane;
    bool keep = false;
    float px = 0.f, py = 0.f, pz = 0.f, dens = 0.f, alpha = 0.f;
    if (j < a.S) {
      const float t = t_table[j];
      px = ox + dx * t; py = oy + dy * t; pz = oz + dz * t;
      const float nrm = a.norm_l2 ? ug_norm3_torch(px, py, pz) : fmaxf(fabsf(px), fmaxf(fabsf(py), fabsf(pz)));
      if (!(nrm <= 1.0f)) {
        const float sc = a.B - (1.0f / nrm) * a.A;      // `A / norm` = reciprocal(norm) * A in torch (ug_contract)
        px = px / nrm * sc; py = py / nrm * sc; pz = pz / nrm * sc;
      }
      const float ux = ug_unorm(px, lox, hix), uy = ug_unorm(py, loy, hiy), uz = ug_unorm(pz, loz, hiz);
      auto level = [&](int l, float cx, float cy, float cz) -> float {
        const ug_taps tp = ug_tap_setup_ld(a.X, a.Y, a.Z, cx, cy, cz);
        const float *__restrict__ g = grid + (int64_t)l * vol;
        float acc = 0.f;
#pragma unroll
        for (int c = 0; c < 8; ++c) acc += g[tp.off[c]] * tp.w[c];
        return acc;
      };
      // as k_grid_query: level 0, then the sin and the cos level of a frequency together (one sin / cos evaluation for both, 16 corner
      // loads in flight), sums added in level order: the densities stay bit-identical to the composed path's
      dens = level(0, ux, uy, uz);
      for (int k = 0; 2 * k + 2 < a.P; ++k) {
        const float f = (float)(1 << k);
        float sx, kx, sy, ky, sz, kz;
        ug_sincos(f * ux, &sx, &kx);
        ug_sincos(f * uy, &sy, &ky);
        ug_sincos(f * uz, &sz, &kz);
        const ug_taps ts = ug_tap_setup_ld(a.X, a.Y, a.Z, sx, sy, sz), tc = ug_tap_setup_ld(a.X, a.Y, a.Z, kx, ky, kz);
        const float *__restrict__ gs = grid + (int64_t)(2 * k + 1) * vol, *__restrict__ gc = grid + (int64_t)(2 * k + 2) * vol;
        float vs[8], vc[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) vs[c] = gs[ts.off[c]];
#pragma unroll
        for (int c = 0; c < 8; ++c) vc[c] = gc[tc.off[c]];
        float as = 0.f, ac = 0.f;
#pragma unroll
        for (int c = 0; c < 8; ++c) as += vs[c] * ts.w[c];
#pragma unroll
        for (int c = 0; c < 8; ++c) ac += vc[c] * tc.w[c];
        dens = dens + as;
        dens = dens + ac;
      }
      if (a.F > 0) dens = dens / (float)a.P;
      float e;
      alpha = ug_train_alpha(dens, a.shift, a.interval, &e);
      keep = alpha > a.thres;
    }
    unsigned long long m = __ballot(keep);
    float myT = 1.f, myW = 0.f;
    if (W2) {
      unsigned long long mm = m;
      while (mm != 0ull) {
        const int k = __builtin_ctzll(mm);
        mm &= mm - 1ull;
        const float ak = ug_readlane_f(alpha, k);
        if (lane == k) {
          myT = T_cum;
          myW = T_cum * ak;
        }
        T_cum = (float)((double)T_cum * (1. - (double)ak));
        if ((double)T_cum < 1e-3) {          // the sample that crosses keeps its weight; the ray ends here
          stopped = true;
          m &= (2ull << k) - 1ull;
          keep = keep && lane <= k;
          break;
        }
      }
    }
    if (m != 0ull) {
      if (keep) {
        const int64_t idx = slot + kept + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        s_pts[3 * idx] = px; s_pts[3 * idx + 1] = py; s_pts[3 * idx + 2] = pz;
        s_dens[idx] = dens;
        s_step[idx] = j;
        if (W2) { s_w[idx] = myW; s_T[idx] = myT; }
      }
      kept += __popcll(m);
      if (W2) kept2 += __popcll(__ballot(keep && myW > a.thres));
    }
  }
  if (lane == 0) {
    count[ray] = kept;
    if (W2) { count2[ray] = kept2; alphainv_last[ray] = T_cum; }
  }
}

// The density source of the march below: the eight corners of a dense [X,Y,Z] grid, or the six factors of a TensoRF grid
// (ugrid_tensorf.h: tf_density, the function k_tensorf_query calls -- 3 groups x Rg components x (4 plane + 2 vector) loads).
struct ug_dens_dense { const float *__restrict__ grid; };
template <bool CL> struct ug_dens_tensorf { const tf_factors &f; };
__device__ __forceinline__ float ug_train_density(const ug_train_args &a, const ug_dens_dense &s, float ux, float uy, float uz) {
  const ug_taps tp = ug_tap_setup_ld(a.X, a.Y, a.Z, ux, uy, uz);
  float acc = 0.f;
#pragma unroll
  for (int c = 0; c < 8; ++c) acc += s.grid[tp.off[c]] * tp.w[c];
  return acc;
}
template <bool CL>
__device__ __forceinline__ float ug_train_density(const ug_train_args &, const ug_dens_tensorf<CL> &s, float ux, float uy, float uz) {
  return tf_density<CL>(s.f, ux, uy, uz);
}

// k_train_march<true> for the dense-grid models (ug_train_vox above): MODE 1 = DirectContractedVoxGO, 2 = DirectVoxGO, 3 = DirectMPIGO.
// Same slot / scratch contract and the same stage-2 recurrence; P = 1, F = 0.  One body for both density sources (DENS): the kernels
// below only name their arguments.  No workgroup barrier and no LDS: waves past n_rays return at the top and leave the loop on their own.
template <int MODE, class DENS>
__device__ __forceinline__ void
ug_train_march_vox(const ug_train_args &a, const ug_train_vox &v, const DENS &src, const float *__restrict__ rays_o,
                   const float *__restrict__ rays_d, const float *__restrict__ t_table, const float *__restrict__ xyz_min,
                   const float *__restrict__ xyz_max, float *__restrict__ s_pts, float *__restrict__ s_dens,
                   int32_t *__restrict__ s_step, int32_t *__restrict__ count, float *__restrict__ s_w, float *__restrict__ s_T,
                   int32_t *__restrict__ count2, float *__restrict__ alphainv_last) {
  const int64_t ray = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (ray >= a.n_rays) return;
  const int lane = ug_lane();
  const float lox = xyz_min[0], loy = xyz_min[1], loz = xyz_min[2], hix = xyz_max[0], hiy = xyz_max[1], hiz = xyz_max[2];
  const float rox = rays_o[3 * ray], roy = rays_o[3 * ray + 1], roz = rays_o[3 * ray + 2];
  const float rdx = rays_d[3 * ray], rdy = rays_d[3 * ray + 1], rdz = rays_d[3 * ray + 2];
  float ox, oy, oz, dx, dy, dz;
  int n = a.S;               // samples of this ray (wave-uniform)
  if (MODE == 1) {
    ox = (rox - a.cx) / a.rx; oy = (roy - a.cy) / a.ry; oz = (roz - a.cz) / a.rz;
    const float dn = ug_norm3_torch(rdx, rdy, rdz);
    dx = rdx / dn; dy = rdy / dn; dz = rdz / dn;
  } else if (MODE == 3) {
    ox = rox; oy = roy; oz = roz;
    dx = rdx; dy = rdy; dz = rdz;
  } else {
    // ray / box slab test; a zero direction component is replaced by float(1e-6) (infer_t_minmax)
    const float vx = (rdx == 0.f) ? (float)1e-6 : rdx, vy = (rdy == 0.f) ? (float)1e-6 : rdy, vz = (rdz == 0.f) ? (float)1e-6 : rdz;
    const float ax = (hix - rox) / vx, ay = (hiy - roy) / vy, az = (hiz - roz) / vz;
    const float bx = (lox - rox) / vx, by = (loy - roy) / vy, bz = (loz - roz) / vz;
    const float tmin = fmaxf(fminf(fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fminf(az, bz)), v.far), v.near);
    const float tmax = fmaxf(fminf(fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz)), v.far), v.near);
    const float rn = sqrtf(rdx * rdx + rdy * rdy + rdz * rdz);
    const double c = (double)ceilf((tmax - tmin) * rn / v.stepdist);        // infer_n_samples
    const double nn = c > 1. ? c : 1.;
    n = nn > (double)a.S ? a.S : (int)nn;
    ox = rox + rdx * tmin; oy = roy + rdy * tmin; oz = roz + rdz * tmin;     // rays_start
    dx = rdx / rn; dy = rdy / rn; dz = rdz / rn;                             // rays_dir
  }
  const int64_t slot = ray * a.S;
  int kept = 0, kept2 = 0;   // wave-uniform
  float T_cum = 1.f;         // wave-uniform
  float cum = 0.f;           // wave-uniform: the cumdist_thres carry (MODE 1)
  bool stopped = false;
  const float nm1 = (float)(a.S - 1), dm1 = (float)(v.D - 1);      // mode 3
  for (int j0 = 0; j0 < n && !stopped; j0 += UG_WAVE) {
    const int j = j0 + lane;
    bool keep = false, inner = true;
    float px = 0.f, py = 0.f, pz = 0.f, dens = 0.f, alpha = 0.f;
    if (MODE == 1) {
      float dj = 0.f;
      if (j < n) {
        inner = ug_train_point(a, ox, oy, oz, dx, dy, dz, t_table[j], px, py, pz) <= 1.0f;
        if (j > 0) {         // |p_j - p_{j-1}| over ALL consecutive samples (dcvgo.py:287)
          float qx, qy, qz;
          ug_train_point(a, ox, oy, oz, dx, dy, dz, t_table[j - 1], qx, qy, qz);
          dj = ug_norm3_torch(px - qx, py - qy, pz - qz);
        }
      }
      bool over = false;
      const int cnt = (n - j0) < UG_WAVE ? (n - j0) : UG_WAVE;
      for (int k = (j0 == 0 ? 1 : 0); k < cnt; ++k) {       // mask[:, 1:] |= cumdist_thres(dist): sample 0 has no distance
        cum += ug_readlane_f(dj, k);
        const bool ov = cum > v.dist_thres;
        cum *= ov ? 0.f : 1.f;
        if (lane == k) over = ov;
      }
      keep = j < n && (inner || over);
    } else {
      if (j < n) {
        const float dist = MODE == 3 ? (float)j / nm1 : v.stepdist * (float)j;
        px = ox + dx * dist; py = oy + dy * dist; pz = oz + dz * dist;
        keep = !((lox > px) | (loy > py) | (loz > pz) | (hix < px) | (hiy < py) | (hiz < pz));   // ~mask_outbbox
      }
    }
    if (keep) keep = ug_mask_lookup(v, px, py, pz);
    if (keep) {
      const float ux = ug_unorm(px, lox, hix), uy = ug_unorm(py, loy, hiy), uz = ug_unorm(pz, loz, hiz);
      const float acc = ug_train_density(a, src, ux, uy, uz);
      dens = acc;
      if (MODE == 3) {
        // act_shift(p), restated from ug_march_tile_mpi (ugrid_render.h: "act_shift: uz in [-1, 1] ..."): v0 * w0 + v1 * w1 as
        // grid_sample forms it, a corner beyond the last plane not added.  The table is read from global memory: 1 KiB at most, two
        // dwords per kept sample next to eight grid corners, and the waves of a block leave independently (no barrier to stage it)
        const float iz = ((uz + 1.f) / 2.f) * dm1;
        const float f0 = floorf(iz);
        const int i0 = min(max((int)f0, 0), v.D - 1);
        float sh = v.plane_shift[i0] * ((f0 + 1.f) - iz);
        if (i0 + 1 < v.D) sh = sh + v.plane_shift[i0 + 1] * (iz - f0);
        dens = acc + sh;
      }
      float e;
      alpha = ug_train_alpha(dens, a.shift, a.interval, &e);
      keep = alpha > a.thres;
    }
    unsigned long long m = __ballot(keep);
    float myT = 1.f, myW = 0.f;
    unsigned long long mm = m;
    while (mm != 0ull) {
      const int k = __builtin_ctzll(mm);
      mm &= mm - 1ull;
      const float ak = ug_readlane_f(alpha, k);
      if (lane == k) {
        myT = T_cum;
        myW = T_cum * ak;
      }
      T_cum = (float)((double)T_cum * (1. - (double)ak));
      if ((double)T_cum < 1e-3) {          // the sample that crosses keeps its weight; the ray ends here
        stopped = true;
        m &= (2ull << k) - 1ull;
        keep = keep && lane <= k;
        break;
      }
    }
    if (m != 0ull) {
      if (keep) {
        const int64_t idx = slot + kept + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        s_pts[3 * idx] = px; s_pts[3 * idx + 1] = py; s_pts[3 * idx + 2] = pz;
        s_dens[idx] = dens;
        s_step[idx] = (MODE == 1 && !inner) ? ~j : j;
        s_w[idx] = myW; s_T[idx] = myT;
      }
      kept += __popcll(m);
      kept2 += __popcll(__ballot(keep && myW > a.thres));
    }
  }
  if (lane == 0) {
    count[ray] = kept;
    count2[ray] = kept2;
    alphainv_last[ray] = T_cum;
  }
}

template <int MODE>
__global__ void __launch_bounds__(256)
k_train_march_vox(ug_train_args a, ug_train_vox v, const float *__restrict__ grid, const float *__restrict__ rays_o,
                  const float *__restrict__ rays_d, const float *__restrict__ t_table, const float *__restrict__ xyz_min,
                  const float *__restrict__ xyz_max, float *__restrict__ s_pts, float *__restrict__ s_dens,
                  int32_t *__restrict__ s_step, int32_t *__restrict__ count, float *__restrict__ s_w, float *__restrict__ s_T,
                  int32_t *__restrict__ count2, float *__restrict__ alphainv_last) {
  ug_train_march_vox<MODE>(a, v, ug_dens_dense{grid}, rays_o, rays_d, t_table, xyz_min, xyz_max, s_pts, s_dens, s_step, count, s_w, s_T, count2,
                           alphainv_last);
}

// the same march over a TensoRF density (MODE 1 / 2; CL: component-last factors): tf_density in place of the eight-corner gather, and
// everything else -- ray set-up, mask cache, alpha, threshold, stage 2, the scratch slots -- the code above, so that the compaction
// and the backward of the dense march serve it unchanged
template <int MODE, bool CL>
__global__ void __launch_bounds__(256)
k_train_march_tensorf(ug_train_args a, ug_train_vox v, tf_factors f, const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                      const float *__restrict__ t_table, const float *__restrict__ xyz_min, const float *__restrict__ xyz_max,
                      float *__restrict__ s_pts, float *__restrict__ s_dens, int32_t *__restrict__ s_step, int32_t *__restrict__ count,
                      float *__restrict__ s_w, float *__restrict__ s_T, int32_t *__restrict__ count2, float *__restrict__ alphainv_last) {
  static_assert(MODE == 1 || MODE == 2, "TensoRF densities: DirectContractedVoxGO and DirectVoxGO");
  ug_train_march_vox<MODE>(a, v, ug_dens_tensorf<CL>{f}, rays_o, rays_d, t_table, xyz_min, xyz_max, s_pts, s_dens, s_step, count, s_w, s_T,
                           count2, alphainv_last);
}

// after the two cumsums: one wave per ray copies its slot to the ray-major arrays of stage 1 (M1 samples: what the backward
// walks) and of stage 2 (M2 samples above the weight threshold: what the k0 lookup, the rgbnet and the loss consume);
// pos2[i] = the stage-2 index of stage-1 sample i or -1
__global__ void __launch_bounds__(256)
k_train_compact2(int64_t n_rays, int32_t S, float shift, float interval, float thres, const float *__restrict__ s_pts,
                 const float *__restrict__ s_dens, const int32_t *__restrict__ s_step, const float *__restrict__ s_w,
                 const float *__restrict__ s_T, const int32_t *__restrict__ count, const int64_t *__restrict__ end1,
                 const int32_t *__restrict__ count2, const int64_t *__restrict__ end2, const float *__restrict__ t_table,
                 float *__restrict__ pts1, float *__restrict__ dens1, float *__restrict__ w1, float *__restrict__ T1,
                 int32_t *__restrict__ pos2, float *__restrict__ pts2, float *__restrict__ dens2, float *__restrict__ alpha2,
                 float *__restrict__ w2, int64_t *__restrict__ ray_id2, int64_t *__restrict__ step_id2, float *__restrict__ tt2,
                 uint8_t *__restrict__ inner2, int64_t cap2) {
  const int64_t ray = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (ray >= n_rays) return;
  const int lane = ug_lane();
  const int n = count[ray];
  const int64_t d1 = end1[ray] - n, src = ray * (int64_t)S;
  int64_t d2 = end2[ray] - count2[ray];
  for (int i0 = 0; i0 < n; i0 += UG_WAVE) {
    const int i = i0 + lane;
    const bool on = i < n;
    float px = 0.f, py = 0.f, pz = 0.f, dn = 0.f, w = 0.f;
    int st = 0;
    bool inr = true;
    if (on) {
      px = s_pts[3 * (src + i)]; py = s_pts[3 * (src + i) + 1]; pz = s_pts[3 * (src + i) + 2];
      dn = s_dens[src + i]; w = s_w[src + i]; st = s_step[src + i];
      if (st < 0) { st = ~st; inr = false; }      // k_train_march_vox<1>: a contracted sample
      pts1[3 * (d1 + i)] = px; pts1[3 * (d1 + i) + 1] = py; pts1[3 * (d1 + i) + 2] = pz;
      dens1[d1 + i] = dn; w1[d1 + i] = w; T1[d1 + i] = s_T[src + i];
    }
    const bool k2 = on && w > thres;
    const unsigned long long m = __ballot(k2);
    const int64_t o = d2 + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
    // cap2: rows the stage-2 arrays hold (sync-free step with a caller-chosen capacity: what exceeds it is dropped, memory-safe, and
    // the caller finds totals[1] > capacity when it next looks; everywhere else cap2 = INT64_MAX)
    if (on) pos2[d1 + i] = (k2 && o < cap2) ? (int32_t)o : -1;
    if (k2 && o < cap2) {
      float e;
      pts2[3 * o] = px; pts2[3 * o + 1] = py; pts2[3 * o + 2] = pz;
      dens2[o] = dn;
      alpha2[o] = ug_train_alpha(dn, shift, interval, &e);
      w2[o] = w;
      ray_id2[o] = ray;
      step_id2[o] = st;
      tt2[o] = t_table ? t_table[st] : (float)st;
      if (inner2) inner2[o] = inr ? 1 : 0;
    }
    d2 += __popcll(m);
  }
}

// backward of stage 2 of the sampling in one pass over the stage-1 samples of a ray, last to first: Alphas2Weights' backward
// (k_alpha2weight_bwd: float running sum from the last sample, per-sample double expression), Raw2Alpha's (k_raw2alpha_bwd:
// exp clamped at 1e10, double product), and the gradient that reaches the raw density directly (the loss's nearclip term on
// the stage-2 samples) added on top -- g_dens1[i] is what the density lookup's scatter consumes.
__global__ void __launch_bounds__(256)
k_train_sample_bwd(int64_t n_rays, float shift, float interval, const float *__restrict__ dens1, const float *__restrict__ w1,
                   const float *__restrict__ T1, const int32_t *__restrict__ pos2, const int32_t *__restrict__ count,
                   const int64_t *__restrict__ end1, const float *__restrict__ alphainv_last, const float *__restrict__ g_w2,
                   const float *__restrict__ g_last, const float *__restrict__ g_dens2, float *__restrict__ g_dens1) {
  const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (r >= n_rays) return;
  const int lane = ug_lane();
  const int64_t i_e = end1[r], i_s = i_e - count[r];
  float back = g_last ? g_last[r] * alphainv_last[r] : 0.f;
  for (int64_t top = i_e; top > i_s; top -= UG_WAVE) {
    const int64_t i = top - 1 - lane;          // lane k holds sample top-1-k
    const bool ok = i >= i_s;
    const int p2 = ok ? pos2[i] : -1;
    const float gw = (p2 >= 0 && g_w2) ? g_w2[p2] : 0.f;
    const float prod = ok ? gw * w1[i] : 0.f;
    const int cnt = (int)((top - i_s) < UG_WAVE ? (top - i_s) : UG_WAVE);
    float my_back = 0.f;
    for (int k = 0; k < cnt; ++k) {
      if (lane == k) my_back = back;
      back += ug_readlane_f(prod, k);
    }
    if (ok) {
      float ef;
      const float a = ug_train_alpha(dens1[i], shift, interval, &ef);
      const float g_alpha = (float)((double)(gw * T1[i]) - (double)my_back / ((double)(1 - a) + 1e-10));
      const double e = (double)ef;
      const double em = e < 1e10 ? e : 1e10;
      const float pw = powf(1 + ef, -interval - 1);
      float g = (float)(em * (double)pw * (double)interval * (double)g_alpha);
      if (p2 >= 0 && g_dens2) g = g + g_dens2[p2];
      g_dens1[i] = g;
    }
  }
}

__global__ void __launch_bounds__(256)
k_train_compact(int64_t n_rays, int32_t S, const float *__restrict__ s_pts, const float *__restrict__ s_dens,
                const int32_t *__restrict__ s_step, const int32_t *__restrict__ count, const int64_t *__restrict__ offset_end,
                const float *__restrict__ t_table, float *__restrict__ pts, float *__restrict__ dens,
                int64_t *__restrict__ ray_id, int64_t *__restrict__ step_id, float *__restrict__ tt) {
  const int64_t ray = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (ray >= n_rays) return;
  const int lane = ug_lane();
  const int n = count[ray];
  const int64_t dst = offset_end[ray] - n, src = ray * (int64_t)S;
  for (int i = lane; i < n; i += UG_WAVE) {
    const int st = s_step[src + i];
    pts[3 * (dst + i)] = s_pts[3 * (src + i)];
    pts[3 * (dst + i) + 1] = s_pts[3 * (src + i) + 1];
    pts[3 * (dst + i) + 2] = s_pts[3 * (src + i) + 2];
    dens[dst + i] = s_dens[src + i];
    ray_id[dst + i] = ray;
    step_id[dst + i] = st;
    tt[dst + i] = t_table[st];
  }
}

// ----------------------------------------------------------------------------------------------
// C ABI
// ----------------------------------------------------------------------------------------------
static int ug_train_march_any(const float *density_grid, int P, int X, int Y, int Z, int freq_num, const float *rays_o,
                              const float *rays_d, int64_t n_rays, const float *t_table, int32_t n_samples,
                              const float *scene_center3, const float *scene_radius3, const float *xyz_min,
                              const float *xyz_max, double bg_len, int norm_l2, float act_shift, float interval,
                              float thres, float *scratch_pts, float *scratch_density, int32_t *scratch_step,
                              int32_t *count, float *scratch_w, float *scratch_T, int32_t *count2, float *alphainv_last,
                              ugrid_stream_t s) {
  if (n_rays <= 0) return 0;
  if (P != (freq_num > 0 ? 2 * freq_num + 1 : 1) || n_samples <= 0) return (int)hipErrorInvalidValue;
  ug_train_args a;
  a.n_rays = n_rays; a.S = n_samples; a.P = P; a.F = freq_num; a.X = X; a.Y = Y; a.Z = Z; a.norm_l2 = norm_l2;
  a.cx = scene_center3[0]; a.cy = scene_center3[1]; a.cz = scene_center3[2];
  a.rx = scene_radius3[0]; a.ry = scene_radius3[1]; a.rz = scene_radius3[2];
  const double Bd = 1.0 + bg_len;
  a.B = (float)Bd; a.A = (float)(Bd * 1.0 - 1.0);
  a.shift = act_shift; a.interval = interval; a.thres = thres;
  if (scratch_w)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_train_march<true>), dim3(ug_blocks(n_rays * UG_WAVE, 256)), dim3(256), 0, ST(s), a, density_grid,
                       rays_o, rays_d, t_table, xyz_min, xyz_max, scratch_pts, scratch_density, scratch_step, count, scratch_w, scratch_T,
                       count2, alphainv_last);
  else
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_train_march<false>), dim3(ug_blocks(n_rays * UG_WAVE, 256)), dim3(256), 0, ST(s), a, density_grid,
                       rays_o, rays_d, t_table, xyz_min, xyz_max, scratch_pts, scratch_density, scratch_step, count, (float *)nullptr,
                       (float *)nullptr, (int32_t *)nullptr, (float *)nullptr);
  UG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ugrid_train_march(const float *density_grid, int P, int X, int Y, int Z, int freq_num, const float *rays_o,
                                 const float *rays_d, int64_t n_rays, const float *t_table, int32_t n_samples,
                                 const float *scene_center3, const float *scene_radius3, const float *xyz_min,
                                 const float *xyz_max, double bg_len, int norm_l2, float act_shift, float interval,
                                 float thres, float *scratch_pts, float *scratch_density, int32_t *scratch_step,
                                 int32_t *count, ugrid_stream_t s) {
  return ug_train_march_any(density_grid, P, X, Y, Z, freq_num, rays_o, rays_d, n_rays, t_table, n_samples, scene_center3, scene_radius3,
                            xyz_min, xyz_max, bg_len, norm_l2, act_shift, interval, thres, scratch_pts, scratch_density, scratch_step,
                            count, nullptr, nullptr, nullptr, nullptr, s);
}

extern "C" int ugrid_train_sample(const float *density_grid, int P, int X, int Y, int Z, int freq_num, const float *rays_o,
                                  const float *rays_d, int64_t n_rays, const float *t_table, int32_t n_samples,
                                  const float *scene_center3, const float *scene_radius3, const float *xyz_min,
                                  const float *xyz_max, double bg_len, int norm_l2, float act_shift, float interval,
                                  float thres, float *scratch_pts, float *scratch_density, int32_t *scratch_step,
                                  float *scratch_w, float *scratch_T, int32_t *count, int32_t *count2, float *alphainv_last,
                                  ugrid_stream_t s) {
  if (!scratch_w || !scratch_T || !count2 || !alphainv_last) return (int)hipErrorInvalidValue;
  return ug_train_march_any(density_grid, P, X, Y, Z, freq_num, rays_o, rays_d, n_rays, t_table, n_samples, scene_center3, scene_radius3,
                            xyz_min, xyz_max, bg_len, norm_l2, act_shift, interval, thres, scratch_pts, scratch_density, scratch_step,
                            count, scratch_w, scratch_T, count2, alphainv_last, s);
}

extern "C" int ugrid_train_sample_compact(int64_t n_rays, int32_t n_samples, float act_shift, float interval, float thres,
                                          const float *scratch_pts, const float *scratch_density, const int32_t *scratch_step,
                                          const float *scratch_w, const float *scratch_T, const int32_t *count,
                                          const int64_t *offset_end, const int32_t *count2, const int64_t *offset_end2,
                                          const float *t_table, float *pts1, float *density1, float *weights1, float *T1,
                                          int32_t *pos2, float *pts2, float *density2, float *alpha2, float *weights2,
                                          int64_t *ray_id2, int64_t *step_id2, float *t2, ugrid_stream_t s) {
  if (n_rays <= 0) return 0;
  hipLaunchKernelGGL(k_train_compact2, dim3(ug_blocks(n_rays * UG_WAVE, 256)), dim3(256), 0, ST(s), n_rays, n_samples, act_shift, interval,
                     thres, scratch_pts, scratch_density, scratch_step, scratch_w, scratch_T, count, offset_end, count2, offset_end2,
                     t_table, pts1, density1, weights1, T1, pos2, pts2, density2, alpha2, weights2, ray_id2, step_id2, t2,
                     (uint8_t *)nullptr, ug_tl_devn.cap > 0 ? ug_tl_devn.cap : INT64_MAX);
  UG_LAUNCH_CHECK();
  return 0;
}

static int ug_fill_train_vox(ug_train_vox *v, const uint8_t *mask, const int32_t *mask_dims3, const float *xyz2ijk_scale3,
                             const float *xyz2ijk_shift3) {
  if (!mask_dims3) return (int)hipErrorInvalidValue;
  v->dist_thres = 0.f; v->near = 0.f; v->far = 0.f; v->stepdist = 1.f;
  v->plane_shift = nullptr; v->D = 1;
  return ug_fill_mask_args(*v, mask, mask_dims3[0], mask_dims3[1], mask_dims3[2], xyz2ijk_scale3, xyz2ijk_shift3);
}

extern "C" int ugrid_train_sample_dcvgo(const float *density_grid, int X, int Y, int Z, const float *rays_o, const float *rays_d,
                                        int64_t n_rays, const float *t_table, int32_t n_samples, const float *scene_center3,
                                        const float *scene_radius3, const float *xyz_min, const float *xyz_max, double bg_len,
                                        int norm_l2, float dist_thres, const uint8_t *mask, const int32_t *mask_dims3,
                                        const float *xyz2ijk_scale3, const float *xyz2ijk_shift3, float act_shift, float interval,
                                        float thres, float *scratch_pts, float *scratch_density, int32_t *scratch_step,
                                        float *scratch_w, float *scratch_T, int32_t *count, int32_t *count2, float *alphainv_last,
                                        ugrid_stream_t s) {
  if (n_rays <= 0) return 0;
  if (n_samples <= 0 || !scratch_w || !scratch_T || !count2 || !alphainv_last || !t_table) return (int)hipErrorInvalidValue;
  ug_train_vox v;
  const int rc = ug_fill_train_vox(&v, mask, mask_dims3, xyz2ijk_scale3, xyz2ijk_shift3);
  if (rc) return rc;
  v.dist_thres = dist_thres;
  ug_train_args a;
  a.n_rays = n_rays; a.S = n_samples; a.P = 1; a.F = 0; a.X = X; a.Y = Y; a.Z = Z; a.norm_l2 = norm_l2;
  a.cx = scene_center3[0]; a.cy = scene_center3[1]; a.cz = scene_center3[2];
  a.rx = scene_radius3[0]; a.ry = scene_radius3[1]; a.rz = scene_radius3[2];
  const double Bd = 1.0 + bg_len;
  a.B = (float)Bd; a.A = (float)bg_len;       // dcvgo.py:261: (1 + bg_len) - bg_len / norm
  a.shift = act_shift; a.interval = interval; a.thres = thres;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_train_march_vox<1>), dim3(ug_blocks(n_rays * UG_WAVE, 256)), dim3(256), 0, ST(s), a, v, density_grid,
                     rays_o, rays_d, t_table, xyz_min, xyz_max, scratch_pts, scratch_density, scratch_step, count, scratch_w, scratch_T,
                     count2, alphainv_last);
  UG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ugrid_train_sample_dvgo(const float *density_grid, int X, int Y, int Z, const float *rays_o, const float *rays_d,
                                       int64_t n_rays, int32_t slots_per_ray, const float *xyz_min, const float *xyz_max, float near,
                                       float far, float stepdist, const uint8_t *mask, const int32_t *mask_dims3,
                                       const float *xyz2ijk_scale3, const float *xyz2ijk_shift3, float act_shift, float interval,
                                       float thres, float *scratch_pts, float *scratch_density, int32_t *scratch_step,
                                       float *scratch_w, float *scratch_T, int32_t *count, int32_t *count2, float *alphainv_last,
                                       ugrid_stream_t s) {
  if (n_rays <= 0) return 0;
  if (slots_per_ray <= 0 || !(stepdist > 0.f) || !scratch_w || !scratch_T || !count2 || !alphainv_last) return (int)hipErrorInvalidValue;
  ug_train_vox v;
  const int rc = ug_fill_train_vox(&v, mask, mask_dims3, xyz2ijk_scale3, xyz2ijk_shift3);
  if (rc) return rc;
  v.near = near; v.far = far; v.stepdist = stepdist;
  ug_train_args a;
  a.n_rays = n_rays; a.S = slots_per_ray; a.P = 1; a.F = 0; a.X = X; a.Y = Y; a.Z = Z; a.norm_l2 = 0;
  a.cx = a.cy = a.cz = 0.f; a.rx = a.ry = a.rz = 1.f; a.B = 1.f; a.A = 0.f;
  a.shift = act_shift; a.interval = interval; a.thres = thres;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_train_march_vox<2>), dim3(ug_blocks(n_rays * UG_WAVE, 256)), dim3(256), 0, ST(s), a, v, density_grid,
                     rays_o, rays_d, (const float *)nullptr, xyz_min, xyz_max, scratch_pts, scratch_density, scratch_step, count, scratch_w,
                     scratch_T, count2, alphainv_last);
  UG_LAUNCH_CHECK();
  return 0;
}

// the TensoRF twins of the two entry points above: the six factors in place of the dense grid
static bool ug_tensorf_density_ok(const float *xy, const float *xz, const float *yz, const float *xv, const float *yv, const float *zv, int X,
                                  int Y, int Z, int R, int Rxy) {
  return xy && xz && yz && xv && yv && zv && X >= 1 && Y >= 1 && Z >= 1 && R >= 1 && Rxy >= 1;
}

extern "C" int ugrid_train_sample_dcvgo_tensorf(const float *xy_plane, const float *xz_plane, const float *yz_plane, const float *x_vec,
                                                const float *y_vec, const float *z_vec, int X, int Y, int Z, int R, int Rxy, int comp_last,
                                                const float *rays_o, const float *rays_d, int64_t n_rays, const float *t_table,
                                                int32_t n_samples, const float *scene_center3, const float *scene_radius3,
                                                const float *xyz_min, const float *xyz_max, double bg_len, int norm_l2, float dist_thres,
                                                const uint8_t *mask, const int32_t *mask_dims3, const float *xyz2ijk_scale3,
                                                const float *xyz2ijk_shift3, float act_shift, float interval, float thres, float *scratch_pts,
                                                float *scratch_density, int32_t *scratch_step, float *scratch_w, float *scratch_T,
                                                int32_t *count, int32_t *count2, float *alphainv_last, ugrid_stream_t s) {
  if (!ug_tensorf_density_ok(xy_plane, xz_plane, yz_plane, x_vec, y_vec, z_vec, X, Y, Z, R, Rxy)) return (int)hipErrorInvalidValue;
  if (n_rays <= 0) return 0;
  if (n_samples <= 0 || !scratch_w || !scratch_T || !count2 || !alphainv_last || !t_table) return (int)hipErrorInvalidValue;
  ug_train_vox v;
  const int rc = ug_fill_train_vox(&v, mask, mask_dims3, xyz2ijk_scale3, xyz2ijk_shift3);
  if (rc) return rc;
  v.dist_thres = dist_thres;
  ug_train_args a;
  a.n_rays = n_rays; a.S = n_samples; a.P = 1; a.F = 0; a.X = X; a.Y = Y; a.Z = Z; a.norm_l2 = norm_l2;
  a.cx = scene_center3[0]; a.cy = scene_center3[1]; a.cz = scene_center3[2];
  a.rx = scene_radius3[0]; a.ry = scene_radius3[1]; a.rz = scene_radius3[2];
  const double Bd = 1.0 + bg_len;
  a.B = (float)Bd; a.A = (float)bg_len;       // dcvgo.py:261: (1 + bg_len) - bg_len / norm
  a.shift = act_shift; a.interval = interval; a.thres = thres;
  const tf_factors f = tf_make(xy_plane, xz_plane, yz_plane, x_vec, y_vec, z_vec, X, Y, Z, R, Rxy);
  const dim3 blocks(ug_blocks(n_rays * UG_WAVE, 256));
  if (comp_last)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_train_march_tensorf<1, true>), blocks, dim3(256), 0, ST(s), a, v, f, rays_o, rays_d, t_table, xyz_min,
                       xyz_max, scratch_pts, scratch_density, scratch_step, count, scratch_w, scratch_T, count2, alphainv_last);
  else
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_train_march_tensorf<1, false>), blocks, dim3(256), 0, ST(s), a, v, f, rays_o, rays_d, t_table, xyz_min,
                       xyz_max, scratch_pts, scratch_density, scratch_step, count, scratch_w, scratch_T, count2, alphainv_last);
  UG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ugrid_train_sample_dvgo_tensorf(const float *xy_plane, const float *xz_plane, const float *yz_plane, const float *x_vec,
                                               const float *y_vec, const float *z_vec, int X, int Y, int Z, int R, int Rxy, int comp_last,
                                               const float *rays_o, const float *rays_d, int64_t n_rays, int32_t slots_per_ray,
                                               const float *xyz_min, const float *xyz_max, float near, float far, float stepdist,
                                               const uint8_t *mask, const int32_t *mask_dims3, const float *xyz2ijk_scale3,
                                               const float *xyz2ijk_shift3, float act_shift, float interval, float thres, float *scratch_pts,
                                               float *scratch_density, int32_t *scratch_step, float *scratch_w, float *scratch_T,
                                               int32_t *count, int32_t *count2, float *alphainv_last, ugrid_stream_t s) {
  if (!ug_tensorf_density_ok(xy_plane, xz_plane, yz_plane, x_vec, y_vec, z_vec, X, Y, Z, R, Rxy)) return (int)hipErrorInvalidValue;
  if (n_rays <= 0) return 0;
  if (slots_per_ray <= 0 || !(stepdist > 0.f) || !scratch_w || !scratch_T || !count2 || !alphainv_last) return (int)hipErrorInvalidValue;
  ug_train_vox v;
  const int rc = ug_fill_train_vox(&v, mask, mask_dims3, xyz2ijk_scale3, xyz2ijk_shift3);
  if (rc) return rc;
  v.near = near; v.far = far; v.stepdist = stepdist;
  ug_train_args a;
  a.n_rays = n_rays; a.S = slots_per_ray; a.P = 1; a.F = 0; a.X = X; a.Y = Y; a.Z = Z; a.norm_l2 = 0;
  a.cx = a.cy = a.cz = 0.f; a.rx = a.ry = a.rz = 1.f; a.B = 1.f; a.A = 0.f;
  a.shift = act_shift; a.interval = interval; a.thres = thres;
  const tf_factors f = tf_make(xy_plane, xz_plane, yz_plane, x_vec, y_vec, z_vec, X, Y, Z, R, Rxy);
  const dim3 blocks(ug_blocks(n_rays * UG_WAVE, 256));
  if (comp_last)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_train_march_tensorf<2, true>), blocks, dim3(256), 0, ST(s), a, v, f, rays_o, rays_d,
                       (const float *)nullptr, xyz_min, xyz_max, scratch_pts, scratch_density, scratch_step, count, scratch_w, scratch_T, count2,
                       alphainv_last);
  else
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_train_march_tensorf<2, false>), blocks, dim3(256), 0, ST(s), a, v, f, rays_o, rays_d,
                       (const float *)nullptr, xyz_min, xyz_max, scratch_pts, scratch_density, scratch_step, count, scratch_w, scratch_T, count2,
                       alphainv_last);
  UG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ugrid_train_sample_mpi(const float *density_grid, int X, int Y, int Z, const float *rays_o, const float *rays_d,
                                      int64_t n_rays, int32_t n_steps, const float *xyz_min, const float *xyz_max,
                                      const float *act_shift, int32_t mpi_depth, const uint8_t *mask, const int32_t *mask_dims3,
                                      const float *xyz2ijk_scale3, const float *xyz2ijk_shift3, float interval, float thres,
                                      float *scratch_pts, float *scratch_density, int32_t *scratch_step, float *scratch_w,
                                      float *scratch_T, int32_t *count, int32_t *count2, float *alphainv_last, ugrid_stream_t s) {
  if (n_rays <= 0) return 0;
  if (n_steps < 2 || !act_shift || mpi_depth < 1 || mpi_depth > 256 || !scratch_w || !scratch_T || !count2 || !alphainv_last)
    return (int)hipErrorInvalidValue;
  ug_train_vox v;
  const int rc = ug_fill_train_vox(&v, mask, mask_dims3, xyz2ijk_scale3, xyz2ijk_shift3);
  if (rc) return rc;
  v.plane_shift = act_shift; v.D = mpi_depth;
  ug_train_args a;
  a.n_rays = n_rays; a.S = n_steps; a.P = 1; a.F = 0; a.X = X; a.Y = Y; a.Z = Z; a.norm_l2 = 0;
  a.cx = a.cy = a.cz = 0.f; a.rx = a.ry = a.rz = 1.f; a.B = 1.f; a.A = 0.f;
  a.shift = 0.f; a.interval = interval; a.thres = thres;      // the per-plane shift is part of the stored density
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_train_march_vox<3>), dim3(ug_blocks(n_rays * UG_WAVE, 256)), dim3(256), 0, ST(s), a, v, density_grid,
                     rays_o, rays_d, (const float *)nullptr, xyz_min, xyz_max, scratch_pts, scratch_density, scratch_step, count, scratch_w,
                     scratch_T, count2, alphainv_last);
  UG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ugrid_train_sample_compact_vox(int64_t n_rays, int32_t slots_per_ray, float act_shift, float interval, float thres,
                                              const float *scratch_pts, const float *scratch_density, const int32_t *scratch_step,
                                              const float *scratch_w, const float *scratch_T, const int32_t *count,
                                              const int64_t *offset_end, const int32_t *count2, const int64_t *offset_end2,
                                              const float *t_table, float *pts1, float *density1, float *weights1, float *T1,
                                              int32_t *pos2, float *pts2, float *density2, float *alpha2, float *weights2,
                                              int64_t *ray_id2, int64_t *step_id2, float *t2, uint8_t *inner2, ugrid_stream_t s) {
  if (n_rays <= 0) return 0;
  hipLaunchKernelGGL(k_train_compact2, dim3(ug_blocks(n_rays * UG_WAVE, 256)), dim3(256), 0, ST(s), n_rays, slots_per_ray, act_shift,
                     interval, thres, scratch_pts, scratch_density, scratch_step, scratch_w, scratch_T, count, offset_end, count2,
                     offset_end2, t_table, pts1, density1, weights1, T1, pos2, pts2, density2, alpha2, weights2, ray_id2, step_id2, t2,
                     inner2, ug_tl_devn.cap > 0 ? ug_tl_devn.cap : INT64_MAX);
  UG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ugrid_train_sample_backward(int64_t n_rays, float act_shift, float interval, const float *density1,
                                           const float *weights1, const float *T1, const int32_t *pos2, const int32_t *count,
                                           const int64_t *offset_end, const float *alphainv_last, const float *g_weights2,
                                           const float *g_alphainv_last, const float *g_density2, float *g_density1,
                                           ugrid_stream_t s) {
  if (n_rays <= 0) return 0;
  hipLaunchKernelGGL(k_train_sample_bwd, dim3(ug_blocks(n_rays * UG_WAVE, 256)), dim3(256), 0, ST(s), n_rays, act_shift, interval,
                     density1, weights1, T1, pos2, count, offset_end, alphainv_last, g_weights2, g_alphainv_last, g_density2, g_density1);
  UG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ugrid_train_compact(int64_t n_rays, int32_t n_samples, const float *scratch_pts, const float *scratch_density,
                                   const int32_t *scratch_step, const int32_t *count, const int64_t *offset_end,
                                   const float *t_table, float *pts, float *density, int64_t *ray_id, int64_t *step_id,
                                   float *t, ugrid_stream_t s) {
  if (n_rays <= 0) return 0;
  hipLaunchKernelGGL(k_train_compact, dim3(ug_blocks(n_rays * UG_WAVE, 256)), dim3(256), 0, ST(s), n_rays, n_samples,
                     scratch_pts, scratch_density, scratch_step, count, offset_end, t_table, pts, density, ray_id, step_id, t);
  UG_LAUNCH_CHECK();
  return 0;
}
