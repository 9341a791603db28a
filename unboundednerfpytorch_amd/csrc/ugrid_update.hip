// libugrid_hip.so -- the parameter update: the total-variation gradient (total_variation_cuda), the Adam family (adam_upd_cuda)
// and their fused passes, for gfx950 (MI355X): 16-byte vector streams, one float4 per lane.  fp32 arithmetic follows the
// reference expression trees (compiled with -ffp-contract=off), so results are bit-identical to oracle/ref_ops.c.
//
// Reference behaviour restated (never copied): FourierGrid/cuda/adam_upd_kernel.cu, total_variation_kernel.cu -- per-function
// file:line citations are in include/ugrid_hip.h.
#include <type_traits>

#include "ugrid_common.h"

#define ST(s) ((hipStream_t)(s))

// ----------------------------------------------------------------------------------------------
// The reference's per-element TV term: six sequential fp32 adds in the order k-, k+, j-, j+, i-, i+ onto zero.  Quirk kept: the
// x-axis (i) term is weighted by wz.  The order of the adds is a bit-exactness contract -- this is its only definition.
//
// Every caller hands in six neighbour values from UNCONDITIONAL loads (a missing neighbour re-reads the element itself) and
// switches the missing terms off by a zero WEIGHT: with `if (k != 0) nk0 = load` every load sat under its own exec branch and
// hipcc waited vmcnt(0) behind each -- seven round trips per element one after the other.  Bit-identical: a switched-off term
// is 0 * clamp(p - p) = 0.
//
// A macro, not a function: through a (forced-inline) function hipcc compiles the MASKED kernels differently -- no branch per
// element, whole float4 neighbour loads for every lane with a non-zero -- and the canonical masked pass at 5 % non-zeros read
// 3 % slower (profiles/refactor_update/ab.txt); as an expression every kernel keeps the instructions it had with the term written out.
// ----------------------------------------------------------------------------------------------
__device__ __forceinline__ float ug_clamp1(float v) { return fminf(fmaxf(v, -1.f), 1.f); }

#define UG_TV_TERM(p, nk0, nk1, nj0, nj1, ni0, ni1, wk0, wk1, wj0, wj1, wi0, wi1)                                        \
  ((((((0.f + (wk0) * ug_clamp1((p) - (nk0))) + (wk1) * ug_clamp1((p) - (nk1))) + (wj0) * ug_clamp1((p) - (nj0))) +      \
     (wj1) * ug_clamp1((p) - (nj1))) + (wi0) * ug_clamp1((p) - (ni0))) + (wi1) * ug_clamp1((p) - (ni1)))

// total variation gradient (in place), dense or masked, any shape and alignment: one element per lane, 64-bit indices
template <bool DENSE>
__global__ void k_tv(const float *__restrict__ param, float *__restrict__ grad, float wy, float wz,
                     int64_t sz_i, int64_t sz_j, int64_t sz_k, int64_t N) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= N) return;
  const float g0 = grad[idx];
  if (!(DENSE || g0 != 0.f)) return;
  const int64_t k = idx % sz_k;
  const int64_t j = idx / sz_k % sz_j;
  const int64_t i = idx / sz_k / sz_j % sz_i;
  const int64_t sj = sz_k, si = sz_k * sz_j;
  const float p = param[idx];
  const float n0 = param[idx - (k == 0 ? 0 : 1)], n1 = param[idx + (k == sz_k - 1 ? 0 : 1)];
  const float n2 = param[idx - (j == 0 ? 0 : sj)], n3 = param[idx + (j == sz_j - 1 ? 0 : sj)];
  const float n4 = param[idx - (i == 0 ? 0 : si)], n5 = param[idx + (i == sz_i - 1 ? 0 : si)];
  grad[idx] = g0 + UG_TV_TERM(p, n0, n1, n2, n3, n4, n5, k == 0 ? 0.f : wz, k == sz_k - 1 ? 0.f : wz, j == 0 ? 0.f : wy,
                              j == sz_j - 1 ? 0.f : wy, i == 0 ? 0.f : wz, i == sz_i - 1 ? 0.f : wz);
}

// XCD = blocks renumbered so that each of the 8 XCDs (the hardware deals consecutive workgroups to them round-robin)
// walks one contiguous eighth of the array: the stencil's j / i neighbour lines are then found in the XCD's own L2
// instead of being fetched again over the fabric by another one (4.98 -> 4.41 ms on the channel-last S3 k0 array).
typedef float ug_v4f __attribute__((ext_vector_type(4)));
// streaming arrays (gradient, moments, the new parameters) bypass the caches' retention: the L2 is left to the stencil
template <bool NT> __device__ __forceinline__ float4 ug_ld4(const float *p) {
  if (NT) { const ug_v4f v = __builtin_nontemporal_load((const ug_v4f *)p); return make_float4(v.x, v.y, v.z, v.w); }
  return *(const float4 *)p;
}
template <bool NT> __device__ __forceinline__ void ug_st4(float *p, float a, float b, float c, float d) {
  if (NT) { ug_v4f v = {a, b, c, d}; __builtin_nontemporal_store(v, (ug_v4f *)p); }
  else *(float4 *)p = make_float4(a, b, c, d);
}

// true for all 8 lanes of a 128-byte line (8 consecutive float4 lanes) when any of them says so: whole-line stores
__device__ __forceinline__ bool ug_line_any(bool mine) {
  const unsigned long long m = __ballot(mine);
  return ((m >> (__lane_id() & ~7u)) & 0xFFull) != 0;
}

// touched-line bitmap of a recycled gradient buffer (k_grid_query_backward): float4 lane q belongs to the 256-byte line
// q >> 4; null = no bitmap, every line counts as touched
__device__ __forceinline__ bool ug_touched(const uint32_t *__restrict__ touch, unsigned q) {
  return !touch || ((touch[q >> 9] >> ((q >> 4) & 31u)) & 1u);
}

template <int XCD>
__device__ __forceinline__ unsigned ug_xcd_block() {
  unsigned b = blockIdx.x;
  if (XCD) {
    const unsigned nb = gridDim.x, per = nb >> 3, rem = nb & 7u, xcd = b & 7u;
    b = xcd * per + (xcd < rem ? xcd : rem) + (b >> 3);
  }
  return b;
}

// ----------------------------------------------------------------------------------------------
// Adam family.  MODE 0 dense, 1 masked (skip grad==0), 2 per-voxel lr.  4 voxels per lane with
// 16-byte loads; in masked mode a lane touches m/v/param only when one of its 4 grads is non-zero,
// so an almost-empty gradient costs ~4 B/voxel of HBM reads.
// ----------------------------------------------------------------------------------------------
template <int MODE>
__device__ __forceinline__ void ug_adam_one(float &p, float g, float &m, float &v, float lrk,
                                            float step_size, float beta1, float beta2, float eps) {
  m = beta1 * m + (1 - beta1) * g;
  v = beta2 * v + (1 - beta2) * g * g;
  if (MODE == 2) p -= step_size * lrk * m / (sqrtf(v) + eps);
  else p -= step_size * m / (sqrtf(v) + eps);
}

// host-side, in float, like the reference (adam_upd_kernel.cu:72)
static inline float ug_adam_step_size(float lr, float beta1, float beta2, int step) {
  return lr * sqrtf(1 - powf(beta2, (float)step)) / (1 - powf(beta1, (float)step));
}

// ----------------------------------------------------------------------------------------------
// TV gradient, and the fused DENSE TV + Adam pass, one float4 per lane with 32-bit index arithmetic (N < 2^31, 16-byte
// aligned arrays).  ADAM: 0 = TV only (grad updated in place), 1 = fused with masked Adam, 2 = fused with dense Adam
// (param_out written; grad untouched, or re-zeroed).
//
// The fused pass has no reference counterpart.  While `tv_dense_before` holds (run_train.py:281-287,
// 10 000 of truck_single's 30 000 iterations) the reference runs total_variation_add_grad(dense) -- which makes EVERY gradient
// entry non-zero -- and then masked_adam_upd, i.e. two full passes over param / grad and one over both moments: 13 arrays of
// traffic.  Fused: the TV term is added to the gradient in registers and fed to ug_adam_one: 7 arrays (param, grad, m, v read;
// param', m, v written), the gradient is never written back.  The stencil needs the neighbours' OLD values, so the new
// parameters go to a second buffer that the caller swaps in.  Bit-identical to the two-kernel sequence; ADAM == 1 is the
// skip_zero_grad rule applied to the TV-added gradient.
//
// The two layouts differ only in what a lane's four elements are, i.e. in how it finds its (i, j, k) and its k-neighbours:
//   canonical ([P][C][X][Y][Z], sz_k % 4 == 0): 4 voxels along k; the inner k-neighbours are in the lane's own float4, the
//     outer two are scalar loads, and only elements 0 / 3 can sit at a k border;
//   CL, channel-last ([P][X][Y][Z][C], torch channels_last_3d, C % 4 == 0): 4 channels of one voxel, the neighbours of the SAME
//     channels at +-C (k), +-Z*C (j), +-Y*Z*C (i).
// Per element the expression is the same, so the results of the two layouts are equal element for element.
// ----------------------------------------------------------------------------------------------
template <bool CL, bool DENSE, int ADAM, int XCD>
__device__ __forceinline__ void ug_tv_lane(const float *__restrict__ param, float *__restrict__ param_out, float *__restrict__ grad,
                                           float *__restrict__ exp_avg, float *__restrict__ exp_avg_sq, float wy, float wz, int sz_i,
                                           int sz_j, int sz_k, int C, unsigned q, float step_size, float beta1, float beta2, float eps,
                                           int rezero, bool hit) {
  const unsigned idx = q * 4u;
  // hit = false: an unmarked line of a recycled gradient is all zero and is not read (dense mode only; the masked mode
  // does not come here for such a line)
  const float4 g0 = hit ? ug_ld4<XCD == 2>(grad + idx) : make_float4(0.f, 0.f, 0.f, 0.f);
  if (!DENSE && g0.x == 0.f && g0.y == 0.f && g0.z == 0.f && g0.w == 0.f) return;
  // k counts lanes along the fastest spatial axis: voxels (CL, C / 4 lanes each) or groups of 4 voxels (canonical)
  const unsigned nk = CL ? (unsigned)sz_k : (unsigned)sz_k >> 2, vox = CL ? q / ((unsigned)C >> 2) : q;
  const unsigned k = vox % nk, j = (vox / nk) % (unsigned)sz_j, i = (vox / (nk * (unsigned)sz_j)) % (unsigned)sz_i;
  const unsigned sk = CL ? (unsigned)C : 1u, sj = (unsigned)sz_k * sk, si = (unsigned)sz_j * sj;
  const float4 p = *(const float4 *)(param + idx);
  const float wk0 = k != 0 ? wz : 0.f, wk1 = k != nk - 1 ? wz : 0.f;
  const float wj0 = j != 0 ? wy : 0.f, wj1 = j != (unsigned)sz_j - 1 ? wy : 0.f;
  const float wi0 = i != 0 ? wz : 0.f, wi1 = i != (unsigned)sz_i - 1 ? wz : 0.f;
  float k0[4], k1[4];
  if (CL) {
    const float4 nk0 = *(const float4 *)(param + idx - (k != 0 ? sk : 0u));
    const float4 nk1 = *(const float4 *)(param + idx + (k != nk - 1 ? sk : 0u));
    k0[0] = nk0.x; k0[1] = nk0.y; k0[2] = nk0.z; k0[3] = nk0.w;
    k1[0] = nk1.x; k1[1] = nk1.y; k1[2] = nk1.z; k1[3] = nk1.w;
  } else {
    k0[0] = param[idx - (k != 0 ? 1u : 0u)]; k0[1] = p.x; k0[2] = p.y; k0[3] = p.z;
    k1[0] = p.y; k1[1] = p.z; k1[2] = p.w; k1[3] = param[idx + (k != nk - 1 ? 4u : 3u)];
  }
  const float4 nj0 = *(const float4 *)(param + idx - (j != 0 ? sj : 0u));
  const float4 nj1 = *(const float4 *)(param + idx + (j != (unsigned)sz_j - 1 ? sj : 0u));
  const float4 ni0 = *(const float4 *)(param + idx - (i != 0 ? si : 0u));
  const float4 ni1 = *(const float4 *)(param + idx + (i != (unsigned)sz_i - 1 ? si : 0u));
  float pv[4] = {p.x, p.y, p.z, p.w};
  const float pold[4] = {p.x, p.y, p.z, p.w}, gv[4] = {g0.x, g0.y, g0.z, g0.w};
  const float a0[4] = {nj0.x, nj0.y, nj0.z, nj0.w}, a1[4] = {nj1.x, nj1.y, nj1.z, nj1.w};
  const float b0[4] = {ni0.x, ni0.y, ni0.z, ni0.w}, b1[4] = {ni1.x, ni1.y, ni1.z, ni1.w};
  float mv[4] = {0.f, 0.f, 0.f, 0.f}, vv[4] = {0.f, 0.f, 0.f, 0.f};
  if (ADAM) {
    const float4 m4 = ug_ld4<XCD == 2>(exp_avg + idx), v4 = ug_ld4<XCD == 2>(exp_avg_sq + idx);
    mv[0] = m4.x; mv[1] = m4.y; mv[2] = m4.z; mv[3] = m4.w;
    vv[0] = v4.x; vv[1] = v4.y; vv[2] = v4.z; vv[3] = v4.w;
  }
  float out[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float term = UG_TV_TERM(pold[e], k0[e], k1[e], a0[e], a1[e], b0[e], b1[e], (CL || e == 0) ? wk0 : wz, (CL || e == 3) ? wk1 : wz,
                                  wj0, wj1, wi0, wi1);
    // the rule after the term: masked TV leaves an exact zero alone; masked Adam skips an exact zero of the SUM
    out[e] = (DENSE || gv[e] != 0.f) ? gv[e] + term : gv[e];
    if (ADAM) {
      if (ADAM == 2 || out[e] != 0.f) ug_adam_one<0>(pv[e], out[e], mv[e], vv[e], 1.f, step_size, beta1, beta2, eps);
    }
  }
  if (ADAM) {
    ug_st4<XCD == 2>(param_out + idx, pv[0], pv[1], pv[2], pv[3]);
    ug_st4<XCD == 2>(exp_avg + idx, mv[0], mv[1], mv[2], mv[3]);
    ug_st4<XCD == 2>(exp_avg_sq + idx, vv[0], vv[1], vv[2], vv[3]);
    // rezero: the gradient buffer goes back to the zero pool (_gradpool.py) -- only the touched 128-byte lines are written
    if (rezero && ug_line_any(g0.x != 0.f || g0.y != 0.f || g0.z != 0.f || g0.w != 0.f))
      *(float4 *)(grad + idx) = make_float4(0.f, 0.f, 0.f, 0.f);     // (a 128-byte line lies inside one 256-byte bitmap line)
  } else {
    *(float4 *)(grad + idx) = make_float4(out[0], out[1], out[2], out[3]);
  }
}

template <bool DENSE, int ADAM, int XCD>
__global__ void __launch_bounds__(256)
k_tv_vec4(const float *__restrict__ param, float *__restrict__ param_out, float *__restrict__ grad,
          float *__restrict__ exp_avg, float *__restrict__ exp_avg_sq, float wy, float wz, int sz_i, int sz_j,
          int sz_k, unsigned n4, float step_size, float beta1, float beta2, float eps, int rezero) {
  const unsigned q = ug_xcd_block<XCD>() * blockDim.x + threadIdx.x;
  if (q >= n4) return;
  ug_tv_lane<false, DENSE, ADAM, XCD>(param, param_out, grad, exp_avg, exp_avg_sq, wy, wz, sz_i, sz_j, sz_k, 4, q, step_size, beta1,
                                      beta2, eps, rezero, true);
}

template <bool DENSE, int ADAM, int XCD>
__global__ void __launch_bounds__(256)
k_tv_cl_vec4(const float *__restrict__ param, float *__restrict__ param_out, float *__restrict__ grad,
             float *__restrict__ exp_avg, float *__restrict__ exp_avg_sq, float wy, float wz, int sz_i, int sz_j,
             int sz_k, int C, unsigned n4, float step_size, float beta1, float beta2, float eps, int rezero,
             const uint32_t *__restrict__ touch) {
  const unsigned q = ug_xcd_block<XCD>() * blockDim.x + threadIdx.x;
  if (q >= n4) return;
  ug_tv_lane<true, DENSE, ADAM, XCD>(param, param_out, grad, exp_avg, exp_avg_sq, wy, wz, sz_i, sz_j, sz_k, C, q, step_size, beta1, beta2,
                                     eps, rezero, ug_touched(touch, q));
}

// SLAB ORDER of the fused dense pass (round 5, tv_xcd = 3).  The linear walk fetches every i-plane of the parameter about THREE times
// from memory: the i-1 / i+1 neighbours of a voxel are a whole plane away (Y x Z x C x 4 B = 1.9 MB at S3's k0 grid), a parameter
// line would have to survive two plane-times in an XCD's 4 MB L2 beside four streaming arrays, and the request counters show it
// does not -- 20.7 GB read per launch where 13.8 GB are needed, 31.0 GB moved in 4.31 ms = 7.2 TB/s of fabric traffic for 5.6 TB/s of
// useful bytes (profiles/r05/tv_adam_dense_pmc.txt).  Here the SAME one-float4-per-lane kernel visits the array in slabs of JW rows
// of j: workgroup b -> (level, slab, i, chunk of the slab's row run) with the chunk fastest, then i, then the slab -- three
// consecutive i-planes of a slab are 3 x JW x Z x C x 4 B = 720 KB and stay in L2, a slab's two boundary rows are the only lines
// read twice (8 %).  Same loads, same expression per element: bit-identical results.  (A variant that walked along i inside a
// workgroup with the three centre values in registers cut the reads to 14.2 GB as well but ran 10 % SLOWER: every step of every
// resident workgroup jumped 1.9 MB in seven arrays -- profiles/r05/tv_adam_dense_ab.txt.)
struct ug_tv_slab { unsigned jw, n_slab, blocks_per_row_run, row4; };      // row4 = Z x C / 4 float4 per j-row

template <int ADAM>
__global__ void __launch_bounds__(256)
k_tv_cl_slab(const float *__restrict__ param, float *__restrict__ param_out, float *__restrict__ grad,
             float *__restrict__ exp_avg, float *__restrict__ exp_avg_sq, float wy, float wz, int sz_i, int sz_j,
             int sz_k, int C, unsigned n4, ug_tv_slab sl, float step_size, float beta1, float beta2, float eps, int rezero,
             const uint32_t *__restrict__ touch) {
  const unsigned b = ug_xcd_block<1>();
  const unsigned chunk = b % sl.blocks_per_row_run, r1 = b / sl.blocks_per_row_run;
  const unsigned i = r1 % (unsigned)sz_i, r2 = r1 / (unsigned)sz_i;
  const unsigned slab = r2 % sl.n_slab, level = r2 / sl.n_slab;
  const unsigned j0 = slab * sl.jw, rows = min(sl.jw, (unsigned)sz_j - j0);
  const unsigned within = chunk * 256u + threadIdx.x;
  if (within >= rows * sl.row4) return;
  const unsigned q = ((level * (unsigned)sz_i + i) * (unsigned)sz_j + j0) * sl.row4 + within;
  if (q >= n4) return;
  ug_tv_lane<true, true, ADAM, 2>(param, param_out, grad, exp_avg, exp_avg_sq, wy, wz, sz_i, sz_j, sz_k, C, q, step_size, beta1, beta2,
                                  eps, rezero, ug_touched(touch, q));
}

// The slab geometry of a [levels][sz_i][sz_j][sz_k][C] array and its workgroup count; 0 = walk it in linear order.  Slab order
// pays when an i-plane is too large to stay in L2 across two plane-times: >= 512 KB per plane
static int64_t ug_tv_slab_geometry(int64_t sz_i, int64_t sz_j, int64_t sz_k, int64_t C, int64_t N, ug_tv_slab &sl) {
  const int64_t row4 = sz_k * C / 4, plane_bytes = sz_j * row4 * 16;
  if (sz_i < 4 || sz_j < 16 || plane_bytes < (512 << 10) || N % (sz_i * sz_j * row4 * 4) != 0) return 0;
  sl.row4 = (unsigned)row4;
  // rows per slab: three slab-planes (+ the streams' working set) well inside the 4 MB L2 -> about 256 KB per slab-plane
  int64_t jw = (256 << 10) / (row4 * 16);
  jw = jw < 4 ? 4 : (jw > sz_j ? sz_j : jw);
  sl.jw = (unsigned)jw;
  sl.n_slab = (unsigned)((sz_j + jw - 1) / jw);
  sl.blocks_per_row_run = (unsigned)((jw * row4 + 255) / 256);
  const int64_t levels = N / (sz_i * sz_j * row4 * 4);
  const int64_t blocks = levels * sl.n_slab * sz_i * sl.blocks_per_row_run;
  return blocks < ((int64_t)1 << 31) ? blocks : 0;
}

// RZ (masked mode only): the gradient is overwritten with zeros after use, whole 128-byte lines at a time and only
// those that held something -- the buffer goes back to the zero pool of the grid's backward (_gradpool.py)
template <int MODE, bool RZ>
__device__ __forceinline__ void ug_adam_vec4_one(float4 *__restrict__ param, const float4 *__restrict__ grad, float4 *__restrict__ exp_avg,
                                                 float4 *__restrict__ exp_avg_sq, const float4 *__restrict__ perlr, int64_t i,
                                                 float step_size, float beta1, float beta2, float eps) {
  const float4 g = grad[i];
  if (RZ && ug_line_any(g.x != 0.f || g.y != 0.f || g.z != 0.f || g.w != 0.f))
    const_cast<float4 *>(grad)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (MODE == 1 && g.x == 0.f && g.y == 0.f && g.z == 0.f && g.w == 0.f) return;
  float4 p = param[i], m = exp_avg[i], v = exp_avg_sq[i];
  float4 l = make_float4(1.f, 1.f, 1.f, 1.f);
  if (MODE == 2) l = perlr[i];
  if (MODE != 1 || g.x != 0.f) ug_adam_one<MODE>(p.x, g.x, m.x, v.x, l.x, step_size, beta1, beta2, eps);
  if (MODE != 1 || g.y != 0.f) ug_adam_one<MODE>(p.y, g.y, m.y, v.y, l.y, step_size, beta1, beta2, eps);
  if (MODE != 1 || g.z != 0.f) ug_adam_one<MODE>(p.z, g.z, m.z, v.z, l.z, step_size, beta1, beta2, eps);
  if (MODE != 1 || g.w != 0.f) ug_adam_one<MODE>(p.w, g.w, m.w, v.w, l.w, step_size, beta1, beta2, eps);
  param[i] = p;
  exp_avg[i] = m;
  exp_avg_sq[i] = v;
}

template <int MODE, bool RZ = false>
__global__ void __launch_bounds__(256)
k_adam_vec4(float4 *__restrict__ param, const float4 *__restrict__ grad, float4 *__restrict__ exp_avg,
            float4 *__restrict__ exp_avg_sq, const float4 *__restrict__ perlr, int64_t n4,
            float step_size, float beta1, float beta2, float eps) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
       i += (int64_t)gridDim.x * blockDim.x)
    ug_adam_vec4_one<MODE, RZ>(param, grad, exp_avg, exp_avg_sq, perlr, i, step_size, beta1, beta2, eps);
}

template <int MODE, bool RZ = false>
__global__ void k_adam_scalar(float *__restrict__ param, const float *__restrict__ grad,
                              float *__restrict__ exp_avg, float *__restrict__ exp_avg_sq,
                              const float *__restrict__ perlr, int64_t begin, int64_t N,
                              float step_size, float beta1, float beta2, float eps) {
  const int64_t i = begin + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const float g = grad[i];
  if (RZ && g != 0.f) const_cast<float *>(grad)[i] = 0.f;
  if (MODE == 1 && !(g != 0.f)) return;
  float p = param[i], m = exp_avg[i], v = exp_avg_sq[i];
  ug_adam_one<MODE>(p, g, m, v, MODE == 2 ? perlr[i] : 1.f, step_size, beta1, beta2, eps);
  param[i] = p;
  exp_avg[i] = m;
  exp_avg_sq[i] = v;
}

// Walk over the touched-line bitmap of a recycled gradient (k_grid_query_backward).  One wave owns 64 consecutive 32-bit words
// (= 2 048 lines of 256 bytes): every lane fetches one word, a ballot finds the words that hold anything, and the wave visits those in
// turn -- a word's set bits dealt to the wave's four 16-lane quarters, so a word with <= 4 marked lines costs one round.  `q` handed to
// the body is the float4 index of the lane.  (Until round 6 a wave owned ONE word: at a few per cent of the lines marked most of the
// 4e5 waves of S3's k0 grid lived for one load and an exit, and the kernel's time was its wave count times a memory latency.)
// wpw = words per wave (1..64): ug_touch_wpw keeps >= ~16 k waves in the launch (a small grid must not be walked by a handful of waves)
static inline int ug_touch_wpw(int64_t n_words) {
  int w = 64;
  while (w > 1 && n_words / w < 16384) w >>= 1;
  return w;
}
#define UG_TOUCH_WALK(touch, n_words, n4, wpw, BODY)                                                                   \
  {                                                                                                                    \
    const int64_t w0 = (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6) * (wpw);                                \
    if (w0 >= (n_words)) return;                                                                                       \
    const int64_t wi = w0 + ug_lane();                                                                                 \
    const bool have = ug_lane() < (wpw) && wi < (n_words);                                                             \
    const uint32_t mine = (touch)[have ? wi : w0] * (have ? 1u : 0u);                                                  \
    unsigned long long nz = __ballot(mine != 0u);                                                                      \
    const int quarter = ug_lane() >> 4;                                                                                \
    while (nz != 0ull) {                                                                                               \
      const int src = __builtin_ctzll(nz);                                                                             \
      nz &= nz - 1ull;                                                                                                 \
      const uint32_t mask = (uint32_t)__builtin_amdgcn_readlane((int)mine, src);                                       \
      const int64_t word = w0 + src;                                                                                   \
      const int cnt = __popc(mask);                                                                                    \
      for (int base = 0; base < cnt; base += 4) {                                                                      \
        const int k = base + quarter;                                                                                  \
        uint32_t m = mask;                                                                                             \
        for (int i = 0; i < k; ++i) m &= m - 1u;                                                                       \
        const int64_t q = ((word << 5) + (int64_t)(__ffs(m) - 1)) * 16 + (ug_lane() & 15);                             \
        if (k < cnt && q < (int64_t)(n4)) { BODY }                                                                     \
      }                                                                                                                \
    }                                                                                                                  \
  }

// masked Adam on the marked lines only; the gradient comes back all zero (RZ)
__global__ void __launch_bounds__(256)
k_adam_vec4_touch(float4 *__restrict__ param, const float4 *__restrict__ grad, float4 *__restrict__ exp_avg,
                  float4 *__restrict__ exp_avg_sq, int64_t n4, float step_size, float beta1, float beta2, float eps,
                  const uint32_t *__restrict__ touch, int64_t n_words, int wpw) {
  UG_TOUCH_WALK(touch, n_words, n4, wpw, (ug_adam_vec4_one<1, true>(param, grad, exp_avg, exp_avg_sq, nullptr, q, step_size, beta1, beta2, eps));)
}

// masked TV gradient on the marked lines of a recycled gradient
__global__ void __launch_bounds__(256)
k_tv_cl_touch(const float *__restrict__ param, float *__restrict__ grad, float wy, float wz, int sz_i, int sz_j, int sz_k, int C,
              unsigned n4, const uint32_t *__restrict__ touch, int64_t n_words, int wpw) {
  UG_TOUCH_WALK(touch, n_words, n4, wpw, (ug_tv_lane<true, false, 0, 0>(param, nullptr, grad, nullptr, nullptr, wy, wz, sz_i, sz_j, sz_k, C,
                                                                     (unsigned)q, 0.f, 0.f, 0.f, 0.f, 0, true));)
}

// ---- multi-tensor Adam (round 5): the small parameters of a model (the rgbnet's six tensors: 22 k elements) in ONE launch instead
// of one launch -- and one host round trip through the binding -- each (masked_adam.py:43-75 loops over the parameters; a DVGO
// training step spent 0.25 ms of its 1.3 ms issuing eight such updates).  Element for element the arithmetic of ugrid_adam_upd
// (ug_adam_one), so the results are bit-identical to the per-tensor calls.
#define UG_ADAM_MULTI_MAX 16
struct ug_adam_table {
  float *param[UG_ADAM_MULTI_MAX];
  const float *grad[UG_ADAM_MULTI_MAX];
  float *m[UG_ADAM_MULTI_MAX], *v[UG_ADAM_MULTI_MAX];
  float step_size[UG_ADAM_MULTI_MAX];
  int32_t first_block[UG_ADAM_MULTI_MAX + 1];      // blocks [first_block[t], first_block[t+1]) work on tensor t
  int64_t numel[UG_ADAM_MULTI_MAX];
  int32_t n;
};

template <int MODE>
__global__ void __launch_bounds__(256) k_adam_multi(ug_adam_table tab, float beta1, float beta2, float eps) {
  int t = 0;
  while (t + 1 < tab.n && (int)blockIdx.x >= tab.first_block[t + 1]) ++t;     // wave-uniform, <= 16 steps
  const int64_t i = (int64_t)((int)blockIdx.x - tab.first_block[t]) * 256 + threadIdx.x;
  if (i >= tab.numel[t]) return;
  const float g = tab.grad[t][i];
  if (MODE == 1 && !(g != 0.f)) return;
  float p = tab.param[t][i], m = tab.m[t][i], v = tab.v[t][i];
  ug_adam_one<MODE>(p, g, m, v, 1.f, tab.step_size[t], beta1, beta2, eps);
  tab.param[t][i] = p;
  tab.m[t][i] = m;
  tab.v[t][i] = v;
}

// ----------------------------------------------------------------------------------------------
// C ABI
// ----------------------------------------------------------------------------------------------
static int g_tv_xcd = 3;   // ugrid_tune("tv_xcd", 0|1|2|3): dense TV (+ Adam) kernels: linear block order | XCD-contiguous | + non-temporal
                           // streams | + slab order of the fused channel-last pass (k_tv_cl_slab, default)
extern "C" int ug_set_tv_xcd(int m) { if (m < 0 || m > 3) return 1; g_tv_xcd = m; return 0; }

// g_tv_xcd as the XCD template argument of a kernel: pick(std::integral_constant<int, XCD>) with XCD = min(g_tv_xcd, MAX).  MAX = 1 for
// the TV-only kernels (the gradient is read and written in place: no non-temporal streams), 2 for the fused passes
template <int MAX, class F>
static inline auto ug_with_tv_xcd(F &&pick) {
  if constexpr (MAX >= 2) {
    if (g_tv_xcd >= 2) return pick(std::integral_constant<int, 2>{});
  }
  if (g_tv_xcd >= 1) return pick(std::integral_constant<int, 1>{});
  return pick(std::integral_constant<int, 0>{});
}

// What every TV entry point does first: wx is ignored and the other two weights are divided by 6, like the reference
// (total_variation_kernel.cu:31-32).  True when the float4 kernels apply: `vec_len` (sz_k canonical, C channel-last) a multiple of 4,
// N < 2^31 (32-bit indices) and all arrays -- `ptrs` = their addresses OR-ed together -- 16-byte aligned
static inline bool ug_tv_prepare(float wx, float &wy, float &wz, int64_t vec_len, int64_t N, uintptr_t ptrs) {
  (void)wx;
  wy /= 6;
  wz /= 6;
  return vec_len % 4 == 0 && N < ((int64_t)1 << 31) && (ptrs & 15) == 0;
}

extern "C" int64_t ugrid_touch_words(int64_t N) { return ((N + 63) / 64 + 31) / 32; }

extern "C" int ugrid_total_variation_add_grad(const float *param, float *grad, float wx, float wy,
                                              float wz, int dense_mode, int64_t sz_i, int64_t sz_j,
                                              int64_t sz_k, int64_t N, ugrid_stream_t s) {
  if (N <= 0) return 0;
  if (ug_tv_prepare(wx, wy, wz, sz_k, N, (uintptr_t)param | (uintptr_t)grad) && sz_i * sz_j * sz_k > 0) {
    const unsigned n4 = (unsigned)(N / 4);
    const auto kernel = !dense_mode ? k_tv_vec4<false, 0, 0> : ug_with_tv_xcd<1>([](auto xcd) { return k_tv_vec4<true, 0, xcd()>; });
    hipLaunchKernelGGL(kernel, dim3((n4 + 255) / 256), dim3(256), 0, ST(s), param, (float *)nullptr, grad, (float *)nullptr,
                       (float *)nullptr, wy, wz, (int)sz_i, (int)sz_j, (int)sz_k, n4, 0.f, 0.f, 0.f, 0.f, 0);
  } else {
    hipLaunchKernelGGL(dense_mode ? k_tv<true> : k_tv<false>, dim3(ug_blocks(N, 256)), dim3(256), 0, ST(s), param, grad, wy, wz,
                       sz_i, sz_j, sz_k, N);
  }
  UG_LAUNCH_CHECK();
  return 0;
}

// channel-last total_variation_add_grad: param / grad are [planes][sz_i][sz_j][sz_k][C] (C % 4 == 0, N < 2^31, 16-byte aligned)
static int ug_tv_cl(const float *param, float *grad, float wx, float wy, float wz, int dense_mode, int64_t sz_i, int64_t sz_j,
                    int64_t sz_k, int64_t C, int64_t N, const uint32_t *touch, ugrid_stream_t s) {
  if (N <= 0) return 0;
  if (!ug_tv_prepare(wx, wy, wz, C, N, (uintptr_t)param | (uintptr_t)grad)) return (int)hipErrorNotSupported;
  const unsigned n4 = (unsigned)(N / 4);
  if (!dense_mode && touch) {
    const int64_t n_words = ugrid_touch_words(N);
    const int wpw = ug_touch_wpw(n_words);
    hipLaunchKernelGGL(k_tv_cl_touch, dim3(ug_blocks((n_words + wpw - 1) / wpw * UG_WAVE, 256)), dim3(256), 0, ST(s), param, grad, wy, wz, (int)sz_i,
                       (int)sz_j, (int)sz_k, (int)C, n4, touch, n_words, wpw);
  } else {
    const auto kernel = !dense_mode ? k_tv_cl_vec4<false, 0, 0> : ug_with_tv_xcd<1>([](auto xcd) { return k_tv_cl_vec4<true, 0, xcd()>; });
    hipLaunchKernelGGL(kernel, dim3((n4 + 255) / 256), dim3(256), 0, ST(s), param, (float *)nullptr, grad, (float *)nullptr,
                       (float *)nullptr, wy, wz, (int)sz_i, (int)sz_j, (int)sz_k, (int)C, n4, 0.f, 0.f, 0.f, 0.f, 0, (const uint32_t *)nullptr);
  }
  UG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ugrid_total_variation_add_grad_cl(const float *param, float *grad, float wx, float wy, float wz, int dense_mode,
                                                 int64_t sz_i, int64_t sz_j, int64_t sz_k, int64_t C, int64_t N,
                                                 ugrid_stream_t s) {
  return ug_tv_cl(param, grad, wx, wy, wz, dense_mode, sz_i, sz_j, sz_k, C, N, nullptr, s);
}

// masked mode with the touched-line bitmap of the gradient (ugrid_grid_query_backward_cl_touch): only marked lines are read
extern "C" int ugrid_total_variation_add_grad_cl_touch(const float *param, float *grad, float wx, float wy, float wz,
                                                       int64_t sz_i, int64_t sz_j, int64_t sz_k, int64_t C, int64_t N,
                                                       const uint32_t *touch, ugrid_stream_t s) {
  return ug_tv_cl(param, grad, wx, wy, wz, 0, sz_i, sz_j, sz_k, C, N, touch, s);
}

extern "C" int ugrid_tv_adam_dense(const float *param, float *param_out, const float *grad, float *exp_avg,
                                   float *exp_avg_sq, float wx, float wy, float wz, int64_t sz_i, int64_t sz_j,
                                   int64_t sz_k, int64_t N, int step, float beta1, float beta2, float lr, float eps,
                                   int flags, ugrid_stream_t s) {
  if (N <= 0) return 0;
  const int skip_zero_grad = flags & 1, rezero = (flags >> 1) & 1;
  const uintptr_t al = (uintptr_t)param | (uintptr_t)param_out | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq;
  if (!ug_tv_prepare(wx, wy, wz, sz_k, N, al) || sz_i * sz_j * sz_k <= 0 || param == param_out)
    return (int)hipErrorNotSupported;   // caller falls back to total_variation_add_grad + adam_upd
  const unsigned n4 = (unsigned)(N / 4);
  // (canonical layout, C = 1: an i-plane is Y x Z floats -- 160 KB at G = 200 -- and stays in L2: no slab order needed)
  const auto kernel = ug_with_tv_xcd<2>([&](auto xcd) { return skip_zero_grad ? k_tv_vec4<true, 1, xcd()> : k_tv_vec4<true, 2, xcd()>; });
  hipLaunchKernelGGL(kernel, dim3((n4 + 255) / 256), dim3(256), 0, ST(s), param, param_out, const_cast<float *>(grad), exp_avg, exp_avg_sq,
                     wy, wz, (int)sz_i, (int)sz_j, (int)sz_k, n4, ug_adam_step_size(lr, beta1, beta2, step), beta1, beta2, eps, rezero);
  UG_LAUNCH_CHECK();
  return 0;
}

static int ug_tv_adam_dense_cl(const float *param, float *param_out, const float *grad, float *exp_avg, float *exp_avg_sq,
                               float wx, float wy, float wz, int64_t sz_i, int64_t sz_j, int64_t sz_k, int64_t C, int64_t N, int step,
                               float beta1, float beta2, float lr, float eps, int flags, uint32_t *touch, ugrid_stream_t s) {
  if (N <= 0) return 0;
  const int skip_zero_grad = flags & 1, rezero = (flags >> 1) & 1;
  const uintptr_t al = (uintptr_t)param | (uintptr_t)param_out | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq;
  if (!ug_tv_prepare(wx, wy, wz, C, N, al) || param == param_out) return (int)hipErrorNotSupported;
  const float step_size = ug_adam_step_size(lr, beta1, beta2, step);
  const unsigned n4 = (unsigned)(N / 4);
  float *g = const_cast<float *>(grad);   // written by the rezero flag only
  ug_tv_slab sl;
  const int64_t slab_blocks = g_tv_xcd == 3 ? ug_tv_slab_geometry(sz_i, sz_j, sz_k, C, N, sl) : 0;
  if (slab_blocks) {
    hipLaunchKernelGGL(skip_zero_grad ? k_tv_cl_slab<1> : k_tv_cl_slab<2>, dim3((unsigned)slab_blocks), dim3(256), 0, ST(s), param,
                       param_out, g, exp_avg, exp_avg_sq, wy, wz, (int)sz_i, (int)sz_j, (int)sz_k, (int)C, n4, sl, step_size, beta1, beta2,
                       eps, rezero, (const uint32_t *)touch);
  } else {
    const auto kernel = ug_with_tv_xcd<2>([&](auto xcd) { return skip_zero_grad ? k_tv_cl_vec4<true, 1, xcd()> : k_tv_cl_vec4<true, 2, xcd()>; });
    hipLaunchKernelGGL(kernel, dim3((n4 + 255) / 256), dim3(256), 0, ST(s), param, param_out, g, exp_avg, exp_avg_sq, wy, wz, (int)sz_i,
                       (int)sz_j, (int)sz_k, (int)C, n4, step_size, beta1, beta2, eps, rezero, (const uint32_t *)touch);
  }
  UG_LAUNCH_CHECK();
  if (touch && rezero) UG_HIP(hipMemsetAsync(touch, 0, sizeof(uint32_t) * (size_t)ugrid_touch_words(N), ST(s)));
  return 0;
}

extern "C" int ugrid_tv_adam_dense_cl(const float *param, float *param_out, const float *grad, float *exp_avg,
                                      float *exp_avg_sq, float wx, float wy, float wz, int64_t sz_i, int64_t sz_j,
                                      int64_t sz_k, int64_t C, int64_t N, int step, float beta1, float beta2, float lr,
                                      float eps, int flags, ugrid_stream_t s) {
  return ug_tv_adam_dense_cl(param, param_out, grad, exp_avg, exp_avg_sq, wx, wy, wz, sz_i, sz_j, sz_k, C, N, step, beta1, beta2, lr,
                             eps, flags, nullptr, s);
}

// + the touched-line bitmap of the gradient: lines not marked are known to be zero and are not read; with the rezero flag
// the bitmap is cleared after the pass (the gradient is all zero again)
extern "C" int ugrid_tv_adam_dense_cl_touch(const float *param, float *param_out, const float *grad, float *exp_avg,
                                            float *exp_avg_sq, float wx, float wy, float wz, int64_t sz_i, int64_t sz_j,
                                            int64_t sz_k, int64_t C, int64_t N, int step, float beta1, float beta2, float lr,
                                            float eps, int flags, uint32_t *touch, ugrid_stream_t s) {
  return ug_tv_adam_dense_cl(param, param_out, grad, exp_avg, exp_avg_sq, wx, wy, wz, sz_i, sz_j, sz_k, C, N, step, beta1, beta2, lr,
                             eps, flags, touch, s);
}

template <int MODE, bool RZ = false>
static int ug_adam_launch(float *param, const float *grad, float *m, float *v, const float *perlr,
                          int64_t N, float step_size, float b1, float b2, float eps, hipStream_t st) {
  const uintptr_t al = (uintptr_t)param | (uintptr_t)grad | (uintptr_t)m | (uintptr_t)v |
                       (MODE == 2 ? (uintptr_t)perlr : 0);
  int64_t done = 0;
  if ((al & 15) == 0 && N >= 4) {
    const int64_t n4 = N / 4;
    // one float4 per lane, no grid-stride loop: measured against the reference's own one-element-per-thread kernels on
    // the same MI355X (tools/bench_dropin_ops.py), a capped grid of 32 blocks per CU streamed 672 M voxels at
    // 5.5 TB/s where the plain huge grid reaches > 6 TB/s (the loop only serialises independent 16-byte streams)
    const int64_t blocks = (n4 + 255) / 256;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_adam_vec4<MODE, RZ>), dim3((unsigned)blocks), dim3(256), 0, st,
                       (float4 *)param, (const float4 *)grad, (float4 *)m, (float4 *)v,
                       (const float4 *)perlr, n4, step_size, b1, b2, eps);
    done = n4 * 4;
  }
  if (done < N)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_adam_scalar<MODE, RZ>), dim3(ug_blocks(N - done, 256)), dim3(256), 0,
                       st, param, grad, m, v, perlr, done, N, step_size, b1, b2, eps);
  UG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ugrid_adam_upd(float *param, const float *grad, float *exp_avg, float *exp_avg_sq,
                              const float *perlr, int64_t N, int step, float beta1, float beta2, float lr,
                              float eps, int mode, ugrid_stream_t s) {
  if (N <= 0) return 0;
  const float step_size = ug_adam_step_size(lr, beta1, beta2, step);
  switch (mode) {
    case 0: return ug_adam_launch<0>(param, grad, exp_avg, exp_avg_sq, nullptr, N, step_size, beta1, beta2, eps, ST(s));
    case 1: return ug_adam_launch<1>(param, grad, exp_avg, exp_avg_sq, nullptr, N, step_size, beta1, beta2, eps, ST(s));
    case 2:
      if (!perlr) return (int)hipErrorInvalidValue;
      return ug_adam_launch<2>(param, grad, exp_avg, exp_avg_sq, perlr, N, step_size, beta1, beta2, eps, ST(s));
    case 3: return ug_adam_launch<1, true>(param, grad, exp_avg, exp_avg_sq, nullptr, N, step_size, beta1, beta2, eps, ST(s));
    default: return (int)hipErrorInvalidValue;
  }
}

// masked_adam_upd with the touched-line bitmap of a recycled gradient buffer: only marked lines are visited; the gradient
// comes back all zero and the bitmap cleared (mode 3 of ugrid_adam_upd restricted to the marked lines)
extern "C" int ugrid_masked_adam_upd_touch(float *param, float *grad, float *exp_avg, float *exp_avg_sq, int64_t N, int step,
                                           float beta1, float beta2, float lr, float eps, uint32_t *touch, ugrid_stream_t s) {
  if (N <= 0) return 0;
  if (!touch) return (int)hipErrorInvalidValue;
  const float step_size = ug_adam_step_size(lr, beta1, beta2, step);
  const uintptr_t al = (uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq;
  if ((al & 15) != 0) return (int)hipErrorNotSupported;
  const int64_t n4 = N / 4, n_words = ugrid_touch_words(N);
  // one word per wave for the masked Adam: its body is one load and (where the gradient is non-zero) three more -- the many short waves
  // hide that latency better than a few waves walking 16 words each (measured: 0.24 against 0.48 ms on S3's k0 grid, visit V); the TV
  // body's eight loads per element like the longer walk (0.88 -> 0.74 ms)
  const int wpw = 1;
  if (n4 > 0)
    hipLaunchKernelGGL(k_adam_vec4_touch, dim3(ug_blocks((n_words + wpw - 1) / wpw * UG_WAVE, 256)), dim3(256), 0, ST(s), (float4 *)param,
                       (const float4 *)grad, (float4 *)exp_avg, (float4 *)exp_avg_sq, n4, step_size, beta1, beta2, eps, touch, n_words, wpw);
  if (n4 * 4 < N)      // the last 1-3 elements, whatever their line says
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_adam_scalar<1, true>), dim3(1), dim3(256), 0, ST(s), param, grad, exp_avg, exp_avg_sq,
                       (const float *)nullptr, n4 * 4, N, step_size, beta1, beta2, eps);
  UG_LAUNCH_CHECK();
  UG_HIP(hipMemsetAsync(touch, 0, sizeof(uint32_t) * (size_t)n_words, ST(s)));
  return 0;
}

extern "C" int ugrid_adam_upd_multi(const ugrid_adam_item *items, int32_t n_items, float beta1, float beta2, float eps,
                                    int32_t mode, ugrid_stream_t s) {
  if (n_items <= 0) return 0;
  if (!items || (mode != 0 && mode != 1)) return (int)hipErrorInvalidValue;
  for (int32_t base = 0; base < n_items; base += UG_ADAM_MULTI_MAX) {
    ug_adam_table tab;
    tab.n = 0;
    int64_t blocks = 0;
    for (int32_t k = base; k < n_items && tab.n < UG_ADAM_MULTI_MAX; ++k) {
      const ugrid_adam_item &it = items[k];
      if (it.numel <= 0) continue;
      if (!it.param || !it.grad || !it.exp_avg || !it.exp_avg_sq || it.numel > ((int64_t)1 << 30)) return (int)hipErrorInvalidValue;
      const int t = tab.n++;
      tab.param[t] = it.param; tab.grad[t] = it.grad; tab.m[t] = it.exp_avg; tab.v[t] = it.exp_avg_sq;
      tab.numel[t] = it.numel;
      tab.step_size[t] = ug_adam_step_size(it.lr, beta1, beta2, it.step);
      tab.first_block[t] = (int32_t)blocks;
      blocks += (it.numel + 255) / 256;
    }
    if (tab.n == 0) continue;
    tab.first_block[tab.n] = (int32_t)blocks;
    hipLaunchKernelGGL(mode == 0 ? k_adam_multi<0> : k_adam_multi<1>, dim3((unsigned)blocks), dim3(256), 0, ST(s), tab, beta1, beta2, eps);
    UG_LAUNCH_CHECK();
  }
  return 0;
}
