// Screening of sampled structures on the device (chm_screen_*, include/chemeleon_hip.h): per crystal the cell
// parameters, the shortest interatomic distance under periodic boundaries (exact for any cell, not only over the
// 27 neighbouring cells), the formula units and the pass / fail flags of the reference's test_valid
// (scripts/evaluate.py) and composition filter (scripts/sample_target_composition.py), one 64-byte record each.
// The plan (chm_screen) is independent of chm_model / chm_batch, like chm_snapshot: node offsets, uploaded once.
//
// The shortest distance is searched in two passes. Pass 1 takes, per pair i < j, the fractional difference
// wrapped to [-0.5, 0.5] and its 27 images; its minimum d0 bounds the crystal's answer from above. A vector
// (w + n) L with |w_k| <= 0.5 is at least |w_k + n_k| h_k long, h_k = volume / |L_{k+1} x L_{k+2}| being the
// spacing of the lattice planes along axis k, so an image closer than d0 has |n_k| <= 0.5 + d0 / h_k. With
// R_k = floor of that bound (widened by 1e-5 against rounding), pass 1 stands when every R_k <= 1, which is
// the normal case; otherwise pass 2 repeats the search over (2 R_0 + 1)(2 R_1 + 1)(2 R_2 + 1) images with R_k
// capped at kMaxRange. A capped crystal is flagged degenerate and keeps the capped search's value.
#include <hip/hip_runtime.h>

#include <math.h>

#include <cstdint>
#include <string>
#include <vector>

#include "chm_host.h"
#include "plan_common.h"

// Distances are fp32 with every product and sum rounded on its own, each Cartesian component summed over
// k = 0, 1, 2 in order, so that the record is the same expression on every build (constrain.hip explains why
// the toolchain's __fmul_rn alone does not prevent contraction).
#pragma clang fp contract(off)

namespace {

constexpr int kClasses = 104;  // classes 0..103 (X + 103 elements)
constexpr int kBlock = 256;    // four waves per crystal
constexpr int kTile = 256;     // atoms staged in LDS at a time
constexpr int kMaxRange = 4;   // cap of the image range per axis
constexpr int kNone = 0x7fffffff;

using chm::fail;

// k_state_snapshot's clamp: a class outside [0, 103] is X
__device__ inline int clamp_number(long a) { return (a >= 0 && a < kClasses) ? (int)a : 0; }

// the closest pair so far; ties go to the smallest d2, then the smallest i, then the smallest j, a total order,
// so the result does not depend on which thread met which pair
struct Best {
  float d2;
  int i, j;
};
__device__ inline bool closer(float d2, int i, int j, const Best& b) {
  return d2 < b.d2 || (d2 == b.d2 && (i < b.i || (i == b.i && j < b.j)));
}

struct Cell {
  float L[9];
};

struct ScreenArgs {
  const long* a;
  const float* x;
  const float* lat;
  const int* off;
  const int* target;  // reduced counts: NULL, or [104] (stride 0), or [B,104] (stride 104)
  int target_stride;
  float max_length, min_distance;
  chm_screen_record* out;
};

// The minimum over pairs i < j of the crystal and the images n_k in [-R_k, R_k] of |(wrap(f_j - f_i) + n) L|^2.
// Fractional coordinates are staged in LDS in tiles of kTile atoms (larger crystals loop over tile pairs). A
// thread owns (atom j of the j tile, image n) and walks the i tile: every lane reads the same LDS address per
// iteration (a broadcast), its own j stays in registers.
__device__ Best search(const float* __restrict__ x, int n0, int n, const Cell& c, int R0, int R1, int R2,
                       float* s_fi, float* s_fj, Best* s_red) {
  const int tid = threadIdx.x;
  const int S1 = 2 * R1 + 1, S2 = 2 * R2 + 1;
  const int M = (2 * R0 + 1) * S1 * S2;
  Best best{INFINITY, kNone, kNone};
  for (int tj0 = 0; tj0 < n; tj0 += kTile) {  // (n is uniform over the block: every barrier is reached by all)
    const int cntj = min(n - tj0, kTile);
    __syncthreads();
    for (int k = tid; k < 3 * cntj; k += kBlock) s_fj[k] = x[3 * ((long)n0 + tj0) + k];
    for (int ti0 = 0; ti0 <= tj0; ti0 += kTile) {
      const int cnti = min(n - ti0, kTile);
      const bool diag = ti0 == tj0;
      __syncthreads();
      if (!diag)
        for (int k = tid; k < 3 * cnti; k += kBlock) s_fi[k] = x[3 * ((long)n0 + ti0) + k];
      __syncthreads();
      const float* fi = diag ? s_fj : s_fi;
      const int items = cntj * M;
      for (int w = tid; w < items; w += kBlock) {
        const int m = w / cntj, jl = w - m * cntj;
        const int m0 = m / (S1 * S2), m12 = m - m0 * (S1 * S2);
        const int m1 = m12 / S2, m2 = m12 - m1 * S2;
        const float e0 = (float)(m0 - R0), e1 = (float)(m1 - R1), e2 = (float)(m2 - R2);
        const int j = tj0 + jl;
        const float xj0 = s_fj[3 * jl], xj1 = s_fj[3 * jl + 1], xj2 = s_fj[3 * jl + 2];
        const int iend = min(cnti, j - ti0);  // i < j
        for (int il = 0; il < iend; ++il) {
          float w0 = xj0 - fi[3 * il], w1 = xj1 - fi[3 * il + 1], w2 = xj2 - fi[3 * il + 2];
          w0 = (w0 - rintf(w0)) + e0;
          w1 = (w1 - rintf(w1)) + e1;
          w2 = (w2 - rintf(w2)) + e2;
          const float c0 = (w0 * c.L[0] + w1 * c.L[3]) + w2 * c.L[6];
          const float c1 = (w0 * c.L[1] + w1 * c.L[4]) + w2 * c.L[7];
          const float c2 = (w0 * c.L[2] + w1 * c.L[5]) + w2 * c.L[8];
          const float d2 = (c0 * c0 + c1 * c1) + c2 * c2;
          if (closer(d2, ti0 + il, j, best)) best = Best{d2, ti0 + il, j};
        }
      }
    }
  }
  // the wave's minimum by shuffles, then the four waves' through LDS
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float od = __shfl_xor(best.d2, o, 64);
    const int oi = __shfl_xor(best.i, o, 64);
    const int oj = __shfl_xor(best.j, o, 64);
    if (closer(od, oi, oj, best)) best = Best{od, oi, oj};
  }
  __syncthreads();  // (s_red may still be read from the previous pass)
  if ((tid & 63) == 0) s_red[tid >> 6] = best;
  __syncthreads();
  best = s_red[0];
#pragma unroll
  for (int wv = 1; wv < kBlock / 64; ++wv) {
    const Best o = s_red[wv];
    if (closer(o.d2, o.i, o.j, best)) best = o;
  }
  return best;
}

__device__ inline float dot3(const float* u, const float* v) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }
__device__ inline void cross3(const float* u, const float* v, float* o) {
  o[0] = u[1] * v[2] - u[2] * v[1];
  o[1] = u[2] * v[0] - u[0] * v[2];
  o[2] = u[0] * v[1] - u[1] * v[0];
}
__device__ inline float angle_deg(const float* u, const float* v, float lu, float lv) {
  const float d = lu * lv;
  if (!(d > 0.f)) return 90.f;  // (a zero row: schema.cell_parameters' convention)
  const float cs = fminf(fmaxf(dot3(u, v) / d, -1.f), 1.f);
  return acosf(cs) * 57.29577951308232f;
}
// the image range along one axis for the bound d0 and the plane spacing h; *capped if it exceeds kMaxRange
__device__ inline int image_range(float d0, float h, bool* capped) {
  const float r = (0.5f + d0 / h) * (1.0f + 1.0e-5f);
  if (!(r < (float)(kMaxRange + 1))) {  // (also NaN and inf)
    *capped = true;
    return kMaxRange;
  }
  return (int)floorf(r);
}

// Block g (four waves) = crystal g: atoms [off[g], off[g + 1]).
__global__ __launch_bounds__(kBlock) void k_screen(ScreenArgs p) {
  __shared__ float s_fi[3 * kTile], s_fj[3 * kTile];
  __shared__ int s_cnt[kClasses];
  __shared__ Best s_red[kBlock / 64];
  __shared__ int s_bad;
  const int g = blockIdx.x, tid = threadIdx.x;
  const int n0 = p.off[g], n = p.off[g + 1] - n0;
  for (int k = tid; k < kClasses; k += kBlock) s_cnt[k] = 0;
  if (tid == 0) s_bad = 0;
  __syncthreads();
  // element counts (LDS adds of integers: the order does not matter) and the finiteness of the inputs
  bool bad = false;
  for (int i = tid; i < n; i += kBlock) atomicAdd(&s_cnt[clamp_number(p.a[n0 + i])], 1);
  for (int k = tid; k < 3 * n; k += kBlock) bad |= !isfinite(p.x[3 * (long)n0 + k]);
  Cell c;
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    c.L[q] = p.lat[(long)g * 9 + q];
    bad |= !isfinite(c.L[q]);
  }
  if (bad) s_bad = 1;
  // the cell (every thread computes the same values)
  const float la = sqrtf(dot3(c.L, c.L)), lb = sqrtf(dot3(c.L + 3, c.L + 3)), lc = sqrtf(dot3(c.L + 6, c.L + 6));
  float x12[3], x20[3], x01[3];
  cross3(c.L + 3, c.L + 6, x12);
  cross3(c.L + 6, c.L, x20);
  cross3(c.L, c.L + 3, x01);
  const float vol = fabsf(dot3(c.L, x12));
  const float h0 = vol / sqrtf(dot3(x12, x12)), h1 = vol / sqrtf(dot3(x20, x20)), h2 = vol / sqrtf(dot3(x01, x01));

  Best best = search(p.x, n0, n, c, 1, 1, 1, s_fi, s_fj, s_red);
  bool degenerate = !(vol > 0.f);
  if (n > 1 && !degenerate) {
    const float d0 = sqrtf(best.d2);
    bool capped = false;
    const int R0 = image_range(d0, h0, &capped), R1 = image_range(d0, h1, &capped),
              R2 = image_range(d0, h2, &capped);
    degenerate = capped;
    if (R0 > 1 || R1 > 1 || R2 > 1)  // (uniform over the block: d0 and the cell are)
      best = search(p.x, n0, n, c, max(R0, 1), max(R1, 1), max(R2, 1), s_fi, s_fj, s_red);
  }
  __syncthreads();  // s_cnt and s_bad are complete (search has barriers of its own unless n == 0)
  if (tid != 0) return;
  int units = 0;
  for (int z = 0; z < kClasses; ++z) {
    int u = units, v = s_cnt[z];
    while (v) {
      const int t = u % v;
      u = v;
      v = t;
    }
    units = u;
  }
  int flags = 0;
  const bool found = best.i != kNone;
  const float dmin = found ? sqrtf(best.d2) : INFINITY;
  if (fmaxf(fmaxf(la, lb), lc) > p.max_length) flags |= CHM_SCREEN_TOO_LONG;
  if (dmin < p.min_distance) flags |= CHM_SCREEN_TOO_CLOSE;
  if (p.target) {
    const int* tg = p.target + (long)g * p.target_stride;
    bool same = units > 0;
    for (int z = 0; z < kClasses && same; ++z) same = s_cnt[z] == tg[z] * units;
    if (!same) flags |= CHM_SCREEN_COMPOSITION;
  }
  if (degenerate) flags |= CHM_SCREEN_DEGENERATE;
  if (s_bad) flags |= CHM_SCREEN_NONFINITE;
  float4* of = reinterpret_cast<float4*>(p.out + g);
  of[0] = make_float4(la, lb, lc, angle_deg(c.L + 3, c.L + 6, lb, lc));
  of[1] = make_float4(angle_deg(c.L, c.L + 6, la, lc), angle_deg(c.L, c.L + 3, la, lb), vol, dmin);
  reinterpret_cast<int4*>(of)[2] = make_int4(found ? best.i : -1, found ? best.j : -1, units, flags);
  reinterpret_cast<int4*>(of)[3] = make_int4(0, 0, 0, 0);
}

}  // namespace

struct chm_screen : chm::NodePlan {};

extern "C" int chm_screen_create(const int32_t* h_natoms, int num_graphs, chm_screen** out) {
  static_assert(sizeof(chm_screen_record) == 64, "the record is 64 bytes");
  return chm::node_plan_create(h_natoms, num_graphs, {"screen"}, "chm_screen_create", out);
}

extern "C" void chm_screen_destroy(chm_screen* p) { chm::node_plan_destroy(p); }

extern "C" int chm_screen_run(const chm_screen* p, const int64_t* d_atom_types, int64_t n_atom_types,
                              const float* d_frac, int64_t n_frac, const float* d_lattices, int64_t n_lattices,
                              const int32_t* d_target, int64_t n_target, float max_length, float min_distance,
                              void* d_out, size_t n_out_bytes, void* stream) {
  if (!p) return fail(CHM_E_ARG, "screen plan is NULL");
  const chm::Check c{"the screen"};
  int rc, target_stride;
  if ((rc = c.count(d_atom_types, n_atom_types, p->N, "atom_types [N]"))) return rc;
  if ((rc = c.count(d_frac, n_frac, 3 * p->N, "frac [N,3]"))) return rc;
  if ((rc = c.count(d_lattices, n_lattices, 9L * p->B, "lattices [B,3,3]"))) return rc;
  if ((rc = c.broadcast(d_target, n_target, kClasses, p->B, "target", "[B,104]", &target_stride))) return rc;
  if (!(max_length > 0.f)) return fail(CHM_E_ARG, "max_length must be > 0");
  if (!(min_distance > 0.f)) return fail(CHM_E_ARG, "min_distance must be > 0");
  if ((rc = c.count(d_out, (long)n_out_bytes, 64L * p->B, "out", "bytes"))) return rc;
  if ((rc = c.aligned16(d_out, "out"))) return rc;
  ScreenArgs a;
  a.a = reinterpret_cast<const long*>(d_atom_types);
  a.x = d_frac;
  a.lat = d_lattices;
  a.off = p->d_off;
  a.target = d_target;
  a.target_stride = target_stride;
  a.max_length = max_length;
  a.min_distance = min_distance;
  a.out = static_cast<chm_screen_record*>(d_out);
  hipLaunchKernelGGL(k_screen, dim3(p->B), dim3(kBlock), 0, (hipStream_t)stream, a);
  HIPCHK(hipGetLastError());
  return CHM_OK;
}
