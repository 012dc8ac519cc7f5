// Grouping of duplicate structures on the device (chm_dedup_*, include/chemeleon_hip.h, where the fingerprint and
// the grouping rule are defined): k_fingerprint writes per crystal a smooth radial distribution in two channels,
// the reduced element counts and the flags; k_dedup_match compares every pair of fingerprints into a bit matrix;
// k_dedup_lead assigns groups by the leader rule. The plan (chm_dedup) holds node offsets only, like chm_screen;
// chm_dedup_group needs no plan, so fingerprints of several calls group as one list.
//
// k_fingerprint works in rounds of two phases. Phase A: a thread owns (atom j, lattice image) and walks a few
// atoms i; the pairs within r_cut are appended to its wave's list in LDS (position = the wave's count so far +
// the number of hitting lanes below, from one ballot per i), so a list's order depends on the crystal alone.
// Phase B: a thread owns one (channel, bin) and walks the four lists in wave order, adding each pair's term to
// a register. With fewer than 256 bins the lists' entries are dealt round-robin to 256 / bins threads per bin,
// whose sums are added in order at the end. Every bin sum therefore has one fixed order: no float atomics.
#include <hip/hip_runtime.h>

#include <math.h>

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "chm_host.h"
#include "plan_common.h"

// fp32 with every product and sum rounded on its own (screen.hip, constrain.hip): the fingerprint is the same
// expression on every build
#pragma clang fp contract(off)

namespace {

constexpr int kClasses = 104;  // classes 0..103 (X + 103 elements)
constexpr int kBlock = 256;    // four waves per crystal
constexpr int kWaves = kBlock / 64;
constexpr int kTile = 128;     // atoms staged in LDS at a time
constexpr int kMaxRange = 8;   // cap of the image range per axis
constexpr int kChunk = 8;      // atoms i a thread walks per round
constexpr int kListCap = kChunk * 64;  // a wave's list: at most one hit per lane and i
constexpr float kSupport = 6.0f;       // a pair touches the bins within 6 sigma of its distance
constexpr int kMinBins = 8, kMaxBins = 256;
constexpr int kPairTile = 32;  // k_dedup_match: 32 x 32 pairs per block, one word of 32 rows
constexpr int kDimChunk = 64;  // fingerprint entries staged at a time
constexpr int kLeadBlock = 64;  // k_dedup_lead: one wave

using chm::fail;

// k_state_snapshot's clamp: a class outside [0, 103] is X
__device__ inline int clamp_number(long a) { return (a >= 0 && a < kClasses) ? (int)a : 0; }

__device__ inline float dot3(const float* u, const float* v) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }
__device__ inline void cross3(const float* u, const float* v, float* o) {
  o[0] = u[1] * v[2] - u[2] * v[1];
  o[1] = u[2] * v[0] - u[0] * v[2];
  o[2] = u[0] * v[1] - u[1] * v[0];
}
// the image range along one axis for the cut-off and the plane spacing h; *capped if it exceeds kMaxRange
__device__ inline int image_range(float r_cut, float h, bool* capped) {
  const float r = (0.5f + r_cut / h) * (1.0f + 1.0e-5f);
  if (!(r < (float)(kMaxRange + 1))) {  // (also NaN and inf)
    *capped = true;
    return kMaxRange;
  }
  return (int)floorf(r);
}

struct FpArgs {
  const long* a;
  const float* x;
  const float* lat;
  const int* off;
  int K;
  float r_cut, sigma;
  float* fp;    // [B, 2K]
  int* counts;  // [B, 104]
  int* flags;   // [B]
};

// Block g (four waves) = crystal g: atoms [off[g], off[g + 1]).
__global__ __launch_bounds__(kBlock) void k_fingerprint(FpArgs p) {
  __shared__ float s_fi[3 * kTile], s_fj[3 * kTile];
  __shared__ int s_zi[kTile], s_zj[kTile];
  __shared__ float s_d[kWaves][kListCap], s_t[kWaves][kListCap], s_zz[kWaves][kListCap];
  __shared__ int s_n[kWaves];
  __shared__ int s_cnt[kClasses];
  __shared__ int s_bad, s_units;
  __shared__ float s_scale1;
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = p.off[g], n = p.off[g + 1] - n0;
  const int K = p.K, nb = 2 * K;
  for (int k = tid; k < kClasses; k += kBlock) s_cnt[k] = 0;
  if (tid == 0) s_bad = 0;
  __syncthreads();
  // element counts (LDS adds of integers: the order does not matter) and the finiteness of the inputs
  bool bad = false;
  for (int i = tid; i < n; i += kBlock) atomicAdd(&s_cnt[clamp_number(p.a[n0 + i])], 1);
  for (int k = tid; k < 3 * n; k += kBlock) bad |= !isfinite(p.x[3 * (long)n0 + k]);
  float L[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    L[q] = p.lat[(long)g * 9 + q];
    bad |= !isfinite(L[q]);
  }
  if (bad) s_bad = 1;
  __syncthreads();
  if (tid == 0) {
    int units = 0;
    long zs = 0;
    for (int z = 0; z < kClasses; ++z) {
      int u = units, v = s_cnt[z];
      zs += (long)z * v;
      while (v) {
        const int t = u % v;
        u = v;
        v = t;
      }
      units = u;
    }
    s_units = units;
    const float fz = (float)zs;
    s_scale1 = zs > 0 ? (float)n / (fz * fz) : 0.f;  // (1/n) / zbar^2
  }
  __syncthreads();
  for (int z = tid; z < kClasses; z += kBlock) p.counts[(long)g * kClasses + z] = s_cnt[z] / s_units;
  // the cell and the image ranges (every thread computes the same values)
  float x12[3], x20[3], x01[3];
  cross3(L + 3, L + 6, x12);
  cross3(L + 6, L, x20);
  cross3(L, L + 3, x01);
  const float vol = fabsf(dot3(L, x12));
  const float h0 = vol / sqrtf(dot3(x12, x12)), h1 = vol / sqrtf(dot3(x20, x20)), h2 = vol / sqrtf(dot3(x01, x01));
  bool degenerate = !(vol > 0.f);
  const int R0 = image_range(p.r_cut, h0, &degenerate), R1 = image_range(p.r_cut, h1, &degenerate),
            R2 = image_range(p.r_cut, h2, &degenerate);
  const int flags = (degenerate ? CHM_DEDUP_DEGENERATE : 0) | (s_bad ? CHM_DEDUP_NONFINITE : 0);
  if (tid == 0) p.flags[g] = flags;
  float* out = p.fp + (long)g * nb;
  if (flags) {  // (uniform over the block)
    for (int b = tid; b < nb; b += kBlock) out[b] = 0.f;
    return;
  }

  // phase B's ownership: `parts` threads per bin when there are fewer bins than threads, else up to two bins
  // per thread
  const int span = min(nb, kBlock), parts = kBlock / span;
  const int part = tid / span, bin0 = tid - part * span, bin1 = bin0 + kBlock;
  const bool binner = part < parts, has1 = bin1 < nb;
  const float delta = p.r_cut / (float)K, cut = kSupport * p.sigma;
  const float inv2s2 = 1.0f / ((2.0f * p.sigma) * p.sigma);
  const float rk0 = ((float)(bin0 % K) + 0.5f) * delta, rk1 = ((float)(bin1 % K) + 0.5f) * delta;
  const bool ch0 = bin0 >= K;  // channel 1?
  float acc0 = 0.f, acc1 = 0.f;  // (bin1 is always in channel 1: bin1 >= 256 >= K)

  const int S1 = 2 * R1 + 1, S2 = 2 * R2 + 1;
  const int M = (2 * R0 + 1) * S1 * S2;
  const int mzero = (R0 * S1 + R1) * S2 + R2;  // the image R = 0
  const float pi_rc = 3.14159265358979323846f;
  for (int tj0 = 0; tj0 < n; tj0 += kTile) {  // (n, M are uniform over the block: every barrier is reached by all)
    const int cntj = min(n - tj0, kTile);
    for (int ti0 = 0; ti0 < n; ti0 += kTile) {
      const int cnti = min(n - ti0, kTile);
      // (the previous round ended with a barrier: nobody still reads the tiles)
      for (int k = tid; k < 3 * cntj; k += kBlock) s_fj[k] = p.x[3 * ((long)n0 + tj0) + k];
      for (int k = tid; k < cntj; k += kBlock) s_zj[k] = clamp_number(p.a[(long)n0 + tj0 + k]);
      for (int k = tid; k < 3 * cnti; k += kBlock) s_fi[k] = p.x[3 * ((long)n0 + ti0) + k];
      for (int k = tid; k < cnti; k += kBlock) s_zi[k] = clamp_number(p.a[(long)n0 + ti0 + k]);
      __syncthreads();
      const int items = cntj * M;
      for (int w0 = 0; w0 < items; w0 += kBlock) {
        const int w = w0 + tid;
        const bool valid = w < items;
        const int wv = valid ? w : 0;
        const int m = wv / cntj, jl = wv - m * cntj;
        const int m0 = m / (S1 * S2), m12 = m - m0 * (S1 * S2);
        const int m1 = m12 / S2, m2 = m12 - m1 * S2;
        const float e0 = (float)(m0 - R0), e1 = (float)(m1 - R1), e2 = (float)(m2 - R2);
        const int j = tj0 + jl;
        const float xj0 = s_fj[3 * jl], xj1 = s_fj[3 * jl + 1], xj2 = s_fj[3 * jl + 2];
        const int zj = s_zj[jl];
        for (int ic0 = 0; ic0 < cnti; ic0 += kChunk) {
          // ---- phase A: the pairs within r_cut, appended to the wave's list in (i, lane) order
          const int iend = min(cnti, ic0 + kChunk);
          int cnt = 0;  // (uniform over the wave)
          for (int il = ic0; il < iend; ++il) {
            float w0f = xj0 - s_fi[3 * il], w1f = xj1 - s_fi[3 * il + 1], w2f = xj2 - s_fi[3 * il + 2];
            w0f = (w0f - rintf(w0f)) + e0;
            w1f = (w1f - rintf(w1f)) + e1;
            w2f = (w2f - rintf(w2f)) + e2;
            const float c0 = (w0f * L[0] + w1f * L[3]) + w2f * L[6];
            const float c1 = (w0f * L[1] + w1f * L[4]) + w2f * L[7];
            const float c2 = (w0f * L[2] + w1f * L[5]) + w2f * L[8];
            const float d = sqrtf((c0 * c0 + c1 * c1) + c2 * c2);
            const bool hit = valid && d <= p.r_cut && !(ti0 + il == j && m == mzero);
            const unsigned long long mask = __ballot(hit);
            if (hit) {
              const int pos = cnt + __popcll(mask & ((1ull << lane) - 1ull));
              s_d[wave][pos] = d;
              s_t[wave][pos] = 0.5f * (1.0f + cosf((pi_rc * d) / p.r_cut));
              s_zz[wave][pos] = (float)(s_zi[il] * zj);
            }
            cnt += __popcll(mask);
          }
          if (lane == 0) s_n[wave] = cnt;
          __syncthreads();
          // ---- phase B: every bin takes the lists' pairs in order
          if (binner) {
            for (int lw = 0; lw < kWaves; ++lw) {
              const int c = s_n[lw];
              for (int e = part; e < c; e += parts) {
                const float d = s_d[lw][e], tp = s_t[lw][e], zz = s_zz[lw][e];
                const float t0 = d - rk0;
                if (fabsf(t0) <= cut) {
                  float v = expf(-(t0 * t0) * inv2s2) * tp;
                  if (ch0) v = v * zz;
                  acc0 = acc0 + v;
                }
                if (has1) {
                  const float t1 = d - rk1;
                  if (fabsf(t1) <= cut) acc1 = acc1 + (expf(-(t1 * t1) * inv2s2) * tp) * zz;
                }
              }
            }
          }
          __syncthreads();
        }
      }
    }
  }
  // the bins' partial sums in part order, then the normalisation
  float* s_acc = &s_d[0][0];  // (kWaves * kListCap = 2048 floats >= parts * span + 256)
  if (binner) {
    s_acc[part * span + bin0] = acc0;
    if (has1) s_acc[bin1] = acc1;  // (parts = 1, span = 256 here)
  }
  __syncthreads();
  const float inv_n = 1.0f / (float)n, scale1 = s_scale1;
  for (int b = tid; b < nb; b += kBlock) {
    float s = s_acc[b];
    for (int q = 1; q < parts; ++q) s = s + s_acc[q * span + b];
    out[b] = b < K ? s * inv_n : s * scale1;
  }
}

struct MatchArgs {
  int B, D, W;  // crystals, fingerprint entries (2K), words per row of the bit matrix
  const float* fp;
  const int* counts;
  const int* flags;             // NULL: none flagged
  const unsigned char* exclude;  // NULL: none excluded
  float tol2;
  unsigned* match;  // [B, W]: bit h of row g = (g < h and g, h match)
};

// Block (x = word wd, y = row tile): rows g = 32 y .. 32 y + 31 against columns h = 32 wd .. 32 wd + 31. A thread
// owns column tx and rows ty, ty + 8, ty + 16, ty + 24; |F_g - F_h|^2 and both norms are summed over the entries
// in order, staged through LDS in chunks of 64. Every word of the matrix is written (no clearing needed).
__global__ __launch_bounds__(kBlock) void k_dedup_match(MatchArgs p) {
  __shared__ float s_a[kPairTile][kDimChunk + 1], s_b[kPairTile][kDimChunk + 1];
  const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
  const int wd = blockIdx.x, g0 = blockIdx.y * kPairTile, h0 = wd * kPairTile;
  if (h0 + kPairTile - 1 <= g0) {  // no pair g < h in this tile (uniform over the block)
    if (tid < kPairTile && g0 + tid < p.B) p.match[(long)(g0 + tid) * p.W + wd] = 0u;
    return;
  }
  float d2[4] = {0.f, 0.f, 0.f, 0.f}, na[4] = {0.f, 0.f, 0.f, 0.f}, nbh = 0.f;
  for (int c0 = 0; c0 < p.D; c0 += kDimChunk) {
    const int cn = min(kDimChunk, p.D - c0);
    __syncthreads();
    for (int k = tid; k < kPairTile * kDimChunk; k += kBlock) {
      const int r = k / kDimChunk, c = k - r * kDimChunk;
      const bool in = c < cn;
      s_a[r][c] = (in && g0 + r < p.B) ? p.fp[(long)(g0 + r) * p.D + c0 + c] : 0.f;
      s_b[r][c] = (in && h0 + r < p.B) ? p.fp[(long)(h0 + r) * p.D + c0 + c] : 0.f;
    }
    __syncthreads();
    for (int c = 0; c < cn; ++c) {
      const float b = s_b[tx][c];
      nbh = nbh + b * b;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float a = s_a[ty + 8 * q][c], t = a - b;
        d2[q] = d2[q] + t * t;
        na[q] = na[q] + a * a;
      }
    }
  }
  const int h = h0 + tx;
  const bool okh = h < p.B && !(p.flags && p.flags[h]) && !(p.exclude && p.exclude[h]);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = ty + 8 * q, g = g0 + r;
    bool m = okh && g < h && !(p.flags && p.flags[g]) && !(p.exclude && p.exclude[g]) &&
             d2[q] <= p.tol2 * fmaxf(na[q], nbh);
    if (m) {
      const int* cg = p.counts + (long)g * kClasses;
      const int* ch = p.counts + (long)h * kClasses;
      for (int z = 0; z < kClasses && m; ++z) m = cg[z] == ch[z];
    }
    // a wave holds two rows (ty even in lanes 0..31, ty odd in 32..63)
    const unsigned long long bits = __ballot(m);
    if (tx == 0 && g < p.B) p.match[(long)g * p.W + wd] = (unsigned)(bits >> (32 * (ty & 1)));
  }
}

struct LeadArgs {
  int B, W;
  const unsigned* match;
  const int* flags;
  const unsigned char* exclude;
  int* reps;  // workspace [B]: the representatives so far, ascending
  int* group;
  int* count;
};

// One wave. g in index order; the lanes scan the representatives so far for the earliest that matches g.
__global__ __launch_bounds__(kLeadBlock) void k_dedup_lead(LeadArgs p) {
  const int lane = threadIdx.x;
  int nrep = 0;  // (uniform)
  for (int g = 0; g < p.B; ++g) {
    const bool ok = !(p.flags && p.flags[g]) && !(p.exclude && p.exclude[g]);
    int best = 0x7fffffff;
    if (ok)
      for (int q = lane; q < nrep; q += kLeadBlock) {
        const int r = p.reps[q];
        if ((p.match[(long)r * p.W + (g >> 5)] >> (g & 31)) & 1u) best = min(best, r);
      }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o, 64));
    const bool lead = ok && best == 0x7fffffff;
    if (lane == 0) {
      p.group[g] = !ok ? -1 : lead ? g : best;
      p.count[g] = lead ? 1 : 0;
      if (lead) p.reps[nrep] = g;
      if (ok && !lead) p.count[best] = p.count[best] + 1;
    }
    if (lead) ++nrep;
    __syncthreads();  // (lane 0's reps entry is visible to the wave's next scan)
  }
}

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
size_t match_words(int64_t B) { return (size_t)B * (size_t)((B + 31) / 32); }

bool positive_finite(float v) { return v > 0.f && std::isfinite(v); }

}  // namespace

// k_dedup_lead for the units that fill a bit matrix of their own (match.hip's grouping by matching)
hipError_t chm::dedup_lead(int B, int W, const unsigned* match, const int* flags, const unsigned char* exclude, int* reps,
                           int* group, int* count, hipStream_t s) {
  LeadArgs l;
  l.B = B;
  l.W = W;
  l.match = match;
  l.flags = flags;
  l.exclude = exclude;
  l.reps = reps;
  l.group = group;
  l.count = count;
  hipLaunchKernelGGL(k_dedup_lead, dim3(1), dim3(kLeadBlock), 0, s, l);
  return hipGetLastError();
}

struct chm_dedup : chm::NodePlan {};

extern "C" int chm_dedup_create(const int32_t* h_natoms, int num_graphs, chm_dedup** out) {
  return chm::node_plan_create(h_natoms, num_graphs, {"dedup plan"}, "chm_dedup_create", out);
}

extern "C" void chm_dedup_destroy(chm_dedup* p) { chm::node_plan_destroy(p); }

namespace {
const chm::Check check{"the dedup"};
int want_bins(int K) {
  if (K < kMinBins || K > kMaxBins)
    return fail(CHM_E_ARG, "K (bins per channel) must be in [8, 256], got " + std::to_string(K));
  return CHM_OK;
}
}  // namespace

extern "C" int chm_dedup_fingerprint(const chm_dedup* p, const int64_t* d_atom_types, int64_t n_atom_types,
                                     const float* d_frac, int64_t n_frac, const float* d_lattices, int64_t n_lattices,
                                     int K, float r_cut, float sigma, float* d_fp, int64_t n_fp, int32_t* d_counts,
                                     int64_t n_counts, int32_t* d_flags, int64_t n_flags, void* stream) {
  int rc;
  if ((rc = want_bins(K))) return rc;
  if (!positive_finite(r_cut)) return fail(CHM_E_ARG, "r_cut must be positive and finite");
  if (!positive_finite(sigma)) return fail(CHM_E_ARG, "sigma must be positive and finite");
  if (!p) return fail(CHM_E_ARG, "dedup plan is NULL");
  if ((rc = check.count(d_atom_types, n_atom_types, p->N, "atom_types [N]"))) return rc;
  if ((rc = check.count(d_frac, n_frac, 3 * p->N, "frac [N,3]"))) return rc;
  if ((rc = check.count(d_lattices, n_lattices, 9L * p->B, "lattices [B,3,3]"))) return rc;
  if ((rc = check.count(d_fp, n_fp, 2L * K * p->B, "fp [B,2K]"))) return rc;
  if ((rc = check.count(d_counts, n_counts, (long)kClasses * p->B, "counts [B,104]"))) return rc;
  if ((rc = check.count(d_flags, n_flags, p->B, "flags [B]"))) return rc;
  FpArgs a;
  a.a = reinterpret_cast<const long*>(d_atom_types);
  a.x = d_frac;
  a.lat = d_lattices;
  a.off = p->d_off;
  a.K = K;
  a.r_cut = r_cut;
  a.sigma = sigma;
  a.fp = d_fp;
  a.counts = d_counts;
  a.flags = d_flags;
  hipLaunchKernelGGL(k_fingerprint, dim3(p->B), dim3(kBlock), 0, (hipStream_t)stream, a);
  HIPCHK(hipGetLastError());
  return CHM_OK;
}

// the bit matrix [B, ceil(B/32)] words, then the representatives' list [B]
extern "C" size_t chm_dedup_workspace_bytes(int64_t B) {
  if (B <= 0 || B > INT32_MAX) return 0;
  return align_up(match_words(B) * sizeof(unsigned), 16) + (size_t)B * sizeof(int);
}

extern "C" int chm_dedup_group(int64_t B, int K, const float* d_fp, int64_t n_fp, const int32_t* d_counts,
                               int64_t n_counts, const int32_t* d_flags, int64_t n_flags, const uint8_t* d_exclude,
                               int64_t n_exclude, float tol, int32_t* d_group, int64_t n_group, int32_t* d_count,
                               int64_t n_count, void* d_workspace, size_t workspace_bytes, void* stream) {
  if (B <= 0) return fail(CHM_E_ARG, "B must be >= 1");
  if ((B + kPairTile - 1) / kPairTile > 65535)
    return fail(CHM_E_UNSUPPORTED, "more than 65535 * 32 fingerprints in one grouping");
  int rc;
  if ((rc = want_bins(K))) return rc;
  if (!positive_finite(tol)) return fail(CHM_E_ARG, "tol must be positive and finite");
  if ((rc = check.count(d_fp, n_fp, 2L * K * B, "fp [B,2K]"))) return rc;
  if ((rc = check.count(d_counts, n_counts, (long)kClasses * B, "counts [B,104]"))) return rc;
  if ((rc = check.optional(d_flags, n_flags, B, "flags [B]"))) return rc;
  if ((rc = check.optional(d_exclude, n_exclude, B, "exclude [B]"))) return rc;
  if ((rc = check.count(d_group, n_group, B, "group [B]"))) return rc;
  if ((rc = check.count(d_count, n_count, B, "count [B]"))) return rc;
  if ((rc = check.workspace(d_workspace, workspace_bytes, chm_dedup_workspace_bytes(B)))) return rc;
  if (reinterpret_cast<uintptr_t>(d_workspace) % 4) return fail(CHM_E_ARG, "workspace must be 4-byte aligned");
  const int W = (int)((B + 31) / 32);
  unsigned* match = static_cast<unsigned*>(d_workspace);
  int* reps = reinterpret_cast<int*>(static_cast<char*>(d_workspace) + align_up(match_words(B) * sizeof(unsigned), 16));
  MatchArgs m;
  m.B = (int)B;
  m.D = 2 * K;
  m.W = W;
  m.fp = d_fp;
  m.counts = d_counts;
  m.flags = d_flags;
  m.exclude = d_exclude;
  m.tol2 = tol * tol;
  m.match = match;
  hipLaunchKernelGGL(k_dedup_match, dim3(W, W), dim3(kBlock), 0, (hipStream_t)stream, m);
  HIPCHK(hipGetLastError());
  LeadArgs l;
  l.B = (int)B;
  l.W = W;
  l.match = match;
  l.flags = d_flags;
  l.exclude = d_exclude;
  l.reps = reps;
  l.group = d_group;
  l.count = d_count;
  hipLaunchKernelGGL(k_dedup_lead, dim3(1), dim3(kLeadBlock), 0, (hipStream_t)stream, l);
  HIPCHK(hipGetLastError());
  return CHM_OK;
}
