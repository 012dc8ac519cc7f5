// Matching finished structures against reference structures on the device (chm_match_*, include/chemeleon_hip.h):
// per crystal the integer lattice mappings M that carry the scaled reduced cell of the sample onto the reduced cell
// of its reference within ltol / angle_tol, and for each of them the origin shifts t_j that put an atom of the
// rarest species onto the reference's first atom of that species; a candidate (M, t_j) survives when every
// reference atom's nearest sample atom of its type is within stol l and no sample atom is taken twice. The
// survivor with the smallest rms displacement (mean removed) is the record (test_structure_matching of the
// reference's scripts/evaluate.py). One 64-byte record per crystal and, if asked, the winner's atom pairing. The
// plan (chm_match) is independent of chm_model / chm_batch: node offsets of both lists and ref_of, uploaded once.
//
// One 256-thread block per crystal. The reduced coordinates and types of the sample and of its reference (16 bytes
// per atom, at most 256 atoms each) and the accepted mappings (at most 256 candidate indices, appended in ascending
// order pass by pass) are staged in LDS. The candidates (M, t_j) are spread over the block, one thread each, with a
// 256-bit "taken" set per thread in LDS. The winner is a 64-bit integer minimum in LDS over (rms bits, mapping
// position, anchor position), every count an integer add, so the record does not depend on any order.
//
// Grouping a batch by pairwise matching (chm_match_group_*): the same block body (match_block) runs once per pair
// (h, g), h < g, of crystals of one state with equal atom counts (k_match_pairs), crystal h as the reference side;
// a match sets bit g of row h of a bit matrix with one atomicOr, k_dedup_lead (dedup.hip) applies the leader rule
// to the matrix and k_match_group_gather writes each crystal's record against its leader.
#include <hip/hip_runtime.h>

#include <limits.h>
#include <math.h>
#include <string.h>

#include <cstdint>
#include <string>
#include <vector>

#include "chm_host.h"
#include "plan_common.h"
#include "cell_shared.h"

// Every product and sum is rounded on its own (as in cell.hip).
#pragma clang fp contract(off)

namespace {

using namespace chm_cellshared;

constexpr int kBlock = 256;     // four waves per crystal
constexpr int kMaxAtoms = 256;  // the LDS staging
constexpr int kMaxMaps = CHM_MATCH_MAX_MAPPINGS;
constexpr int kNoCell = CHM_CELL_NOT_REDUCED | CHM_CELL_DEGENERATE | CHM_CELL_NONFINITE;

using chm::fail;

struct MatchArgs {
  const chm_cell_record* rec;   // [B] of the samples
  const long long* types;
  const float* x;
  const float* lat;
  const int* off;               // [B + 1]
  const chm_cell_record* rrec;  // [R] of the references
  const long long* rtypes;
  const float* rx;
  const float* rlat;
  const int* roff;              // [R + 1]
  const int* ref_of;            // [B]
  float ltol, stol, angle_tol;
  int4* out;                    // [B] records of 64 bytes
  int* perm;                    // NULL or [N]
};

struct __align__(16) Atom {
  float x[3];  // in the reduced basis, [0, 1)
  int type;
};

// the rows of M A, entries (m0 a0 + m1 a1) + m2 a2
__device__ inline void rows_of(const int* M, const float* A, float* out) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k)
      out[3 * i + k] = ((float)M[3 * i] * A[k] + (float)M[3 * i + 1] * A[3 + k]) + (float)M[3 * i + 2] * A[6 + k];
}

// G(A): the six distinct entries 00, 11, 22, 01, 02, 12
__device__ inline void gram(const float* A, float* g) {
  g[0] = dot3(A, A), g[1] = dot3(A + 3, A + 3), g[2] = dot3(A + 6, A + 6);
  g[3] = dot3(A, A + 3), g[4] = dot3(A, A + 6), g[5] = dot3(A + 3, A + 6);
}

// |d|^2 under the metric g (gram's order): (u0 d0 + u1 d1) + u2 d2, u_k = (d0 G[0][k] + d1 G[1][k]) + d2 G[2][k]
__device__ inline float norm2(const float* g, const float* d) {
  const float u0 = (d[0] * g[0] + d[1] * g[3]) + d[2] * g[4];
  const float u1 = (d[0] * g[3] + d[1] * g[1]) + d[2] * g[5];
  const float u2 = (d[0] * g[4] + d[1] * g[5]) + d[2] * g[2];
  return (u0 * d[0] + u1 * d[1]) + u2 * d[2];
}

// Is candidate idx a unimodular M whose M sL has every row length within ltol (relative) and every inter-row angle
// within atol (degrees) of the reference cell's (lr, ar of cell_metric)?
__device__ inline bool mapping_accepted(int idx, const float* sL, const float* lr, const float* ar, float ltol, float atol) {
  int M[9], det, tr;
  decode_candidate(idx, M, &det, &tr);
  if (det != 1 && det != -1) return false;
  float A[9];
  rows_of(M, sL, A);
  const float m0 = sqrtf(dot3(A, A)), m1 = sqrtf(dot3(A + 3, A + 3)), m2 = sqrtf(dot3(A + 6, A + 6));
  bool acc = fabsf(m0 / lr[0] - 1.f) <= ltol && fabsf(m1 / lr[1] - 1.f) <= ltol && fabsf(m2 / lr[2] - 1.f) <= ltol;
  if (acc)
    acc = fabsf(angle_deg(A + 3, A + 6, m1, m2) - ar[0]) <= atol && fabsf(angle_deg(A, A + 6, m0, m2) - ar[1]) <= atol &&
          fabsf(angle_deg(A, A + 3, m0, m1) - ar[2]) <= atol;
  return acc;
}

// Minv = det(M) adj(M) as floats (entries within +-2), and the metric 0.5 (G(M sL) + gr) of mapping idx
__device__ inline void mapping_frame(int idx, const float* sL, const float* gr, float* Minv, float* g) {
  int M[9], det, tr;
  decode_candidate(idx, M, &det, &tr);
  Minv[0] = (float)(det * (M[4] * M[8] - M[5] * M[7]));
  Minv[1] = (float)(det * (M[2] * M[7] - M[1] * M[8]));
  Minv[2] = (float)(det * (M[1] * M[5] - M[2] * M[4]));
  Minv[3] = (float)(det * (M[5] * M[6] - M[3] * M[8]));
  Minv[4] = (float)(det * (M[0] * M[8] - M[2] * M[6]));
  Minv[5] = (float)(det * (M[2] * M[3] - M[0] * M[5]));
  Minv[6] = (float)(det * (M[3] * M[7] - M[4] * M[6]));
  Minv[7] = (float)(det * (M[1] * M[6] - M[0] * M[7]));
  Minv[8] = (float)(det * (M[0] * M[4] - M[1] * M[3]));
  float A[9], gm[6];
  rows_of(M, sL, A);
  gram(A, gm);
#pragma unroll
  for (int q = 0; q < 6; ++q) g[q] = 0.5f * (gm[q] + gr[q]);
}

// x'' = frac(x' Minv)
__device__ inline void mapped(const float* Minv, const float* x, float* out) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float y = (x[0] * Minv[k] + x[1] * Minv[3 + k]) + x[2] * Minv[6 + k];
    float f = y - floorf(y);
    if (f >= 1.0f) f = 0.0f;
    out[k] = f;
  }
}

// The sample atom of b's type nearest to reference atom b under (Minv, t, g): its index (-1 if none), |D|^2 and D.
__device__ inline int nearest(const Atom* s_s, int n, const Atom b, const float* Minv, const float* t, const float* g,
                              float* best, float* D) {
  int bi = -1;
  *best = INFINITY;
  for (int i = 0; i < n; ++i) {
    const Atom a = s_s[i];
    if (a.type != b.type) continue;
    float xm[3], d[3];
    mapped(Minv, a.x, xm);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      d[k] = (xm[k] - t[k]) - b.x[k];
      d[k] -= rintf(d[k]);
    }
    const float q = norm2(g, d);
    if (q < *best) {
      *best = q, bi = i;
      D[0] = d[0], D[1] = d[1], D[2] = d[2];
    }
  }
  return bi;
}

__device__ inline double det3(const float* L) {
  const double l[9] = {L[0], L[1], L[2], L[3], L[4], L[5], L[6], L[7], L[8]};
  return (l[0] * (l[4] * l[8] - l[5] * l[7]) - l[1] * (l[3] * l[8] - l[5] * l[6])) + l[2] * (l[3] * l[7] - l[4] * l[6]);
}

// ---- optimal assignment of a collided candidate (pairing = CHM_MATCH_PAIRING_ASSIGNMENT), one wave per candidate
constexpr int kMaxAssign = CHM_MATCH_MAX_ASSIGN;
constexpr int kBitWords = kMaxMaps * kMaxAtoms / 32;  // one bit per candidate (M, t_j)

// LDS of one wave: y (the mapped, shifted sample coordinates), the duals u (rows) and v (columns), minv, way and
// row_of_col of the shortest-augmenting-path search, and col (row -> column, in the block's freed "taken" words)
struct AssignLds {
  float* y;  // [3 * kMaxAtoms]
  float* u;
  float* v;
  float* minv;
  int* way;
  int* row_of_col;
  int* col;
};

// The lanes of one wave see each other's LDS writes behind this (LDS operations of a wave complete in order).
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// D = (y_i - xr_k) - rintf(y_i - xr_k) and |D|^2, the arithmetic of nearest()
__device__ __forceinline__ float pair_cost(const float* y, int i, const Atom& b, const float* g, float* D) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    D[k] = y[3 * i + k] - b.x[k];
    D[k] -= rintf(D[k]);
  }
  return norm2(g, D);
}

// The type-preserving bijection of minimal sum |D|^2 under (Minv, t, g) by shortest augmenting paths, and its score.
// Every lane of the wave calls it with the same arguments. Every loop is bounded by n: a row whose search finds no
// column (NaN or Inf costs) ends the solve with false. On true L.col[k] is reference atom k's sample atom and
// (*rms, *maxq) the score, the same in every lane.
__device__ bool assign_solve(const Atom* s_s, const Atom* s_r, const int n, const float* Minv, const float* t, const float* g,
                             const AssignLds& L, const int lane, const float ell, float* rms, float* maxq) {
  for (int i = lane; i < n; i += 64) {
    float xm[3];
    mapped(Minv, s_s[i].x, xm);
#pragma unroll
    for (int k = 0; k < 3; ++k) L.y[3 * i + k] = xm[k] - t[k];
    L.v[i] = 0.f;
    L.row_of_col[i] = -1;
  }
  wave_sync();
  // the dual start: u_k = the row minimum (ties: the smallest column), v = 0
  for (int k = lane; k < n; k += 64) {
    const Atom b = s_r[k];
    float best = INFINITY;
    int bi = -1;
    for (int i = 0; i < n; ++i) {
      if (s_s[i].type != b.type) continue;
      float D[3];
      const float q = pair_cost(L.y, i, b, g, D);
      if (q < best) best = q, bi = i;
    }
    L.u[k] = best;
    L.col[k] = bi;
    if (bi >= 0) atomicMin(reinterpret_cast<unsigned*>(L.row_of_col) + bi, (unsigned)k);  // (-1 is the largest unsigned)
  }
  wave_sync();
  // a column keeps the smallest row that wants it: the non-colliding row minima are placed
  bool whole = true;
  for (int k = lane; k < n; k += 64) {
    const int bi = L.col[k];
    if (bi < 0) whole = false;
    else if (L.row_of_col[bi] != k) L.col[k] = -1;
  }
  if (__ballot(!whole)) return false;  // (a row without a finite cost: the prefilter lets none through)
  wave_sync();
  for (int i = 0; i < n; ++i) {
    if (L.col[i] >= 0) continue;  // (uniform: from LDS behind wave_sync)
    const int ty = s_r[i].type;
    unsigned used = 0u;  // bit q: column lane + 64 q is in the tree
#pragma unroll
    for (int q = 0; q < kMaxAtoms / 64; ++q)
      if (lane + 64 * q < n) L.minv[lane + 64 * q] = INFINITY;
    int i0 = i, j0 = -1;
    bool reached = false;
    for (int step = 0; step < n; ++step) {  // (every step puts one more column into the tree)
      const Atom b = s_r[i0];
      const float ui0 = L.u[i0];
      float ld = INFINITY;
      int lj = INT_MAX;
#pragma unroll
      for (int q = 0; q < kMaxAtoms / 64; ++q) {
        const int j = lane + 64 * q;
        if (j >= n || ((used >> q) & 1u) || s_s[j].type != ty) continue;
        float D[3];
        const float cur = (pair_cost(L.y, j, b, g, D) - ui0) - L.v[j];
        float mv = L.minv[j];
        if (cur < mv) {
          mv = cur;
          L.minv[j] = cur;
          L.way[j] = j0;
        }
        if (mv < ld) ld = mv, lj = j;
      }
      for (int d = 32; d >= 1; d >>= 1) {  // the minimum over the wave, ties to the smallest column
        const float od = __shfl_xor(ld, d, 64);
        const int oj = __shfl_xor(lj, d, 64);
        if (od < ld || (od == ld && oj < lj)) ld = od, lj = oj;
      }
      if (lj == INT_MAX) break;  // no column left with a finite reduced cost
      if (lane == 0) L.u[i] += ld;
#pragma unroll
      for (int q = 0; q < kMaxAtoms / 64; ++q) {
        const int j = lane + 64 * q;
        if (j >= n || s_s[j].type != ty) continue;
        if ((used >> q) & 1u) {
          L.u[L.row_of_col[j]] += ld;  // (the rows of the tree's columns are all different)
          L.v[j] -= ld;
        } else {
          L.minv[j] -= ld;
        }
      }
      if ((lj & 63) == lane) used |= 1u << (lj >> 6);
      wave_sync();
      j0 = lj;
      const int r = L.row_of_col[lj];
      if (r < 0) {
        reached = true;
        break;
      }
      i0 = r;
    }
    if (!reached) return false;  // (uniform: lj and r are the same in every lane)
    if (lane == 0) {
      int j = j0;
      for (int s = 0; s < n && j >= 0; ++s) {  // back along the path: every column takes the row of the one before
        const int jp = L.way[j];
        const int row = jp < 0 ? i : L.row_of_col[jp];
        L.row_of_col[j] = row;
        L.col[row] = j;
        j = jp;
      }
    }
    wave_sync();
  }
  // the score: D_k by the lanes into the freed u, v, minv; the sums in index order in every lane
  for (int k = lane; k < n; k += 64) {
    float D[3];
    (void)pair_cost(L.y, L.col[k], s_r[k], g, D);
    L.u[k] = D[0], L.v[k] = D[1], L.minv[k] = D[2];
  }
  wave_sync();
  float sum[3] = {0.f, 0.f, 0.f};
  for (int k = 0; k < n; ++k) sum[0] += L.u[k], sum[1] += L.v[k], sum[2] += L.minv[k];
  const float fn = (float)n;
  const float mean[3] = {sum[0] / fn, sum[1] / fn, sum[2] / fn};
  float sumq = 0.f, mq = 0.f;
  for (int k = 0; k < n; ++k) {
    const float e[3] = {L.u[k] - mean[0], L.v[k] - mean[1], L.minv[k] - mean[2]};
    const float q = norm2(g, e);
    sumq += q;
    mq = fmaxf(mq, q);
  }
  *rms = sqrtf(sumq / fn) / ell;
  *maxq = mq;
  return true;
}

// LDS integers of the block
enum { I_COMP = 0, I_MINCNT, I_PTYPE, I_PREF, I_VOLOK, I_NSURV, I_COUNT };
// LDS floats of the block
enum { F_SCALE = 0, F_ELL, F_MAXD, F_COUNT };

// One block (four waves) = sample crystal g against reference r. kPairs = false is k_match (the record of 64
// bytes at oi, the pairing in p.perm); kPairs = true is k_match_pairs, where both sides come from one state: the
// compact record {rms, max_dist, flags, matched} at oi[0] and, on a match, `bit` or-ed into *bit_word. kAssign =
// true is the pairing CHM_MATCH_PAIRING_ASSIGNMENT: phase A (a thread per candidate) scores the candidates whose
// nearest partners are all different and marks the others in a bitmap, phase B (a wave per marked candidate, the
// lowest kMaxAssign of them) solves their assignment. kAssign = false holds none of that.
template <bool kPairs, bool kAssign>
__device__ __forceinline__ void match_block(const MatchArgs& p, const int g, const int r, int4* oi, unsigned* bit_word,
                                            unsigned bit) {
  __shared__ Atom s_s[kMaxAtoms];  // the sample
  __shared__ Atom s_r[kMaxAtoms];  // its reference
  __shared__ int s_map[kMaxMaps];  // accepted candidate indices, ascending
  __shared__ int s_piv[kMaxAtoms];  // the sample's atoms of the anchor species in node order
  __shared__ unsigned s_taken[8 * kBlock];  // word w of thread t at [w * kBlock + t]
  __shared__ float s_Ls[9], s_Lr[9], s_f[F_COUNT];
  __shared__ int s_i[I_COUNT], s_wcnt[kBlock / 64];
  __shared__ unsigned long long s_best;
  unsigned* s_bits = nullptr;  // kAssign: bit `cand` = candidate cand is alive and its nearest partners collide
  int* s_list = nullptr;       // kAssign: the lowest marked candidates, ascending
  int* s_nmark = nullptr;      // kAssign: how many are marked
  AssignLds asg = {};
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if constexpr (kAssign) {
    __shared__ unsigned a_bits[kBitWords];
    __shared__ float a_f[kBlock / 64][6 * kMaxAtoms];
    __shared__ int a_i[kBlock / 64][2 * kMaxAtoms];
    __shared__ int a_list[kMaxAssign], a_nmark;
    s_bits = a_bits, s_list = a_list, s_nmark = &a_nmark;
    asg.y = a_f[wave], asg.u = a_f[wave] + 3 * kMaxAtoms, asg.v = asg.u + kMaxAtoms, asg.minv = asg.v + kMaxAtoms;
    asg.way = a_i[wave], asg.row_of_col = a_i[wave] + kMaxAtoms;
    asg.col = reinterpret_cast<int*>(s_taken) + wave * kMaxAtoms;  // (phase A is over when phase B starts)
  }
  const int n0 = p.off[g], n = p.off[g + 1] - n0;  // (1 <= n <= kMaxAtoms: chm_match_create)
  // (r, n, nr and everything read from the cell records are the same in every thread: the branches on them are uniform)
  if constexpr (!kPairs) {
    if (r < 0) {
      if (p.perm && tid < n) p.perm[(long)n0 + tid] = -1;
      if (tid == 0) {
        oi[0] = make_int4(0, 0, 0, 0);
        oi[1] = make_int4(-1, -1, 0, 0);
        oi[2] = make_int4(0, 0, CHM_MATCH_NO_REFERENCE, -1);
        oi[3] = make_int4(0, 0, 0, 0);
      }
      return;
    }
  }
  const int m0 = p.roff[r], nr = p.roff[r + 1] - m0;
  const chm_cell_record* rec = p.rec + g;
  const chm_cell_record* rrec = p.rrec + r;
  int flags = 0;
  if ((rec->flags & kNoCell) || (rrec->flags & kNoCell)) flags |= CHM_MATCH_NO_LATTICE;
  if (n != nr) flags |= CHM_MATCH_SIZE;
  int Ts[9], Tr[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) Ts[q] = rec->transform[q], Tr[q] = rrec->transform[q];

  if (tid < 9) {
    s_Ls[tid] = reduced_entry(Ts, p.lat + (long)g * 9, tid);
    s_Lr[tid] = reduced_entry(Tr, p.rlat + (long)r * 9, tid);
  }
  if (tid < n) {
    double adj[9];
    adjugate(Ts, adj);
    reduced_frac(adj, p.x + 3 * ((long)n0 + tid), s_s[tid].x);
    s_s[tid].type = (int)p.types[(long)n0 + tid];
  }
  if (tid < nr) {
    double adj[9];
    adjugate(Tr, adj);
    reduced_frac(adj, p.rx + 3 * ((long)m0 + tid), s_r[tid].x);
    s_r[tid].type = (int)p.rtypes[(long)m0 + tid];
  }
  if (tid < I_COUNT) s_i[tid] = (tid == I_MINCNT || tid == I_PTYPE || tid == I_PREF) ? INT_MAX : 0;
  if (tid < F_COUNT) s_f[tid] = 0.f;
  if (tid == 0) s_best = ~0ull;
  __syncthreads();

  // ---- composition, and the anchor species: the one with the fewest atoms (ties: the smallest type)
  int n_piv = 0, pref = 0;
  if (n == nr) {
    const int my = tid < n ? s_s[tid].type : 0;
    const int myr = tid < n ? s_r[tid].type : 0;
    int cnt_r = 0;
    if (tid < n) {
      int cs = 0, cr = 0;
      for (int q = 0; q < n; ++q) cs += s_s[q].type == my, cr += s_r[q].type == my, cnt_r += s_r[q].type == myr;
      if (cs != cr) s_i[I_COMP] = 1;
      atomicMin(&s_i[I_MINCNT], cnt_r);
    }
    __syncthreads();
    n_piv = s_i[I_MINCNT];
    if (s_i[I_COMP]) flags |= CHM_MATCH_COMPOSITION;
    if (tid < n && cnt_r == n_piv) atomicMin(&s_i[I_PTYPE], myr);
    __syncthreads();
    const int ptype = s_i[I_PTYPE];
    if (tid < n && myr == ptype) atomicMin(&s_i[I_PREF], tid);
    if (tid < n && my == ptype) {
      int rank = 0;
      for (int q = 0; q < tid; ++q) rank += s_s[q].type == ptype;
      s_piv[rank] = tid;  // (rank < n_piv when the compositions are equal; < n always)
    }
    __syncthreads();
    pref = s_i[I_PREF];
  }

  // ---- scale and l: fp64 on one lane, rounded once
  float Ls[9], Lr[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) Ls[q] = s_Ls[q], Lr[q] = s_Lr[q];
  if (!(flags & CHM_MATCH_NO_LATTICE)) {
    if (tid == 0) {
      const double vs = fabs(det3(Ls)), vr = fabs(det3(Lr));
      const bool ok = vs > 0.0 && vr > 0.0 && vs < INFINITY && vr < INFINITY;
      if (ok) {
        s_f[F_SCALE] = (float)cbrt(vr / vs);
        s_f[F_ELL] = (float)cbrt(vr / (double)nr);
      }
      s_i[I_VOLOK] = ok;
    }
    __syncthreads();
    if (!s_i[I_VOLOK]) flags |= CHM_MATCH_NO_LATTICE;  // (uniform: from LDS behind a barrier)
  }
  const float scale = s_f[F_SCALE], ell = s_f[F_ELL];
  const float c = p.stol * ell, c2 = c * c;

  // ---- thin cells: one image per component is exact only while 2 c < the smallest plane spacing of Lr
  if (flags == 0) {
    const float c0[3] = {Lr[4] * Lr[8] - Lr[5] * Lr[7], Lr[5] * Lr[6] - Lr[3] * Lr[8], Lr[3] * Lr[7] - Lr[4] * Lr[6]};
    const float c1[3] = {Lr[7] * Lr[2] - Lr[8] * Lr[1], Lr[8] * Lr[0] - Lr[6] * Lr[2], Lr[6] * Lr[1] - Lr[7] * Lr[0]};
    const float c2v[3] = {Lr[1] * Lr[5] - Lr[2] * Lr[4], Lr[2] * Lr[3] - Lr[0] * Lr[5], Lr[0] * Lr[4] - Lr[1] * Lr[3]};
    const float vol = fabsf(dot3(Lr, c0));
    const float d0 = vol / sqrtf(dot3(c0, c0)), d1 = vol / sqrtf(dot3(c1, c1)), d2 = vol / sqrtf(dot3(c2v, c2v));
    if (!(2.0f * c < fminf(fminf(d0, d1), d2))) flags |= CHM_MATCH_THIN;
  }
  const bool search = flags == 0;

  // ---- the lattice mappings, appended in ascending candidate order pass by pass
  float sL[9], gr[6];
#pragma unroll
  for (int q = 0; q < 9; ++q) sL[q] = scale * Ls[q];
  gram(Lr, gr);
  int n_maps = 0;
  if (search) {
    float lr[3], ar[3];
    cell_metric(Lr, lr, ar);
    for (int first = 0; first < kCandidates; first += kBlock) {  // (every thread takes every pass: the ballot is whole)
      const int idx = first + tid;
      const bool acc = idx < kCandidates && mapping_accepted(idx, sL, lr, ar, p.ltol, p.angle_tol);
      const unsigned long long b = __ballot(acc);
      if (lane == 0) s_wcnt[wave] = __popcll(b);
      __syncthreads();
      int before = 0, all = 0;
#pragma unroll
      for (int w = 0; w < kBlock / 64; ++w) {
        const int cw = s_wcnt[w];
        before += w < wave ? cw : 0;
        all += cw;
      }
      const int slot = n_maps + before + __popcll(b & ((1ull << lane) - 1ull));
      if (acc && slot < kMaxMaps) s_map[slot] = idx;
      n_maps += all;
      __syncthreads();  // (s_wcnt is rewritten in the next pass; s_map is read after the last)
    }
    if (n_maps > kMaxMaps) flags |= CHM_MATCH_MANY_MAPPINGS;
  }
  const int used = n_maps < kMaxMaps ? n_maps : kMaxMaps;

  // ---- the candidates (M, t_j), one per thread
  const int total = search ? used * n_piv : 0;  // (<= 256 * 256)
  unsigned long long mine = ~0ull;
  float mine_maxd = 0.f;
  if constexpr (kAssign) {
    for (int w = tid; w < (total + 31) / 32; w += kBlock) s_bits[w] = 0u;
    if (tid == 0) *s_nmark = 0;
    __syncthreads();
  }
  for (int cand = tid; cand < total; cand += kBlock) {
    const int w = cand / n_piv, jj = cand - w * n_piv;
    float Minv[9], gm[6], t[3];
    mapping_frame(s_map[w], sL, gr, Minv, gm);
    {
      float xj[3];
      mapped(Minv, s_s[s_piv[jj]].x, xj);
#pragma unroll
      for (int k = 0; k < 3; ++k) t[k] = xj[k] - s_r[pref].x[k];
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) s_taken[q * kBlock + tid] = 0u;
    float sum[3] = {0.f, 0.f, 0.f};
    bool ok = true;
    bool collided = false;  // (kAssign only)
    for (int k = 0; k < n && ok; ++k) {
      float best, D[3];
      const int bi = nearest(s_s, n, s_r[k], Minv, t, gm, &best, D);
      if (!(best <= c2)) {  // (also bi < 0 and NaN)
        ok = false;
      } else {
        const unsigned bit = 1u << (bi & 31);
        const unsigned word = s_taken[(bi >> 5) * kBlock + tid];
        if (word & bit) {
          if constexpr (kAssign) collided = true; else ok = false;  // (the prefilter goes on over the other k)
        } else {
          s_taken[(bi >> 5) * kBlock + tid] = word | bit;
          sum[0] += D[0], sum[1] += D[1], sum[2] += D[2];
        }
      }
    }
    if (!ok) continue;
    atomicAdd(&s_i[I_NSURV], 1);
    if constexpr (kAssign) {
      if (collided) {
        atomicOr(&s_bits[cand >> 5], 1u << (cand & 31));
        continue;
      }
    }
    const float fn = (float)n;
    const float mean[3] = {sum[0] / fn, sum[1] / fn, sum[2] / fn};
    float sumq = 0.f, maxq = 0.f;
    for (int k = 0; k < n; ++k) {
      float best, D[3];
      (void)nearest(s_s, n, s_r[k], Minv, t, gm, &best, D);
      const float e[3] = {D[0] - mean[0], D[1] - mean[1], D[2] - mean[2]};
      const float q = norm2(gm, e);
      sumq += q;
      maxq = fmaxf(maxq, q);
    }
    const float rms = sqrtf(sumq / fn) / ell;
    if (rms <= p.stol) {  // (rms >= 0 or -0: its bits with the sign cleared order as the values do)
      const unsigned long long key =
          ((unsigned long long)(__float_as_uint(rms) & 0x7fffffffu) << 32) | ((unsigned long long)w << 8) | (unsigned long long)jj;
      if (key < mine) mine = key, mine_maxd = sqrtf(maxq);
    }
  }
  int n_assigned = 0;
  if constexpr (kAssign) {
    __syncthreads();  // (the bitmap is whole; s_taken is free)
    // the marked candidates in ascending order: wave 0 ranks the set bits, 64 words a pass
    if (wave == 0) {
      const int nwords = (total + 31) / 32;
      int found = 0;
      for (int base = 0; base < nwords; base += 64) {
        const int wi = base + lane;
        unsigned word = wi < nwords ? s_bits[wi] : 0u;
        const int cnt = __popc(word);
        int incl = cnt;
        for (int d = 1; d < 64; d <<= 1) {
          const int up = __shfl_up(incl, d, 64);
          if (lane >= d) incl += up;
        }
        int at = found + incl - cnt;
        while (word != 0u && at < kMaxAssign) {  // (at most 32 turns: one bit leaves the word in each)
          s_list[at++] = wi * 32 + (__ffs(word) - 1);
          word &= word - 1u;
        }
        found += __shfl(incl, 63, 64);
      }
      if (lane == 0) *s_nmark = found;
    }
    __syncthreads();
    const int n_marked = *s_nmark;
    if (n_marked > kMaxAssign) flags |= CHM_MATCH_MANY_ASSIGNMENTS;
    n_assigned = n_marked < kMaxAssign ? n_marked : kMaxAssign;
    // ---- phase B: wave w solves the marked candidates of rank w, w + 4, ...
    for (int q = wave; q < n_assigned; q += kBlock / 64) {
      const int cand = s_list[q];
      const int w = cand / n_piv, jj = cand - w * n_piv;
      float Minv[9], gm[6], t[3], xj[3], rms, maxq;
      mapping_frame(s_map[w], sL, gr, Minv, gm);
      mapped(Minv, s_s[s_piv[jj]].x, xj);
#pragma unroll
      for (int k = 0; k < 3; ++k) t[k] = xj[k] - s_r[pref].x[k];
      if (!assign_solve(s_s, s_r, n, Minv, t, gm, asg, lane, ell, &rms, &maxq)) continue;
      if (lane == 0 && rms <= p.stol) {
        const unsigned long long key =
            ((unsigned long long)(__float_as_uint(rms) & 0x7fffffffu) << 32) | ((unsigned long long)w << 8) | (unsigned long long)jj;
        if (key < mine) mine = key, mine_maxd = sqrtf(maxq);
      }
    }
  }
  if (mine != ~0ull) atomicMin(&s_best, mine);
  __syncthreads();
  const unsigned long long best_key = s_best;
  const bool matched = best_key != ~0ull;
  if (matched && mine == best_key) s_f[F_MAXD] = mine_maxd;  // (one thread: the key names its candidate)
  const int win_w = (int)((best_key >> 8) & 0xffu), win_jj = (int)(best_key & 0xffu);

  // ---- the winner's pairing, recomputed: reference atom k -> its sample atom
  if (!kPairs && p.perm) {
    int partner = -1;
    bool solved = false;  // (uniform) kAssign: the winner was a collided candidate and wave 0 solves it again
    if constexpr (kAssign) {
      const int cand = win_w * n_piv + win_jj;
      solved = matched && ((s_bits[cand >> 5] >> (cand & 31)) & 1u);
      if (solved) {
        __syncthreads();  // (every wave has left phase B: wave 0's slice is free)
        if (wave == 0) {
          float Minv[9], gm[6], t[3], xj[3], rms, maxq;
          mapping_frame(s_map[win_w], sL, gr, Minv, gm);
          mapped(Minv, s_s[s_piv[win_jj]].x, xj);
#pragma unroll
          for (int k = 0; k < 3; ++k) t[k] = xj[k] - s_r[pref].x[k];
          (void)assign_solve(s_s, s_r, n, Minv, t, gm, asg, lane, ell, &rms, &maxq);
        }
        __syncthreads();
        if (tid < n) partner = reinterpret_cast<const int*>(s_taken)[tid];  // (wave 0's col)
      }
    }
    if (!solved && matched && tid < n) {
      float Minv[9], gm[6], t[3], xj[3], best, D[3];
      mapping_frame(s_map[win_w], sL, gr, Minv, gm);
      mapped(Minv, s_s[s_piv[win_jj]].x, xj);
#pragma unroll
      for (int k = 0; k < 3; ++k) t[k] = xj[k] - s_r[pref].x[k];
      partner = nearest(s_s, n, s_r[tid], Minv, t, gm, &best, D);
    }
    if (tid < n) p.perm[(long)n0 + tid] = partner;
  }
  __syncthreads();
  if (tid != 0) return;
  const float rms = matched ? __uint_as_float((unsigned)(best_key >> 32)) : 0.f;
  if constexpr (kPairs) {
    if constexpr (kAssign) flags |= n_assigned << CHM_MATCH_PAIR_ASSIGNED_SHIFT;
    oi[0] = make_int4(__float_as_int(rms), __float_as_int(matched ? s_f[F_MAXD] : 0.f), flags, matched ? 1 : 0);
    if (matched) atomicOr(bit_word, bit);
    return;
  }
  const bool frames = !(flags & CHM_MATCH_NO_LATTICE);
  oi[0] = make_int4(__float_as_int(rms), __float_as_int(matched ? s_f[F_MAXD] : 0.f), __float_as_int(frames ? scale : 0.f),
                    __float_as_int(frames ? ell : 0.f));
  oi[1] = make_int4(matched ? s_map[win_w] : -1, matched ? s_piv[win_jj] : -1, n_maps, total);
  oi[2] = make_int4(s_i[I_NSURV], matched ? 1 : 0, flags, r);
  oi[3] = make_int4(n_assigned, 0, 0, 0);
}

// Block g = crystal g against reference ref_of[g] (-1 <= ref_of[g] < R: chm_match_create).
template <bool kAssign>
__device__ __forceinline__ void match_body(const MatchArgs& p) {
  const int g = blockIdx.x;
  match_block<false, kAssign>(p, g, p.ref_of[g], p.out + 4 * (long)g, nullptr, 0u);
}
__global__ __launch_bounds__(kBlock) void k_match(MatchArgs p) { match_body<false>(p); }
__global__ __launch_bounds__(kBlock) void k_match_assign(MatchArgs p) { match_body<true>(p); }

struct PairArgs {
  MatchArgs m;                   // the reference side aliases the sample side; ref_of, out and perm are unused
  const int2* pairs;             // [P] (h, g), h < g, n_h == n_g
  const unsigned char* exclude;  // NULL: none excluded
  unsigned* bits;                // [B, W]: bit g of row h = (h < g and they match), cleared by k_match_group_cells
  int W;
  int4* pout;                    // [P] {rms, max_dist, flags, matched}
};

// Block b = pair (h, g) = pairs[b]: crystal g as the sample against crystal h as the reference, both of one state.
template <bool kAssign>
__device__ __forceinline__ void match_pairs_body(const PairArgs& q) {
  const int2 pr = q.pairs[blockIdx.x];
  const int h = pr.x, g = pr.y;  // (0 <= h < g < B: chm_match_group_create)
  int4* oi = q.pout + blockIdx.x;
  // (uniform over the block: nothing is staged for a pair that cannot be searched)
  int early = 0;
  if (q.exclude && (q.exclude[h] || q.exclude[g])) early |= CHM_MATCH_EXCLUDED;
  if ((q.m.rec[h].flags | q.m.rec[g].flags) & kNoCell) early |= CHM_MATCH_NO_LATTICE;
  if (early) {
    if (threadIdx.x == 0) oi[0] = make_int4(0, 0, early, 0);
    return;
  }
  match_block<true, kAssign>(q.m, g, h, oi, q.bits + (long)h * q.W + (g >> 5), 1u << (g & 31));
}
__global__ __launch_bounds__(kBlock) void k_match_pairs(PairArgs q) { match_pairs_body<false>(q); }
__global__ __launch_bounds__(kBlock) void k_match_pairs_assign(PairArgs q) { match_pairs_body<true>(q); }

struct GroupArgs {
  int B;
  const chm_cell_record* rec;
  const unsigned char* exclude;
  int* nocell;       // [B] CHM_MATCH_NO_LATTICE or 0: k_dedup_lead's flags
  unsigned* bits;    // [B, W] the match matrix
  int W;
  const int* group;  // [B] of k_dedup_lead
  const int* first;  // [B] crystal g's first pair
  const int* rank;   // [B] crystals before g with g's atom count: pair (h, g) is first[g] + rank[h]
  const int4* pout;
  int4* out;         // [B] records of 32 bytes
};

// Thread g: has crystal g a reduced cell? The grid also clears the match matrix in front of k_match_pairs (a
// kernel, not a memset node: the sequence is replayed from captured graphs).
__global__ __launch_bounds__(kBlock) void k_match_group_cells(GroupArgs p) {
  const int g = blockIdx.x * kBlock + threadIdx.x;
  for (long w = g; w < (long)p.B * p.W; w += (long)gridDim.x * kBlock) p.bits[w] = 0u;
  if (g < p.B) p.nocell[g] = (p.rec[g].flags & kNoCell) ? CHM_MATCH_NO_LATTICE : 0;
}

// Thread g: the record of crystal g's pair with its leader.
__global__ __launch_bounds__(kBlock) void k_match_group_gather(GroupArgs p) {
  const int g = blockIdx.x * kBlock + threadIdx.x;
  if (g >= p.B) return;
  const int lead = p.group[g];
  int4 a = make_int4(0, 0, 0, 0), b = make_int4(-1, -1, 0, 0);
  if (lead < 0) {
    a.z = p.nocell[g] | ((p.exclude && p.exclude[g]) ? CHM_MATCH_EXCLUDED : 0);
  } else if (lead != g) {
    const int at = p.first[g] + p.rank[lead];
    a = p.pout[at];
    b.x = lead, b.y = at;
  }
  p.out[2 * (long)g] = a;
  p.out[2 * (long)g + 1] = b;
}

}  // namespace

struct chm_match {
  int B = 0, R = 0;
  long N = 0, NR = 0;
  int* d_ints = nullptr;  // one allocation: off [B + 1], roff [R + 1], ref_of [B]
  const int* d_off = nullptr;
  const int* d_roff = nullptr;
  const int* d_ref_of = nullptr;
};

namespace {
const chm::OffsetRule kLists{"match plan", kMaxAtoms, "the matcher"};
const chm::Check check{"the match plan"};
}  // namespace

extern "C" int chm_match_create(const int32_t* h_natoms, int num_graphs, const int32_t* h_ref_natoms, int num_refs,
                                const int32_t* h_ref_of, chm_match** out) {
  static_assert(sizeof(chm_match_record) == 64, "the record is 64 bytes");
  if (!out) return fail(CHM_E_ARG, "out is NULL");
  *out = nullptr;
  if (!h_natoms) return fail(CHM_E_ARG, "natoms is NULL");
  if (!h_ref_natoms) return fail(CHM_E_ARG, "ref_natoms is NULL");
  if (!h_ref_of) return fail(CHM_E_ARG, "ref_of is NULL");
  if (num_graphs <= 0) return fail(CHM_E_ARG, "num_graphs must be >= 1");
  if (num_refs <= 0) return fail(CHM_E_ARG, "num_refs must be >= 1");
  std::vector<int> offs, roffs;
  long N = 0, NR = 0;
  int rc;
  if ((rc = chm::node_offsets(h_natoms, num_graphs, "natoms", kLists, offs, &N))) return rc;
  if ((rc = chm::node_offsets(h_ref_natoms, num_refs, "ref_natoms", kLists, roffs, &NR))) return rc;
  for (int g = 0; g < num_graphs; ++g)
    if (h_ref_of[g] < -1 || h_ref_of[g] >= num_refs)
      return fail(CHM_E_ARG, "ref_of[" + std::to_string(g) + "] = " + std::to_string(h_ref_of[g]) + " outside [-1, " +
                                 std::to_string(num_refs) + ")");
  std::vector<int> all(offs);
  all.insert(all.end(), roffs.begin(), roffs.end());
  all.insert(all.end(), h_ref_of, h_ref_of + num_graphs);
  void* d_ints = nullptr;
  if ((rc = chm::upload(all.data(), all.size() * sizeof(int), "chm_match_create", &d_ints))) return rc;
  chm_match* p = new chm_match;
  p->B = num_graphs, p->R = num_refs, p->N = N, p->NR = NR;
  p->d_ints = static_cast<int*>(d_ints);
  p->d_off = p->d_ints;
  p->d_roff = p->d_off + offs.size();
  p->d_ref_of = p->d_roff + roffs.size();
  *out = p;
  return CHM_OK;
}

extern "C" void chm_match_destroy(chm_match* p) {
  if (!p) return;
  (void)hipFree(p->d_ints);
  delete p;
}

namespace {
int check_pairing(int pairing) {
  if (pairing == CHM_MATCH_PAIRING_NEAREST || pairing == CHM_MATCH_PAIRING_ASSIGNMENT) return CHM_OK;
  return fail(CHM_E_ARG, "pairing = " + std::to_string(pairing) + ": neither CHM_MATCH_PAIRING_NEAREST (0) nor "
                         "CHM_MATCH_PAIRING_ASSIGNMENT (1)");
}
}  // namespace

extern "C" int chm_match_run_pairing(const chm_match* p, const void* d_cell_records, size_t n_record_bytes,
                                     const int64_t* d_atom_types, int64_t n_atom_types, const float* d_frac,
                                     int64_t n_frac, const float* d_lattices, int64_t n_lattices,
                                     const void* d_ref_cell_records, size_t n_ref_record_bytes,
                                     const int64_t* d_ref_atom_types, int64_t n_ref_atom_types, const float* d_ref_frac,
                                     int64_t n_ref_frac, const float* d_ref_lattices, int64_t n_ref_lattices, float ltol,
                                     float stol, float angle_tol, void* d_out, size_t n_out_bytes, int32_t* d_perm,
                                     int64_t n_perm, void* stream, int pairing) {
  if (int rc = check_pairing(pairing)) return rc;
  if (!p) return fail(CHM_E_ARG, "match plan is NULL");
  int rc;
  if ((rc = check.count(d_cell_records, (long)n_record_bytes, 128L * p->B, "cell records", "bytes"))) return rc;
  if ((rc = check.aligned16(d_cell_records, "cell records"))) return rc;
  if ((rc = check.count(d_atom_types, n_atom_types, p->N, "atom_types [N]"))) return rc;
  if ((rc = check.count(d_frac, n_frac, 3 * p->N, "frac [N,3]"))) return rc;
  if ((rc = check.count(d_lattices, n_lattices, 9L * p->B, "lattices [B,3,3]"))) return rc;
  if ((rc = check.count(d_ref_cell_records, (long)n_ref_record_bytes, 128L * p->R, "ref cell records", "bytes"))) return rc;
  if ((rc = check.aligned16(d_ref_cell_records, "ref cell records"))) return rc;
  if ((rc = check.count(d_ref_atom_types, n_ref_atom_types, p->NR, "ref_atom_types [NR]"))) return rc;
  if ((rc = check.count(d_ref_frac, n_ref_frac, 3 * p->NR, "ref_frac [NR,3]"))) return rc;
  if ((rc = check.count(d_ref_lattices, n_ref_lattices, 9L * p->R, "ref_lattices [R,3,3]"))) return rc;
  if ((rc = check.range(ltol, CHM_MATCH_MAX_LTOL, "ltol", ""))) return rc;
  if ((rc = check.range(stol, CHM_MATCH_MAX_STOL, "stol", ""))) return rc;
  if ((rc = check.range(angle_tol, CHM_MATCH_MAX_ANGLE_TOL, "angle_tol", " degrees"))) return rc;
  if ((rc = check.count(d_out, (long)n_out_bytes, 64L * p->B, "out", "bytes"))) return rc;
  if ((rc = check.aligned16(d_out, "out"))) return rc;
  if ((rc = check.optional(d_perm, n_perm, p->N, "perm [N]"))) return rc;
  MatchArgs a;
  a.rec = static_cast<const chm_cell_record*>(d_cell_records);
  a.types = reinterpret_cast<const long long*>(d_atom_types);
  a.x = d_frac;
  a.lat = d_lattices;
  a.off = p->d_off;
  a.rrec = static_cast<const chm_cell_record*>(d_ref_cell_records);
  a.rtypes = reinterpret_cast<const long long*>(d_ref_atom_types);
  a.rx = d_ref_frac;
  a.rlat = d_ref_lattices;
  a.roff = p->d_roff;
  a.ref_of = p->d_ref_of;
  a.ltol = ltol;
  a.stol = stol;
  a.angle_tol = angle_tol;
  a.out = static_cast<int4*>(d_out);
  a.perm = d_perm;
  if (pairing == CHM_MATCH_PAIRING_ASSIGNMENT)
    hipLaunchKernelGGL(k_match_assign, dim3(p->B), dim3(kBlock), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(k_match, dim3(p->B), dim3(kBlock), 0, (hipStream_t)stream, a);
  HIPCHK(hipGetLastError());
  return CHM_OK;
}

extern "C" int chm_match_run(const chm_match* p, const void* d_cell_records, size_t n_record_bytes,
                             const int64_t* d_atom_types, int64_t n_atom_types, const float* d_frac, int64_t n_frac,
                             const float* d_lattices, int64_t n_lattices, const void* d_ref_cell_records,
                             size_t n_ref_record_bytes, const int64_t* d_ref_atom_types, int64_t n_ref_atom_types,
                             const float* d_ref_frac, int64_t n_ref_frac, const float* d_ref_lattices,
                             int64_t n_ref_lattices, float ltol, float stol, float angle_tol, void* d_out,
                             size_t n_out_bytes, int32_t* d_perm, int64_t n_perm, void* stream) {
  return chm_match_run_pairing(p, d_cell_records, n_record_bytes, d_atom_types, n_atom_types, d_frac, n_frac, d_lattices,
                               n_lattices, d_ref_cell_records, n_ref_record_bytes, d_ref_atom_types, n_ref_atom_types,
                               d_ref_frac, n_ref_frac, d_ref_lattices, n_ref_lattices, ltol, stol, angle_tol, d_out,
                               n_out_bytes, d_perm, n_perm, stream, CHM_MATCH_PAIRING_NEAREST);
}

// ---- grouping a batch by pairwise matching (chm_match_group_*): k_match_pairs over the plan's pair table into the
// bit matrix, k_dedup_lead (dedup.hip) over the matrix, k_match_group_gather for the members' records
struct chm_match_group {
  int B = 0;
  long N = 0, P = 0;
  char* d_mem = nullptr;  // one allocation: off [B + 1], first [B], rank [B], (padding), pairs [P] int2
  const int* d_off = nullptr;
  const int* d_first = nullptr;
  const int* d_rank = nullptr;
  const int2* d_pairs = nullptr;
};

namespace {
size_t align16(size_t v) { return (v + 15) / 16 * 16; }
size_t group_bits_bytes(int B) { return align16((size_t)B * (size_t)((B + 31) / 32) * sizeof(unsigned)); }
}  // namespace

extern "C" int chm_match_group_create(const int32_t* h_natoms, int num_graphs, chm_match_group** out) {
  static_assert(sizeof(chm_match_group_record) == 32 && sizeof(chm_match_pair_record) == 16, "the records' sizes");
  if (!out) return fail(CHM_E_ARG, "out is NULL");
  *out = nullptr;
  if (!h_natoms) return fail(CHM_E_ARG, "natoms is NULL");
  if (num_graphs <= 0) return fail(CHM_E_ARG, "num_graphs must be >= 1");
  std::vector<int> offs;
  long N = 0;
  int rc;
  if ((rc = chm::node_offsets(h_natoms, num_graphs, "natoms", kLists, offs, &N))) return rc;
  const int B = num_graphs;
  // rank[g] = crystals before g with g's atom count; P = sum of the ranks, counted before anything is built
  std::vector<int> seen(kMaxAtoms + 1, 0), rank((size_t)B), first((size_t)B);
  long P = 0;
  for (int g = 0; g < B; ++g) {
    rank[g] = seen[h_natoms[g]]++;
    if (P > INT32_MAX - (long)rank[g])
      return fail(CHM_E_UNSUPPORTED, "more than 2^31 - 1 pairs of equal atom count: they do not fit one grid");
    first[g] = (int)P;
    P += rank[g];
  }
  std::vector<int2> pairs((size_t)P);
  std::vector<std::vector<int>> by_size(kMaxAtoms + 1);
  for (int g = 0; g < B; ++g) {
    std::vector<int>& earlier = by_size[h_natoms[g]];
    for (size_t k = 0; k < earlier.size(); ++k) pairs[(size_t)first[g] + k] = make_int2(earlier[k], g);
    earlier.push_back(g);
  }
  const size_t n_ints = (size_t)3 * B + 1, ints_bytes = align16(n_ints * sizeof(int));
  std::vector<char> host(ints_bytes + (size_t)P * sizeof(int2), 0);
  int* hi = reinterpret_cast<int*>(host.data());
  for (int g = 0; g <= B; ++g) hi[g] = offs[g];
  for (int g = 0; g < B; ++g) hi[B + 1 + g] = first[g], hi[2 * B + 1 + g] = rank[g];
  if (P) memcpy(host.data() + ints_bytes, pairs.data(), (size_t)P * sizeof(int2));
  void* d_mem = nullptr;
  if ((rc = chm::upload(host.data(), host.size(), "chm_match_group_create", &d_mem))) return rc;
  chm_match_group* p = new chm_match_group;
  p->B = B, p->N = N, p->P = P;
  p->d_mem = static_cast<char*>(d_mem);
  p->d_off = reinterpret_cast<const int*>(p->d_mem);
  p->d_first = p->d_off + B + 1;
  p->d_rank = p->d_first + B;
  p->d_pairs = reinterpret_cast<const int2*>(p->d_mem + ints_bytes);
  *out = p;
  return CHM_OK;
}

extern "C" void chm_match_group_destroy(chm_match_group* p) {
  if (!p) return;
  (void)hipFree(p->d_mem);
  delete p;
}

extern "C" int64_t chm_match_group_num_pairs(const chm_match_group* p) { return p ? p->P : 0; }

// the bit matrix [B, ceil(B/32)] words, the representatives' list [B], the cell flags [B]
extern "C" size_t chm_match_group_workspace_bytes(const chm_match_group* p) {
  if (!p) return 0;
  return group_bits_bytes(p->B) + 2 * (size_t)p->B * sizeof(int);
}

extern "C" int chm_match_group_run_pairing(const chm_match_group* p, const void* d_cell_records, size_t n_record_bytes,
                                           const int64_t* d_atom_types, int64_t n_atom_types, const float* d_frac,
                                           int64_t n_frac, const float* d_lattices, int64_t n_lattices,
                                           const uint8_t* d_exclude, int64_t n_exclude, float ltol, float stol,
                                           float angle_tol, int32_t* d_group, int64_t n_group, int32_t* d_count,
                                           int64_t n_count, void* d_out, size_t n_out_bytes, void* d_pair_records,
                                           size_t n_pair_bytes, void* d_workspace, size_t workspace_bytes, void* stream,
                                           int pairing) {
  if (int rc = check_pairing(pairing)) return rc;
  if (!p) return fail(CHM_E_ARG, "match-group plan is NULL");
  int rc;
  if ((rc = check.count(d_cell_records, (long)n_record_bytes, 128L * p->B, "cell records", "bytes"))) return rc;
  if ((rc = check.aligned16(d_cell_records, "cell records"))) return rc;
  if ((rc = check.count(d_atom_types, n_atom_types, p->N, "atom_types [N]"))) return rc;
  if ((rc = check.count(d_frac, n_frac, 3 * p->N, "frac [N,3]"))) return rc;
  if ((rc = check.count(d_lattices, n_lattices, 9L * p->B, "lattices [B,3,3]"))) return rc;
  if ((rc = check.optional(d_exclude, n_exclude, p->B, "exclude [B]"))) return rc;
  if ((rc = check.range(ltol, CHM_MATCH_MAX_LTOL, "ltol", ""))) return rc;
  if ((rc = check.range(stol, CHM_MATCH_MAX_STOL, "stol", ""))) return rc;
  if ((rc = check.range(angle_tol, CHM_MATCH_MAX_ANGLE_TOL, "angle_tol", " degrees"))) return rc;
  if ((rc = check.count(d_group, n_group, p->B, "group [B]"))) return rc;
  if ((rc = check.count(d_count, n_count, p->B, "count [B]"))) return rc;
  if ((rc = check.count(d_out, (long)n_out_bytes, 32L * p->B, "out", "bytes"))) return rc;
  if ((rc = check.aligned16(d_out, "out"))) return rc;
  if (p->P == 0) {
    if (n_pair_bytes != 0) return fail(CHM_E_ARG, "pair records: " + std::to_string(n_pair_bytes) + " bytes, the plan has no pair");
  } else if ((rc = check.count(d_pair_records, (long)n_pair_bytes, 16L * p->P, "pair records", "bytes"))) {
    return rc;
  }
  if ((rc = check.aligned16(d_pair_records, "pair records"))) return rc;
  const chm::Check grouping{"the match grouping"};
  if ((rc = grouping.workspace(d_workspace, workspace_bytes, chm_match_group_workspace_bytes(p)))) return rc;
  if ((rc = grouping.aligned16(d_workspace, "workspace"))) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int B = p->B, W = (B + 31) / 32;
  unsigned* bits = static_cast<unsigned*>(d_workspace);
  int* reps = reinterpret_cast<int*>(static_cast<char*>(d_workspace) + group_bits_bytes(B));
  int* nocell = reps + B;
  GroupArgs ga;
  ga.B = B;
  ga.rec = static_cast<const chm_cell_record*>(d_cell_records);
  ga.exclude = d_exclude;
  ga.nocell = nocell;
  ga.bits = bits;
  ga.W = W;
  ga.group = d_group;
  ga.first = p->d_first;
  ga.rank = p->d_rank;
  ga.pout = static_cast<const int4*>(d_pair_records);
  ga.out = static_cast<int4*>(d_out);
  const dim3 per_crystal((unsigned)((B + kBlock - 1) / kBlock));
  hipLaunchKernelGGL(k_match_group_cells, per_crystal, dim3(kBlock), 0, s, ga);
  HIPCHK(hipGetLastError());
  if (p->P) {
    PairArgs a;
    a.m.rec = a.m.rrec = ga.rec;
    a.m.types = a.m.rtypes = reinterpret_cast<const long long*>(d_atom_types);
    a.m.x = a.m.rx = d_frac;
    a.m.lat = a.m.rlat = d_lattices;
    a.m.off = a.m.roff = p->d_off;
    a.m.ref_of = nullptr;
    a.m.ltol = ltol;
    a.m.stol = stol;
    a.m.angle_tol = angle_tol;
    a.m.out = nullptr;
    a.m.perm = nullptr;
    a.pairs = p->d_pairs;
    a.exclude = d_exclude;
    a.bits = bits;
    a.W = W;
    a.pout = static_cast<int4*>(d_pair_records);
    if (pairing == CHM_MATCH_PAIRING_ASSIGNMENT)
      hipLaunchKernelGGL(k_match_pairs_assign, dim3((unsigned)p->P), dim3(kBlock), 0, s, a);
    else
      hipLaunchKernelGGL(k_match_pairs, dim3((unsigned)p->P), dim3(kBlock), 0, s, a);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(chm::dedup_lead(B, W, bits, nocell, d_exclude, reps, d_group, d_count, s));
  hipLaunchKernelGGL(k_match_group_gather, per_crystal, dim3(kBlock), 0, s, ga);
  HIPCHK(hipGetLastError());
  return CHM_OK;
}

extern "C" int chm_match_group_run(const chm_match_group* p, const void* d_cell_records, size_t n_record_bytes,
                                   const int64_t* d_atom_types, int64_t n_atom_types, const float* d_frac,
                                   int64_t n_frac, const float* d_lattices, int64_t n_lattices,
                                   const uint8_t* d_exclude, int64_t n_exclude, float ltol, float stol, float angle_tol,
                                   int32_t* d_group, int64_t n_group, int32_t* d_count, int64_t n_count, void* d_out,
                                   size_t n_out_bytes, void* d_pair_records, size_t n_pair_bytes, void* d_workspace,
                                   size_t workspace_bytes, void* stream) {
  return chm_match_group_run_pairing(p, d_cell_records, n_record_bytes, d_atom_types, n_atom_types, d_frac, n_frac,
                                     d_lattices, n_lattices, d_exclude, n_exclude, ltol, stol, angle_tol, d_group, n_group,
                                     d_count, n_count, d_out, n_out_bytes, d_pair_records, n_pair_bytes, d_workspace,
                                     workspace_bytes, stream, CHM_MATCH_PAIRING_NEAREST);
}

// ---- searching a reference set for each sample (chm_match_set_*): k_set_keys finds each sample's candidates in the
// sorted set, k_set_offsets scans their counts, k_set_pairs runs match_block over the compact pair list on a grid
// of fixed size and k_set_gather writes each sample's record against its winner
namespace {

constexpr unsigned long long kMixA = CHM_MATCH_SET_MIX_A, kMixB = CHM_MATCH_SET_MIX_B;

__device__ inline unsigned long long mix_type(long long type) {
  unsigned long long z = (unsigned long long)(unsigned)type + 1ull;  // (the low 32 bits, as match_block compares them)
  z = (z ^ (z >> 30)) * kMixA;
  z = (z ^ (z >> 27)) * kMixB;
  return z ^ (z >> 31);
}

struct SetArgs {
  int B;
  const chm_cell_record* rec;           // [B] of the samples
  const long long* types;               // [N]
  const int* off;                       // [B + 1]
  const unsigned char* exclude;         // NULL: none excluded
  const int* size_first;                // [kMaxAtoms + 2]: the sorted positions of size n are [size_first[n], size_first[n + 1])
  const unsigned long long* rkeys;      // [R] sorted within a size
  const int* rindex;                    // [R] original index of sorted position
  const int* rpos;                      // [R] sorted position of original index
  unsigned long long* keys;             // [B]
  unsigned long long* win;              // [B] (rms bits << 32) | original index of the best matched candidate
  int* lo;                              // [B]
  int* cnt;                             // [B]
  int* n_matched;                       // [B]
  int* first;                           // [B + 1]
  const int4* pout;                     // [capacity]
  int4* out;                            // [B] records of 48 bytes
};

// Block g = sample g: its key, its candidates [lo, lo + cnt) in the sorted set, and its winner word and match count
// cleared in front of k_set_pairs (a kernel, not a memset node: the sequence is replayed from captured graphs).
__global__ __launch_bounds__(kBlock) void k_set_keys(SetArgs p) {
  __shared__ unsigned long long s_part[kBlock / 64];
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = p.off[g], n = p.off[g + 1] - n0;  // (1 <= n <= kMaxAtoms: chm_match_set_create)
  unsigned long long v = tid < n ? mix_type(p.types[(long)n0 + tid]) : 0ull;
  // (wrapping integer adds in a fixed tree: lanes, then waves in index order)
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
  if (lane == 0) s_part[wave] = v;
  __syncthreads();
  if (tid != 0) return;
  unsigned long long key = s_part[0];
  for (int w = 1; w < kBlock / 64; ++w) key += s_part[w];
  int lo = 0, cnt = 0;
  const bool out = (p.exclude && p.exclude[g]) || (p.rec[g].flags & kNoCell);
  if (!out) {
    const int a = p.size_first[n], b = p.size_first[n + 1];
    int l = a, r = b;  // the first position in [a, b) whose key is >= key
    while (l < r) {
      const int m = l + (r - l) / 2;
      if (p.rkeys[m] < key) l = m + 1; else r = m;
    }
    lo = l, r = b;     // the first position in [lo, b) whose key is > key
    while (l < r) {
      const int m = l + (r - l) / 2;
      if (p.rkeys[m] <= key) l = m + 1; else r = m;
    }
    cnt = l - lo;
  }
  p.keys[g] = key;
  p.lo[g] = lo;
  p.cnt[g] = cnt;
  p.win[g] = ~0ull;
  p.n_matched[g] = 0;
}

// One block: first[B + 1] = the exclusive scan of cnt[B] (a chunked integer scan, as k_prim_offsets).
__global__ __launch_bounds__(kBlock) void k_set_offsets(SetArgs p) {
  __shared__ int s[kBlock];
  __shared__ int s_carry;
  const int tid = threadIdx.x;
  if (tid == 0) {
    s_carry = 0;
    p.first[0] = 0;
  }
  __syncthreads();
  for (int base = 0; base < p.B; base += kBlock) {  // (B is the same in every thread: the barriers are uniform)
    const int g = base + tid;
    s[tid] = g < p.B ? p.cnt[g] : 0;
    __syncthreads();
    for (int d = 1; d < kBlock; d <<= 1) {
      const int add = tid >= d ? s[tid - d] : 0;
      __syncthreads();
      s[tid] += add;
      __syncthreads();
    }
    const int carry = s_carry;
    if (g < p.B) p.first[g + 1] = carry + s[tid];
    __syncthreads();
    if (tid == kBlock - 1) s_carry = carry + s[tid];
    __syncthreads();
  }
}

struct SetPairArgs {
  MatchArgs m;  // the reference side is the sorted set; ref_of, out and perm are unused
  int B;
  const int* first;          // [B + 1]; first[B] = P, the pairs of this run
  const int* lo;             // [B]
  const int* rindex;         // [R]
  int4* pout;                // [capacity] {rms, max_dist, flags, matched}; [0, P) are written
  int* n_matched;            // [B]
  unsigned long long* win;   // [B]
  unsigned* sink;            // one word that match_block or-s 0 into
};

// The blocks stride over the pairs b < P of this run: pair b is sample g = the last one with first[g] <= b against
// the set's sorted position lo[g] + b - first[g]. The record at b depends on the two structures alone; a match adds
// one to the sample's count and takes the integer minimum of (rms bits, original index) into its winner word.
template <bool kAssign>
__device__ __forceinline__ void set_pairs_body(const SetPairArgs& q) {
  const int P = q.first[q.B];
  for (int b = blockIdx.x; b < P; b += gridDim.x) {  // (b and everything derived from it are uniform over the block)
    int g = 0, hi = q.B - 1;  // first[g] <= b < first[hi + 1]
    while (g < hi) {
      const int mid = g + (hi - g + 1) / 2;
      if (q.first[mid] <= b) g = mid; else hi = mid - 1;
    }
    const int pos = q.lo[g] + (b - q.first[g]);
    int4* oi = q.pout + b;
    match_block<true, kAssign>(q.m, g, pos, oi, q.sink, 0u);
    if (threadIdx.x == 0) {
      const int4 r = oi[0];
      if (r.w) {
        atomicAdd(q.n_matched + g, 1);
        atomicMin(q.win + g, ((unsigned long long)(unsigned)r.x << 32) | (unsigned long long)(unsigned)q.rindex[pos]);
      }
    }
    __syncthreads();  // (thread 0 has read the block's LDS before the next pair is staged)
  }
}
__global__ __launch_bounds__(kBlock) void k_set_pairs(SetPairArgs q) { set_pairs_body<false>(q); }
__global__ __launch_bounds__(kBlock) void k_set_pairs_assign(SetPairArgs q) { set_pairs_body<true>(q); }

// Thread g: the record of sample g against its winner.
__global__ __launch_bounds__(kBlock) void k_set_gather(SetArgs p) {
  const int g = blockIdx.x * kBlock + threadIdx.x;
  if (g >= p.B) return;
  const unsigned long long w = p.win[g], key = p.keys[g];
  const int first = p.first[g], lo = p.lo[g], cnt = p.cnt[g];
  int4 a = make_int4(0, 0, 0, 0), b = make_int4(-1, -1, cnt, p.n_matched[g]);
  a.z = ((p.exclude && p.exclude[g]) ? CHM_MATCH_EXCLUDED : 0) | ((p.rec[g].flags & kNoCell) ? CHM_MATCH_NO_LATTICE : 0);
  if (w != ~0ull) {
    const int ref = (int)(unsigned)(w & 0xffffffffull), pos = p.rpos[ref];
    const int4 r = p.pout[first + (pos - lo)];
    a = make_int4(r.x, r.y, r.z, 1);
    b.x = ref, b.y = pos;
  }
  p.out[3 * (long)g] = a;
  p.out[3 * (long)g + 1] = b;
  p.out[3 * (long)g + 2] = make_int4((int)(unsigned)(key & 0xffffffffull), (int)(unsigned)(key >> 32), first, lo);
}

const chm::OffsetRule kSetLists{"match-set plan", kMaxAtoms, "the matcher"};
const chm::Check set_check{"the match-set plan"};

}  // namespace

struct chm_match_set {
  int B = 0, R = 0, grid = 0;
  long N = 0, NR = 0, capacity = 0;
  char* d_mem = nullptr;  // one allocation: rkeys [R] u64, then off [B + 1], roff [R + 1], rindex [R], rpos [R], size_first
  const unsigned long long* d_rkeys = nullptr;
  const int* d_off = nullptr;
  const int* d_roff = nullptr;
  const int* d_rindex = nullptr;
  const int* d_rpos = nullptr;
  const int* d_size_first = nullptr;
};

extern "C" int chm_match_set_create(const int32_t* h_natoms, int num_graphs, const int32_t* h_ref_natoms,
                                    const uint64_t* h_ref_keys, const int32_t* h_ref_index, int num_refs,
                                    chm_match_set** out) {
  static_assert(sizeof(chm_match_set_record) == 48, "the record is 48 bytes");
  if (!out) return fail(CHM_E_ARG, "out is NULL");
  *out = nullptr;
  if (!h_natoms) return fail(CHM_E_ARG, "natoms is NULL");
  if (!h_ref_natoms) return fail(CHM_E_ARG, "ref_natoms is NULL");
  if (!h_ref_keys) return fail(CHM_E_ARG, "ref_keys is NULL");
  if (!h_ref_index) return fail(CHM_E_ARG, "ref_index is NULL");
  if (num_graphs <= 0) return fail(CHM_E_ARG, "num_graphs must be >= 1");
  if (num_refs <= 0) return fail(CHM_E_ARG, "num_refs must be >= 1");
  const int B = num_graphs, R = num_refs;
  std::vector<int> offs, roffs;
  long N = 0, NR = 0;
  int rc;
  if ((rc = chm::node_offsets(h_natoms, B, "natoms", kSetLists, offs, &N))) return rc;
  if ((rc = chm::node_offsets(h_ref_natoms, R, "ref_natoms", kSetLists, roffs, &NR))) return rc;
  std::vector<int> rpos((size_t)R, -1), size_first(kMaxAtoms + 2, 0);
  for (int k = 0; k < R; ++k) {
    const int at = h_ref_index[k];
    if (at < 0 || at >= R || rpos[at] >= 0)
      return fail(CHM_E_ARG, "ref_index[" + std::to_string(k) + "] = " + std::to_string(at) + ": not a permutation of [0, " +
                                 std::to_string(R) + ")");
    rpos[at] = k;
    if (k) {
      const bool ordered = h_ref_natoms[k - 1] != h_ref_natoms[k] ? h_ref_natoms[k - 1] < h_ref_natoms[k]
                           : h_ref_keys[k - 1] != h_ref_keys[k]   ? h_ref_keys[k - 1] < h_ref_keys[k]
                                                                  : h_ref_index[k - 1] < at;
      if (!ordered)
        return fail(CHM_E_ARG, "the reference set is not sorted by (atom count, key, index) at position " + std::to_string(k));
    }
    size_first[h_ref_natoms[k] + 1] += 1;
  }
  for (int n = 1; n <= kMaxAtoms + 1; ++n) size_first[n] += size_first[n - 1];  // (size_first[n] = references smaller than n)
  long capacity = 0;
  for (int g = 0; g < B; ++g) {
    capacity += size_first[h_natoms[g] + 1] - size_first[h_natoms[g]];
    if (capacity > INT32_MAX)
      return fail(CHM_E_UNSUPPORTED, "more than 2^31 - 1 pairs of equal atom count: they do not fit the pair list");
  }
  int device = 0;
  hipDeviceProp_t prop;
  hipError_t e = hipGetDevice(&device);
  if (e == hipSuccess) e = hipGetDeviceProperties(&prop, device);
  if (e != hipSuccess) return fail(CHM_E_HIP, std::string("chm_match_set_create: ") + hipGetErrorString(e));
  const size_t keys_bytes = (size_t)R * sizeof(unsigned long long);
  const size_t n_ints = (size_t)B + 1 + (size_t)R + 1 + 2 * (size_t)R + size_first.size();
  std::vector<char> host(keys_bytes + n_ints * sizeof(int), 0);
  memcpy(host.data(), h_ref_keys, keys_bytes);
  int* hi = reinterpret_cast<int*>(host.data() + keys_bytes);
  memcpy(hi, offs.data(), offs.size() * sizeof(int));
  memcpy(hi + B + 1, roffs.data(), roffs.size() * sizeof(int));
  memcpy(hi + B + 1 + R + 1, h_ref_index, (size_t)R * sizeof(int));
  memcpy(hi + B + 1 + R + 1 + R, rpos.data(), (size_t)R * sizeof(int));
  memcpy(hi + B + 1 + R + 1 + 2 * (size_t)R, size_first.data(), size_first.size() * sizeof(int));
  void* d_mem = nullptr;
  if ((rc = chm::upload(host.data(), host.size(), "chm_match_set_create", &d_mem))) return rc;
  chm_match_set* p = new chm_match_set;
  p->B = B, p->R = R, p->N = N, p->NR = NR, p->capacity = capacity;
  const long full = (long)CHM_MATCH_SET_BLOCKS_PER_CU * (prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 1);
  p->grid = (int)(capacity < full ? capacity : full);
  p->d_mem = static_cast<char*>(d_mem);
  p->d_rkeys = reinterpret_cast<const unsigned long long*>(p->d_mem);
  p->d_off = reinterpret_cast<const int*>(p->d_mem + keys_bytes);
  p->d_roff = p->d_off + B + 1;
  p->d_rindex = p->d_roff + R + 1;
  p->d_rpos = p->d_rindex + R;
  p->d_size_first = p->d_rpos + R;
  *out = p;
  return CHM_OK;
}

extern "C" void chm_match_set_destroy(chm_match_set* p) {
  if (!p) return;
  (void)hipFree(p->d_mem);
  delete p;
}

extern "C" int64_t chm_match_set_num_pairs_max(const chm_match_set* p) { return p ? p->capacity : 0; }

// keys [B] and winner words [B] (64 bits each), then lo [B], cnt [B], n_matched [B], first [B + 1] and the sink word
extern "C" size_t chm_match_set_workspace_bytes(const chm_match_set* p) {
  if (!p) return 0;
  return align16(2 * (size_t)p->B * sizeof(unsigned long long) + (4 * (size_t)p->B + 2) * sizeof(int));
}

extern "C" int chm_match_set_run_pairing(const chm_match_set* p, const void* d_cell_records, size_t n_record_bytes,
                                         const int64_t* d_atom_types, int64_t n_atom_types, const float* d_frac,
                                         int64_t n_frac, const float* d_lattices, int64_t n_lattices,
                                         const void* d_ref_cell_records, size_t n_ref_record_bytes,
                                         const int64_t* d_ref_atom_types, int64_t n_ref_atom_types,
                                         const float* d_ref_frac, int64_t n_ref_frac, const float* d_ref_lattices,
                                         int64_t n_ref_lattices, const uint8_t* d_exclude, int64_t n_exclude, float ltol,
                                         float stol, float angle_tol, void* d_out, size_t n_out_bytes,
                                         void* d_pair_records, size_t n_pair_bytes, void* d_workspace,
                                         size_t workspace_bytes, void* stream, int pairing) {
  if (int rc = check_pairing(pairing)) return rc;
  if (!p) return fail(CHM_E_ARG, "match-set plan is NULL");
  const chm::Check& check = set_check;
  int rc;
  if ((rc = check.count(d_cell_records, (long)n_record_bytes, 128L * p->B, "cell records", "bytes"))) return rc;
  if ((rc = check.aligned16(d_cell_records, "cell records"))) return rc;
  if ((rc = check.count(d_atom_types, n_atom_types, p->N, "atom_types [N]"))) return rc;
  if ((rc = check.count(d_frac, n_frac, 3 * p->N, "frac [N,3]"))) return rc;
  if ((rc = check.count(d_lattices, n_lattices, 9L * p->B, "lattices [B,3,3]"))) return rc;
  if ((rc = check.count(d_ref_cell_records, (long)n_ref_record_bytes, 128L * p->R, "ref cell records", "bytes"))) return rc;
  if ((rc = check.aligned16(d_ref_cell_records, "ref cell records"))) return rc;
  if ((rc = check.count(d_ref_atom_types, n_ref_atom_types, p->NR, "ref_atom_types [NR]"))) return rc;
  if ((rc = check.count(d_ref_frac, n_ref_frac, 3 * p->NR, "ref_frac [NR,3]"))) return rc;
  if ((rc = check.count(d_ref_lattices, n_ref_lattices, 9L * p->R, "ref_lattices [R,3,3]"))) return rc;
  if ((rc = check.optional(d_exclude, n_exclude, p->B, "exclude [B]"))) return rc;
  if ((rc = check.range(ltol, CHM_MATCH_MAX_LTOL, "ltol", ""))) return rc;
  if ((rc = check.range(stol, CHM_MATCH_MAX_STOL, "stol", ""))) return rc;
  if ((rc = check.range(angle_tol, CHM_MATCH_MAX_ANGLE_TOL, "angle_tol", " degrees"))) return rc;
  if ((rc = check.count(d_out, (long)n_out_bytes, 48L * p->B, "out", "bytes"))) return rc;
  if ((rc = check.aligned16(d_out, "out"))) return rc;
  if (p->capacity == 0) {
    if (n_pair_bytes != 0) return fail(CHM_E_ARG, "pair records: " + std::to_string(n_pair_bytes) + " bytes, the plan has no pair");
  } else if ((rc = check.count(d_pair_records, (long)n_pair_bytes, 16L * p->capacity, "pair records", "bytes"))) {
    return rc;
  }
  if ((rc = check.aligned16(d_pair_records, "pair records"))) return rc;
  if ((rc = check.workspace(d_workspace, workspace_bytes, chm_match_set_workspace_bytes(p)))) return rc;
  if ((rc = check.aligned16(d_workspace, "workspace"))) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int B = p->B;
  SetArgs a;
  a.B = B;
  a.rec = static_cast<const chm_cell_record*>(d_cell_records);
  a.types = reinterpret_cast<const long long*>(d_atom_types);
  a.off = p->d_off;
  a.exclude = d_exclude;
  a.size_first = p->d_size_first;
  a.rkeys = p->d_rkeys;
  a.rindex = p->d_rindex;
  a.rpos = p->d_rpos;
  a.keys = static_cast<unsigned long long*>(d_workspace);
  a.win = a.keys + B;
  a.lo = reinterpret_cast<int*>(a.win + B);
  a.cnt = a.lo + B;
  a.n_matched = a.cnt + B;
  a.first = a.n_matched + B;
  a.pout = static_cast<const int4*>(d_pair_records);
  a.out = static_cast<int4*>(d_out);
  hipLaunchKernelGGL(k_set_keys, dim3((unsigned)B), dim3(kBlock), 0, s, a);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_set_offsets, dim3(1), dim3(kBlock), 0, s, a);
  HIPCHK(hipGetLastError());
  if (p->capacity) {
    SetPairArgs q;
    q.m.rec = a.rec;
    q.m.types = a.types;
    q.m.x = d_frac;
    q.m.lat = d_lattices;
    q.m.off = p->d_off;
    q.m.rrec = static_cast<const chm_cell_record*>(d_ref_cell_records);
    q.m.rtypes = reinterpret_cast<const long long*>(d_ref_atom_types);
    q.m.rx = d_ref_frac;
    q.m.rlat = d_ref_lattices;
    q.m.roff = p->d_roff;
    q.m.ref_of = nullptr;
    q.m.ltol = ltol;
    q.m.stol = stol;
    q.m.angle_tol = angle_tol;
    q.m.out = nullptr;
    q.m.perm = nullptr;
    q.B = B;
    q.first = a.first;
    q.lo = a.lo;
    q.rindex = p->d_rindex;
    q.pout = static_cast<int4*>(d_pair_records);
    q.n_matched = a.n_matched;
    q.win = a.win;
    q.sink = reinterpret_cast<unsigned*>(a.first + B + 1);
    if (pairing == CHM_MATCH_PAIRING_ASSIGNMENT)
      hipLaunchKernelGGL(k_set_pairs_assign, dim3((unsigned)p->grid), dim3(kBlock), 0, s, q);
    else
      hipLaunchKernelGGL(k_set_pairs, dim3((unsigned)p->grid), dim3(kBlock), 0, s, q);
    HIPCHK(hipGetLastError());
  }
  hipLaunchKernelGGL(k_set_gather, dim3((unsigned)((B + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, a);
  HIPCHK(hipGetLastError());
  return CHM_OK;
}

extern "C" int chm_match_set_run(const chm_match_set* p, const void* d_cell_records, size_t n_record_bytes,
                                 const int64_t* d_atom_types, int64_t n_atom_types, const float* d_frac, int64_t n_frac,
                                 const float* d_lattices, int64_t n_lattices, const void* d_ref_cell_records,
                                 size_t n_ref_record_bytes, const int64_t* d_ref_atom_types, int64_t n_ref_atom_types,
                                 const float* d_ref_frac, int64_t n_ref_frac, const float* d_ref_lattices,
                                 int64_t n_ref_lattices, const uint8_t* d_exclude, int64_t n_exclude, float ltol,
                                 float stol, float angle_tol, void* d_out, size_t n_out_bytes, void* d_pair_records,
                                 size_t n_pair_bytes, void* d_workspace, size_t workspace_bytes, void* stream) {
  return chm_match_set_run_pairing(p, d_cell_records, n_record_bytes, d_atom_types, n_atom_types, d_frac, n_frac,
                                   d_lattices, n_lattices, d_ref_cell_records, n_ref_record_bytes, d_ref_atom_types,
                                   n_ref_atom_types, d_ref_frac, n_ref_frac, d_ref_lattices, n_ref_lattices, d_exclude,
                                   n_exclude, ltol, stol, angle_tol, d_out, n_out_bytes, d_pair_records, n_pair_bytes,
                                   d_workspace, workspace_bytes, stream, CHM_MATCH_PAIRING_NEAREST);
}
