// Crystal system with the atoms on the device (chm_symm_*, include/chemeleon_hip.h): per crystal the lattice
// operations W that k_cell accepted at the cell record's final level are found again (the same candidate test,
// cell_shared.h), and for each of them the translations t that carry the atoms onto themselves, x -> x W + t in
// the Niggli-reduced basis (the same Lr and x' as chm_cell_apply, cell_shared.h). The accepted pairs' point
// group names the crystal system (test_crystal_system_matching of the reference's scripts/evaluate.py). One
// 64-byte record per crystal and, if asked, one (W, t) per point-group operation. The plan (chm_symm) is
// independent of chm_model / chm_batch, like chm_cell: node offsets, uploaded once.
//
// One 256-thread block per crystal. The reduced coordinates and types (16 bytes per atom, at most 256 atoms) and
// the accepted W (at most 48 candidate indices) are staged in LDS. The candidates (W, t_j), j over the atoms of
// the rarest species, are spread over the block, one thread each; a thread gives a candidate up at the first
// atom without a partner. Every count is an integer add or min in LDS, so the record does not depend on any order.
#include <hip/hip_runtime.h>

#include <limits.h>
#include <math.h>

#include <cstdint>
#include <string>
#include <vector>

#include "chm_host.h"
#include "plan_common.h"
#include "cell_shared.h"
#include "symm_shared.h"

// Every product and sum is rounded on its own (as in cell.hip).
#pragma clang fp contract(off)

namespace {

using namespace chm_cellshared;
using chm_symmshared::Atom;
using chm_symmshared::lands_on;

constexpr int kBlock = 256;     // four waves per crystal
constexpr int kMaxAtoms = 256;  // the LDS staging
constexpr int kMaxOps = CHM_SYMM_MAX_OPS;

using chm::fail;

struct SymmArgs {
  const chm_cell_record* rec;
  const long long* types;
  const float* x;
  const float* lat;
  const int* off;
  const int* require;  // NULL, or [1] (stride 0), or [B] (stride 1): the wanted system code
  int require_stride;
  float symprec, angle_tolerance;
  chm_symm_record* out;
  int4* ops;  // NULL, or [B, 48] slots of (candidate index, t0, t1, t2)
};

// (m, m2, m3, m4, m6) of the distinct proper parts -> the crystal system code, or -1
__device__ inline int crystal_system_of(int m, int m2, int m3, int m4, int m6) {
  if (m == 1 && m2 == 0 && m3 == 0 && m4 == 0 && m6 == 0) return CHM_SYMM_TRICLINIC;       // 1
  if (m == 2 && m2 == 1 && m3 == 0 && m4 == 0 && m6 == 0) return CHM_SYMM_MONOCLINIC;      // 2
  if (m == 4 && m2 == 3 && m3 == 0 && m4 == 0 && m6 == 0) return CHM_SYMM_ORTHORHOMBIC;    // 222
  if (m == 4 && m2 == 1 && m3 == 0 && m4 == 2 && m6 == 0) return CHM_SYMM_TETRAGONAL;      // 4
  if (m == 8 && m2 == 5 && m3 == 0 && m4 == 2 && m6 == 0) return CHM_SYMM_TETRAGONAL;      // 422
  if (m == 3 && m2 == 0 && m3 == 2 && m4 == 0 && m6 == 0) return CHM_SYMM_TRIGONAL;        // 3
  if (m == 6 && m2 == 3 && m3 == 2 && m4 == 0 && m6 == 0) return CHM_SYMM_TRIGONAL;        // 32
  if (m == 6 && m2 == 1 && m3 == 2 && m4 == 0 && m6 == 2) return CHM_SYMM_HEXAGONAL;       // 6
  if (m == 12 && m2 == 7 && m3 == 2 && m4 == 0 && m6 == 2) return CHM_SYMM_HEXAGONAL;      // 622
  if (m == 12 && m2 == 3 && m3 == 8 && m4 == 0 && m6 == 0) return CHM_SYMM_CUBIC;          // 23
  if (m == 24 && m2 == 9 && m3 == 8 && m4 == 6 && m6 == 0) return CHM_SYMM_CUBIC;          // 432
  return -1;
}

// t = x_j - x_p W for candidate idx, component k (x_p0 W[0][k] + x_p1 W[1][k]) + x_p2 W[2][k]; W as floats
__device__ inline void translation_of(const float* W, const float* xp, const float* xj, float* t) {
#pragma unroll
  for (int k = 0; k < 3; ++k) t[k] = xj[k] - ((xp[0] * W[k] + xp[1] * W[3 + k]) + xp[2] * W[6 + k]);
}

// LDS integers of the block
enum { I_NW = 0, I_MINCNT, I_PTYPE, I_NSYM, I_NTRANS, I_NPG, I_INV, I_M, I_M2, I_M3, I_M4, I_M6, I_COUNT };

// Block g (four waves) = crystal g.
__global__ __launch_bounds__(kBlock) void k_symm(SymmArgs p) {
  __shared__ Atom s_at[kMaxAtoms];
  __shared__ int s_raw[kMaxOps];    // accepted candidate indices as they arrived
  __shared__ int s_w[kMaxOps];      // ascending
  __shared__ int s_first[kMaxOps];  // per W the first accepted translation (position in the pivot list)
  __shared__ int s_piv[kMaxAtoms];  // the pivot species' atoms in node order
  __shared__ float s_L[9];
  __shared__ int s_i[I_COUNT];
  const int g = blockIdx.x, tid = threadIdx.x;
  const int n0 = p.off[g], n = p.off[g + 1] - n0;  // (1 <= n <= kMaxAtoms: chm_symm_create)
  const chm_cell_record* rec = p.rec + g;
  int T[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) T[q] = rec->transform[q];
  const int lsys = rec->system, lhalv = rec->halvings, n_ops = rec->n_ops;
  // (everything read from the cell record is the same in every thread: the branches on it are uniform)
  bool lattice = lsys >= 0 && lsys <= CHM_CELL_CUBIC && lhalv >= 0 && lhalv <= kMaxHalvings && n_ops >= 1 && n_ops <= kMaxOps;

  if (tid < 9) s_L[tid] = reduced_entry(T, p.lat + (long)g * 9, tid);
  if (tid < n) {
    double adj[9];  // (the same in every thread, from registers: sharing it would cost a barrier more than it saves)
    adjugate(T, adj);
    reduced_frac(adj, p.x + 3 * ((long)n0 + tid), s_at[tid].x);
    s_at[tid].type = (int)p.types[(long)n0 + tid];
  }
  if (tid < kMaxOps) s_first[tid] = INT_MAX;
  if (tid < I_COUNT) s_i[tid] = (tid == I_MINCNT || tid == I_PTYPE) ? INT_MAX : 0;
  __syncthreads();
  float L[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) L[q] = s_L[q];

  // ---- the lattice operations of the record's final level, in ascending candidate order
  int nW = 0;
  if (lattice) {
    float len[3], ang[3];
    cell_metric(L, len, ang);
    const float scale = 1.0f / (float)(1 << lhalv);  // (a power of two: the product is exact)
    const float tl = p.symprec * scale, ta = p.angle_tolerance * scale;
    for (int idx = tid; idx < kCandidates; idx += kBlock) {
      int det, tr;
      if (candidate_accepted(idx, L, len, ang, tl, ta, &det, &tr)) {
        const int slot = atomicAdd(&s_i[I_NW], 1);
        if (slot < kMaxOps) s_raw[slot] = idx;
      }
    }
    __syncthreads();
    nW = s_i[I_NW];
    if (nW != n_ops) lattice = false;  // (uniform: from LDS behind a barrier; the record is of another lattice or tolerance)
  }
  if (lattice) {
    if (tid < nW) {
      const int mine = s_raw[tid];
      int rank = 0;
      for (int q = 0; q < nW; ++q) rank += s_raw[q] < mine;
      s_w[rank] = mine;
    }
    __syncthreads();
  }

  // ---- thin cells: one image per component is exact only while 2 symprec < the smallest plane spacing
  bool thin = false;
  if (lattice) {
    const float c0[3] = {L[4] * L[8] - L[5] * L[7], L[5] * L[6] - L[3] * L[8], L[3] * L[7] - L[4] * L[6]};  // a1 x a2
    const float c1[3] = {L[7] * L[2] - L[8] * L[1], L[8] * L[0] - L[6] * L[2], L[6] * L[1] - L[7] * L[0]};  // a2 x a0
    const float c2[3] = {L[1] * L[5] - L[2] * L[4], L[2] * L[3] - L[0] * L[5], L[0] * L[4] - L[1] * L[3]};  // a0 x a1
    const float vol = fabsf(dot3(L, c0));
    const float d0 = vol / sqrtf(dot3(c0, c0)), d1 = vol / sqrtf(dot3(c1, c1)), d2 = vol / sqrtf(dot3(c2, c2));
    thin = !(2.0f * p.symprec < fminf(fminf(d0, d1), d2));
  }
  const bool search = lattice && !thin;

  // ---- the pivot: the species with the fewest atoms (ties: the smallest type), its atoms in node order
  int n_piv = 0, pivot = 0;
  if (search) {
    const int my = tid < n ? s_at[tid].type : 0;
    int cnt = 0;
    if (tid < n) {
      for (int q = 0; q < n; ++q) cnt += s_at[q].type == my;
      atomicMin(&s_i[I_MINCNT], cnt);
    }
    __syncthreads();
    n_piv = s_i[I_MINCNT];
    if (tid < n && cnt == n_piv) atomicMin(&s_i[I_PTYPE], my);
    __syncthreads();
    const int ptype = s_i[I_PTYPE];
    if (tid < n && my == ptype) {
      int rank = 0;
      for (int q = 0; q < tid; ++q) rank += s_at[q].type == ptype;
      s_piv[rank] = tid;
    }
    __syncthreads();
    pivot = s_piv[0];
  }

  // ---- the atom search, level by level
  int code = -1, halvings = 0;
  int c_sym = 0, c_trans = 0, c_pg = 0, c_inv = 0, c_m = 0, c_2 = 0, c_3 = 0, c_4 = 0, c_6 = 0;
  float tol = 0.f;
  if (thin) tol = p.symprec;
  if (search) {
    const int total = nW * n_piv;  // (<= 48 * 256)
    for (int h = 0; h <= kMaxHalvings; ++h) {
      tol = p.symprec * (1.0f / (float)(1 << h));
      const float tol2 = tol * tol;
      for (int c = tid; c < total; c += kBlock) {
        const int w = c / n_piv, jj = c - w * n_piv;
        const int idx = s_w[w];
        int Wi[9], det, tr;
        decode_candidate(idx, Wi, &det, &tr);
        float W[9];
#pragma unroll
        for (int q = 0; q < 9; ++q) W[q] = (float)Wi[q];
        float t[3];
        translation_of(W, s_at[pivot].x, s_at[s_piv[jj]].x, t);
        bool ok = true;
        for (int i = 0; i < n && ok; ++i) {
          const Atom a = s_at[i];
          float y[3];
#pragma unroll
          for (int k = 0; k < 3; ++k) y[k] = ((a.x[0] * W[k] + a.x[1] * W[3 + k]) + a.x[2] * W[6 + k]) + t[k];
          bool found = false;
          for (int q = 0; q < n && !found; ++q) {
            const Atom b = s_at[q];
            if (b.type != a.type) continue;
            found = lands_on(y, b.x, L, tol2);  // (symm_shared.h: the test k_prim runs too)
          }
          ok = found;
        }
        if (ok) {
          atomicAdd(&s_i[I_NSYM], 1);
          if (idx == kIdentityIndex) atomicAdd(&s_i[I_NTRANS], 1);
          atomicMin(&s_first[w], jj);
        }
      }
      __syncthreads();
      // the point group: the W with a translation, and their distinct proper parts det(W) W
      if (tid < nW && s_first[tid] != INT_MAX) {
        const int idx = s_w[tid];
        int Wi[9], det, tr;
        decode_candidate(idx, Wi, &det, &tr);
        atomicAdd(&s_i[I_NPG], 1);
        if (idx == kCandidates - 1 - kIdentityIndex) s_i[I_INV] = 1;
        bool fresh = true;  // an improper W whose -W is in the group too adds no proper part
        if (det == -1)
          for (int q = 0; q < nW; ++q) fresh &= !(s_w[q] == kCandidates - 1 - idx && s_first[q] != INT_MAX);
        if (fresh) {
          const int ptr = det * tr;
          atomicAdd(&s_i[I_M], 1);
          if (ptr == -1) atomicAdd(&s_i[I_M2], 1);
          if (ptr == 0) atomicAdd(&s_i[I_M3], 1);
          if (ptr == 1) atomicAdd(&s_i[I_M4], 1);
          if (ptr == 2) atomicAdd(&s_i[I_M6], 1);
        }
      }
      __syncthreads();
      c_sym = s_i[I_NSYM], c_trans = s_i[I_NTRANS], c_pg = s_i[I_NPG], c_inv = s_i[I_INV], c_m = s_i[I_M];
      c_2 = s_i[I_M2], c_3 = s_i[I_M3], c_4 = s_i[I_M4], c_6 = s_i[I_M6];
      halvings = h;
      code = crystal_system_of(c_m, c_2, c_3, c_4, c_6);
      if (!(c_sym == c_pg * c_trans && c_pg == c_m * (1 + c_inv))) code = -1;
      if (code >= 0 || h == kMaxHalvings) break;  // (uniform: the counts came from LDS behind a barrier)
      __syncthreads();  // (every thread has read the counts and s_first before they are cleared)
      if (tid < kMaxOps) s_first[tid] = INT_MAX;
      if (tid >= I_NSYM && tid < I_COUNT) s_i[tid] = 0;
      __syncthreads();
    }
  }

  // ---- the operations: one slot per W of the point group, ascending, with its first translation
  if (p.ops) {
    int4* slots = p.ops + (long)g * kMaxOps;
    if (tid < kMaxOps && tid >= c_pg) slots[tid] = make_int4(-1, 0, 0, 0);
    if (search && tid < nW && s_first[tid] != INT_MAX) {
      int rank = 0;
      for (int q = 0; q < tid; ++q) rank += s_first[q] != INT_MAX;
      const int idx = s_w[tid];
      int Wi[9], det, tr;
      decode_candidate(idx, Wi, &det, &tr);
      float W[9], t[3];
#pragma unroll
      for (int q = 0; q < 9; ++q) W[q] = (float)Wi[q];
      translation_of(W, s_at[pivot].x, s_at[s_piv[s_first[tid]]].x, t);
      slots[rank] = make_int4(idx, __float_as_int(t[0]), __float_as_int(t[1]), __float_as_int(t[2]));
    }
  }
  if (tid != 0) return;
  int flags = 0;
  if (!lattice) flags |= CHM_SYMM_NO_LATTICE;
  if (thin) flags |= CHM_SYMM_THIN;
  if (search && code < 0) flags |= CHM_SYMM_AMBIGUOUS;
  if (p.require && p.require[(long)g * p.require_stride] != code) flags |= CHM_SYMM_MISMATCH;
  int4* oi = reinterpret_cast<int4*>(p.out + g);
  oi[0] = make_int4(code, c_sym, c_trans, c_pg);
  oi[1] = make_int4(c_m, c_2, c_3, c_4);
  oi[2] = make_int4(c_6, c_inv, halvings, flags);
  oi[3] = make_int4(n_piv, lattice ? lsys : -1, __float_as_int(tol), 0);
}

}  // namespace

struct chm_symm : chm::NodePlan {};

extern "C" int chm_symm_create(const int32_t* h_natoms, int num_graphs, chm_symm** out) {
  static_assert(sizeof(chm_symm_record) == 64, "the record is 64 bytes");
  return chm::node_plan_create(h_natoms, num_graphs, {"symmetry plan", kMaxAtoms, "the symmetry search"},
                               "chm_symm_create", out);
}

extern "C" void chm_symm_destroy(chm_symm* p) { chm::node_plan_destroy(p); }

extern "C" int chm_symm_run(const chm_symm* p, const void* d_cell_records, size_t n_record_bytes,
                            const int64_t* d_atom_types, int64_t n_atom_types, const float* d_frac, int64_t n_frac,
                            const float* d_lattices, int64_t n_lattices, const int32_t* d_require, int64_t n_require,
                            float symprec, float angle_tolerance, void* d_out, size_t n_out_bytes, void* d_ops,
                            size_t n_ops_bytes, void* stream) {
  if (!p) return fail(CHM_E_ARG, "symmetry plan is NULL");
  const chm::Check c{"the symmetry plan"};
  int rc, require_stride;
  if ((rc = c.count(d_cell_records, (long)n_record_bytes, 128L * p->B, "cell records", "bytes"))) return rc;
  if ((rc = c.aligned16(d_cell_records, "cell records"))) return rc;
  if ((rc = c.count(d_atom_types, n_atom_types, p->N, "atom_types [N]"))) return rc;
  if ((rc = c.count(d_frac, n_frac, 3 * p->N, "frac [N,3]"))) return rc;
  if ((rc = c.count(d_lattices, n_lattices, 9L * p->B, "lattices [B,3,3]"))) return rc;
  if ((rc = c.broadcast(d_require, n_require, 1, p->B, "require", "[B]", &require_stride))) return rc;
  if ((rc = c.range(symprec, CHM_CELL_MAX_SYMPREC, "symprec", " A"))) return rc;
  if ((rc = c.range(angle_tolerance, CHM_CELL_MAX_ANGLE_TOLERANCE, "angle_tolerance", " degrees"))) return rc;
  if ((rc = c.count(d_out, (long)n_out_bytes, 64L * p->B, "out", "bytes"))) return rc;
  if ((rc = c.aligned16(d_out, "out"))) return rc;
  if ((rc = c.optional(d_ops, (long)n_ops_bytes, 16L * kMaxOps * p->B, "ops", "bytes"))) return rc;
  if ((rc = c.aligned16(d_ops, "ops"))) return rc;
  SymmArgs a;
  a.rec = static_cast<const chm_cell_record*>(d_cell_records);
  a.types = reinterpret_cast<const long long*>(d_atom_types);
  a.x = d_frac;
  a.lat = d_lattices;
  a.off = p->d_off;
  a.require = d_require;
  a.require_stride = require_stride;
  a.symprec = symprec;
  a.angle_tolerance = angle_tolerance;
  a.out = static_cast<chm_symm_record*>(d_out);
  a.ops = static_cast<int4*>(d_ops);
  hipLaunchKernelGGL(k_symm, dim3(p->B), dim3(kBlock), 0, (hipStream_t)stream, a);
  HIPCHK(hipGetLastError());
  return CHM_OK;
}
