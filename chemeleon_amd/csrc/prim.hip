// Primitive cells of finished structures on the device (chm_prim_*, include/chemeleon_hip.h): per crystal the pure
// translations that carry the atoms onto themselves are found as k_symm finds them (the same pivot, the same
// distance test, symm_shared.h, in the same reduced basis, cell_shared.h), turned into an integer lattice whose
// Hermite normal form H names the primitive basis Lp = H Lr / m, and one atom per orbit of the translations is
// kept. The plan (chm_prim) is independent of chm_model / chm_batch, like chm_symm: node offsets, uploaded once.
//
// k_prim: one 256-thread block per crystal, atoms staged in LDS, one candidate translation per thread with an
// early exit at the first atom without a partner; every count is an integer add or min in LDS and H is computed
// on one lane in 64-bit integers, so the record does not depend on any order. It writes the record, Lp and per
// input atom its rank among the kept atoms (or -1). k_prim_offsets turns the records' n_prim into the new node
// offsets (one block, a chunked integer scan); k_prim_pack gathers types and coordinates to new_off[g] + rank, into
// buffers that k_prim_clear zeroed first.
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

// Every product and sum is rounded on its own (as in symm.hip).
#pragma clang fp contract(off)

namespace {

using namespace chm_cellshared;
using chm_symmshared::Atom;
using chm_symmshared::lands_on;

constexpr int kBlock = 256;     // four waves per crystal
constexpr int kMaxAtoms = 256;  // the LDS staging

using chm::fail;

struct PrimArgs {
  const chm_cell_record* rec;
  const long long* types;
  const float* x;
  const float* lat;
  const int* off;
  float symprec, angle_tolerance;
  chm_prim_record* out;
  float* lat_out;  // [B,9]
  int* source;     // [N] rank among the kept atoms of the crystal, or -1
};

struct PackArgs {
  const chm_cell_record* rec;
  const chm_prim_record* prim;
  const long long* types;
  const float* x;
  const int* off;
  const int* new_off;
  const int* source;
  long long* types_out;
  float* x_out;
};

// g = gcd(a, b) = u a + v b for a > 0, b >= 0
__device__ inline long long egcd(long long a, long long b, long long* u, long long* v) {
  long long r0 = a, r1 = b, u0 = 1, u1 = 0, v0 = 0, v1 = 1;
  while (r1 != 0) {
    const long long q = r0 / r1, r2 = r0 - q * r1, u2 = u0 - q * u1, v2 = v0 - q * v1;
    r0 = r1, r1 = r2, u0 = u1, u1 = u2, v0 = v1, v1 = v2;
  }
  *u = u0, *v = v0;
  return r0;
}

__device__ inline long long mod_pos(long long a, long long m) {
  const long long r = a % m;
  return r < 0 ? r + m : r;
}

// H = (h0 h1 h2 / 0 h3 h4 / 0 0 h5), the row Hermite normal form of a lattice that contains m Z^3; adds the
// generator v (entries in [0, m)) and returns to the normal form. Entries stay below m: every reduction modulo m
// subtracts a multiple of m e_k, which lies in the span of the rows below the one that is reduced.
__device__ inline void hnf_add(long long* H, const int* vi, long long m) {
  long long v[3] = {vi[0], vi[1], vi[2]};
  long long u, w;
  if (v[0] != 0) {
    const long long g = egcd(H[0], v[0], &u, &w), a = H[0] / g, b = v[0] / g;
    const long long r1 = u * H[1] + w * v[1], r2 = u * H[2] + w * v[2];
    v[1] = mod_pos(a * v[1] - b * H[1], m);
    v[2] = mod_pos(a * v[2] - b * H[2], m);
    H[0] = g, H[1] = mod_pos(r1, m), H[2] = mod_pos(r2, m);
  }
  if (v[1] != 0) {
    const long long g = egcd(H[3], v[1], &u, &w), a = H[3] / g, b = v[1] / g;
    const long long r2 = u * H[4] + w * v[2];
    v[2] = mod_pos(a * v[2] - b * H[4], m);
    H[3] = g, H[4] = mod_pos(r2, m);
  }
  if (v[2] != 0) H[5] = egcd(H[5], v[2], &u, &w);
  // 0 <= H[i][k] < H[k][k] above the diagonal: column 1 with row 1, then column 2 with row 2
  {
    const long long q = (H[1] - mod_pos(H[1], H[3])) / H[3];
    H[1] -= q * H[3];
    H[2] -= q * H[4];
  }
  H[2] = mod_pos(H[2], H[5]);
  H[4] = mod_pos(H[4], H[5]);
}

// LDS integers of the block
enum { I_NW = 0, I_MINCNT, I_PTYPE, I_M, I_BAD, I_KEPT, I_OK, I_COUNT };

// Block g (four waves) = crystal g.
__global__ __launch_bounds__(kBlock) void k_prim(PrimArgs p) {
  __shared__ Atom s_at[kMaxAtoms];
  __shared__ int s_piv[kMaxAtoms];   // the pivot species' atoms in node order
  __shared__ int s_acc[kMaxAtoms];   // per position of the pivot list: is t_j accepted at this level
  __shared__ int s_q[kMaxAtoms][3];  // q_j of the accepted ones
  __shared__ int s_keep[kMaxAtoms];  // per atom: no partner of a lower index (condition d)
  __shared__ float s_L[9];
  __shared__ int s_H[6];
  __shared__ int s_i[I_COUNT];
  const int g = blockIdx.x, tid = threadIdx.x;
  const int n0 = p.off[g], n = p.off[g + 1] - n0;  // (1 <= n <= kMaxAtoms: chm_prim_create)
  const chm_cell_record* rec = p.rec + g;
  int T[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) T[q] = rec->transform[q];
  const int lsys = rec->system, lhalv = rec->halvings, n_ops = rec->n_ops;
  // (everything read from the cell record is the same in every thread: the branches on it are uniform)
  bool lattice = lsys >= 0 && lsys <= CHM_CELL_CUBIC && lhalv >= 0 && lhalv <= kMaxHalvings && n_ops >= 1 &&
                 n_ops <= CHM_SYMM_MAX_OPS;

  if (tid < 9) s_L[tid] = reduced_entry(T, p.lat + (long)g * 9, tid);
  if (tid < n) {
    double adj[9];
    adjugate(T, adj);
    reduced_frac(adj, p.x + 3 * ((long)n0 + tid), s_at[tid].x);
    s_at[tid].type = (int)p.types[(long)n0 + tid];
  }
  if (tid < I_COUNT) s_i[tid] = (tid == I_MINCNT || tid == I_PTYPE) ? INT_MAX : 0;
  __syncthreads();
  float L[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) L[q] = s_L[q];

  // ---- the NO_LATTICE rule of k_symm: the record's final level must be found again with n_ops operations
  if (lattice) {
    float len[3], ang[3];
    cell_metric(L, len, ang);
    const float scale = 1.0f / (float)(1 << lhalv);  // (a power of two: the product is exact)
    const float tl = p.symprec * scale, ta = p.angle_tolerance * scale;
    for (int idx = tid; idx < kCandidates; idx += kBlock) {
      int det, tr;
      if (candidate_accepted(idx, L, len, ang, tl, ta, &det, &tr)) atomicAdd(&s_i[I_NW], 1);
    }
    __syncthreads();
    if (s_i[I_NW] != n_ops) lattice = false;  // (uniform: from LDS behind a barrier)
  }

  // ---- the THIN rule of k_symm
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

  // ---- the pivot of k_symm: the species with the fewest atoms (ties: the smallest type), its atoms in node order
  int n_piv = 0, pivot = 0, cnt = 0;  // cnt: the atoms of this thread's atom's species
  if (search) {
    const int my = tid < n ? s_at[tid].type : 0;
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

  // ---- the translations, level by level
  int halvings = 0, m = 0;
  bool consistent = false;
  float tol = 0.f;
  if (thin) tol = p.symprec;
  if (search) {
    for (int h = 0; h <= kMaxHalvings; ++h) {
      tol = p.symprec * (1.0f / (float)(1 << h));
      const float tol2 = tol * tol;
      // t_j = x'_j - x'_p: accepted when every atom moved by it lands on one of its type
      float t[3] = {0.f, 0.f, 0.f};
      if (tid < n_piv) {
#pragma unroll
        for (int k = 0; k < 3; ++k) t[k] = s_at[s_piv[tid]].x[k] - s_at[pivot].x[k];
        bool ok = true;
        for (int i = 0; i < n && ok; ++i) {
          const Atom a = s_at[i];
          const float y[3] = {a.x[0] + t[0], a.x[1] + t[1], a.x[2] + t[2]};
          bool found = false;
          for (int q = 0; q < n && !found; ++q) {
            const Atom b = s_at[q];
            if (b.type != a.type) continue;
            found = lands_on(y, b.x, L, tol2);
          }
          ok = found;
        }
        s_acc[tid] = ok;
        if (ok) atomicAdd(&s_i[I_M], 1);
      }
      __syncthreads();
      m = s_i[I_M];
      // per accepted t_j: q_j = rint(m t_j) mod m and condition (c); per atom: conditions (a) and (d)
      if (tid < n_piv && s_acc[tid]) {  // (m >= 1 here)
        const float fm = (float)m;
        float r[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          int qi = (int)rintf(fm * t[k]) % m;
          if (qi < 0) qi += m;
          s_q[tid][k] = qi;
          r[k] = (float)qi / fm;
        }
        if (!lands_on(t, r, L, tol2)) atomicAdd(&s_i[I_BAD], 1);
      }
      if (tid < n) {
        if (m >= 1 && cnt % m != 0) atomicAdd(&s_i[I_BAD], 1);
        const Atom a = s_at[tid];
        bool lower = false;  // is some partner(tid, j) < tid
        for (int jj = 0; jj < n_piv && !lower; ++jj) {
          if (!s_acc[jj]) continue;
          float y[3];
#pragma unroll
          for (int k = 0; k < 3; ++k) y[k] = a.x[k] + (s_at[s_piv[jj]].x[k] - s_at[pivot].x[k]);
          for (int q = 0; q < tid && !lower; ++q) {
            const Atom b = s_at[q];
            if (b.type != a.type) continue;
            lower = lands_on(y, b.x, L, tol2);
          }
        }
        s_keep[tid] = !lower;
        if (!lower) atomicAdd(&s_i[I_KEPT], 1);
      }
      __syncthreads();
      // the Hermite normal form and conditions (b) and (d), on one lane in 64-bit integers
      if (tid == 0) {
        bool ok = m >= 1 && s_i[I_BAD] == 0 && (long long)s_i[I_KEPT] * m == n;
        long long H[6] = {m, 0, 0, m, 0, m};
        if (ok) {
          for (int jj = 0; jj < n_piv; ++jj)
            if (s_acc[jj]) hnf_add(H, s_q[jj], m);
          ok = H[0] * H[3] * H[5] == (long long)m * m;
        }
#pragma unroll
        for (int q = 0; q < 6; ++q) s_H[q] = (int)H[q];  // (entries <= m <= 256)
        s_i[I_OK] = ok;
      }
      __syncthreads();
      consistent = s_i[I_OK] != 0;
      halvings = h;
      if (consistent || h == kMaxHalvings) break;  // (uniform: from LDS behind a barrier)
      if (tid == I_M || tid == I_BAD || tid == I_KEPT) s_i[tid] = 0;  // (m and the decision are in registers)
      __syncthreads();
    }
  }

  // ---- the output: the primitive cell, or the crystal as it is in the reduced basis
  const bool reduced = search && consistent && m > 1;
  if (tid < n) {
    int rank = tid;
    if (reduced) {
      rank = 0;
      for (int q = 0; q < tid; ++q) rank += s_keep[q];
      if (!s_keep[tid]) rank = -1;
    }
    p.source[(long)n0 + tid] = rank;
  }
  if (tid < 9) {
    float v = L[tid];
    if (reduced) {
      const int i = tid / 3, k = tid - 3 * i;
      const double h0 = i == 0 ? (double)s_H[0] : 0.0, h1 = i == 0 ? (double)s_H[1] : i == 1 ? (double)s_H[3] : 0.0,
                   h2 = i == 0 ? (double)s_H[2] : i == 1 ? (double)s_H[4] : (double)s_H[5];
      v = (float)(((h0 * (double)L[k] + h1 * (double)L[3 + k]) + h2 * (double)L[6 + k]) / (double)m);
    }
    p.lat_out[(long)g * 9 + tid] = v;
  }
  if (tid != 0) return;
  int flags = 0;
  if (!lattice) flags |= CHM_PRIM_NO_LATTICE;
  if (thin) flags |= CHM_PRIM_THIN;
  if (search && !consistent) flags |= CHM_PRIM_AMBIGUOUS;
  int4* oi = reinterpret_cast<int4*>(p.out + g);
  oi[0] = make_int4(reduced ? n / m : n, m, n_piv, halvings);
  oi[1] = reduced ? make_int4(flags, s_H[0], s_H[1], s_H[2]) : make_int4(flags, 1, 0, 0);
  oi[2] = reduced ? make_int4(s_H[3], s_H[4], s_H[5], __float_as_int(tol)) : make_int4(1, 0, 1, __float_as_int(tol));
  oi[3] = make_int4(lattice ? lsys : -1, 0, 0, 0);
}

// Zeroes the packed outputs (types [N], coordinates [N,3]) before anything is gathered into them. A kernel and not
// hipMemsetAsync: a captured hipMemsetAsync of these buffers left other bytes than zero behind the packed rows
// when the graph was replayed (tests/test_gpu_primitive.py, the graph test), while plain stores replay as they ran.
__global__ __launch_bounds__(kBlock) void k_prim_clear(long long* types_out, float* x_out, long N) {
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < N; i += (long)gridDim.x * kBlock) {
    types_out[i] = 0;
    x_out[3 * i] = 0.f;
    x_out[3 * i + 1] = 0.f;
    x_out[3 * i + 2] = 0.f;
  }
}

// new_off[0] = 0, new_off[g + 1] = n_prim[0] + ... + n_prim[g]: one block, 256 records per round (integers only)
__global__ __launch_bounds__(kBlock) void k_prim_offsets(const chm_prim_record* rec, int B, int* new_off) {
  __shared__ int s[kBlock];
  __shared__ int s_carry;
  const int tid = threadIdx.x;
  if (tid == 0) {
    s_carry = 0;
    new_off[0] = 0;
  }
  __syncthreads();
  for (int base = 0; base < B; base += kBlock) {  // (B is the same in every thread: the barriers are uniform)
    const int g = base + tid;
    s[tid] = g < B ? rec[g].n_prim : 0;
    __syncthreads();
    for (int d = 1; d < kBlock; d <<= 1) {
      const int add = tid >= d ? s[tid - d] : 0;
      __syncthreads();
      s[tid] += add;
      __syncthreads();
    }
    const int carry = s_carry;
    if (g < B) new_off[g + 1] = carry + s[tid];
    __syncthreads();
    if (tid == kBlock - 1) s_carry = carry + s[tid];
    __syncthreads();
  }
}

// Block g = crystal g: the kept atoms' types and coordinates to new_off[g] + rank.
__global__ __launch_bounds__(kBlock) void k_prim_pack(PackArgs p) {
  const int g = blockIdx.x, tid = threadIdx.x;
  const int n0 = p.off[g], n = p.off[g + 1] - n0;
  if (tid >= n) return;
  const int4* pr = reinterpret_cast<const int4*>(p.prim + g);
  const int4 r0 = pr[0], r1 = pr[1], r2 = pr[2];
  const int n_prim = r0.x, m = r0.y;
  const int rank = p.source[(long)n0 + tid];
  if (rank < 0 || rank >= n_prim) return;  // (rank < n_prim for every kept atom: condition (d))
  const long dst = (long)p.new_off[g] + rank;  // (< new_off[g + 1] <= N)
  int T[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) T[q] = p.rec[g].transform[q];
  double adj[9];
  adjugate(T, adj);
  float xr[3];
  reduced_frac(adj, p.x + 3 * ((long)n0 + tid), xr);
  if (n_prim < n) {  // x_p = frac(x' adj(H) / m), fp64, rounded once
    const int H[9] = {r1.y, r1.z, r1.w, 0, r2.x, r2.y, 0, 0, r2.z};
    adjugate(H, adj);
    const double x0 = (double)xr[0], x1 = (double)xr[1], x2 = (double)xr[2], dm = (double)m;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double y = ((x0 * adj[k] + x1 * adj[3 + k]) + x2 * adj[6 + k]) / dm;
      float f = (float)(y - floor(y));
      if (f >= 1.0f) f = 0.0f;  // (as reduced_frac)
      xr[k] = f;
    }
  }
  p.types_out[dst] = p.types[(long)n0 + tid];
  p.x_out[3 * dst] = xr[0];
  p.x_out[3 * dst + 1] = xr[1];
  p.x_out[3 * dst + 2] = xr[2];
}

}  // namespace

struct chm_prim : chm::NodePlan {};

extern "C" int chm_prim_create(const int32_t* h_natoms, int num_graphs, chm_prim** out) {
  static_assert(sizeof(chm_prim_record) == 64, "the record is 64 bytes");
  return chm::node_plan_create(h_natoms, num_graphs, {"primitive-cell plan", kMaxAtoms, "the primitive-cell search"},
                               "chm_prim_create", out);
}

extern "C" void chm_prim_destroy(chm_prim* p) { chm::node_plan_destroy(p); }

extern "C" int chm_prim_run(const chm_prim* p, const void* d_cell_records, size_t n_record_bytes,
                            const int64_t* d_atom_types, int64_t n_atom_types, const float* d_frac, int64_t n_frac,
                            const float* d_lattices, int64_t n_lattices, float symprec, float angle_tolerance,
                            void* d_out, size_t n_out_bytes, int32_t* d_source, int64_t n_source,
                            int32_t* d_new_offsets, int64_t n_new_offsets, int64_t* d_atom_types_out,
                            int64_t n_atom_types_out, float* d_frac_out, int64_t n_frac_out, float* d_lattices_out,
                            int64_t n_lattices_out, void* stream) {
  if (!p) return fail(CHM_E_ARG, "primitive-cell plan is NULL");
  const chm::Check c{"the primitive-cell plan"};
  int rc;
  if ((rc = c.count(d_cell_records, (long)n_record_bytes, 128L * p->B, "cell records", "bytes"))) return rc;
  if ((rc = c.aligned16(d_cell_records, "cell records"))) return rc;
  if ((rc = c.count(d_atom_types, n_atom_types, p->N, "atom_types [N]"))) return rc;
  if ((rc = c.count(d_frac, n_frac, 3 * p->N, "frac [N,3]"))) return rc;
  if ((rc = c.count(d_lattices, n_lattices, 9L * p->B, "lattices [B,3,3]"))) return rc;
  if ((rc = c.range(symprec, CHM_CELL_MAX_SYMPREC, "symprec", " A"))) return rc;
  if ((rc = c.range(angle_tolerance, CHM_CELL_MAX_ANGLE_TOLERANCE, "angle_tolerance", " degrees"))) return rc;
  if ((rc = c.count(d_out, (long)n_out_bytes, 64L * p->B, "out", "bytes"))) return rc;
  if ((rc = c.aligned16(d_out, "out"))) return rc;
  if ((rc = c.count(d_source, n_source, p->N, "source [N]"))) return rc;
  if ((rc = c.count(d_new_offsets, n_new_offsets, p->B + 1L, "new_offsets [B+1]"))) return rc;
  if ((rc = c.count(d_atom_types_out, n_atom_types_out, p->N, "atom_types_out [N]"))) return rc;
  if ((rc = c.count(d_frac_out, n_frac_out, 3 * p->N, "frac_out [N,3]"))) return rc;
  if ((rc = c.count(d_lattices_out, n_lattices_out, 9L * p->B, "lattices_out [B,3,3]"))) return rc;
  if (d_atom_types_out == d_atom_types)
    return fail(CHM_E_ARG, "atom_types_out must not be atom_types: the state is never changed in place");
  if (d_frac_out == d_frac) return fail(CHM_E_ARG, "frac_out must not be frac: the state is never changed in place");
  if (d_lattices_out == d_lattices)
    return fail(CHM_E_ARG, "lattices_out must not be lattices: the state is never changed in place");
  hipStream_t st = (hipStream_t)stream;
  // the rows past new_offsets[B] stay zero: every byte of the ragged outputs is defined
  const int clear_blocks = (int)((p->N + kBlock - 1) / kBlock < 1024 ? (p->N + kBlock - 1) / kBlock : 1024);
  hipLaunchKernelGGL(k_prim_clear, dim3(clear_blocks), dim3(kBlock), 0, st,
                     reinterpret_cast<long long*>(d_atom_types_out), d_frac_out, p->N);
  HIPCHK(hipGetLastError());
  PrimArgs a;
  a.rec = static_cast<const chm_cell_record*>(d_cell_records);
  a.types = reinterpret_cast<const long long*>(d_atom_types);
  a.x = d_frac;
  a.lat = d_lattices;
  a.off = p->d_off;
  a.symprec = symprec;
  a.angle_tolerance = angle_tolerance;
  a.out = static_cast<chm_prim_record*>(d_out);
  a.lat_out = d_lattices_out;
  a.source = d_source;
  hipLaunchKernelGGL(k_prim, dim3(p->B), dim3(kBlock), 0, st, a);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_prim_offsets, dim3(1), dim3(kBlock), 0, st, a.out, p->B, d_new_offsets);
  HIPCHK(hipGetLastError());
  PackArgs k;
  k.rec = a.rec;
  k.prim = a.out;
  k.types = a.types;
  k.x = d_frac;
  k.off = p->d_off;
  k.new_off = d_new_offsets;
  k.source = d_source;
  k.types_out = reinterpret_cast<long long*>(d_atom_types_out);
  k.x_out = d_frac_out;
  hipLaunchKernelGGL(k_prim_pack, dim3(p->B), dim3(kBlock), 0, st, k);
  HIPCHK(hipGetLastError());
  return CHM_OK;
}
