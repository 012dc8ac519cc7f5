// Lattice system and reduced cell of sampled structures on the device (chm_cell_*, include/chemeleon_hip.h): per
// crystal the Niggli-reduced cell Lr = T L, the tolerant set of integer matrices W (entries in {-1, 0, 1},
// |det W| = 1) that map Lr onto itself within symprec / angle_tolerance, and the holohedry read off that set's
// size and rotation orders, one 128-byte record each; k_cell_apply then writes the reduced lattices and the
// fractional coordinates in the reduced basis into caller buffers. The question is about the lattice alone
// (test_lattice_system_matching of the reference's scripts/evaluate.py); the plan (chm_cell) is independent of
// chm_model / chm_batch, like chm_screen: node offsets, uploaded once.
//
// The reduction is nine numbers of scalar work: lane 0 runs it in fp64 (the rows are recomputed from T and the
// input in every pass, so nothing drifts), rounds Lr to fp32 and leaves it in LDS. The search is the parallel
// part: the block's 256 threads walk the 3^9 = 19 683 candidate indices, decode the base-3 digits, take the
// determinant in integers and compare the lengths and angles of W Lr in fp32. Acceptance is counted per wave
// by ballot and popcount and across waves by integer adds in LDS, so the counts do not depend on any order.
#include <hip/hip_runtime.h>

#include <math.h>

#include <cstdint>
#include <string>
#include <vector>

#include "chm_host.h"
#include "plan_common.h"
#include "cell_shared.h"

// Every product and sum is rounded on its own, in fp32 and in fp64, so that the record is the same expression on
// every build (constrain.hip explains why the toolchain's __fmul_rn alone does not prevent contraction).
#pragma clang fp contract(off)

namespace {

using namespace chm_cellshared;  // dot3, angle_deg, the candidate test, the reduced cell: shared with symm.hip

constexpr int kBlock = 256;          // four waves per crystal (kCandidates = 3^9 = 76 * 256 + 227: the last pass has idle lanes)
constexpr int kMaxPasses = 100;      // cap of the reduction
constexpr int kMaxEntry = 32767;     // cap of |T|'s entries: products of two stay inside 2^31 and far inside fp64
constexpr double kNiggliEps = 1.0e-5;  // times V^(2/3): the comparisons are between squared lengths

using chm::fail;

struct CellArgs {
  const float* lat;
  const int* require;  // NULL, or [1] (stride 0), or [B] (stride 1): the wanted system code
  int require_stride;
  float symprec, angle_tolerance;
  chm_cell_record* out;
};

struct ApplyArgs {
  const float* x;
  const float* lat;
  const int* off;
  const chm_cell_record* rec;
  float* x_out;
  float* lat_out;
};

__device__ inline double dot3d(const double* u, const double* v) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }
__device__ inline double det3d(const double* m) {
  return (m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6])) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}
// R = T L in fp64, each entry (t0 l0 + t1 l1) + t2 l2
__device__ inline void rows_of(const int* T, const double* L, double* R) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k)
      R[3 * i + k] = ((double)T[3 * i] * L[k] + (double)T[3 * i + 1] * L[3 + k]) + (double)T[3 * i + 2] * L[6 + k];
}
__device__ inline int sign_eps(double v, double eps) { return fabs(v) < eps ? 0 : (v > 0 ? 1 : -1); }

// row i of T += k * row j, k an integer held in a double; false (and T unchanged) if k or an entry of the new row
// would exceed kMaxEntry: the reduction stops there and the cell is NOT_REDUCED
__device__ inline bool add_rows(int* T, int i, int j, double k) {
  if (!(fabs(k) <= (double)kMaxEntry)) return false;
  long long r[3];
  for (int q = 0; q < 3; ++q) {
    r[q] = (long long)T[3 * i + q] + (long long)k * (long long)T[3 * j + q];
    if (r[q] > kMaxEntry || r[q] < -kMaxEntry) return false;
  }
  for (int q = 0; q < 3; ++q) T[3 * i + q] = (int)r[q];
  return true;
}

// Krivy-Gruber reduction of a cell of volume > 0: T (integer, det +1) with T L reduced. Returns the passes
// taken; *done is false if the cap of the passes or of T's entries ended it (T holds what it has).
__device__ int niggli(const double* L, int* T, bool* done) {
  const double eps = kNiggliEps * (cbrt(fabs(det3d(L))) * cbrt(fabs(det3d(L))));
#pragma unroll
  for (int q = 0; q < 9; ++q) T[q] = (q % 4 == 0) ? 1 : 0;
  *done = false;
  for (int pass = 1; pass <= kMaxPasses; ++pass) {
    double R[9];
    rows_of(T, L, R);
    double A = dot3d(R, R), B = dot3d(R + 3, R + 3);
    const double C = dot3d(R + 6, R + 6);
    double E = 2.0 * dot3d(R + 3, R + 6), N = 2.0 * dot3d(R, R + 6), Y = 2.0 * dot3d(R, R + 3);
    if (A > B + eps || (fabs(A - B) < eps && fabs(E) > fabs(N) + eps)) {  // A1: a <-> b
      for (int k = 0; k < 3; ++k) {
        const int t0 = T[k], t1 = T[3 + k];
        T[k] = -t1;
        T[3 + k] = -t0;
        T[6 + k] = -T[6 + k];
      }
      double t = A;
      A = B;
      B = t;
      t = E;
      E = N;
      N = t;
    }
    if (B > C + eps || (fabs(B - C) < eps && fabs(N) > fabs(Y) + eps)) {  // A2: b <-> c
      for (int k = 0; k < 3; ++k) {
        const int t1 = T[3 + k], t2 = T[6 + k];
        T[k] = -T[k];
        T[3 + k] = -t2;
        T[6 + k] = -t1;
      }
      continue;
    }
    const int l = sign_eps(E, eps), m = sign_eps(N, eps), n = sign_eps(Y, eps);
    int i, j, k;
    if (l * m * n == 1) {  // A3: all angles acute
      i = l == -1 ? -1 : 1;
      j = m == -1 ? -1 : 1;
      k = n == -1 ? -1 : 1;
    } else {  // A4: all angles obtuse or right
      i = l == 1 ? -1 : 1;
      j = m == 1 ? -1 : 1;
      k = n == 1 ? -1 : 1;
      if (i * j * k == -1) {
        if (n == 0) k = -1;
        else if (m == 0) j = -1;
        else if (l == 0) i = -1;
      }
    }
    for (int q = 0; q < 3; ++q) {
      T[q] *= i;
      T[3 + q] *= j;
      T[6 + q] *= k;
    }
    E = (double)(j * k) * E;
    N = (double)(i * k) * N;
    Y = (double)(i * j) * Y;
    // A5-A7 take the whole multiple at once where the off-diagonal term exceeds the diagonal one (a cell sheared
    // by k rows needs one pass, not k); on the boundary cases they take the unit step of the published rules
    if (fabs(E) > B + eps) {  // A5
      if (!add_rows(T, 2, 1, -rint(E / (2.0 * B)))) return pass;
      continue;
    }
    if ((fabs(E - B) < eps && 2.0 * N < Y - eps) || (fabs(E + B) < eps && Y < -eps)) {
      if (!add_rows(T, 2, 1, E > 0 ? -1.0 : 1.0)) return pass;
      continue;
    }
    if (fabs(N) > A + eps) {  // A6
      if (!add_rows(T, 2, 0, -rint(N / (2.0 * A)))) return pass;
      continue;
    }
    if ((fabs(N - A) < eps && 2.0 * E < Y - eps) || (fabs(N + A) < eps && Y < -eps)) {
      if (!add_rows(T, 2, 0, N > 0 ? -1.0 : 1.0)) return pass;
      continue;
    }
    if (fabs(Y) > A + eps) {  // A7
      if (!add_rows(T, 1, 0, -rint(Y / (2.0 * A)))) return pass;
      continue;
    }
    if ((fabs(Y - A) < eps && 2.0 * E < N - eps) || (fabs(Y + A) < eps && N < -eps)) {
      if (!add_rows(T, 1, 0, Y > 0 ? -1.0 : 1.0)) return pass;
      continue;
    }
    const double sum = E + N + Y + A + B;
    if (sum < -eps || (fabs(sum) < eps && 2.0 * (A + N) + Y > eps)) {  // A8
      if (!add_rows(T, 2, 0, 1.0) || !add_rows(T, 2, 1, 1.0)) return pass;
      continue;
    }
    *done = true;
    return pass;
  }
  return kMaxPasses;
}

// (n, n2, n3, n4, n6) -> the system code, or -1 where the tolerant set is no holohedry
__device__ inline int system_of(int n, int n2, int n3, int n4, int n6) {
  if (n == 2 && n2 == 0 && n3 == 0 && n4 == 0 && n6 == 0) return CHM_CELL_TRICLINIC;
  if (n == 4 && n2 == 1 && n3 == 0 && n4 == 0 && n6 == 0) return CHM_CELL_MONOCLINIC;
  if (n == 8 && n2 == 3 && n3 == 0 && n4 == 0 && n6 == 0) return CHM_CELL_ORTHORHOMBIC;
  if (n == 16 && n2 == 5 && n3 == 0 && n4 == 2 && n6 == 0) return CHM_CELL_TETRAGONAL;
  if (n == 12 && n2 == 3 && n3 == 2 && n4 == 0 && n6 == 0) return CHM_CELL_RHOMBOHEDRAL;
  if (n == 24 && n2 == 7 && n3 == 2 && n4 == 0 && n6 == 2) return CHM_CELL_HEXAGONAL;
  if (n == 48 && n2 == 9 && n3 == 8 && n4 == 6 && n6 == 0) return CHM_CELL_CUBIC;
  return -1;
}

// Block g (four waves) = crystal g.
__global__ __launch_bounds__(kBlock) void k_cell(CellArgs p) {
  __shared__ float s_L[9];   // the reduced cell (the input cell where nothing was reduced)
  __shared__ int s_T[9];
  __shared__ int s_head[3];  // flags so far, passes, skip the search?
  __shared__ int s_cnt[5];   // n, n2, n3, n4, n6 of the current level
  const int g = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) {
    double L[9];
    bool finite = true;
#pragma unroll
    for (int q = 0; q < 9; ++q) {
      const float v = p.lat[(long)g * 9 + q];
      finite &= isfinite(v);
      L[q] = (double)v;
      s_L[q] = v;
      s_T[q] = (q % 4 == 0) ? 1 : 0;
    }
    int flags = 0, passes = 0;
    if (!finite) flags = CHM_CELL_NONFINITE;
    else if (!(fabs(det3d(L)) > 0.0)) flags = CHM_CELL_DEGENERATE;
    if (!flags) {
      int T[9];
      bool done;
      passes = niggli(L, T, &done);
      if (!done) flags |= CHM_CELL_NOT_REDUCED;
      double R[9];
      rows_of(T, L, R);
#pragma unroll
      for (int q = 0; q < 9; ++q) {
        s_L[q] = (float)R[q];
        s_T[q] = T[q];
      }
    }
    s_head[0] = flags;
    s_head[1] = passes;
    s_head[2] = flags ? 1 : 0;  // (the search means something on a reduced cell only)
  }
  __syncthreads();
  float L[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) L[q] = s_L[q];
  const bool skip = s_head[2] != 0;  // (uniform over the block: read behind the barrier)
  // the cell's own lengths and angles (every thread computes the same values)
  float len[3], ang[3];
  cell_metric(L, len, ang);
  const float l0 = len[0], l1 = len[1], l2 = len[2], al = ang[0], be = ang[1], ga = ang[2];

  int cnt[5] = {0, 0, 0, 0, 0};
  int code = -1, halvings = 0;
  if (!skip) {
    for (int h = 0; h <= kMaxHalvings; ++h) {
      const float scale = 1.0f / (float)(1 << h);  // (a power of two: the product is exact)
      const float tl = p.symprec * scale, ta = p.angle_tolerance * scale;
      if (tid < 5) s_cnt[tid] = 0;
      __syncthreads();
      int w_n = 0, w_2 = 0, w_3 = 0, w_4 = 0, w_6 = 0;  // this wave's counts (the same in all its lanes)
      for (int base = 0; base < kCandidates; base += kBlock) {  // (the trip count is uniform: ballots are whole)
        const int idx = base + tid;
        bool acc = false;
        int det = 0, tr = 0;
        if (idx < kCandidates)  // (tail lanes of the last pass take no part)
          acc = candidate_accepted(idx, L, len, ang, tl, ta, &det, &tr);
        const bool rot = acc && det == 1;
        w_n += __popcll(__ballot(acc));
        w_2 += __popcll(__ballot(rot && tr == -1));
        w_3 += __popcll(__ballot(rot && tr == 0));
        w_4 += __popcll(__ballot(rot && tr == 1));
        w_6 += __popcll(__ballot(rot && tr == 2));
      }
      if ((tid & 63) == 0) {  // integer adds: the order of the waves does not matter
        atomicAdd(&s_cnt[0], w_n);
        atomicAdd(&s_cnt[1], w_2);
        atomicAdd(&s_cnt[2], w_3);
        atomicAdd(&s_cnt[3], w_4);
        atomicAdd(&s_cnt[4], w_6);
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < 5; ++q) cnt[q] = s_cnt[q];
      halvings = h;
      code = system_of(cnt[0], cnt[1], cnt[2], cnt[3], cnt[4]);
      __syncthreads();  // (every thread has read s_cnt before the next level clears it)
      if (code >= 0) break;  // (uniform: the counts came from LDS behind a barrier)
    }
  }
  if (tid != 0) return;
  int flags = s_head[0];
  if (!skip && code < 0) flags |= CHM_CELL_AMBIGUOUS;
  if (p.require && p.require[(long)g * p.require_stride] != code) flags |= CHM_CELL_MISMATCH;
  float x12[3] = {L[4] * L[8] - L[5] * L[7], L[5] * L[6] - L[3] * L[8], L[3] * L[7] - L[4] * L[6]};
  const float vol = fabsf(dot3(L, x12));
  float4* of = reinterpret_cast<float4*>(p.out + g);
  int4* oi = reinterpret_cast<int4*>(p.out + g);
  of[0] = make_float4(l0, l1, l2, al);
  of[1] = make_float4(be, ga, vol, 0.f);
  oi[2] = make_int4(s_T[0], s_T[1], s_T[2], s_T[3]);
  oi[3] = make_int4(s_T[4], s_T[5], s_T[6], s_T[7]);
  oi[4] = make_int4(s_T[8], cnt[0], cnt[1], cnt[2]);
  oi[5] = make_int4(cnt[3], cnt[4], code, halvings);
  oi[6] = make_int4(flags, s_head[1], 0, 0);
  oi[7] = make_int4(0, 0, 0, 0);
}

// Block g = crystal g: the reduced lattice T L (fp64, rounded once: the bits k_cell searched) and, per atom,
// x' = frac(x adj(T)) in fp64, rounded once. adj(T) = T^-1 exactly, because det T = +1.
__global__ __launch_bounds__(kBlock) void k_cell_apply(ApplyArgs p) {
  const int g = blockIdx.x, tid = threadIdx.x;
  const int n0 = p.off[g], n = p.off[g + 1] - n0;
  int T[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) T[q] = p.rec[g].transform[q];
  if (tid < 9) p.lat_out[(long)g * 9 + tid] = reduced_entry(T, p.lat + (long)g * 9, tid);
  double adj[9];
  adjugate(T, adj);
  for (int i = tid; i < n; i += kBlock) {
    const long at = 3 * ((long)n0 + i);
    float f[3];
    reduced_frac(adj, p.x + at, f);
#pragma unroll
    for (int k = 0; k < 3; ++k) p.x_out[at + k] = f[k];
  }
}

}  // namespace

struct chm_cell : chm::NodePlan {};

extern "C" int chm_cell_create(const int32_t* h_natoms, int num_graphs, chm_cell** out) {
  static_assert(sizeof(chm_cell_record) == 128, "the record is 128 bytes");
  return chm::node_plan_create(h_natoms, num_graphs, {"cell plan"}, "chm_cell_create", out);
}

extern "C" void chm_cell_destroy(chm_cell* p) { chm::node_plan_destroy(p); }

namespace {
const chm::Check check{"the cell plan"};
}  // namespace

extern "C" int chm_cell_run(const chm_cell* p, const float* d_lattices, int64_t n_lattices, const int32_t* d_require,
                            int64_t n_require, float symprec, float angle_tolerance, void* d_out,
                            size_t n_out_bytes, void* stream) {
  if (!p) return fail(CHM_E_ARG, "cell plan is NULL");
  int rc, require_stride;
  if ((rc = check.count(d_lattices, n_lattices, 9L * p->B, "lattices [B,3,3]"))) return rc;
  if ((rc = check.broadcast(d_require, n_require, 1, p->B, "require", "[B]", &require_stride))) return rc;
  if ((rc = check.range(symprec, CHM_CELL_MAX_SYMPREC, "symprec", " A"))) return rc;
  if ((rc = check.range(angle_tolerance, CHM_CELL_MAX_ANGLE_TOLERANCE, "angle_tolerance", " degrees"))) return rc;
  if ((rc = check.count(d_out, (long)n_out_bytes, 128L * p->B, "out", "bytes"))) return rc;
  if ((rc = check.aligned16(d_out, "out"))) return rc;
  CellArgs a;
  a.lat = d_lattices;
  a.require = d_require;
  a.require_stride = require_stride;
  a.symprec = symprec;
  a.angle_tolerance = angle_tolerance;
  a.out = static_cast<chm_cell_record*>(d_out);
  hipLaunchKernelGGL(k_cell, dim3(p->B), dim3(kBlock), 0, (hipStream_t)stream, a);
  HIPCHK(hipGetLastError());
  return CHM_OK;
}

extern "C" int chm_cell_apply(const chm_cell* p, const void* d_records, size_t n_record_bytes, const float* d_frac,
                              int64_t n_frac, const float* d_lattices, int64_t n_lattices, float* d_frac_out,
                              int64_t n_frac_out, float* d_lattices_out, int64_t n_lattices_out, void* stream) {
  if (!p) return fail(CHM_E_ARG, "cell plan is NULL");
  int rc;
  if ((rc = check.count(d_records, (long)n_record_bytes, 128L * p->B, "records", "bytes"))) return rc;
  if ((rc = check.aligned16(d_records, "records"))) return rc;
  if ((rc = check.count(d_frac, n_frac, 3 * p->N, "frac [N,3]"))) return rc;
  if ((rc = check.count(d_lattices, n_lattices, 9L * p->B, "lattices [B,3,3]"))) return rc;
  if ((rc = check.count(d_frac_out, n_frac_out, 3 * p->N, "frac_out [N,3]"))) return rc;
  if ((rc = check.count(d_lattices_out, n_lattices_out, 9L * p->B, "lattices_out [B,3,3]"))) return rc;
  if (d_frac_out == d_frac) return fail(CHM_E_ARG, "frac_out must not be frac: the cell is never applied in place");
  if (d_lattices_out == d_lattices)
    return fail(CHM_E_ARG, "lattices_out must not be lattices: the cell is never applied in place");
  ApplyArgs a;
  a.x = d_frac;
  a.lat = d_lattices;
  a.off = p->d_off;
  a.rec = static_cast<const chm_cell_record*>(d_records);
  a.x_out = d_frac_out;
  a.lat_out = d_lattices_out;
  hipLaunchKernelGGL(k_cell_apply, dim3(p->B), dim3(kBlock), 0, (hipStream_t)stream, a);
  HIPCHK(hipGetLastError());
  return CHM_OK;
}
