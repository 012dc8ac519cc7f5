// Device code shared by cell.hip (k_cell, k_cell_apply) and symm.hip (k_symm): the test of one candidate W of the
// lattice search, and the reduced lattice Lr = T L and reduced coordinates x' = frac(x adj(T)) as chm_cell_apply
// writes them. Both files decide about the same numbers with the same expressions because they call these
// functions; the definition is in include/chemeleon_hip.h at chm_cell_* and chm_symm_*.
#ifndef CHM_CELL_SHARED_H
#define CHM_CELL_SHARED_H

#include <hip/hip_runtime.h>

#include <math.h>

// Every product and sum is rounded on its own, in fp32 and in fp64 (constrain.hip explains why the toolchain's
// __fmul_rn alone does not prevent contraction).
#pragma clang fp contract(off)

namespace chm_cellshared {

constexpr int kCandidates = 19683;  // 3^9; index = sum_q (W[q] + 1) 3^q, so -W has index kCandidates - 1 - index
constexpr int kIdentityIndex = 16484;  // digits (entries + 1) = 2 on the diagonal, 1 elsewhere: 9841 + 1 + 81 + 6561
constexpr int kMaxHalvings = 4;

__device__ inline float dot3(const float* u, const float* v) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }
// (as k_screen's: 90 where a row is zero)
__device__ inline float angle_deg(const float* u, const float* v, float lu, float lv) {
  const float d = lu * lv;
  if (!(d > 0.f)) return 90.f;
  const float cs = fminf(fmaxf(dot3(u, v) / d, -1.f), 1.f);
  return acosf(cs) * 57.29577951308232f;
}

// the row-major entries of candidate `idx`, its determinant and trace, in integers
__device__ inline void decode_candidate(int idx, int* W, int* det, int* tr) {
  int r = idx;
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    W[q] = r % 3 - 1;
    r /= 3;
  }
  *det = (W[0] * (W[4] * W[8] - W[5] * W[7]) - W[1] * (W[3] * W[8] - W[5] * W[6])) + W[2] * (W[3] * W[7] - W[4] * W[6]);
  *tr = W[0] + W[4] + W[8];
}

// The cell's own row lengths l[3] and angles a[3] = alpha (rows 1-2), beta (rows 0-2), gamma (rows 0-1).
__device__ inline void cell_metric(const float* L, float* l, float* a) {
  l[0] = sqrtf(dot3(L, L));
  l[1] = sqrtf(dot3(L + 3, L + 3));
  l[2] = sqrtf(dot3(L + 6, L + 6));
  a[0] = angle_deg(L + 3, L + 6, l[1], l[2]);
  a[1] = angle_deg(L, L + 6, l[0], l[2]);
  a[2] = angle_deg(L, L + 3, l[0], l[1]);
}

// Is candidate `idx` (< kCandidates) a unimodular W whose W L keeps every row length within tl and every
// inter-row angle within ta of the cell's own (l, a of cell_metric)? *det and *tr are W's determinant and trace.
__device__ inline bool candidate_accepted(int idx, const float* L, const float* l, const float* a, float tl, float ta,
                                          int* det, int* tr) {
  int W[9];
  decode_candidate(idx, W, det, tr);
  if (*det != 1 && *det != -1) return false;
  float M[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k)
      M[3 * i + k] = ((float)W[3 * i] * L[k] + (float)W[3 * i + 1] * L[3 + k]) + (float)W[3 * i + 2] * L[6 + k];
  const float m0 = sqrtf(dot3(M, M)), m1 = sqrtf(dot3(M + 3, M + 3)), m2 = sqrtf(dot3(M + 6, M + 6));
  bool acc = fabsf(m0 - l[0]) <= tl && fabsf(m1 - l[1]) <= tl && fabsf(m2 - l[2]) <= tl;
  if (acc)
    acc = fabsf(angle_deg(M + 3, M + 6, m1, m2) - a[0]) <= ta && fabsf(angle_deg(M, M + 6, m0, m2) - a[1]) <= ta &&
          fabsf(angle_deg(M, M + 3, m0, m1) - a[2]) <= ta;
  return acc;
}

// Entry q of the reduced lattice T L (fp64, rounded once: the bits k_cell searched). T = identity copies the
// cell as it is: a flagged cell's NaN stays where it was, 0 * NaN would spread it.
__device__ inline float reduced_entry(const int* T, const float* L, int q) {
  const int i = q / 3, k = q - 3 * i;
  bool identity = true;
#pragma unroll
  for (int r = 0; r < 9; ++r) identity &= T[r] == ((r % 4 == 0) ? 1 : 0);
  return identity ? L[q]
                  : (float)(((double)T[3 * i] * (double)L[k] + (double)T[3 * i + 1] * (double)L[3 + k]) +
                            (double)T[3 * i + 2] * (double)L[6 + k]);
}

// adj(T) = T^-1 exactly, because det T = +1 (64-bit: a product of two entries of a T that did not come from
// k_cell need not fit 32 bits)
__device__ inline void adjugate(const int* T, double* a) {
  long long t[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) t[q] = T[q];
  a[0] = (double)(t[4] * t[8] - t[5] * t[7]);
  a[1] = (double)(t[2] * t[7] - t[1] * t[8]);
  a[2] = (double)(t[1] * t[5] - t[2] * t[4]);
  a[3] = (double)(t[5] * t[6] - t[3] * t[8]);
  a[4] = (double)(t[0] * t[8] - t[2] * t[6]);
  a[5] = (double)(t[2] * t[3] - t[0] * t[5]);
  a[6] = (double)(t[3] * t[7] - t[4] * t[6]);
  a[7] = (double)(t[1] * t[6] - t[0] * t[7]);
  a[8] = (double)(t[0] * t[4] - t[1] * t[3]);
}

// x' = frac(x adj(T)) in fp64, rounded once, in [0, 1)
__device__ inline void reduced_frac(const double* a, const float* x, float* out) {
  const double x0 = (double)x[0], x1 = (double)x[1], x2 = (double)x[2];
  const double y[3] = {(x0 * a[0] + x1 * a[3]) + x2 * a[6], (x0 * a[1] + x1 * a[4]) + x2 * a[7],
                       (x0 * a[2] + x1 * a[5]) + x2 * a[8]};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float f = (float)(y[k] - floor(y[k]));
    if (f >= 1.0f) f = 0.0f;  // (a value just below an integer rounds up to 1: the same point is 0)
    out[k] = f;
  }
}

}  // namespace chm_cellshared

#endif  // CHM_CELL_SHARED_H
