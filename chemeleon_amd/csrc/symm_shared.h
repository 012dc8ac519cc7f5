// Device code shared by symm.hip (k_symm) and prim.hip (k_prim): the staged atom and the distance test of the atom
// search. Both kernels decide whether a moved atom lands on another with this one expression, so a translation
// that k_symm counts in n_trans is one that k_prim accepts at the same tolerance; the definition is in
// include/chemeleon_hip.h at chm_symm_* ("Acceptance") and chm_prim_*.
#ifndef CHM_SYMM_SHARED_H
#define CHM_SYMM_SHARED_H

#include <hip/hip_runtime.h>

#include <math.h>

// Every product and sum is rounded on its own (as in cell_shared.h).
#pragma clang fp contract(off)

namespace chm_symmshared {

struct __align__(16) Atom {
  float x[3];  // in the reduced basis, [0, 1)
  int type;
};

// Is the point y (fractional, not wrapped) within sqrt(tol2) of the point b, nearest image per component?
// d = y - b, d -= rintf(d), c = d L with entries (d0 l0 + d1 l1) + d2 l2, (c0 c0 + c1 c1) + c2 c2 <= tol2.
__device__ inline bool lands_on(const float* y, const float* b, const float* L, float tol2) {
  float d[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    d[k] = y[k] - b[k];
    d[k] -= rintf(d[k]);
  }
  const float e0 = (d[0] * L[0] + d[1] * L[3]) + d[2] * L[6], e1 = (d[0] * L[1] + d[1] * L[4]) + d[2] * L[7],
              e2 = (d[0] * L[2] + d[1] * L[5]) + d[2] * L[8];
  return (e0 * e0 + e1 * e1) + e2 * e2 <= tol2;
}

}  // namespace chm_symmshared

#endif  // CHM_SYMM_SHARED_H
