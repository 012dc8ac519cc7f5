// Constrained sampling (chm_constrain_state / chm_sample_step_con, include/chemeleon_hip.h): after a reverse
// step has reached level s = t - 1, the entries the caller marked as known are replaced by their clean values
// forward-noised to level s, the training forward's q_sample (k_train_noise / k_train_lattice, kernels.hip):
//   types        a = a0 at s = 0, else argmax_d(log(q_mats[s-1][a0][d] + 1e-6) - log(-log(clamp(u, 1e-6, 1))))
//   lattices     l = (fwd[s][0] l0 + fwd[s][1] (z mask9)) mask9
//   coordinates  x = rem1(x0 + fwd[s][2] z)
// every product / sum explicitly rounded, in this order (the same expression op by op in torch fp32).
// One self-contained kernel beside the step kernels: none of them changes, and a step without a constraint
// enqueues exactly what it did before.
#include "chm_internal.h"

#include <math.h>

// The replacement must equal its reference bit for bit: every product and sum below is rounded on its own. The
// toolchain's __fmul_rn / __fadd_rn are plain * and + compiled in its headers with contraction allowed, so the
// compiler fuses a product and a sum made of them into one FMA (one rounding where torch's separate ops round
// twice). mul_rn / add_rn are the same operators compiled here with contraction off, which it honours per
// instruction. (The library's logf / cospif / sqrtf are unaffected, and the Philox helpers hold no a * b + c
// pattern: they stay identical to kernels.hip's.)
#pragma clang fp contract(off)

namespace chm {
namespace {

__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }

// The helpers below restate kernels.hip's (rem1, better, the Philox4x32-10 streams) line for line, so that
// kernels.hip itself stays as it is; chm_debug_philox (k_philox_fill there) must return what this kernel draws.
__device__ __forceinline__ float rem1(float x) {
  float m = fmodf(x, 1.0f);
  if (m != 0.0f && m < 0.0f) m = add_rn(m, 1.0f);
  return m;
}
__device__ __forceinline__ bool better(float v, int i, float bv, int bi) {
  const bool vn = v != v, bn = bv != bv;
  if (vn || bn) return vn && (!bn || i < bi);
  return v > bv || (v == bv && i < bi);
}
struct U4 { uint32_t x, y, z, w; };
__device__ __forceinline__ U4 philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    uint32_t h0 = (uint32_t)(p0 >> 32), l0 = (uint32_t)p0;
    uint32_t h1 = (uint32_t)(p1 >> 32), l1 = (uint32_t)p1;
    uint32_t n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
    c0 = n0; c1 = l1; c2 = n2; c3 = l0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return U4{c0, c1, c2, c3};
}
// kind: 4 constraint atom-type uniforms, 5 constraint lattice normals, 6 constraint coordinate normals
__device__ __forceinline__ float rng_uniform(uint64_t seed, int t, int kind, uint64_t idx) {
  U4 r = philox((uint32_t)idx, (uint32_t)(idx >> 32), (uint32_t)t, (uint32_t)kind, (uint32_t)seed,
                (uint32_t)(seed >> 32));
  return (float)(r.x >> 8) * (1.0f / 16777216.0f);  // [0, 1)
}
__device__ __forceinline__ float rng_normal(uint64_t seed, int t, int kind, uint64_t idx) {
  U4 r = philox((uint32_t)idx, (uint32_t)(idx >> 32), (uint32_t)t, (uint32_t)kind | 0x100u, (uint32_t)seed,
                (uint32_t)(seed >> 32));
  float u1 = ((float)(r.x >> 8) + 1.0f) * (1.0f / 16777216.0f);  // (0, 1]
  float u2 = (float)(r.y >> 8) * (1.0f / 16777216.0f);
  return sqrtf(-2.0f * logf(u1)) * cospif(2.0f * u2);
}

// the reference's lattice mask [[1,0,1],[1,1,1],[0,0,1]] (chemeleon.py:70-72), as kernels.hip's c_lat_mask
__device__ __forceinline__ float lat_mask(int q) { return (q == 1 || q == 6 || q == 7) ? 0.f : 1.f; }

// Blocks [0, node_blocks): four waves, one wave per node. Blocks behind them: one thread per lattice entry.
__global__ __launch_bounds__(256) void k_constrain(ConstrainArgs g) {
  int s = g.level;
  if (g.d_t) s = *g.d_t - 1;
  s = min(max(s, 0), g.T);  // (the host checked level; a device t outside [1, T + 1] must not leave the tables)
  const int t = s + 1;      // the Philox key's t: the step t -> t - 1 that arrived at level s
  if ((long)blockIdx.x >= g.node_blocks) {
    const long r = ((long)blockIdx.x - g.node_blocks) * 256 + threadIdx.x;
    if (r >= (long)g.B * 9) return;
    const long gph = r / 9;
    if (!g.lattice_mask[gph]) return;
    const int q = (int)(r - gph * 9);
    const float* cf = g.fwd + (long)s * 4;  // {sqrt(abar), sqrt(1 - abar), sigma_x, sigma_norm}
    const float z = g.rl ? g.rl[r] : rng_normal(g.seed, t, 5, (uint64_t)(gph + g.graph_base) * 9 + q);
    const float m = lat_mask(q);
    const float zm = mul_rn(z, m);
    const float v = add_rn(mul_rn(cf[0], g.l0[r]), mul_rn(cf[1], zm));
    g.l[r] = mul_rn(v, m);
    return;
  }
  const int lane = threadIdx.x & 63;
  const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= g.N) return;
  const bool do_type = g.type_mask && g.type_mask[i];
  const bool do_frac = g.frac_mask && g.frac_mask[i];
  if (!do_type && !do_frac) return;
  if (do_type) {  // (wave-uniform)
    const int A = g.A;
    const int64_t a0 = g.a0[i];
    if (s == 0) {
      if (lane == 0) g.a[i] = a0;
    } else {
      const float eps = 1.0e-6f;
      const int x0 = (int)min(max(a0, (int64_t)0), (int64_t)(A - 1));  // (clamped for the table read only)
      const float* Q = g.q_mats + ((long)(s - 1) * A + x0) * A;
      float bv = -INFINITY;
      int bi = 1 << 30;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int d = lane + 64 * h;
        if (d < A) {
          const float lg = logf(add_rn(Q[d], eps));
          float u = g.ra ? g.ra[i * A + d] : rng_uniform(g.seed, t, 4, (uint64_t)(i + g.node_base) * 128 + d);
          u = fminf(fmaxf(u, eps), 1.0f);
          const float v = add_rn(lg, -logf(-logf(u)));
          if (better(v, d, bv, bi)) { bv = v; bi = d; }
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
      }
      if (lane == 0) g.a[i] = bi;
    }
  }
  if (do_frac && lane < 3) {
    const float* cf = g.fwd + (long)s * 4;
    const long k = i * 3 + lane;
    const float z = g.rx ? g.rx[k] : rng_normal(g.seed, t, 6, (uint64_t)(i + g.node_base) * 3 + lane);
    g.x[k] = rem1(add_rn(g.x0[k], mul_rn(cf[2], z)));
  }
}

}  // namespace

// `what` bits: 1 types, 2 lattices, 4 coordinates. A field without its known-value / mask pair is skipped, and
// a call with nothing to do launches nothing (stage 2 of a step whose constraint holds no coordinates).
hipError_t constrain(const ConstrainArgs& in, int what, hipStream_t s) {
  ConstrainArgs g = in;
  if (g.A < 1 || g.A > 128) return hipErrorInvalidValue;
  if (!(what & 1)) g.type_mask = nullptr;
  if (!(what & 4)) g.frac_mask = nullptr;
  if (!(what & 2)) g.lattice_mask = nullptr;
  g.node_blocks = (g.type_mask || g.frac_mask) ? (g.N + 3) / 4 : 0;
  const long lat_blocks = g.lattice_mask ? ((long)g.B * 9 + 255) / 256 : 0;
  const long blocks = g.node_blocks + lat_blocks;
  if (blocks == 0) return hipSuccess;
  if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_constrain, dim3((unsigned)blocks), dim3(256), 0, s, g);
  return hipGetLastError();
}

}  // namespace chm
