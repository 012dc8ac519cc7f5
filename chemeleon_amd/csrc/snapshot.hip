// Device-side snapshot of the sampler state in output order (chm_snapshot_*, include/chemeleon_hip.h).
//
// Streaming output (Chemeleon.sample(stream=True) / return_trajectory=True) hands every step's state to
// the host as a list of structures whose atoms are sorted by chemical symbol (the reference's
// ase.build.tools.sort, schema.py:81). k_state_snapshot does the clamp and the stable sort on the device
// and packs the result into one slot, so the host copies one buffer per step and builds the structures
// by slicing. The plan (chm_snapshot) is independent of chm_model / chm_batch: node offsets and the
// symbol-rank table, uploaded once.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "chm_host.h"

namespace {

constexpr int kRanks = 104;    // classes 0..103 (X + 103 elements): the rank table's length
constexpr int kWave = 64;      // one wavefront per crystal
constexpr int kChunk = 1024;   // sort keys staged in LDS at a time (bytes)
constexpr unsigned kPadKey = 0xffu;  // above every rank: never counted

using chm::fail;

// the atomic number a structure gets for class a: the reference's clamp (classes above 103 -> 0); negative
// classes, which the sampler never produces, also -> 0
__device__ inline unsigned clamp_number(long a) { return (a >= 0 && a < kRanks) ? (unsigned)a : 0u; }

// Block g (one wavefront) = crystal g: atoms [off[g], off[g + 1]). Atom i's output position is the number
// of atoms of its crystal with a smaller key, or an equal key and a smaller index (a stable sort without
// atomics; key = the rank of the atom's chemical symbol in string order). The crystal's keys are staged in
// LDS kChunk at a time (every crystal the sampler meets fits one chunk; larger ones re-stage per 64 atoms),
// four keys per LDS read, the same address on every lane.
__global__ __launch_bounds__(kWave) void k_state_snapshot(const long* __restrict__ a, const float* __restrict__ x,
                                                          const float* __restrict__ lat,
                                                          const int* __restrict__ off,
                                                          const unsigned char* __restrict__ rank,
                                                          float* __restrict__ o_lat, float* __restrict__ o_x,
                                                          int* __restrict__ o_perm,
                                                          unsigned char* __restrict__ o_num) {
  __shared__ unsigned s_keys[kChunk / 4];
  __shared__ unsigned char s_rank[kRanks];
  const int g = blockIdx.x, lane = threadIdx.x;
  const int n0 = off[g], n = off[g + 1] - n0;
  for (int k = lane; k < kRanks; k += kWave) s_rank[k] = rank[k];
  if (lane < 9) o_lat[(long)g * 9 + lane] = lat[(long)g * 9 + lane];
  __syncthreads();
  unsigned char* s_kb = reinterpret_cast<unsigned char*>(s_keys);
  auto stage = [&](int j0) {  // keys of atoms [j0, j0 + kChunk), padded
    for (int k = lane; k < kChunk; k += kWave) {
      const int j = j0 + k;
      s_kb[k] = j < n ? s_rank[clamp_number(a[n0 + j])] : (unsigned char)kPadKey;
    }
  };
  const bool one = n <= kChunk;
  if (one) {
    stage(0);
    __syncthreads();
  }
  for (int i0 = 0; i0 < n; i0 += kWave) {  // (n is uniform over the block: every barrier below is reached by all)
    const int i = i0 + lane;
    const bool live = i < n;
    const unsigned num = live ? clamp_number(a[n0 + i]) : 0u;
    const unsigned ki = live ? s_rank[num] : 0u;
    int pos = 0;
    for (int j0 = 0; j0 < n; j0 += kChunk) {
      if (!one) {
        __syncthreads();
        stage(j0);
        __syncthreads();
      }
      const int cnt = min(n - j0, kChunk);
      for (int j = 0; j < cnt; j += 4) {
        const unsigned w = s_keys[j >> 2];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const unsigned kj = (w >> (8 * b)) & 0xffu;
          pos += (kj < ki) | ((kj == ki) & (j0 + j + b < i));
        }
      }
    }
    if (live) {
      const long src = (long)n0 + i, dst = (long)n0 + pos;
      o_x[3 * dst + 0] = x[3 * src + 0];
      o_x[3 * dst + 1] = x[3 * src + 1];
      o_x[3 * dst + 2] = x[3 * src + 2];
      o_perm[dst] = i;
      o_num[dst] = (unsigned char)num;
    }
  }
}

}  // namespace

struct chm_snapshot {
  int B = 0;
  long N = 0;
  int* d_off = nullptr;            // [B + 1] first node of each crystal
  unsigned char* d_rank = nullptr; // [104]
  size_t lat_bytes = 0, slot_bytes = 0;
};

extern "C" int chm_snapshot_create(const int32_t* h_natoms, int num_graphs, const uint8_t* h_rank, int n_rank,
                                   chm_snapshot** out) {
  if (!out) return fail(CHM_E_ARG, "out is NULL");
  *out = nullptr;
  if (!h_natoms) return fail(CHM_E_ARG, "natoms is NULL");
  if (!h_rank) return fail(CHM_E_ARG, "rank is NULL");
  if (n_rank != kRanks)
    return fail(CHM_E_ARG, "rank: " + std::to_string(n_rank) + " entries, the symbol table has " + std::to_string(kRanks));
  if (num_graphs <= 0) return fail(CHM_E_ARG, "num_graphs must be >= 1");
  for (int k = 0; k < n_rank; ++k)
    if (h_rank[k] >= kRanks) return fail(CHM_E_ARG, "rank[" + std::to_string(k) + "] outside [0, 104)");
  std::vector<int> offs((size_t)num_graphs + 1, 0);
  long N = 0;
  for (int g = 0; g < num_graphs; ++g) {
    if (h_natoms[g] <= 0) return fail(CHM_E_ARG, "natoms[" + std::to_string(g) + "] must be >= 1");
    N += h_natoms[g];
    if (N > INT32_MAX) return fail(CHM_E_UNSUPPORTED, "more than 2^31 - 1 atoms in one snapshot");
    offs[(size_t)g + 1] = (int)N;
  }
  chm_snapshot* p = new chm_snapshot;
  p->B = num_graphs;
  p->N = N;
  p->lat_bytes = (size_t)num_graphs * 9 * sizeof(float);
  p->slot_bytes = (p->lat_bytes + (size_t)N * 17 + 15) / 16 * 16;
  auto bail = [&](hipError_t e, const char* what) {
    if (p->d_off) (void)hipFree(p->d_off);
    if (p->d_rank) (void)hipFree(p->d_rank);
    delete p;
    return fail(CHM_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
  };
  hipError_t e;
  if ((e = hipMalloc((void**)&p->d_off, offs.size() * sizeof(int))) != hipSuccess) return bail(e, "hipMalloc");
  if ((e = hipMalloc((void**)&p->d_rank, kRanks)) != hipSuccess) return bail(e, "hipMalloc");
  if ((e = hipMemcpy(p->d_off, offs.data(), offs.size() * sizeof(int), hipMemcpyHostToDevice)) != hipSuccess)
    return bail(e, "hipMemcpy");
  if ((e = hipMemcpy(p->d_rank, h_rank, kRanks, hipMemcpyHostToDevice)) != hipSuccess) return bail(e, "hipMemcpy");
  *out = p;
  return CHM_OK;
}

extern "C" void chm_snapshot_destroy(chm_snapshot* p) {
  if (!p) return;
  (void)hipFree(p->d_off);
  (void)hipFree(p->d_rank);
  delete p;
}

extern "C" size_t chm_snapshot_slot_bytes(const chm_snapshot* p) { return p ? p->slot_bytes : 0; }

extern "C" int chm_snapshot_run(const chm_snapshot* p, const int64_t* d_atom_types, int64_t n_atom_types,
                                const float* d_frac, int64_t n_frac, const float* d_lattices, int64_t n_lattices,
                                void* d_slot, size_t slot_bytes, void* stream) {
  if (!p) return fail(CHM_E_ARG, "snapshot plan is NULL");
  auto want = [&](const void* ptr, long n, long expect, const char* name, const char* unit) -> int {
    if (!ptr) return fail(CHM_E_ARG, std::string(name) + " is NULL");
    if (n != expect)
      return fail(CHM_E_ARG, std::string(name) + ": " + std::to_string(n) + " " + unit + ", the snapshot needs " +
                                 std::to_string(expect));
    return CHM_OK;
  };
  int rc;
  if ((rc = want(d_atom_types, n_atom_types, p->N, "atom_types [N]", "elements"))) return rc;
  if ((rc = want(d_frac, n_frac, 3 * p->N, "frac [N,3]", "elements"))) return rc;
  if ((rc = want(d_lattices, n_lattices, 9L * p->B, "lattices [B,3,3]", "elements"))) return rc;
  if ((rc = want(d_slot, (long)slot_bytes, (long)p->slot_bytes, "slot", "bytes"))) return rc;
  if (reinterpret_cast<uintptr_t>(d_slot) % 16) return fail(CHM_E_ARG, "slot must be 16-byte aligned");
  unsigned char* s = static_cast<unsigned char*>(d_slot);
  float* o_lat = reinterpret_cast<float*>(s);
  float* o_x = reinterpret_cast<float*>(s + p->lat_bytes);
  int* o_perm = reinterpret_cast<int*>(s + p->lat_bytes + (size_t)p->N * 12);
  unsigned char* o_num = s + p->lat_bytes + (size_t)p->N * 16;
  hipLaunchKernelGGL(k_state_snapshot, dim3(p->B), dim3(kWave), 0, (hipStream_t)stream,
                     reinterpret_cast<const long*>(d_atom_types), d_frac, d_lattices, p->d_off, p->d_rank, o_lat, o_x,
                     o_perm, o_num);
  HIPCHK(hipGetLastError());
  return CHM_OK;
}
