// What the host code of the finishing legs shares (screen.hip, cell.hip, symm.hip, dedup.hip, match.hip): the plan
// table of a crystal list and the argument checks of an entry point. A leg is its kernels, its record and the
// order of its checks; the three properties every leg owes its callers live here once:
//   * an entry point launches nothing after it has refused an argument (every check returns before the launch);
//   * the node offsets of a plan fit an int (node_offsets' 2^31 check) and a per-crystal cap holds before upload;
//   * a plan that failed to build leaves nothing allocated (upload frees what it made).
// Host-only: no kernel includes anything from here.
#pragma once
#include <string.h>

#include <cstdint>
#include <string>
#include <vector>

#include "chm_host.h"

namespace chm {

// How a leg words the limits of its crystal lists: "more than 2^31 - 1 atoms in one <plan>", and with a cap
// "<list>[g] = n: <holder> holds at most <cap> atoms per crystal".
struct OffsetRule {
  const char* plan;
  int cap = 0;  // atoms per crystal the kernels stage in LDS; 0 = none
  const char* holder = nullptr;
};

// offs [count + 1] = the first node of each crystal of nat [count] (`what` names the list in messages), *total = N
inline int node_offsets(const int32_t* nat, int count, const char* what, const OffsetRule& r, std::vector<int>& offs,
                        long* total) {
  offs.assign((size_t)count + 1, 0);
  long N = 0;
  for (int g = 0; g < count; ++g) {
    const std::string at = std::string(what) + "[" + std::to_string(g) + "]";
    if (nat[g] <= 0) return fail(CHM_E_ARG, at + " must be >= 1");
    if (r.cap && nat[g] > r.cap)
      return fail(CHM_E_UNSUPPORTED, at + " = " + std::to_string(nat[g]) + ": " + r.holder + " holds at most " +
                                         std::to_string(r.cap) + " atoms per crystal");
    N += nat[g];
    if (N > INT32_MAX) return fail(CHM_E_UNSUPPORTED, std::string("more than 2^31 - 1 atoms in one ") + r.plan);
    offs[(size_t)g + 1] = (int)N;
  }
  *total = N;
  return CHM_OK;
}

// A device copy of a host byte range (synchronous, like everything at plan creation); on failure nothing stays
// allocated and the message is "<entry point>: <HIP's error string>".
inline int upload(const void* host, size_t bytes, const char* entry, void** d_out) {
  void* d = nullptr;
  hipError_t e = hipMalloc(&d, bytes);
  if (e == hipSuccess) e = hipMemcpy(d, host, bytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    if (d) (void)hipFree(d);
    return fail(CHM_E_HIP, std::string(entry) + ": " + hipGetErrorString(e));
  }
  *d_out = d;
  return CHM_OK;
}

// The plan of a leg that needs the node offsets only. The C ABI keeps one opaque type per leg (chm_screen, chm_cell,
// chm_symm, chm_dedup): each is this layout under its own name.
struct NodePlan {
  int B = 0;
  long N = 0;
  int* d_off = nullptr;  // [B + 1] first node of each crystal
};

template <class Plan>
int node_plan_create(const int32_t* h_natoms, int num_graphs, const OffsetRule& rule, const char* entry, Plan** out) {
  if (!out) return fail(CHM_E_ARG, "out is NULL");
  *out = nullptr;
  if (!h_natoms) return fail(CHM_E_ARG, "natoms is NULL");
  if (num_graphs <= 0) return fail(CHM_E_ARG, "num_graphs must be >= 1");
  std::vector<int> offs;
  long N = 0;
  void* d_off = nullptr;
  int rc;
  if ((rc = node_offsets(h_natoms, num_graphs, "natoms", rule, offs, &N))) return rc;
  if ((rc = upload(offs.data(), offs.size() * sizeof(int), entry, &d_off))) return rc;
  Plan* p = new Plan;
  p->B = num_graphs;
  p->N = N;
  p->d_off = static_cast<int*>(d_off);
  *out = p;
  return CHM_OK;
}

template <class Plan>
void node_plan_destroy(Plan* p) {
  if (!p) return;
  (void)hipFree(p->d_off);
  delete p;
}

// The argument checks of one unit's entry points; `unit` is the noun its messages use ("the cell plan needs ...").
// Every member returns CHM_OK or fail()'s code, so a caller's checks read in the order they are reported.
struct Check {
  const char* unit;

  // a required buffer of exactly `expect` elements (or bytes)
  int count(const void* ptr, long n, long expect, const char* name, const char* what = "elements") const {
    if (!ptr) return fail(CHM_E_ARG, std::string(name) + " is NULL");
    if (n != expect)
      return fail(CHM_E_ARG, std::string(name) + ": " + std::to_string(n) + " " + what + ", " + unit + " needs " +
                                 std::to_string(expect));
    return CHM_OK;
  }
  // a buffer that may be absent (NULL with a count of 0); `name` may carry its shape, "exclude [B]"
  int optional(const void* ptr, long n, long expect, const char* name, const char* what = "elements") const {
    if (ptr) return count(ptr, n, expect, name, what);
    if (n == 0) return CHM_OK;
    const char* shape = strstr(name, " [");
    return fail(CHM_E_ARG, (shape ? std::string(name, shape) : std::string(name)) + " is NULL but " +
                               std::to_string(n) + " " + what);
  }
  // an optional buffer of K elements for every crystal or K per crystal (`shape` = "[B]", "[B,104]"); *stride is
  // what crystal g's row starts at, times g
  int broadcast(const void* ptr, long n, long K, long B, const char* name, const char* shape, int* stride) const {
    *stride = 0;
    if (!ptr) return optional(ptr, n, 0, name);
    if (n != K && n != K * B)
      return fail(CHM_E_ARG, std::string(name) + ": " + std::to_string(n) + " elements, " + unit + " needs " +
                                 std::to_string(K) + " (one for all) or " + std::to_string(K * B) + " (" + shape + ")");
    if (n == K * B && B > 1) *stride = (int)K;
    return CHM_OK;
  }
  // the records are read and written as 16-byte vectors
  int aligned16(const void* ptr, const char* name) const {
    if (reinterpret_cast<uintptr_t>(ptr) % 16) return fail(CHM_E_ARG, std::string(name) + " must be 16-byte aligned");
    return CHM_OK;
  }
  // a tolerance in (0, max] (NaN fails); `tail` = its unit in the message, " A", " degrees" or ""
  int range(float v, float max, const char* name, const char* tail) const {
    if (v > 0.f && v <= max) return CHM_OK;
    return fail(CHM_E_ARG, std::string(name) + " must be in (0, " + std::to_string((int)max) + "]" + tail);
  }
  // a workspace of at least `need` bytes
  int workspace(const void* ptr, size_t bytes, size_t need) const {
    if (!ptr) return fail(CHM_E_ARG, "workspace is NULL");
    if (bytes < need)
      return fail(CHM_E_ARG, "workspace: " + std::to_string(bytes) + " bytes, " + unit + " needs " + std::to_string(need));
    return CHM_OK;
  }
};

}  // namespace chm
