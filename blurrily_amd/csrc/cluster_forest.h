// cluster_forest.h -- what the clustering kernels' translation units share (cluster_kernels.hip,
// cluster_levels_kernels.hip, cluster_centres_kernels.hip, cluster_cores_kernels.hip, cluster_extend_kernels.hip, cluster_within_kernels.hip, cluster_tree_kernels.hip, cluster_core_tree_kernels.hip): the sweeps' workgroup shape and the lock-free union-find forest in device memory.  The
// forest's invariants and why relaxed agent-scope atomics are enough: cluster_kernels.hip's header comment.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_index.h"

namespace blurrily {

namespace {

constexpr uint32_t kCluThreads  = 512;
constexpr uint32_t kCluWaves    = kCluThreads / 64;
constexpr uint32_t kCluWords    = kWindowSize / 4;            // 64 KiB of counters: a window in bytes, half a window in 16 bits
constexpr uint32_t kCluMaxDense = 64;                         // dense slices of a (needle, window) that may be left out

__device__ __forceinline__ uint32_t pf_load(uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// parent[x]: want -> to if it still holds `want`; returns what it held
__device__ __forceinline__ uint32_t pf_cas(uint32_t* p, uint32_t want, uint32_t to) {
  __hip_atomic_compare_exchange_strong(p, &want, to, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return want;
}
__device__ __forceinline__ void pf_min(uint32_t* p, uint32_t v) {
  (void)__hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// x's root as far as this lane can tell, halving the path on the way; false: the budget ran out
__device__ inline bool pf_find(uint32_t* parent, uint32_t* x, uint64_t* budget) {
  uint32_t v = *x;
  for (;;) {
    const uint32_t p = pf_load(parent + v);
    if (p >= v) { *x = v; return true; }                      // (p == v: a root; above v nothing is ever stored)
    const uint32_t g = pf_load(parent + p);
    if (g < p) pf_min(parent + v, g);
    v = g < p ? g : p;
    if ((*budget)-- == 0) return false;
  }
}

// a and b in one tree; *a ends as their root as far as this lane can tell (the next union of a starts there).
// *hooked: this lane made the hook (false: it saw both under one root)
__device__ inline bool pf_unite(uint32_t* parent, uint32_t* a, uint32_t b, uint64_t* budget, bool* hooked) {
  *hooked = false;
  for (;;) {
    if (!pf_find(parent, a, budget) || !pf_find(parent, &b, budget)) return false;
    if (*a == b) return true;
    const uint32_t hi = max(*a, b), lo = min(*a, b);
    const uint32_t was = pf_cas(parent + hi, hi, lo);
    if (was == hi) { *a = lo; *hooked = true; return true; }
    *a = lo; b = was;                                         // hi was hooked meanwhile: on from where it hangs now
    if ((*budget)-- == 0) return false;
  }
}
__device__ inline bool pf_unite(uint32_t* parent, uint32_t* a, uint32_t b, uint64_t* budget) {
  bool hooked;
  return pf_unite(parent, a, b, budget, &hooked);
}

}  // namespace

}  // namespace blurrily
