// rg_workspace.h -- the host plumbing the workspace-carrying units share (the rasterizer's state buffers in rg_layout.h and its ordered
// backward's scratch, densify, knn, tetmesh, mesheval, tsdf, tnteval, tntcull, meshclean, appearance, and the sort's own temp): sizes, the launch
// status, the library's ONE carver, which every unit lays its buffers out with, and the one device binary search.  What
// else is shared lives next door: the fixed-order fp64 sum in rg_reduce.h, the two-word sort with its joined 64-bit key in rg_prims.h /
// radegs_sort.hip, and the Python host layer of every module in geom_host.py.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/radegs.h"

namespace rg {

constexpr unsigned long long kMaxItems = 0xFFFFFFFFull - 65536ull;   // what the u32 sort / scan address

inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }
inline unsigned blocks_of(size_t n) { return (unsigned)((n + 255) / 256); }
inline int launch_status() { return hipGetLastError() == hipSuccess ? 0 : RADEGS_ERR_HIP; }
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Hands out consecutive 256-byte aligned arrays of one buffer.  A null base hands out null pointers and only adds up: a unit's layout
// function run once with a null base is its *_bytes, run with the workspace it is the pointer view, so the two cannot disagree.
struct Carver {
  char* base;
  size_t off = 0;
  explicit Carver(void* b) : base(static_cast<char*>(b)) {}
  template <class T>
  T* take(size_t count) {
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += align256(count * sizeof(T));
    return p;
  }
};

// first position in the ascending keys [0, n) whose key is not below `key`
template <class K>
__device__ __forceinline__ uint32_t lower_bound(const K* __restrict__ keys, uint32_t n, K key) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

}  // namespace rg
