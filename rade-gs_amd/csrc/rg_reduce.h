// rg_reduce.h -- the one fixed-order fp64 sum (mesheval, tnteval and the three loss units).  Two stages: up to kSumBlocks blocks each leave K
// partial sums, then one block adds the partials.  Both stages end in the same 256-wide halving tree in LDS, so the order of every addition
// is a function of the sizes alone -- the reason these outputs repeat bit for bit.  Only additions here: nothing -ffp-contract could fuse.
// tests/mesheval_restatement.py's fixed_order_sum restates the order in NumPy.
#pragma once
#include <hip/hip_runtime.h>

namespace rg {

constexpr int kSumBlocks = 1024;

// the grid of a first stage over n items: one item per thread until kSumBlocks blocks, a grid-stride loop beyond
inline int sum_blocks(long long n) {
  const long long want = (n + 255) / 256;
  return (int)(want < kSumBlocks ? want : kSumBlocks);
}

// v[k] summed over the block, left in v on every thread.  Needs a 1-D block of exactly 256 threads, all of them calling; sh: K * 256 doubles.
template <int K>
__device__ __forceinline__ void block_sum(double (&v)[K], double* sh) {
#pragma unroll
  for (int k = 0; k < K; k++) sh[k * 256 + threadIdx.x] = v[k];
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
#pragma unroll
      for (int k = 0; k < K; k++) sh[k * 256 + threadIdx.x] += sh[k * 256 + threadIdx.x + w];
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < K; k++) v[k] = sh[k * 256];
}

// the second stage's loads: thread t adds the partials of blocks t, t + 256, ... onto v
template <int K>
__device__ __forceinline__ void add_partials(const double* __restrict__ partial, int nblocks, double (&v)[K]) {
  for (int b = threadIdx.x; b < nblocks; b += 256) {
#pragma unroll
    for (int k = 0; k < K; k++) v[k] += partial[K * b + k];
  }
}

}  // namespace rg
