// The fixed-order fp64 sums that close the evaluation kernels (MMD and its null, silhouette, GMM, the decodability probes, t-SNE,
// HSIC): how per-thread, per-wave and per-block values are added up once the pairwise arithmetic (pair_tiles.h) is done.  Three
// orders, each stated here once; the bit-for-bit promises of those kernels rest on them:
//   NeumaierSums   a thread's compensated sum of the values first, first + stride, ... in that order; the total is sum + comp
//   block_tree     the shared-memory tree over the T threads of a block: t takes t + T/2, then t + T/4, ... down to t + STOP
//   waves4         the four waves of a 256-thread block, in order: ((w0 + w1) + w2) + w3
// Device helpers only.  They hold additions and subtractions and nothing else, so there is nothing in them for the compiler to
// contract, and this header sets NO #pragma clang fp contract: gmm.hip and decode.hip use fma on purpose and must keep the
// translation unit's setting for everything they compile after the include.  A product that feeds a sum (k * k, a * b) stays at the
// call site, in a statement of its own, under the includer's setting.
#pragma once
#include <hip/hip_runtime.h>

namespace svae {

// One step of a compensated (Neumaier) sum; the total is sum + comp
__device__ __forceinline__ void neumaier_add(double& sum, double& comp, double v) {
  const double tsum = sum + v;
  comp = comp + (fabs(sum) >= fabs(v) ? (sum - tsum) + v : (v - tsum) + sum);
  sum = tsum;
}

// K compensated sums side by side
template <int K>
struct NeumaierSums {
  double sum[K] = {}, comp[K] = {};
  __device__ __forceinline__ void add(int k, double v) { neumaier_add(sum[k], comp[k], v); }
  __device__ __forceinline__ double total(int k) const { return sum[k] + comp[k]; }
};

// K interleaved sums over the T threads of a block: the caller has written red[k T + t]; on return red[k T + c] holds the sum of
// the threads congruent to c modulo STOP, for c < STOP (STOP = 1: the block's sum in red[k T]).  One barrier after the caller's
// writes, one after every level: the results are visible to every thread.
template <int T, int K, int STOP = 1>
__device__ __forceinline__ void block_tree(double* red) {
  const int t = threadIdx.x;
  __syncthreads();
  for (int o = T / 2; o >= STOP; o >>= 1) {
    if (t < o)
#pragma unroll
      for (int k = 0; k < K; ++k) red[k * T + t] = red[k * T + t] + red[k * T + t + o];
    __syncthreads();
  }
}

// The tree sum of one value per thread, returned in every thread; red [T] is free again on return
template <int T>
__device__ __forceinline__ double block_sum_all(double v, double* red) {
  red[threadIdx.x] = v;
  block_tree<T, 1>(red);
  const double r = red[0];
  __syncthreads();
  return r;
}

// The sum of v [n] by one block of T threads: thread t adds v[t], v[t + T], ... compensated, then the tree; valid in every thread
template <int T>
__device__ __forceinline__ double block_sum_of(const double* __restrict__ v, long long n, double* red) {
  NeumaierSums<1> acc;
  for (long long i = threadIdx.x; i < n; i += T) acc.add(0, v[i]);
  red[threadIdx.x] = acc.total(0);
  block_tree<T, 1>(red);
  return red[0];
}

// r[w stride] = the value of wave w
__device__ __forceinline__ double waves4(const double* r, int stride) { return ((r[0] + r[stride]) + r[2 * stride]) + r[3 * stride]; }

}  // namespace svae
