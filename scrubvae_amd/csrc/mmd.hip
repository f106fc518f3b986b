// Maximum mean discrepancy between two sets of latents with a squared-exponential kernel (reference eval/metrics.py::mmd_estimate),
// fp64, nothing of size n^2 stored.  Z = [X; Y] stacked, n = nx + ny rows; the pairs are the upper triangle i < j of Z.
//
// Arithmetic contract (tests/mmd_checks.py restates it in numpy): s = ((z_i0 - z_j0)^2 + (z_i1 - z_j1)^2) + ... in feature order,
// every operation rounded on its own (pair_tiles.h), dist = sqrt(s) correctly rounded: scipy's pdist / cdist euclidean.
// Bandwidth h = med * med, med = the median of the M = n (n - 1) / 2 distances as np.median takes it: the value of rank M / 2
// (0-based) for odd M, the mean of ranks M / 2 - 1 and M / 2 for even M.  The order statistic is exact: a radix select over the
// uint64 bits of s (non-negative doubles order like their bits, sqrt is monotone), 13 bits per pass from bit 62 down, every pass
// recomputing the distances; the histogram is global, so a pass is one launch over all tiles plus a one-block scan that writes
// the next prefix and rank to device memory.  Kernel value of a pair: exp((-(dist * dist)) / h).  kxx, kyy, kxy = the means over
// the pairs inside X, inside Y and across; result kxx + kyy - 2 kxy.  Sums go to per-block partials at fixed positions and are
// reduced in the fixed orders of fixed_sum.h; the histogram counts are integer atomics.  Nothing depends on scheduling.
#include "svae_internal.h"

#include <algorithm>

#include "pair_tiles.h"  // the tile walk and #pragma clang fp contract(off)
#include "fixed_sum.h"   // the closing sums
#include "mmd_common.h"  // mmd_value, mmd_statistic

namespace svae {

constexpr int MBITS = 13;            // digit width: 5 passes cover bits 62 .. 0 (shifts 50, 37, 24, 11, then the low 11 bits)
constexpr int MBINS = 1 << MBITS;
constexpr int MPASSES = 5;
constexpr int MCH_MAX = 16;          // column tiles per block at most
// work words after the MBINS histogram bins
enum { W_PREF = MBINS, W_MASK, W_KREM, W_LE, W_MINGT, W_EVEN, W_END };
static_assert(W_END <= SVAE_MMD_WORK_WORDS, "svae_mmd_select work buffer");

__host__ __device__ inline int mmd_shift(int pass) { return pass < MPASSES - 1 ? 63 - MBITS * (pass + 1) : 0; }
__host__ __device__ inline u64 mmd_digit_mask(int pass) { return pass < MPASSES - 1 ? (u64)(MBINS - 1) : (1ull << (63 - MBITS * (MPASSES - 1))) - 1ull; }

__global__ __launch_bounds__(256) void mmd_init_kernel(u64* __restrict__ work, u64 krem, u64 even) {
  for (int e = threadIdx.x; e < W_END; e += 256) work[e] = 0ull;
  __syncthreads();
  if (threadIdx.x == 0) {
    work[W_KREM] = krem;
    work[W_MINGT] = ~0ull;
    work[W_EVEN] = even;
  }
}

// One radix pass: histogram of digit `pass` of the keys that match the prefix found so far.  Each lane counts runs of equal digits
// before it touches LDS (in the first pass nearly every key has the same exponent: one LDS atomic per run, not per key), the
// block's bins are then added to the global histogram.
__global__ __launch_bounds__(256) void mmd_hist_kernel(const double* __restrict__ Z, int ld, int d, int n, int ch, int pass,
                                                       u64* __restrict__ work) {
  __shared__ __attribute__((aligned(16))) double qs[HQCH * HD * HQLD];
  __shared__ __attribute__((aligned(16))) double cs[HT * HD];
  __shared__ unsigned hist[MBINS];
  const PairTileRange t = pair_upper_tiles(n, ch);
  if (t.t_lo >= t.t_hi) return;  // block-uniform
  const u64 pref = work[W_PREF], mask = work[W_MASK];
  const int shift = mmd_shift(pass);
  const u64 dmask = mmd_digit_mask(pass);
  for (int e = threadIdx.x; e < MBINS; e += 256) hist[e] = 0u;
  const PairRows rows = pair_rows(Z, ld, d, n, t.r0, qs, cs);
  const long long i = t.r0 + rows.lane;
  int run_digit = -1;
  unsigned run = 0u;
  for (int ct = t.t_lo; ct < t.t_hi; ++ct) {
    const long long c0 = (long long)ct * HT;
    double s[HQ];
    pair_tile(rows, c0, s);  // its first barrier also orders the zeroing of hist
#pragma unroll
    for (int q = 0; q < HQ; ++q) {
      const long long c = c0 + rows.wave * HQ + q;
      const u64 key = (u64)__double_as_longlong(s[q]);
      if (i < c && c < n && (key & mask) == pref) {
        const int digit = (int)((key >> shift) & dmask);
        if (digit == run_digit) {
          ++run;
        } else {
          if (run) atomicAdd(&hist[run_digit], run);
          run_digit = digit;
          run = 1u;
        }
      }
    }
  }
  if (run) atomicAdd(&hist[run_digit], run);
  __syncthreads();
  for (int e = threadIdx.x; e < MBINS; e += 256) {
    const unsigned h = hist[e];
    if (h) atomicAdd(work + e, (u64)h);
  }
}

// One block: the bin that holds rank krem (1-based among the keys that match the prefix), the prefix extended by its digit, the
// rank inside the bin, the histogram zeroed for the next pass.
__global__ __launch_bounds__(256) void mmd_scan_kernel(u64* __restrict__ work, int pass) {
  constexpr int PER = MBINS / 256;
  __shared__ u64 chunk[256];
  u64 sum = 0ull;
  for (int b = 0; b < PER; ++b) sum += work[threadIdx.x * PER + b];
  chunk[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    const u64 krem = work[W_KREM];
    u64 cum = 0ull;
    int c = 0;
    while (c < 255 && cum + chunk[c] < krem) cum += chunk[c++];
    int b = c * PER;
    while (b < c * PER + PER - 1 && cum + work[b] < krem) cum += work[b++];
    work[W_KREM] = krem - cum;
    work[W_PREF] |= (u64)b << mmd_shift(pass);
    work[W_MASK] |= mmd_digit_mask(pass) << mmd_shift(pass);
  }
  __syncthreads();
  for (int b = 0; b < PER; ++b) work[threadIdx.x * PER + b] = 0ull;
}

// Even M, after the last pass (prefix = s_lo, the key of rank M / 2 - 1): the count of keys <= s_lo and the smallest key above it
__global__ __launch_bounds__(256) void mmd_upper_kernel(const double* __restrict__ Z, int ld, int d, int n, int ch,
                                                        u64* __restrict__ work) {
  __shared__ __attribute__((aligned(16))) double qs[HQCH * HD * HQLD];
  __shared__ __attribute__((aligned(16))) double cs[HT * HD];
  __shared__ u64 r_le[256], r_gt[256];
  const PairTileRange t = pair_upper_tiles(n, ch);
  if (t.t_lo >= t.t_hi) return;
  const u64 s_lo = work[W_PREF];
  const PairRows rows = pair_rows(Z, ld, d, n, t.r0, qs, cs);
  const long long i = t.r0 + rows.lane;
  u64 le = 0ull, gt = ~0ull;
  for (int ct = t.t_lo; ct < t.t_hi; ++ct) {
    const long long c0 = (long long)ct * HT;
    double s[HQ];
    pair_tile(rows, c0, s);
#pragma unroll
    for (int q = 0; q < HQ; ++q) {
      const long long c = c0 + rows.wave * HQ + q;
      const u64 key = (u64)__double_as_longlong(s[q]);
      if (i < c && c < n) {
        if (key <= s_lo) ++le;
        else gt = min(gt, key);
      }
    }
  }
  r_le[threadIdx.x] = le;
  r_gt[threadIdx.x] = gt;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      r_le[threadIdx.x] += r_le[threadIdx.x + o];
      r_gt[threadIdx.x] = min(r_gt[threadIdx.x], r_gt[threadIdx.x + o]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    atomicAdd(work + W_LE, r_le[0]);
    atomicMin(work + W_MINGT, r_gt[0]);
  }
}

// hm[0] = med, hm[1] = h = med * med
__global__ void mmd_bandwidth_kernel(const u64* __restrict__ work, u64 k_hi, double* __restrict__ hm) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const u64 s_lo = work[W_PREF];
  double med = sqrt(__longlong_as_double((long long)s_lo));
  if (work[W_EVEN]) {  // rank k_hi (0-based) is s_lo again when more than k_hi keys are <= s_lo
    const u64 s_hi = work[W_LE] > k_hi ? s_lo : work[W_MINGT];
    const double hi = sqrt(__longlong_as_double((long long)s_hi));
    med = (med + hi) / 2.0;
  }
  hm[0] = med;
  hm[1] = med * med;
}

// Three sums of exp(-(dist^2) / h): pairs inside X (j < nx), inside Y (i >= nx), across.  part[3 block + kind].
__global__ __launch_bounds__(256) void mmd_sums_kernel(const double* __restrict__ Z, int ld, int d, int n, int nx, int ch,
                                                       const double* __restrict__ hp, double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) double qs[HQCH * HD * HQLD];
  __shared__ __attribute__((aligned(16))) double cs[HT * HD];
  __shared__ double red[3 * 256];
  const PairTileRange t = pair_upper_tiles(n, ch);
  const long long block = (long long)blockIdx.y * gridDim.x + blockIdx.x;
  if (t.t_lo >= t.t_hi) {
    if (threadIdx.x < 3) part[3 * block + threadIdx.x] = 0.0;
    return;
  }
  const double h = hp[0];
  const PairRows rows = pair_rows(Z, ld, d, n, t.r0, qs, cs);
  const long long i = t.r0 + rows.lane;
  double a[3] = {0.0, 0.0, 0.0};
  for (int ct = t.t_lo; ct < t.t_hi; ++ct) {
    const long long c0 = (long long)ct * HT;
    double s[HQ];
    pair_tile(rows, c0, s);
#pragma unroll
    for (int q = 0; q < HQ; ++q) {
      const long long c = c0 + rows.wave * HQ + q;
      if (i < c && c < n) {
        const double v = mmd_value(s[q], h);
        if (c < nx) a[0] = a[0] + v;
        else if (i >= nx) a[1] = a[1] + v;
        else a[2] = a[2] + v;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) red[k * 256 + threadIdx.x] = a[k];
  block_tree<256, 3>(red);
  if (threadIdx.x < 3) part[3 * block + threadIdx.x] = red[threadIdx.x * 256];
}

// One block: thread t adds the partials of blocks t, t + 1024, ... compensated, then the block tree (fixed_sum.h).
// out = {kxx, kyy, kxy, kxx + kyy - 2 kxy}
__global__ __launch_bounds__(1024) void mmd_reduce_kernel(const double* __restrict__ part, long long blocks, int nx, int ny,
                                                          double* __restrict__ out) {
  __shared__ double red[3 * 1024];
  NeumaierSums<3> acc;
  for (long long b = threadIdx.x; b < blocks; b += 1024) {
#pragma unroll
    for (int k = 0; k < 3; ++k) acc.add(k, part[3 * b + k]);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) red[k * 1024 + threadIdx.x] = acc.total(k);
  block_tree<1024, 3>(red);
  if (threadIdx.x == 0) mmd_statistic(red[0], red[1024], red[2048], nx, ny, out);
}

}  // namespace svae

using namespace svae;

// column tiles per block: enough blocks to fill the device at small n, long tile loops (rows staged once) at large n
static int mmd_chunk(int n) {
  const long long nt = pair_tile_count(n);
  return (int)std::min<long long>(MCH_MAX, std::max<long long>(1, nt * nt / 4096));
}

static dim3 mmd_grid(int n) {
  const int nt = pair_tile_count(n), ch = mmd_chunk(n);
  return dim3((unsigned)nt, (unsigned)((nt + ch - 1) / ch));
}

static int mmd_args(const char* what, const double* Z, int ld, int d, int n) {
  if (int e = check_pair_rows(what, Z, ld, d, n, 2)) return e;
  SVAE_REQUIRE(mmd_grid(n).y <= 65535u, SVAE_ERR_ARG, "%s: n=%d rows exceed the tile grid", what, n);
  return SVAE_OK;
}

extern "C" long long svae_mmd_blocks(int n) {
  if (n < 2) return 0;
  const dim3 g = mmd_grid(n);
  return (long long)g.x * g.y;
}

extern "C" int svae_mmd_select(const double* Z, int ld, int d, int n, unsigned long long* work, double* hm, void* stream) {
  if (int e = mmd_args("mmd_select", Z, ld, d, n)) return e;
  SVAE_REQUIRE(work && hm, SVAE_ERR_ARG, "mmd_select: null buffer");
  const u64 M = (u64)n * (u64)(n - 1) / 2ull;
  const bool even = (M & 1ull) == 0ull;
  const u64 k_hi = M / 2ull, k_lo = even ? k_hi - 1ull : k_hi;  // 0-based ranks
  const dim3 g = mmd_grid(n);
  const int ch = mmd_chunk(n);
  hipLaunchKernelGGL(mmd_init_kernel, dim3(1), dim3(256), 0, ST(stream), work, k_lo + 1ull, even ? 1ull : 0ull);
  if (int e = check_launch("mmd_init")) return e;
  for (int pass = 0; pass < MPASSES; ++pass) {
    hipLaunchKernelGGL(mmd_hist_kernel, g, dim3(256), 0, ST(stream), Z, ld, d, n, ch, pass, work);
    if (int e = check_launch("mmd_hist")) return e;
    hipLaunchKernelGGL(mmd_scan_kernel, dim3(1), dim3(256), 0, ST(stream), work, pass);
    if (int e = check_launch("mmd_scan")) return e;
  }
  if (even) {
    hipLaunchKernelGGL(mmd_upper_kernel, g, dim3(256), 0, ST(stream), Z, ld, d, n, ch, work);
    if (int e = check_launch("mmd_upper")) return e;
  }
  hipLaunchKernelGGL(mmd_bandwidth_kernel, dim3(1), dim3(64), 0, ST(stream), work, k_hi, hm);
  return check_launch("mmd_bandwidth");
}

extern "C" int svae_mmd_sums(const double* Z, int ld, int d, int n, int nx, const double* h, double* part, double* out, void* stream) {
  if (int e = mmd_args("mmd_sums", Z, ld, d, n)) return e;
  SVAE_REQUIRE(h && part && out && nx >= 2 && n - nx >= 2, SVAE_ERR_ARG, "mmd_sums: bad args (n=%d nx=%d)", n, nx);
  const dim3 g = mmd_grid(n);
  hipLaunchKernelGGL(mmd_sums_kernel, g, dim3(256), 0, ST(stream), Z, ld, d, n, nx, mmd_chunk(n), h, part);
  if (int e = check_launch("mmd_sums")) return e;
  hipLaunchKernelGGL(mmd_reduce_kernel, dim3(1), dim3(1024), 0, ST(stream), part, (long long)g.x * g.y, nx, n - nx, out);
  return check_launch("mmd_reduce");
}
