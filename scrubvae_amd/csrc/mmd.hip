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
// reduced in a fixed order; the histogram counts are integer atomics.  Nothing depends on scheduling.
#include "svae_internal.h"

#include <algorithm>

#include "pair_tiles.h"  // the staging helpers and #pragma clang fp contract(off)

namespace svae {

typedef unsigned long long u64;

constexpr int MBITS = 13;            // digit width: 5 passes cover bits 62 .. 0 (shifts 50, 37, 24, 11, then the low 11 bits)
constexpr int MBINS = 1 << MBITS;
constexpr int MPASSES = 5;
constexpr int MCH_MAX = 16;          // column tiles per block at most
// work words after the MBINS histogram bins
enum { W_PREF = MBINS, W_MASK, W_KREM, W_LE, W_MINGT, W_EVEN, W_END };
static_assert(W_END <= SVAE_MMD_WORK_WORDS, "svae_mmd_select work buffer");

__host__ __device__ inline int mmd_shift(int pass) { return pass < MPASSES - 1 ? 63 - MBITS * (pass + 1) : 0; }
__host__ __device__ inline u64 mmd_digit_mask(int pass) { return pass < MPASSES - 1 ? (u64)(MBINS - 1) : (1ull << (63 - MBITS * (MPASSES - 1))) - 1ull; }

// Block (x, y): row tile x against the column tiles [y ch, (y + 1) ch) that lie on or above the diagonal.
struct Tiles {
  long long r0;
  int t_lo, t_hi;  // column tiles [t_lo, t_hi); empty when t_lo >= t_hi
};
__device__ __forceinline__ Tiles mmd_tiles(int n, int ch) {
  const int nt = (n + HT - 1) / HT;
  Tiles t;
  t.r0 = (long long)blockIdx.x * HR;
  t.t_lo = max((int)blockIdx.y * ch, (int)blockIdx.x);
  t.t_hi = min(((int)blockIdx.y + 1) * ch, nt);
  return t;
}

// squared distances of the block's rows to the 16 candidates of this wave in column tile ct
__device__ __forceinline__ void mmd_tile(const double* __restrict__ Z, int ld, int d, int n, long long r0, long long c0, bool resident,
                                         double* qs, double* cs, int lane, int wave, double (&s)[HQ]) {
  const int nch = (d + HD - 1) / HD;
#pragma unroll
  for (int q = 0; q < HQ; ++q) s[q] = 0.0;
  for (int ch = 0; ch < nch; ++ch) hdb_accumulate(hdb_stage(Z, ld, d, n, r0, c0, ch, resident, qs, cs), cs, lane, wave, s);
}

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
  const Tiles t = mmd_tiles(n, ch);
  if (t.t_lo >= t.t_hi) return;  // block-uniform
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const u64 pref = work[W_PREF], mask = work[W_MASK];
  const int shift = mmd_shift(pass);
  const u64 dmask = mmd_digit_mask(pass);
  for (int e = threadIdx.x; e < MBINS; e += 256) hist[e] = 0u;
  const bool resident = hdb_rows_resident(Z, ld, d, n, t.r0, qs);
  const long long i = t.r0 + lane;
  int run_digit = -1;
  unsigned run = 0u;
  for (int ct = t.t_lo; ct < t.t_hi; ++ct) {
    const long long c0 = (long long)ct * HT;
    double s[HQ];
    mmd_tile(Z, ld, d, n, t.r0, c0, resident, qs, cs, lane, wave, s);  // its first barrier also orders the zeroing of hist
#pragma unroll
    for (int q = 0; q < HQ; ++q) {
      const long long c = c0 + wave * HQ + q;
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
  const Tiles t = mmd_tiles(n, ch);
  if (t.t_lo >= t.t_hi) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const u64 s_lo = work[W_PREF];
  const bool resident = hdb_rows_resident(Z, ld, d, n, t.r0, qs);
  const long long i = t.r0 + lane;
  u64 le = 0ull, gt = ~0ull;
  for (int ct = t.t_lo; ct < t.t_hi; ++ct) {
    const long long c0 = (long long)ct * HT;
    double s[HQ];
    mmd_tile(Z, ld, d, n, t.r0, c0, resident, qs, cs, lane, wave, s);
#pragma unroll
    for (int q = 0; q < HQ; ++q) {
      const long long c = c0 + wave * HQ + q;
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
  const Tiles t = mmd_tiles(n, ch);
  const long long block = (long long)blockIdx.y * gridDim.x + blockIdx.x;
  if (t.t_lo >= t.t_hi) {
    if (threadIdx.x < 3) part[3 * block + threadIdx.x] = 0.0;
    return;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double h = hp[0];
  const bool resident = hdb_rows_resident(Z, ld, d, n, t.r0, qs);
  const long long i = t.r0 + lane;
  double a[3] = {0.0, 0.0, 0.0};
  for (int ct = t.t_lo; ct < t.t_hi; ++ct) {
    const long long c0 = (long long)ct * HT;
    double s[HQ];
    mmd_tile(Z, ld, d, n, t.r0, c0, resident, qs, cs, lane, wave, s);
#pragma unroll
    for (int q = 0; q < HQ; ++q) {
      const long long c = c0 + wave * HQ + q;
      if (i < c && c < n) {
        const double dist = sqrt(s[q]);
        const double dd = dist * dist;
        const double v = exp(-dd / h);
        if (c < nx) a[0] = a[0] + v;
        else if (i >= nx) a[1] = a[1] + v;
        else a[2] = a[2] + v;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) red[k * 256 + threadIdx.x] = a[k];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o)
#pragma unroll
      for (int k = 0; k < 3; ++k) red[k * 256 + threadIdx.x] = red[k * 256 + threadIdx.x] + red[k * 256 + threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x < 3) part[3 * block + threadIdx.x] = red[threadIdx.x * 256];
}

// One block: thread t adds the partials of blocks t, t + 1024, ... with a compensated (Neumaier) sum, then a fixed tree.
// out = {kxx, kyy, kxy, kxx + kyy - 2 kxy}
__global__ __launch_bounds__(1024) void mmd_reduce_kernel(const double* __restrict__ part, long long blocks, int nx, int ny,
                                                          double* __restrict__ out) {
  __shared__ double red[3 * 1024];
  double sum[3] = {0.0, 0.0, 0.0}, comp[3] = {0.0, 0.0, 0.0};
  for (long long b = threadIdx.x; b < blocks; b += 1024) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double v = part[3 * b + k];
      const double tsum = sum[k] + v;
      comp[k] = comp[k] + (fabs(sum[k]) >= fabs(v) ? (sum[k] - tsum) + v : (v - tsum) + sum[k]);
      sum[k] = tsum;
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) red[k * 1024 + threadIdx.x] = sum[k] + comp[k];
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if (threadIdx.x < o)
#pragma unroll
      for (int k = 0; k < 3; ++k) red[k * 1024 + threadIdx.x] = red[k * 1024 + threadIdx.x] + red[k * 1024 + threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double kxx = red[0] / ((double)nx * (double)(nx - 1) / 2.0);
    const double kyy = red[1024] / ((double)ny * (double)(ny - 1) / 2.0);
    const double kxy = red[2048] / ((double)nx * (double)ny);
    out[0] = kxx;
    out[1] = kyy;
    out[2] = kxy;
    out[3] = (kxx + kyy) - 2.0 * kxy;
  }
}

}  // namespace svae

using namespace svae;

#define ST(s) ((hipStream_t)(s))

// column tiles per block: enough blocks to fill the device at small n, long tile loops (rows staged once) at large n
static int mmd_chunk(int n) {
  const long long nt = ((long long)n + HT - 1) / HT;
  return (int)std::min<long long>(MCH_MAX, std::max<long long>(1, nt * nt / 4096));
}

static dim3 mmd_grid(int n) {
  const int nt = (int)(((long long)n + HT - 1) / HT), ch = mmd_chunk(n);
  return dim3((unsigned)nt, (unsigned)((nt + ch - 1) / ch));
}

static int mmd_args(const char* what, const double* Z, int ld, int d, int n) {
  SVAE_REQUIRE(Z && n >= 2 && d >= 1 && ld >= d, SVAE_ERR_ARG, "%s: bad rows (n=%d d=%d ld=%d)", what, n, d, ld);
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
