// Hilbert-Schmidt independence criterion between latents z [n][d] and a variable y (real [n][q], or integer labels [n]) with a
// permutation null (Gretton et al. 2008; the unbiased estimator of Song et al. 2012), fp64, nothing of size n^2 stored.
//
// K_ij = hsic_value(s_ij, hz) on the squared distances of pair_tiles.h, L_ij = hsic_value(t_ij, hy) on those of the rows of y, or
// hsic_delta(y_i, y_j) for labels (hsic_common.h).  The estimators need, per pairing pi of y_pi(i) with z_i,
//     A_pi = sum_{i<j} K_ij L_pi(i)pi(j)      svae_hsic_cross, the hot path
//     S_pi = sum_i k_i l_pi(i)                svae_hsic_dots (k_i = sum_j K_ij, l_i = sum_j L_ij, diagonal included)
// and the constants C = sum_ij K_ij, D = sum_ij L_ij (svae_hsic_moments, which also gives sum K_ij^2 and sum k_i^2 for the
// normalised form).  The closing formulas run on the host from these sums.
//
// svae_hsic_cross: the matrix-core scheme of mmd_null.hip does not apply, because L changes with every permutation.  A block walks
// the upper-triangle column tiles of its 64 rows, turns s[16] into K values kept in registers, and for each of the HPC permutations
// of its chunk regenerates L for the same 16 pairs from the permuted rows of y staged in LDS: the row's y_pi(i) per lane, the 16
// candidates' y_pi(j) read wave-uniformly as a broadcast.  K is recomputed once per chunk of HPC permutations.
// Fixed order: the 16 pairs of a lane within a tile, the tile's sum added to the permutation's accumulator in column order of the
// tiles, a fixed cross-lane tree, then the orders of fixed_sum.h: the four waves in order, per-block partials at fixed positions,
// compensated strided sums and the block tree.  No floating-point atomics.  out[p] depends on row p of the permutation table
// alone: every slot of a chunk runs the same instructions on its own operands.
#include "svae_internal.h"

#include <algorithm>
#include <type_traits>

#include "pair_tiles.h"   // the tile walk and #pragma clang fp contract(off)
#include "fixed_sum.h"    // the closing sums
#include "hsic_common.h"  // hsic_value, hsic_delta

namespace svae {

constexpr int HPC = SVAE_HSIC_PERMS;  // permutations per block (grid.z = chunks of them; K is recomputed per chunk)
constexpr int HYM = SVAE_HSIC_MAX_Y;  // widest real y
constexpr int HGY = 8;                // column chunks per row tile at most: bounds the partials at 8 * (n / 64) * P doubles

// dynamic LDS of the cross kernel: the rows of pair_tiles.h as far as d needs them (the chunks of resident rows, or the one
// chunk restaged per tile), its candidates, then yr[(p q + k) 64 + row] the block's rows of y under permutation p and
// yc[(p 64 + cand) q + k] the tile's candidates.  No kt tile.  Sized per launch, so that narrow z and y leave room for a second block
// on the CU: 8 192 B + 8 320 B per resident chunk of 16 features (d <= 64; one chunk beyond) + 16 384 q B, 24 832 B + 16 384 q at
// 16 < d <= 32.
__host__ __device__ inline int cross_row_doubles(int d) {
  const int nch = (d + HD - 1) / HD;
  return (nch <= HQCH ? nch : 1) * HD * HQLD;
}
static size_t cross_lds(int d, int q, bool lab) {
  return (size_t)(cross_row_doubles(d) + HT * HD) * sizeof(double) + 2 * (size_t)HPC * HR * (lab ? sizeof(int) : (size_t)q * sizeof(double));
}
static_assert(HQCH * HD * HQLD == PAIR_LDS_CS, "the widest resident rows");
static_assert((size_t)PAIR_LDS_KT * 8 + 2 * (size_t)HPC * HR * HYM * 8 <= 160 * 1024, "LDS per workgroup");
static_assert(HPC <= 64, "one thread per permutation slot writes the block's partials");

// ---- moments of one kernel matrix ------------------------------------------------------------------------------------------------
// Block (x, y): rows [64 x, 64 x + 64) against the column tiles [y ch, (y + 1) ch) of the full matrix (K is symmetric to the bit, so
// the row sums need no transposed contribution).  part[y npad + i] = the block's share of sum_j K_ij, part[(gy + y) npad + i] that
// of sum_j K_ij^2.
template <bool LAB>
__global__ __launch_bounds__(256) void hsic_moments_kernel(const double* __restrict__ X, int ld, int d, const int* __restrict__ lab, int n,
                                                           int ch, const double* __restrict__ hp, long long npad,
                                                           double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) double qs[LAB ? 1 : HQCH * HD * HQLD];
  __shared__ __attribute__((aligned(16))) double cs[LAB ? 1 : HT * HD];
  __shared__ double red[2 * 256];
  const PairTileRange tr = pair_chunk_tiles(n, ch);
  const long long r0 = tr.r0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long i = r0 + lane;
  double a1 = 0.0, a2 = 0.0;
  if constexpr (LAB) {
    const int li = i < n ? lab[i] : 0;
    for (int ct = tr.t_lo; ct < tr.t_hi; ++ct) {
      const long long c0 = (long long)ct * HT + wave * HQ;
#pragma unroll
      for (int q = 0; q < HQ; ++q) {
        const long long c = c0 + q;
        if (i < n && c < n) {
          const double v = hsic_delta(li, lab[c]);
          a1 = a1 + v;
          a2 = a2 + v * v;
        }
      }
    }
  } else {
    const double h = hp[0];
    const PairRows rows = pair_rows(X, ld, d, n, r0, qs, cs);
    for (int ct = tr.t_lo; ct < tr.t_hi; ++ct) {
      const long long c0 = (long long)ct * HT;
      double s[HQ];
      pair_tile(rows, c0, s);
#pragma unroll
      for (int q = 0; q < HQ; ++q) {
        const long long c = c0 + wave * HQ + q;
        if (i < n && c < n) {
          const double v = hsic_value(s[q], h);
          a1 = a1 + v;
          a2 = a2 + v * v;
        }
      }
    }
  }
  red[threadIdx.x] = a1;
  red[256 + threadIdx.x] = a2;
  __syncthreads();
  if (threadIdx.x < 128) {  // the four waves of a row in order
    const int k = threadIdx.x >> 6;
    part[((long long)k * gridDim.y + blockIdx.y) * npad + r0 + lane] = waves4(red + k * 256 + lane, 64);
  }
}

// thread i: rowsum[i] = the compensated sum over the gy column chunks; the row's sum of squares goes to part[gy npad + i]
__global__ __launch_bounds__(256) void hsic_rows_kernel(double* __restrict__ part, int gy, long long npad, int n,
                                                        double* __restrict__ rowsum) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  NeumaierSums<2> acc;
  for (int y = 0; y < gy; ++y) {
#pragma unroll
    for (int k = 0; k < 2; ++k) acc.add(k, part[((long long)k * gy + y) * npad + i]);
  }
  rowsum[i] = acc.total(0);
  part[(long long)gy * npad + i] = acc.total(1);  // read above by this thread alone
}

// One block: mom = {sum_i k_i, sum_i (row i's sum of squares), sum_i k_i^2}, compensated per thread, then the block tree
__global__ __launch_bounds__(1024) void hsic_totals_kernel(const double* __restrict__ rowsum, const double* __restrict__ sq, int n,
                                                           double* __restrict__ mom) {
  __shared__ double red[3 * 1024];
  NeumaierSums<3> acc;
  for (int i = threadIdx.x; i < n; i += 1024) {
    const double k = rowsum[i];
    acc.add(0, k);
    acc.add(1, sq[i]);
    acc.add(2, k * k);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) red[k * 1024 + threadIdx.x] = acc.total(k);
  block_tree<1024, 3>(red);
  if (threadIdx.x < 3) mom[threadIdx.x] = red[threadIdx.x * 1024];
}

// ---- cross sums --------------------------------------------------------------------------------------------------------------------
// the row of y that permutation slot p of this block pairs with row r of z (rows past n: any valid row, their K is 0)
__device__ __forceinline__ long long hsic_source(const int* __restrict__ perm, int p, int P, int n, long long r) {
  if (r >= n) return 0;
  return perm ? (long long)perm[(long long)min(p, P - 1) * n + r] : r;  // slots past P repeat the last row and are not written
}

// part[block ppad + p] = this block's share of A_p; T = double: Y [n][q] rows, T = int: lab [n]
template <bool LAB>
__global__ __launch_bounds__(256) void hsic_cross_kernel(const double* __restrict__ Z, int ld, int d, int n, int ch,
                                                         const double* __restrict__ hzp, const double* __restrict__ Y, int q,
                                                         const int* __restrict__ lab, const double* __restrict__ hyp,
                                                         const int* __restrict__ perm, int P, int ppad, double* __restrict__ part) {
  using T = typename std::conditional<LAB, int, double>::type;
  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* cs = lds + cross_row_doubles(d);
  T* yr = reinterpret_cast<T*>(cs + HT * HD);
  T* yc = yr + HPC * HR * q;
  __shared__ double red[4 * HPC];
  const PairTileRange tr = pair_upper_tiles(n, ch);
  const long long block = (long long)blockIdx.y * gridDim.x + blockIdx.x;
  const int p0 = (int)blockIdx.z * HPC;
  double* out = part + block * ppad + p0;
  if (tr.t_lo >= tr.t_hi) {  // block-uniform: below the diagonal
    if (threadIdx.x < HPC) out[threadIdx.x] = 0.0;
    return;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double hz = hzp[0];
  const double hy = LAB ? 0.0 : hyp[0];
  // the block's rows of y under each permutation of the chunk (visible after the first barrier of the first pair_tile)
  for (int e = threadIdx.x; e < HPC * HR; e += 256) {
    const int p = e >> 6, r = e & 63;
    const long long src = hsic_source(perm, p0 + p, P, n, tr.r0 + r);
    if constexpr (LAB) {
      yr[p * HR + r] = lab[src];
    } else {
      for (int k = 0; k < q; ++k) yr[(p * q + k) * HR + r] = Y[src * q + k];
    }
  }
  const PairRows rows = pair_rows(Z, ld, d, n, tr.r0, lds, cs);
  const long long i = tr.r0 + lane;
  double acc[HPC];
#pragma unroll
  for (int p = 0; p < HPC; ++p) acc[p] = 0.0;
  for (int ct = tr.t_lo; ct < tr.t_hi; ++ct) {
    const long long c0 = (long long)ct * HT;
    double kv[HQ];
    pair_tile(rows, c0, kv);  // its first barrier also ends the previous tile's reads of yc
#pragma unroll
    for (int c = 0; c < HQ; ++c) {
      const long long j = c0 + wave * HQ + c;
      kv[c] = i < j && j < n ? hsic_value(kv[c], hz) : 0.0;
    }
    for (int e = threadIdx.x; e < HPC * HT; e += 256) {
      const int p = e >> 6, c = e & 63;
      const long long src = hsic_source(perm, p0 + p, P, n, c0 + c);
      if constexpr (LAB) {
        yc[p * HT + c] = lab[src];
      } else {
        for (int k = 0; k < q; ++k) yc[(p * HT + c) * q + k] = Y[src * q + k];
      }
    }
    __syncthreads();
#pragma unroll 1  // one copy of the 16 exp bodies: unrolled over the slots the loop would not fit the instruction cache
    for (int p = 0; p < HPC; ++p) {
      double sum = 0.0;
      if constexpr (LAB) {
        const int a = yr[p * HR + lane];
        const int* cw = yc + p * HT + wave * HQ;
#pragma unroll
        for (int c = 0; c < HQ; ++c) sum = sum + kv[c] * hsic_delta(a, cw[c]);
      } else {
        double t[HQ];
#pragma unroll
        for (int c = 0; c < HQ; ++c) t[c] = 0.0;
        const double* cw = yc + (p * HT + wave * HQ) * q;
        for (int k = 0; k < q; ++k) {
          const double a = yr[(p * q + k) * HR + lane];
#pragma unroll
          for (int c = 0; c < HQ; ++c) {
            const double e = a - cw[c * q + k];
            const double m = e * e;
            t[c] = t[c] + m;
          }
        }
#pragma unroll
        for (int c = 0; c < HQ; ++c) {
          const double l = hsic_value(t[c], hy);
          const double m = kv[c] * l;
          sum = sum + m;
        }
      }
      // acc[p] += sum with p a loop variable: a select per slot keeps the accumulators in registers
#pragma unroll
      for (int s = 0; s < HPC; ++s) acc[s] = s == p ? acc[s] + sum : acc[s];
    }
  }
#pragma unroll
  for (int p = 0; p < HPC; ++p) {
    double v = acc[p];  // wave_sum_d's butterfly, written out: the call moves the registers of the whole kernel
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);  // a + b == b + a: the same bits in every lane
    if (lane == 0) red[wave * HPC + p] = v;
  }
  __syncthreads();
  if (threadIdx.x < HPC) out[threadIdx.x] = waves4(red + threadIdx.x, HPC);
}

// Block b: permutations [16 b, 16 b + 16).  Thread (column c = t & 15, slot s = t >> 4) adds the partials of blocks s, s + 16, ...
// with a compensated sum, then the block tree stopped at the 16 columns (fixed_sum.h).
__global__ __launch_bounds__(256) void hsic_cross_reduce_kernel(const double* __restrict__ part, long long blocks, int ppad, int P,
                                                                double* __restrict__ out) {
  __shared__ double red[256];
  const int slot = threadIdx.x >> 4;
  const int p = (int)blockIdx.x * 16 + (threadIdx.x & 15);
  NeumaierSums<1> acc;
  if (p < ppad)
    for (long long b = slot; b < blocks; b += 16) acc.add(0, part[b * ppad + p]);
  red[threadIdx.x] = acc.total(0);
  block_tree<256, 1, 16>(red);
  if (slot == 0 && p < P) out[p] = red[threadIdx.x];
}

// ---- permuted dot products ---------------------------------------------------------------------------------------------------------
// Block p: out[p] = sum_i (k_i - shift) (l_pi_p(i) - shift), shift = 0 or 1 (the unbiased estimator's k~, l~); thread t adds the rows
// t, t + 256, ... with a compensated sum, then the block tree
__global__ __launch_bounds__(256) void hsic_dots_kernel(const double* __restrict__ k, const double* __restrict__ l, int n,
                                                        const int* __restrict__ perm, double shift, double* __restrict__ out) {
  __shared__ double red[256];
  const int* row = perm ? perm + (long long)blockIdx.x * n : nullptr;
  NeumaierSums<1> acc;
  for (int i = threadIdx.x; i < n; i += 256) {
    const double a = k[i] - shift;
    const double b = l[row ? row[i] : i] - shift;
    acc.add(0, a * b);
  }
  red[threadIdx.x] = acc.total(0);
  block_tree<256, 1>(red);
  if (threadIdx.x == 0) out[blockIdx.x] = red[0];
}

}  // namespace svae

using namespace svae;

constexpr int HSIC_N_MAX = (1 << 26) - 1;

// column tiles per block: at most HGY blocks per row tile
static int hsic_chunk(int n) {
  const int nt = pair_tile_count(n), gy = std::min(nt, HGY);
  return (nt + gy - 1) / gy;
}

static dim3 hsic_grid(int n, int P) {
  const int nt = pair_tile_count(n), ch = hsic_chunk(n);
  return dim3((unsigned)nt, (unsigned)((nt + ch - 1) / ch), (unsigned)((P + HPC - 1) / HPC));
}

extern "C" long long svae_hsic_work(int n, int P) {
  if (n < 2 || n > HSIC_N_MAX || P < 1 || P > SVAE_MMD_NULL_MAX) return 0;
  const dim3 g = hsic_grid(n, P);
  const long long moments = 2ll * g.y * g.x * HR, cross = (long long)g.x * g.y * g.z * HPC;
  return std::max(moments, cross);
}

extern "C" int svae_hsic_moments(const double* X, int ld, int d, const int* lab, int n, const double* h, double* work, double* rowsum,
                                 double* mom, void* stream) {
  SVAE_REQUIRE((X != nullptr) != (lab != nullptr), SVAE_ERR_ARG, "hsic_moments: exactly one of rows and labels");
  SVAE_REQUIRE(n >= 2 && n <= HSIC_N_MAX, SVAE_ERR_ARG, "hsic_moments: bad rows (n=%d)", n);
  if (X) {
    if (int e = check_pair_rows("hsic_moments", X, ld, d, n, 2, HSIC_N_MAX)) return e;
    SVAE_REQUIRE(h, SVAE_ERR_ARG, "hsic_moments: null bandwidth");
  }
  SVAE_REQUIRE(work && rowsum && mom, SVAE_ERR_ARG, "hsic_moments: null buffer");
  const dim3 g = hsic_grid(n, 1);
  const dim3 grid(g.x, g.y);
  const long long npad = (long long)g.x * HR;
  const int ch = hsic_chunk(n);
  if (X) hipLaunchKernelGGL(hsic_moments_kernel<false>, grid, dim3(256), 0, ST(stream), X, ld, d, lab, n, ch, h, npad, work);
  else hipLaunchKernelGGL(hsic_moments_kernel<true>, grid, dim3(256), 0, ST(stream), X, ld, d, lab, n, ch, h, npad, work);
  if (int e = check_launch("hsic_moments")) return e;
  hipLaunchKernelGGL(hsic_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ST(stream), work, (int)g.y, npad, n, rowsum);
  if (int e = check_launch("hsic_rows")) return e;
  hipLaunchKernelGGL(hsic_totals_kernel, dim3(1), dim3(1024), 0, ST(stream), rowsum, work + (long long)g.y * npad, n, mom);
  return check_launch("hsic_totals");
}

extern "C" int svae_hsic_cross(const double* Z, int ld, int d, int n, const double* hz, const double* Y, int q, const int* lab,
                               const double* hy, const int* perm, int P, double* work, double* out, void* stream) {
  if (int e = check_pair_rows("hsic_cross", Z, ld, d, n, 2, HSIC_N_MAX)) return e;
  SVAE_REQUIRE((Y != nullptr) != (lab != nullptr), SVAE_ERR_ARG, "hsic_cross: exactly one of y rows and labels");
  SVAE_REQUIRE(!Y || (q >= 1 && q <= SVAE_HSIC_MAX_Y && hy), SVAE_ERR_ARG, "hsic_cross: bad y (q=%d, at most %d)", q, SVAE_HSIC_MAX_Y);
  SVAE_REQUIRE(P >= 1 && P <= SVAE_MMD_NULL_MAX && (perm || P == 1), SVAE_ERR_ARG, "hsic_cross: bad permutation count (P=%d)", P);
  SVAE_REQUIRE(hz && work && out, SVAE_ERR_ARG, "hsic_cross: null buffer");
  const dim3 g = hsic_grid(n, P);
  const int ppad = (int)g.z * HPC, ch = hsic_chunk(n);
  if (Y) {
    static DeviceOnce once;
    if (int e = allow_lds(hsic_cross_kernel<false>, once, (int)cross_lds(HQCH * HD, HYM, false), "hsic_cross")) return e;
    hipLaunchKernelGGL(hsic_cross_kernel<false>, g, dim3(256), cross_lds(d, q, false), ST(stream), Z, ld, d, n, ch, hz, Y, q, lab, hy, perm, P,
                       ppad, work);
  } else {
    hipLaunchKernelGGL(hsic_cross_kernel<true>, g, dim3(256), cross_lds(d, 1, true), ST(stream), Z, ld, d, n, ch, hz, Y, 1, lab, hy, perm, P,
                       ppad, work);
  }
  if (int e = check_launch("hsic_cross")) return e;
  hipLaunchKernelGGL(hsic_cross_reduce_kernel, dim3((unsigned)((P + 15) / 16)), dim3(256), 0, ST(stream), work, (long long)g.x * g.y, ppad,
                     P, out);
  return check_launch("hsic_cross_reduce");
}

extern "C" int svae_hsic_dots(const double* k, const double* l, int n, const int* perm, int P, int tilde, double* out, void* stream) {
  SVAE_REQUIRE(k && l && out, SVAE_ERR_ARG, "hsic_dots: null buffer");
  SVAE_REQUIRE(n >= 2 && n <= HSIC_N_MAX, SVAE_ERR_ARG, "hsic_dots: bad rows (n=%d)", n);
  SVAE_REQUIRE(P >= 1 && P <= SVAE_MMD_NULL_MAX && (perm || P == 1), SVAE_ERR_ARG, "hsic_dots: bad permutation count (P=%d)", P);
  hipLaunchKernelGGL(hsic_dots_kernel, dim3((unsigned)P), dim3(256), 0, ST(stream), k, l, n, perm, tilde ? 1.0 : 0.0, out);
  return check_launch("hsic_dots");
}
