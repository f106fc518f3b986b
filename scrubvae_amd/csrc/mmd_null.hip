// Permutation null of the MMD statistic of mmd.hip: T_p = kxx + kyy - 2 kxy of P relabellings of the pooled rows Z = [X; Y], fp64,
// nothing of size n^2 stored.  The kernel values K_ij = mmd_value(s_ij, h) (mmd_common.h, shared with mmd_sums_kernel; pair_tiles.h
// distances) do not depend on the labels, so all P statistics come from one all-pairs pass: a block computes its 64 x 64
// tile of K (zero where i >= j or past n), lays it out in LDS as the A operand and multiplies it on the fp64 matrix cores
// (v_mfma_f64_16x16x4_f64) with the tile's 64 x 256 label columns m_jp in {0, 1} (1: row j is in "X" under relabelling p),
// expanded on the fly from packed bits [n][words].  U_ip = sum_j K_ij m_jp accumulates in registers over the block's column
// tiles, next to the label-free row sums R_i = sum_j K_ij; once per block, with the row's own label,
//     m_ip = 1:  XX += U_ip,  cross += R_i - U_ip        m_ip = 0:  cross += U_ip,  YY += R_i - U_ip.
// Direct sums of non-negative terms (not the +-1 quadratic form plus row sums): one product per tile all the same, and no
// difference of totals -- the only subtraction is per (row, column), of a row's own partial sum.  That difference carries an
// error of a rounding of R_i, which a sum over few pairs cannot absorb: m marks the smaller side (the bits are read inverted when
// nx > n - nx), so the sum inside the small side is the direct one, and the two sums that take differences hold at least
// n / 2 - 1 terms per row of R_i on average.  The statistic is symmetric in the sides, so the swap changes nothing else.
// A product K_ij x {0, 1} is exact, so only the order of the additions matters, and the tile schedule fixes it: the MFMA's k
// order within a tile, tiles in column order, the four rows of a lane, a fixed cross-lane tree, then the orders of fixed_sum.h:
// the four waves in order, per-block partials at fixed positions, compensated strided sums and the tree over their 16 slots.
// No floating-point atomics.  A column's value depends on its own label bits only: not on its neighbours, its position in the
// chunk or the chunk it falls in.
#include "svae_internal.h"

#include <algorithm>

#include "pair_tiles.h"  // the tile walk, the A-operand tile and #pragma clang fp contract(off)
#include "fixed_sum.h"   // the closing sums
#include "mmd_common.h"  // mmd_value, mmd_statistic

namespace svae {

constexpr int NPC = SVAE_MMD_NULL_COLS;  // permutation columns per block (grid.z = chunks of them; K is recomputed per chunk)
constexpr int NPW = NPC / 64;            // label words per row and chunk
constexpr int NPT = NPC / 16;            // 16 x 16 result tiles per wave: 4 fp64 accumulators per lane each
constexpr int NGY = 8;                   // column chunks per row tile at most: bounds the partials at 3 * 8 * (n / 64) * P doubles

// dynamic LDS, in doubles, after the prefix of pair_tiles.h; kt holds the K tile and, after the loop, red[3][4][NPC]
constexpr int L_LB = PAIR_LDS_END;               // label words of the tile's columns [64][NPW]
constexpr int L_RB = L_LB + HT * NPW;            // label words of the block's rows [64][NPW]
constexpr int L_RS = L_RB + HR * NPW;            // row sums [64]
constexpr int L_END = L_RS + HR;
constexpr size_t NULL_LDS = (size_t)L_END * sizeof(double);  // 78,848 B: two blocks per CU
static_assert(3 * 4 * NPC <= HT * HR, "the epilogue's partials reuse the K tile");
static_assert(NULL_LDS <= 160 * 1024, "LDS per workgroup");

// part[(kind * blocks + block) * ppad + p], kind = inside the marked side, inside the other, cross; flip = ~0: the marked side is Y
__global__ __launch_bounds__(256) void mmd_null_kernel(const double* __restrict__ Z, int ld, int d, int n, int ch,
                                                       const double* __restrict__ hp, const u64* __restrict__ bits, int words,
                                                       u64 flip, int ppad, double* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* kt = lds + PAIR_LDS_KT;
  u64* lb = reinterpret_cast<u64*>(lds + L_LB);
  u64* rb = reinterpret_cast<u64*>(lds + L_RB);
  double* rs = lds + L_RS;
  const PairTileRange tr = pair_upper_tiles(n, ch);
  const long long r0 = tr.r0;
  const long long blocks = (long long)gridDim.x * gridDim.y, block = (long long)blockIdx.y * gridDim.x + blockIdx.x;
  double* out = part + block * ppad + (long long)blockIdx.z * NPC + threadIdx.x;
  const long long kind = blocks * ppad;
  if (tr.t_lo >= tr.t_hi) {  // block-uniform: below the diagonal
    out[0] = 0.0;
    out[kind] = 0.0;
    out[2 * kind] = 0.0;
    return;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l16 = lane & 15, kg = lane >> 4;
  const int wz = (int)blockIdx.z * NPW + (threadIdx.x & (NPW - 1));  // the label word this thread stages, of row threadIdx.x / NPW
  const int srow = threadIdx.x / NPW;
  const double h = hp[0];
  rb[threadIdx.x] = r0 + srow < n && wz < words ? bits[(r0 + srow) * words + wz] ^ flip : 0ull;
  const PairRows rows = pair_rows(Z, ld, d, n, r0, lds + PAIR_LDS_QS, lds + PAIR_LDS_CS);
  const long long i = r0 + lane;
  double4_t acc[NPT];
#pragma unroll
  for (int t = 0; t < NPT; ++t) acc[t] = double4_t{0.0, 0.0, 0.0, 0.0};
  double rsum = 0.0;
  for (int ct = tr.t_lo; ct < tr.t_hi; ++ct) {
    const long long c0 = (long long)ct * HT;
    double s[HQ];
    pair_tile(rows, c0, s);  // its first barrier also ends the previous tile's reads of kt and lb
#pragma unroll
    for (int q = 0; q < HQ; ++q) {
      const long long c = c0 + wave * HQ + q;
      pair_kt_value(kt, lane, wave, q) = i < c && c < n ? mmd_value(s[q], h) : 0.0;
    }
    lb[threadIdx.x] = c0 + srow < n && wz < words ? bits[(c0 + srow) * words + wz] ^ flip : 0ull;
    __syncthreads();
    // wave w: rows [16 w, 16 w + 16) of the tile x all NPC columns (lane layouts: pair_tiles.h)
#pragma unroll 2
    for (int ks = 0; ks < HT / 4; ++ks) {
      const int j = 4 * ks + kg;
      const double a = pair_kt_a(kt, j, wave, l16);
      rsum = rsum + a;
#pragma unroll
      for (int w = 0; w < NPW; ++w) {
        const u64 x = lb[j * NPW + w] >> l16;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const double m = (x >> (16 * b)) & 1ull ? 1.0 : 0.0;
          acc[4 * w + b] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, m, acc[4 * w + b], 0, 0, 0);
        }
      }
    }
  }
  // R_i: the four k groups of a row, the same bits in each of them
  rsum = rsum + __shfl_xor(rsum, 16, 64);
  rsum = rsum + __shfl_xor(rsum, 32, 64);
  __syncthreads();  // every wave is done with kt
  if (kg == 0) rs[16 * wave + l16] = rsum;
  __syncthreads();
  // acc[t][r] is [row (l >> 4) + 4 r][col l & 15] of result tile t
#pragma unroll
  for (int t = 0; t < NPT; ++t) {
    double sa = 0.0, sb = 0.0, sc = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * wave + kg + 4 * r;
      const double u = acc[t][r];
      const double v = rs[row] - u;
      if ((rb[row * NPW + (t >> 2)] >> (16 * (t & 3) + l16)) & 1ull) {
        sa = sa + u;
        sc = sc + v;
      } else {
        sc = sc + u;
        sb = sb + v;
      }
    }
    sa = sa + __shfl_xor(sa, 16, 64);
    sb = sb + __shfl_xor(sb, 16, 64);
    sc = sc + __shfl_xor(sc, 16, 64);
    sa = sa + __shfl_xor(sa, 32, 64);
    sb = sb + __shfl_xor(sb, 32, 64);
    sc = sc + __shfl_xor(sc, 32, 64);
    if (kg == 0) {
      kt[(0 * 4 + wave) * NPC + 16 * t + l16] = sa;
      kt[(1 * 4 + wave) * NPC + 16 * t + l16] = sb;
      kt[(2 * 4 + wave) * NPC + 16 * t + l16] = sc;
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 3; ++k) out[k * kind] = waves4(kt + k * 4 * NPC + threadIdx.x, NPC);
}

// Block b: columns [16 b, 16 b + 16).  Thread (column c = t & 15, slot s = t >> 4) adds the partials of blocks s, s + 16, ... with a
// compensated sum, then the block tree stopped at the 16 columns (fixed_sum.h); na rows on the marked side, nb on the other.
__global__ __launch_bounds__(256) void mmd_null_reduce_kernel(const double* __restrict__ part, long long blocks, int ppad, int P,
                                                              int na, int nb, double* __restrict__ out) {
  __shared__ double red[3 * 256];
  const int slot = threadIdx.x >> 4;
  const int p = (int)blockIdx.x * 16 + (threadIdx.x & 15);  // < ppad: ppad is a multiple of NPC
  NeumaierSums<3> acc;
  for (long long b = slot; b < blocks; b += 16) {
#pragma unroll
    for (int k = 0; k < 3; ++k) acc.add(k, part[(k * blocks + b) * ppad + p]);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) red[k * 256 + threadIdx.x] = acc.total(k);
  block_tree<256, 3, 16>(red);
  if (slot == 0 && p < P) out[p] = mmd_statistic(red[threadIdx.x], red[256 + threadIdx.x], red[512 + threadIdx.x], na, nb, nullptr);
}

}  // namespace svae

using namespace svae;

// column tiles per block: at most NGY blocks per row tile, so a block's accumulators see a long run of tiles at large n
static int null_chunk(int n) {
  const int nt = pair_tile_count(n), gy = std::min(nt, NGY);
  return (nt + gy - 1) / gy;
}

static dim3 null_grid(int n, int P) {
  const int nt = pair_tile_count(n), ch = null_chunk(n);
  return dim3((unsigned)nt, (unsigned)((nt + ch - 1) / ch), (unsigned)((P + NPC - 1) / NPC));
}

extern "C" long long svae_mmd_null_blocks(int n, int P) {
  if (n < 2 || P < 1 || P > SVAE_MMD_NULL_MAX) return 0;
  const dim3 g = null_grid(n, P);
  return 3ll * g.x * g.y * g.z * NPC;
}

extern "C" int svae_mmd_null(const double* Z, int ld, int d, int n, int nx, const double* h, const unsigned long long* bits, int words,
                             int P, double* work, double* out, void* stream) {
  if (int e = check_pair_rows("mmd_null", Z, ld, d, n, 2, (1 << 26) - 1)) return e;
  SVAE_REQUIRE(h && bits && work && out && nx >= 2 && n - nx >= 2, SVAE_ERR_ARG, "mmd_null: bad args (n=%d nx=%d)", n, nx);
  SVAE_REQUIRE(P >= 1 && P <= SVAE_MMD_NULL_MAX && words >= (P + 63) / 64, SVAE_ERR_ARG, "mmd_null: bad permutation count (P=%d words=%d)",
               P, words);
  static DeviceOnce once;
  if (int e = allow_lds(mmd_null_kernel, once, (int)NULL_LDS, "mmd_null")) return e;
  const dim3 g = null_grid(n, P);
  const int ppad = (int)g.z * NPC;
  const bool flip = nx > n - nx;  // mark the smaller side
  hipLaunchKernelGGL(mmd_null_kernel, g, dim3(256), NULL_LDS, ST(stream), Z, ld, d, n, null_chunk(n), h, bits, words, flip ? ~0ull : 0ull, ppad,
                     work);
  if (int e = check_launch("mmd_null")) return e;
  hipLaunchKernelGGL(mmd_null_reduce_kernel, dim3((unsigned)((P + 15) / 16)), dim3(256), 0, ST(stream), work, (long long)g.x * g.y, ppad, P,
                     flip ? n - nx : nx, flip ? nx : n - nx, out);
  return check_launch("mmd_null_reduce");
}
