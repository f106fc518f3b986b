// Silhouette of a clustering of fp64 rows, nothing of size n^2 stored.  For every row i and cluster c,
//     S[i][c] = sum over the rows j of cluster c of dist(i, j)        (pair_tiles.h distances, dist = sqrt(s): scipy's cdist)
// and from it a_i = S[i][own] / (m_own - 1), b_i = min over c != own of S[i][c] / m_c, s_i = (b_i - a_i) / max(a_i, b_i): sklearn's
// silhouette_samples with the Euclidean metric.  A block owns 64 rows and walks the full row of 64 x 64 distance tiles (not the upper
// triangle: the transposed half of a tile would need a second product and n x K partials per column tile; twice the distance work
// is the cheaper trade).  Each tile is laid out in LDS as the A operand and multiplied on the fp64 matrix cores
// (v_mfma_f64_16x16x4_f64) with the tile's 64 x NC membership columns, generated in registers as lab[j] == column ? 1.0 : 0.0, as
// mmd_null.hip does with its permutation columns.  A product dist x {0, 1} is exact, so only the order of the additions matters,
// and the schedule fixes it: the MFMA's k order within a tile, the tiles of a block in column order, the blocks of a row tile
// (grid y, at most NGY, only while the grid would otherwise leave the device idle) added in order by the finish kernel.  Every
// S[i][c] is one accumulator of one wave: no cross-lane sums, no floating-point atomics.  A column's sum depends on the members
// of its cluster only: not on its id, its position in the chunk or the chunk (grid z, K > 256) it falls in.
#include "svae_internal.h"

#include <algorithm>

#include "pair_tiles.h"  // the tile walk, the A-operand tile and #pragma clang fp contract(off)
#include "fixed_sum.h"   // the closing sum of the mean

namespace svae {

constexpr int SIL_NGY = 8;        // column chunks per row tile at most
constexpr int SIL_BLOCKS = 512;   // grid y splits the column tiles only while the grid holds fewer blocks than this

// dynamic LDS, in doubles, after the prefix of pair_tiles.h; kt holds the distance tile
constexpr int S_LB = PAIR_LDS_END;               // cluster of the tile's columns [64] int32, -1 past n
constexpr int S_END = S_LB + HT / 2;
constexpr size_t SIL_LDS = (size_t)S_END * sizeof(double);  // 74,496 B: two blocks per CU
static_assert(SIL_LDS <= 160 * 1024, "LDS per workgroup");

// part[(y * rpad + row) * kpad + c]: the sum over the column tiles of chunk y of dist(row0 + row, j) [lab[j] == c]
template <int NC>
__global__ __launch_bounds__(256) void sil_sums_kernel(const double* __restrict__ Z, int ld, int d, int n, const int* __restrict__ lab,
                                                       int row0, int ch, long long rpad, int kpad, double* __restrict__ part) {
  constexpr int NT = NC / 16;  // 16 x 16 result tiles per wave: 4 fp64 accumulators per lane each
  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* kt = lds + PAIR_LDS_KT;
  int* lb = reinterpret_cast<int*>(lds + S_LB);
  const PairTileRange tr = pair_chunk_tiles(n, ch);
  const long long r0 = (long long)row0 + tr.r0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l16 = lane & 15, kg = lane >> 4;
  const int cbase = (int)blockIdx.z * NC + l16;  // this lane's column of result tile 0
  const PairRows rows = pair_rows(Z, ld, d, n, r0, lds + PAIR_LDS_QS, lds + PAIR_LDS_CS);
  double4_t acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = double4_t{0.0, 0.0, 0.0, 0.0};
  for (int ct = tr.t_lo; ct < tr.t_hi; ++ct) {
    const long long c0 = (long long)ct * HT;
    double s[HQ];
    pair_tile(rows, c0, s);  // its first barrier also ends the previous tile's reads of kt and lb
#pragma unroll
    for (int q = 0; q < HQ; ++q) pair_kt_value(kt, lane, wave, q) = c0 + wave * HQ + q < n ? sqrt(s[q]) : 0.0;
    if (threadIdx.x < HT) lb[threadIdx.x] = c0 + threadIdx.x < n ? lab[c0 + threadIdx.x] : -1;
    __syncthreads();
    // wave w: rows [16 w, 16 w + 16) of the tile x all NC columns (lane layouts: pair_tiles.h)
#pragma unroll 2
    for (int ks = 0; ks < HT / 4; ++ks) {
      const int j = 4 * ks + kg;
      const double a = pair_kt_a(kt, j, wave, l16);
      const int rel = lb[j] - cbase;  // 16 t: row j of the tile is a member of this lane's column of result tile t
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, rel == 16 * t ? 1.0 : 0.0, acc[t], 0, 0, 0);
    }
  }
  // acc[t][r] is [row (l >> 4) + 4 r][col l & 15] of result tile t
  double* out = part + ((long long)blockIdx.y * rpad + (long long)blockIdx.x * HR + 16 * wave + kg) * kpad + (int)blockIdx.z * NC + l16;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) out[(long long)(4 * r) * kpad + 16 * t] = acc[t][r];
}

// 16 lanes per row, 16 rows per block.  Lane q scans the columns q, q + 16, ... in order with a strict <, then the 16 lanes are
// combined preferring the lower column on equal values: the minimum is exact, so b and nearest do not depend on this split.
__global__ __launch_bounds__(256) void sil_finish_kernel(const double* __restrict__ part, int gy, long long rpad, int kpad, int K,
                                                         const int* __restrict__ lab, const int* __restrict__ count, int row0, int rows,
                                                         double* __restrict__ s, double* __restrict__ a, double* __restrict__ b,
                                                         int* __restrict__ nearest) {
  const int q = threadIdx.x & 15;
  const int r = (int)blockIdx.x * 16 + (threadIdx.x >> 4);
  const int rr = min(r, rows - 1);  // every lane stays in the shuffles
  const int own = lab[row0 + rr];
  const double* p = part + (long long)rr * kpad;
  const long long ystride = rpad * kpad;
  double best = INFINITY;
  int bc = 0x7fffffff;
  for (int c = q; c < K; c += 16) {
    if (c == own) continue;
    double S = 0.0;
    for (int y = 0; y < gy; ++y) S = S + p[y * ystride + c];
    const double v = S / (double)count[c];
    if (v < best) {
      best = v;
      bc = c;
    }
  }
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) {
    const double ov = __shfl_xor(best, o, 64);
    const int oc = __shfl_xor(bc, o, 64);
    if (ov < best || (ov == best && oc < bc)) {
      best = ov;
      bc = oc;
    }
  }
  if (q != 0 || r >= rows) return;
  double So = 0.0;
  for (int y = 0; y < gy; ++y) So = So + p[y * ystride + own];
  const int m = count[own];
  double av = 0.0, sv = 0.0;
  if (m > 1) {  // a row alone in its cluster: a = 0, s = 0
    av = So / (double)(m - 1);
    const double mx = fmax(av, best);
    sv = mx == 0.0 ? 0.0 : (best - av) / mx;
  }
  s[r] = sv;
  a[r] = av;
  b[r] = best;
  nearest[r] = bc;
}

// out[0] = mean of v [n], summed by one block in the order of block_sum_of (fixed_sum.h)
__global__ __launch_bounds__(256) void sil_mean_kernel(const double* __restrict__ v, long long n, double* __restrict__ out) {
  __shared__ double red[256];
  const double sum = block_sum_of<256>(v, n, red);
  if (threadIdx.x == 0) out[0] = sum / (double)n;
}

// a >= +0 and finite: its bits order as unsigned integers.  key[c] = the smallest a of cluster c, then row[c] = the lowest row
// that holds it: integer minima, the same whatever the order of arrival.
__global__ __launch_bounds__(256) void sil_medoid_key_kernel(const double* __restrict__ a, const int* __restrict__ lab, int n,
                                                             u64* __restrict__ key) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) atomicMin(&key[lab[i]], (u64)__double_as_longlong(a[i]));
}

__global__ __launch_bounds__(256) void sil_medoid_row_kernel(const double* __restrict__ a, const int* __restrict__ lab, int n,
                                                             const u64* __restrict__ key, u64* __restrict__ row) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n && (u64)__double_as_longlong(a[i]) == key[lab[i]]) atomicMin(&row[lab[i]], (u64)i);
}

}  // namespace svae

using namespace svae;

struct SilPlan {
  int nc, ch;
  unsigned gx, gy, gz;
  long long rpad;
  int kpad;
};

// rows x n pairs, K clusters: the cluster columns per block, the grid and the layout of the partials
static SilPlan sil_plan(int rows, int n, int K) {
  SilPlan p;
  p.nc = K <= 16 ? 16 : K <= 64 ? 64 : 256;
  p.gz = (unsigned)((K + p.nc - 1) / p.nc);
  p.gx = (unsigned)pair_tile_count(rows);
  const ChunkSplit s = chunk_split(pair_tile_count(n), (long long)p.gx * p.gz, SIL_NGY, SIL_BLOCKS);
  p.ch = s.per;
  p.gy = (unsigned)s.parts;
  p.rpad = (long long)p.gx * HR;
  p.kpad = (int)p.gz * p.nc;
  return p;
}

static bool sil_sizes_ok(int rows, int n, int K) {
  return n >= 3 && n < (1 << 26) && K >= 2 && K <= SVAE_SIL_MAX_CLUSTERS && rows >= 1 && rows <= n;
}

extern "C" long long svae_silhouette_work(int rows, int n, int K) {
  if (!sil_sizes_ok(rows, n, K)) return 0;
  const SilPlan p = sil_plan(rows, n, K);
  return (long long)p.gy * p.rpad * p.kpad;
}

template <int NC>
static int sil_launch_sums(const SilPlan& p, const double* Z, int ld, int d, int n, const int* lab, int row0, double* work, hipStream_t st) {
  static DeviceOnce once;
  if (int e = allow_lds(sil_sums_kernel<NC>, once, (int)SIL_LDS, "silhouette")) return e;
  hipLaunchKernelGGL(sil_sums_kernel<NC>, dim3(p.gx, p.gy, p.gz), dim3(256), SIL_LDS, st, Z, ld, d, n, lab, row0, p.ch, p.rpad, p.kpad, work);
  return check_launch("silhouette_sums");
}

extern "C" int svae_silhouette(const double* Z, int ld, int d, int n, const int* lab, const int* count, int K, int row0, int rows,
                               double* work, double* s, double* a, double* b, int* nearest, void* stream) {
  if (int e = check_pair_rows("silhouette", Z, ld, d, n, 3, (1 << 26) - 1)) return e;
  SVAE_REQUIRE(K >= 2 && K <= SVAE_SIL_MAX_CLUSTERS && K <= n - 1, SVAE_ERR_ARG, "silhouette: bad cluster count (K=%d n=%d)", K, n);
  SVAE_REQUIRE(row0 >= 0 && rows >= 1 && rows <= n - row0, SVAE_ERR_ARG, "silhouette: bad row range (row0=%d rows=%d n=%d)", row0, rows, n);
  SVAE_REQUIRE(lab && count && work && s && a && b && nearest, SVAE_ERR_ARG, "silhouette: null argument");
  const SilPlan p = sil_plan(rows, n, K);
  int e;
  if (p.nc == 16)
    e = sil_launch_sums<16>(p, Z, ld, d, n, lab, row0, work, ST(stream));
  else if (p.nc == 64)
    e = sil_launch_sums<64>(p, Z, ld, d, n, lab, row0, work, ST(stream));
  else
    e = sil_launch_sums<256>(p, Z, ld, d, n, lab, row0, work, ST(stream));
  if (e) return e;
  hipLaunchKernelGGL(sil_finish_kernel, dim3((unsigned)((rows + 15) / 16)), dim3(256), 0, ST(stream), work, (int)p.gy, p.rpad, p.kpad, K, lab,
                     count, row0, rows, s, a, b, nearest);
  return check_launch("silhouette_finish");
}

extern "C" int svae_silhouette_mean(const double* v, long long n, double* out, void* stream) {
  SVAE_REQUIRE(v && out && n >= 1, SVAE_ERR_ARG, "silhouette_mean: bad args (n=%lld)", n);
  hipLaunchKernelGGL(sil_mean_kernel, dim3(1), dim3(256), 0, ST(stream), v, n, out);
  return check_launch("silhouette_mean");
}

extern "C" int svae_silhouette_medoids(const double* a, const int* lab, int n, int K, unsigned long long* key, long long* row, void* stream) {
  SVAE_REQUIRE(a && lab && key && row && n >= 1 && K >= 1 && K <= SVAE_SIL_MAX_CLUSTERS, SVAE_ERR_ARG, "silhouette_medoids: bad args (n=%d K=%d)",
               n, K);
  hipError_t e = hipMemsetAsync(key, 0xff, (size_t)K * sizeof(u64), ST(stream));
  if (e == hipSuccess) e = hipMemsetAsync(row, 0xff, (size_t)K * sizeof(u64), ST(stream));
  SVAE_REQUIRE(e == hipSuccess, SVAE_ERR_LAUNCH, "silhouette_medoids: hipMemsetAsync: %s", hipGetErrorString(e));
  const dim3 g((unsigned)(((long long)n + 255) / 256));
  hipLaunchKernelGGL(sil_medoid_key_kernel, g, dim3(256), 0, ST(stream), a, lab, n, key);
  if (int err = check_launch("silhouette_medoid_key")) return err;
  hipLaunchKernelGGL(sil_medoid_row_kernel, g, dim3(256), 0, ST(stream), a, lab, n, key, reinterpret_cast<u64*>(row));
  return check_launch("silhouette_medoid_row");
}
