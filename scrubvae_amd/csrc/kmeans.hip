// Lloyd's k-means on fp64 rows A [n][lda] (svae_cv_center: columns [0, d) = x - mean, column d = 1), one iteration in three steps:
//   assign   every row against the K centres through pair_rows / pair_tile with the centres as the candidate matrix (the knn_cross
//            form): s = ((a0 - c0)^2 + (a1 - c1)^2) + ... in feature order, the running minimum under the strict key (s, centre
//            index) and the second-smallest s per row.  Nothing of size n x K is written unless the caller asks for D.
//   update   sums [K][d + 1] = M^T [A | 1] with M[r][c] = (label[r] == c): a block takes a fixed chunk of rows, generates the 0/1
//            operand in registers and multiplies on the fp64 matrix cores (v_mfma_f64_16x16x4_f64), as silhouette.hip does with its
//            membership columns (the count, the product by the column of ones, as an integer histogram); the chunks are added in a
//            fixed order.  A product by 0 or 1 is exact, so every sum is a plain fp64 sum of
//            its cluster's rows in a fixed order: bit-reproducible, and it depends on the members of a cluster only, not on its id.
//   finish   C_new = sums / count (the old centre where the count is 0), shift = sum |C_new - C_old|^2 and the empty clusters: the
//            one record the host reads per iteration.  (The inertia is the sum of the assignment's block sums: svae_gmm_sum_f64.)
// No floating-point atomics; the only atomics are integer adds (rows whose label changed, empty clusters).
#include "svae_internal.h"

#include "pair_tiles.h"  // the tile walk, the matrix-core lane layout and #pragma clang fp contract(off)
#include "fixed_sum.h"   // the order of the inertia and shift sums

namespace svae {

constexpr int KM_UNIT = 256;          // rows per unit of the update's chunk rule
constexpr int KM_MAX_CHUNKS = 1024;   // row chunks of the update at most
constexpr int KM_AHEAD = 8;           // steps of 4 rows whose loads the update issues together
constexpr long long KM_PART_MAX = 1ll << 24;  // doubles of chunk partials at most (while that leaves one chunk)

// Block = 64 rows (lane = row in each of the 4 waves); wave w takes centres [16 w, 16 w + 16) of every tile of 64.
__global__ __launch_bounds__(256) void kmeans_assign_kernel(const double* __restrict__ A, int lda, int d, int n, const double* __restrict__ C,
                                                            int ldc, int K, const int* __restrict__ prev, int* __restrict__ label,
                                                            double* __restrict__ dist, double* __restrict__ gap, double* __restrict__ D,
                                                            double* __restrict__ part, int* __restrict__ changed) {
  __shared__ __attribute__((aligned(16))) double qs[HQCH * HD * HQLD];
  __shared__ __attribute__((aligned(16))) double cs[HT * HD];
  __shared__ double m1[256], m2[256];
  __shared__ int mi[256];
  const long long r0 = (long long)blockIdx.x * HR;
  const PairRows rows = pair_rows(A, lda, d, n, r0, qs, cs, C, ldc, K);
  const int lane = rows.lane, wave = rows.wave;
  const long long row = r0 + lane;
  double b1 = INFINITY, b2 = INFINITY;  // the smallest and second-smallest s so far
  int i1 = INT_MAX;                     // the centre of b1
  const int tiles = pair_tile_count(K);
  for (int ct = 0; ct < tiles; ++ct) {
    const int cb = ct * HT + wave * HQ;
    double s[HQ];
    pair_tile(rows, (long long)ct * HT, s, cb < K);
    // ascending centre index within a thread: the strict < keeps the lower index on equal s
#pragma unroll
    for (int q = 0; q < HQ; ++q) {
      const int c = cb + q;
      if (c < K) {
        const double v = s[q];
        if (D && row < n) D[row * K + c] = v;
        if (v < b1) {
          b2 = b1;
          b1 = v;
          i1 = c;
        } else if (v < b2) {
          b2 = v;
        }
      }
    }
  }
  m1[threadIdx.x] = b1;
  m2[threadIdx.x] = b2;
  mi[threadIdx.x] = i1;
  __syncthreads();
  if (wave == 0) {
    for (int w = 1; w < 4; ++w) {
      const double c1 = m1[w * 64 + lane], c2 = m2[w * 64 + lane];
      const int j = mi[w * 64 + lane];
      if (c1 < b1 || (c1 == b1 && j < i1)) {
        b2 = fmin(b1, c2);
        b1 = c1;
        i1 = j;
      } else {
        b2 = fmin(b2, c1);
      }
    }
    const bool in = row < n;
    if (in) {
      if (label) label[row] = i1;
      if (dist) dist[row] = b1;
      if (gap) gap[row] = b2 - b1;  // +inf when K = 1
    }
    if (changed) {
      const int cnt = __popcll(__ballot(in && prev[row] != i1));
      if (lane == 0 && cnt) atomicAdd(changed, cnt);
    }
    m1[lane] = in ? b1 : 0.0;  // only wave 0 reads or writes m1[0, 64) from here on
  }
  if (part) {  // kernel-uniform
    block_tree<64, 1>(m1);
    if (threadIdx.x == 0) part[blockIdx.x] = m1[0];
  }
}

// part[(chunk * K + c) * (d + 1) + f] = sum over the rows r of the chunk with label[r] == c of A[r][f], f < d, and their number in
// column d.  One wave per block: block (chunk, y, z) takes the 16 features of tile y and the clusters [16 NT z, 16 NT (z + 1)); step
// by step it multiplies M^T [16 clusters x 4 rows] with A [4 rows x 16 features] (lane layouts: pair_tiles.h), only for the
// cluster tiles that hold a cluster below K.  The count is an integer histogram of the chunk's labels in LDS (the blocks of
// feature tile 0): exact like the product by the column of ones it stands for, without a feature tile of its own when d is a
// multiple of 16.
template <int NT>
__global__ __launch_bounds__(64) void kmeans_sums_kernel(const double* __restrict__ A, int lda, int d, int n, const int* __restrict__ label,
                                                         int K, int rows_per, double* __restrict__ part) {
  __shared__ int hist[16 * NT];
  const int lane = threadIdx.x;
  const int l16 = lane & 15, kg = lane >> 4;
  const int zbase = (int)blockIdx.z * (16 * NT);
  const int nt = min(NT, (K - zbase + 15) / 16);  // block-uniform, >= 1
  const int f = (int)blockIdx.y * 16 + l16;
  const bool fin = f < d;
  const int cbase = zbase + l16;  // this lane's cluster of result tile 0 (as the A operand's row)
  const long long lo = (long long)blockIdx.x * rows_per;
  const long long hi = lo + rows_per < n ? lo + rows_per : n;
  double* out = part + (long long)blockIdx.x * K * (d + 1);
  if (blockIdx.y == 0) {  // block-uniform
    for (int i = lane; i < 16 * NT; i += 64) hist[i] = 0;
    __syncthreads();
    for (long long r = lo + lane; r < hi; r += 64) {
      const unsigned rel = (unsigned)(label[r] - zbase);
      if (rel < 16u * NT) atomicAdd(&hist[rel], 1);
    }
    __syncthreads();
    for (int i = lane; i < 16 * NT; i += 64)
      if (zbase + i < K) out[(long long)(zbase + i) * (d + 1) + d] = (double)hist[i];
  }
  double4_t acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = double4_t{0.0, 0.0, 0.0, 0.0};
  // KM_AHEAD steps of 4 rows per trip: all their loads are issued before the first product (a step past the chunk's end adds +0)
  for (long long rb = lo; rb < hi; rb += 4 * KM_AHEAD) {
    double b[KM_AHEAD];
    int rel[KM_AHEAD];  // 16 t: the row is a member of this lane's cluster of result tile t
#pragma unroll
    for (int u = 0; u < KM_AHEAD; ++u) {
      const long long r = rb + 4 * u + kg;
      const bool in = r < hi;
      b[u] = in && fin ? A[r * lda + f] : 0.0;
      rel[u] = in ? label[r] - cbase : -1;
    }
#pragma unroll
    for (int u = 0; u < KM_AHEAD; ++u)
#pragma unroll
      for (int t = 0; t < NT; ++t)
        if (t < nt) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(rel[u] == 16 * t ? 1.0 : 0.0, b[u], acc[t], 0, 0, 0);
  }
  // acc[t][r] is [cluster 16 NT z + 16 t + (l >> 4) + 4 r][feature 16 y + (l & 15)]
  if (!fin) return;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = zbase + 16 * t + kg + 4 * r;
      if (c < K) out[(long long)c * (d + 1) + f] = acc[t][r];
    }
}

// sums[e] = the sum over the chunks of part[chunk][e] in a fixed order: a block takes 16 elements; thread (g, e) adds the chunks
// g, g + 16, g + 32, ... in order, then the 16 group sums are added in the order g = 0, 1, ..., 15.
__global__ __launch_bounds__(256) void kmeans_chunk_sum_kernel(const double* __restrict__ part, int chunks, long long m, double* __restrict__ sums) {
  __shared__ double grp[256];
  const int el = threadIdx.x & 15, g = threadIdx.x >> 4;
  const long long e = (long long)blockIdx.x * 16 + el;
  double s = 0.0;
  if (e < m)
    for (int ch = g; ch < chunks; ch += 16) s = s + part[(long long)ch * m + e];
  grp[threadIdx.x] = s;
  __syncthreads();
  if (g == 0 && e < m) {
    for (int k = 1; k < 16; ++k) s = s + grp[k * 16 + el];
    sums[e] = s;
  }
}

// One block.  rec = {rows whose label changed (-1 without a counter), shift, empty clusters}; thread t takes the centre elements
// t, t + 256, ... compensated, then the block tree (fixed_sum.h).
__global__ __launch_bounds__(256) void kmeans_finish_kernel(const double* __restrict__ sums, int d, int K, const double* __restrict__ C_old,
                                                            double* __restrict__ C_new, int ldc, const int* __restrict__ changed,
                                                            double* __restrict__ rec) {
  __shared__ double red[256];
  __shared__ int empty;
  if (threadIdx.x == 0) empty = 0;
  NeumaierSums<1> acc;
  const long long m = (long long)K * d;
  for (long long e = threadIdx.x; e < m; e += 256) {
    const int k = (int)(e / d), j = (int)(e - (long long)k * d);
    const double cnt = sums[(long long)k * (d + 1) + d];
    const double old = C_old[(long long)k * ldc + j];
    const double nw = cnt > 0.0 ? sums[(long long)k * (d + 1) + j] / cnt : old;
    C_new[(long long)k * ldc + j] = nw;
    const double diff = nw - old;
    const double sq = diff * diff;
    acc.add(0, sq);
  }
  red[threadIdx.x] = acc.total(0);
  block_tree<256, 1>(red);  // its first barrier also publishes empty = 0
  int mine = 0;
  for (int k = threadIdx.x; k < K; k += 256) mine += sums[(long long)k * (d + 1) + d] > 0.0 ? 0 : 1;
  if (mine) atomicAdd(&empty, mine);
  __syncthreads();
  if (threadIdx.x == 0) {
    rec[0] = changed ? (double)changed[0] : -1.0;
    rec[1] = red[0];
    rec[2] = (double)empty;
  }
}

static int kmeans_args(const char* what, const double* A, int lda, int d, int n, int K) {
  SVAE_REQUIRE(A && n > 0 && d > 0 && d <= SVAE_CV_MAX_DIM && lda > d && K >= 1 && K <= SVAE_KMEANS_MAX_CLUSTERS, SVAE_ERR_ARG,
               "%s: bad args (n=%d d=%d lda=%d K=%d)", what, n, d, lda, K);
  return SVAE_OK;
}

struct KmPlan {
  int chunks, rows_per;
};

// the update's row chunks: units of 256 rows, as many chunks as units up to 1024, fewer while the partials would pass 2^24 doubles
static KmPlan kmeans_plan(int n, int d, int K) {
  const int units = (int)(((long long)n + KM_UNIT - 1) / KM_UNIT);
  const long long fit = std::max<long long>(1, KM_PART_MAX / ((long long)K * (d + 1)));
  const ChunkSplit s = chunk_split_into(units, (int)std::min<long long>(std::min(units, KM_MAX_CHUNKS), fit));
  return KmPlan{s.parts, s.per * KM_UNIT};
}

template <int NT>
static void kmeans_launch_sums(const KmPlan& p, const double* A, int lda, int d, int n, const int* label, int K, double* part, hipStream_t st) {
  const dim3 g((unsigned)p.chunks, (unsigned)((d + 15) / 16), (unsigned)((K + 16 * NT - 1) / (16 * NT)));
  hipLaunchKernelGGL(kmeans_sums_kernel<NT>, g, dim3(64), 0, st, A, lda, d, n, label, K, p.rows_per, part);
}

}  // namespace svae

using namespace svae;

extern "C" int svae_kmeans_assign_blocks(int n) { return n > 0 ? pair_tile_count(n) : 0; }

extern "C" int svae_kmeans_assign_f64(const double* A, int lda, int d, int n, const double* C, int ldc, int K, const int* prev, int* label,
                                      double* dist, double* gap, double* D, double* part, int* changed, void* stream) {
  if (int e = kmeans_args("kmeans_assign_f64", A, lda, d, n, K)) return e;
  SVAE_REQUIRE(C && ldc >= d, SVAE_ERR_ARG, "kmeans_assign_f64: bad centres (ldc=%d d=%d)", ldc, d);
  SVAE_REQUIRE(label || dist || gap || D || part || changed, SVAE_ERR_ARG, "kmeans_assign_f64: no output asked for");
  SVAE_REQUIRE(!changed || prev, SVAE_ERR_ARG, "kmeans_assign_f64: changed needs prev");
  SVAE_REQUIRE(!prev || prev != label, SVAE_ERR_ARG, "kmeans_assign_f64: prev and label are the same buffer");
  if (changed) {
    const hipError_t e = hipMemsetAsync(changed, 0, sizeof(int), ST(stream));
    SVAE_REQUIRE(e == hipSuccess, SVAE_ERR_LAUNCH, "kmeans_assign_f64: hipMemsetAsync: %s", hipGetErrorString(e));
  }
  hipLaunchKernelGGL(kmeans_assign_kernel, dim3((unsigned)pair_tile_count(n)), dim3(256), 0, ST(stream), A, lda, d, n, C, ldc, K, prev, label,
                     dist, gap, D, part, changed);
  return check_launch("kmeans_assign_f64");
}

extern "C" int svae_kmeans_chunks(int n, int d, int K) {
  if (n <= 0 || d <= 0 || d > SVAE_CV_MAX_DIM || K < 1 || K > SVAE_KMEANS_MAX_CLUSTERS) return 0;
  return kmeans_plan(n, d, K).chunks;
}

extern "C" int svae_kmeans_update_f64(const double* A, int lda, int d, int n, const int* label, int K, double* part, double* sums,
                                      void* stream) {
  if (int e = kmeans_args("kmeans_update_f64", A, lda, d, n, K)) return e;
  SVAE_REQUIRE(label && part && sums, SVAE_ERR_ARG, "kmeans_update_f64: null argument");
  const KmPlan p = kmeans_plan(n, d, K);
  if (K <= 16)
    kmeans_launch_sums<1>(p, A, lda, d, n, label, K, part, ST(stream));
  else if (K <= 64)
    kmeans_launch_sums<4>(p, A, lda, d, n, label, K, part, ST(stream));
  else
    kmeans_launch_sums<16>(p, A, lda, d, n, label, K, part, ST(stream));
  if (int e = check_launch("kmeans_sums")) return e;
  const long long m = (long long)K * (d + 1);
  hipLaunchKernelGGL(kmeans_chunk_sum_kernel, dim3((unsigned)((m + 15) / 16)), dim3(256), 0, ST(stream), part, p.chunks, m, sums);
  return check_launch("kmeans_chunk_sum");
}

extern "C" int svae_kmeans_finish_f64(const double* sums, int d, int K, const double* C_old, double* C_new, int ldc, const int* changed,
                                      double* rec, void* stream) {
  SVAE_REQUIRE(d > 0 && d <= SVAE_CV_MAX_DIM && K >= 1 && K <= SVAE_KMEANS_MAX_CLUSTERS && ldc >= d, SVAE_ERR_ARG,
               "kmeans_finish_f64: bad args (d=%d K=%d ldc=%d)", d, K, ldc);
  SVAE_REQUIRE(sums && C_old && C_new && rec && C_old != C_new, SVAE_ERR_ARG, "kmeans_finish_f64: null or aliased argument");
  hipLaunchKernelGGL(kmeans_finish_kernel, dim3(1), dim3(256), 0, ST(stream), sums, d, K, C_old, C_new, ldc, changed, rec);
  return check_launch("kmeans_finish_f64");
}
