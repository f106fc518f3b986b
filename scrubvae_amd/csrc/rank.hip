// Ranks of given neighbours among all the other rows, and the sums that trustworthiness, continuity and the co-ranking curves are
// made of.  rank[i][m] = 1 + #{l != i : key(i, l) < key(i, idx[i][m])} with the strict key of knn.hip: the bit pattern of the
// pair_tiles.h squared distance s_il, then the lower index.  Every output is an integer built by integer adds only, so it does not
// depend on scheduling, on the column chunks or on the order of a row's entries.  Nothing of size n^2 is stored.
//   rank_threshold_kernel  one block per row: s(i, idx[i][m]) in the arithmetic of pair_accumulate (0.0, then e = a - b; m = e * e;
//                          s = s + m in feature order; the zero padding of the tiles adds +0), then the row's K (key, index)
//                          thresholds sorted ascending by counting, each with its original column
//   rank_count_kernel      the walk of knn_lists_kernel / mi_count_kernel: a block owns 64 rows (lane = row) and keeps their sorted
//                          thresholds and a histogram [K][64] in LDS.  A candidate at or above the row's largest threshold (held
//                          in registers) costs nothing more; one below it finds b = the number of the row's thresholds <= its key
//                          by a binary search of at most 7 steps and adds 1 to hist[b][row] by an LDS integer atomic.  Each column
//                          chunk (grid y) writes its histograms to its own slab of the work buffer.
//   rank_finish_kernel     one thread per row: the number of keys strictly below the threshold at sorted position p is the sum of
//                          hist[0..p] over the chunks; 1 + that goes to the threshold's original column
//   rank_curves_kernel     pen[k], hit[k] for every k <= K from a rank table, int64, thread = k, combined by integer atomics
#include "svae_internal.h"

#include "knn_buffer.h"  // pair_tiles.h: the tile walk and #pragma clang fp contract(off)

namespace svae {

constexpr int RANK_NGY = 8;        // column chunks per row tile at most
constexpr int RANK_BLOCKS = 512;   // grid y splits the column tiles only while the grid holds fewer blocks than this
constexpr int RANK_TB = 128;       // threads of rank_threshold_kernel and rank_curves_kernel: one per entry of a row
constexpr int RANK_SLAB = 32;      // rows of the rank table that rank_curves_kernel stages at a time
constexpr int RANK_CURVE_BLOCKS = 1024;
static_assert(SVAE_KNN_MAX_K <= RANK_TB, "one thread per entry of a row");

// dynamic LDS of rank_count_kernel, in doubles, after the rows and candidates of pair_tiles.h (the kt region is not used):
// tkey [k][64] uint64, tidx [k][64] int32, hist [k][64] uint32, entry-major as in knn_buffer.h
constexpr int R_KEY = PAIR_LDS_KT;
__host__ __device__ constexpr int rank_lds_words(int k) { return R_KEY + k * HR + k * HR / 2 + k * HR / 2; }
constexpr size_t RANK_LDS_MAX = (size_t)rank_lds_words(SVAE_KNN_MAX_K) * sizeof(double);  // 133,632 B at k = 90: one block per CU
static_assert(RANK_LDS_MAX <= 160 * 1024, "LDS per workgroup");

// Block i, thread m < k: the key of (i, idx[i][m]) and its place among the row's k keys.  An entry that is out of range or the
// row itself reads nothing and gets the key (all ones, KNN_PAD), above every candidate.  Equal keys (a repeated entry) are placed
// in column order, so the places are always a permutation of 0..k-1 and every slot of the row is written.
__global__ __launch_bounds__(RANK_TB) void rank_threshold_kernel(const double* __restrict__ X, int ld, int d, int n,
                                                                 const int* __restrict__ idx, int k, u64* __restrict__ thr_key,
                                                                 int* __restrict__ thr_idx, int* __restrict__ thr_col) {
  __shared__ u64 skey[RANK_TB];
  __shared__ int sidx[RANK_TB];
  const long long i = blockIdx.x;
  const int m = threadIdx.x;
  u64 key = ~0ull;
  int j = KNN_PAD;
  if (m < k) {
    const int c = idx[i * k + m];
    if (c >= 0 && c < n && c != i) {
      const double* a = X + i * ld;
      const double* b = X + (long long)c * ld;
      double s = 0.0;
      for (int f = 0; f < d; ++f) {
        const double e = a[f] - b[f];
        const double mm = e * e;
        s = s + mm;
      }
      key = (u64)__double_as_longlong(s);
      j = c;
    }
  }
  skey[m] = key;
  sidx[m] = j;
  __syncthreads();
  if (m < k) {
    int pos = 0;
    for (int o = 0; o < k; ++o) {
      const u64 ko = skey[o];
      const int jo = sidx[o];
      pos += knn_less(ko, jo, key, j) || (ko == key && jo == j && o < m) ? 1 : 0;
    }
    thr_key[i * k + pos] = key;
    thr_idx[i * k + pos] = j;
    thr_col[i * k + pos] = m;
  }
}

// part [(y * n + row) * k + b]: the candidates of chunk y whose key has exactly b of the row's thresholds at or below it, b < k
__global__ __launch_bounds__(256) void rank_count_kernel(const double* __restrict__ X, int ld, int d, int n, int k, int ch,
                                                         const u64* __restrict__ thr_key, const int* __restrict__ thr_idx,
                                                         int* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  u64* tkey = reinterpret_cast<u64*>(lds + R_KEY);
  int* tidx = reinterpret_cast<int*>(lds + R_KEY + k * HR);
  unsigned* hist = reinterpret_cast<unsigned*>(lds + R_KEY + k * HR + k * HR / 2);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const PairTileRange tr = pair_chunk_tiles(n, ch);
  const long long r0 = tr.r0;
  const long long r = r0 + lane;
  const bool ok = r < n;
  // a row past n holds thresholds below every candidate, so its lanes count nothing
  for (int e = threadIdx.x; e < k * HR; e += 256) {
    const int p = e >> 6;
    const long long rr = r0 + (e & 63);
    tkey[e] = rr < n ? thr_key[rr * k + p] : 0ull;
    tidx[e] = rr < n ? thr_idx[rr * k + p] : -1;
    hist[e] = 0u;
  }
  const u64 top_key = ok ? thr_key[r * k + k - 1] : 0ull;  // the row's largest threshold
  const int top_idx = ok ? thr_idx[r * k + k - 1] : -1;
  const PairRows rows = pair_rows(X, ld, d, n, r0, lds + PAIR_LDS_QS, lds + PAIR_LDS_CS);
  for (int ct = tr.t_lo; ct < tr.t_hi; ++ct) {
    const long long c0 = (long long)ct * HT;
    double s[HQ];
    pair_tile(rows, c0, s);  // its first barrier also ends the setup above
#pragma unroll
    for (int q = 0; q < HQ; ++q) {
      const long long c = c0 + wave * HQ + q;
      const u64 key = (u64)__double_as_longlong(s[q]);
      if (c < n && c != r && knn_less(key, (int)c, top_key, top_idx)) {
        int lo = 0, hi = k - 1;  // the thresholds before lo are at or below the key, those from hi on above it
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (knn_less(key, (int)c, tkey[mid * HR + lane], tidx[mid * HR + lane])) hi = mid;
          else lo = mid + 1;
        }
        atomicAdd(&hist[lo * HR + lane], 1u);
      }
    }
  }
  __syncthreads();  // an empty tile range comes here straight from the setup
  for (int e = threadIdx.x; e < k * HR; e += 256) {
    const long long rr = r0 + (e & 63);
    if (rr < n) part[((long long)blockIdx.y * n + rr) * k + (e >> 6)] = (int)hist[e];
  }
}

__global__ __launch_bounds__(256) void rank_finish_kernel(const int* __restrict__ part, const int* __restrict__ thr_col, int gy, int n,
                                                          int k, int* __restrict__ rank) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  int below = 0;
  for (int p = 0; p < k; ++p) {
    for (int y = 0; y < gy; ++y) below += part[((long long)y * n + r) * k + p];
    const int col = thr_col[r * k + p];  // a place of rank_threshold_kernel: 0 <= col < k
    rank[r * k + col] = 1 + below;
  }
}

// Thread t holds kk = t + 1: pen[kk - 1] += sum_m<kk max(0, rank[i][m] - kk), hit[kk - 1] += #{m < kk : rank[i][m] <= kk} over
// the block's rows; pen_row[i] is the first sum of row i for kk = row_k.  pen and hit are zero on entry.
__global__ __launch_bounds__(RANK_TB) void rank_curves_kernel(const int* __restrict__ rank, int n, int k, int row_k,
                                                              unsigned long long* __restrict__ pen, unsigned long long* __restrict__ hit,
                                                              long long* __restrict__ pen_row) {
  __shared__ int sr[RANK_SLAB * SVAE_KNN_MAX_K];
  const int kk = threadIdx.x + 1;
  long long ap = 0, ah = 0;
  for (long long b0 = (long long)blockIdx.x * RANK_SLAB; b0 < n; b0 += (long long)gridDim.x * RANK_SLAB) {
    const int cnt = (int)min((long long)RANK_SLAB, n - b0);
    __syncthreads();  // the previous slab's reads
    for (int e = threadIdx.x; e < cnt * k; e += RANK_TB) sr[e] = rank[b0 * k + e];
    __syncthreads();
    if (kk <= k) {
      for (int row = 0; row < cnt; ++row) {
        long long p = 0;
        int h = 0;
        for (int m = 0; m < kk; ++m) {
          const int v = sr[row * k + m];
          p += v > kk ? v - kk : 0;
          h += v <= kk ? 1 : 0;
        }
        ap += p;
        ah += h;
        if (kk == row_k) pen_row[b0 + row] = p;
      }
    }
  }
  if (kk <= k) {
    atomicAdd(&pen[kk - 1], (unsigned long long)ap);
    atomicAdd(&hit[kk - 1], (unsigned long long)ah);
  }
}

}  // namespace svae

using namespace svae;

static KnnPlan rank_plan(int n) { return knn_plan(n, RANK_NGY, RANK_BLOCKS); }

static bool rank_sizes_ok(int n, int k) { return n >= 2 && k >= 1 && k <= SVAE_KNN_MAX_K && k <= n - 1; }

extern "C" long long svae_rank_work(int n, int k) {
  if (!rank_sizes_ok(n, k)) return 0;
  return (long long)n * k * 16 + (long long)rank_plan(n).gy * n * k * 4;
}

extern "C" int svae_knn_ranks(const double* X, int ld, int d, int n, const int* idx, int k, void* work, int* rank, void* stream) {
  if (int e = check_pair_rows("knn_ranks", X, ld, d, n, 2)) return e;
  SVAE_REQUIRE(rank_sizes_ok(n, k), SVAE_ERR_ARG, "knn_ranks: bad neighbour count (k=%d n=%d, at most %d)", k, n, SVAE_KNN_MAX_K);
  SVAE_REQUIRE(idx && work && rank, SVAE_ERR_ARG, "knn_ranks: null argument");
  SVAE_REQUIRE((reinterpret_cast<uintptr_t>(work) & 7u) == 0, SVAE_ERR_ALIGN, "knn_ranks: work must be 8-byte aligned");
  const KnnPlan p = rank_plan(n);
  const long long cells = (long long)n * k;
  u64* thr_key = static_cast<u64*>(work);
  int* thr_idx = reinterpret_cast<int*>(thr_key + cells);
  int* thr_col = thr_idx + cells;
  int* part = thr_col + cells;
  hipLaunchKernelGGL(rank_threshold_kernel, dim3((unsigned)n), dim3(RANK_TB), 0, ST(stream), X, ld, d, n, idx, k, thr_key, thr_idx, thr_col);
  if (int e = check_launch("rank_threshold")) return e;
  static DeviceOnce once;
  if (int e = allow_lds(rank_count_kernel, once, (int)RANK_LDS_MAX, "knn_ranks")) return e;
  hipLaunchKernelGGL(rank_count_kernel, dim3(p.gx, p.gy), dim3(256), (size_t)rank_lds_words(k) * sizeof(double), ST(stream), X, ld, d, n, k,
                     p.ch, thr_key, thr_idx, part);
  if (int e = check_launch("rank_count")) return e;
  hipLaunchKernelGGL(rank_finish_kernel, dim3((unsigned)(((long long)n + 255) / 256)), dim3(256), 0, ST(stream), part, thr_col, (int)p.gy, n,
                     k, rank);
  return check_launch("rank_finish");
}

extern "C" int svae_rank_curves(const int* rank, int n, int k, int row_k, long long* pen, long long* hit, long long* pen_row,
                                void* stream) {
  SVAE_REQUIRE(n >= 1 && k >= 1 && k <= SVAE_KNN_MAX_K, SVAE_ERR_ARG, "rank_curves: bad sizes (n=%d k=%d, at most %d)", n, k,
               SVAE_KNN_MAX_K);
  SVAE_REQUIRE(row_k >= 0 && row_k <= k, SVAE_ERR_ARG, "rank_curves: bad row_k (%d, k=%d)", row_k, k);
  SVAE_REQUIRE(rank && pen && hit, SVAE_ERR_ARG, "rank_curves: null argument");
  SVAE_REQUIRE((pen_row != nullptr) == (row_k > 0), SVAE_ERR_ARG, "rank_curves: pen_row belongs to row_k");
  SVAE_REQUIRE(((reinterpret_cast<uintptr_t>(pen) | reinterpret_cast<uintptr_t>(hit) | reinterpret_cast<uintptr_t>(pen_row)) & 7u) == 0,
               SVAE_ERR_ALIGN, "rank_curves: pen, hit and pen_row must be 8-byte aligned");
  hipError_t err = hipMemsetAsync(pen, 0, (size_t)k * sizeof(long long), ST(stream));
  if (err == hipSuccess) err = hipMemsetAsync(hit, 0, (size_t)k * sizeof(long long), ST(stream));
  SVAE_REQUIRE(err == hipSuccess, SVAE_ERR_LAUNCH, "rank_curves: hipMemsetAsync: %s", hipGetErrorString(err));
  const long long slabs = ((long long)n + RANK_SLAB - 1) / RANK_SLAB;
  hipLaunchKernelGGL(rank_curves_kernel, dim3((unsigned)(slabs < RANK_CURVE_BLOCKS ? slabs : RANK_CURVE_BLOCKS)), dim3(RANK_TB), 0, ST(stream),
                     rank, n, k, row_k, reinterpret_cast<unsigned long long*>(pen), reinterpret_cast<unsigned long long*>(hit), pen_row);
  return check_launch("rank_curves");
}
