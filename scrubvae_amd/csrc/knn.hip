// Exact k nearest neighbours of every fp64 row, one pass over the n^2 distances, nothing of size n^2 stored.
// The neighbours of row i are the k smallest keys (s_ij, j) over j != i (and group[j] != group[i] when groups are given): s the
// pair_tiles.h squared distance compared by its bit pattern (non-negative doubles order like their bits), then the lower j.  The
// key is strict, so the neighbour set is unique, and the lists are written in key order: nothing depends on thread scheduling or on
// how the columns are split, and no floating-point sum is involved.
//
// A block owns 64 rows (lane = row) and walks its column tiles in ascending order, with the running best k of every row in the LDS
// buffer of knn_buffer.h (KNN_CAP candidates per row, appended below a per-lane threshold, cut to the k smallest when a buffer could
// overflow at the next tile).  After t tiles a row accepts about k / t candidates per tile, so cuts become rare quickly and the
// distance arithmetic bounds the kernel.  At the end each block writes its rows' lists, sorted, to the work buffer, and
// knn_finish_kernel merges the lists of the column chunks of a row by rank (a plain copy when there is one chunk) and takes the
// square roots.
//
// svae_knn_cross is the same search for a query set Q against a database X (pair_tiles.h with a candidate matrix of its own): the
// key runs over all rows of X, nothing is left out, and the column chunks are planned from the row tiles of Q and the column
// tiles of X.
#include "svae_internal.h"

#include "knn_buffer.h"  // pair_tiles.h: the tile walk and #pragma clang fp contract(off)

namespace svae {

constexpr int KNN_NGY = 8;        // column chunks per row tile at most
constexpr int KNN_BLOCKS = 512;   // grid y splits the column tiles only while the grid holds fewer blocks than this
constexpr int KNN_CAP = 154;      // buffered candidates per row
typedef KnnBuffer<KNN_CAP> KnnBuf;
static_assert(SVAE_KNN_MAX_K <= KnnBuf::FULL, "a buffer cut to k entries takes one more tile");

// dynamic LDS, in doubles, after the rows and candidates of pair_tiles.h (the kt region is not used)
constexpr int N_KEY = PAIR_LDS_KT;                // the buffers of knn_buffer.h
constexpr int N_GRP = N_KEY + KnnBuf::WORDS;      // cgrp [64] int32: group of the tile's columns
constexpr int N_END = N_GRP + HT / 2;
constexpr size_t KNN_LDS = (size_t)N_END * sizeof(double);  // 161,024 B: one block per CU, as hdb_core_kernel
static_assert(KNN_LDS <= 160 * 1024, "LDS per workgroup");

// part_key / part_idx [(y * rpad + row) * k + e]: the k smallest keys of row `row` among the columns of chunk y, ascending, padded
// with (all ones, KNN_PAD) where the chunk holds fewer than k candidates of the row
__global__ __launch_bounds__(256) void knn_lists_kernel(const double* __restrict__ Z, int ld, int d, int n, int k,
                                                        const int* __restrict__ group, int ch, long long rpad,
                                                        u64* __restrict__ part_key, int* __restrict__ part_idx) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const KnnBuf buf(lds + N_KEY);
  int* cgrp = reinterpret_cast<int*>(lds + N_GRP);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long r0 = (long long)blockIdx.x * HR;
  const long long r = r0 + lane;
  const bool ok = r < n;
  const int t_lo = (int)blockIdx.y * ch, t_hi = min(((int)blockIdx.y + 1) * ch, pair_tile_count(n));
  const int mygrp = group && ok ? group[r] : 0;
  const PairRows rows = pair_rows(Z, ld, d, n, r0, lds + PAIR_LDS_QS, lds + PAIR_LDS_CS);
  u64 thr = buf.reset(ok, lane);
  for (int ct = t_lo; ct < t_hi; ++ct) {
    const long long c0 = (long long)ct * HT;
    // the previous tile's reads of cgrp ended at the barrier after its appends; the barriers of pair_tile publish this write
    if (group && threadIdx.x < HT) cgrp[threadIdx.x] = c0 + threadIdx.x < n ? group[c0 + threadIdx.x] : 0;
    double s[HQ];
    pair_tile(rows, c0, s);  // its first barrier also ends the setup above and the previous tile's cut
#pragma unroll
    for (int q = 0; q < HQ; ++q) {
      const u64 key = (u64)__double_as_longlong(s[q]);
      if (key < thr) {
        const int cl = wave * HQ + q;
        const long long c = c0 + cl;
        if (c < n && c != r && !(group && cgrp[cl] == mygrp)) buf.append(lane, key, (int)c);
      }
    }
    __syncthreads();
    if (buf.could_overflow(lane)) {
      buf.cut(k, lane, wave);
      thr = buf.ths[lane];
    }
  }
  __syncthreads();  // an empty tile range comes here straight from the setup
  buf.cut(k, lane, wave);
  if (ok) buf.write_sorted(k, lane, wave, part_key + ((long long)blockIdx.y * rpad + r) * k, part_idx + ((long long)blockIdx.y * rpad + r) * k);
}

// The same walk for the m rows of Q against the n rows of X (svae_knn_cross): every column is a candidate, a query that equals a
// reference row included, so there is no self or group test.  When d > 64 the rows restaged per tile come from Q (pair_rows).
__global__ __launch_bounds__(256) void knn_cross_lists_kernel(const double* __restrict__ Q, int ldq, int m, const double* __restrict__ X,
                                                              int ldx, int n, int d, int k, int ch, long long rpad,
                                                              u64* __restrict__ part_key, int* __restrict__ part_idx) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const KnnBuf buf(lds + N_KEY);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long r0 = (long long)blockIdx.x * HR;
  const long long r = r0 + lane;
  const bool ok = r < m;
  const int t_lo = (int)blockIdx.y * ch, t_hi = min(((int)blockIdx.y + 1) * ch, pair_tile_count(n));
  const PairRows rows = pair_rows(Q, ldq, d, m, r0, lds + PAIR_LDS_QS, lds + PAIR_LDS_CS, X, ldx, n);
  u64 thr = buf.reset(ok, lane);
  for (int ct = t_lo; ct < t_hi; ++ct) {
    const long long c0 = (long long)ct * HT;
    double s[HQ];
    pair_tile(rows, c0, s);  // its first barrier also ends the setup above and the previous tile's cut
#pragma unroll
    for (int q = 0; q < HQ; ++q) {
      const u64 key = (u64)__double_as_longlong(s[q]);
      if (key < thr) {
        const long long c = c0 + wave * HQ + q;
        if (c < n) buf.append(lane, key, (int)c);
      }
    }
    __syncthreads();
    if (buf.could_overflow(lane)) {
      buf.cut(k, lane, wave);
      thr = buf.ths[lane];
    }
  }
  __syncthreads();
  buf.cut(k, lane, wave);
  if (ok) buf.write_sorted(k, lane, wave, part_key + ((long long)blockIdx.y * rpad + r) * k, part_idx + ((long long)blockIdx.y * rpad + r) * k);
}

// One thread per (row, position e): the entry at e of each chunk's list goes to its rank among all the chunks' entries of the row,
// e plus the number of smaller keys in every other list (a binary search: the lists ascend, padding last).  Keys are unique, so
// every rank below k is written exactly once when the row has at least k candidates.
__global__ __launch_bounds__(256) void knn_finish_kernel(const u64* __restrict__ part_key, const int* __restrict__ part_idx, int gy,
                                                         long long rpad, int n, int k, int* __restrict__ idx, double* __restrict__ dist) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= (long long)n * k) return;
  const long long row = g / k;
  const int e = (int)(g - row * k);
  for (int y = 0; y < gy; ++y) {
    const long long base = ((long long)y * rpad + row) * k;
    const u64 k0 = part_key[base + e];
    const int j0 = part_idx[base + e];
    if (j0 == KNN_PAD) continue;
    const int rank = knn_merged_rank(part_key, part_idx, gy, rpad, row, k, y, e, k0, j0, k);
    if (rank < k) {
      idx[row * k + rank] = j0;
      dist[row * k + rank] = sqrt(__longlong_as_double((long long)k0));
    }
  }
}

}  // namespace svae

using namespace svae;

// the row tiles counted from the m searching rows and the column tiles from the n searched ones
static KnnPlan knn_plan(int m, int n) { return knn_plan(m, n, KNN_NGY, KNN_BLOCKS); }

static int knn_finish(const KnnPlan& p, const KnnLists& l, int rows, int k, int* idx, double* dist, void* stream) {
  const long long cells = (long long)rows * k;
  hipLaunchKernelGGL(knn_finish_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, ST(stream), l.key, l.idx, (int)p.gy, p.rpad,
                     rows, k, idx, dist);
  return check_launch("knn_finish");
}

static bool knn_sizes_ok(int n, int k) { return n >= 2 && k >= 1 && k <= SVAE_KNN_MAX_K && k <= n - 1; }

extern "C" long long svae_knn_work(int n, int k) {
  if (!knn_sizes_ok(n, k)) return 0;
  return knn_work_bytes(knn_plan(n, n), k);
}

extern "C" int svae_knn(const double* Z, int ld, int d, int n, int k, const int* group, void* work, int* idx, double* dist, void* stream) {
  if (int e = check_pair_rows("knn", Z, ld, d, n, 2)) return e;
  SVAE_REQUIRE(knn_sizes_ok(n, k), SVAE_ERR_ARG, "knn: bad neighbour count (k=%d n=%d, at most %d)", k, n, SVAE_KNN_MAX_K);
  SVAE_REQUIRE(work && idx && dist, SVAE_ERR_ARG, "knn: null argument");
  const KnnPlan p = knn_plan(n, n);
  KnnLists l;
  if (int e = knn_work_lists("knn", work, p, k, &l)) return e;
  static DeviceOnce once;
  if (int e = allow_lds(knn_lists_kernel, once, (int)KNN_LDS, "knn")) return e;
  hipLaunchKernelGGL(knn_lists_kernel, dim3(p.gx, p.gy), dim3(256), KNN_LDS, ST(stream), Z, ld, d, n, k, group, p.ch, p.rpad, l.key, l.idx);
  if (int e = check_launch("knn_lists")) return e;
  return knn_finish(p, l, n, k, idx, dist, stream);
}

static bool knn_cross_sizes_ok(int m, int n, int k) { return m >= 1 && n >= 1 && k >= 1 && k <= SVAE_KNN_MAX_K && k <= n; }

extern "C" long long svae_knn_cross_work(int m, int n, int k) {
  if (!knn_cross_sizes_ok(m, n, k)) return 0;
  return knn_work_bytes(knn_plan(m, n), k);
}

extern "C" int svae_knn_cross(const double* Q, int ldq, int m, const double* X, int ldx, int n, int d, int k, void* work, int* idx,
                              double* dist, void* stream) {
  if (int e = check_pair_rows("knn_cross (queries)", Q, ldq, d, m, 1)) return e;
  if (int e = check_pair_rows("knn_cross (reference)", X, ldx, d, n, 1)) return e;
  SVAE_REQUIRE(knn_cross_sizes_ok(m, n, k), SVAE_ERR_ARG, "knn_cross: bad neighbour count (k=%d n=%d, at most %d)", k, n, SVAE_KNN_MAX_K);
  SVAE_REQUIRE(work && idx && dist, SVAE_ERR_ARG, "knn_cross: null argument");
  const KnnPlan p = knn_plan(m, n);
  KnnLists l;
  if (int e = knn_work_lists("knn_cross", work, p, k, &l)) return e;
  static DeviceOnce once;
  if (int e = allow_lds(knn_cross_lists_kernel, once, (int)KNN_LDS, "knn_cross")) return e;
  hipLaunchKernelGGL(knn_cross_lists_kernel, dim3(p.gx, p.gy), dim3(256), KNN_LDS, ST(stream), Q, ldq, m, X, ldx, n, d, k, p.ch, p.rpad, l.key,
                     l.idx);
  if (int e = check_launch("knn_cross_lists")) return e;
  return knn_finish(p, l, m, k, idx, dist, stream);
}
