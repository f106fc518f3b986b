// The running best k of 64 rows in LDS, the shared layer of knn.hip and mi.hip (rank.hip takes the key order, the plan and
// knn_count_below from here): a block of 256 threads (lane = row, the same rows in each of the 4 waves, as in pair_tiles.h) walks
// its column tiles in ascending order and keeps, for every row, the k smallest keys (s, j) seen so far: s a non-negative double
// compared by its bit pattern, then the lower j.  Below the buffer: the merge of the column chunks' lists, their plan and layout.
//
// Every row has a buffer of CAP candidates, entry-major (entry e of row r at [e * 64 + r]: conflict-free for the lanes of a wave),
// filled through a per-row LDS counter because the four waves see different candidates of the same row.  Each lane holds the s of
// its row's current k-th key as a threshold and appends only candidates strictly below it: a later candidate with the same s has a
// higher index than the k-th key, which came from an earlier tile, so it can never displace it.  When some row's buffer could
// overflow at the next tile (more than CAP - 64 entries: a block-uniform test) every buffer with more than k entries is cut to its
// k smallest keys and the thresholds tighten.  k is read per lane (the same value in the four waves of a row); it may differ from
// row to row, and must not exceed CAP - 64 so that a buffer cut to k entries takes one more tile.
#pragma once
#include <climits>

#include "pair_tiles.h"
#include "svae_internal.h"  // chunk_split, SVAE_REQUIRE

namespace svae {

constexpr int KNN_PAD = INT_MAX;  // index of the padding behind a list of fewer than k candidates (n < 2^31: no row has it)

__device__ __forceinline__ bool knn_less(u64 ka, int ja, u64 kb, int jb) { return ka < kb || (ka == kb && ja < jb); }

template <int CAP>
struct KnnBuffer {
  static constexpr int FULL = CAP - HT;  // a buffer holding more than this could overflow at the next tile
  // LDS, in doubles from the start of the buffer's region
  static constexpr int N_IDX = CAP * HR;           // after key [CAP][64] uint64: idx [CAP][64] int32
  static constexpr int N_CNT = N_IDX + CAP * HR / 2;  // cnt [64] uint32: entries in each row's buffer
  static constexpr int N_THS = N_CNT + HR / 2;     // ths [64] uint64: s of the row's k-th key (all ones: none yet; 0: no row)
  static constexpr int N_THJ = N_THS + HR;         // thj [64] int32: its index
  static constexpr int WORDS = N_THJ + HR / 2;     // doubles in all
  static_assert(CAP > HT && (CAP * HR) % 2 == 0, "a tile may add 64 candidates to a row");

  u64* key;
  int* idx;
  unsigned* cnt;
  u64* ths;
  int* thj;

  __device__ __forceinline__ explicit KnnBuffer(double* lds)
      : key(reinterpret_cast<u64*>(lds)), idx(reinterpret_cast<int*>(lds + N_IDX)), cnt(reinterpret_cast<unsigned*>(lds + N_CNT)),
        ths(reinterpret_cast<u64*>(lds + N_THS)), thj(reinterpret_cast<int*>(lds + N_THJ)) {}

  // Empties the buffers; returns the lane's first threshold.  A lane without a row (ok = false) accepts nothing.  Visible to the
  // block after its next barrier.
  __device__ __forceinline__ u64 reset(bool ok, int lane) const {
    if (threadIdx.x < HR) {
      cnt[lane] = 0u;
      ths[lane] = ok ? ~0ull : 0ull;
      thj[lane] = KNN_PAD;
    }
    return ok ? ~0ull : 0ull;
  }

  // The caller has found k0 below the lane's threshold: at most FULL entries before the tile and at most 64 added, so pos < CAP
  __device__ __forceinline__ void append(int lane, u64 k0, int j0) const {
    const unsigned pos = atomicAdd(&cnt[lane], 1u);
    key[pos * HR + lane] = k0;
    idx[pos * HR + lane] = j0;
  }

  // After the barrier that ends a tile's appends: every wave reads the same 64 counters, so the answer is block-uniform
  __device__ __forceinline__ bool could_overflow(int lane) const { return __any((int)cnt[lane] > FULL) != 0; }

  // Cuts every buffer with more than k entries to its k smallest keys and sets ths / thj to the k-th.  Wave w ranks the entries
  // w, w + 4, ... of its rows against the whole buffer to find the k-th key; then wave 0 moves the keys up to it to the front, in
  // place (an entry never moves to a higher position).  Block-uniform call; ends with the buffers and ths visible to every thread.
  __device__ __forceinline__ void cut(int k, int lane, int wave) const {
    const int m = (int)cnt[lane];
    if (m > k) {
      for (int e = wave; e < m; e += 4) {
        const u64 k0 = key[e * HR + lane];
        const int j0 = idx[e * HR + lane];
        int rank = 0;
        for (int o = 0; o < m; ++o) rank += knn_less(key[o * HR + lane], idx[o * HR + lane], k0, j0) ? 1 : 0;
        if (rank == k - 1) {
          ths[lane] = k0;
          thj[lane] = j0;
        }
      }
    }
    __syncthreads();
    if (wave == 0 && m > k) {
      const u64 ts = ths[lane];
      const int tj = thj[lane];
      int w = 0;
      for (int e = 0; e < m; ++e) {
        const u64 ke = key[e * HR + lane];
        const int je = idx[e * HR + lane];
        if (!knn_less(ts, tj, ke, je)) {  // key <= the k-th key
          key[w * HR + lane] = ke;
          idx[w * HR + lane] = je;
          ++w;
        }
      }
      cnt[lane] = (unsigned)k;
    }
    __syncthreads();
  }

  // After the last cut (at most k entries per row): the row's list in key order, by rank, to out_key / out_idx [kmax], padded
  // behind its entries.  Wave w writes the entries w, w + 4, ...
  __device__ __forceinline__ void write_sorted(int kmax, int lane, int wave, u64* out_key, int* out_idx) const {
    const int m = (int)cnt[lane];
    for (int e = wave; e < kmax; e += 4) {
      if (e < m) {
        const u64 k0 = key[e * HR + lane];
        const int j0 = idx[e * HR + lane];
        int rank = 0;
        for (int o = 0; o < m; ++o) rank += knn_less(key[o * HR + lane], idx[o * HR + lane], k0, j0) ? 1 : 0;
        out_key[rank] = k0;
        out_idx[rank] = j0;
      } else {
        out_key[e] = ~0ull;
        out_idx[e] = KNN_PAD;
      }
    }
  }
};

// lists [gy][rpad][k] of (key, idx), each ascending with the padding last: the number of entries of list b2 below (k0, j0)
__device__ __forceinline__ int knn_count_below(const u64* __restrict__ part_key, const int* __restrict__ part_idx, long long b2, int k,
                                               u64 k0, int j0) {
  int lo = 0, hi = k;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (knn_less(part_key[b2 + mid], part_idx[b2 + mid], k0, j0)) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// The merge of a row's gy lists by rank: the entry (k0, j0) at position e of chunk y's list has the rank e plus the number of
// smaller keys in every other list (the keys are unique).  Exact below `limit`; once the rank reaches it, some value >= limit.
__device__ __forceinline__ int knn_merged_rank(const u64* __restrict__ part_key, const int* __restrict__ part_idx, int gy, long long rpad,
                                               long long row, int k, int y, int e, u64 k0, int j0, int limit) {
  int rank = e;
  for (int y2 = 0; y2 < gy && rank < limit; ++y2) {
    if (y2 == y) continue;
    rank += knn_count_below(part_key, part_idx, ((long long)y2 * rpad + row) * k, k, k0, j0);
  }
  return rank;
}

// The column-chunk plan of a walk over rows x cols pairs: grid x the row tiles, grid y the chunks of chunk_split (svae_internal.h)
// over the column tiles, at most ngy of them
struct KnnPlan {
  int ch;
  unsigned gx, gy;
  long long rpad;
};

inline KnnPlan knn_plan(int rows, int cols, int ngy, int blocks) {
  const int rt = pair_tile_count(rows);
  const ChunkSplit s = chunk_split(pair_tile_count(cols), rt, ngy, blocks);
  return KnnPlan{s.per, (unsigned)rt, (unsigned)s.parts, (long long)rt * HR};
}
inline KnnPlan knn_plan(int n, int ngy, int blocks) { return knn_plan(n, n, ngy, blocks); }

// The lists of a plan in the caller's work buffer: part_key [gy][rpad][k] uint64, then part_idx [gy][rpad][k] int32
inline long long knn_work_bytes(const KnnPlan& p, int k) {
  return (long long)p.gy * p.rpad * k * (long long)(sizeof(u64) + sizeof(int));
}
struct KnnLists {
  u64* key;
  int* idx;
};
inline int knn_work_lists(const char* what, void* work, const KnnPlan& p, int k, KnnLists* l) {
  SVAE_REQUIRE((reinterpret_cast<uintptr_t>(work) & 7u) == 0, SVAE_ERR_ALIGN, "%s: work must be 8-byte aligned", what);
  l->key = static_cast<u64*>(work);
  l->idx = reinterpret_cast<int*>(l->key + (long long)p.gy * p.rpad * k);
  return SVAE_OK;
}

}  // namespace svae
