// Exact k nearest neighbours of every fp64 row, one pass over the n^2 distances, nothing of size n^2 stored.
// The neighbours of row i are the k smallest keys (s_ij, j) over j != i (and group[j] != group[i] when groups are given): s the
// pair_tiles.h squared distance compared by its bit pattern (non-negative doubles order like their bits), then the lower j.  The
// key is strict, so the neighbour set is unique, and the lists are written in key order: nothing depends on thread scheduling or on
// how the columns are split, and no floating-point sum is involved.
//
// A block owns 64 rows (lane = row) and walks its column tiles in ascending order.  Every row has a buffer of KNN_CAP candidates
// in LDS, entry-major (entry e of row r at [e * 64 + r]: conflict-free for the lanes of a wave), filled through a per-row LDS
// counter because the four waves see different candidates of the same row.  Each lane holds the s of its row's current k-th key as
// a threshold and appends only candidates strictly below it: a later candidate with the same s has a higher index than the k-th
// key, which came from an earlier tile, so it can never displace it.  When some row's buffer could overflow at the next tile (more
// than KNN_CAP - 64 entries: a block-uniform test) every buffer with more than k entries is cut to its k smallest keys and the
// thresholds tighten.  After t tiles a row accepts about k / t candidates per tile, so cuts become rare quickly and the distance
// arithmetic bounds the kernel.  At the end each block writes its rows' lists, sorted, to the work buffer, and knn_finish_kernel
// merges the lists of the column chunks of a row by rank (a plain copy when there is one chunk) and takes the square roots.
#include "svae_internal.h"

#include <algorithm>

#include "pair_tiles.h"  // the tile walk and #pragma clang fp contract(off)

namespace svae {

constexpr int KNN_NGY = 8;        // column chunks per row tile at most
constexpr int KNN_BLOCKS = 512;   // grid y splits the column tiles only while the grid holds fewer blocks than this
constexpr int KNN_CAP = 154;      // buffered candidates per row
constexpr int KNN_FULL = KNN_CAP - HT;  // a buffer holding more than this could overflow at the next tile
constexpr int KNN_PAD = INT_MAX;  // index of the padding behind a list of fewer than k candidates (n < 2^31: no row has it)
static_assert(SVAE_KNN_MAX_K <= KNN_FULL, "a buffer cut to k entries takes one more tile");

// dynamic LDS, in doubles, after the rows and candidates of pair_tiles.h (the kt region is not used)
constexpr int N_KEY = PAIR_LDS_KT;                // bkey [KNN_CAP][64] uint64
constexpr int N_IDX = N_KEY + KNN_CAP * HR;       // bidx [KNN_CAP][64] int32
constexpr int N_CNT = N_IDX + KNN_CAP * HR / 2;   // cnt  [64] uint32: entries in each row's buffer
constexpr int N_THS = N_CNT + HR / 2;             // ths  [64] uint64: s of the row's k-th key (all ones: none yet; 0: no row)
constexpr int N_THJ = N_THS + HR;                 // thj  [64] int32: its index
constexpr int N_GRP = N_THJ + HR / 2;             // cgrp [64] int32: group of the tile's columns
constexpr int N_END = N_GRP + HT / 2;
constexpr size_t KNN_LDS = (size_t)N_END * sizeof(double);  // 161,024 B: one block per CU, as hdb_core_kernel
static_assert(KNN_LDS <= 160 * 1024, "LDS per workgroup");

__device__ __forceinline__ bool knn_less(u64 ka, int ja, u64 kb, int jb) { return ka < kb || (ka == kb && ja < jb); }

// Cuts every buffer with more than k entries to its k smallest keys and sets ths / thj to the k-th.  Wave w ranks the entries
// w, w + 4, ... of its rows against the whole buffer to find the k-th key; then wave 0 moves the keys up to it to the front, in
// place (an entry never moves to a higher position).  Block-uniform call; ends with the buffers and ths visible to every thread.
__device__ __forceinline__ void knn_cut(u64* bkey, int* bidx, unsigned* cnt, u64* ths, int* thj, int k, int lane, int wave) {
  const int m = (int)cnt[lane];
  if (m > k) {
    for (int e = wave; e < m; e += 4) {
      const u64 k0 = bkey[e * HR + lane];
      const int j0 = bidx[e * HR + lane];
      int rank = 0;
      for (int o = 0; o < m; ++o) rank += knn_less(bkey[o * HR + lane], bidx[o * HR + lane], k0, j0) ? 1 : 0;
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
      const u64 ke = bkey[e * HR + lane];
      const int je = bidx[e * HR + lane];
      if (!knn_less(ts, tj, ke, je)) {  // key <= the k-th key
        bkey[w * HR + lane] = ke;
        bidx[w * HR + lane] = je;
        ++w;
      }
    }
    cnt[lane] = (unsigned)k;
  }
  __syncthreads();
}

// part_key / part_idx [(y * rpad + row) * k + e]: the k smallest keys of row `row` among the columns of chunk y, ascending, padded
// with (all ones, KNN_PAD) where the chunk holds fewer than k candidates of the row
__global__ __launch_bounds__(256) void knn_lists_kernel(const double* __restrict__ Z, int ld, int d, int n, int k,
                                                        const int* __restrict__ group, int ch, long long rpad,
                                                        u64* __restrict__ part_key, int* __restrict__ part_idx) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  u64* bkey = reinterpret_cast<u64*>(lds + N_KEY);
  int* bidx = reinterpret_cast<int*>(lds + N_IDX);
  unsigned* cnt = reinterpret_cast<unsigned*>(lds + N_CNT);
  u64* ths = reinterpret_cast<u64*>(lds + N_THS);
  int* thj = reinterpret_cast<int*>(lds + N_THJ);
  int* cgrp = reinterpret_cast<int*>(lds + N_GRP);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long r0 = (long long)blockIdx.x * HR;
  const long long r = r0 + lane;
  const bool ok = r < n;
  const int t_lo = (int)blockIdx.y * ch, t_hi = min(((int)blockIdx.y + 1) * ch, pair_tile_count(n));
  const int mygrp = group && ok ? group[r] : 0;
  const PairRows rows = pair_rows(Z, ld, d, n, r0, lds + PAIR_LDS_QS, lds + PAIR_LDS_CS);
  if (threadIdx.x < HR) {
    cnt[lane] = 0u;
    ths[lane] = ok ? ~0ull : 0ull;  // a lane past n accepts nothing
    thj[lane] = KNN_PAD;
  }
  u64 thr = ok ? ~0ull : 0ull;
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
        if (c < n && c != r && !(group && cgrp[cl] == mygrp)) {
          const unsigned pos = atomicAdd(&cnt[lane], 1u);  // < KNN_CAP: at most KNN_FULL before the tile, at most 64 added
          bkey[pos * HR + lane] = key;
          bidx[pos * HR + lane] = (int)c;
        }
      }
    }
    __syncthreads();
    if (__any((int)cnt[lane] > KNN_FULL)) {  // every wave reads the same 64 counters: block-uniform
      knn_cut(bkey, bidx, cnt, ths, thj, k, lane, wave);
      thr = ths[lane];
    }
  }
  __syncthreads();  // an empty tile range comes here straight from the setup
  knn_cut(bkey, bidx, cnt, ths, thj, k, lane, wave);
  // at most k entries per row now: write them in key order, by rank
  const int m = (int)cnt[lane];
  if (ok) {
    u64* out_key = part_key + ((long long)blockIdx.y * rpad + r) * k;
    int* out_idx = part_idx + ((long long)blockIdx.y * rpad + r) * k;
    for (int e = wave; e < k; e += 4) {
      if (e < m) {
        const u64 k0 = bkey[e * HR + lane];
        const int j0 = bidx[e * HR + lane];
        int rank = 0;
        for (int o = 0; o < m; ++o) rank += knn_less(bkey[o * HR + lane], bidx[o * HR + lane], k0, j0) ? 1 : 0;
        out_key[rank] = k0;
        out_idx[rank] = j0;
      } else {
        out_key[e] = ~0ull;
        out_idx[e] = KNN_PAD;
      }
    }
  }
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
    int rank = e;
    for (int y2 = 0; y2 < gy && rank < k; ++y2) {
      if (y2 == y) continue;
      const long long b2 = ((long long)y2 * rpad + row) * k;
      int lo = 0, hi = k;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (knn_less(part_key[b2 + mid], part_idx[b2 + mid], k0, j0)) lo = mid + 1;
        else hi = mid;
      }
      rank += lo;
    }
    if (rank < k) {
      idx[row * k + rank] = j0;
      dist[row * k + rank] = sqrt(__longlong_as_double((long long)k0));
    }
  }
}

}  // namespace svae

using namespace svae;

struct KnnPlan {
  int ch;
  unsigned gx, gy;
  long long rpad;
};

static KnnPlan knn_plan(int n) {
  KnnPlan p;
  const int nt = pair_tile_count(n);
  p.gx = (unsigned)nt;
  const int want = (int)std::min<long long>(std::min(nt, KNN_NGY), (KNN_BLOCKS + (long long)nt - 1) / nt);
  p.ch = (nt + want - 1) / want;
  p.gy = (unsigned)((nt + p.ch - 1) / p.ch);
  p.rpad = (long long)nt * HR;
  return p;
}

static bool knn_sizes_ok(int n, int k) { return n >= 2 && k >= 1 && k <= SVAE_KNN_MAX_K && k <= n - 1; }

extern "C" long long svae_knn_work(int n, int k) {
  if (!knn_sizes_ok(n, k)) return 0;
  const KnnPlan p = knn_plan(n);
  return (long long)p.gy * p.rpad * k * 12;
}

extern "C" int svae_knn(const double* Z, int ld, int d, int n, int k, const int* group, void* work, int* idx, double* dist, void* stream) {
  if (int e = check_pair_rows("knn", Z, ld, d, n, 2)) return e;
  SVAE_REQUIRE(knn_sizes_ok(n, k), SVAE_ERR_ARG, "knn: bad neighbour count (k=%d n=%d, at most %d)", k, n, SVAE_KNN_MAX_K);
  SVAE_REQUIRE(work && idx && dist, SVAE_ERR_ARG, "knn: null argument");
  SVAE_REQUIRE((reinterpret_cast<uintptr_t>(work) & 7u) == 0, SVAE_ERR_ALIGN, "knn: work must be 8-byte aligned");
  const KnnPlan p = knn_plan(n);
  u64* part_key = static_cast<u64*>(work);
  int* part_idx = reinterpret_cast<int*>(part_key + (long long)p.gy * p.rpad * k);
  static DeviceOnce once;
  if (int e = allow_lds(knn_lists_kernel, once, (int)KNN_LDS, "knn")) return e;
  hipLaunchKernelGGL(knn_lists_kernel, dim3(p.gx, p.gy), dim3(256), KNN_LDS, ST(stream), Z, ld, d, n, k, group, p.ch, p.rpad, part_key, part_idx);
  if (int e = check_launch("knn_lists")) return e;
  const long long cells = (long long)n * k;
  hipLaunchKernelGGL(knn_finish_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, ST(stream), part_key, part_idx, (int)p.gy, p.rpad,
                     n, k, idx, dist);
  return check_launch("knn_finish");
}
