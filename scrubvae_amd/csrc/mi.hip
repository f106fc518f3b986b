// k-nearest-neighbour estimate of the mutual information of fp64 rows z and a variable y: Kraskov-Stoegbauer-Grassberger
// (algorithm 1) for a real y of 1..4 features, Ross (2014) for integer labels.  Three launches, nothing of size n^2 stored, every
// output an integer or one order statistic until the closing sums:
//   mi_radius_kernel    rho2 [n]: the k-th smallest key of every row over j != i.  Real y: the key is max(s^z_ij, s^y_ij) (the
//                       squared max-metric of the joint space).  Labels: the key is s^z_ij over the j with lab_j == lab_i, and k is
//                       the row's own kk[i].  s is the pair_tiles.h squared distance, compared by its bit pattern.
//   mi_count_kernel     nz [n] = #{j != i : s^z_ij < rho2_i} and, for a real y, ny [n] = #{j != i : s^y_ij < rho2_i}, both strict
//   mi_psi_sums_kernel  out[0] = sum_i psi(nz_i + 1), out[1] = sum_i psi(ny_i + 1), in the fixed order of fixed_sum.h
// The caller closes with I = psi(n) + psi(k) - out[0] / n - out[1] / n (real y), or the label form, on the host.
//
// mi_radius_kernel is the walk of knn_lists_kernel: a block owns 64 rows (lane = row), walks its column tiles in ascending order
// and keeps the running best k of every row in the LDS buffer of knn_buffer.h.  The row itself is left out by index, so a
// duplicate row counts at 0.  Each lane keeps its row's q <= 4 values of y in registers and the tile's 64 rows of y sit in a small
// LDS array; s^y is summed in feature order like s^z.  A finish kernel merges the column chunks by rank and writes only the value
// of the k-th key.  The counts are int32, combined over the four waves in LDS and over the column chunks by global integer
// atomics: exact, and independent of scheduling and of the chunking.
//
// Below them, on the same walk, buffer, finish kernel and psi sums: the integer parts of the conditional estimate I(z; y | c)
// (cmi_radius_kernel, cmi_count_kernel) and the draw of its local permutation null (cmi_local_perm_kernel).
#include "svae_internal.h"

#include "fixed_sum.h"
#include "knn_buffer.h"  // pair_tiles.h: the tile walk and #pragma clang fp contract(off)

namespace svae {

constexpr int MI_NGY = 8;        // column chunks per row tile at most
constexpr int MI_BLOCKS = 512;   // grid y splits the column tiles only while the grid holds fewer blocks than this
constexpr int MI_CAP = 128;      // buffered candidates per row: a buffer cut to k <= 32 entries takes two tiles at least
typedef KnnBuffer<MI_CAP> MiBuf;
static_assert(SVAE_MI_MAX_K <= MI_CAP - HT, "a buffer cut to k entries takes one more tile");

// dynamic LDS, in doubles, after the rows and candidates of pair_tiles.h (the kt region is not used)
constexpr int MI_Y = PAIR_LDS_KT;                         // cy [64][4] fp64: y of the tile's columns, zero past q and past n
constexpr int MI_LAB = MI_Y + HT * SVAE_MI_MAX_Y;         // clab [64] int32: label of the tile's columns
constexpr int MI_KEY = MI_LAB + HT / 2;                   // the buffers of knn_buffer.h (radius kernel)
constexpr int MI_END = MI_KEY + MiBuf::WORDS;
constexpr size_t MI_RADIUS_LDS = (size_t)MI_END * sizeof(double);  // 143,104 B: one block per CU
static_assert(MI_RADIUS_LDS <= 160 * 1024, "LDS per workgroup");
constexpr int MI_CNT = MI_KEY;                            // cz, cy counts [2][4][64] int32 (count kernel)
constexpr size_t MI_COUNT_LDS = (size_t)(MI_CNT + 2 * 4 * HR / 2) * sizeof(double);  // 45,824 B: room for three blocks per CU
static_assert(MI_COUNT_LDS <= 64 * 1024, "below the default dynamic LDS limit");

// y of the tile's 64 columns: thread t stages feature t & 3 of column t >> 2.  The previous tile's reads of cy ended at the
// barrier after its appends (or counts); the barriers of pair_tile publish this write.
__device__ __forceinline__ void mi_stage_y(const double* __restrict__ Y, int q, int n, long long c0, double* cy) {
  const int cl = threadIdx.x >> 2, f = threadIdx.x & 3;
  cy[threadIdx.x] = f < q && c0 + cl < n ? Y[(c0 + cl) * q + f] : 0.0;
}

// s^y of the lane's row against column cl of the tile, in feature order; the features past q are zero on both sides and add +0
__device__ __forceinline__ double mi_sy(const double (&my)[SVAE_MI_MAX_Y], const double* cy, int cl) {
  double s = 0.0;
#pragma unroll
  for (int f = 0; f < SVAE_MI_MAX_Y; ++f) {
    const double e = my[f] - cy[cl * SVAE_MI_MAX_Y + f];
    const double m = e * e;
    s = s + m;
  }
  return s;
}

// part_key / part_idx [(y * rpad + row) * k + e]: the smallest keys of row `row` among the columns of chunk y, ascending, at most
// the row's own k of them (kk[row] with labels), padded with (all ones, KNN_PAD) up to k
template <bool LABELS>
__global__ __launch_bounds__(256) void mi_radius_kernel(const double* __restrict__ Z, int ld, int d, int n, const double* __restrict__ Y,
                                                        int q, const int* __restrict__ lab, const int* __restrict__ kk, int k, int ch,
                                                        long long rpad, u64* __restrict__ part_key, int* __restrict__ part_idx) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const MiBuf buf(lds + MI_KEY);
  double* cy = lds + MI_Y;
  int* clab = reinterpret_cast<int*>(lds + MI_LAB);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long r0 = (long long)blockIdx.x * HR;
  const long long r = r0 + lane;
  const bool ok = r < n;
  const int t_lo = (int)blockIdx.y * ch, t_hi = min(((int)blockIdx.y + 1) * ch, pair_tile_count(n));
  double my[SVAE_MI_MAX_Y] = {0.0, 0.0, 0.0, 0.0};
  int mylab = 0, myk = k;
  if (LABELS) {
    if (ok) {
      mylab = lab[r];
      myk = max(1, min(kk[r], k));  // the caller guarantees 1 <= kk <= k; the buffers rely on it
    }
  } else {
#pragma unroll
    for (int f = 0; f < SVAE_MI_MAX_Y; ++f)
      if (ok && f < q) my[f] = Y[r * q + f];
  }
  const PairRows rows = pair_rows(Z, ld, d, n, r0, lds + PAIR_LDS_QS, lds + PAIR_LDS_CS);
  u64 thr = buf.reset(ok, lane);
  for (int ct = t_lo; ct < t_hi; ++ct) {
    const long long c0 = (long long)ct * HT;
    if (LABELS) {
      if (threadIdx.x < HT) clab[threadIdx.x] = c0 + threadIdx.x < n ? lab[c0 + threadIdx.x] : 0;
    } else {
      mi_stage_y(Y, q, n, c0, cy);
    }
    double s[HQ];
    pair_tile(rows, c0, s);  // its first barrier also ends the setup above and the previous tile's cut
#pragma unroll
    for (int c4 = 0; c4 < HQ; ++c4) {
      const int cl = wave * HQ + c4;
      double m = s[c4];
      if (!LABELS) {
        const double sy = mi_sy(my, cy, cl);
        m = sy > m ? sy : m;
      }
      const u64 key = (u64)__double_as_longlong(m);
      if (key < thr) {
        const long long c = c0 + cl;
        if (c < n && c != r && (!LABELS || clab[cl] == mylab)) buf.append(lane, key, (int)c);
      }
    }
    __syncthreads();
    if (buf.could_overflow(lane)) {
      buf.cut(myk, lane, wave);
      thr = buf.ths[lane];
    }
  }
  __syncthreads();  // an empty tile range comes here straight from the setup
  buf.cut(myk, lane, wave);
  if (ok) buf.write_sorted(k, lane, wave, part_key + ((long long)blockIdx.y * rpad + r) * k, part_idx + ((long long)blockIdx.y * rpad + r) * k);
}

// One thread per (row, position e), ranking the entry at e of each chunk's list among all the chunks' entries of the row
// (knn_merged_rank).  Keys are unique, so exactly one entry has the rank k - 1 (kk[row] - 1 with labels) when the row has that
// many candidates: its s is rho2.
__global__ __launch_bounds__(256) void mi_finish_kernel(const u64* __restrict__ part_key, const int* __restrict__ part_idx, int gy,
                                                        long long rpad, int n, int k, const int* __restrict__ kk, double* __restrict__ rho2) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= (long long)n * k) return;
  const long long row = g / k;
  const int e = (int)(g - row * k);
  const int want = (kk ? max(1, min(kk[row], k)) : k) - 1;
  for (int y = 0; y < gy; ++y) {
    const long long base = ((long long)y * rpad + row) * k;
    const u64 k0 = part_key[base + e];
    const int j0 = part_idx[base + e];
    if (j0 == KNN_PAD) continue;
    const int rank = knn_merged_rank(part_key, part_idx, gy, rpad, row, k, y, e, k0, j0, want + 1);
    if (rank == want) rho2[row] = __longlong_as_double((long long)k0);
  }
}

// nz and ny are zero on entry; every block adds the counts of its rows over its column tiles
template <bool REAL>
__global__ __launch_bounds__(256) void mi_count_kernel(const double* __restrict__ Z, int ld, int d, int n, const double* __restrict__ Y,
                                                       int q, const double* __restrict__ rho2, int ch, int* __restrict__ nz,
                                                       int* __restrict__ ny) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* cy = lds + MI_Y;
  int* cnt = reinterpret_cast<int*>(lds + MI_CNT);  // [which][wave][lane]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const PairTileRange tr = pair_chunk_tiles(n, ch);
  const long long r = tr.r0 + lane;
  const bool ok = r < n;
  const u64 rb = ok ? (u64)__double_as_longlong(rho2[r]) : 0ull;  // a lane past n counts nothing
  double my[SVAE_MI_MAX_Y] = {0.0, 0.0, 0.0, 0.0};
  if (REAL) {
#pragma unroll
    for (int f = 0; f < SVAE_MI_MAX_Y; ++f)
      if (ok && f < q) my[f] = Y[r * q + f];
  }
  const PairRows rows = pair_rows(Z, ld, d, n, tr.r0, lds + PAIR_LDS_QS, lds + PAIR_LDS_CS);
  int az = 0, ay = 0;
  for (int ct = tr.t_lo; ct < tr.t_hi; ++ct) {
    const long long c0 = (long long)ct * HT;
    if (REAL) mi_stage_y(Y, q, n, c0, cy);
    double s[HQ];
    pair_tile(rows, c0, s);
#pragma unroll
    for (int c4 = 0; c4 < HQ; ++c4) {
      const int cl = wave * HQ + c4;
      const long long c = c0 + cl;
      const bool live = c < n && c != r;
      az += live && (u64)__double_as_longlong(s[c4]) < rb ? 1 : 0;
      if (REAL) ay += live && (u64)__double_as_longlong(mi_sy(my, cy, cl)) < rb ? 1 : 0;
    }
    if (REAL) __syncthreads();  // the reads of cy end here; the next tile stages it again
  }
  cnt[wave * HR + lane] = az;
  cnt[(4 + wave) * HR + lane] = ay;
  __syncthreads();
  if (wave == 0 && ok) {
    atomicAdd(&nz[r], ((cnt[lane] + cnt[HR + lane]) + cnt[2 * HR + lane]) + cnt[3 * HR + lane]);
    if (REAL) atomicAdd(&ny[r], ((cnt[4 * HR + lane] + cnt[5 * HR + lane]) + cnt[6 * HR + lane]) + cnt[7 * HR + lane]);
  }
}

// psi of a positive integer: the harmonic sum below 16, the asymptotic series from 16 on (the recipe of eval/mutual_info.py)
__device__ __forceinline__ double mi_psi(int m) {
  if (m < 16) {
    double h = 0.0;
    for (int j = 1; j < m; ++j) h = h + 1.0 / (double)j;
    return -0.5772156649015329 + h;
  }
  const double x = (double)m;
  const double t = 1.0 / (x * x);
  return log(x) - 0.5 / x - t * (1.0 / 12.0 - t * (1.0 / 120.0 - t * (1.0 / 252.0 - t * (1.0 / 240.0 - t / 132.0))));
}

// block b: out[b] = sum_i psi(v_b[i] + 1) in the order of block_sum_of (fixed_sum.h): thread t adds the terms t, t + 256, ...
// compensated, then the tree
__global__ __launch_bounds__(256) void mi_psi_sums_kernel(const int* __restrict__ a, const int* __restrict__ b, long long n,
                                                          double* __restrict__ out) {
  __shared__ double red[256];
  const int* v = blockIdx.x == 0 ? a : b;
  NeumaierSums<1> acc;
  for (long long i = threadIdx.x; i < n; i += 256) acc.add(0, mi_psi(v[i] + 1));
  red[threadIdx.x] = acc.total(0);
  block_tree<256, 1>(red);
  if (threadIdx.x == 0) out[blockIdx.x] = red[0];
}

// ---- conditional mutual information I(z; y | c): Frenzel-Pompe (2007) for a real c, the estimate inside every class for labels ----
//   cmi_radius_kernel   rho2 [n]: the k-th smallest key of every row over j != i.  Real c: the key is max(s^z_ij, s^y_ij, s^c_ij).
//                       Labels: the key is max(s^z_ij, s^y_ij) over the j with clab_j == clab_i.  The walk and buffer of
//                       mi_radius_kernel with one k for every row; mi_finish_kernel merges the chunks.
//   cmi_count_kernel    real c: nzc = #{max(s^z, s^c) < rho2_i}, nyc = #{max(s^y, s^c) < rho2_i}, nc = #{s^c < rho2_i};
//                       labels: nzc = #{same label, s^z < rho2_i}, nyc = #{same label, s^y < rho2_i}; all strict, over j != i
// c is staged and summed like y (mi_stage_y, mi_sy): the two caps are one number.
static_assert(SVAE_CMI_MAX_C == SVAE_MI_MAX_Y, "c is staged by mi_stage_y and summed by mi_sy");

// dynamic LDS of the two kernels, in doubles, after the rows and candidates of pair_tiles.h
constexpr int CMI_Y = PAIR_LDS_KT;                        // cy [64][4] fp64: y of the tile's columns
constexpr int CMI_C = CMI_Y + HT * SVAE_MI_MAX_Y;         // cc [64][4] fp64: c of the tile's columns
constexpr int CMI_LAB = CMI_C + HT * SVAE_CMI_MAX_C;      // clab [64] int32: label of the tile's columns
constexpr int CMI_KEY = CMI_LAB + HT / 2;                 // the buffers of knn_buffer.h (radius kernel)
constexpr int CMI_END = CMI_KEY + MiBuf::WORDS;
constexpr size_t CMI_RADIUS_LDS = (size_t)CMI_END * sizeof(double);  // 145,152 B: one block per CU
static_assert(CMI_RADIUS_LDS == MI_RADIUS_LDS + 2048 && CMI_RADIUS_LDS <= 160 * 1024, "LDS per workgroup");
constexpr int CMI_CNT = CMI_KEY;                          // zc, yc, c counts [3][4][64] int32 (count kernel)
constexpr size_t CMI_COUNT_LDS = (size_t)(CMI_CNT + 3 * 4 * HR / 2) * sizeof(double);  // 48,896 B
static_assert(CMI_COUNT_LDS <= 64 * 1024, "below the default dynamic LDS limit");

__device__ __forceinline__ u64 cmi_bits(double s) { return (u64)__double_as_longlong(s); }
__device__ __forceinline__ double cmi_max(double a, double b) { return b > a ? b : a; }

template <bool CLAB>
__global__ __launch_bounds__(256) void cmi_radius_kernel(const double* __restrict__ Z, int ld, int d, int n, const double* __restrict__ Y,
                                                         int q, const double* __restrict__ C, int p, const int* __restrict__ lab, int k,
                                                         int ch, long long rpad, u64* __restrict__ part_key, int* __restrict__ part_idx) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const MiBuf buf(lds + CMI_KEY);
  double* cy = lds + CMI_Y;
  double* cc = lds + CMI_C;
  int* clab = reinterpret_cast<int*>(lds + CMI_LAB);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long r0 = (long long)blockIdx.x * HR;
  const long long r = r0 + lane;
  const bool ok = r < n;
  const int t_lo = (int)blockIdx.y * ch, t_hi = min(((int)blockIdx.y + 1) * ch, pair_tile_count(n));
  double my[SVAE_MI_MAX_Y] = {0.0, 0.0, 0.0, 0.0}, mc[SVAE_CMI_MAX_C] = {0.0, 0.0, 0.0, 0.0};
  int mylab = 0;
#pragma unroll
  for (int f = 0; f < SVAE_MI_MAX_Y; ++f) {
    if (ok && f < q) my[f] = Y[r * q + f];
    if (!CLAB && ok && f < p) mc[f] = C[r * p + f];
  }
  if (CLAB && ok) mylab = lab[r];
  const PairRows rows = pair_rows(Z, ld, d, n, r0, lds + PAIR_LDS_QS, lds + PAIR_LDS_CS);
  u64 thr = buf.reset(ok, lane);
  for (int ct = t_lo; ct < t_hi; ++ct) {
    const long long c0 = (long long)ct * HT;
    mi_stage_y(Y, q, n, c0, cy);
    if (CLAB) {
      if (threadIdx.x < HT) clab[threadIdx.x] = c0 + threadIdx.x < n ? lab[c0 + threadIdx.x] : 0;
    } else {
      mi_stage_y(C, p, n, c0, cc);
    }
    double s[HQ];
    pair_tile(rows, c0, s);  // its first barrier also ends the setup above and the previous tile's cut
#pragma unroll
    for (int c4 = 0; c4 < HQ; ++c4) {
      const int cl = wave * HQ + c4;
      double m = cmi_max(s[c4], mi_sy(my, cy, cl));
      if (!CLAB) m = cmi_max(m, mi_sy(mc, cc, cl));
      const u64 key = cmi_bits(m);
      if (key < thr) {
        const long long c = c0 + cl;
        if (c < n && c != r && (!CLAB || clab[cl] == mylab)) buf.append(lane, key, (int)c);
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

// nzc, nyc and nc are zero on entry; every block adds the counts of its rows over its column tiles
template <bool CLAB>
__global__ __launch_bounds__(256) void cmi_count_kernel(const double* __restrict__ Z, int ld, int d, int n, const double* __restrict__ Y,
                                                        int q, const double* __restrict__ C, int p, const int* __restrict__ lab,
                                                        const double* __restrict__ rho2, int ch, int* __restrict__ nzc,
                                                        int* __restrict__ nyc, int* __restrict__ nc) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* cy = lds + CMI_Y;
  double* cc = lds + CMI_C;
  int* clab = reinterpret_cast<int*>(lds + CMI_LAB);
  int* cnt = reinterpret_cast<int*>(lds + CMI_CNT);  // [which][wave][lane]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const PairTileRange tr = pair_chunk_tiles(n, ch);
  const long long r = tr.r0 + lane;
  const bool ok = r < n;
  const u64 rb = ok ? cmi_bits(rho2[r]) : 0ull;  // a lane past n counts nothing
  double my[SVAE_MI_MAX_Y] = {0.0, 0.0, 0.0, 0.0}, mc[SVAE_CMI_MAX_C] = {0.0, 0.0, 0.0, 0.0};
  int mylab = 0;
#pragma unroll
  for (int f = 0; f < SVAE_MI_MAX_Y; ++f) {
    if (ok && f < q) my[f] = Y[r * q + f];
    if (!CLAB && ok && f < p) mc[f] = C[r * p + f];
  }
  if (CLAB && ok) mylab = lab[r];
  const PairRows rows = pair_rows(Z, ld, d, n, tr.r0, lds + PAIR_LDS_QS, lds + PAIR_LDS_CS);
  int azc = 0, ayc = 0, ac = 0;
  for (int ct = tr.t_lo; ct < tr.t_hi; ++ct) {
    const long long c0 = (long long)ct * HT;
    mi_stage_y(Y, q, n, c0, cy);
    if (CLAB) {
      if (threadIdx.x < HT) clab[threadIdx.x] = c0 + threadIdx.x < n ? lab[c0 + threadIdx.x] : 0;
    } else {
      mi_stage_y(C, p, n, c0, cc);
    }
    double s[HQ];
    pair_tile(rows, c0, s);
#pragma unroll
    for (int c4 = 0; c4 < HQ; ++c4) {
      const int cl = wave * HQ + c4;
      const long long c = c0 + cl;
      const double sy = mi_sy(my, cy, cl);
      if (CLAB) {
        const bool live = c < n && c != r && clab[cl] == mylab;
        azc += live && cmi_bits(s[c4]) < rb ? 1 : 0;
        ayc += live && cmi_bits(sy) < rb ? 1 : 0;
      } else {
        const bool live = c < n && c != r;
        const double sc = mi_sy(mc, cc, cl);
        azc += live && cmi_bits(cmi_max(s[c4], sc)) < rb ? 1 : 0;
        ayc += live && cmi_bits(cmi_max(sy, sc)) < rb ? 1 : 0;
        ac += live && cmi_bits(sc) < rb ? 1 : 0;
      }
    }
    __syncthreads();  // the reads of cy, cc and clab end here; the next tile stages them again
  }
  cnt[wave * HR + lane] = azc;
  cnt[(4 + wave) * HR + lane] = ayc;
  cnt[(8 + wave) * HR + lane] = ac;
  __syncthreads();
  if (wave == 0 && ok) {
    atomicAdd(&nzc[r], ((cnt[lane] + cnt[HR + lane]) + cnt[2 * HR + lane]) + cnt[3 * HR + lane]);
    atomicAdd(&nyc[r], ((cnt[4 * HR + lane] + cnt[5 * HR + lane]) + cnt[6 * HR + lane]) + cnt[7 * HR + lane]);
    if (!CLAB) atomicAdd(&nc[r], ((cnt[8 * HR + lane] + cnt[9 * HR + lane]) + cnt[10 * HR + lane]) + cnt[11 * HR + lane]);
  }
}

// The draw of the local permutation null (Runge 2018): block b is one wave and draws permutation b.  Rows are visited in the
// order order[b][0..n); lane e holds the row's e-th scanned donor j = nbr[i][scan[b][i][e]] and its bit of the used-bitmap in LDS;
// one ballot picks the first unused donor in scan order, or the last one tried when all kp are used.  One wave-step per row.  An
// entry out of range reads and marks nothing: a row index past n skips the visit, a donor past n counts as used.
constexpr int CMI_PERM_MAX_N = 1 << 19;  // the bitmap: n / 8 bytes, at most 64 KiB
__global__ __launch_bounds__(64) void cmi_local_perm_kernel(const int* __restrict__ nbr, int n, int kp, const int* __restrict__ order,
                                                            const unsigned char* __restrict__ scan, int* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned used[];
  const int lane = threadIdx.x;
  const int words = (n + 31) >> 5;
  for (int w = lane; w < words; w += 64) used[w] = 0u;
  const int* ord = order + (long long)blockIdx.x * n;
  const unsigned char* sc = scan + (long long)blockIdx.x * n * kp;
  int* o = out + (long long)blockIdx.x * n;
  // the candidate of this lane for visit t: independent of the bitmap, so the loads of visit t + 1 are issued before visit t ends
  auto candidate = [&](int t, int* i_out) {
    int j = -1;
    const int i = t < n ? ord[t] : -1;
    if (i >= 0 && i < n && lane < kp) {
      const int pos = min((int)sc[(long long)i * kp + lane], kp - 1);
      j = nbr[(long long)i * kp + pos];
    }
    *i_out = i;
    return j;
  };
  int i, j = candidate(0, &i);
  for (int t = 0; t < n; ++t) {
    int i2;
    const int j2 = candidate(t + 1, &i2);
    __syncthreads();  // one wave: orders the bitmap write of the previous visit (and the zeroing) before this read
    const bool in = j >= 0 && j < n;
    const bool free_ = lane < kp && in && !((used[in ? j >> 5 : 0] >> (j & 31)) & 1u);
    const unsigned long long mask = __ballot(free_);
    const int pick = mask ? __ffsll((long long)mask) - 1 : kp - 1;
    const int jp = __shfl(j, pick);
    if (lane == 0 && i >= 0 && i < n) {
      o[i] = jp;
      if (jp >= 0 && jp < n) used[jp >> 5] |= 1u << (jp & 31);
    }
    i = i2;
    j = j2;
  }
}

}  // namespace svae

using namespace svae;

static KnnPlan mi_plan(int n) { return knn_plan(n, MI_NGY, MI_BLOCKS); }

static bool mi_sizes_ok(int n, int k) { return n >= 2 && k >= 1 && k <= SVAE_MI_MAX_K && k <= n - 1; }

extern "C" long long svae_mi_work(int n, int k) {
  if (!mi_sizes_ok(n, k)) return 0;
  return knn_work_bytes(mi_plan(n), k);
}

// the checks that svae_mi_radius and svae_mi_counts share
static int mi_check_rows(const char* what, const double* Z, int ld, int d, int n, const double* Y, int q, bool labels) {
  if (int e = check_pair_rows(what, Z, ld, d, n, 2)) return e;
  SVAE_REQUIRE((Y != nullptr) != labels, SVAE_ERR_ARG, "%s: exactly one of Y and the labels must be given", what);
  SVAE_REQUIRE(labels || (q >= 1 && q <= SVAE_MI_MAX_Y), SVAE_ERR_ARG, "%s: bad width of y (q=%d, at most %d)", what, q, SVAE_MI_MAX_Y);
  return SVAE_OK;
}

extern "C" int svae_mi_radius(const double* Z, int ld, int d, int n, const double* Y, int q, const int* lab, const int* kk, int k,
                              void* work, double* rho2, void* stream) {
  if (int e = mi_check_rows("mi_radius", Z, ld, d, n, Y, q, lab != nullptr)) return e;
  SVAE_REQUIRE(mi_sizes_ok(n, k), SVAE_ERR_ARG, "mi_radius: bad neighbour count (k=%d n=%d, at most %d)", k, n, SVAE_MI_MAX_K);
  SVAE_REQUIRE((kk != nullptr) == (lab != nullptr), SVAE_ERR_ARG, "mi_radius: kk belongs to the labels");
  SVAE_REQUIRE(work && rho2, SVAE_ERR_ARG, "mi_radius: null argument");
  const KnnPlan p = mi_plan(n);
  KnnLists l;
  if (int e = knn_work_lists("mi_radius", work, p, k, &l)) return e;
  if (lab) {
    static DeviceOnce once;
    if (int e = allow_lds(mi_radius_kernel<true>, once, (int)MI_RADIUS_LDS, "mi_radius")) return e;
    hipLaunchKernelGGL(mi_radius_kernel<true>, dim3(p.gx, p.gy), dim3(256), MI_RADIUS_LDS, ST(stream), Z, ld, d, n, Y, q, lab, kk, k, p.ch,
                       p.rpad, l.key, l.idx);
  } else {
    static DeviceOnce once;
    if (int e = allow_lds(mi_radius_kernel<false>, once, (int)MI_RADIUS_LDS, "mi_radius")) return e;
    hipLaunchKernelGGL(mi_radius_kernel<false>, dim3(p.gx, p.gy), dim3(256), MI_RADIUS_LDS, ST(stream), Z, ld, d, n, Y, q, lab, kk, k, p.ch,
                       p.rpad, l.key, l.idx);
  }
  if (int e = check_launch("mi_radius")) return e;
  const long long cells = (long long)n * k;
  hipLaunchKernelGGL(mi_finish_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, ST(stream), l.key, l.idx, (int)p.gy, p.rpad,
                     n, k, kk, rho2);
  return check_launch("mi_finish");
}

extern "C" int svae_mi_counts(const double* Z, int ld, int d, int n, const double* Y, int q, const double* rho2, int* nz, int* ny,
                              void* stream) {
  if (int e = mi_check_rows("mi_counts", Z, ld, d, n, Y, q, Y == nullptr)) return e;
  SVAE_REQUIRE((Y != nullptr) == (ny != nullptr), SVAE_ERR_ARG, "mi_counts: ny belongs to Y");
  SVAE_REQUIRE(rho2 && nz, SVAE_ERR_ARG, "mi_counts: null argument");
  const KnnPlan p = mi_plan(n);
  hipError_t err = hipMemsetAsync(nz, 0, (size_t)n * sizeof(int), ST(stream));
  if (err == hipSuccess && ny) err = hipMemsetAsync(ny, 0, (size_t)n * sizeof(int), ST(stream));
  SVAE_REQUIRE(err == hipSuccess, SVAE_ERR_LAUNCH, "mi_counts: hipMemsetAsync: %s", hipGetErrorString(err));
  if (Y)
    hipLaunchKernelGGL(mi_count_kernel<true>, dim3(p.gx, p.gy), dim3(256), MI_COUNT_LDS, ST(stream), Z, ld, d, n, Y, q, rho2, p.ch, nz, ny);
  else
    hipLaunchKernelGGL(mi_count_kernel<false>, dim3(p.gx, p.gy), dim3(256), MI_COUNT_LDS, ST(stream), Z, ld, d, n, Y, q, rho2, p.ch, nz, ny);
  return check_launch("mi_counts");
}

extern "C" int svae_mi_psi_sums(const int* a, const int* b, long long n, double* out, void* stream) {
  SVAE_REQUIRE(a && out && n >= 1, SVAE_ERR_ARG, "mi_psi_sums: bad args (n=%lld)", n);
  hipLaunchKernelGGL(mi_psi_sums_kernel, dim3(b ? 2 : 1), dim3(256), 0, ST(stream), a, b, n, out);
  return check_launch("mi_psi_sums");
}

// the checks that svae_cmi_radius and svae_cmi_counts share
static int cmi_check_rows(const char* what, const double* Z, int ld, int d, int n, const double* Y, int q, const double* C, int p,
                          const int* clab) {
  if (int e = check_pair_rows(what, Z, ld, d, n, 2)) return e;
  SVAE_REQUIRE(Y != nullptr, SVAE_ERR_ARG, "%s: null argument (Y)", what);
  SVAE_REQUIRE(q >= 1 && q <= SVAE_MI_MAX_Y, SVAE_ERR_ARG, "%s: bad width of y (q=%d, at most %d)", what, q, SVAE_MI_MAX_Y);
  SVAE_REQUIRE((C != nullptr) != (clab != nullptr), SVAE_ERR_ARG, "%s: exactly one of C and clab must be given", what);
  SVAE_REQUIRE(clab || (p >= 1 && p <= SVAE_CMI_MAX_C), SVAE_ERR_ARG, "%s: bad width of c (p=%d, at most %d)", what, p, SVAE_CMI_MAX_C);
  return SVAE_OK;
}

extern "C" int svae_cmi_radius(const double* Z, int ld, int d, int n, const double* Y, int q, const double* C, int p, const int* clab,
                               int k, void* work, double* rho2, void* stream) {
  if (int e = cmi_check_rows("cmi_radius", Z, ld, d, n, Y, q, C, p, clab)) return e;
  SVAE_REQUIRE(mi_sizes_ok(n, k), SVAE_ERR_ARG, "cmi_radius: bad neighbour count (k=%d n=%d, at most %d)", k, n, SVAE_MI_MAX_K);
  SVAE_REQUIRE(work && rho2, SVAE_ERR_ARG, "cmi_radius: null argument");
  const KnnPlan pl = mi_plan(n);
  KnnLists l;
  if (int e = knn_work_lists("cmi_radius", work, pl, k, &l)) return e;
  if (clab) {
    static DeviceOnce once;
    if (int e = allow_lds(cmi_radius_kernel<true>, once, (int)CMI_RADIUS_LDS, "cmi_radius")) return e;
    hipLaunchKernelGGL(cmi_radius_kernel<true>, dim3(pl.gx, pl.gy), dim3(256), CMI_RADIUS_LDS, ST(stream), Z, ld, d, n, Y, q, C, p, clab, k,
                       pl.ch, pl.rpad, l.key, l.idx);
  } else {
    static DeviceOnce once;
    if (int e = allow_lds(cmi_radius_kernel<false>, once, (int)CMI_RADIUS_LDS, "cmi_radius")) return e;
    hipLaunchKernelGGL(cmi_radius_kernel<false>, dim3(pl.gx, pl.gy), dim3(256), CMI_RADIUS_LDS, ST(stream), Z, ld, d, n, Y, q, C, p, clab, k,
                       pl.ch, pl.rpad, l.key, l.idx);
  }
  if (int e = check_launch("cmi_radius")) return e;
  const long long cells = (long long)n * k;
  hipLaunchKernelGGL(mi_finish_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, ST(stream), l.key, l.idx, (int)pl.gy, pl.rpad,
                     n, k, (const int*)nullptr, rho2);
  return check_launch("cmi_finish");
}

extern "C" int svae_cmi_counts(const double* Z, int ld, int d, int n, const double* Y, int q, const double* C, int p, const int* clab,
                               const double* rho2, int* nzc, int* nyc, int* nc, void* stream) {
  if (int e = cmi_check_rows("cmi_counts", Z, ld, d, n, Y, q, C, p, clab)) return e;
  SVAE_REQUIRE((C != nullptr) == (nc != nullptr), SVAE_ERR_ARG, "cmi_counts: nc belongs to C (with clab the class size is the host's)");
  SVAE_REQUIRE(rho2 && nzc && nyc, SVAE_ERR_ARG, "cmi_counts: null argument");
  const KnnPlan pl = mi_plan(n);
  hipError_t err = hipMemsetAsync(nzc, 0, (size_t)n * sizeof(int), ST(stream));
  if (err == hipSuccess) err = hipMemsetAsync(nyc, 0, (size_t)n * sizeof(int), ST(stream));
  if (err == hipSuccess && nc) err = hipMemsetAsync(nc, 0, (size_t)n * sizeof(int), ST(stream));
  SVAE_REQUIRE(err == hipSuccess, SVAE_ERR_LAUNCH, "cmi_counts: hipMemsetAsync: %s", hipGetErrorString(err));
  if (clab)
    hipLaunchKernelGGL(cmi_count_kernel<true>, dim3(pl.gx, pl.gy), dim3(256), CMI_COUNT_LDS, ST(stream), Z, ld, d, n, Y, q, C, p, clab, rho2,
                       pl.ch, nzc, nyc, nc);
  else
    hipLaunchKernelGGL(cmi_count_kernel<false>, dim3(pl.gx, pl.gy), dim3(256), CMI_COUNT_LDS, ST(stream), Z, ld, d, n, Y, q, C, p, clab, rho2,
                       pl.ch, nzc, nyc, nc);
  return check_launch("cmi_counts");
}

extern "C" int svae_local_permutations(const int* nbr, int n, int kp, const int* order, const unsigned char* scan, int P, int* out,
                                       void* stream) {
  SVAE_REQUIRE(nbr && order && scan && out, SVAE_ERR_ARG, "local_permutations: null argument");
  SVAE_REQUIRE(n >= 1 && n <= CMI_PERM_MAX_N, SVAE_ERR_ARG, "local_permutations: bad row count (n=%d, at most %d)", n, CMI_PERM_MAX_N);
  SVAE_REQUIRE(kp >= 1 && kp <= SVAE_CMI_MAX_DONORS, SVAE_ERR_ARG, "local_permutations: bad donor count (kp=%d, at most %d)", kp,
               SVAE_CMI_MAX_DONORS);
  SVAE_REQUIRE(P >= 1 && P <= SVAE_MMD_NULL_MAX, SVAE_ERR_ARG, "local_permutations: bad permutation count (P=%d, at most %d)", P,
               SVAE_MMD_NULL_MAX);
  const size_t lds = (size_t)((n + 31) / 32) * sizeof(unsigned);  // at most 64 KiB: the default dynamic LDS limit
  hipLaunchKernelGGL(cmi_local_perm_kernel, dim3((unsigned)P), dim3(64), lds, ST(stream), nbr, n, kp, order, scan, out);
  return check_launch("local_permutations");
}
