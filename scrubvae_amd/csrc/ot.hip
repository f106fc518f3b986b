// Entropic optimal transport between two sets of fp64 rows (Sinkhorn in the log domain), nothing of size m x n stored.  With s_ij
// the squared distance of pair_tiles.h between query row i of Q [m] and candidate row j of X [n], the cost is c_ij = s_ij (kind 0)
// or the correctly rounded sqrt(s_ij) (kind 1), and for a column offset vector u [n]
//     v_ij = u_j - c_ij * inv_eps                       (a product with the host's 1.0 / eps, not a division per pair)
// svae_ot_softmin: L_i = log sum_j exp(v_ij) and, when asked, cbar_i = (sum_j exp(v_ij) c_ij) / (sum_j exp(v_ij)): the streaming
// log-sum-exp a Sinkhorn sweep runs twice.  A block holds 64 rows (lane = row) and walks its column tiles; for every tile a thread
// takes the maximum of its 16 values and its running maximum M, rescales its running sum S (and the cost-weighted sum W) once by
// exp(M_old - M_new) and adds exp(v - M_new) for its candidates in ascending q.  (M, S, W) of a thread, wave or chunk that saw no
// candidate is (-inf, 0, 0) and merges without a NaN.  The merge M = max, S = S1 exp(M1 - M) + S2 exp(M2 - M) runs in a fixed
// order: the four waves ((w0, w1), w2), w3 in the block, then the column chunks in chunk order in the finish kernel, which closes
// with L = M + log(S).  The chunks are chunk_split's (row tiles counted from m, column tiles from n): the order is a function of
// (m, n) alone, so every result is bit-reproducible.  No cross-lane sums, no floating-point atomics.
// svae_ot_apply: out_i = sum_j exp(v_ij - L_i) V_j, the row-normalised plan times the c columns of V, silhouette.hip's pattern: the
// 64 x 64 tile of weights goes to LDS column-major as the A operand, V's rows of the tile are staged next to it, and the fp64
// matrix cores (v_mfma_f64_16x16x4_f64) multiply them; per-chunk partials are added in chunk order.  It runs once or twice per
// solve, so it is written for clarity, not tuned.
#include "svae_internal.h"

#include <cmath>

#include "knn_buffer.h"  // pair_tiles.h (#pragma clang fp contract(off)) and the row-tile x column-chunk plan

namespace svae {

constexpr int OT_NGY = 8;        // column chunks per row tile at most
constexpr int OT_BLOCKS = 512;   // grid y splits the column tiles only while the grid holds fewer blocks than this

// ---- softmin -----------------------------------------------------------------------------------------------------------------------
// static LDS, in doubles: the rows and candidates of pair_tiles.h, u of two tiles (written for tile t while tile t - 1 may still be
// read), the four waves' (M, S, W)
constexpr int O_US = PAIR_LDS_KT;
constexpr int O_RED = O_US + 2 * HT;
constexpr int O_END = O_RED + 3 * 4 * HR;
static_assert((size_t)O_END * sizeof(double) <= 64 * 1024, "static LDS per workgroup");

struct OtAcc {
  double M, S, W;
};

// (M, S, W) of two disjoint sets of candidates -> of their union; a side that saw none is (-inf, 0, 0): exp(-inf) = 0, no NaN
__device__ __forceinline__ OtAcc ot_merge(const OtAcc a, const OtAcc b) {
  const double M = fmax(a.M, b.M);
  if (!(M > -INFINITY)) return OtAcc{-INFINITY, 0.0, 0.0};
  const double ea = exp(a.M - M), eb = exp(b.M - M);
  const double sa = a.S * ea, sb = b.S * eb;
  const double wa = a.W * ea, wb = b.W * eb;
  return OtAcc{M, sa + sb, wa + wb};
}

template <int KIND>
__device__ __forceinline__ double ot_cost(double s) {
  return KIND ? sqrt(s) : s;
}

// part: three planes [gy][rpad] of M, S, W (W only with CBAR): the block's rows against the column tiles of chunk y
template <int KIND, bool CBAR>
__global__ __launch_bounds__(256) void ot_softmin_kernel(const double* __restrict__ Q, int ldq, int m, const double* __restrict__ X,
                                                         int ldx, int n, int d, const double* __restrict__ u, double inv_eps, int ch,
                                                         long long rpad, double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) double lds[O_END];
  double* us = lds + O_US;
  double* red = lds + O_RED;
  const PairTileRange tr = pair_chunk_tiles(n, ch);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const PairRows rows = pair_rows(Q, ldq, d, m, tr.r0, lds + PAIR_LDS_QS, lds + PAIR_LDS_CS, X, ldx, n);
  double M = -INFINITY, S = 0.0, W = 0.0;
  for (int ct = tr.t_lo; ct < tr.t_hi; ++ct) {
    const long long c0 = (long long)ct * HT;
    double* ut = us + (ct & 1) * HT;  // the reads of tile ct - 2 ended before the barriers of tile ct - 1
    if (threadIdx.x < HT) ut[threadIdx.x] = c0 + threadIdx.x < n ? u[c0 + threadIdx.x] : -INFINITY;  // past n: v = -inf, exp = 0
    double s[HQ];
    pair_tile(rows, c0, s);  // its barriers publish ut
    double v[HQ], c[HQ];
    double tmax = -INFINITY;
#pragma unroll
    for (int q = 0; q < HQ; ++q) {
      c[q] = ot_cost<KIND>(s[q]);
      const double p = c[q] * inv_eps;
      v[q] = ut[wave * HQ + q] - p;
      tmax = fmax(tmax, v[q]);
    }
    const double Mn = fmax(M, tmax);
    if (Mn > -INFINITY) {  // else the thread has seen no candidate yet
      const double r = exp(M - Mn);  // exp(-inf) = 0 at the first candidates, exp(0) = 1 when the maximum stays
      S = S * r;
      if (CBAR) W = W * r;
      M = Mn;
#pragma unroll
      for (int q = 0; q < HQ; ++q) {
        const double e = exp(v[q] - M);
        S = S + e;
        if (CBAR) {
          const double w = e * c[q];
          W = W + w;
        }
      }
    }
  }
  red[(0 * 4 + wave) * HR + lane] = M;
  red[(1 * 4 + wave) * HR + lane] = S;
  red[(2 * 4 + wave) * HR + lane] = W;
  __syncthreads();
  if (wave != 0) return;
  OtAcc a{red[lane], red[4 * HR + lane], red[8 * HR + lane]};
#pragma unroll
  for (int w = 1; w < 4; ++w) a = ot_merge(a, OtAcc{red[w * HR + lane], red[(4 + w) * HR + lane], red[(8 + w) * HR + lane]});
  const long long plane = (long long)gridDim.y * rpad;
  const long long at = (long long)blockIdx.y * rpad + tr.r0 + lane;  // rows past m hold zeros: finite values nobody reads
  part[at] = a.M;
  part[plane + at] = a.S;
  if (CBAR) part[2 * plane + at] = a.W;
}

// one thread per row: the chunks in chunk order, then L = M + log(S) and cbar = W / S
__global__ __launch_bounds__(256) void ot_softmin_finish_kernel(const double* __restrict__ part, int gy, long long rpad, int m,
                                                                double* __restrict__ L, double* __restrict__ cbar) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= m) return;
  const long long plane = (long long)gy * rpad;
  OtAcc a{part[r], part[plane + r], cbar ? part[2 * plane + r] : 0.0};
  for (int y = 1; y < gy; ++y) {
    const long long at = (long long)y * rpad + r;
    a = ot_merge(a, OtAcc{part[at], part[plane + at], cbar ? part[2 * plane + at] : 0.0});
  }
  L[r] = a.M + log(a.S);
  if (cbar) cbar[r] = a.W / a.S;
}

// ---- apply -------------------------------------------------------------------------------------------------------------------------
// dynamic LDS, in doubles, after the prefix of pair_tiles.h; kt holds the tile of weights, vs [64][NC] the tile's rows of V
constexpr int A_VS = PAIR_LDS_END;
constexpr size_t ot_apply_lds(int nc) { return (size_t)(A_VS + HT * nc) * sizeof(double); }
static_assert(ot_apply_lds(SVAE_OT_MAX_COLS) <= 160 * 1024, "LDS per workgroup");

// part[(y * rpad + row) * NC + col]: the sum over the column tiles of chunk y of exp(v - L[row]) V[j][col]
template <int KIND, int NC>
__global__ __launch_bounds__(256) void ot_apply_kernel(const double* __restrict__ Q, int ldq, int m, const double* __restrict__ X, int ldx,
                                                       int n, int d, const double* __restrict__ u, double inv_eps,
                                                       const double* __restrict__ L, const double* __restrict__ V, int ldv, int c, int ch,
                                                       long long rpad, double* __restrict__ part) {
  constexpr int NT = NC / 16;  // 16 x 16 result tiles per wave: 4 fp64 accumulators per lane each
  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* kt = lds + PAIR_LDS_KT;
  double* vs = lds + A_VS;
  const PairTileRange tr = pair_chunk_tiles(n, ch);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l16 = lane & 15, kg = lane >> 4;
  const PairRows rows = pair_rows(Q, ldq, d, m, tr.r0, lds + PAIR_LDS_QS, lds + PAIR_LDS_CS, X, ldx, n);
  const bool ok = tr.r0 + lane < m;
  const double Li = ok ? L[tr.r0 + lane] : 0.0;
  double4_t acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = double4_t{0.0, 0.0, 0.0, 0.0};
  for (int ct = tr.t_lo; ct < tr.t_hi; ++ct) {
    const long long c0 = (long long)ct * HT;
    double s[HQ];
    pair_tile(rows, c0, s);  // its first barrier also ends the previous tile's reads of kt and vs
#pragma unroll
    for (int q = 0; q < HQ; ++q) {
      const long long j = c0 + wave * HQ + q;
      double w = 0.0;  // rows past m and candidates past n weigh nothing
      if (ok && j < n) {
        const double p = ot_cost<KIND>(s[q]) * inv_eps;
        const double v = u[j] - p;
        w = exp(v - Li);
      }
      pair_kt_value(kt, lane, wave, q) = w;
    }
    for (int e = threadIdx.x; e < HT * NC; e += 256) {
      const int j = e / NC, col = e - j * NC;
      vs[e] = c0 + j < n && col < c ? V[(c0 + j) * ldv + col] : 0.0;
    }
    __syncthreads();
    // wave w: rows [16 w, 16 w + 16) of the tile x all NC columns (lane layouts: pair_tiles.h)
#pragma unroll 2
    for (int ks = 0; ks < HT / 4; ++ks) {
      const int j = 4 * ks + kg;
      const double a = pair_kt_a(kt, j, wave, l16);
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, vs[j * NC + 16 * t + l16], acc[t], 0, 0, 0);
    }
  }
  // acc[t][r] is [row (l >> 4) + 4 r][col l & 15] of result tile t
  double* out = part + ((long long)blockIdx.y * rpad + tr.r0 + 16 * wave + kg) * NC + l16;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) out[(long long)(4 * r) * NC + 16 * t] = acc[t][r];
}

// one thread per (row, column): the chunks' partials in chunk order
__global__ __launch_bounds__(256) void ot_apply_finish_kernel(const double* __restrict__ part, int gy, long long rpad, int nc, int m, int c,
                                                              double* __restrict__ out, int ldo) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= (long long)m * c) return;
  const long long row = g / c;
  const int col = (int)(g - row * c);
  double sum = 0.0;
  for (int y = 0; y < gy; ++y) sum = sum + part[((long long)y * rpad + row) * nc + col];
  out[row * ldo + col] = sum;
}

}  // namespace svae

using namespace svae;

// the row tiles counted from the m query rows and the column tiles from the n candidates
static KnnPlan ot_plan(int m, int n) { return knn_plan(m, n, OT_NGY, OT_BLOCKS); }
static bool ot_sizes_ok(int m, int n) { return m >= 1 && m < (1 << 26) && n >= 1 && n < (1 << 26); }
static int ot_apply_cols(int c) { return c <= 16 ? 16 : c <= 64 ? 64 : SVAE_OT_MAX_COLS; }

static int ot_check(const char* what, const double* Q, int ldq, int m, const double* X, int ldx, int n, int d, const double* u,
                    double inv_eps, int kind) {
  if (int e = check_pair_rows(what, Q, ldq, d, m, 1, (1 << 26) - 1)) return e;
  if (int e = check_pair_rows(what, X, ldx, d, n, 1, (1 << 26) - 1)) return e;
  SVAE_REQUIRE(u && std::isfinite(inv_eps) && inv_eps > 0.0, SVAE_ERR_ARG, "%s: bad offsets or inv_eps (%g)", what, inv_eps);
  SVAE_REQUIRE(kind == 0 || kind == 1, SVAE_ERR_ARG, "%s: kind must be 0 (squared Euclidean) or 1 (Euclidean), got %d", what, kind);
  return SVAE_OK;
}

extern "C" long long svae_ot_softmin_work(int m, int n) {
  if (!ot_sizes_ok(m, n)) return 0;
  const KnnPlan p = ot_plan(m, n);
  return 3ll * p.gy * p.rpad;
}

template <int KIND, bool CBAR>
static void ot_launch_softmin(const KnnPlan& p, const double* Q, int ldq, int m, const double* X, int ldx, int n, int d, const double* u,
                              double inv_eps, double* work, hipStream_t st) {
  hipLaunchKernelGGL((ot_softmin_kernel<KIND, CBAR>), dim3(p.gx, p.gy), dim3(256), 0, st, Q, ldq, m, X, ldx, n, d, u, inv_eps, p.ch, p.rpad,
                     work);
}

extern "C" int svae_ot_softmin(const double* Q, int ldq, int m, const double* X, int ldx, int n, int d, const double* u, double inv_eps,
                               int kind, double* work, double* L, double* cbar, void* stream) {
  if (int e = ot_check("ot_softmin", Q, ldq, m, X, ldx, n, d, u, inv_eps, kind)) return e;
  SVAE_REQUIRE(work && L, SVAE_ERR_ARG, "ot_softmin: null argument");
  const KnnPlan p = ot_plan(m, n);
  if (kind == 0 && !cbar) ot_launch_softmin<0, false>(p, Q, ldq, m, X, ldx, n, d, u, inv_eps, work, ST(stream));
  else if (kind == 0) ot_launch_softmin<0, true>(p, Q, ldq, m, X, ldx, n, d, u, inv_eps, work, ST(stream));
  else if (!cbar) ot_launch_softmin<1, false>(p, Q, ldq, m, X, ldx, n, d, u, inv_eps, work, ST(stream));
  else ot_launch_softmin<1, true>(p, Q, ldq, m, X, ldx, n, d, u, inv_eps, work, ST(stream));
  if (int e = check_launch("ot_softmin")) return e;
  hipLaunchKernelGGL(ot_softmin_finish_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, ST(stream), work, (int)p.gy, p.rpad, m, L,
                     cbar);
  return check_launch("ot_softmin_finish");
}

extern "C" long long svae_ot_apply_work(int m, int n, int c) {
  if (!ot_sizes_ok(m, n) || c < 1 || c > SVAE_OT_MAX_COLS) return 0;
  const KnnPlan p = ot_plan(m, n);
  return (long long)p.gy * p.rpad * ot_apply_cols(c);
}

template <int KIND, int NC>
static int ot_launch_apply(const KnnPlan& p, const double* Q, int ldq, int m, const double* X, int ldx, int n, int d, const double* u,
                           double inv_eps, const double* L, const double* V, int ldv, int c, double* work, hipStream_t st) {
  static DeviceOnce once;
  if (int e = allow_lds(ot_apply_kernel<KIND, NC>, once, (int)ot_apply_lds(NC), "ot_apply")) return e;
  hipLaunchKernelGGL((ot_apply_kernel<KIND, NC>), dim3(p.gx, p.gy), dim3(256), ot_apply_lds(NC), st, Q, ldq, m, X, ldx, n, d, u, inv_eps, L, V,
                     ldv, c, p.ch, p.rpad, work);
  return check_launch("ot_apply");
}

template <int KIND>
static int ot_apply_kind(int nc, const KnnPlan& p, const double* Q, int ldq, int m, const double* X, int ldx, int n, int d, const double* u,
                         double inv_eps, const double* L, const double* V, int ldv, int c, double* work, hipStream_t st) {
  if (nc == 16) return ot_launch_apply<KIND, 16>(p, Q, ldq, m, X, ldx, n, d, u, inv_eps, L, V, ldv, c, work, st);
  if (nc == 64) return ot_launch_apply<KIND, 64>(p, Q, ldq, m, X, ldx, n, d, u, inv_eps, L, V, ldv, c, work, st);
  return ot_launch_apply<KIND, SVAE_OT_MAX_COLS>(p, Q, ldq, m, X, ldx, n, d, u, inv_eps, L, V, ldv, c, work, st);
}

extern "C" int svae_ot_apply(const double* Q, int ldq, int m, const double* X, int ldx, int n, int d, const double* u, double inv_eps,
                             int kind, const double* L, const double* V, int ldv, int c, double* work, double* out, int ldo,
                             void* stream) {
  if (int e = ot_check("ot_apply", Q, ldq, m, X, ldx, n, d, u, inv_eps, kind)) return e;
  SVAE_REQUIRE(c >= 1 && c <= SVAE_OT_MAX_COLS && ldv >= c && ldo >= c, SVAE_ERR_ARG, "ot_apply: bad columns (c=%d ldv=%d ldo=%d, at most %d)",
               c, ldv, ldo, SVAE_OT_MAX_COLS);
  SVAE_REQUIRE(L && V && work && out, SVAE_ERR_ARG, "ot_apply: null argument");
  const KnnPlan p = ot_plan(m, n);
  const int nc = ot_apply_cols(c);
  const int e = kind == 0 ? ot_apply_kind<0>(nc, p, Q, ldq, m, X, ldx, n, d, u, inv_eps, L, V, ldv, c, work, ST(stream))
                          : ot_apply_kind<1>(nc, p, Q, ldq, m, X, ldx, n, d, u, inv_eps, L, V, ldv, c, work, ST(stream));
  if (e) return e;
  const long long cells = (long long)m * c;
  hipLaunchKernelGGL(ot_apply_finish_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, ST(stream), work, (int)p.gy, p.rpad, nc, m, c,
                     out, ldo);
  return check_launch("ot_apply_finish");
}
