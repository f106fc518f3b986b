// t-SNE of fp64 rows on their exact kNN graph: sklearn's TSNE with an exact gradient (scrubvae_amd/eval/embed.py).
//   tsne_search_kernel      the perplexity search of every row's k neighbour distances (sklearn's _binary_search_perplexity)
//   tsne_repulsion_kernel   the hot path: for every row the sums over ALL other rows of q^2 (y_i - y_j) and of q,
//                           q = 1 / (1 + |y_i - y_j|^2); the full square, not the triangle, so a row's sums have one owner and one
//                           order.  At d = 2 pair_tiles.h's 16-feature staging would be all padding: a thread keeps its row's
//                           (y0, y1) in registers and every lane reads the same candidate from LDS (a broadcast).
//   tsne_step_kernel        per row the attraction and KL part over its CSR entries in stored order, gradient, gains, update;
//   tsne_move_kernel        Y += update in a launch of its own, so that no row sees a neighbour's new position.
// Placing new rows on a fitted map (scrubvae_amd/eval/embed_transform.py): every query is a 2-D optimisation of its own in the
// field of the fixed map points.
//   tsne_repulsion_kernel<true>   the same sums for m queries over all n map points, none left out: m x n pairs;
//   tsne_place_kernel             per query the attraction to its k reference neighbours, its own KL term, the gradient with the
//                                 query's own normaliser rowq, an optional clip of its norm, gains, update and the move.
// Everything is fp64 with contraction off: each subtract, multiply, add and divide is rounded on its own, the division
// correctly.  No floating-point atomics, no cross-lane sums whose order depends on the schedule: every result is bit-reproducible
// for a given (n, chunks).
#include "svae_internal.h"

#include <algorithm>
#include <cmath>

#include "fixed_sum.h"  // the closing sums

#pragma clang fp contract(off)

namespace svae {

constexpr int TS_ROWS = 256;     // rows per repulsion block: one per thread
constexpr int TS_CT = 64;        // the column split counts tiles of this many columns
constexpr int TS_BLOCKS = 512;   // chunks = 0 splits the columns only while the grid holds fewer blocks than this
constexpr int TS_SR = 64;        // rows per search block: one per lane of its single wave
constexpr int TS_NMAX = 1 << 26;

// One row per lane; the block's distances sit in LDS transposed ([neighbour][row]: conflict-free, staged with coalesced reads).
// The k values of P are not kept: the last pass recomputes exp(-d2 beta) at the beta they belong to, which gives the same bits.
__global__ __launch_bounds__(TS_SR) void tsne_search_kernel(const double* __restrict__ d2, int k, int n, double want, double* __restrict__ P,
                                                            double* __restrict__ beta_out) {
  extern __shared__ __attribute__((aligned(16))) double sd[];
  const long long r0 = (long long)blockIdx.x * TS_SR;
  const int lane = threadIdx.x;
  const int rows = (int)std::min<long long>(TS_SR, n - r0);
  for (int e = lane; e < rows * k; e += TS_SR) {
    const int r = e / k, j = e - r * k;
    sd[j * TS_SR + r] = d2[r0 * k + e];
  }
  __syncthreads();
  if (lane >= rows) return;
  double beta = 1.0, lo = -INFINITY, hi = INFINITY, used = 1.0, sum = 1.0;
  for (int step = 0; step < SVAE_TSNE_SEARCH_STEPS; ++step) {
    used = beta;
    sum = 0.0;
    double sdp = 0.0;
    for (int j = 0; j < k; ++j) {
      const double dd = sd[j * TS_SR + lane];
      const double p = exp(-dd * beta);
      sum = sum + p;
      sdp = sdp + dd * p;
    }
    if (sum == 0.0) sum = 1e-8;
    const double diff = (log(sum) + beta * sdp / sum) - want;
    if (fabs(diff) <= 1e-5) break;
    if (diff > 0.0) {
      lo = beta;
      beta = hi == INFINITY ? beta * 2.0 : (beta + hi) / 2.0;
    } else {
      hi = beta;
      beta = lo == -INFINITY ? beta / 2.0 : (beta + lo) / 2.0;
    }
  }
  double* out = P + (r0 + lane) * k;
  for (int j = 0; j < k; ++j) out[j] = exp(-sd[j * TS_SR + lane] * used) / sum;
  beta_out[r0 + lane] = beta;
}

// part[(y * 3 + c) * rpad + i]: the sums of row i over the columns [y ch 64, (y + 1) ch 64) in ascending j; c = 0, 1: q^2 d, 2: q.
// CROSS: the rows are the m queries Y and the columns the nc points of Yc, none left out (svae_tsne_cross_repulsion); otherwise
// the columns are Y's own rows and (Yc, nc) are not read.
template <bool CROSS>
__global__ __launch_bounds__(TS_ROWS) void tsne_repulsion_kernel(const double* __restrict__ Y, int n, const double* __restrict__ Yc, int nc,
                                                                 int ch, long long rpad, double* __restrict__ part) {
  __shared__ double2 cs[TS_ROWS];
  const int i = (int)blockIdx.x * TS_ROWS + (int)threadIdx.x;  // < rpad <= 2^26 + 255
  const int ii = min(i, n - 1);
  const double yi0 = Y[2 * (long long)ii], yi1 = Y[2 * (long long)ii + 1];
  const double* __restrict__ C = CROSS ? Yc : Y;
  const int cols = CROSS ? nc : n;
  const int c_lo = (int)std::min<long long>(cols, (long long)blockIdx.y * ch * TS_CT);
  const int c_hi = (int)std::min<long long>(cols, ((long long)blockIdx.y + 1) * ch * TS_CT);
  double r0 = 0.0, r1 = 0.0, sq = 0.0;
  for (int c0 = c_lo; c0 < c_hi; c0 += TS_ROWS) {
    const int cnt = min(TS_ROWS, c_hi - c0);
    __syncthreads();  // the previous stage's reads are done
    if ((int)threadIdx.x < cnt) {
      const long long j = c0 + (int)threadIdx.x;
      cs[threadIdx.x] = make_double2(C[2 * j], C[2 * j + 1]);
    }
    __syncthreads();
    const int self = i - c0;  // the row's own position in this stage, if it is in it
#pragma unroll 4
    for (int t = 0; t < cnt; ++t) {
      const double2 c = cs[t];
      const double d0 = yi0 - c.x, d1 = yi1 - c.y;
      double q = 1.0 / (1.0 + (d0 * d0 + d1 * d1));
      if (!CROSS) q = t == self ? 0.0 : q;  // left out by index: adds +0 to the three sums
      const double qq = q * q;
      r0 = r0 + qq * d0;
      r1 = r1 + qq * d1;
      sq = sq + q;
    }
  }
  double* out = part + (long long)blockIdx.y * 3 * rpad + i;
  out[0] = r0;
  out[rpad] = r1;
  out[2 * rpad] = sq;
}

__global__ __launch_bounds__(256) void tsne_repulsion_finish_kernel(const double* __restrict__ part, int gy, long long rpad, int n,
                                                                    double* __restrict__ R, double* __restrict__ rowq) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double s[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double a = 0.0;
    for (int y = 0; y < gy; ++y) a = a + part[((long long)y * 3 + c) * rpad + i];
    s[c] = a;
  }
  R[2 * i] = s[0];
  R[2 * i + 1] = s[1];
  rowq[i] = s[2];
}

// block b: out[b] = the sum of v_b [n] in the order of block_sum_of (fixed_sum.h)
__global__ __launch_bounds__(256) void tsne_sums_kernel(const double* __restrict__ a, const double* __restrict__ b, long long n,
                                                        double* __restrict__ out) {
  __shared__ double red[256];
  const double sum = block_sum_of<256>(blockIdx.x == 0 ? a : b, n, red);
  if (threadIdx.x == 0) out[blockIdx.x] = sum;
}

// One row per thread: the row's entries in stored order.  Reads Y, writes update and gains (the row's own) only.
__global__ __launch_bounds__(256) void tsne_step_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                        const double* __restrict__ val, double exag, const double* __restrict__ Y,
                                                        const double* __restrict__ R, const double* __restrict__ Zp,
                                                        double* __restrict__ update, double* __restrict__ gains, double momentum, double lr,
                                                        int n, double* __restrict__ klpart, double* __restrict__ gradsq) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double yi0 = Y[2 * i], yi1 = Y[2 * i + 1];
  const bool want_kl = klpart != nullptr;
  double a0 = 0.0, a1 = 0.0, kl = 0.0;
  for (int e = rowptr[i], end = rowptr[i + 1]; e < end; ++e) {
    const long long j = col[e];
    const double v = val[e];
    const double d0 = yi0 - Y[2 * j], d1 = yi1 - Y[2 * j + 1];
    const double w = 1.0 + (d0 * d0 + d1 * d1);
    const double pq = v * (1.0 / w);
    a0 = a0 + pq * d0;
    a1 = a1 + pq * d1;
    if (want_kl) {
      const double p = exag * v;
      kl = kl + (p > 0.0 ? p * log(p * w) : 0.0);  // an entry that underflowed to 0 adds nothing, as its limit
    }
  }
  const double Z = Zp[0];
  double g[2] = {4.0 * (exag * a0 - R[2 * i] / Z), 4.0 * (exag * a1 - R[2 * i + 1] / Z)};
  if (update) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const double u = update[2 * i + c];
      double gn = gains[2 * i + c];
      gn = u * g[c] < 0.0 ? gn + 0.2 : gn * 0.8;
      gn = fmax(gn, 0.01);
      g[c] = g[c] * gn;
      gains[2 * i + c] = gn;
      update[2 * i + c] = momentum * u - lr * g[c];
    }
  }
  if (want_kl) klpart[i] = kl;
  if (gradsq) gradsq[i] = g[0] * g[0] + g[1] * g[1];
}

__global__ __launch_bounds__(256) void tsne_move_kernel(double* __restrict__ Y, const double* __restrict__ update, long long count) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e < count) Y[e] = Y[e] + update[e];
}

// One query per thread against the fixed map: its k neighbours idx / P [m][k] in stored order, R and rowq from the cross
// repulsion.  A thread reads Yref and its own row of everything else, and writes only its own row: the move needs no launch of
// its own.
__global__ __launch_bounds__(256) void tsne_place_kernel(const int* __restrict__ idx, const double* __restrict__ P, int k, double exag,
                                                         double* __restrict__ Yq, const double* __restrict__ Yref,
                                                         const double* __restrict__ R, const double* __restrict__ rowq,
                                                         double* __restrict__ update, double* __restrict__ gains, double momentum, double lr,
                                                         double max_grad_norm, int m, double* __restrict__ klrow,
                                                         double* __restrict__ gradsq) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const double yi0 = Yq[2 * i], yi1 = Yq[2 * i + 1];
  const bool want_kl = klrow != nullptr;
  double a0 = 0.0, a1 = 0.0, kl = 0.0;
  for (long long e = i * k, end = e + k; e < end; ++e) {
    const long long j = idx[e];
    const double v = P[e];
    const double d0 = yi0 - Yref[2 * j], d1 = yi1 - Yref[2 * j + 1];
    const double w = 1.0 + (d0 * d0 + d1 * d1);
    const double pq = v * (1.0 / w);
    a0 = a0 + pq * d0;
    a1 = a1 + pq * d1;
    if (want_kl) {
      const double p = exag * v;
      kl = kl + (p > 0.0 ? p * log(p * w) : 0.0);  // an entry that underflowed to 0 adds nothing, as its limit
    }
  }
  const double zq = rowq[i];
  double g[2] = {2.0 * (exag * a0 - R[2 * i] / zq), 2.0 * (exag * a1 - R[2 * i + 1] / zq)};
  if (max_grad_norm > 0.0) {
    const double norm = sqrt(g[0] * g[0] + g[1] * g[1]);
    if (norm > max_grad_norm) {
      const double s = max_grad_norm / norm;
      g[0] = g[0] * s;
      g[1] = g[1] * s;
    }
  }
  if (update) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const double u = update[2 * i + c];
      double gn = gains[2 * i + c];
      gn = u * g[c] < 0.0 ? gn + 0.2 : gn * 0.8;
      gn = fmax(gn, 0.01);
      g[c] = g[c] * gn;
      gains[2 * i + c] = gn;
      const double un = momentum * u - lr * g[c];
      update[2 * i + c] = un;
      Yq[2 * i + c] = (c == 0 ? yi0 : yi1) + un;
    }
  }
  if (want_kl) klrow[i] = kl + log(zq);
  if (gradsq) gradsq[i] = g[0] * g[0] + g[1] * g[1];
}

}  // namespace svae

using namespace svae;

struct TsnePlan {
  int ch;  // 64-column tiles per chunk
  unsigned gx, gy;
  long long rpad;
};

static bool tsne_sizes_ok(int n, int chunks) { return n >= 2 && n <= TS_NMAX && chunks >= 0 && chunks <= SVAE_TSNE_MAX_CHUNKS; }

static TsnePlan tsne_plan(int n, int chunks) {
  TsnePlan p;
  p.gx = (unsigned)((n + TS_ROWS - 1) / TS_ROWS);
  const int nt = (n + TS_CT - 1) / TS_CT;
  const ChunkSplit s = chunks > 0 ? chunk_split_into(nt, std::min(chunks, nt)) : chunk_split(nt, p.gx, SVAE_TSNE_MAX_CHUNKS, TS_BLOCKS);
  p.ch = s.per;
  p.gy = (unsigned)s.parts;
  p.rpad = (long long)p.gx * TS_ROWS;
  return p;
}

extern "C" int svae_tsne_search(const double* d2, int k, int n, double perplexity, double* P, double* beta, void* stream) {
  SVAE_REQUIRE(d2 && P && beta, SVAE_ERR_ARG, "tsne_search: null argument");
  SVAE_REQUIRE(n >= 1 && k >= 1 && k <= SVAE_KNN_MAX_K && perplexity > 0.0 && std::isfinite(perplexity), SVAE_ERR_ARG,
               "tsne_search: bad args (n=%d k=%d perplexity=%g)", n, k, perplexity);
  const unsigned blocks = (unsigned)(((long long)n + TS_SR - 1) / TS_SR);
  hipLaunchKernelGGL(tsne_search_kernel, dim3(blocks), dim3(TS_SR), (size_t)k * TS_SR * sizeof(double), ST(stream), d2, k, n,
                     std::log(perplexity), P, beta);
  return check_launch("tsne_search");
}

extern "C" long long svae_tsne_repulsion_work(int n, int chunks) {
  if (!tsne_sizes_ok(n, chunks)) return 0;
  const TsnePlan p = tsne_plan(n, chunks);
  return (long long)p.gy * 3 * p.rpad;
}

extern "C" int svae_tsne_repulsion(const double* Y, int n, int chunks, double* work, double* R, double* rowq, double* Z, void* stream) {
  SVAE_REQUIRE(tsne_sizes_ok(n, chunks), SVAE_ERR_ARG, "tsne_repulsion: bad args (n=%d chunks=%d)", n, chunks);
  SVAE_REQUIRE(Y && work && R && rowq && Z, SVAE_ERR_ARG, "tsne_repulsion: null argument");
  const TsnePlan p = tsne_plan(n, chunks);
  hipLaunchKernelGGL(tsne_repulsion_kernel<false>, dim3(p.gx, p.gy), dim3(TS_ROWS), 0, ST(stream), Y, n, (const double*)nullptr, 0, p.ch, p.rpad,
                     work);
  if (int e = check_launch("tsne_repulsion")) return e;
  hipLaunchKernelGGL(tsne_repulsion_finish_kernel, dim3(p.gx), dim3(256), 0, ST(stream), work, (int)p.gy, p.rpad, n, R, rowq);
  if (int e = check_launch("tsne_repulsion_finish")) return e;
  hipLaunchKernelGGL(tsne_sums_kernel, dim3(1), dim3(256), 0, ST(stream), rowq, (const double*)nullptr, (long long)n, Z);
  return check_launch("tsne_repulsion_z");
}

extern "C" int svae_tsne_step(const int* rowptr, const int* col, const double* val, double exag, double* Y, const double* R, const double* Z,
                              double* update, double* gains, double momentum, double lr, int n, double* klpart, double* gradsq,
                              void* stream) {
  SVAE_REQUIRE(n >= 2 && n <= TS_NMAX, SVAE_ERR_ARG, "tsne_step: bad row count (n=%d)", n);
  SVAE_REQUIRE(rowptr && col && val && Y && R && Z, SVAE_ERR_ARG, "tsne_step: null argument");
  SVAE_REQUIRE((update != nullptr) == (gains != nullptr), SVAE_ERR_ARG, "tsne_step: update and gains go together");
  SVAE_REQUIRE(update || klpart || gradsq, SVAE_ERR_ARG, "tsne_step: nothing to do");
  const unsigned blocks = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(tsne_step_kernel, dim3(blocks), dim3(256), 0, ST(stream), rowptr, col, val, exag, Y, R, Z, update, gains, momentum, lr, n,
                     klpart, gradsq);
  if (int e = check_launch("tsne_step")) return e;
  if (!update) return SVAE_OK;
  hipLaunchKernelGGL(tsne_move_kernel, dim3((unsigned)((2ll * n + 255) / 256)), dim3(256), 0, ST(stream), Y, update, 2ll * n);
  return check_launch("tsne_move");
}

static bool tsne_cross_sizes_ok(int m, int n, int chunks) {
  return m >= 1 && m <= TS_NMAX && n >= 1 && n <= TS_NMAX && chunks >= 0 && chunks <= SVAE_TSNE_MAX_CHUNKS;
}

// The rows come from m, the column split from n alone: chunks = 0 takes the most chunks there are, min(8, tiles), whatever m is, so a
// query's chunk boundaries, and with them its bits, do not depend on how many other queries share the launch.  (A rule that looked
// at the grid would; and measured, a grid of 391 x 2 blocks keeps 3 waves per SIMD busy and runs at two thirds of the rate of a
// full one, while the partials of 8 chunks cost 192 B per query next to n pairs.)
static TsnePlan tsne_cross_plan(int m, int n, int chunks) {
  TsnePlan p = tsne_plan(n, chunks > 0 ? chunks : SVAE_TSNE_MAX_CHUNKS);
  p.gx = (unsigned)((m + TS_ROWS - 1) / TS_ROWS);
  p.rpad = (long long)p.gx * TS_ROWS;
  return p;
}

extern "C" long long svae_tsne_cross_repulsion_work(int m, int n, int chunks) {
  if (!tsne_cross_sizes_ok(m, n, chunks)) return 0;
  const TsnePlan p = tsne_cross_plan(m, n, chunks);
  return (long long)p.gy * 3 * p.rpad;
}

extern "C" int svae_tsne_cross_repulsion(const double* Yq, int m, const double* Yref, int n, int chunks, double* work, double* R,
                                         double* rowq, void* stream) {
  SVAE_REQUIRE(tsne_cross_sizes_ok(m, n, chunks), SVAE_ERR_ARG, "tsne_cross_repulsion: bad args (m=%d n=%d chunks=%d)", m, n, chunks);
  SVAE_REQUIRE(Yq && Yref && work && R && rowq, SVAE_ERR_ARG, "tsne_cross_repulsion: null argument");
  const uintptr_t q0 = reinterpret_cast<uintptr_t>(Yq), r0 = reinterpret_cast<uintptr_t>(Yref);
  SVAE_REQUIRE(q0 + 16ull * m <= r0 || r0 + 16ull * n <= q0, SVAE_ERR_ARG, "tsne_cross_repulsion: Yq and Yref overlap");
  const TsnePlan p = tsne_cross_plan(m, n, chunks);
  hipLaunchKernelGGL(tsne_repulsion_kernel<true>, dim3(p.gx, p.gy), dim3(TS_ROWS), 0, ST(stream), Yq, m, Yref, n, p.ch, p.rpad, work);
  if (int e = check_launch("tsne_cross_repulsion")) return e;
  hipLaunchKernelGGL(tsne_repulsion_finish_kernel, dim3(p.gx), dim3(256), 0, ST(stream), work, (int)p.gy, p.rpad, m, R, rowq);
  return check_launch("tsne_cross_repulsion_finish");
}

extern "C" int svae_tsne_place_step(const int* idx, const double* P, int k, double exag, double* Yq, const double* Yref, const double* R,
                                    const double* rowq, double* update, double* gains, double momentum, double lr, double max_grad_norm,
                                    int m, double* klrow, double* gradsq, void* stream) {
  SVAE_REQUIRE(m >= 1 && m <= TS_NMAX && k >= 1 && k <= SVAE_KNN_MAX_K, SVAE_ERR_ARG, "tsne_place_step: bad sizes (m=%d k=%d)", m, k);
  SVAE_REQUIRE(idx && P && Yq && Yref && R && rowq, SVAE_ERR_ARG, "tsne_place_step: null argument");
  SVAE_REQUIRE((update != nullptr) == (gains != nullptr), SVAE_ERR_ARG, "tsne_place_step: update and gains go together");
  SVAE_REQUIRE(update || klrow || gradsq, SVAE_ERR_ARG, "tsne_place_step: nothing to do");
  SVAE_REQUIRE(max_grad_norm >= 0.0, SVAE_ERR_ARG, "tsne_place_step: max_grad_norm must be >= 0 (0: no clip), got %g", max_grad_norm);
  hipLaunchKernelGGL(tsne_place_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, ST(stream), idx, P, k, exag, Yq, Yref, R, rowq, update,
                     gains, momentum, lr, max_grad_norm, m, klrow, gradsq);
  return check_launch("tsne_place_step");
}

extern "C" int svae_tsne_sums(const double* a, const double* b, long long n, double* out, void* stream) {
  SVAE_REQUIRE(a && out && n >= 1, SVAE_ERR_ARG, "tsne_sums: bad args (n=%lld)", n);
  hipLaunchKernelGGL(tsne_sums_kernel, dim3(b ? 2 : 1), dim3(256), 0, ST(stream), a, b, n, out);
  return check_launch("tsne_sums");
}
