// Gaussian mixture clustering of latents (reference eval/cluster.py::gmm and eval/metrics.py::epoch_cluster_entropy, which fit
// sklearn's GaussianMixture with k-means++ seeding): the seeding rounds, the E-step and the M-step, all in fp64.
//
// Rows: A [n][lda] from svae_cv_center (identity perm, ny = 0), columns [0, d) = x - global mean, column d = 1.  Component means
// live in the same centred frame.  Every floating-point reduction runs in one fixed order (no float atomics): the same input and
// the same host random draws give bit-identical results on one device.
#include "svae_internal.h"

#include "fixed_sum.h"  // block_sum_all; sets no contraction pragma: the fma below stay

namespace svae {

constexpr int KPP_ROWS = 256;   // rows per block of the k-means++ distance kernel = one chunk of its prefix sum
constexpr int ES_ROWS = 64;     // E-step: one wave per 64 rows, lane = row
constexpr int ES_LDV = ES_ROWS + 1;
constexpr int ES_J = 8;         // E-step (full): output columns of (x - mu) P per pass over the row
constexpr int MS_ROWS = 64;     // M-step: rows staged per step
constexpr int GT = 32;          // M-step (full): edge of one output tile of the weighted Gram matrix
constexpr int CHUNK_ROWS = 4096;  // M-step row chunk per output tile (see svae_gmm_chunks)

// ---- k-means++ -----------------------------------------------------------------------------------------------------------------
// d2[t][r] = min(closest[r], sum_j (A[r][j] - A[cand[t]][j])^2) (closest NULL: no minimum), part[t][b] = tree sum of d2[t] over
// block b's rows.  A candidate drawn twice runs the same arithmetic: bit-equal distances and potentials.
__global__ __launch_bounds__(256) void gmm_kpp_dist_kernel(const double* __restrict__ A, int lda, int d, int n,
                                                           const int* __restrict__ cand, int T, const double* __restrict__ closest,
                                                           double* __restrict__ d2, double* __restrict__ part) {
  __shared__ double red[256];
  const long long r = (long long)blockIdx.x * KPP_ROWS + threadIdx.x;
  const bool ok = r < n;
  const double cl = ok && closest ? closest[r] : INFINITY;
  for (int t = 0; t < T; ++t) {
    const double* c = A + (long long)min(max(cand[t], 0), n - 1) * lda;
    double s = 0.0;
    if (ok) {
      const double* a = A + r * lda;
      for (int j = 0; j < d; ++j) {
        const double e = a[j] - c[j];
        s = fma(e, e, s);
      }
      s = fmin(cl, s);
      d2[(long long)t * n + r] = s;
    }
    const double bs = block_sum_all<256>(s, red);
    if (threadIdx.x == 0) part[(long long)t * gridDim.x + blockIdx.x] = bs;
  }
}

// potential of candidate t = sum_b part[t][b] in ascending b; the first smallest wins: pot[0], id[0] = cand[best], best[0] = best
__global__ __launch_bounds__(64) void gmm_kpp_choose_kernel(const double* __restrict__ part, int nb, int T, const int* __restrict__ cand,
                                                            double* __restrict__ pot, int* __restrict__ id, int* __restrict__ best) {
  __shared__ double p[SVAE_GMM_MAX_TRIALS];
  const int t = threadIdx.x;
  if (t < T) {
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s += part[(long long)t * nb + b];
    p[t] = s;
  }
  __syncthreads();
  if (t == 0) {
    int bt = 0;
    for (int u = 1; u < T; ++u)
      if (p[u] < p[bt]) bt = u;
    pot[0] = p[bt];
    id[0] = cand[bt];
    best[0] = bt;
  }
}

// the winner's distances become the closest distances and its block sums the chunk totals of the next prefix sum
__global__ __launch_bounds__(256) void gmm_kpp_keep_kernel(const double* __restrict__ d2, const double* __restrict__ part,
                                                           const int* __restrict__ best, int n, int nb, double* __restrict__ closest,
                                                           double* __restrict__ tot) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long b = best[0];
  if (i < n) closest[i] = d2[b * n + i];
  if (i < nb) tot[i] = part[b * nb + i];
}

// np.searchsorted(cumsum(closest), vals[t]) (side left) clipped to n - 1, on the prefix sum
//   prefix(r) = (tot[0] + ... + tot[b - 1]) + closest[b * 256] + ... + closest[r],   b = r / 256,
// whose chunk bases are added in the order gmm_kpp_choose_kernel adds the potential
__global__ __launch_bounds__(64) void gmm_kpp_search_kernel(const double* __restrict__ closest, const double* __restrict__ tot, int n,
                                                            int nb, const double* __restrict__ vals, int T, int* __restrict__ cand) {
  const int t = threadIdx.x;
  if (t >= T) return;
  const double v = vals[t];
  double base = 0.0;
  int b = 0;
  for (; b < nb; ++b) {
    const double nx = base + tot[b];
    if (nx >= v) break;
    base = nx;
  }
  int r = n - 1;
  if (b < nb) {
    const int r0 = b * KPP_ROWS, r1 = min(n, r0 + KPP_ROWS);
    double s = base;
    r = r1 - 1;
    for (int i = r0; i < r1; ++i) {
      s += closest[i];
      if (s >= v) { r = i; break; }
    }
  }
  cand[t] = r;
}

// ---- E-step ---------------------------------------------------------------------------------------------------------------------
// One wave per 64 rows (lane = row), the rows staged in LDS as v[j][lane].  Weighted log density of row r under component k:
//   w_k = cst[k] - q / 2,  full: q = |(a - mu_k) P_k|^2 (P_k upper triangular [d][ldp], ldp = pad8(d), zero elsewhere),
//                          diag: q = sum_j ((a_j - mu_kj) p_kj)^2 (P [K][d]).
// With resp: the w_k are parked in resp[k][r], lse = max + log sum_k exp(w_k - max) (components in order), then
// resp[k][r] = exp(w_k - lse), lpn[r] = lse and part[block] = wave sum of lse.  label[r] = first argmax, gap[r] = top-two gap.
__global__ __launch_bounds__(64) void gmm_estep_kernel(const double* __restrict__ A, int lda, int d, int n, int K, int diag,
                                                       const double* __restrict__ mu, const double* __restrict__ P, int ldp,
                                                       const double* __restrict__ cst, double* __restrict__ resp, double* __restrict__ lpn,
                                                       double* __restrict__ part, int* __restrict__ label, double* __restrict__ gap) {
  extern __shared__ __attribute__((aligned(16))) double v[];  // [d][ES_LDV]
  const int lane = threadIdx.x;
  const long long row0 = (long long)blockIdx.x * ES_ROWS;
  for (int e = lane; e < ES_ROWS * d; e += ES_ROWS) {  // coalesced along the row
    const int rr = e / d, j = e - rr * d;
    v[j * ES_LDV + rr] = row0 + rr < n ? A[(row0 + rr) * lda + j] : 0.0;
  }
  __syncthreads();
  const long long r = row0 + lane;
  const bool ok = r < n;
  const double* vr = v + lane;
  double best = -INFINITY, second = -INFINITY;
  int arg = 0;
  for (int k = 0; k < K; ++k) {
    const double* mk = mu + (long long)k * d;
    double q = 0.0;
    if (diag) {
      const double* pk = P + (long long)k * d;
      for (int j = 0; j < d; ++j) {
        const double y = (vr[j * ES_LDV] - mk[j]) * pk[j];
        q = fma(y, y, q);
      }
    } else {
      const double* Pk = P + (long long)k * d * ldp;
      for (int j0 = 0; j0 < d; j0 += ES_J) {
        double y[ES_J];
#pragma unroll
        for (int jj = 0; jj < ES_J; ++jj) y[jj] = 0.0;
        const int i1 = min(d, j0 + ES_J);
        for (int i = 0; i < i1; ++i) {
          const double vi = vr[i * ES_LDV] - mk[i];
          const double* pr = Pk + (long long)i * ldp + j0;
#pragma unroll
          for (int jj = 0; jj < ES_J; ++jj) y[jj] = fma(vi, pr[jj], y[jj]);
        }
#pragma unroll
        for (int jj = 0; jj < ES_J; ++jj) q = fma(y[jj], y[jj], q);
      }
    }
    const double w = cst[k] - 0.5 * q;
    if (resp && ok) resp[(long long)k * n + r] = w;
    if (w > best) { second = best; best = w; arg = k; }
    else if (w > second) second = w;
  }
  if (resp) {
    double lse = 0.0;
    if (ok) {
      double s = 0.0;
      for (int k = 0; k < K; ++k) s += exp(resp[(long long)k * n + r] - best);
      lse = best + log(s);
      for (int k = 0; k < K; ++k) resp[(long long)k * n + r] = exp(resp[(long long)k * n + r] - lse);
      if (lpn) lpn[r] = lse;
    }
    if (part) {
      const double t = wave_sum_d(lse);
      if (lane == 0) part[blockIdx.x] = t;
    }
  }
  if (ok) {
    if (label) label[r] = arg;
    if (gap) gap[r] = best - second;
  }
}

// out[0] = (sum of x[0:m]) / div: thread t adds x[t], x[t + 256], ... in order, then a fixed tree
__global__ __launch_bounds__(256) void gmm_sum_kernel(const double* __restrict__ x, int m, double div, double* __restrict__ out) {
  __shared__ double red[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < m; i += 256) s += x[i];
  s = block_sum_all<256>(s, red);
  if (threadIdx.x == 0) out[0] = s / div;
}

// ---- M-step ---------------------------------------------------------------------------------------------------------------------
// Per (row chunk c, component k = 4 blockIdx.y + wave, 64-column tile): lane = column j, rows of the chunk in ascending order.
//   mu NULL: part[c][k][j] = sum_r resp[k][r] A[r][j], j <= d (column d of A is 1: the responsibility total)
//   mu set : part[c][k][j] = sum_r resp[k][r] (A[r][j] - mu[k][j])^2, j < d (diagonal covariance, about the new means)
// The four waves of a block read the same rows.
__global__ __launch_bounds__(256) void gmm_wsum_kernel(const double* __restrict__ A, int lda, int d, int n, int K,
                                                       const double* __restrict__ resp, const double* __restrict__ mu, int rows_per,
                                                       double* __restrict__ part) {
  const int c = blockIdx.x, k = blockIdx.y * 4 + (threadIdx.x >> 6);
  const int j = blockIdx.z * 64 + (threadIdx.x & 63);
  const int D = mu ? d : d + 1;
  if (k >= K || j >= D) return;
  const long long lo = (long long)c * rows_per, hi = min((long long)n, lo + rows_per);
  const double* wk = resp + (long long)k * n;
  double acc = 0.0;
  if (mu) {
    const double mj = mu[(long long)k * d + j];
    for (long long r = lo; r < hi; ++r) {
      const double e = A[r * lda + j] - mj;
      acc = fma(wk[r] * e, e, acc);
    }
  } else {
    for (long long r = lo; r < hi; ++r) acc = fma(wk[r], A[r * lda + j], acc);
  }
  part[((long long)c * K + k) * D + j] = acc;
}

// part[c][k][i][j] = sum_{r in chunk c} resp[k][r] (A[r][i] - mu[k][i]) (A[r][j] - mu[k][j]), j <= i, mirrored into j > i.
// Workgroup = (chunk, lower-triangle 32 x 32 tile, component), thread = 2 x 2 entries, rows staged 64 at a time in ascending order.
__global__ __launch_bounds__(256) void gmm_gram_kernel(const double* __restrict__ A, int lda, int d, int n, int K,
                                                       const double* __restrict__ resp, const double* __restrict__ mu, int rows_per,
                                                       double* __restrict__ part) {
  __shared__ double vi[MS_ROWS][GT + 1], vj[MS_ROWS][GT + 1], wr[MS_ROWS];
  const int c = blockIdx.x, k = blockIdx.z;
  int bi = 0, t = blockIdx.y;
  while (t > bi) { t -= bi + 1; ++bi; }
  const int i0 = bi * GT, j0 = t * GT;
  const int ti = threadIdx.x >> 4, tj = threadIdx.x & 15;
  const long long lo = (long long)c * rows_per, hi = min((long long)n, lo + rows_per);
  const double* wk = resp + (long long)k * n;
  const double* mk = mu + (long long)k * d;
  double a00 = 0.0, a01 = 0.0, a10 = 0.0, a11 = 0.0;
  for (long long rb = lo; rb < hi; rb += MS_ROWS) {
    for (int e = threadIdx.x; e < MS_ROWS * GT; e += 256) {
      const int rr = e / GT, cc = e % GT;
      const long long r = rb + rr;
      const bool ok = r < hi;
      vi[rr][cc] = ok && i0 + cc < d ? A[r * lda + i0 + cc] - mk[i0 + cc] : 0.0;
      vj[rr][cc] = ok && j0 + cc < d ? A[r * lda + j0 + cc] - mk[j0 + cc] : 0.0;
    }
    if (threadIdx.x < MS_ROWS) {
      const long long r = rb + threadIdx.x;
      wr[threadIdx.x] = r < hi ? wk[r] : 0.0;
    }
    __syncthreads();
#pragma unroll 8
    for (int rr = 0; rr < MS_ROWS; ++rr) {
      const double w = wr[rr];
      const double x0 = w * vi[rr][2 * ti], x1 = w * vi[rr][2 * ti + 1];
      const double y0 = vj[rr][2 * tj], y1 = vj[rr][2 * tj + 1];
      a00 = fma(x0, y0, a00);
      a01 = fma(x0, y1, a01);
      a10 = fma(x1, y0, a10);
      a11 = fma(x1, y1, a11);
    }
    __syncthreads();
  }
  double* o = part + ((long long)c * K + k) * d * d;
  const double acc[2][2] = {{a00, a01}, {a10, a11}};
  for (int u = 0; u < 2; ++u)
    for (int s = 0; s < 2; ++s) {
      const int i = i0 + 2 * ti + u, j = j0 + 2 * tj + s;
      if (i < d && j <= i) {
        o[(long long)i * d + j] = acc[u][s];
        o[(long long)j * d + i] = acc[u][s];
      }
    }
}

// out[e] = sum_c part[c][e] in ascending c
__global__ __launch_bounds__(256) void gmm_chunk_sum_kernel(const double* __restrict__ part, int chunks, long long m,
                                                            double* __restrict__ out) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= m) return;
  double s = 0.0;
  for (int c = 0; c < chunks; ++c) s += part[(long long)c * m + e];
  out[e] = s;
}

// block k: nk = s1[k][d] + 10 eps, mu[k] = s1[k][0:d] / nk, w[k] = nk / sum_k' nk' (components in order)
__global__ __launch_bounds__(256) void gmm_means_kernel(const double* __restrict__ s1, int d, int K, double* __restrict__ nk,
                                                        double* __restrict__ w, double* __restrict__ mu) {
  const int k = blockIdx.x;
  const double e10 = 10.0 * __DBL_EPSILON__;
  const double nkk = s1[(long long)k * (d + 1) + d] + e10;
  for (int j = threadIdx.x; j < d; j += 256) mu[(long long)k * d + j] = s1[(long long)k * (d + 1) + j] / nkk;
  if (threadIdx.x == 0) {
    double tot = 0.0;
    for (int u = 0; u < K; ++u) tot += s1[(long long)u * (d + 1) + d] + e10;
    nk[k] = nkk;
    w[k] = nkk / tot;
  }
}

// full: cov[k] = S[k] / nk + reg I in place.  diag: var = S / nk + reg in place, P = 1 / sqrt(var), cst = log w + sum log P
// - d log(2 pi) / 2, and bad[k] = 1 when some var <= 0 (not a number included).
__global__ __launch_bounds__(256) void gmm_cov_kernel(double* __restrict__ S, const double* __restrict__ nk, const double* __restrict__ w,
                                                      int d, int diag, double reg, double* __restrict__ P, double* __restrict__ cst,
                                                      int* __restrict__ bad) {
  const int k = blockIdx.x;
  const double nkk = nk[k];
  if (!diag) {
    double* Sk = S + (long long)k * d * d;
    for (int e = threadIdx.x; e < d * d; e += 256) Sk[e] = Sk[e] / nkk + (e / d == e % d ? reg : 0.0);
    return;
  }
  double* Sk = S + (long long)k * d;
  for (int j = threadIdx.x; j < d; j += 256) {
    const double var = Sk[j] / nkk + reg;
    Sk[j] = var;
    P[(long long)k * d + j] = var > 0.0 ? 1.0 / sqrt(var) : 0.0;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double ld = 0.0;
    int b = 0;
    for (int j = 0; j < d; ++j) {
      const double var = Sk[j];
      if (!(var > 0.0)) b = 1;
      else ld += log(P[(long long)k * d + j]);
    }
    bad[k] = b;
    cst[k] = log(w[k]) + ld - 0.5 * d * log(2.0 * M_PI);
  }
}

// full: from the Cholesky factor L[k] (lower, [d][d]) of cov[k]: P[k] = L^-T (upper, [d][ldp], zero elsewhere), one thread per
// column j of L^-1 (forward substitution, ascending), cst = log w + sum log P_jj - d log(2 pi) / 2; bad[k] = rank[k] < d
// (not positive definite), P and cst then left as they are.
__global__ __launch_bounds__(128) void gmm_prec_kernel(const double* __restrict__ L, const int* __restrict__ rank,
                                                       const double* __restrict__ w, int d, int ldp, double* __restrict__ P,
                                                       double* __restrict__ cst, int* __restrict__ bad) {
  const int k = blockIdx.x, j = threadIdx.x;
  const bool pd = rank[k] == d;
  if (j == 0) bad[k] = pd ? 0 : 1;
  if (!pd) return;
  const double* Lk = L + (long long)k * d * d;
  if (j < d) {
    double* Pj = P + ((long long)k * d + j) * ldp;  // row j of P = column j of L^-1
    for (int i = 0; i < ldp; ++i)
      if (i < j || i >= d) Pj[i] = 0.0;
    Pj[j] = 1.0 / Lk[(long long)j * d + j];
    for (int i = j + 1; i < d; ++i) {
      const double* li = Lk + (long long)i * d;
      double s = 0.0;
      for (int m = j; m < i; ++m) s = fma(li[m], Pj[m], s);
      Pj[i] = -s / li[i];
    }
  }
  if (j == 0) {
    double ld = 0.0;
    for (int i = 0; i < d; ++i) ld += log(1.0 / Lk[(long long)i * d + i]);
    cst[k] = log(w[k]) + ld - 0.5 * d * log(2.0 * M_PI);
  }
}

static int kpp_args(const double* A, int lda, int d, int n) {
  SVAE_REQUIRE(A && n > 0 && d > 0 && d <= SVAE_CV_MAX_DIM && lda > d, SVAE_ERR_ARG, "gmm_kpp: bad rows (n=%d d=%d lda=%d)", n, d, lda);
  return SVAE_OK;
}

static int mixture_args(const char* what, const double* A, int lda, int d, int n, int K) {
  SVAE_REQUIRE(A && n > 0 && d > 0 && d <= SVAE_CV_MAX_DIM && lda > d && K >= 1 && K <= SVAE_GMM_MAX_COMPONENTS, SVAE_ERR_ARG,
               "%s: bad args (n=%d d=%d lda=%d K=%d)", what, n, d, lda, K);
  return SVAE_OK;
}

}  // namespace svae

using namespace svae;

extern "C" int svae_gmm_kpp_blocks(int n) { return (n + KPP_ROWS - 1) / KPP_ROWS; }

extern "C" int svae_gmm_kpp_round(const double* A, int lda, int d, int n, const double* vals, int T, int* cand, double* closest,
                                  double* tot, double* d2, double* part, double* pot, int* id, int* best, void* stream) {
  if (int e = kpp_args(A, lda, d, n)) return e;
  SVAE_REQUIRE(cand && closest && tot && d2 && part && pot && id && best && T >= 1 && T <= SVAE_GMM_MAX_TRIALS && (vals || T == 1),
               SVAE_ERR_ARG, "gmm_kpp_round: bad args (T=%d)", T);
  const int nb = (n + KPP_ROWS - 1) / KPP_ROWS;
  if (vals) {
    hipLaunchKernelGGL(gmm_kpp_search_kernel, dim3(1), dim3(64), 0, ST(stream), closest, tot, n, nb, vals, T, cand);
    if (int e = check_launch("gmm_kpp_search")) return e;
  }
  hipLaunchKernelGGL(gmm_kpp_dist_kernel, dim3(nb), dim3(256), 0, ST(stream), A, lda, d, n, cand, T, vals ? closest : nullptr, d2, part);
  if (int e = check_launch("gmm_kpp_dist")) return e;
  hipLaunchKernelGGL(gmm_kpp_choose_kernel, dim3(1), dim3(64), 0, ST(stream), part, nb, T, cand, pot, id, best);
  if (int e = check_launch("gmm_kpp_choose")) return e;
  hipLaunchKernelGGL(gmm_kpp_keep_kernel, dim3(nb), dim3(256), 0, ST(stream), d2, part, best, n, nb, closest, tot);
  return check_launch("gmm_kpp_keep");
}

extern "C" int svae_gmm_estep_f64(const double* A, int lda, int d, int n, int K, int diag, const double* mu, const double* P, int ldp,
                                  const double* cst, double* resp, double* lpn, double* part, int* label, double* gap, void* stream) {
  if (int e = mixture_args("gmm_estep_f64", A, lda, d, n, K)) return e;
  SVAE_REQUIRE(mu && P && cst && (diag || ldp == (d + 7) / 8 * 8) && (resp || (!lpn && !part)) && (resp || label || gap), SVAE_ERR_ARG,
               "gmm_estep_f64: bad args (d=%d ldp=%d)", d, ldp);
  const size_t smem = (size_t)d * ES_LDV * sizeof(double);
  static DeviceOnce once;
  if (int e = allow_lds(gmm_estep_kernel, once, 96 * 1024, "gmm_estep_f64")) return e;
  hipLaunchKernelGGL(gmm_estep_kernel, dim3((n + ES_ROWS - 1) / ES_ROWS), dim3(ES_ROWS), smem, ST(stream), A, lda, d, n, K, diag, mu, P,
                     ldp, cst, resp, lpn, part, label, gap);
  return check_launch("gmm_estep_f64");
}

extern "C" int svae_gmm_estep_blocks(int n) { return (n + ES_ROWS - 1) / ES_ROWS; }

extern "C" int svae_gmm_sum_f64(const double* x, int m, double div, double* out, void* stream) {
  SVAE_REQUIRE(x && out && m > 0, SVAE_ERR_ARG, "gmm_sum_f64: bad args (m=%d)", m);
  hipLaunchKernelGGL(gmm_sum_kernel, dim3(1), dim3(256), 0, ST(stream), x, m, div, out);
  return check_launch("gmm_sum_f64");
}

static int gram_tiles(int d) {
  const int nt = (d + GT - 1) / GT;
  return nt * (nt + 1) / 2;
}

extern "C" int svae_gmm_chunks(int n, int d) {
  if (n <= 0 || d <= 0) return 0;
  const long long rows = (long long)CHUNK_ROWS * gram_tiles(d);
  return (int)((n + rows - 1) / rows);
}

extern "C" int svae_gmm_mstep_f64(const double* A, int lda, int d, int n, int K, int diag, const double* resp, double reg, double* part,
                                  double* s1, double* nk, double* w, double* mu, double* cov, double* P, double* cst, int* bad,
                                  void* stream) {
  if (int e = mixture_args("gmm_mstep_f64", A, lda, d, n, K)) return e;
  SVAE_REQUIRE(resp && part && s1 && nk && w && mu && cov && bad && (!diag || (P && cst)) && reg >= 0.0, SVAE_ERR_ARG,
               "gmm_mstep_f64: null buffer");
  const int chunks = svae_gmm_chunks(n, d);
  const int rows_per = (n + chunks - 1) / chunks;
  hipLaunchKernelGGL(gmm_wsum_kernel, dim3(chunks, (K + 3) / 4, (d + 1 + 63) / 64), dim3(256), 0, ST(stream), A, lda, d, n, K, resp,
                     nullptr, rows_per, part);
  if (int e = check_launch("gmm_wsum")) return e;
  const long long m1 = (long long)K * (d + 1);
  hipLaunchKernelGGL(gmm_chunk_sum_kernel, dim3((unsigned)((m1 + 255) / 256)), dim3(256), 0, ST(stream), part, chunks, m1, s1);
  if (int e = check_launch("gmm_chunk_sum")) return e;
  hipLaunchKernelGGL(gmm_means_kernel, dim3(K), dim3(256), 0, ST(stream), s1, d, K, nk, w, mu);
  if (int e = check_launch("gmm_means")) return e;
  long long m2;
  if (diag) {
    hipLaunchKernelGGL(gmm_wsum_kernel, dim3(chunks, (K + 3) / 4, (d + 63) / 64), dim3(256), 0, ST(stream), A, lda, d, n, K, resp, mu,
                       rows_per, part);
    m2 = (long long)K * d;
  } else {
    hipLaunchKernelGGL(gmm_gram_kernel, dim3(chunks, gram_tiles(d), K), dim3(256), 0, ST(stream), A, lda, d, n, K, resp, mu, rows_per,
                       part);
    m2 = (long long)K * d * d;
  }
  if (int e = check_launch(diag ? "gmm_wsum" : "gmm_gram")) return e;
  hipLaunchKernelGGL(gmm_chunk_sum_kernel, dim3((unsigned)((m2 + 255) / 256)), dim3(256), 0, ST(stream), part, chunks, m2, cov);
  if (int e = check_launch("gmm_chunk_sum")) return e;
  hipLaunchKernelGGL(gmm_cov_kernel, dim3(K), dim3(256), 0, ST(stream), cov, nk, w, d, diag, reg, P, cst, bad);
  return check_launch("gmm_cov");
}

extern "C" int svae_gmm_precision_f64(const double* L, const int* rank, const double* w, int d, int K, int ldp, double* P, double* cst,
                                      int* bad, void* stream) {
  SVAE_REQUIRE(L && rank && w && P && cst && bad && d > 0 && d <= SVAE_CV_MAX_DIM && K >= 1 && K <= SVAE_GMM_MAX_COMPONENTS &&
                   ldp == (d + 7) / 8 * 8, SVAE_ERR_ARG, "gmm_precision_f64: bad args (d=%d K=%d ldp=%d)", d, K, ldp);
  hipLaunchKernelGGL(gmm_prec_kernel, dim3(K), dim3(128), 0, ST(stream), L, rank, w, d, ldp, P, cst, bad);
  return check_launch("gmm_precision_f64");
}
