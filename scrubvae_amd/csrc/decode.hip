// Latent decodability metrics (reference eval/metrics.py:231-329, called by train() at trainer.py:416-506): cross-validated
// linear regression, QDA and elastic-net one-vs-rest logistic regression on the validation latents, all in fp64.
//
// Row layout shared by every kernel here: the host sorts the downsampled rows by group (fold, then class) and
// svae_cv_center writes them as one fp64 matrix A [n][lda] with columns
//     [0, d)          x - mean(x)     (global column mean over all n rows: |mean| >> std does not cancel)
//     d               1               (counts / intercepts fall out of the same Gram matrix)
//     [d+1, d+1+ny)   y - mean(y)     (regression targets, ny may be 0)
// so one Gram matrix sum_r w_r a_r a_r^T per group holds the count, sum x, sum x x^T, sum x y^T, sum y and sum y y^T of the
// group.  Every reduction walks its rows in one fixed order (no atomics on floating point): results are bit-reproducible.
#include "svae_internal.h"

#include "fixed_sum.h"  // block_sum_all; sets no contraction pragma

namespace svae {

constexpr int CV_LDS_MAX = 152 * 1024;  // dynamic LDS ceiling: 160 KiB less the kernels' static arrays (<= 5 KiB)

__device__ __forceinline__ double softplus_d(double t) {  // log(1 + exp(t)), stable
  return t > 0.0 ? t + log1p(exp(-t)) : log1p(exp(t));
}
__device__ __forceinline__ double sigmoid_d(double t) {
  if (t >= 0.0) return 1.0 / (1.0 + exp(-t));
  const double e = exp(t);
  return e / (1.0 + e);
}

// ---- column means: one block per column, thread t sums rows t, t + 256, ... in order, then a fixed tree
__global__ __launch_bounds__(256) void cv_colmean_kernel(const float* __restrict__ x, int ldx, int d, const float* __restrict__ y,
                                                         int ldy, int n, double* __restrict__ mean) {
  __shared__ double red[256];
  const int c = blockIdx.x;
  const float* src = c < d ? x + c : y + (c - d);
  const int ld = c < d ? ldx : ldy;
  double s = 0.0;
  for (int r = threadIdx.x; r < n; r += 256) s += (double)src[(long long)r * ld];
  s = block_sum_all<256>(s, red);
  if (threadIdx.x == 0) mean[c] = s / (double)n;
}

__global__ __launch_bounds__(256) void cv_center_kernel(const float* __restrict__ x, int ldx, int d, const float* __restrict__ y,
                                                        int ldy, int ny, const int* __restrict__ perm, int n,
                                                        const double* __restrict__ mean, double* __restrict__ A, int lda) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)n * lda) return;
  const int r = (int)(i / lda), c = (int)(i - (long long)r * lda);
  const long long src = perm[r];
  double v = 0.0;
  if (c < d) v = (double)x[src * ldx + c] - mean[c];
  else if (c == d) v = 1.0;
  else if (c < d + 1 + ny) v = (double)y[src * ldy + (c - d - 1)] - mean[c - 1];
  A[i] = v;
}

// ---- weighted Gram matrices: out[g] = sum_{r in [lo_g, hi_g)} w[g][r] a_r a_r^T (w NULL: 1).  Workgroup = (16 x 16 tile of
// the lower triangle, group); thread = one entry; rows staged 64 at a time; the sum runs over rows in ascending order.
constexpr int GR_ROWS = 64;
__global__ __launch_bounds__(256) void cv_gram_kernel(const double* __restrict__ A, int lda, int D, const int* __restrict__ lo,
                                                      const int* __restrict__ hi, const double* __restrict__ w, long long ldw,
                                                      const int* __restrict__ skip, double* __restrict__ out, int ldo) {
  __shared__ double ai[GR_ROWS][17], aj[GR_ROWS][17], wr[GR_ROWS];
  const int g = blockIdx.y;
  if (skip && skip[g]) return;
  int bi = 0, t = blockIdx.x;
  while (t > bi) { t -= bi + 1; ++bi; }
  const int bj = t;
  const int i0 = bi * 16, j0 = bj * 16;
  const int ti = threadIdx.x >> 4, tj = threadIdx.x & 15;
  const int r0 = lo[g], r1 = hi[g];
  const double* wg = w ? w + (long long)g * ldw : nullptr;
  double acc = 0.0;
  for (int rb = r0; rb < r1; rb += GR_ROWS) {
    for (int e = threadIdx.x; e < GR_ROWS * 16; e += 256) {
      const int rr = e >> 4, cc = e & 15, r = rb + rr;
      const bool ok = r < r1;
      ai[rr][cc] = ok && i0 + cc < D ? A[(long long)r * lda + i0 + cc] : 0.0;
      aj[rr][cc] = ok && j0 + cc < D ? A[(long long)r * lda + j0 + cc] : 0.0;
    }
    if (threadIdx.x < GR_ROWS) {
      const int r = rb + threadIdx.x;
      wr[threadIdx.x] = r < r1 ? (wg ? wg[r] : 1.0) : 0.0;
    }
    __syncthreads();
#pragma unroll 8
    for (int rr = 0; rr < GR_ROWS; ++rr) acc = fma(wr[rr] * ai[rr][ti], aj[rr][tj], acc);
    __syncthreads();
  }
  const int i = i0 + ti, j = j0 + tj;
  if (i < D && j < D && j <= i) {
    double* o = out + (long long)g * ldo * ldo;
    o[(long long)i * ldo + j] = acc;
    o[(long long)j * ldo + i] = acc;
  }
}

// ---- batched Cholesky with rank-revealing zero pivots, one workgroup per matrix, its lower triangle packed in LDS (row i starts
// at i (i + 1) / 2: 66 KB at n = 128, two workgroups per CU)
__device__ __forceinline__ int tri(int i, int j) { return i * (i + 1) / 2 + j; }  // j <= i
__global__ __launch_bounds__(256) void spd_factor_solve_kernel(const double* __restrict__ M, int ldm, long long strideM, int n,
                                                               const double* __restrict__ B, int nrhs, long long strideB,
                                                               double* __restrict__ L, double* __restrict__ X,
                                                               double* __restrict__ logdet, int* __restrict__ rank, double rtol) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  double* a = sm;                      // packed lower triangle
  double* b = sm + n * (n + 1) / 2;    // [n][nrhs]
  __shared__ double red[256];
  const int tid = threadIdx.x;
  const double* Mg = M + blockIdx.x * strideM;
  for (int i = 0; i < n; ++i)
    for (int j = tid; j <= i; j += 256) a[tri(i, j)] = Mg[(long long)i * ldm + j];
  if (B)
    for (int e = tid; e < n * nrhs; e += 256) b[e] = B[blockIdx.x * strideB + e];
  __syncthreads();
  double md = 0.0;
  for (int i = tid; i < n; i += 256) md = fmax(md, a[tri(i, i)]);
  red[tid] = md;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] = fmax(red[tid], red[tid + s]);
    __syncthreads();
  }
  const double thr = rtol * red[0];
  double ld_acc = 0.0;  // thread 0 only
  int rk = 0;
  for (int k = 0; k < n; ++k) {
    const double piv = a[tri(k, k)];
    __syncthreads();
    const bool keep = piv > thr && piv > 0.0;
    if (keep) {
      const double lkk = sqrt(piv);
      for (int i = k + tid; i < n; i += 256) a[tri(i, k)] = i == k ? lkk : a[tri(i, k)] / lkk;
      if (tid == 0) { ld_acc += 2.0 * log(lkk); ++rk; }
      __syncthreads();
      const int m = n - k - 1;
      for (int e = tid; e < m * m; e += 256) {
        const int i = k + 1 + e / m, j = k + 1 + e % m;
        if (j <= i) a[tri(i, j)] -= a[tri(i, k)] * a[tri(j, k)];
      }
    } else {
      for (int i = k + tid; i < n; i += 256) a[tri(i, k)] = 0.0;  // a zero direction: its column (and coefficient) is 0
    }
    __syncthreads();
  }
  if (B) {  // forward then backward substitution, dropped pivots give 0
    for (int k = 0; k < n; ++k) {
      const double lkk = a[tri(k, k)];
      if (tid < nrhs) b[k * nrhs + tid] = lkk != 0.0 ? b[k * nrhs + tid] / lkk : 0.0;
      __syncthreads();
      for (int e = tid; e < (n - k - 1) * nrhs; e += 256) {
        const int i = k + 1 + e / nrhs, r = e % nrhs;
        b[i * nrhs + r] -= a[tri(i, k)] * b[k * nrhs + r];
      }
      __syncthreads();
    }
    for (int k = n - 1; k >= 0; --k) {
      const double lkk = a[tri(k, k)];
      if (tid < nrhs) b[k * nrhs + tid] = lkk != 0.0 ? b[k * nrhs + tid] / lkk : 0.0;
      __syncthreads();
      for (int e = tid; e < k * nrhs; e += 256) {
        const int i = e / nrhs, r = e % nrhs;
        b[i * nrhs + r] -= a[tri(k, i)] * b[k * nrhs + r];
      }
      __syncthreads();
    }
    for (int e = tid; e < n * nrhs; e += 256) X[blockIdx.x * strideB + e] = b[e];
  }
  if (L)
    for (int e = tid; e < n * n; e += 256) {
      const int i = e / n, j = e % n;
      L[blockIdx.x * strideM + (long long)i * ldm + j] = j <= i ? a[tri(i, j)] : 0.0;
    }
  if (tid == 0) {
    if (logdet) logdet[blockIdx.x] = ld_acc;
    if (rank) rank[blockIdx.x] = rk;
  }
}

// ---- R^2 statistics per (fold, output): stats[f][o] = {sum (y - yhat)^2, sum yc, sum yc^2, count} over the rows of fold f.
// Linear: yhat_c = a_r[0:d] . beta[f][:, o] + c0[f][o] in the centred frame.  MLP (pred != NULL): yhat = pred[member][r][o], compared
// with the raw target yc + ymean.
__global__ __launch_bounds__(256) void cv_r2_kernel(const double* __restrict__ A, int lda, int d, int ny, const int* __restrict__ lo,
                                                    const int* __restrict__ hi, const double* __restrict__ beta,
                                                    const double* __restrict__ c0, const float* const* __restrict__ pred,
                                                    int ldp, const double* __restrict__ ymean, double* __restrict__ stats) {
  __shared__ double red[256];
  const int f = blockIdx.x, o = blockIdx.y;
  double sr = 0.0, sy = 0.0, syy = 0.0;
  for (int r = lo[f] + threadIdx.x; r < hi[f]; r += 256) {
    const double* ar = A + (long long)r * lda;
    const double yc = ar[d + 1 + o];
    double e;
    if (pred) {
      e = (yc + ymean[o]) - (double)pred[f][(long long)r * ldp + o];
    } else {
      const double* bt = beta + (long long)f * d * ny;
      double p = c0[f * ny + o];
      for (int i = 0; i < d; ++i) p = fma(ar[i], bt[i * ny + o], p);
      e = yc - p;
    }
    sr = fma(e, e, sr);
    sy += yc;
    syy = fma(yc, yc, syy);
  }
  sr = block_sum_all<256>(sr, red);
  sy = block_sum_all<256>(sy, red);
  syy = block_sum_all<256>(syy, red);
  if (threadIdx.x == 0) {
    double* s = stats + ((long long)f * ny + o) * 4;
    s[0] = sr; s[1] = sy; s[2] = syy; s[3] = (double)(hi[f] - lo[f]);
  }
}

// ---- QDA scores: one wave per 64 test rows of one fold.  v = x - mu_c lives in LDS ([d][64], lane = row) and is overwritten by
// L_c^-1 v; score_c = cst[f][c] - |L^-1 v|^2 / 2 with cst = -logdet/2 + log prior (-inf: class absent from the training fold).
constexpr int QDA_ROWS = 64;
__global__ __launch_bounds__(64) void cv_qda_kernel(const double* __restrict__ A, int lda, int d, int K, const int* __restrict__ lo,
                                                    const int* __restrict__ hi, const double* __restrict__ mu,
                                                    const double* __restrict__ L, int ldl, const double* __restrict__ cst,
                                                    const int* __restrict__ label, int* __restrict__ correct, int* __restrict__ pred,
                                                    double* __restrict__ gap) {
  extern __shared__ __attribute__((aligned(16))) double v[];
  const int f = blockIdx.y, lane = threadIdx.x;
  const int r = lo[f] + blockIdx.x * QDA_ROWS + lane;
  if (lo[f] + blockIdx.x * QDA_ROWS >= hi[f]) return;  // wave-uniform
  const bool ok = r < hi[f];
  double best = -INFINITY, second = -INFINITY;
  int arg = -1;
  for (int c = 0; c < K; ++c) {
    const double k0 = cst[f * K + c];
    if (!(k0 > -INFINITY)) continue;  // uniform
    const double* m = mu + ((long long)f * K + c) * d;
    const double* Lc = L + ((long long)f * K + c) * ldl * ldl;
    for (int i = 0; i < d; ++i) v[i * QDA_ROWS + lane] = ok ? A[(long long)r * lda + i] - m[i] : 0.0;
    double q = 0.0;
    for (int i = 0; i < d; ++i) {
      const double* li = Lc + (long long)i * ldl;
      double s = v[i * QDA_ROWS + lane];
      for (int j = 0; j < i; ++j) s = fma(-li[j], v[j * QDA_ROWS + lane], s);
      const double z = li[i] != 0.0 ? s / li[i] : 0.0;
      v[i * QDA_ROWS + lane] = z;
      q = fma(z, z, q);
    }
    const double sc = k0 - 0.5 * q;
    if (sc > best) { second = best; best = sc; arg = c; }
    else if (sc > second) second = sc;
  }
  if (ok) {
    if (pred) pred[r] = arg;
    if (gap) gap[r] = best - second;
    if (arg == label[r]) atomicAdd(correct + f, 1);  // integer count: exact in any order
  }
}

// ---- elastic-net logistic regression, one-vs-rest.  Problem p = (fold pfold[p], positive class pos[p]); its training rows are the
// rows of every other fold; row r is positive when label[r] == pos[p].  w[p] = [coef (d), intercept] in the centred frame.
struct LogregProb {
  const double* A; int lda, D, n;
  const int* fold; const int* label;
  const int* pfold; const int* pos;  // [P]
  int P;
};

// per (row chunk, problem): partial loss and gradient of C * sum softplus(-s u), and the Hessian weights C sigma(u)(1-sigma(u)) of
// every row (0 for the problem's test fold)
constexpr int LR_ROWS = 256;
__global__ __launch_bounds__(256) void logreg_stats_kernel(const LogregProb pb, const double* __restrict__ W, double Cc,
                                                           const int* __restrict__ done, double* __restrict__ part,
                                                           double* __restrict__ hw) {
  __shared__ double red[256], wsh[160], cf[LR_ROWS];
  const int p = blockIdx.y;
  if (done[p]) return;
  const int D = pb.D;
  for (int j = threadIdx.x; j < D; j += 256) wsh[j] = W[(long long)p * D + j];
  __syncthreads();
  const int r = blockIdx.x * LR_ROWS + threadIdx.x;
  double loss = 0.0, coef = 0.0;
  if (r < pb.n) {
    double h = 0.0;
    if (pb.fold[r] != pb.pfold[p]) {
      const double* ar = pb.A + (long long)r * pb.lda;
      double u = 0.0;
      for (int j = 0; j < D; ++j) u = fma(ar[j], wsh[j], u);
      const double s = pb.label[r] == pb.pos[p] ? 1.0 : -1.0;
      loss = Cc * softplus_d(-s * u);
      coef = -Cc * s * sigmoid_d(-s * u);
      const double q = sigmoid_d(u);
      h = Cc * q * (1.0 - q);
    }
    hw[(long long)p * pb.n + r] = h;
  }
  cf[threadIdx.x] = coef;
  const int chunks = gridDim.x;
  double* pp = part + ((long long)p * chunks + blockIdx.x) * (D + 1);
  const double ls = block_sum_all<256>(loss, red);  // also orders the cf writes before the reads below
  if (threadIdx.x == 0) pp[D] = ls;
  const int r0 = blockIdx.x * LR_ROWS, nr = min(LR_ROWS, pb.n - r0);
  for (int j = threadIdx.x; j < D; j += 256) {
    double g = 0.0;
    for (int rr = 0; rr < nr; ++rr) g = fma(cf[rr], pb.A[(long long)(r0 + rr) * pb.lda + j], g);
    pp[j] = g;
  }
}

// One wave per problem.  Reduces the gradient, records the KKT residual; unless it is below tol (or kkt_only), solves the proximal
// Newton subproblem  min_v g.(v - w) + 1/2 (v - w)^T H (v - w) + rho |v_pen|_1  by cyclic coordinate descent on the LDS-resident
// Hessian H = Gram(hw) + alpha I_pen, and writes the direction v - w and the predicted decrease.
struct LogregState {
  double* W;       // [P][D]
  double* dir;     // [P][D]
  double* f0;      // [P] objective at W
  double* delta;   // [P] g.d + rho (|w + d|_1 - |w|_1)
  double* kkt;     // [P]
  double* g0;      // [P] max |gradient| at w = 0 (set on the first call)
  int* done;       // [P]
  int* iters;      // [P]
};

__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

__global__ __launch_bounds__(64) void logreg_newton_kernel(const LogregProb pb, LogregState st, const double* __restrict__ part, int chunks,
                                                           const double* __restrict__ H, double alpha, double rho, double tol,
                                                           int kkt_only, int max_sweeps) {
  extern __shared__ __attribute__((aligned(16))) double h[];  // [D][D]
  __shared__ double g[160], w[160], v[160], hd[160];
  const int p = blockIdx.x, lane = threadIdx.x, D = pb.D, pen = D - 1;  // the last coordinate is the intercept
  if (st.done[p]) return;
  double fpen = 0.0;
  for (int j = lane; j < D; j += 64) {
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s += part[((long long)p * chunks + c) * (D + 1) + j];
    const double wj = st.W[(long long)p * D + j];
    if (j < pen) { s += alpha * wj; fpen += 0.5 * alpha * wj * wj + rho * fabs(wj); }
    g[j] = s; w[j] = wj; v[j] = wj; hd[j] = 0.0;
  }
  double loss = 0.0;
  if (lane == 0)
    for (int c = 0; c < chunks; ++c) loss += part[((long long)p * chunks + c) * (D + 1) + D];
  fpen = wave_sum_d(fpen);
  loss = __shfl(loss, 0, 64);
  __syncthreads();
  double res = 0.0, gm = 0.0;
  for (int j = lane; j < D; j += 64) {
    double e;
    if (j == pen) e = fabs(g[j]);
    else if (w[j] > 0.0) e = fabs(g[j] + rho);
    else if (w[j] < 0.0) e = fabs(g[j] - rho);
    else e = fmax(fabs(g[j]) - rho, 0.0);
    res = fmax(res, e);
    gm = fmax(gm, fabs(g[j]));
  }
  res = wave_max_d(res);
  gm = wave_max_d(gm);
  if (lane == 0) {
    if (st.g0[p] < 0.0) st.g0[p] = gm;  // first call: w = 0
    st.kkt[p] = res;
    st.f0[p] = loss + fpen;
  }
  const double g0 = st.g0[p] < 0.0 ? gm : st.g0[p];
  if (res <= tol * g0 || kkt_only) {
    if (lane == 0 && res <= tol * g0) st.done[p] = 1;
    return;
  }
  const double* Hp = H + (long long)p * D * D;
  for (int e = lane; e < D * D; e += 64) {
    const int i = e / D, j = e % D;
    h[e] = Hp[e] + (i == j && i < pen ? alpha : 0.0);
  }
  __syncthreads();
  for (int sw = 0; sw < max_sweeps; ++sw) {
    double big = 0.0, vmax = 0.0;
    for (int j = 0; j < D; ++j) {
      const double hjj = h[j * D + j];
      const double vj = v[j], wj = w[j];
      const double bq = g[j] + hd[j] - hjj * (vj - wj);  // gradient of the model at v with coordinate j removed, about v_j = w_j
      double nv;
      if (j == pen) nv = wj - bq / hjj;
      else {
        const double z = hjj * wj - bq;  // minimise 1/2 hjj v^2 - z v + rho |v|
        nv = z > rho ? (z - rho) / hjj : (z < -rho ? (z + rho) / hjj : 0.0);
      }
      const double dl = nv - vj;
      __syncthreads();
      if (dl != 0.0) {
        for (int i = lane; i < D; i += 64) hd[i] = fma(h[j * D + i], dl, hd[i]);
        if (lane == 0) v[j] = nv;
      }
      __syncthreads();
      big = fmax(big, fabs(dl));
      vmax = fmax(vmax, fabs(nv));
    }
    if (big <= 1e-13 * fmax(vmax, 1e-300) || big == 0.0) break;
  }
  double dg = 0.0, dl1 = 0.0;
  for (int j = lane; j < D; j += 64) {
    const double dj = v[j] - w[j];
    st.dir[(long long)p * D + j] = dj;
    dg = fma(g[j], dj, dg);
    if (j < pen) dl1 += fabs(v[j]) - fabs(w[j]);
  }
  dg = wave_sum_d(dg);
  dl1 = wave_sum_d(dl1);
  if (lane == 0) st.delta[p] = dg + rho * dl1;
}

// line search: per (row chunk, problem) the data loss at w + t dir for t = 2^-k, k < LS_STEPS
constexpr int LS_STEPS = 12;
__global__ __launch_bounds__(256) void logreg_ls_kernel(const LogregProb pb, LogregState st, double Cc, double* __restrict__ part) {
  __shared__ double red[256], wsh[160], dsh[160];
  const int p = blockIdx.y;
  if (st.done[p]) return;
  const int D = pb.D;
  for (int j = threadIdx.x; j < D; j += 256) { wsh[j] = st.W[(long long)p * D + j]; dsh[j] = st.dir[(long long)p * D + j]; }
  __syncthreads();
  const int r = blockIdx.x * LR_ROWS + threadIdx.x;
  double u = 0.0, du = 0.0, s = 0.0;
  const bool ok = r < pb.n && pb.fold[r] != pb.pfold[p];
  if (ok) {
    const double* ar = pb.A + (long long)r * pb.lda;
    for (int j = 0; j < D; ++j) { u = fma(ar[j], wsh[j], u); du = fma(ar[j], dsh[j], du); }
    s = pb.label[r] == pb.pos[p] ? 1.0 : -1.0;
  }
  double t = 1.0;
  for (int k = 0; k < LS_STEPS; ++k, t *= 0.5) {
    const double l = ok ? Cc * softplus_d(-s * (u + t * du)) : 0.0;
    const double sum = block_sum_all<256>(l, red);
    if (threadIdx.x == 0) part[((long long)p * gridDim.x + blockIdx.x) * LS_STEPS + k] = sum;
  }
}

// one wave per problem: first t (largest) passing Armijo, then w += t dir
__global__ __launch_bounds__(64) void logreg_update_kernel(const LogregProb pb, LogregState st, const double* __restrict__ part, int chunks,
                                                           double alpha, double rho) {
  __shared__ double fl[LS_STEPS];
  const int p = blockIdx.x, lane = threadIdx.x, D = pb.D, pen = D - 1;
  if (st.done[p]) return;
  if (lane < LS_STEPS) {
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s += part[((long long)p * chunks + c) * LS_STEPS + lane];
    fl[lane] = s;
  }
  double t = 1.0, tk = 0.0;
  int chosen = -1;
  double bestf = st.f0[p];
  int bestk = -1;
  for (int k = 0; k < LS_STEPS; ++k, t *= 0.5) {
    double pen_t = 0.0;
    for (int j = lane; j < pen; j += 64) {
      const double x = st.W[(long long)p * D + j] + t * st.dir[(long long)p * D + j];
      pen_t += 0.5 * alpha * x * x + rho * fabs(x);
    }
    pen_t = wave_sum_d(pen_t);
    __syncthreads();
    const double ft = fl[k] + pen_t;
    if (ft < bestf) { bestf = ft; bestk = k; }
    if (ft <= st.f0[p] + 1e-4 * t * st.delta[p] + 1e-15 * fabs(st.f0[p])) { chosen = k; tk = t; break; }
  }
  if (chosen < 0 && bestk >= 0) { chosen = bestk; tk = ldexp(1.0, -bestk); }
  if (chosen >= 0)
    for (int j = lane; j < D; j += 64) st.W[(long long)p * D + j] += tk * st.dir[(long long)p * D + j];
  if (lane == 0) {
    st.iters[p] += 1;
    if (chosen < 0) st.done[p] = 2;  // no decrease along the direction: stalled at rounding level
  }
}

// logistic decision values of the test rows of fold f with its problems p in [pstart[f], pstart[f + 1]): argmax of w_p . a (first on
// a tie) -> class pos[p]; a fold with one problem is binary: decision > 0 -> pos[p], else neg[f] (sklearn's classes_[1] / [0])
__global__ __launch_bounds__(256) void logreg_score_kernel(const LogregProb pb, const double* __restrict__ W, const int* __restrict__ pstart,
                                                           const int* __restrict__ neg, const int* __restrict__ lo,
                                                           const int* __restrict__ hi, int* __restrict__ correct, int* __restrict__ pred) {
  const int f = blockIdx.y;
  const int r = lo[f] + blockIdx.x * 256 + threadIdx.x;
  if (r >= hi[f]) return;
  const double* ar = pb.A + (long long)r * pb.lda;
  const int p0 = pstart[f], p1 = pstart[f + 1];
  int arg = -1;
  double best = -INFINITY;
  for (int p = p0; p < p1; ++p) {
    const double* wc = W + (long long)p * pb.D;
    double u = 0.0;
    for (int j = 0; j < pb.D; ++j) u = fma(ar[j], wc[j], u);
    if (p1 - p0 == 1) { arg = u > 0.0 ? pb.pos[p] : neg[f]; break; }
    if (u > best || arg < 0) { best = u; arg = pb.pos[p]; }
  }
  if (pred) pred[r] = arg;
  if (arg == pb.label[r]) atomicAdd(correct + f, 1);
}

// masked MSE gradient of the cross-validated MLPs: member m trains on every row outside fold mfold[m]
__global__ __launch_bounds__(256) void cv_mse_grad_kernel(const float* const* __restrict__ outs, float* const* __restrict__ dpred, int n_members,
                                                          const int* __restrict__ mfold, const float* __restrict__ y, int ldy, int ny,
                                                          int ld, const int* __restrict__ fold, int n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)n * ny) return;
  const int r = (int)(i / ny), o = (int)(i - (long long)r * ny);
  const float t = y[(long long)r * ldy + o];
  for (int m = 0; m < n_members; ++m) {
    const float e = outs[m][(long long)r * ld + o] - t;
    dpred[m][(long long)r * ld + o] = fold[r] == mfold[m] ? 0.f : 2.f * e;
  }
}

static int lr_prob(LogregProb& pb, const double* A, int lda, int D, int n, const int* fold, const int* label, const int* pfold,
                   const int* pos, int P) {
  SVAE_REQUIRE(A && fold && label && pfold && pos && n > 0 && D >= 2 && D <= SVAE_CV_MAX_DIM + 1 && lda >= D && P >= 1 &&
                   P <= SVAE_CV_MAX_GROUPS, SVAE_ERR_ARG, "logreg: bad problem description (D=%d, P=%d)", D, P);
  pb.A = A; pb.lda = lda; pb.D = D; pb.n = n; pb.fold = fold; pb.label = label; pb.pfold = pfold; pb.pos = pos; pb.P = P;
  return SVAE_OK;
}

}  // namespace svae

using namespace svae;

extern "C" int svae_cv_center(const float* x, int ldx, int d, const float* y, int ldy, int ny, const int* perm, int n, double* mean,
                              double* A, int lda, void* stream) {
  SVAE_REQUIRE(x && perm && mean && A && n > 0 && d > 0 && d <= SVAE_CV_MAX_DIM && ldx >= d && ny >= 0 && ny <= SVAE_CV_MAX_TARGETS &&
                   (ny == 0 || (y && ldy >= ny)) && lda >= d + 1 + ny, SVAE_ERR_ARG, "cv_center: bad args (n=%d d=%d ny=%d lda=%d)", n, d, ny, lda);
  hipLaunchKernelGGL(cv_colmean_kernel, dim3(d + ny), dim3(256), 0, ST(stream), x, ldx, d, y, ldy, n, mean);
  if (int e = check_launch("cv_colmean")) return e;
  const long long tot = (long long)n * lda;
  hipLaunchKernelGGL(cv_center_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, ST(stream), x, ldx, d, y, ldy, ny, perm, n, mean,
                     A, lda);
  return check_launch("cv_center");
}

extern "C" int svae_cv_moments(const double* A, int lda, int D, const int* lo, const int* hi, int G, const double* w, long long ldw,
                               const int* skip, double* out, int ldo, void* stream) {
  SVAE_REQUIRE(A && lo && hi && out && D > 0 && D <= lda && D <= ldo && G >= 1 && G <= SVAE_CV_MAX_GROUPS, SVAE_ERR_ARG,
               "cv_moments: bad args (D=%d G=%d)", D, G);
  const int nt = (D + 15) / 16;
  hipLaunchKernelGGL(cv_gram_kernel, dim3(nt * (nt + 1) / 2, G), dim3(256), 0, ST(stream), A, lda, D, lo, hi, w, ldw, skip, out, ldo);
  return check_launch("cv_moments");
}

extern "C" int svae_spd_factor_solve_f64(const double* M, int ldm, long long strideM, int n, int batch, const double* B, int nrhs,
                                         long long strideB, double* L, double* X, double* logdet, int* rank, double rtol, void* stream) {
  SVAE_REQUIRE(M && n > 0 && n <= SVAE_CV_MAX_DIM && ldm >= n && strideM >= (long long)n * ldm && batch >= 1 && batch <= SVAE_CV_MAX_GROUPS &&
                   nrhs >= 0 && nrhs <= SVAE_CV_MAX_TARGETS && (!B || (X && nrhs > 0 && strideB >= (long long)n * nrhs)),
               SVAE_ERR_ARG, "spd_factor_solve_f64: bad args (n=%d batch=%d nrhs=%d)", n, batch, nrhs);
  const size_t smem = (size_t)(n * (n + 1) / 2 + n * (B ? nrhs : 0)) * sizeof(double);
  static DeviceOnce once;
  if (int e = allow_lds(spd_factor_solve_kernel, once, CV_LDS_MAX, "spd_factor_solve_f64")) return e;
  hipLaunchKernelGGL(spd_factor_solve_kernel, dim3(batch), dim3(256), smem, ST(stream), M, ldm, strideM, n, B, B ? nrhs : 0, strideB, L, X,
                     logdet, rank, rtol);
  return check_launch("spd_factor_solve_f64");
}

extern "C" int svae_cv_r2_stats(const double* A, int lda, int d, int ny, const int* lo, const int* hi, int folds, const double* beta,
                                const double* c0, const float* const* pred, int ldp, const double* ymean, double* stats, void* stream) {
  SVAE_REQUIRE(A && lo && hi && stats && d > 0 && d <= SVAE_CV_MAX_DIM && ny >= 1 && ny <= SVAE_CV_MAX_TARGETS && lda >= d + 1 + ny &&
                   folds >= 1 && folds <= SVAE_CV_MAX_FOLDS && ((beta && c0) || (pred && ymean && ldp >= ny)),
               SVAE_ERR_ARG, "cv_r2_stats: bad args");
  hipLaunchKernelGGL(cv_r2_kernel, dim3(folds, ny), dim3(256), 0, ST(stream), A, lda, d, ny, lo, hi, pred ? nullptr : beta, c0, pred, ldp,
                     ymean, stats);
  return check_launch("cv_r2_stats");
}

extern "C" int svae_cv_qda_score(const double* A, int lda, int d, int K, const int* lo, const int* hi, int folds, int max_rows,
                                 const double* mu, const double* L, int ldl, const double* cst, const int* label, int* correct, int* pred,
                                 double* gap, void* stream) {
  SVAE_REQUIRE(A && lo && hi && mu && L && cst && label && correct && d > 0 && d <= SVAE_CV_MAX_DIM && lda > d && ldl >= d && K >= 2 &&
                   K <= SVAE_CV_MAX_CLASSES && folds >= 1 && folds <= SVAE_CV_MAX_FOLDS && max_rows > 0,
               SVAE_ERR_ARG, "cv_qda_score: bad args");
  static DeviceOnce once;
  if (int e = allow_lds(cv_qda_kernel, once, CV_LDS_MAX, "cv_qda_score")) return e;
  hipLaunchKernelGGL(cv_qda_kernel, dim3((max_rows + QDA_ROWS - 1) / QDA_ROWS, folds), dim3(QDA_ROWS), (size_t)d * QDA_ROWS * sizeof(double),
                     ST(stream), A, lda, d, K, lo, hi, mu, L, ldl, cst, label, correct, pred, gap);
  return check_launch("cv_qda_score");
}

extern "C" int svae_logreg_stats(const double* A, int lda, int D, int n, const int* fold, const int* label, const int* pfold, const int* pos,
                                 int P, const double* W, double C, const int* done, double* part, double* hw, void* stream) {
  LogregProb pb;
  if (int e = lr_prob(pb, A, lda, D, n, fold, label, pfold, pos, P)) return e;
  SVAE_REQUIRE(W && done && part && hw, SVAE_ERR_ARG, "logreg_stats: null buffer");
  hipLaunchKernelGGL(logreg_stats_kernel, dim3((n + LR_ROWS - 1) / LR_ROWS, P), dim3(256), 0, ST(stream), pb, W, C, done, part, hw);
  return check_launch("logreg_stats");
}

extern "C" int svae_logreg_chunks(int n) { return (n + LR_ROWS - 1) / LR_ROWS; }

extern "C" int svae_logreg_newton(const double* A, int lda, int D, int n, const int* fold, const int* label, const int* pfold,
                                  const int* pos, int P, const double* part, const double* H, double* W, double* dir, double* f0,
                                  double* delta, double* kkt, double* g0, int* done, int* iters, double alpha, double rho, double tol,
                                  int kkt_only, int max_sweeps, void* stream) {
  LogregProb pb;
  if (int e = lr_prob(pb, A, lda, D, n, fold, label, pfold, pos, P)) return e;
  SVAE_REQUIRE(part && (H || kkt_only) && W && dir && f0 && delta && kkt && g0 && done && iters && max_sweeps > 0, SVAE_ERR_ARG,
               "logreg_newton: null buffer");
  LogregState st{W, dir, f0, delta, kkt, g0, done, iters};
  static DeviceOnce once;
  if (int e = allow_lds(logreg_newton_kernel, once, CV_LDS_MAX, "logreg_newton")) return e;
  hipLaunchKernelGGL(logreg_newton_kernel, dim3(P), dim3(64), (size_t)D * D * sizeof(double), ST(stream), pb, st, part,
                     (n + LR_ROWS - 1) / LR_ROWS, H, alpha, rho, tol, kkt_only, max_sweeps);
  return check_launch("logreg_newton");
}

extern "C" int svae_logreg_line_search(const double* A, int lda, int D, int n, const int* fold, const int* label, const int* pfold,
                                       const int* pos, int P, double* W, const double* dir, const double* f0, const double* delta,
                                       int* done, int* iters, double C, double alpha, double rho, double* part, void* stream) {
  LogregProb pb;
  if (int e = lr_prob(pb, A, lda, D, n, fold, label, pfold, pos, P)) return e;
  SVAE_REQUIRE(W && dir && f0 && delta && done && iters && part, SVAE_ERR_ARG, "logreg_line_search: null buffer");
  LogregState st{W, const_cast<double*>(dir), const_cast<double*>(f0), const_cast<double*>(delta), nullptr, nullptr, done, iters};
  const int chunks = (n + LR_ROWS - 1) / LR_ROWS;
  hipLaunchKernelGGL(logreg_ls_kernel, dim3(chunks, P), dim3(256), 0, ST(stream), pb, st, C, part);
  if (int e = check_launch("logreg_ls")) return e;
  hipLaunchKernelGGL(logreg_update_kernel, dim3(P), dim3(64), 0, ST(stream), pb, st, part, chunks, alpha, rho);
  return check_launch("logreg_update");
}

extern "C" int svae_logreg_score(const double* A, int lda, int D, int n, const int* fold, const int* label, const int* pfold, const int* pos,
                                 int P, const double* W, const int* pstart, const int* neg, const int* lo, const int* hi, int folds,
                                 int max_rows, int* correct, int* pred, void* stream) {
  LogregProb pb;
  if (int e = lr_prob(pb, A, lda, D, n, fold, label, pfold, pos, P)) return e;
  SVAE_REQUIRE(W && pstart && neg && lo && hi && correct && folds >= 1 && folds <= SVAE_CV_MAX_FOLDS && max_rows > 0, SVAE_ERR_ARG,
               "logreg_score: bad args");
  hipLaunchKernelGGL(logreg_score_kernel, dim3((max_rows + 255) / 256, folds), dim3(256), 0, ST(stream), pb, W, pstart, neg, lo, hi,
                     correct, pred);
  return check_launch("logreg_score");
}

extern "C" int svae_cv_mse_grad(const float* const* outs, float* const* dpred, int n_members, const int* mfold, const float* y, int ldy,
                                int ny, int ld, const int* fold, int n, void* stream) {
  SVAE_REQUIRE(outs && dpred && mfold && y && fold && n_members >= 1 && n_members <= SVAE_ENS_MEMBERS && ny >= 1 && ld >= ny && ldy >= ny &&
                   n > 0, SVAE_ERR_ARG, "cv_mse_grad: bad args");
  const long long tot = (long long)n * ny;
  hipLaunchKernelGGL(cv_mse_grad_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, ST(stream), outs, dpred, n_members, mfold, y,
                     ldy, ny, ld, fold, n);
  return check_launch("cv_mse_grad");
}
