// Gaussian hidden Markov model over the latents in time: the scaled forward-backward pass, parallel in time and exact (Sarkka and
// Garcia-Fernandez 2021, "Temporal parallelization of inference in hidden Markov models"), and Viterbi decoding.  fp64 throughout.
//
// Inputs: B [K][ldb] = the E-step's resp with unit weights (svae_gmm_estep_f64: every frame's column sums to 1, exact zeros allowed),
// lpn [n] its log scale, startprob [K], transmat A [K][K], and the host's segment table: every sequence is cut into segments of
// L = svae_hmm_segment(K) frames (the last one shorter), a segment never crosses a sequence boundary.
//   seg [nseg][4] = {first frame, frames, 1 for the first segment of its sequence, sequence}
//   seq [nseq][4] = {first segment, segments, first frame, frames}
// States are padded to KP = 16, 32 or 64 with zero rows and columns.  Four phases:
//   transfer  per segment g: T_g = prod_t A diag(b_t) (the first segment of a sequence starts with diag(b_1)), kept as R_g [KP][KP]
//             with one power-of-two scale per row: T_g[i][:] = 2^expo_g[i] R_g[i][:], row sums of R in [1, 2).  Every step is
//             R <- scale((R A) o b_t) with R A on the fp64 matrix cores.  The scale is a power of two, so scaling rounds nothing and
//             the exponent is an integer sum: the log scale of a row is exact.  A row whose sum is 0 stays 0 (expo = INT_MIN).
//             The product is formed transposed, S = R^T: S <- A^T S.  With lane l = 16 q + c the B operand of step m is
//             S[4 m + q][c] and register r of result tile rt is S[16 rt + 4 r + q][c]: the result registers ARE the next step's
//             operand (m = 4 rt + r), so a wave chains through its segment with no exchange and no barrier but the staging of b.
//   carry     per sequence, over its segments: the normalised forward vectors entering every segment and the normalised backward
//             vectors at every segment's last frame, combined relative to the largest exponent (ldexp: exact weights).
//   fill      per segment, the plain scaled recursion from its boundary vector: forward writes alpha and c, backward overwrites
//             alpha with gamma and accumulates the expected transition counts; a finish kernel adds the per-block partials in
//             block order and gives the log-likelihood and the start posteriors.
//   viterbi   one wave per sequence, sequential in time, byte back-pointers.
// No floating-point atomics, every sum in a fixed order, and the work of a segment depends on its own sequence only: the alpha,
// gamma and c of a sequence do not change by a bit when other sequences are added, removed or reordered.
#include "svae_internal.h"

#include "pair_tiles.h"  // double4_t, the matrix-core lane layout and #pragma clang fp contract(off)
#include "fixed_sum.h"   // block_sum_of: the order of the log-likelihood sum

namespace svae {

constexpr int HMM_TF = 32;   // frames of B staged per step of the transfer kernel
constexpr int HMM_FF = 16;   // frames staged per step of the fill kernels
constexpr int HMM_VF = 32;   // frames of logB staged per step of the Viterbi kernel
constexpr int HMM_VB = 256;  // frames of back-pointers staged per step of the backtrace
constexpr int HMM_CU = 16;   // entries of a transfer matrix a lane of the carry kernel loads at a time
constexpr int HMM_XI_BLOCKS = 1024;  // most blocks of the backward fill: each keeps one partial of the transition counts

__host__ __device__ inline int hmm_pad(int K) { return K <= 16 ? 16 : K <= 32 ? 32 : 64; }

// the workspace of one pass, carved from one buffer of doubles (svae_hmm_work)
struct HmmWork {
  double* R;       // [nseg][KP][KP]
  double* vstart;  // [nseg][KP] forward vector entering the segment
  double* wend;    // [nseg][KP] backward vector at the segment's last frame
  double* llseg;   // [nseg] sum of log c_t + lpn_t over the segment
  double* xipart;  // [xi blocks][KP][KP]
  int* expo;       // [nseg][KP]
};
inline int hmm_xi_blocks(int nseg) { return std::min(nseg, HMM_XI_BLOCKS); }
inline long long hmm_work_doubles(int KP, int nseg) {
  const long long s = nseg, kp = KP;
  return s * kp * kp + 2 * s * kp + s + (long long)hmm_xi_blocks(nseg) * kp * kp + (s * kp + 1) / 2;
}
inline HmmWork hmm_carve(double* w, int KP, int nseg) {
  const long long s = nseg, kp = KP;
  HmmWork k;
  k.R = w;
  k.vstart = k.R + s * kp * kp;
  k.wend = k.vstart + s * kp;
  k.llseg = k.wend + s * kp;
  k.xipart = k.llseg + s;
  k.expo = reinterpret_cast<int*>(k.xipart + (long long)hmm_xi_blocks(nseg) * kp * kp);
  return k;
}

// the frames of segment g, clipped to [0, n): a table that does not fit the arrays makes no access outside them
struct HmmSeg {
  int t0, len, first;
};
__device__ __forceinline__ HmmSeg hmm_seg(const int* __restrict__ seg, int g, int n) {
  HmmSeg s{seg[4 * g], seg[4 * g + 1], seg[4 * g + 2]};
  if (s.t0 < 0 || s.t0 >= n) s.len = 0;
  else s.len = max(0, min(s.len, n - s.t0));
  return s;
}

// frames [t, t + nf) of X [K][ld] into xs[f][j] (row stride KP + 1), zero for j >= K and f >= nf; coalesced along the frames
template <int KP, int F, int T>
__device__ __forceinline__ void hmm_stage(const double* __restrict__ X, long long ld, int K, long long t, int nf, double* xs) {
  for (int e = threadIdx.x; e < KP * F; e += T) {
    const int j = e / F, f = e - j * F;
    xs[f * (KP + 1) + j] = j < K && f < nf ? X[j * ld + t + f] : 0.0;
  }
}

// ---- transfer -------------------------------------------------------------------------------------------------------------------
template <int KP>
__global__ __launch_bounds__(KP * 4) void hmm_transfer_kernel(const double* __restrict__ B, long long ldb, int n, int K,
                                                              const double* __restrict__ A, const int* __restrict__ seg,
                                                              double* __restrict__ R, int* __restrict__ expo) {
  constexpr int NM = KP / 4, NT = KP / 16, LD = KP + 1;
  __shared__ double bs[HMM_TF * LD];
  const int g = blockIdx.x;
  const HmmSeg sg = hmm_seg(seg, g, n);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, c = lane & 15;
  const int i = 16 * wave + c;  // this lane's row of R
  // A^T as the A operand: tile rt, step ks holds A^T[16 rt + c][4 ks + q] = A[4 ks + q][16 rt + c]
  double at[NT][NM];
#pragma unroll
  for (int rt = 0; rt < NT; ++rt)
#pragma unroll
    for (int ks = 0; ks < NM; ++ks) {
      const int k = 4 * ks + q, j = 16 * rt + c;
      at[rt][ks] = k < K && j < K ? A[k * K + j] : 0.0;
    }
  double s[NM];  // s[m] = R[i][4 m + q]
#pragma unroll
  for (int m = 0; m < NM; ++m) s[m] = 4 * m + q == i ? 1.0 : 0.0;
  int e = 0;
  bool dead = false;
  for (int f0 = 0; f0 < sg.len; f0 += HMM_TF) {
    const int nf = min(HMM_TF, sg.len - f0);
    __syncthreads();
    hmm_stage<KP, HMM_TF, KP * 4>(B, ldb, K, (long long)sg.t0 + f0, nf, bs);
    __syncthreads();
    for (int f = 0; f < nf; ++f) {
      const double* bf = bs + f * LD + q;
      if (sg.first && f0 + f == 0) {
#pragma unroll
        for (int m = 0; m < NM; ++m) s[m] = s[m] * bf[4 * m];
      } else {
        double4_t acc[NT];
#pragma unroll
        for (int rt = 0; rt < NT; ++rt) acc[rt] = double4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int ks = 0; ks < NM; ++ks)
#pragma unroll
          for (int rt = 0; rt < NT; ++rt) acc[rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(at[rt][ks], s[ks], acc[rt], 0, 0, 0);
#pragma unroll
        for (int rt = 0; rt < NT; ++rt)
#pragma unroll
          for (int r = 0; r < 4; ++r) s[4 * rt + r] = acc[rt][r] * bf[16 * rt + 4 * r];
      }
      double sum = s[0];
#pragma unroll
      for (int m = 1; m < NM; ++m) sum = sum + s[m];
      sum = sum + __shfl_xor(sum, 16, 64);
      sum = sum + __shfl_xor(sum, 32, 64);
      if (sum > 0.0) {
        const int ex = ilogb(sum);
#pragma unroll
        for (int m = 0; m < NM; ++m) s[m] = ldexp(s[m], -ex);
        e += ex;
      } else {
        dead = true;
      }
    }
  }
  double* Rg = R + ((long long)g * KP + i) * KP + q;
#pragma unroll
  for (int m = 0; m < NM; ++m) Rg[4 * m] = dead ? 0.0 : s[m];
  if (q == 0) expo[(long long)g * KP + i] = dead || sg.len == 0 ? INT_MIN : e;
}

// ---- carry ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

// grid (sequence, direction), one wave: lane = state.  direction 0: vstart[g] for every segment of the sequence; 1: wend[g].
__global__ __launch_bounds__(64) void hmm_carry_kernel(const double* __restrict__ R, const int* __restrict__ expo, int KP, int K,
                                                       const int* __restrict__ seq, int nseg, const double* __restrict__ startprob,
                                                       double* __restrict__ vstart, double* __restrict__ wend) {
  const int lane = threadIdx.x;
  int g0 = seq[4 * blockIdx.x], cnt = seq[4 * blockIdx.x + 1];
  if (g0 < 0 || g0 >= nseg) return;
  cnt = min(cnt, nseg - g0);
  const bool in = lane < K;
  if (blockIdx.y == 0) {
    double v = in ? startprob[lane] : 0.0;
    for (int u = 0; u < cnt; ++u) {
      const long long g = g0 + u;
      if (lane < KP) vstart[g * KP + lane] = v;
      if (u == cnt - 1) break;
      const int ex = in ? expo[g * KP + lane] : INT_MIN;
      const bool live = v > 0.0 && ex != INT_MIN;
      const int me = wave_max_i(live ? ex : INT_MIN);
      const double wgt = live ? ldexp(v, max(ex - me, -4000)) : 0.0;
      const double* Rg = R + g * KP * KP + lane;
      double acc = 0.0;
      for (int i0 = 0; i0 < K; i0 += HMM_CU) {  // the loads of a chunk are issued together; the sum stays in state order
        double r[HMM_CU];
#pragma unroll
        for (int h = 0; h < HMM_CU; ++h) r[h] = in && i0 + h < K ? Rg[(long long)(i0 + h) * KP] : 0.0;
#pragma unroll
        for (int h = 0; h < HMM_CU; ++h) {
          const double wi = __shfl(wgt, i0 + h, 64);
          if (i0 + h < K) {
            const double p = wi * r[h];
            acc = acc + p;
          }
        }
      }
      const double tot = wave_sum_d(acc);
      v = tot > 0.0 ? acc / tot : 0.0;
    }
  } else {
    double w = in ? 1.0 / K : 0.0;
    for (int u = cnt - 1; u >= 0; --u) {
      const long long g = g0 + u;
      if (lane < KP) wend[g * KP + lane] = w;
      if (u == 0) break;
      const double* Rg = R + (g * KP + lane) * KP;
      double x = 0.0;
      for (int j0 = 0; j0 < K; j0 += HMM_CU) {
        double r[HMM_CU];
#pragma unroll
        for (int h = 0; h < HMM_CU; ++h) r[h] = in && j0 + h < K ? Rg[j0 + h] : 0.0;
#pragma unroll
        for (int h = 0; h < HMM_CU; ++h) {
          const double wj = __shfl(w, j0 + h, 64);
          if (j0 + h < K) {
            const double p = r[h] * wj;
            x = x + p;
          }
        }
      }
      const int ex = in ? expo[g * KP + lane] : INT_MIN;
      const bool live = x > 0.0 && ex != INT_MIN;
      const int me = wave_max_i(live ? ex : INT_MIN);
      const double y = live ? ldexp(x, max(ex - me, -4000)) : 0.0;
      const double tot = wave_sum_d(y);
      w = tot > 0.0 ? y / tot : 0.0;
    }
  }
}

// ---- fill -----------------------------------------------------------------------------------------------------------------------
// One wave per segment, lane = state j, column j of A in registers.  alpha_t = ((alpha_{t-1} A) o b_t) / c_t, c_t = its sum.
template <int KP>
__global__ __launch_bounds__(64) void hmm_forward_kernel(const double* __restrict__ B, long long ldb, const double* __restrict__ lpn,
                                                         int n, int K, const double* __restrict__ A, const int* __restrict__ seg,
                                                         const double* __restrict__ vstart, double* __restrict__ alpha,
                                                         double* __restrict__ cc, double* __restrict__ llseg) {
  constexpr int LD = KP + 1;
  __shared__ double bs[HMM_FF * LD], os[HMM_FF * LD];
  const int g = blockIdx.x, lane = threadIdx.x;
  const HmmSeg sg = hmm_seg(seg, g, n);
  double acol[KP];
#pragma unroll
  for (int i = 0; i < KP; ++i) acol[i] = i < K && lane < K ? A[i * K + lane] : 0.0;
  double a = lane < KP ? vstart[(long long)g * KP + lane] : 0.0;
  double ll = 0.0;
  for (int f0 = 0; f0 < sg.len; f0 += HMM_FF) {
    const int nf = min(HMM_FF, sg.len - f0);
    const long long tb = (long long)sg.t0 + f0;
    __syncthreads();
    hmm_stage<KP, HMM_FF, 64>(B, ldb, K, tb, nf, bs);
    const double lp = lane < nf ? lpn[tb + lane] : 0.0;
    __syncthreads();
    double cf = 0.0;  // lane f keeps c of frame f
    for (int f = 0; f < nf; ++f) {
      double pred;
      if (sg.first && f0 + f == 0) {
        pred = a;
      } else {
        pred = 0.0;
#pragma unroll
        for (int i = 0; i < KP; ++i) {
          const double p = __shfl(a, i, 64) * acol[i];
          pred = pred + p;
        }
      }
      const double u = lane < KP ? pred * bs[f * LD + lane] : 0.0;
      const double ct = wave_sum_d(u);
      a = ct > 0.0 ? u / ct : 0.0;
      if (lane < KP) os[f * LD + lane] = a;
      if (lane == f) cf = ct;
      const double lt = log(ct) + __shfl(lp, f, 64);
      ll = ll + lt;
    }
    if (lane < nf) cc[tb + lane] = cf;
    __syncthreads();
    for (int e = lane; e < KP * HMM_FF; e += 64) {
      const int j = e / HMM_FF, f = e - j * HMM_FF;
      if (j < K && f < nf) alpha[(long long)j * n + tb + f] = os[f * LD + j];
    }
  }
  if (lane == 0) llseg[g] = ll;
}

// Block b takes the segments b, b + grid, ... in that order; lane = state, row `lane` of A in registers (the recursion of beta) and
// column `lane` of the block's partial M[i][lane] = sum_t alpha_{t-1}(i) q_t(lane), q_t = b_t o beta_t / (c_t D_t), D_t = alpha_t . beta_t:
// the expected transition counts are A o sum of the M (the finish kernel).  gamma_t = alpha_t o beta_t / D_t overwrites alpha_t.
template <int KP>
__global__ __launch_bounds__(64) void hmm_backward_kernel(const double* __restrict__ B, long long ldb, int n, int K,
                                                          const double* __restrict__ A, const int* __restrict__ seg, int nseg,
                                                          const double* __restrict__ vstart, const double* __restrict__ wend,
                                                          const double* __restrict__ cc, double* __restrict__ alpha,
                                                          double* __restrict__ xipart) {
  constexpr int LD = KP + 1;
  __shared__ double bs[HMM_FF * LD], as[(HMM_FF + 1) * LD];
  const int lane = threadIdx.x;
  double arow[KP], M[KP];
#pragma unroll
  for (int j = 0; j < KP; ++j) {
    arow[j] = j < K && lane < K ? A[lane * K + j] : 0.0;
    M[j] = 0.0;
  }
  for (int g = blockIdx.x; g < nseg; g += gridDim.x) {
    const HmmSeg sg = hmm_seg(seg, g, n);
    if (sg.len == 0) continue;
    double beta = lane < KP ? wend[(long long)g * KP + lane] : 0.0;
    const int nblk = (sg.len + HMM_FF - 1) / HMM_FF;
    for (int blk = nblk - 1; blk >= 0; --blk) {
      const int f0 = blk * HMM_FF, nf = min(HMM_FF, sg.len - f0);
      const long long tb = (long long)sg.t0 + f0;
      __syncthreads();
      hmm_stage<KP, HMM_FF, 64>(B, ldb, K, tb, nf, bs);
      hmm_stage<KP, HMM_FF, 64>(alpha, n, K, tb, nf, as + LD);
      // the frame before the block: alpha of the previous frame, or the vector entering the segment
      if (lane < KP) as[lane] = f0 > 0 ? (lane < K ? alpha[(long long)lane * n + tb - 1] : 0.0) : vstart[(long long)g * KP + lane];
      const double cl = lane < nf ? cc[tb + lane] : 0.0;
      __syncthreads();
      for (int f = nf - 1; f >= 0; --f) {
        const bool has_prev = !(sg.first && f0 + f == 0);
        const double al = lane < KP ? as[(f + 1) * LD + lane] : 0.0;
        const double x = al * beta;
        const double D = wave_sum_d(x);
        if (lane < KP) as[(f + 1) * LD + lane] = D > 0.0 ? x / D : 0.0;
        const double y = lane < KP ? bs[f * LD + lane] * beta : 0.0;
        if (has_prev) {
          const double den = __shfl(cl, f, 64) * D;
          const double qv = den > 0.0 ? y / den : 0.0;
          const double ap = lane < KP ? as[f * LD + lane] : 0.0;
#pragma unroll
          for (int i = 0; i < KP; ++i) {
            const double p = __shfl(ap, i, 64) * qv;
            M[i] = M[i] + p;
          }
        }
        if (f0 + f > 0) {  // beta of the frame before, inside the segment
          double nb = 0.0;
#pragma unroll
          for (int j = 0; j < KP; ++j) {
            const double p = arow[j] * __shfl(y, j, 64);
            nb = nb + p;
          }
          const double tot = wave_sum_d(nb);
          beta = tot > 0.0 ? nb / tot : 0.0;
        }
      }
      __syncthreads();
      for (int e = lane; e < KP * HMM_FF; e += 64) {
        const int j = e / HMM_FF, f = e - j * HMM_FF;
        if (j < K && f < nf) alpha[(long long)j * n + tb + f] = as[(f + 1) * LD + j];
      }
    }
  }
  double* o = xipart + (long long)blockIdx.x * KP * KP + lane;
  if (lane < KP)
#pragma unroll
    for (int i = 0; i < KP; ++i) o[i * KP] = M[i];
}

// block i < K: Xi[i][j] = A[i][j] * (sum of the partials in block order).  block K: loglik = sum of llseg (compensated per thread,
// then a tree: fixed_sum.h), start_post[j] = sum over the sequences, in order, of gamma at their first frame.
__global__ __launch_bounds__(256) void hmm_finish_kernel(const double* __restrict__ xipart, int nb, int KP, int K,
                                                         const double* __restrict__ A, const double* __restrict__ llseg, int nseg,
                                                         const int* __restrict__ seq, int nseq, const double* __restrict__ gamma, int n,
                                                         double* __restrict__ Xi, double* __restrict__ start_post,
                                                         double* __restrict__ loglik) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  if ((int)blockIdx.x < K) {
    const int i = blockIdx.x;
    if (t < K) {
      double s = 0.0;
      for (int b = 0; b < nb; ++b) s = s + xipart[((long long)b * KP + i) * KP + t];
      Xi[i * K + t] = A[i * K + t] * s;
    }
    return;
  }
  const double ll = block_sum_of<256>(llseg, nseg, red);
  if (t == 0) loglik[0] = ll;
  if (t < K) {
    double s = 0.0;
    for (int q = 0; q < nseq; ++q) {
      const int t0 = seq[4 * q + 2];
      if (t0 >= 0 && t0 < n) s = s + gamma[(long long)t * n + t0];
    }
    start_post[t] = s;
  }
}

// transmat[i] = max(Xi[i] + tprior - 1, 0) / its sum (in state order); a row whose sum is 0 keeps its values; startprob alike
__global__ __launch_bounds__(64) void hmm_update_kernel(const double* __restrict__ Xi, const double* __restrict__ start_post, int K,
                                                        double tprior, double sprior, double* __restrict__ transmat,
                                                        double* __restrict__ startprob) {
  const int i = threadIdx.x;
  if (i < K) {
    double tot = 0.0;
    for (int j = 0; j < K; ++j) tot = tot + fmax(Xi[i * K + j] + (tprior - 1.0), 0.0);
    if (tot > 0.0)
      for (int j = 0; j < K; ++j) transmat[i * K + j] = fmax(Xi[i * K + j] + (tprior - 1.0), 0.0) / tot;
  }
  if (i == 0) {
    double tot = 0.0;
    for (int j = 0; j < K; ++j) tot = tot + fmax(start_post[j] + (sprior - 1.0), 0.0);
    if (tot > 0.0)
      for (int j = 0; j < K; ++j) startprob[j] = fmax(start_post[j] + (sprior - 1.0), 0.0) / tot;
  }
}

// ---- Viterbi --------------------------------------------------------------------------------------------------------------------
// One wave per sequence, lane = state j: delta_t(j) = max_i (delta_{t-1}(i) + logA[i][j]) + logB[j][t], the first largest i kept as
// the back-pointer bp[t][j]; then the path is read backwards from the first largest final state.  Only adds and compares.
__global__ __launch_bounds__(64) void hmm_viterbi_kernel(const double* __restrict__ log_start, const double* __restrict__ log_trans,
                                                         const double* __restrict__ logB, int n, int K, const int* __restrict__ seq,
                                                         unsigned char* __restrict__ bp, int* __restrict__ states,
                                                         double* __restrict__ logprob) {
  constexpr int LD = SVAE_HMM_MAX_STATES + 1;
  __shared__ double la[SVAE_HMM_MAX_STATES * LD], ls[HMM_VF * LD];
  static_assert(HMM_VF * LD * sizeof(double) >= (size_t)HMM_VB * SVAE_HMM_MAX_STATES, "the back-pointers reuse the logB stage");
  const int lane = threadIdx.x;
  int t0 = seq[4 * blockIdx.x + 2], len = seq[4 * blockIdx.x + 3];
  if (t0 < 0 || t0 >= n) return;
  len = min(len, n - t0);
  if (len <= 0) return;
  for (int e = lane; e < K * K; e += 64) la[(e / K) * LD + e % K] = log_trans[e];
  double delta = 0.0;
  for (int f0 = 0; f0 < len; f0 += HMM_VF) {
    const int nf = min(HMM_VF, len - f0);
    const long long tb = (long long)t0 + f0;
    __syncthreads();
    for (int e = lane; e < K * HMM_VF; e += 64) {
      const int j = e / HMM_VF, f = e - j * HMM_VF;
      if (f < nf) ls[f * LD + j] = logB[(long long)j * n + tb + f];
    }
    __syncthreads();
    for (int f = 0; f < nf; ++f) {
      const double lb = lane < K ? ls[f * LD + lane] : 0.0;
      if (f0 + f == 0) {
        delta = lane < K ? log_start[lane] + lb : -INFINITY;
        continue;
      }
      double best = -INFINITY;
      int arg = 0;
      for (int i = 0; i < K; ++i) {
        const double cnd = __shfl(delta, i, 64) + la[i * LD + (lane < K ? lane : 0)];
        if (cnd > best) { best = cnd; arg = i; }
      }
      delta = lane < K ? best + lb : -INFINITY;
      if (lane < K) bp[(tb + f) * K + lane] = (unsigned char)arg;
    }
  }
  double best = __shfl(delta, 0, 64);
  int st = 0;
  for (int j = 1; j < K; ++j) {
    const double dj = __shfl(delta, j, 64);
    if (dj > best) { best = dj; st = j; }
  }
  if (lane == 0) {
    logprob[blockIdx.x] = best;
    states[(long long)t0 + len - 1] = st;
  }
  // frames t0 + len - 1 down to t0 + 1: states[t - 1] = bp[t][states[t]], the back-pointers staged HMM_VB frames at a time
  unsigned char* bq = reinterpret_cast<unsigned char*>(ls);
  for (int hi = len; hi > 1; hi -= HMM_VB) {
    const int lo = max(1, hi - HMM_VB);  // frames [lo, hi) of the sequence
    __syncthreads();
    const unsigned char* src = bp + ((long long)t0 + lo) * K;
    for (int e = lane; e < (hi - lo) * K; e += 64) bq[e] = src[e];
    __syncthreads();
    if (lane == 0)
      for (int f = hi - 1; f >= lo; --f) {
        st = bq[(f - lo) * K + st];
        states[(long long)t0 + f - 1] = st;
      }
    st = __shfl(st, 0, 64);
  }
}

static int hmm_args(const char* what, int n, int K, const int* seg, int nseg, const int* seq, int nseq) {
  SVAE_REQUIRE(n >= 1 && n < (1 << 26) && K >= 1 && K <= SVAE_HMM_MAX_STATES && seg && seq && nseq >= 1 && nseg >= nseq && nseg <= n,
               SVAE_ERR_ARG, "%s: bad args (n=%d K=%d nseg=%d nseq=%d)", what, n, K, nseg, nseq);
  return SVAE_OK;
}

}  // namespace svae

using namespace svae;

extern "C" int svae_hmm_padded(int K) { return K >= 1 && K <= SVAE_HMM_MAX_STATES ? hmm_pad(K) : 0; }

extern "C" int svae_hmm_segment(int K) {
  if (K < 1 || K > SVAE_HMM_MAX_STATES) return 0;
  const int KP = hmm_pad(K);
  return KP == 16 ? SVAE_HMM_SEGMENT_16 : KP == 32 ? SVAE_HMM_SEGMENT_32 : SVAE_HMM_SEGMENT_64;
}

extern "C" int svae_hmm_xi_blocks(int nseg) { return nseg >= 1 ? hmm_xi_blocks(nseg) : 0; }

extern "C" long long svae_hmm_work(int K, int nseg) {
  if (K < 1 || K > SVAE_HMM_MAX_STATES || nseg < 1) return 0;
  return hmm_work_doubles(hmm_pad(K), nseg);
}

extern "C" int svae_hmm_transfer_f64(const double* B, long long ldb, int n, int K, const double* transmat, const int* seg, int nseg,
                                     const int* seq, int nseq, double* work, void* stream) {
  if (int e = hmm_args("hmm_transfer_f64", n, K, seg, nseg, seq, nseq)) return e;
  SVAE_REQUIRE(B && transmat && work && ldb >= n, SVAE_ERR_ARG, "hmm_transfer_f64: null buffer or ldb < n");
  const int KP = hmm_pad(K);
  const HmmWork w = hmm_carve(work, KP, nseg);
  if (KP == 16) hipLaunchKernelGGL(hmm_transfer_kernel<16>, dim3(nseg), dim3(64), 0, ST(stream), B, ldb, n, K, transmat, seg, w.R, w.expo);
  else if (KP == 32) hipLaunchKernelGGL(hmm_transfer_kernel<32>, dim3(nseg), dim3(128), 0, ST(stream), B, ldb, n, K, transmat, seg, w.R, w.expo);
  else hipLaunchKernelGGL(hmm_transfer_kernel<64>, dim3(nseg), dim3(256), 0, ST(stream), B, ldb, n, K, transmat, seg, w.R, w.expo);
  return check_launch("hmm_transfer");
}

extern "C" int svae_hmm_carry_f64(int n, int K, const double* startprob, const int* seg, int nseg, const int* seq, int nseq,
                                  double* work, void* stream) {
  if (int e = hmm_args("hmm_carry_f64", n, K, seg, nseg, seq, nseq)) return e;
  SVAE_REQUIRE(startprob && work, SVAE_ERR_ARG, "hmm_carry_f64: null buffer");
  const int KP = hmm_pad(K);
  const HmmWork w = hmm_carve(work, KP, nseg);
  hipLaunchKernelGGL(hmm_carry_kernel, dim3(nseq, 2), dim3(64), 0, ST(stream), w.R, w.expo, KP, K, seq, nseg, startprob, w.vstart, w.wend);
  return check_launch("hmm_carry");
}

extern "C" int svae_hmm_fill_f64(const double* B, long long ldb, const double* lpn, int n, int K, const double* transmat, const int* seg,
                                 int nseg, const int* seq, int nseq, double* work, double* gamma, double* c, double* Xi,
                                 double* start_post, double* loglik, void* stream) {
  if (int e = hmm_args("hmm_fill_f64", n, K, seg, nseg, seq, nseq)) return e;
  SVAE_REQUIRE(B && lpn && transmat && work && gamma && c && Xi && start_post && loglik && ldb >= n && gamma != B, SVAE_ERR_ARG,
               "hmm_fill_f64: null buffer, ldb < n or gamma == B");
  const int KP = hmm_pad(K), nb = hmm_xi_blocks(nseg);
  const HmmWork w = hmm_carve(work, KP, nseg);
#define SVAE_HMM_FILL(KP_)                                                                                                          \
  do {                                                                                                                              \
    hipLaunchKernelGGL(hmm_forward_kernel<KP_>, dim3(nseg), dim3(64), 0, ST(stream), B, ldb, lpn, n, K, transmat, seg, w.vstart,    \
                       gamma, c, w.llseg);                                                                                          \
    if (int e = check_launch("hmm_forward")) return e;                                                                              \
    hipLaunchKernelGGL(hmm_backward_kernel<KP_>, dim3(nb), dim3(64), 0, ST(stream), B, ldb, n, K, transmat, seg, nseg, w.vstart,    \
                       w.wend, c, gamma, w.xipart);                                                                                 \
    if (int e = check_launch("hmm_backward")) return e;                                                                             \
  } while (0)
  if (KP == 16) SVAE_HMM_FILL(16);
  else if (KP == 32) SVAE_HMM_FILL(32);
  else SVAE_HMM_FILL(64);
#undef SVAE_HMM_FILL
  hipLaunchKernelGGL(hmm_finish_kernel, dim3(K + 1), dim3(256), 0, ST(stream), w.xipart, nb, KP, K, transmat, w.llseg, nseg, seq, nseq,
                     gamma, n, Xi, start_post, loglik);
  return check_launch("hmm_finish");
}

extern "C" int svae_hmm_update_f64(const double* Xi, const double* start_post, int K, double transmat_prior, double startprob_prior,
                                   double* transmat, double* startprob, void* stream) {
  SVAE_REQUIRE(Xi && start_post && transmat && startprob && K >= 1 && K <= SVAE_HMM_MAX_STATES && transmat_prior >= 0.0 &&
                   startprob_prior >= 0.0, SVAE_ERR_ARG, "hmm_update_f64: bad args (K=%d)", K);
  hipLaunchKernelGGL(hmm_update_kernel, dim3(1), dim3(64), 0, ST(stream), Xi, start_post, K, transmat_prior, startprob_prior, transmat,
                     startprob);
  return check_launch("hmm_update");
}

extern "C" int svae_hmm_viterbi(const double* log_startprob, const double* log_transmat, const double* logB, int n, int K,
                                const int* seq, int nseq, unsigned char* backptr, int* states, double* logprob, void* stream) {
  SVAE_REQUIRE(log_startprob && log_transmat && logB && seq && backptr && states && logprob && n >= 1 && n < (1 << 26) && K >= 1 &&
                   K <= SVAE_HMM_MAX_STATES && nseq >= 1 && nseq <= n, SVAE_ERR_ARG, "hmm_viterbi: bad args (n=%d K=%d nseq=%d)", n, K,
               nseq);
  hipLaunchKernelGGL(hmm_viterbi_kernel, dim3(nseq), dim3(64), 0, ST(stream), log_startprob, log_transmat, logB, n, K, seq, backptr,
                     states, logprob);
  return check_launch("hmm_viterbi");
}
