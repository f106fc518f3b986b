/*
 * scrubvae_hip.h -- C ABI of libscrubvae_hip.so (gfx950 / MI355X).
 *
 * The reference (tdunnlab/scrubvae) is pure Python and has NO FFI/plugin boundary
 * (SURVEY.md 8b); this ABI is new and sits underneath the reference's Python API.  Each
 * entry point states which reference op (file:line under /root/reference) it replaces.
 * The Python binding is scrubvae_amd/_lib.py (ctypes); INTEGRATION.md shows the stub a
 * maintainer of the reference would add.
 *
 * Conventions
 *  - plain C, no C++/torch types; every pointer is a DEVICE pointer unless noted;
 *  - the caller owns every buffer (inputs, outputs, workspaces); the callee never
 *    allocates, frees, synchronises or keeps a pointer past return;
 *  - all launches go to the hipStream_t passed as `void* stream`;
 *  - return value: 0 = ok, negative = svae_status error; svae_last_error() gives text;
 *  - activations are channels-last ("NLC"): row r = b*L + l, `ld` floats per row, the
 *    first C entries valid, entries C..Cp-1 (Cp = channels padded to a multiple of 16)
 *    are zero.  This makes the reference's [B,W,C] <-> [B,C,W] moveaxis copies
 *    (residual.py:450,479) free;
 *  - conv / linear weights are "TIO": w[tap][c_in_pad][c_out_pad], pads zero.
 *    Conv1d weight [Cout,Cin,k]      -> w[t][ci][co] = W[co][ci][t]
 *    ConvTranspose1d weight [Cin,Cout,k] -> w[t][ci][co] = W[ci][co][t]
 *    Linear weight [out,in]          -> w[0][in][out].
 */
#ifndef SCRUBVAE_HIP_H
#define SCRUBVAE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  SVAE_OK = 0,
  SVAE_ERR_SHAPE = -1,     /* inconsistent / unsupported shape */
  SVAE_ERR_ALIGN = -2,     /* pointer or leading dimension not 16-byte aligned */
  SVAE_ERR_WORKSPACE = -3, /* workspace too small */
  SVAE_ERR_LAUNCH = -4,    /* hipLaunch failed (see svae_last_error) */
  SVAE_ERR_ARG = -5        /* null pointer / bad enum */
} svae_status;

#define SVAE_MAX_TAPS 128
#define SVAE_MAX_JOINTS 32
#define SVAE_MAX_CHAINS 8
#define SVAE_MAX_CHAIN_LEN 8

int svae_version(void);
/* copies the calling thread's last error text into buf (NUL-terminated) */
void svae_last_error(char* buf, size_t n);

/* ------------------------------------------------------------------ conv / linear --- */
typedef struct {
  int batch;
  int l_in, l_out;   /* sequence lengths; l_out must match the PyTorch formula */
  int c_in, c_out;   /* padded channel counts, multiples of 16 */
  int ld_in, ld_out; /* floats per activation row (>= c_in / c_out, multiple of 4) */
  int kernel, stride, padding, dilation;
  int transposed;    /* 0 = nn.Conv1d, 1 = nn.ConvTranspose1d; Linear: kernel=1,l=1 */
  /* tuning overrides (results are bit-identical for every tile: the per-output summation
   * order over K does not depend on it).  tile[kind] = BM*1000+BN with BM,BN in {64,128}, or
   * 0 for the built-in heuristic; kind 0 fwd, 1 dgrad, 2 wgrad.  Adding 1000000 (fwd/dgrad) selects
   * the LDS-DMA staging variant (global_load_lds, XOR-swizzled LDS image).  tile[2] = 1 selects the tap-fused
   * small-weight gradient kernel (64x64 tiles, all taps of a tile in one workgroup). */
  int tile[3];
  /* 1: the conv's input is nn.Upsample(scale_factor=2, mode="linear", align_corners=False) of a [batch, l_in / 2, c_in] tensor
   * (the decoder's skip path, residual.py:160): l_in stays the UPSAMPLED length, x points to the half-length tensor, and the
   * forward (svae_conv_fwd_split*, halo tile codes 8 / 9) and weight-gradient (svae_conv_wgrad_split, all-taps tile codes) kernels
   * blend its rows while they stage the operand -- the upsampled tensor need not exist.  nn.Conv1d with stride 1 only; the fp32
   * entry points and the other tile codes return SVAE_ERR_SHAPE.  The data-gradient entry points ignore the flag: dx is the
   * gradient with respect to the upsampled input (fold it back with svae_upsample2_bwd).  0 elsewhere. */
  int up2;
} svae_conv_desc;

/* y[b,lo,:] (+)= bias + sum_t x[b,li(lo,t),:] @ w[t]     (residual.py:79-109,137-170,
 * 198,219-222,264,286: every nn.Conv1d / nn.ConvTranspose1d / nn.Linear of the trunk).
 * fp32 MFMA (v_mfma_f32_32x32x2_f32) implicit GEMM, 128xBN tiles. */
int svae_conv_fwd(const svae_conv_desc* d, const float* x, const float* w, const float* bias,
                  float* y, int accumulate, void* stream);
/* dx (+)= conv_backward_input(dy, w)      (autograd of the above) */
int svae_conv_dgrad(const svae_conv_desc* d, const float* dy, const float* w, float* dx,
                    int accumulate, void* stream);
/* The same two calls with an optional split-K workspace (the Linear heads: few output tiles, long reduction): partial
 * tiles go to `ws` (svae_conv_splitk_workspace(d, kind) bytes, kind 0 = fwd / 1 = dgrad; 0 = no split for this
 * geometry) and are summed in a fixed order.  ws == NULL or too small: identical to the calls above. */
size_t svae_conv_splitk_workspace(const svae_conv_desc* d, int kind);
int svae_conv_fwd_ws(const svae_conv_desc* d, const float* x, const float* w, const float* bias, float* y,
                     int accumulate, void* ws, size_t ws_bytes, void* stream);
int svae_conv_dgrad_ws(const svae_conv_desc* d, const float* dy, const float* w, float* dx, int accumulate,
                       void* ws, size_t ws_bytes, void* stream);
/* dw (+)= conv_backward_weight(x, dy); split-K partial slabs in `ws`, reduced in a fixed
 * order (bit-reproducible).  db (optional, may be NULL) (+)= column sums of dy. */
size_t svae_conv_wgrad_workspace(const svae_conv_desc* d);
int svae_conv_wgrad(const svae_conv_desc* d, const float* x, const float* dy, float* dw,
                    float* db, void* ws, size_t ws_bytes, int accumulate, void* stream);

/* ---- split-bf16 variants of the three contractions (scrubvae_amd/csrc/gemm_bf16s.hip) -----
 * Same geometry, layouts and results contract as svae_conv_fwd / _dgrad / _wgrad, but the
 * products run on the bf16 matrix cores: each fp32 operand is split into `pieces` (1..3) bf16
 * pieces and the cross products with i + j < pieces are accumulated in fp32.  pieces = 3 is
 * fp32-accurate (dropped terms O(2^-24)); 2 -> O(2^-16); 1 = plain bf16 operands.
 * `wsplit` (svae_conv_split_bytes(d) bytes, caller-owned) holds the weight pieces written by
 * svae_conv_split_weights from the fp32 master weights w[tap][c_in][c_out]; refresh it whenever
 * the weights change.  d->tile[0..1]: V*1000000 + BM*1000 + BN, V = kernel variant (0 .. 19, 29: the list is next to
 * split_gather_geometry in scrubvae_amd/csrc/split_gather.h, the one place that resolves a code).  d->tile[2] for the split
 * weight gradient: V*1000000 + BM*1000 + BN with V a bit set -- 1: single LDS buffer,
 * 2: XCD-aware workgroup order, 4: all taps of a tile in one workgroup (contiguous 5 / 6-tap geometries, 2 pieces;
 * SVAE_ERR_SHAPE otherwise), 8: that kernel on the 16x16x32 MFMA shape, 16: the taps folded into the dY columns (transposed
 * convs) or into the X channel rows (convs) of the tile -- one tile padding for all taps.  Results do not depend on the tile code beyond
 * the summation order (deterministic for a given code). */
size_t svae_conv_split_bytes(const svae_conv_desc* d);
int svae_conv_split_weights(const svae_conv_desc* d, const float* w, void* wsplit, void* stream);
/* the same for up to SVAE_MAX_SPLIT_TASKS convolutions in one launch (all layers of a model, once per step) */
#define SVAE_MAX_SPLIT_TASKS 48
typedef struct {
  const float* w;   /* fp32 master weights [kernel][c_in][c_out] (padded channel counts) */
  void* wsplit;     /* svae_conv_split_bytes() bytes */
  int kernel, c_in, c_out;
} svae_split_task;
int svae_conv_split_weights_batched(const svae_split_task* tasks, int n, void* stream);
int svae_conv_fwd_split(const svae_conv_desc* d, const float* x, const void* wsplit, const float* bias,
                        float* y, int accumulate, int pieces, void* stream);
/* pieces = SVAE_PIECES_F16X2 (forward only): two fp16 pieces per operand (22 of the 24 significand bits), three cross products --
 * fp32-class accuracy (~2^-22 per product) at half the matrix-core work of pieces = 3; the weights' fp16 planes (of 2^10 w, undone in
 * the epilogue) are part of the svae_conv_split_weights output.  Operands beyond fp16's range (|x| > 65504) saturate. */
#define SVAE_PIECES_F16X2 22
/* The same launch with the train-mode BatchNorm statistics of the conv output fused into its epilogue (nn.BatchNorm1d right
 * behind the conv, residual.py:88,112,146,173): bn_part[tile][2][c_out] = per-column (sum y, sum y^2) over the valid rows of
 * row tile `tile`, y = the value written (bias and, with accumulate, the previous content included) -- the layout of
 * svae_bn_stats_partial with svae_conv_fwd_stats_tiles(d) in place of svae_bn_chunks(rows); feed it to
 * svae_bn_stats_finalize / svae_bn_reduce_partials.  Removes one full read of the conv output per BatchNorm.
 * bn_pivot [c_out] (NULL: zeros): the sums are taken about it, (sum (y - p), sum (y - p)^2), as in svae_bn_stats_partial; the
 * finalize call must be given the same pivot, and must come after this launch in stream order where it overwrites the pivot. */
int svae_conv_fwd_stats_tiles(const svae_conv_desc* d);
int svae_conv_fwd_split_stats(const svae_conv_desc* d, const float* x, const void* wsplit, const float* bias,
                              float* y, int accumulate, int pieces, float* bn_part, const float* bn_pivot, void* stream);
/* The same launch for a descriptor with up2 = 1 (conv behind nn.Upsample(x2, linear): residual.py:153-170) that additionally
 * writes the upsampled operand rows it blends to up_out[batch * l_in][c_in] (each row once; ld_in == c_in) -- the tensor the
 * conv's weight gradient reads in the backward pass -- so that no separate svae_upsample2_fwd launch (one more read of x) is
 * needed.  up_out = NULL: nothing is written; bn_part as above (NULL: off). */
int svae_conv_fwd_split_up2(const svae_conv_desc* d, const float* x, const void* wsplit, const float* bias,
                            float* y, int accumulate, int pieces, float* bn_part, float* up_out, const float* bn_pivot,
                            void* stream);
int svae_conv_dgrad_split(const svae_conv_desc* d, const float* dy, const void* wsplit, float* dx,
                          int accumulate, int pieces, void* stream);
/* The same launch when dx is the gradient with respect to the OUTPUT of a BatchNorm1d + PReLU / Tanh stage (the `add` / `residual.1-2`
 * pairs of residual.py:88-89,112-113,146-147,173-174) whose saved input is f->x ([rows][ld_in], the layout of dx): the first pass of that
 * stage's backward -- (sum du, sum du * xhat) per channel and the PReLU slope's partial, what svae_affine_prelu_bwd_partial computes
 * from a re-read of dx and x -- comes out of the epilogue: part[tile][2][c_in], dalpha_part[2 * (tile * col_blocks + col_block)] =
 * the (hi, lo) float pair of the tile's fp64 slope partial (2 * tiles * col_blocks floats), with
 * svae_conv_dgrad_stats_tiles(d, &col_blocks) row tiles.  scale / shift (and mean / rstd) NULL: bare activation; alpha NULL: tanh.
 * With accumulate the sums are those of the accumulated value (the launch that writes dx last carries them). */
typedef struct {
  const float* x;
  const float* scale; const float* shift; const float* mean; const float* rstd;
  const float* alpha;
  float* part;
  float* dalpha_part;   /* may be NULL (tanh) */
} svae_bn_bwd_fuse;
int svae_conv_dgrad_stats_tiles(const svae_conv_desc* d, int* col_blocks);
int svae_conv_dgrad_split_bn(const svae_conv_desc* d, const float* dy, const void* wsplit, float* dx,
                             int accumulate, int pieces, const svae_bn_bwd_fuse* f, void* stream);
int svae_conv_wgrad_split(const svae_conv_desc* d, const float* x, const float* dy, float* dw,
                          float* db, void* ws, size_t ws_bytes, int accumulate, int pieces, void* stream);
/* introspection: tile, kernel variant and (halo variant) image rows of the split fwd (0) / dgrad (1) launch */
int svae_conv_split_tile(const svae_conv_desc* d, int kind, int* bm, int* bn, int* variant, int* rmax);
/* how the split fwd / dgrad kernels move their output tiles: 1 (default) = 16-byte loads and stores behind an LDS transposition
 * in the kernels built with it, 0 = one dword per accumulator register.  Same values either way (A/B runs, tests).
 * Process-wide; returns the previous setting */
int svae_conv_epilogue_wide(int on);

/* introspection: the (BM, BN) workgroup tile the dispatcher uses; kind 0 fwd, 1 dgrad, 2 wgrad */
int svae_conv_tile(const svae_conv_desc* d, int kind, int* bm, int* bn);

/* ------------------------------------------------------------- elementwise / norm --- */
/* E0: ResVAE.normalize_root + input pack (residual.py:428-431,438-451).
 * x6d [rows, 6J], root [rows,3], arena = HOST pointer to 6 floats [2,3] (may be NULL:
 * no root channels)
 * -> x_in [rows, ld] = [x6d | 2(root-a0)/(a1-a0)-1 | 0 pad]. */
int svae_pack_input(const float* x6d, const float* root, const float* arena, float* x_in,
                    long long rows, int n_joints, int ld, void* stream);

/* Train-mode BatchNorm1d statistics (residual.py:88,112,146,173): per-channel partial
 * sums over row chunks.  part [n_chunks][2][C] (sum, sum of squares) of x - pivot; n_chunks returned by
 * svae_bn_chunks(rows).  pivot [C] (NULL: zeros) is any per-channel value near the batch mean, e.g. the running mean: each
 * partial is an fp32 sum, so the rounding of the sum of squares scales with var + (mean - pivot)^2, and the variance
 * E[(x-p)^2] - E[x-p]^2 keeps its relative accuracy only while |mean - pivot| is not large against the standard deviation. */
int svae_bn_chunks(long long rows);
int svae_bn_stats_partial(const float* x, long long rows, int C, int ld, float* part, const float* pivot, void* stream);
/* Finalize: sums over chunks in fixed order (fp64), `count` = rows over ALL ranks (the
 * caller all-reduces `part` reduced to [2][C] for sync-BN, see svae_bn_reduce_partials).
 * Writes scale = gamma*rstd, shift = beta-mean*scale, saves mean/rstd, updates running
 * stats with momentum (unbiased var) when running_mean != NULL.  pivot [C] (NULL: zeros) is the pivot the sums were taken
 * about: mean = pivot + S/N, var = Q/N - (S/N)^2.  It may be running_mean itself: each channel's pivot is read before
 * its running mean is written, by the same thread. */
int svae_bn_reduce_partials(const float* part, int n_chunks, int C, float* sums /*[2][C]*/, void* stream);
int svae_bn_finalize(const float* sums, double count, int C, const float* gamma, const float* beta,
                     float eps, float momentum, float* running_mean, float* running_var,
                     float* mean, float* rstd, float* scale, float* shift, const float* pivot, void* stream);
/* single-rank fast path: svae_bn_reduce_partials + svae_bn_finalize in one launch; also
 * increments *num_batches_tracked (int64, may be NULL) */
int svae_bn_stats_finalize(const float* part, int n_chunks, double count, int C, const float* gamma,
                           const float* beta, float eps, float momentum, float* running_mean,
                           float* running_var, long long* num_batches_tracked, float* mean, float* rstd,
                           float* scale, float* shift, const float* pivot, void* stream);
/* backward: chunk partials -> sums[2][C], plus (+)= dgamma, dbeta (from the sums) and dalpha
 * (from dalpha_part[n_parts]); any of the three may be NULL */
int svae_bn_bwd_reduce(const float* part, int n_chunks, int C, float* sums, float* dgamma, float* dbeta,
                       float* dalpha, const float* dalpha_part, int n_parts, int accumulate, void* stream);
/* eval mode: scale/shift from running stats */
int svae_bn_eval_coeffs(int C, const float* gamma, const float* beta, float eps,
                        const float* running_mean, const float* running_var,
                        float* scale, float* shift, void* stream);
/* y = PReLU(x*scale+shift) with scalar slope *alpha (nn.PReLU(), residual.py:89,113,147,
 * 174,199).  scale/shift NULL => identity affine (conv_in's bare PReLU).  alpha NULL in this and the
 * two backward calls => tanh instead of PReLU (model.activation == "tanh", nn.Tanh() at the same
 * lines): act'(u) = 1 - tanh(u)^2, no slope gradient (dalpha_part is written as zeros). */
int svae_affine_prelu_fwd(const float* x, const float* scale, const float* shift, const float* alpha,
                          float* y, long long rows, int C, int ld, void* stream);
/* backward, pass 1: partial column sums  part[n_chunks][2][C] = (sum du, sum du*xhat),
 * dalpha_part[2 * (chunk * ceil(C/64) + column block)] = (hi, lo) float pair of sum dy*u*[u<=0] formed in fp64 (the slope's gradient
 * sums ~1e6 cancelling terms; 2 * n_chunks * ceil(C/64) floats; the reduction calls below sum all n_parts floats in fp64);
 * du = dy*(u>0?1:alpha), u = x*scale+shift. */
int svae_affine_prelu_bwd_partial(const float* dy, const float* x, const float* scale, const float* shift,
                                  const float* mean, const float* rstd, const float* alpha,
                                  long long rows, int C, int ld, float* part, float* dalpha_part,
                                  void* stream);
/* pass 2: dx = gamma*rstd*(du - s0/count - xhat*s1/count)  (train-mode BN backward);
 * with sums == NULL: dx = du*scale (eval BN / bare PReLU: scale may be NULL => 1).
 * Also (+)= dgamma, dbeta from sums and dalpha from the n_parts entries of dalpha_part when those
 * pointers are given. */
int svae_affine_prelu_bwd_apply(const float* dy, const float* x, const float* scale, const float* shift,
                                const float* mean, const float* rstd, const float* gamma,
                                const float* alpha, const float* sums, double count,
                                float* dx, long long rows, int C, int ld,
                                float* dgamma, float* dbeta, float* dalpha,
                                const float* dalpha_part, int n_parts, int accumulate_param_grads,
                                void* stream);   /* n_parts = entries of dalpha_part */
/* the same pass, also leaving the column sums of dx -- the bias gradient of the conv(s) in front of the stage (autograd of the
 * reference's `bias=True` convs) -- as per-workgroup partials colsum_part[svae_affine_prelu_colsum_rows(rows, C)][C] for
 * svae_colsum_from_partials (needs C / 4 a power of two <= 256; colsum_part may be NULL) */
int svae_affine_prelu_colsum_rows(long long rows, int C);
int svae_affine_prelu_bwd_apply_colsum(const float* dy, const float* x, const float* scale, const float* shift,
                                       const float* mean, const float* rstd, const float* gamma,
                                       const float* alpha, const float* sums, double count,
                                       float* dx, long long rows, int C, int ld,
                                       float* dgamma, float* dbeta, float* dalpha,
                                       const float* dalpha_part, int n_parts, int accumulate_param_grads,
                                       float* colsum_part, void* stream);

/* nn.Upsample(scale_factor=2, mode="linear", align_corners=False) (residual.py:160) */
int svae_upsample2_fwd(const float* x, float* y, int batch, int l_in, int C, int ld, void* stream);
int svae_upsample2_bwd(const float* dy, float* dx, int batch, int l_in, int C, int ld, int accumulate,
                       void* stream);

/* ------------------------------------------------------------------- latent heads --- */
/* E4+S1+L3 (diag): mu/sigma/dmu/dsigma are [B, ldm] (ldm >= z); eps is [B, z]; h [B, ld]: mu at columns [0,z), raw at [raw_off, raw_off+z); sigma = softplus(raw) (residual.py:60-68),
 * z = mu + sigma*eps (residual.py:305-316; eps NULL => z = mu, eval mode),
 * kl_part[blocks] = per-block partial of -0.5*sum(1+2log(sigma)-mu^2-sigma^2)
 * (losses.py:138-146, before the /B). */
int svae_heads_diag_fwd(const float* h, int ld, const float* eps, float* mu, float* sigma, float* z,
                        int ldz, float* kl_part, int batch, int zdim, int raw_off, int ldm, void* stream);
int svae_heads_blocks(int batch, int zdim);
/* dh = [dmu_total | draw]: dmu_total = dmu + dz + kl_scale*mu,
 * draw = (dz*eps + dsigma + kl_scale*(sigma-1/sigma)) * sigmoid(raw). */
int svae_heads_diag_bwd(const float* h, int ld, const float* eps, const float* sigma,
                        const float* dz, int lddz, const float* dmu, const float* dsigma, float kl_scale,
                        float* dh, int batch, int zdim, int raw_off, int ldm, void* stream);

/* Full-Cholesky variant (model.diag = False; CholeskyL residual.py:39-68): raw holds the
 * z(z+1)/2 lower-triangle entries in torch.tril_indices order at h[:, raw_off:], softplus on
 * the diagonal; L [B,z,z] is written densely (zeros above the diagonal); z = L eps + mu;
 * kl_part as above with diag(L L^T) = row sums of squares. */
int svae_heads_tril_fwd(const float* h, int ld, const float* eps, float* mu, int ldm, float* L, float* z,
                        int ldz, float* kl_part, int batch, int zdim, int raw_off, void* stream);
/* dlv (optional, [B,z]): upstream gradient w.r.t. log diag(L L^T) (total-correlation loss) */
int svae_heads_tril_bwd(const float* h, int ld, const float* eps, const float* L, const float* dz, int lddz,
                        const float* dmu, int ldm, float kl_scale, const float* dlv, float* dh, int batch,
                        int zdim, int raw_off, void* stream);

/* model.prior = "beta" (residual.py:223-239,301-302,328-331,453-456; losses.py:198-206).  h [B, ld]: raw alpha at columns [0, z), raw beta
 * at [raw_off, raw_off + z).  Forward: alpha = softplus(raw) + 1, beta likewise, mu = (alpha - 1 + 1e-8) / (alpha + beta - 2 + 2e-8) * 2 - 1
 * (all [B, ldm]); kl_part[svae_heads_blocks] = partials of sum KL(Beta(alpha, beta) || Beta(1, 1)) (before the / B).  The draw
 * x ~ Beta(alpha, beta) is the CALLER's (z = 2 x - 1; torch's sampler as RNG plumbing, injected in parity tests).  Backward:
 * dh = [d raw_alpha | d raw_beta] from dz [B, lddz] (gradient wrt z, through the implicit reparameterisation of x: the reference's
 * Beta.rsample = Dirichlet rsample with torch._dirichlet_grad, restated in the kernel), dmu [B, ldm] (seed on mu; may be NULL) and
 * kl_scale * d KL. */
int svae_heads_beta_fwd(const float* h, int ld, float* alpha, float* beta, float* mu, int ldm, float* kl_part, int batch, int zdim,
                        int raw_off, void* stream);
int svae_heads_beta_bwd(const float* h, int ld, const float* x, const float* alpha, const float* beta, int ldm, const float* dz,
                        int lddz, const float* dmu, float kl_scale, float* dh, int batch, int zdim, int raw_off, void* stream);

/* L5: total_correlation (losses.py:41-101), beta-TCVAE minibatch estimator, z detached.
 * svae_tc_logvar: lv[b,l] = log diag(L L^T) from sigma (diag; 2 log sigma) or a dense L.
 * svae_tc_fwd: loss[j] (TC = mean_j), plus the two log-sum-exp tables the backward reuses
 * (lse_l [B,z], lse_a [B]).  svae_tc_bwd: d_mu[i,:] += weight * dTCsum/dmu, d_lv = weight *
 * dTCsum/dlv (weight = loss_scale / B).  O(B^2 z), nothing of size [B,B,z] is materialised. */
int svae_tc_logvar(const float* sigma, int lds, const float* L, float* lv, int batch, int zdim, void* stream);
int svae_tc_fwd(const float* z, int ldz, const float* mu, int ldm, const float* lv, int batch, int zdim,
                float* lse_l, float* lse_a, float* loss, void* stream);
int svae_tc_bwd(const float* z, int ldz, const float* mu, int ldm, const float* lv, int batch, int zdim,
                const float* lse_l, const float* lse_a, float weight, float* d_mu, int ldd, float* d_lv,
                int ldv, const float* sigma /* optional: emit d/dsigma = d/dlv*2/sigma */, int lds, void* stream);

/* ----------------------------------------------------------------- pose-loss tail --- */
typedef struct {
  int n_joints;
  int n_chains;
  int chain_len[SVAE_MAX_CHAINS];
  int chain[SVAE_MAX_CHAINS][SVAE_MAX_CHAIN_LEN];
} svae_tree;

/* D3 tail + K1 + K3 + L1 + L2 fused, one pass over the decoder output:
 *   y [rows, ld] conv_out pre-activation -> x_hat = tanh(y)            (residual.py:291)
 *   x6d_hat [rows, 6J], root_hat [rows,3] = inv_normalize_root(...)     (residual.py:479-489)
 *   pose_hat = fwd_kin_cont6d_torch(x6d_hat, tree, offsets, root=0, eps=1e-8)
 *                                                     (dataset.py:83-116, quaternion.py:337-353)
 *   jpe partial  = sum (target_pose - pose_hat)^2     (losses.py:148-171, before /(B*3*J))
 *   root partial = sum (root_hat - root)^2            (losses.py:216-219, before /B)
 *   dy [rows, ld] = jpe_scale * d jpe_sum/dy + root_scale * d root_sum/dy   (analytic
 *   reverse-mode through the kinematic chains, the 6D->matrix map and tanh).
 * `arena` is a HOST pointer to 6 floats (NULL: no root channels).
 * input_is_pre_tanh = 0: `y` already holds x_hat (no tanh, dy = d/dx_hat): the stand-alone
 * mpjpe_loss form.
 * pose_out (optional) [rows, J, 3] receives pose_hat (used to synthesise target_pose and by
 * the evaluation path).
 * loss_part [blocks][2].  dy may be NULL (eval: forward only).  ext_dx6d/ext_droot
 * (optional) are extra upstream grads w.r.t. x6d_hat/root_hat added before the tanh
 * backward (used by the rotation loss and by autograd callers). */
int svae_tail_blocks(long long rows);
int svae_pose_tail(const float* y, int ld, const float* offsets, const float* target_pose,
                   const float* root, const float* arena, const svae_tree* tree,
                   float jpe_scale, float root_scale, const float* ext_dx6d, const float* ext_droot,
                   float* x6d_hat, float* root_hat, float* loss_part, float* dy, float* pose_out,
                   long long rows, int input_is_pre_tanh, void* stream);

/* L4: stable_rotation_loss (losses.py:123-136, rotation_conversion.py:469-488):
 * part[blocks] partial sums of 2*asin(clamp(|R(x_hat)-R(x)|_F/2^1.5)); dx6d_hat (optional)
 * = scale * d/dx_hat. n = rows*J six-vectors. */
int svae_rot_loss(const float* x6d, const float* x6d_hat, float scale, float* part, float* dx6d_hat,
                  long long n, void* stream);
int svae_rot_blocks(long long n);

/* Bias gradients of a whole step in two launches: out_t[c] (+)= sum over rows of x_t[:, c]. */
#define SVAE_MAX_COLSUM_TASKS 48
typedef struct {
  const float* x; /* [rows, ld] */
  float* out;     /* [C] */
  long long rows;
  int C, ld;
} svae_colsum_task;
/* out[c] (+)= sum over rows of part[rows][C] for up to SVAE_MAX_COLSUM_TASKS partial arrays in one launch (fp64, fixed order) */
typedef struct {
  const float* part;
  float* out;
  int rows, C;
} svae_colsum_part_task;
int svae_colsum_from_partials(const svae_colsum_part_task* tasks, int n, int accumulate, void* stream);
size_t svae_colsum_batched_workspace(const svae_colsum_task* tasks, int n);
int svae_colsum_batched(const svae_colsum_task* tasks, int n, void* ws, size_t ws_bytes, int accumulate,
                        void* stream);

/* --------------------------------------------------------- preprocessing --- */
/* inv_kin (dataset.py:11-46, forward_indices=[1,0]) + root centring / "midfwd" re-orientation (dataset.py:385-404)
 * + quaternion_to_cont6d (quaternion.py:291-334) + get_segment_len (dataset.py:279-296) + heading of the window's
 * middle frame (dataset.py:234-241,258-265), one thread per frame.
 *   pose [frames][J][3] (frames = windows*window, windowed order), unit_offset = HOST pointer [J][3]
 *   -> x6d [frames][J][6]; offsets [frames][J][3], root [frames][3], heading [frames/window][2] (each may be NULL).
 * truncate_len != 0 reproduces the reference when OFFSET is an integer array (segment lengths truncated toward
 * zero on assignment, dataset.py:289-294).  Frame 0 gets the identity root quaternion (dataset.py:31). */
int svae_inv_kin(const float* pose, const float* unit_offset_host, const svae_tree* tree, int window, int midfwd,
                 int centre_root, int truncate_len, float* x6d, float* offsets, float* root, float* heading,
                 long long frames, void* stream);
/* get_speed_parts (dataset.py:133-163) + limbs averaged (:373-375): pose [windows][W][J][3] -> out [windows][3].
 * parts_host: the part joint lists concatenated (HOST), part_len_host[n_parts] their lengths (HOST). */
int svae_speed_parts(const float* pose, const int* parts_host, const int* part_len_host, int n_parts, int W, int J,
                     float* out, long long windows, void* stream);

/* ---- Training batches from a resident recording ----
 * The two kernels above, reading their windows out of a raw recording pose [frames][J][3] that stays in device memory:
 * batch row b is the recording's frames starts[b] .. starts[b]+window-1 (starts: DEVICE int64 [batch], each in
 * [0, frames-window]; the kernels clamp a start outside that range into it, so they never read outside the recording).
 * The outputs are written in batch layout -- x6d [batch][window][J][6]; offsets [batch][window][J][3], root [batch][window][3],
 * heading [batch][2] (each may be NULL) -- and the gathered [batch][window][J][3] pose tensor is never materialised.  The
 * arithmetic per frame and per window is svae_inv_kin's / svae_speed_parts' own code, so on the same windows the results are
 * bit-identical; the yaw, centring and "midfwd" turn come from the row's own middle frame starts[b] + window/2.
 * index: NULL or DEVICE int64 [batch], the dataset index of each row.  The identity root quaternion that svae_inv_kin gives
 * frame 0 of its array goes to frame 0 of the row with index[b] == 0, wherever it sits in the batch (no row with index NULL).
 * Rejections (SVAE_ERR_ARG for null pose / starts / x6d / out, else SVAE_ERR_SHAPE; nothing launched): window < 1 (W < 2 for the
 * speeds), frames < window, batch < 0, and the joint / chain / part limits of the two entry points above.  batch == 0: no-op. */
int svae_window_batch(const float* pose, long long frames, const long long* starts, const long long* index,
                      const float* unit_offset_host, const svae_tree* tree, int window, int midfwd, int centre_root,
                      int truncate_len, float* x6d, float* offsets, float* root, float* heading, long long batch,
                      void* stream);
/* out [batch][3] as svae_speed_parts; mean_host / std_host: HOST float[3] each or both NULL; given, out = (speed - mean) / std
 * in fp32, in that order (the reference's in-place normalisation of avg_speed_3d). */
int svae_window_speed_parts(const float* pose, long long frames, const long long* starts, const int* parts_host,
                            const int* part_len_host, int n_parts, int W, int J, const float* mean_host,
                            const float* std_host, float* out, long long batch, void* stream);

/* ------------------------------------------------------------- MLP-ensemble scrubber heads --- */
/* G2/G3/A1: MLPEnsemble (disentangle.py:583-632) = up to four small MLPs (Linear/ReLU chains of <= 3 Linears) on the same input,
 * as ONE launch forward and one (+ a reduction launch) backward; GRScrubber (:635-660) feeds it mu, AdvNetScrubber (:663-684)
 * cat([mu;mu],[v;v_shuffle]).  The input is assembled in the kernel: columns [0,n0) = src0[b][0..n0), columns [n0,n0+n1) =
 * src1[b][0..n1); halves = 2 appends a second copy of the batch (rows batch..2*batch-1) whose column `shuf_col` of src1 is read
 * from row perm[b] (AdvNetScrubber.shuffle, :678-684; perm = int64 device array) or, when shuf_vals != NULL, is shuf_vals[b].  Weights are TIO Linear weights
 * [K][N] (K, N = features padded to multiples of 16, pads zero) -- the model's own parameter storage, nothing repacked. */
#define SVAE_ENS_MEMBERS 4
#define SVAE_ENS_MAX_LAYERS 3
typedef struct {
  const float* w;   /* [K][N] */
  const float* b;   /* [N] */
  float* dw;        /* gradient destinations; NULL (both) = frozen parameters: no weight gradients for this member */
  float* db;
  int K, N;
} svae_ens_layer;
typedef struct {
  svae_ens_layer layer[SVAE_ENS_MAX_LAYERS];
  int n_layers;
  float* out;          /* fwd: [rows][N_last] pre-activation outputs of the last Linear (rows = batch * halves) */
  const float* d_out;  /* bwd: gradient with respect to `out`, same shape */
} svae_ens_member;
typedef struct {
  svae_ens_member member[SVAE_ENS_MEMBERS];
  int n_members;
  const float* src0; int ld0, n0;
  const float* src1; int ld1, n1;
  const long long* perm; int shuf_col;
  int batch, halves;
  const float* shuf_vals;  /* optional [batch]: the shuffled column's values for the second copy, used instead of src1[perm[b]]
                            * (data parallel: the permutation runs over the GLOBAL batch, the values come from other ranks) */
} svae_ens_desc;
int svae_ens_fwd(const svae_ens_desc* d, void* stream);
/* Backward: recomputes the hidden activations, then writes parameter gradients (dw/db of every non-frozen member; summed over
 * row tiles in a fixed order, no atomics) and the input gradient: d_src0[b][k] += coef * sum over members and halves of
 * d/d input[b][k] for k < n0 (d_src0 may be NULL), and, when gx_raw != NULL, gx_raw[row][k] = sum over members for all rows and
 * all K_0 input columns.  coef = -alpha is the gradient reversal (disentangle.py:541-556). */
size_t svae_ens_bwd_workspace(const svae_ens_desc* d);
int svae_ens_bwd(const svae_ens_desc* d, float* d_src0, int ld_d, float coef, float* gx_raw, void* ws, size_t ws_bytes,
                 int accumulate_param_grads, void* stream);
/* Losses of all members in one launch (losses.py:267-309).  kind 0: sum((out - target)^2) over [rows][C]; 1: CrossEntropy(sum) vs
 * int32 labels; 2: the adversarial net's CrossEntropy applied to softmax(out) with class = (row >= rows/2) (double-softmax quirk,
 * disentangle.py:675 + losses.py:304-307; C = 2).  outs / dpred / loss_w / grad_s are HOST arrays of n_members entries:
 * part[m * nb + j] = loss_w[m] * (sum over the rows of block j), nb = svae_rowloss_blocks(rows); dpred[m] (may be NULL) =
 * grad_s[m] * d loss_m / d out_m. */
int svae_ens_loss(int kind, const float* const* outs, float* const* dpred, const float* loss_w, const float* grad_s, int n_members,
                  const float* target, int ld_t, const int* labels, int rows, int C, int ld, float* part, void* stream);

/* ------------------------------------------------------------------------- optimizer --- */
/* O1: torch.optim.AdamW / Adam step over one flat fp32 buffer (trainer.py:60-65,165).
 * step_t = 1-based step count; decoupled != 0 => AdamW. grad_scale multiplies g first
 * (1/world_size after a sum all-reduce, or the clip coefficient). */
int svae_adam_step(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1,
                   float beta2, float eps, float weight_decay, int step_t, int decoupled,
                   float grad_scale, void* stream);
/* hipGraph-capturable form: hyper (device, 4 floats) = {lr, lr/(1-beta1^t), 1/sqrt(1-beta2^t), t}.  The caller writes
 * lr (stream-ordered) when the schedule changes it; svae_adam_advance, captured in front of the step, does t += 1 and
 * derives the two bias-correction terms ON THE DEVICE, so queued replays never race a host buffer. */
int svae_adam_step_dev(float* p, const float* g, float* m, float* v, long long n, const float* hyper,
                       float beta1, float beta2, float eps, float weight_decay, int decoupled,
                       float grad_scale, void* stream);
int svae_adam_advance(float* hyper, float beta1, float beta2, void* stream);
/* torch.nn.utils.clip_grad_norm_ (trainer.py:164): g *= min(1, max_norm / (sqrt(*sumsq) + 1e-6)); sumsq = device scalar
 * holding the sum of squares of ALL gradients.  Returns without touching g when the clip does not bite (a NaN norm poisons every
 * gradient, as torch's clamp(NaN, max=1) * g does).  norm_out (may be NULL): the total norm sqrt(*sumsq), the function's return value
 * in torch. */
int svae_clip_grads(float* g, long long n, const float* sumsq, float max_norm, float* norm_out, void* stream);

/* Batched small dense solves for the streaming scrubbers (reference: MovingAvgLeastSquares.forward,
 * src/scrubvae/model/disentangle.py:466-486 -- torch.linalg.solve(Sxx + l2 I, Sxy) twice per step; direct_lsq_loss,
 * src/scrubvae/train/losses.py:173-179).  System s: (A[s] + diag(diag)) X[s] = B[s], A row-major [n][n], B / X row-major
 * [n][nrhs], strides in elements between systems; diag may be NULL; n, nrhs <= 64.  LU with partial pivoting, fp32. */
int svae_small_solve(const float* A, long long strideA, const float* diag, const float* B, long long strideB, float* X,
                     long long strideX, int n, int nrhs, int batch, void* stream);
/* Gaussian log-likelihoods of the streaming quadratic discriminants (reference: QuadraticDiscriminantFilter.cgll,
 * src/scrubvae/model/disentangle.py:129-134 -- torch.linalg.solve + torch.logdet per (mean, covariance) pair, 4 pairs per class
 * and step, evaluate_loss :186-232).  x [batch][ldx] (first n columns), mean [pairs][n], S [pairs][n][n] row-major, n <= 64:
 *   ll[p][b] = -0.5 (logdet S_p + r^T S_p^-1 r),  r = x_b - mean_p   (NaN for det < 0, +inf for a singular S, as torch.logdet gives)
 *   grad[p][b][:] = d ll[p][b] / d x_b = -0.5 (S_p^-1 + S_p^-T) r     (grad may be NULL) */
int svae_gauss_ll(const float* x, int ldx, const float* mean, const float* S, float* ll, float* grad, int batch, int n, int pairs,
                  void* stream);
/* Kernel-density mutual information between latent means and conditioning variables (reference: MutInfoEstimator.forward,
 * src/scrubvae/model/disentangle.py:278-317; loss `mcmi`, src/scrubvae/train/losses.py:221-225).  x [batch][ldx] (zx columns),
 * y [batch][ldy] (dy columns), centres xs [centres][zx], ys [centres][dy]; var: one value (var_per_centre = 0, "sphere",
 * logAx[1]) or [centres][zx] ("diagonal", logAx[centres]); zx, dy <= 64.
 *   val[b] = lse_s a_s - lse_s b_s - lse_s c_s  (the reference's three un-normalised log-sum-exps; the loss is mean_b val[b])
 *   grad[b][:] = d val[b] / d x_b               (grad may be NULL) */
int svae_kde_mi(const float* x, int ldx, const float* y, int ldy, const float* xs, const float* ys, const float* var,
                int var_per_centre, const float* logAx, float logAy, float gamma, float* val, float* grad, int batch, int centres,
                int zx, int dy, void* stream);
/* sum of squares partials for clip_grad_norm_ (trainer.py:164): part[svae_sumsq_blocks(n)] */
int svae_sumsq_blocks(long long n);
int svae_sumsq_partial(const float* x, long long n, float* part, void* stream);
/* out[0..k) = sum over rows of part[rows][k] in fixed order (fp64 accumulate) * scale */
int svae_reduce_rows(const float* part, int rows, int k, float scale, float* out, int accumulate, void* stream);
/* the same with one scale per column (host array scales[k], k <= 8): the jpe and root terms -- summed by one tail launch,
 * normalised by 1 / (B 3 J) and 1 / B (losses.py:171,216-219) -- in one launch */
int svae_reduce_rows_scaled(const float* part, int rows, int k, const float* scales, float* out, void* stream);
/* L6 (losses.py:320-322): out[0] = sum_i weights[i] * terms[i] over the loss terms' device scalars, in index order (fp32, like the
 * reference's running total); weights = the loss_scale entries on the host, n <= SVAE_MAX_LOSS_TERMS; terms with weight 0 are
 * skipped as in the reference */
#define SVAE_MAX_LOSS_TERMS 48
int svae_loss_total(const float* terms, const float* weights, int n, float* out, void* stream);

/* ----------------------------------------------------------- small elementwise ops --- */
int svae_relu_fwd(const float* x, float* y, long long n, void* stream);
int svae_relu_bwd(const float* dy, const float* y, float* dx, long long n, void* stream);
int svae_axpy(float a, const float* x, float* y, long long n, void* stream); /* y += a*x */
int svae_fill(float* x, float v, long long n, void* stream);
/* G3: sum of squared error vs target, rows x C (pred ld, target ld_t); part[blocks];
 * dpred (optional) = scale*2*(pred-target) */
int svae_mse_sum(const float* pred, int ld, const float* target, int ld_t, int rows, int C, float scale,
                 float* part, float* dpred, void* stream);
int svae_rowloss_blocks(int rows);
/* CrossEntropyLoss(reduction="sum") on logits with integer labels (losses.py:271-273) */
int svae_ce_sum(const float* logits, int ld, const int* labels, int rows, int C, float scale,
                float* part, float* dlogits, void* stream);
/* A1: softmax then CrossEntropyLoss(sum) on the softmax OUTPUT against one-hot class
 * `cls(row) = row >= rows/2` (double softmax, disentangle.py:675 + losses.py:297-307) */
int svae_double_softmax_ce_sum(const float* logits, int ld, int rows, float scale, float* part,
                               float* dlogits, void* stream);

/* ------------------------------------------------------ latent decodability (csrc/decode.hip) --- */
/* Cross-validated decoders of train()'s test metrics (reference: linear_rand_cv, log_class_rand_cv, qda_rand_cv, mlp_rand_cv,
 * src/scrubvae/eval/metrics.py:231-329; called at src/scrubvae/train/trainer.py:416-506).  All statistics are fp64.
 * Rows are the downsampled latents sorted by group (fold, then class); perm[i] = source row of sorted row i.  A fold's rows,
 * or a (fold, class) group's rows, are one contiguous range [lo[g], hi[g]) of the sorted order (lo / hi: device int arrays). */
#define SVAE_CV_MAX_DIM 128      /* latent width d */
#define SVAE_CV_MAX_TARGETS 8    /* regression outputs ny */
#define SVAE_CV_MAX_CLASSES 64
#define SVAE_CV_MAX_FOLDS 10
#define SVAE_CV_MAX_GROUPS 640   /* folds * classes */
/* mean[d + ny] = column means of x [n][ldx] (first d) and y [n][ldy] (first ny, y may be NULL when ny = 0), then
 * A[i][:] = [x[perm[i]] - mean_x, 1, y[perm[i]] - mean_y, 0...]  (fp64, lda >= d + 1 + ny) */
int svae_cv_center(const float* x, int ldx, int d, const float* y, int ldy, int ny, const int* perm, int n, double* mean,
                   double* A, int lda, void* stream);
/* out[g] = sum_{r in [lo[g], hi[g])} w[g * ldw + r] A[r][0:D] A[r][0:D]^T  ([D][D] blocks with leading dimension ldo, G <= 640 groups,
 * w NULL = 1, skip[g] != 0 leaves group g untouched, skip may be NULL).  With the layout of svae_cv_center one block holds the
 * group's count, sum x, sum x x^T, sum x y^T, sum y and sum y y^T about the global mean; with w = the Hessian weights it is the
 * logistic Hessian X^T D X.  Rows are summed in ascending order: bit-reproducible. */
int svae_cv_moments(const double* A, int lda, int D, const int* lo, const int* hi, int G, const double* w, long long ldw,
                    const int* skip, double* out, int ldo, void* stream);
/* Batched Cholesky of symmetric positive semi-definite M[b] (n <= 128, row-major, ld ldm, batch <= 640; the lower triangle is
 * read), one workgroup each with the triangle packed in LDS.
 * A pivot <= rtol * max(diag M[b]) is a zero direction: its column of L is 0, it adds nothing to logdet and its solution
 * coefficient is 0; rank[b] counts the kept pivots.  For a dropped direction that is an exact null space of M (a constant or
 * duplicated latent column) the solution gives the same predictions as the minimum-norm least-squares solution.
 * Outputs (each may be NULL): L[b] (lower, ld ldm, strideM), logdet[b] = sum log l_kk^2 over kept pivots, rank[b], and
 * X[b] = M[b]^-1 B[b] for B[b] [n][nrhs] (nrhs <= 8, stride strideB; B NULL: no solve). */
int svae_spd_factor_solve_f64(const double* M, int ldm, long long strideM, int n, int batch, const double* B, int nrhs,
                              long long strideB, double* L, double* X, double* logdet, int* rank, double rtol, void* stream);
/* R^2 statistics per (fold f, output o) over the fold's rows: stats[f][o] = {sum (y - yhat)^2, sum yc, sum yc^2, count}, yc = the
 * centred target column d + 1 + o of A.  Linear: yhat = A[r][0:d] . beta[f][:, o] + c0[f][o] (beta [folds][d][ny]); MLP: pred != NULL,
 * a device array of folds fp32 output pointers ([rows][ldp], sorted order), compared with yc + ymean[o]. */
int svae_cv_r2_stats(const double* A, int lda, int d, int ny, const int* lo, const int* hi, int folds, const double* beta,
                     const double* c0, const float* const* pred, int ldp, const double* ymean, double* stats, void* stream);
/* QDA on the test rows of every fold: score_c = cst[f][c] - |L[f][c]^-1 (x - mu[f][c])|^2 / 2 (cst = -logdet/2 + log prior,
 * -inf = class not in the training fold; mu [folds][K][d], L [folds][K][ldl][ldl]); predicted class = first argmax;
 * correct[f] += rows with prediction == label (int, zeroed by the caller); pred / gap (top-two score gap) per row may be NULL.
 * max_rows >= the largest fold. */
int svae_cv_qda_score(const double* A, int lda, int d, int K, const int* lo, const int* hi, int folds, int max_rows,
                      const double* mu, const double* L, int ldl, const double* cst, const int* label, int* correct, int* pred,
                      double* gap, void* stream);
/* Elastic-net one-vs-rest logistic regression by proximal Newton, one problem p per (fold pfold[p], positive class pos[p]):
 *   min_w  C sum_{r: fold[r] != pfold[p]} log(1 + exp(-s_r w . A[r][0:D]))  + alpha/2 |w_pen|^2 + rho |w_pen|_1,
 * s_r = +1 when label[r] == pos[p], D = d + 1 (the last coordinate multiplies A's column of ones: the unpenalised intercept).
 * One iteration = svae_logreg_stats (loss, gradient partials part[P][chunks][D + 1], Hessian weights hw[P][n]) ->
 * svae_cv_moments(w = hw) (H) -> svae_logreg_newton (KKT residual; done[p] = 1 below tol * max|grad at w = 0|; else coordinate
 * descent on the LDS-resident H for the direction) -> svae_logreg_line_search (Armijo over t = 2^-k, k < 12, then w += t dir).
 * Problems with done[p] != 0 are skipped by every kernel.  kkt_only = 1 only records the residual.  g0 must start at -1, W at 0,
 * done and iters at 0.  chunks = svae_logreg_chunks(n); the line search needs part of P * chunks * 12 doubles. */
int svae_logreg_chunks(int n);
int svae_logreg_stats(const double* A, int lda, int D, int n, const int* fold, const int* label, const int* pfold, const int* pos,
                      int P, const double* W, double C, const int* done, double* part, double* hw, void* stream);
int svae_logreg_newton(const double* A, int lda, int D, int n, const int* fold, const int* label, const int* pfold, const int* pos,
                       int P, const double* part, const double* H, double* W, double* dir, double* f0, double* delta, double* kkt,
                       double* g0, int* done, int* iters, double alpha, double rho, double tol, int kkt_only, int max_sweeps,
                       void* stream);
int svae_logreg_line_search(const double* A, int lda, int D, int n, const int* fold, const int* label, const int* pfold,
                            const int* pos, int P, double* W, const double* dir, const double* f0, const double* delta, int* done,
                            int* iters, double C, double alpha, double rho, double* part, void* stream);
/* decision values of the test rows of fold f with its problems p in [pstart[f], pstart[f + 1]) (pstart: folds + 1 ints; a fold's
 * problems are those of the classes present in its training rows, as sklearn fits them): argmax (first on a tie) -> pos[p]; a fold
 * with one problem is binary: decision > 0 -> pos[p], else neg[f].  correct[f] += matches with label (zeroed by the caller), pred may
 * be NULL */
int svae_logreg_score(const double* A, int lda, int D, int n, const int* fold, const int* label, const int* pfold, const int* pos,
                      int P, const double* W, const int* pstart, const int* neg, const int* lo, const int* hi, int folds, int max_rows,
                      int* correct, int* pred, void* stream);
/* MLP decoders (train_MLP, metrics.py:307-329) on the svae_ens_* kernels, one ensemble member per fold: dpred[m][r][o] =
 * 2 (outs[m][r][o] - y[r][o]) for rows outside fold mfold[m], 0 inside (MSELoss(reduction="sum") on the training rows only).
 * outs / dpred: device arrays of n_members pointers to [n][ld] fp32. */
int svae_cv_mse_grad(const float* const* outs, float* const* dpred, int n_members, const int* mfold, const float* y, int ldy, int ny,
                     int ld, const int* fold, int n, void* stream);

/* ---------------------------------------------------------- Gaussian mixture clustering (csrc/gmm.hip) --- */
/* sklearn GaussianMixture(init_params="k-means++", n_init=1) of the reference's eval/cluster.py::gmm, fp64.  Rows are A [n][lda]
 * from svae_cv_center (identity perm, ny = 0: columns [0, d) = x - global mean, column d = 1); means mu [K][d] are in that centred
 * frame.  d <= SVAE_CV_MAX_DIM, K <= SVAE_GMM_MAX_COMPONENTS.  Every reduction runs in a fixed order: bit-reproducible. */
#define SVAE_GMM_MAX_COMPONENTS 64
#define SVAE_GMM_MAX_TRIALS 8  /* k-means++ candidates per round: 2 + int(log K) */
/* One k-means++ round.  vals NULL (the first round): cand[0] (device, set by the caller) is the first center.  Otherwise cand[t] =
 * searchsorted(prefix sum of closest, vals[t]) clipped to n - 1 for t < T (vals: device, the host's uniform draws times the
 * current potential).  Then d2[t][r] = min(closest[r], |A[r] - A[cand[t]]|^2) (no minimum on the first round), potentials
 * summed in a fixed order, the first smallest wins: pot[0], id[0] = its row, best[0] = its t; closest and tot (the block sums
 * the next round's prefix sum reads) take its distances.  Buffers: closest [n], tot and part [T][blocks], d2 [T][n],
 * blocks = svae_gmm_kpp_blocks(n). */
int svae_gmm_kpp_blocks(int n);
int svae_gmm_kpp_round(const double* A, int lda, int d, int n, const double* vals, int T, int* cand, double* closest, double* tot,
                       double* d2, double* part, double* pot, int* id, int* best, void* stream);
/* E-step.  Weighted log density w_k(r) = cst[k] - |(A[r][0:d] - mu[k]) P_k|^2 / 2 with cst = log weight + log det P - d log(2 pi) / 2;
 * full (diag = 0): P [K][d][ldp] upper triangular (precisions_cholesky_, ldp = pad8(d), zero below the diagonal and in the pad
 * columns); diag: P [K][d].  Outputs (NULL: not written): resp [K][n] = exp(w_k - logsumexp_k w_k) (needed for lpn and part),
 * lpn [n] = logsumexp, part [svae_gmm_estep_blocks(n)] = per-block sums of lpn, label [n] = first argmax_k w_k, gap [n] = top-two
 * gap of w. */
int svae_gmm_estep_blocks(int n);
int svae_gmm_estep_f64(const double* A, int lda, int d, int n, int K, int diag, const double* mu, const double* P, int ldp,
                       const double* cst, double* resp, double* lpn, double* part, int* label, double* gap, void* stream);
/* out[0] = (x[0] + ... + x[m - 1]) / div in a fixed order (the lower bound from the E-step's part) */
int svae_gmm_sum_f64(const double* x, int m, double div, double* out, void* stream);
/* M-step from resp [K][n], as sklearn's _estimate_gaussian_parameters but two-pass about the new means:
 *   s1 [K][d + 1] = sum_r resp A (column d: the responsibility total), nk = s1[:, d] + 10 eps, mu = s1[:, :d] / nk, w = nk / sum nk;
 *   full: cov [K][d][d] = sum_r resp (a - mu)(a - mu)^T / nk + reg I (factor it with svae_spd_factor_solve_f64, rtol = 0, then
 *         svae_gmm_precision_f64);
 *   diag: cov [K][d] = sum_r resp (a - mu)^2 / nk + reg, P [K][d] = 1 / sqrt(cov), cst as in the E-step, bad[k] = some cov <= 0.
 * Rows are summed in svae_gmm_chunks(n, d) chunks, each in ascending order, the chunks in order: part holds
 * chunks * K * max(d + 1, full ? d * d : d) doubles. */
int svae_gmm_chunks(int n, int d);
int svae_gmm_mstep_f64(const double* A, int lda, int d, int n, int K, int diag, const double* resp, double reg, double* part,
                       double* s1, double* nk, double* w, double* mu, double* cov, double* P, double* cst, int* bad, void* stream);
/* full covariance: P[k] = L[k]^-T ([d][ldp], ldp = pad8(d)) from the Cholesky factors L [K][d][d] and rank [K] of
 * svae_spd_factor_solve_f64 (rtol = 0), cst[k] = log w[k] + sum log P_jj - d log(2 pi) / 2; bad[k] = rank[k] < d (the covariance
 * is not positive definite; P[k] and cst[k] are then not written). */
int svae_gmm_precision_f64(const double* L, const int* rank, const double* w, int d, int K, int ldp, double* P, double* cst, int* bad,
                           void* stream);

/* ------------------------------------------------------------- Gaussian hidden Markov model (csrc/hmm.hip) --- */
/* Scaled forward-backward pass of a K-state HMM over n frames, parallel in time and exact, and Viterbi decoding; fp64.
 * B [K][ldb] = the resp of svae_gmm_estep_f64 run with unit weights (cst = log det P - d log(2 pi) / 2): the emission densities of
 * every frame scaled to sum to 1 (exact zeros allowed), lpn [n] = the log of that scale; startprob [K]; transmat [K][K], rows sum
 * to 1, zeros allowed.  K <= SVAE_HMM_MAX_STATES, n < 2^26.  The host cuts every sequence into segments of L = svae_hmm_segment(K)
 * frames (a function of K alone; the last segment of a sequence is shorter), never across a sequence boundary:
 *   seg [nseg][4] int = {first frame, frames, 1 for the first segment of its sequence else 0, sequence}
 *   seq [nseq][4] int = {first segment, segments, first frame, frames}
 * (device arrays; a table that does not fit n makes no access outside the arrays; seg[.][3] is the host's, no kernel reads it, and
 * every entry point takes both tables so that they are called alike: transfer reads seg only).  States are padded to KP = svae_hmm_padded(K)
 * in {16, 32, 64}.  work holds svae_hmm_work(K, nseg) doubles: the transfer matrices [nseg][KP][KP] with their row exponents, the
 * boundary vectors, the per-segment log-likelihoods and svae_hmm_xi_blocks(nseg) partials [KP][KP] of the transition counts.
 * Nothing of size n x K^2 is stored.  No floating-point atomics and every sum in a fixed order: all outputs are bit-reproducible,
 * and alpha, gamma and c of a sequence do not depend on the other sequences of the call or on their order (Xi, start_post and
 * loglik are sums over the sequences in table order). */
#define SVAE_HMM_MAX_STATES 64  /* = SVAE_GMM_MAX_COMPONENTS */
#define SVAE_HMM_SEGMENT_16 512 /* L for KP = 16 */
#define SVAE_HMM_SEGMENT_32 512 /* L for KP = 32 */
#define SVAE_HMM_SEGMENT_64 512 /* L for KP = 64 */
int svae_hmm_padded(int K);
int svae_hmm_segment(int K);
int svae_hmm_xi_blocks(int nseg);
long long svae_hmm_work(int K, int nseg);
/* Transfer: per segment T = prod_t transmat diag(b_t) (diag(b_1) first in the first segment of a sequence) as R [KP][KP] times one
 * power of two per row (an integer exponent: the scaling rounds nothing), rescaled at every frame; R transmat runs on the fp64
 * matrix cores.  A row whose sum reaches 0 stays 0. */
int svae_hmm_transfer_f64(const double* B, long long ldb, int n, int K, const double* transmat, const int* seg, int nseg,
                          const int* seq, int nseq, double* work, void* stream);
/* Carry (after transfer): per sequence, the normalised forward vector entering every segment and the normalised backward vector at
 * every segment's last frame, combined relative to the largest row exponent. */
int svae_hmm_carry_f64(int n, int K, const double* startprob, const int* seg, int nseg, const int* seq, int nseq, double* work,
                       void* stream);
/* Fill (after carry): the scaled recursion inside every segment.  c [n] = the scale of every frame, gamma [K][n] = the smoothed
 * posteriors (every column sums to 1; the buffer holds alpha between the two kernels; it must not be B),
 * Xi [K][K] = sum_t alpha_{t-1}(i) transmat[i][j] b_t(j) beta_t(j) / c_t, start_post [K] = sum of gamma at the first frame of every
 * sequence, loglik [1] = sum_t (log c_t + lpn_t). */
int svae_hmm_fill_f64(const double* B, long long ldb, const double* lpn, int n, int K, const double* transmat, const int* seg, int nseg,
                      const int* seq, int nseq, double* work, double* gamma, double* c, double* Xi, double* start_post, double* loglik,
                      void* stream);
/* transmat[i] = max(Xi[i] + transmat_prior - 1, 0) / its sum, startprob likewise from start_post; a row whose sum is 0 keeps its
 * values. */
int svae_hmm_update_f64(const double* Xi, const double* start_post, int K, double transmat_prior, double startprob_prior,
                        double* transmat, double* startprob, void* stream);
/* Viterbi: delta_t(j) = max_i (delta_{t-1}(i) + log_transmat[i][j]) + logB[j][t] with logB [K][n], one workgroup per sequence (only
 * seq[.][2..3] are read), ties to the lower state at every step as np.argmax.  backptr [n][K] bytes (work), states [n],
 * logprob [nseq] = the log-probability of each sequence's path.  Only adds and compares: equal to the same recursion in numpy. */
int svae_hmm_viterbi(const double* log_startprob, const double* log_transmat, const double* logB, int n, int K, const int* seq,
                     int nseq, unsigned char* backptr, int* states, double* logprob, void* stream);

/* ---------------------------------------------------------------------- k-means clustering (csrc/kmeans.hip) --- */
/* Lloyd's iteration of sklearn's KMeans(algorithm="lloyd"), fp64, on the centred rows A [n][lda] of svae_cv_center (as for the
 * mixture above: column d = 1) and centres C [K][ldc] in that centred frame.  d <= SVAE_CV_MAX_DIM, K <= SVAE_KMEANS_MAX_CLUSTERS.
 * Every sum runs in a fixed order and there are no floating-point atomics: bit-reproducible. */
#define SVAE_KMEANS_MAX_CLUSTERS 1024
/* Assignment.  s(r, c) = ((a0 - c0)^2 + (a1 - c1)^2) + ... in feature order (csrc/pair_tiles.h); every row takes the centre with
 * the smallest key (s by its bit pattern, then the lower centre index).  Outputs (NULL: not written): label [n], dist [n] = that
 * s, gap [n] = the second-smallest s minus the smallest (+inf when K = 1), D [n][K] = every s, part [svae_kmeans_assign_blocks(n)]
 * = the sums of dist over blocks of 64 rows, each in a fixed tree order, changed[0] = the rows with label != prev (an integer count;
 * needs prev [n], which must not be the label buffer).  Nothing of size n x K is written unless D is given. */
int svae_kmeans_assign_blocks(int n);
int svae_kmeans_assign_f64(const double* A, int lda, int d, int n, const double* C, int ldc, int K, const int* prev, int* label,
                           double* dist, double* gap, double* D, double* part, int* changed, void* stream);
/* Update.  sums [K][d + 1] = sum over the rows r with label[r] == c of A[r][0..d] (column d: the count), as the product M^T [A | 1]
 * with the 0/1 membership matrix on the fp64 matrix cores: exact products, so each sum is the plain fp64 sum of its cluster's rows
 * in a fixed order and does not depend on the numbering of the clusters.  Rows are summed in svae_kmeans_chunks(n, d, K) chunks
 * (a function of the sizes alone: 256-row units, at most 1024 chunks and at most 2^24 doubles of partials), the chunks added in
 * a fixed order; part holds chunks * K * (d + 1) doubles.  label values outside [0, K) are counted nowhere. */
int svae_kmeans_chunks(int n, int d, int K);
int svae_kmeans_update_f64(const double* A, int lda, int d, int n, const int* label, int K, double* part, double* sums, void* stream);
/* Finish.  C_new[k] = sums[k][0:d] / sums[k][d], or C_old[k] where that count is 0 (C_new must not be C_old);
 * rec [3] = {changed[0] (-1 when changed is NULL), sum |C_new - C_old|^2 in a fixed order, the clusters with count 0}: the one
 * record a host reads per iteration.  (The inertia is svae_gmm_sum_f64 of the assignment's part with div = 1.) */
int svae_kmeans_finish_f64(const double* sums, int d, int K, const double* C_old, double* C_new, int ldc, const int* changed,
                           double* rec, void* stream);

/* ---------------------------------------------------------------------- HDBSCAN clustering (csrc/hdbscan.hip) --- */
/* sklearn HDBSCAN(metric="euclidean") of the reference's eval/cluster.py::dbscan, fp64.  Rows X [n][ld] (the latents converted to
 * fp64, not centred).  Squared distance s = ((x0 - y0)^2 + (x1 - y1)^2) + ... in feature order, no FMA; distance = sqrt(s),
 * correctly rounded.  Mutual reachability w_ij = max(core_i, core_j, d_ij / alpha).  MST edges are ordered by the strict key
 * (w, min(i, j), max(i, j)), so the tree is unique and every result is bit-reproducible.  Any d >= 1, 2 <= n < 2^31. */
/* core [n] = sqrt of the k-th smallest s over all n rows (the row itself included at 0), 1 <= k <= n; k = 1 writes zeros */
int svae_hdb_core(const double* X, int ld, int d, int n, int k, double* core, void* stream);
/* One Boruvka round.  Rows in ascending order of core distance: X [n][ld], core [n], id [n] (the row's index in the caller's order,
 * used in the key), comp [n] (component ids 0 .. n_comp - 1, n_comp >= 2).  Per row: bw [n], bp [n] = the minimum-key edge to another
 * component (bp = (lo << 32) | hi of the ids); per component: cw [n_comp] = the bits of its minimum weight, cp [n_comp] = the
 * minimum packed pair among its rows at that weight.  Copy cw / cp to the host for svae_hdb_merge. */
int svae_hdb_boruvka(const double* X, int ld, int d, int n, const double* core, const int* id, const int* comp, double alpha, int n_comp,
                     double* bw, unsigned long long* bp, unsigned long long* cw, unsigned long long* cp, void* stream);
/* comp[r] = map[comp[r]] for r < n (the relabelling svae_hdb_merge returns) */
int svae_hdb_relabel(int* comp, int n, const int* map, void* stream);
/* HOST memory, no stream.  Adds each component's edge (cw, cp) to lo / hi / w [n - 1] at *n_edges (an edge chosen from both sides
 * once), merges components: comp [n] (caller's row order) relabelled in place, map [n_comp] = new id of each old component,
 * *n_comp_out = the new count (ids numbered by first old component). */
int svae_hdb_merge(int n, int n_comp, const unsigned long long* cw, const unsigned long long* cp, int* comp, int* map, int* lo, int* hi,
                   double* w, int* n_edges, int* n_comp_out);
/* HOST memory, no stream.  From the n - 1 MST edges (lo < hi, any order): the single-linkage tree sl_* [n - 1] (edges in key order,
 * the root of lo on the left, internal node n + edge index), then sklearn 1.7's condensed tree (lambda = 1 / w, inf at w = 0),
 * stabilities, excess-of-mass (leaf = 0) or leaf (leaf = 1) selection with epsilon, max_cluster_size (<= 0: none) and
 * allow_single_cluster, labels [n] (-1 noise, clusters numbered in ascending condensed node order) and prob [n]. */
int svae_hdb_tree(int n, const int* lo, const int* hi, const double* w, int min_cluster_size, int leaf, int allow_single, double epsilon,
                  long long max_cluster_size, long long* sl_left, long long* sl_right, double* sl_value, long long* sl_size,
                  long long* labels, double* prob);
/* HOST memory, no stream.  sklearn's labelling_at_cut over a single-linkage tree of n_nodes points: merges below `cut`, clusters of
 * fewer than min_cluster_size points are noise (-1), the rest numbered by ascending union-find root. */
int svae_hdb_cut(long long n_nodes, const long long* left, const long long* right, const double* value, double cut,
                 long long min_cluster_size, long long* labels);

/* ------------------------------------------------------- Maximum mean discrepancy between latent sets (csrc/mmd.hip) --- */
/* The reference's eval/metrics.py::mmd_estimate, fp64.  Z [n][ld] = the rows of X (nx) then of Y (ny) converted to fp64, not centred;
 * the pairs are i < j of Z, M = n (n - 1) / 2 of them.  Squared distance s as for HDBSCAN above (feature order, no FMA), dist = sqrt(s):
 * scipy's pdist / cdist.  Nothing of size n^2 is stored; every result is bit-reproducible.  Any d >= 1, n < 2^26. */
#define SVAE_MMD_WORK_WORDS 8256
/* number of blocks of the all-pairs launches at n rows: svae_mmd_sums needs part [3 * blocks] */
long long svae_mmd_blocks(int n);
/* hm[0] = med = np.median of the M distances (the value of rank M / 2 for odd M, the mean of ranks M / 2 - 1 and M / 2 for even M),
 * hm[1] = h = med * med.  Exact: a radix select over the bits of s, 5 all-pairs passes (6 for even M) enqueued back to back, no host
 * round trip.  work [SVAE_MMD_WORK_WORDS] device scratch, initialised here. */
int svae_mmd_select(const double* Z, int ld, int d, int n, unsigned long long* work, double* hm, void* stream);
/* out = {kxx, kyy, kxy, kxx + kyy - 2 kxy}: means of exp((-(dist * dist)) / h[0]) over the pairs inside X, inside Y and across
 * (nx >= 2, n - nx >= 2), h a device pointer (hm + 1 of svae_mmd_select, or a given bandwidth).  One all-pairs pass; per-block
 * partial sums in part [3 * svae_mmd_blocks(n)] reduced in a fixed order. */
int svae_mmd_sums(const double* Z, int ld, int d, int n, int nx, const double* h, double* part, double* out, void* stream);
/* Permutation null of that statistic (csrc/mmd_null.hip).  Relabelling p puts nx of the n rows into "X": bits [n][words] packs the
 * memberships, bit (p & 63) of bits[j][p >> 6] = 1 when row j is in X under p (words >= ceil(P / 64); the bits past P of a row's
 * last used word must be 0).  out[p] = kxx + kyy - 2 kxy of the split p, the estimator of svae_mmd_sums: one all-pairs pass per
 * chunk of SVAE_MMD_NULL_COLS permutations, the 64 x 64 kernel tiles multiplied with the label columns on the fp64 matrix cores,
 * per-block partials in work reduced in a fixed order; out[p] depends on column p of bits alone and is bit-reproducible.
 * 1 <= P <= SVAE_MMD_NULL_MAX. */
#define SVAE_MMD_NULL_COLS 256
#define SVAE_MMD_NULL_MAX 65536
/* doubles of work that svae_mmd_null needs at n rows and P permutations (0 for n < 2 or a P out of range) */
long long svae_mmd_null_blocks(int n, int P);
int svae_mmd_null(const double* Z, int ld, int d, int n, int nx, const double* h, const unsigned long long* bits, int words, int P,
                  double* work, double* out, void* stream);

/* ---------------------------------------------------------- Silhouette of a clustering of latents (csrc/silhouette.hip) --- */
/* sklearn's silhouette_samples with the Euclidean metric, fp64.  Z [n][ld] fp64 rows, not centred; lab [n] = the cluster of each row
 * in 0..K-1, count [K] = the rows of each cluster (every one >= 1), 2 <= K <= min(n - 1, SVAE_SIL_MAX_CLUSTERS), n < 2^26.  With
 * S[i][c] = the sum over the rows j of cluster c of dist(i, j) (distances as for the MMD above):
 *   a_i = S[i][own] / (m_own - 1), b_i = min over c != own of S[i][c] / m_c, nearest_i = that c (the lowest on an exact tie),
 *   s_i = (b_i - a_i) / max(a_i, b_i); s_i = 0 where max(a_i, b_i) == 0; a_i = s_i = 0 for a row alone in its cluster.
 * s, a, b, nearest [rows] receive the rows [row0, row0 + rows) against all n columns: one pass over rows x n distances per chunk of
 * 256 clusters, the 64 x 64 distance tiles multiplied with the membership columns on the fp64 matrix cores, summed in a fixed
 * order.  Nothing of size n^2 is stored; every result is bit-reproducible and does not depend on the numbering of the clusters. */
#define SVAE_SIL_MAX_CLUSTERS 4096
/* doubles of work that svae_silhouette needs for `rows` rows of n with K clusters (0 for n < 3, K < 2, K > SVAE_SIL_MAX_CLUSTERS,
 * rows < 1 or rows > n): column chunks (at most 8, 1 once the grid holds 512 blocks) x rows padded to 64 x K padded to the
 * 16, 64 or 256 cluster columns of a block */
long long svae_silhouette_work(int rows, int n, int K);
int svae_silhouette(const double* Z, int ld, int d, int n, const int* lab, const int* count, int K, int row0, int rows, double* work,
                    double* s, double* a, double* b, int* nearest, void* stream);
/* out[0] = the mean of v [n]: compensated sums at fixed positions, then a fixed tree */
int svae_silhouette_mean(const double* v, long long n, double* out, void* stream);
/* row[c] = the lowest row i of cluster c with the smallest a[i] (a [n] >= 0, finite): the medoid.  key [K] device scratch. */
int svae_silhouette_medoids(const double* a, const int* lab, int n, int K, unsigned long long* key, long long* row, void* stream);

/* ------------------------------------------------------- Exact k nearest neighbours of every latent (csrc/knn.hip) --------- */
/* Z [n][ld] fp64 rows, not centred, d >= 1, 2 <= n < 2^31, 1 <= k <= min(n - 1, SVAE_KNN_MAX_K).  The neighbours of row i are the
 * k smallest keys (s_ij, j) over j != i, compared strictly and lexicographically: s_ij the squared distance of csrc/pair_tiles.h
 * (feature order, no FMA) compared by its uint64 bit pattern, then the lower j.  The row itself is left out by index, not by
 * distance: a duplicate of row i is a neighbour at distance 0.  idx [n][k] and dist [n][k] hold the neighbours of row i in
 * ascending key order, dist = the correctly rounded sqrt(s).  group [n] (nullable) keeps only the candidates j with
 * group[j] != group[i]; the caller guarantees that every row keeps at least k candidates (with fewer, the tail of that row's
 * idx and dist is left unwritten).  One pass over the n^2 distances: a block keeps the running best k of its 64 rows in LDS;
 * nothing of size n^2 or n (n / 64) is stored.  The result is unique, so bit-reproducible, and does not depend on the column
 * chunks.  SVAE_KNN_MAX_K is what 160 KiB of LDS hold next to the staged rows: 64 rows x 154 buffered candidates, of which a
 * tile of 64 columns may add 64 to a row (90 = 3 x 30: what t-SNE asks for at perplexity 30). */
#define SVAE_KNN_MAX_K 90
/* bytes of work that svae_knn needs (0 for n < 2, k < 1, k > n - 1 or k > SVAE_KNN_MAX_K): column chunks (at most 8, 1 once
 * the grid holds 512 blocks) x rows padded to 64 x k x 12 (a uint64 key and an int32 index per kept candidate) */
long long svae_knn_work(int n, int k);
int svae_knn(const double* Z, int ld, int d, int n, int k, const int* group, void* work, int* idx, double* dist, void* stream);
/* svae_knn_cross: the k nearest rows of X [n][ldx] for every row of Q [m][ldq], both of d >= 1 features, 1 <= m, n < 2^31,
 * 1 <= k <= min(n, SVAE_KNN_MAX_K).  The neighbours of query i are the k smallest keys (s_ij, j) over ALL j < n, with svae_knn's
 * strict key (the squared distance of csrc/pair_tiles.h by its bit pattern, then the lower j).  No row is left out: a query equal
 * to a reference row has that row as a neighbour at distance 0 (Q = X gives every row itself first).  idx [m][k] and dist [m][k]
 * are in ascending key order, dist the correctly rounded sqrt(s).  The same kernel walk and LDS buffer as svae_knn, without the
 * self and group tests; the column chunks follow the same rule with the row tiles counted from m and the column tiles from n, and
 * the key is strict, so the result does not depend on the split.
 * svae_knn_cross_work: bytes of work (0 for m < 1, n < 1, k < 1, k > n or k > SVAE_KNN_MAX_K): column chunks (at most 8, 1 once
 * the grid holds 512 blocks) x m padded to 64 x k x 12. */
long long svae_knn_cross_work(int m, int n, int k);
int svae_knn_cross(const double* Q, int ldq, int m, const double* X, int ldx, int n, int d, int k, void* work, int* idx, double* dist,
                   void* stream);

/* ------------------------------------------------------- t-SNE of the latents on their exact kNN graph (csrc/tsne.hip) --------- */
/* sklearn's TSNE with an exact gradient, all fp64, no FMA contraction, every result bit-reproducible for a given (n, chunks).
 *
 * svae_tsne_search: the perplexity search of sklearn's _binary_search_perplexity on d2 [n][k], the squared distances to each
 * row's k neighbours (1 <= k <= SVAE_KNN_MAX_K, n >= 1): beta = 1, bounds -inf / +inf, at most SVAE_TSNE_SEARCH_STEPS steps of
 * sum = sum_j exp(-d2 beta) (a zero sum becomes 1e-8), H = log(sum) + beta * sum_j(d2 exp(-d2 beta)) / sum, both sums in
 * neighbour order, until |H - log(perplexity)| <= 1e-5; H too large doubles beta (or takes the midpoint with the upper bound
 * once there is one), H too small halves it (or the midpoint with the lower bound).  P [n][k] = exp(-d2 beta) / sum at the last
 * beta evaluated; beta [n] is the search variable as the loop leaves it (after 100 steps without convergence: one update past
 * the beta of P, as sklearn's). */
#define SVAE_TSNE_SEARCH_STEPS 100
int svae_tsne_search(const double* d2, int k, int n, double perplexity, double* P, double* beta, void* stream);
/* svae_tsne_repulsion: for every row i of Y [n][2] (2 <= n <= 2^26), over all j != i (the row left out by index) with
 * d = y_i - y_j and q = 1.0 / (1.0 + (d0 d0 + d1 d1)) (the division correctly rounded):
 *     R [n][2] = sum_j q q d        rowq [n] = sum_j q        Z [1] = sum_i rowq[i]
 * The full square, so every row's sums have one owner: a block of 256 threads keeps one row per thread in registers and streams
 * the candidates from LDS in ascending j.  The columns are split into `chunks` ranges of whole 64-column tiles (grid y);
 * 1 <= chunks <= SVAE_TSNE_MAX_CHUNKS is taken as given (at most one per tile), chunks = 0 picks min(8, tiles) and fewer once
 * the grid holds 512 blocks (the silhouette's rule).  The chunk partials are added in chunk order; Z is reduced at fixed
 * positions (thread t of 256 adds rowq[t], rowq[t + 256], ... compensated, then a fixed tree).  work: svae_tsne_repulsion_work
 * doubles (0 for arguments out of range): chunks x 3 x rows padded to 256. */
#define SVAE_TSNE_MAX_CHUNKS 8
long long svae_tsne_repulsion_work(int n, int chunks);
int svae_tsne_repulsion(const double* Y, int n, int chunks, double* work, double* R, double* rowq, double* Z, void* stream);
/* svae_tsne_step: one descent step on the CSR joint probabilities (rowptr [n + 1] int32, col int32, val fp64; p = exag * val).
 * Per row, over its entries in stored order with d = y_i - y_j, w = 1.0 + (d0 d0 + d1 d1):
 *     A_i = sum val (1.0 / w) d        klpart[i] = sum p log(p w)        grad_i = 4.0 (exag A_i - R_i / Z)
 *     gains = update grad < 0 ? gains + 0.2 : gains 0.8, at least 0.01;   grad = grad gains   (sklearn's order)
 *     update = momentum update - lr grad;   gradsq[i] = grad . grad (of the gained gradient: what sklearn's norm is taken of)
 * (an entry with p = 0 adds nothing to klpart) and, in a second launch so that no row sees a neighbour's new position, Y = Y + update.  klpart and gradsq may both be NULL
 * (no check this iteration).  update == NULL evaluates only: klpart and gradsq (of the plain gradient) at Y, nothing modified. */
int svae_tsne_step(const int* rowptr, const int* col, const double* val, double exag, double* Y, const double* R, const double* Z,
                   double* update, double* gains, double momentum, double lr, int n, double* klpart, double* gradsq, void* stream);
/* Placing new rows on a fitted map: every query is an optimisation of its own in the field of the n fixed map points.
 *
 * svae_tsne_cross_repulsion: for every query i < m of Yq [m][2] over ALL j < n of Yref [n][2] in ascending j (1 <= m, n <= 2^26),
 * with d = yq_i - yref_j and q = 1.0 / (1.0 + (d0 d0 + d1 d1)):
 *     R [m][2] = sum_j q q d        rowq [m] = sum_j q
 * No exclusion by index (a query on top of a map point adds q = 1 and no force) and no global Z: a query normalises by its own
 * rowq.  The kernel of svae_tsne_repulsion on a rectangle: one query per thread in registers, candidates broadcast from LDS, the
 * columns split into `chunks` ranges of whole 64-column tiles whose partials are added in chunk order.  1 <= chunks <=
 * SVAE_TSNE_MAX_CHUNKS is taken as given (at most one per tile).  chunks = 0 picks the split from n alone, never from m: the
 * most there are, min(8, tiles), in ranges of ceil(tiles / that) tiles.  So the bits of a query's
 * sums depend on (yq_i, Yref, n, chunks) only, not on the other queries of the launch or on m.  Yq and Yref must not overlap
 * (SVAE_ERR_ARG).  work: svae_tsne_cross_repulsion_work doubles (0 for arguments out of range): chunks x 3 x m padded to 256.
 *
 * svae_tsne_place_step: one descent step of every query against the fixed map.  idx [m][k] int32 (entries in [0, n): the caller's
 * guarantee) and P [m][k] fp64 are the query's reference neighbours and conditional probabilities, 1 <= k <= SVAE_KNN_MAX_K,
 * 1 <= m <= 2^26; R and rowq come from svae_tsne_cross_repulsion at the same Yq.  Per query, over its entries in stored order with
 * d = yq_i - yref_j, w = 1.0 + (d0 d0 + d1 d1) and p = exag P:
 *     A = sum P (1.0 / w) d        klrow[i] = sum p log(p w) + log(rowq[i])        g = 2.0 (exag A - R[i] / rowq[i])
 * (an entry with p = 0 adds nothing to klrow).  At exag = 1 klrow is the query's objective sum_e p log(p / q_e|i) with
 * q_e|i = (1 / w) / rowq_i, and g its exact gradient (hence 2, not the 4 of the symmetric objective).  Then, in this order:
 *     max_grad_norm > 0 and |g| = sqrt(g0 g0 + g1 g1) > max_grad_norm:  g = g (max_grad_norm / |g|)   (0: no clip)
 *     gains = update g < 0 ? gains + 0.2 : gains 0.8, at least 0.01;   g = g gains
 *     update = momentum update - lr g;   gradsq[i] = g . g;   Yq[i] = Yq[i] + update
 * in one launch: a thread writes only its own row and reads only Yref besides.  klrow and gradsq may both be NULL.  update and
 * gains go together; with both NULL only klrow and gradsq (of the clipped, ungained gradient) are evaluated and nothing moves.
 * Everything NULL, or max_grad_norm < 0: SVAE_ERR_ARG. */
long long svae_tsne_cross_repulsion_work(int m, int n, int chunks);
int svae_tsne_cross_repulsion(const double* Yq, int m, const double* Yref, int n, int chunks, double* work, double* R, double* rowq,
                              void* stream);
int svae_tsne_place_step(const int* idx, const double* P, int k, double exag, double* Yq, const double* Yref, const double* R,
                         const double* rowq, double* update, double* gains, double momentum, double lr, double max_grad_norm, int m,
                         double* klrow, double* gradsq, void* stream);
/* out[0] = sum of a [n], out[1] = sum of b [n] (b nullable): compensated sums at fixed positions, then a fixed tree */
int svae_tsne_sums(const double* a, const double* b, long long n, double* out, void* stream);

/* ------------------------------------------------------- Independence of latents and a variable: HSIC (csrc/hsic.hip) ---------- */
/* The Hilbert-Schmidt independence criterion with a permutation null, fp64, nothing of size n^2 stored, every result
 * bit-reproducible.  Z [n][ld] fp64 rows, not centred, 2 <= n < 2^26; K_ij = exp((-s_ij) / hz) with s the squared distance of
 * csrc/pair_tiles.h (feature order, no FMA, no sqrt round trip).  The variable is either Y [n][q] fp64 rows, contiguous,
 * 1 <= q <= SVAE_HSIC_MAX_Y, with L_ij = exp((-t_ij) / hy) built the same way, or lab [n] int32 with L_ij = [lab_i == lab_j].
 * Bandwidths are device pointers (hm + 1 of svae_mmd_select on the rows alone, or a given value).  A permutation table perm
 * [P][n] int32 holds one permutation of 0..n-1 per row (the caller guarantees that): under row p, y_perm[p][i] is paired with z_i.
 * A null perm with P = 1 is the identity.  1 <= P <= SVAE_MMD_NULL_MAX per call.
 *
 * svae_hsic_moments: of one kernel matrix M (X [n][ld] with bandwidth h, or lab; exactly one of X and lab is non-null), over the
 * full square with the diagonal: rowsum [n] = sum_j M_ij, mom = {sum_ij M_ij, sum_ij M_ij^2, sum_i rowsum_i^2}.  One all-pairs
 * pass, per-block partials at fixed positions in work, compensated fixed-order reductions.
 * svae_hsic_cross: out[p] = A_p = sum_{i<j} K_ij L_perm[p][i] perm[p][j].  A block of 256 threads holds a 64 x 64 tile of K in
 * registers and regenerates L for the same pairs for each of the SVAE_HSIC_PERMS permutations of its chunk from the permuted
 * rows of y staged in LDS; K is recomputed once per chunk.  Fixed order throughout (pairs of a tile, tiles in column order, a
 * fixed cross-lane tree, waves in order, per-block partials in work, a compensated reduction), no floating-point atomics: out[p]
 * depends on row p of perm alone, not on its position, on P or on the call it falls in.
 * svae_hsic_dots: out[p] = sum_i (k_i - t) (l_perm[p][i] - t), t = 1 when tilde is non-zero (the unbiased estimator's row sums
 * without the diagonal) and 0 otherwise; a gather and a compensated fixed-order sum per permutation. */
#define SVAE_HSIC_MAX_Y 4
#define SVAE_HSIC_PERMS 16
/* doubles of work that svae_hsic_moments and svae_hsic_cross need at n rows and P permutations per call (0 for n < 2, n >= 2^26
 * or a P out of range): column chunks (at most 8) x row tiles x the larger of 128 and P padded to SVAE_HSIC_PERMS */
long long svae_hsic_work(int n, int P);
int svae_hsic_moments(const double* X, int ld, int d, const int* lab, int n, const double* h, double* work, double* rowsum,
                      double* mom, void* stream);
int svae_hsic_cross(const double* Z, int ld, int d, int n, const double* hz, const double* Y, int q, const int* lab,
                    const double* hy, const int* perm, int P, double* work, double* out, void* stream);
int svae_hsic_dots(const double* k, const double* l, int n, const int* perm, int P, int tilde, double* out, void* stream);

/* ------------------------------------------------------- Mutual information of latents and a variable by kNN (csrc/mi.hip) ---- */
/* The k-nearest-neighbour estimators of I(z; y) in their integer parts: Kraskov-Stoegbauer-Grassberger (algorithm 1) for a real y,
 * Ross (2014) for labels.  Z [n][ld] fp64 rows, not centred, d >= 1, 2 <= n < 2^31, 1 <= k <= min(n - 1, SVAE_MI_MAX_K).  The
 * variable is either Y [n][q] fp64 rows, contiguous, 1 <= q <= SVAE_MI_MAX_Y, or lab [n] int32.  s^z_ij and s^y_ij are the squared
 * distances of csrc/pair_tiles.h (feature order, no FMA), compared by their uint64 bit patterns, never by a square root.  The row
 * itself is left out by index, not by distance: a duplicate of row i counts at 0.
 *
 * svae_mi_radius: rho2 [n].  With Y: the k-th smallest max(s^z_ij, s^y_ij) over j != i.  With lab: the kk[i]-th smallest s^z_ij
 * over the j != i with lab[j] == lab[i]; kk [n] int32, 1 <= kk[i] <= k, and the caller guarantees that row i has at least kk[i]
 * such candidates (with fewer, rho2[i] is left unwritten).  Exactly one of Y and lab is non-null; kk is given with lab only.  One
 * pass over the n^2 distances with the running best k of 64 rows in LDS, as svae_knn (csrc/knn_buffer.h: 64 rows x 128 buffered
 * candidates, of which a tile of 64 columns may add 64 to a row; SVAE_MI_MAX_K = 32 leaves a cut buffer two tiles at least).
 * svae_mi_counts: nz [n] = #{j != i : s^z_ij < rho2[i]} and, with Y, ny [n] = #{j != i : s^y_ij < rho2[i]}, both strict (a row
 * with rho2 = 0 counts 0).  Y and ny are both null for labels.  A second all-pairs pass; int32 counts combined by integer adds
 * only, so exact and independent of scheduling and of the column chunks.
 * svae_mi_psi_sums: out[0] = sum_i psi(a[i] + 1), out[1] = sum_i psi(b[i] + 1) (b nullable), a and b [n] int32 >= 0: compensated
 * sums at fixed positions, then a fixed tree, as svae_tsne_sums.  psi(m) of a positive integer: for m < 16,
 * -0.5772156649015329 + (1/1 + ... + 1/(m - 1)) added in ascending order; from 16 on, with x = m and t = 1 / (x x),
 * log(x) - 0.5 / x - t (1/12 - t (1/120 - t (1/252 - t (1/240 - t / 132)))), no FMA. */
#define SVAE_MI_MAX_K 32
#define SVAE_MI_MAX_Y 4
/* bytes of work that svae_mi_radius needs (0 for n < 2, k < 1, k > n - 1 or k > SVAE_MI_MAX_K): column chunks (at most 8, 1 once
 * the grid holds 512 blocks) x rows padded to 64 x k x 12 (a uint64 key and an int32 index per kept candidate) */
long long svae_mi_work(int n, int k);
int svae_mi_radius(const double* Z, int ld, int d, int n, const double* Y, int q, const int* lab, const int* kk, int k, void* work,
                   double* rho2, void* stream);
int svae_mi_counts(const double* Z, int ld, int d, int n, const double* Y, int q, const double* rho2, int* nz, int* ny, void* stream);
int svae_mi_psi_sums(const int* a, const int* b, long long n, double* out, void* stream);

/* ------------------------------------------------------- Conditional mutual information by kNN; local permutations (csrc/mi.hip) */
/* The integer parts of the kNN estimate of I(z; y | c) (Frenzel and Pompe 2007) and the draw of its local permutation null (Runge
 * 2018).  Z, Y, n, k and the squared distances s^z, s^y are those of svae_mi_radius (Y is always given here).  The condition is
 * either C [n][p] fp64 rows, contiguous, 1 <= p <= SVAE_CMI_MAX_C, with s^c_ij summed like s^y_ij, or clab [n] int32; exactly one
 * of the two is non-null.  The row itself is left out by index.
 *
 * svae_cmi_radius: rho2 [n].  With C: the k-th smallest max(s^z_ij, s^y_ij, s^c_ij) over j != i.  With clab: the k-th smallest
 * max(s^z_ij, s^y_ij) over the j != i with clab[j] == clab[i]; the caller guarantees that every class has more than k rows (with
 * fewer, rho2[i] is left unwritten).  The walk, buffer, finish kernel and svae_mi_work(n, k) workspace of svae_mi_radius.
 * svae_cmi_counts: int32 [n], strict, over j != i.  With C: nzc = #{max(s^z_ij, s^c_ij) < rho2[i]}, nyc = #{max(s^y_ij, s^c_ij) <
 * rho2[i]}, nc = #{s^c_ij < rho2[i]}.  With clab: nzc = #{clab[j] == clab[i], s^z_ij < rho2[i]}, nyc likewise with s^y, and nc
 * must be null (the class size is the host's).  Integer adds only: exact, independent of scheduling and of the column chunks.
 * The psi sums are svae_mi_psi_sums, called twice for the three arrays.
 *
 * svae_local_permutations: out [P][n] int32.  nbr [n][kp] int32 holds the donors of every row, order [P][n] int32 a visiting
 * order per permutation, scan [P][n][kp] uint8 per row a permutation of 0..kp-1.  For permutation p every row starts unused; the
 * rows are visited as i = order[p][t], t = 0..n-1; the donors j = nbr[i][scan[p][i][e]] are tried for e = 0, 1, ... up to the
 * first unused one, and when all kp are used the last one tried is kept (so a donor can serve twice); then out[p][i] = j and j
 * is used.  1 <= kp <= SVAE_CMI_MAX_DONORS, 1 <= n <= 2^19 (the used-bitmap of a permutation sits in 64 KiB of LDS), 1 <= P <=
 * SVAE_MMD_NULL_MAX.  The caller guarantees the ranges of the entries; an entry out of range reads and marks nothing.  One wave per
 * permutation, one wave-step per visit; the result is a function of the inputs alone. */
#define SVAE_CMI_MAX_C 4
#define SVAE_CMI_MAX_DONORS 64
int svae_cmi_radius(const double* Z, int ld, int d, int n, const double* Y, int q, const double* C, int p, const int* clab, int k,
                    void* work, double* rho2, void* stream);
int svae_cmi_counts(const double* Z, int ld, int d, int n, const double* Y, int q, const double* C, int p, const int* clab,
                    const double* rho2, int* nzc, int* nyc, int* nc, void* stream);
int svae_local_permutations(const int* nbr, int n, int kp, const int* order, const unsigned char* scan, int P, int* out, void* stream);

/* ------------------------------------------------------- Ranks of given neighbours; embedding-quality sums (csrc/rank.hip) ---- */
/* svae_knn_ranks: X [n][ld] fp64 rows, not centred, d >= 1, 2 <= n < 2^31; idx [n][k] int32, 1 <= k <= min(n - 1, SVAE_KNN_MAX_K),
 * row i holding k distinct indices in [0, n), none equal to i.  rank [n][k] int32:
 *   rank[i][m] = 1 + #{l != i : key(i, l) < key(i, idx[i][m])}
 * with the strict key of svae_knn: the squared distance of csrc/pair_tiles.h (feature order, no FMA) compared by its uint64 bit
 * pattern, then the lower index.  Rank 1 is the nearest other row, rank n - 1 the farthest; the ranks of a row are distinct, and
 * with idx = the row's own svae_knn list they are 1..k.  One all-pairs pass with the sorted thresholds and a histogram of 64 rows
 * in LDS (41,472 B of staged rows + 128 k x 8 B: 133,632 B at k = 90), integer adds only: the result is exact and does not depend
 * on scheduling, on the column chunks or on the order of a row's entries.  Nothing of size n^2 is stored.  The caller guarantees
 * the conditions on idx; an entry that is out of range or equal to its row reads nothing and gets rank n, and a repeated entry
 * gets its one rank in both columns.
 * svae_rank_curves: from rank [n][k] (n >= 1, 1 <= k <= SVAE_KNN_MAX_K) whose column m belongs to the neighbour of order m + 1 in
 * the other space, for kk = 1..k:  pen[kk - 1] = sum_i sum_{m < kk} max(0, rank[i][m] - kk)  and
 * hit[kk - 1] = sum_i #{m < kk : rank[i][m] <= kk}, int64, by integer adds only.  With 1 <= row_k <= k, pen_row [n] int64
 * receives the inner sum of pen for kk = row_k per row; row_k = 0 and pen_row = NULL ask for none. */
/* bytes of work that svae_knn_ranks needs (0 for n < 2, k < 1, k > n - 1 or k > SVAE_KNN_MAX_K): n x k x 16 for the sorted
 * thresholds (a uint64 key, an int32 index and an int32 column each) + column chunks (at most 8, 1 once the grid holds 512
 * blocks) x n x k x 4 for the histograms */
long long svae_rank_work(int n, int k);
int svae_knn_ranks(const double* X, int ld, int d, int n, const int* idx, int k, void* work, int* rank, void* stream);
int svae_rank_curves(const int* rank, int n, int k, int row_k, long long* pen, long long* hit, long long* pen_row, void* stream);

/* ------------------------------------------------------- Kernel density of a 2-D embedding on a grid (csrc/density.hip) ----- */
/* Y [n][ld] fp64 points of the plane (ld >= 2, columns 0 and 1 are read), n >= 1; bandwidths h_rows [n], all > 0, or, with
 * h_rows = NULL, the one h > 0 (h^2 and 1 / (2 h^2) finite and positive).  The grid is x_a = x0 + a dx for a < gx and
 * y_b = y0 + b dy for b < gy, each node formed so in fp64 (one product, one sum), dx, dy > 0, 2 <= gx, gy <= SVAE_DENSITY_MAX_GRID.
 * D [gy][gx] fp64, row-major:
 *   D[b][a] = (1 / n) sum_i (1 / (2 pi h_i^2)) exp(-(x_a - Y[i][0])^2 / (2 h_i^2)) exp(-(y_b - Y[i][1])^2 / (2 h_i^2))
 * as the product B^T A of the two separable factors, generated 16 points at a time into LDS and multiplied on the fp64 matrix
 * cores, one 128 x 128 tile of D and one slice of the points per block; the slices (a function of n, gx, gy alone, at most 128)
 * are added in order.  Exact: no binning, no cutoff; a term that underflows is zero.  Bit-reproducible on every device. */
#define SVAE_DENSITY_MAX_GRID 1024
/* bytes of work that svae_density_grid needs (0 for n < 1 or a grid side outside 2..SVAE_DENSITY_MAX_GRID): slices x gy x gx x 8
 * for the partial grids + n x 16 for the per-point factors */
long long svae_density_work(int n, int gx, int gy);
/* work: 16-byte aligned, D: 8-byte aligned (SVAE_ERR_ALIGN otherwise) */
int svae_density_grid(const double* Y, int ld, int n, const double* h_rows /* NULL: use h */, double h, double x0, double dx, int gx,
                      double y0, double dy, int gy, void* work, double* D, void* stream);

/* ------------------------------------------------------- Entropic optimal transport between latent sets (csrc/ot.hip) -------- */
/* The two passes of a log-domain Sinkhorn solve between the query rows Q [m][ldq] and the candidate rows X [n][ldx], both fp64 of
 * d >= 1 features, 1 <= m, n < 2^26; nothing of size m x n is stored and every result is bit-reproducible.  With s_ij the squared
 * distance of csrc/pair_tiles.h (feature order, no FMA), the cost is c_ij = s_ij for kind = 0 (squared Euclidean) or the correctly
 * rounded sqrt(s_ij) for kind = 1 (Euclidean), and for the column offsets u [n] (finite)
 *     v_ij = u_j - c_ij * inv_eps,        inv_eps = the host's 1.0 / eps, finite and > 0: one product per pair, no division.
 *
 * svae_ot_softmin: L [m], L_i = log sum_j exp(v_ij) over all j < n, and with cbar [m] non-null
 * cbar_i = (sum_j exp(v_ij) c_ij) / (sum_j exp(v_ij)).  A streaming log-sum-exp: a thread (one query row, 16 candidates of every
 * 64-column tile) keeps a running maximum M and the sums scaled by exp(-M), rescaled once per tile; the (M, S) pairs of the four
 * waves merge as ((w0, w1), w2), w3 and those of the column chunks in chunk order, M = max, S = S1 exp(M1 - M) + S2 exp(M2 - M),
 * L = M + log(S).  The column chunks follow the rule of svae_knn_cross (at most 8, 1 once the grid holds 512 blocks; row tiles
 * counted from m, column tiles from n), so the order of every sum is a function of (m, n) alone.  A row's L does not depend on
 * the other rows of Q.  work: svae_ot_softmin_work doubles (0 for sizes out of range): 3 x column chunks x m padded to 64.
 *
 * svae_ot_apply: out [m][ldo], out_i = sum_j exp(v_ij - L_i) V_j for the c columns of V [n][ldv], 1 <= c <= SVAE_OT_MAX_COLS.
 * With L = svae_ot_softmin's of the same arguments this is the row-normalised transport plan times V; the weights lie in [0, 1]
 * up to rounding whatever the potentials.  The 64 x 64 tiles of weights are multiplied with V's rows on the fp64 matrix cores;
 * the chunks' partials are added in chunk order.  work: svae_ot_apply_work doubles (0 for sizes or c out of range): column
 * chunks x m padded to 64 x c padded to 16, 64 or 128. */
#define SVAE_OT_MAX_COLS 128
long long svae_ot_softmin_work(int m, int n);
int svae_ot_softmin(const double* Q, int ldq, int m, const double* X, int ldx, int n, int d, const double* u, double inv_eps, int kind,
                    double* work, double* L, double* cbar /* nullable */, void* stream);
long long svae_ot_apply_work(int m, int n, int c);
int svae_ot_apply(const double* Q, int ldq, int m, const double* X, int ldx, int n, int d, const double* u, double inv_eps, int kind,
                  const double* L, const double* V, int ldv, int c, double* work, double* out, int ldo, void* stream);

#ifdef __cplusplus
}
#endif
#endif
