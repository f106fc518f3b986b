// Shared by the forward / data-gradient translation units of the split-precision implicit GEMM (gemm_bf16s.hip: per-tap gather
// kernels, the 8-wave halo kernel, dispatch and C entry points; halo_ws_bf16s.hip: the wave-specialised halo kernels): launch
// arguments, the epilogue (bias, accumulate, fused BatchNorm sums), the halo-image row bound, and what a tile code launches
// (split_gather_geometry, with the list of the variants).
#pragma once
#include "split_common.h"

namespace svae {

constexpr int SBK = 32;  // K depth of one LDS stage: a 128-byte line of every gathered fp32 row

struct SplitGatherArgs {
  GatherArgs g;               // g.W / g.ldW / g.w_tap_stride unused
  const unsigned short* Wp;   // weight pieces, pre-tiled [piece][tap][k/32][n][32] (zero padded in k)
  long long w_piece_stride;   // elements between piece planes
  long long rowsA;            // rows of the gathered operand (batch * Lin): bound of the halo image
  int KB;                     // 32-deep k blocks per tap
  float* up_out;              // g.up: where the upsampled operand rows go as a by-product ([rowsA][ldA], NULL: nowhere)
};

// One element's share of the epilogue's sums, with every rounding pinned (forward: `mu` carries the column's pivot, and the sums
// are those of v - pivot; a pivot of 0 leaves v as it is): u = fma(x, scale, shift), 1 - t^2 = fma(-t, t, 1) and
// the fp64 slope term are fused, while sum v^2 and sum du * xhat are a ROUNDED product added to the sum.  That is what every
// instance of these kernels computed while the choice was the compiler's (it pairs (sum, sum of squares) into a packed add, which
// keeps the multiply apart); pinned, because the two paths of one instance would otherwise be free to round differently.
__device__ __forceinline__ void epilogue_sums(float v, float x, bool bwd, bool th, float slope, float sc, float sh, float mu, float rs,
                                              float& cs, float& cq, double& da) {
#pragma clang fp contract(off)
  if (bwd) {
    const float u = __builtin_fmaf(x, sc, sh);
    float du;
    if (th) { const float t = tanhf(u); du = v * __builtin_fmaf(-t, t, 1.f); }
    else { du = u > 0.f ? v : slope * v; if (!(u > 0.f)) da = __builtin_fma((double)v, (double)u, da); }
    cs += du;
    const float p = du * (x - mu) * rs;
    cq += p;
  } else {
    const float d = v - mu;
    cs += d;
    const float p = d * d;
    cq += p;
  }
}

__device__ __forceinline__ void wave_lds_turn() {  // orders this wave's LDS writes and reads of other lanes' elements (LDS serves a wave in order)
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// ---- epilogue shared by the gather kernels: C (+)= acc + bias, and -- when g.stats != NULL -- the BatchNorm batch statistics of
// the values just written (reference: nn.BatchNorm1d in train mode right behind the conv, residual.py:88,112,146,173): per-column
// (sum (v - p), sum (v - p)^2) over the tile's valid rows, p = g.bn_pivot[column] (NULL: 0), go to stats[blockIdx.x][2][N], the
// layout bn_stats_partial writes per 128-row chunk,
// so the finalize kernel sums row tiles instead of chunks and the separate statistics pass over the conv output disappears.
// Fixed summation order (lane rows, the two half-waves, then the WR row-waves): bit-reproducible.
//
// XW > 0 (the kernel's staging LDS holds 4 KiB for each of its XW epilogue waves, and every wave is past its last operand read
// when the epilogue starts): the wide path.  The 32 x 32 accumulator layout gives a lane ONE column and 16 rows of a block, so the
// plain path moves one dword per register: 16 stores (and 16 loads each of the old C under accumulate and of bn_x) per block.  The
// wide path turns each block through the wave's own 32 x 32 fp32 LDS region -- row stride 32 dwords: the 32 lanes of a
// ds_write_b32 / ds_read_b32 group walk one row, and the 16 lanes of a ds_read_b128 group cover four 64-byte row halves on four
// different bank quarters, so neither direction conflicts -- and moves it as 4 x 16 bytes per lane: lane = 4 consecutive columns
// of row lane / 8 + 8 i.  The operands that come in take the reverse trip, all requested before the first one is turned.  Every value and every sum
// is formed per element in the accumulator layout in the (nt, mt, r) order of the plain path: same bits.  Taken when
// g.wide_epi is set, the epilogue READS (accumulate or fused sums: a launch that only stores gains nothing) and C, bn_x
// and ldC are 16-byte aligned (wave-uniform); else the plain path.
template <int MT, int NT, int WM, int WN, int WR, int BN, int XW = 0>
__device__ __forceinline__ void tile_epilogue(const GatherArgs& g, f32x16 (&acc)[MT][NT], const long long* rowoff, int n0, int wr, int wc,
                                              int lr, int h, float* red, int tid, int nth, float oscale = 1.f, int tile_x = -1,
                                              int tile_y = 0) {
  if (tile_x < 0) { tile_x = blockIdx.x; tile_y = blockIdx.y; }  // (row tile, column tile) of this workgroup
  float cs[NT], cq[NT];
  double da = 0.0;  // the PReLU slope's partial: a sum of ~1e6 cancelling terms over the launch -- fp64 products and sums
  const bool bwd = g.bn_x != nullptr;        // uniform
  const bool th = g.bn_alpha == nullptr;     // tanh instead of PReLU
  const float slope = (bwd && !th) ? g.bn_alpha[0] : 0.f;
  bool wide = false;
  if constexpr (XW > 0)  // a launch that only stores gains nothing from the wide path
    wide = g.wide_epi && (g.accumulate || bwd) && ((g.ldC | g.N) & 3) == 0 &&
           ((reinterpret_cast<unsigned long long>(g.C) | reinterpret_cast<unsigned long long>(g.bn_x)) & 15) == 0;
  if (wide) {
    float* xs = red + (tid >> 6) * 1024;  // this wave's block [32 rows][32 columns]
    const int qr = (tid & 63) >> 3, qc = (tid & 7) * 4;  // row layout: rows qr + 8 i, columns qc .. qc + 3
    const bool acc_in = g.accumulate != 0;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int col = n0 + wc * WN + nt * 32 + lr;
      const int c4 = n0 + wc * WN + nt * 32 + qc;
      const bool col_ok = col < g.N;
      cs[nt] = 0.f;
      cq[nt] = 0.f;
      if (n0 + wc * WN + nt * 32 >= g.N) continue;  // uniform: the block lies behind the matrix
      const float bv = (col_ok && g.bias) ? g.bias[col] : 0.f;
      float sc = 1.f, sh = 0.f, mu = 0.f, rs = 0.f;
      if (bwd && col_ok) {
        if (g.bn_scale) { sc = g.bn_scale[col]; sh = g.bn_shift[col]; }
        if (g.bn_mean) { mu = g.bn_mean[col]; rs = g.bn_rstd[col]; }
      } else if (col_ok && g.bn_pivot) {
        mu = g.bn_pivot[col];
      }
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        // what comes in: both requests first, then bn_x turns into registers and the old C stays in the region, where every
        // lane replaces its own 16 elements by the new values
        long long qoff[4];
        float4 po[4], px[4];
        float xv[16];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const long long off = rowoff[wr * WM + mt * 32 + qr + 8 * i];
          qoff[i] = (off >= 0 && c4 < g.N) ? off + c4 : -1;
          po[i] = px[i] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (bwd && qoff[i] >= 0) px[i] = *reinterpret_cast<const float4*>(g.bn_x + qoff[i]);
          if (acc_in && qoff[i] >= 0) po[i] = *reinterpret_cast<const float4*>(g.C + qoff[i]);
        }
        if (bwd) {
#pragma unroll
          for (int i = 0; i < 4; ++i) *reinterpret_cast<float4*>(xs + (qr + 8 * i) * 32 + qc) = px[i];
          wave_lds_turn();
#pragma unroll
          for (int r = 0; r < 16; ++r) xv[r] = xs[((r & 3) + 8 * (r >> 2) + 4 * h) * 32 + lr];
          wave_lds_turn();
        }
        if (acc_in) {
#pragma unroll
          for (int i = 0; i < 4; ++i) *reinterpret_cast<float4*>(xs + (qr + 8 * i) * 32 + qc) = po[i];
          wave_lds_turn();
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int lrow = (r & 3) + 8 * (r >> 2) + 4 * h;
          const long long off = rowoff[wr * WM + mt * 32 + lrow];
          float v = __builtin_fmaf(acc[mt][nt][r], oscale, bv);
          if (acc_in) v += xs[lrow * 32 + lr];
          xs[lrow * 32 + lr] = v;
          if (col_ok && off >= 0) epilogue_sums(v, bwd ? xv[r] : 0.f, bwd, th, slope, sc, sh, mu, rs, cs[nt], cq[nt], da);
        }
        wave_lds_turn();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float4 v4 = *reinterpret_cast<const float4*>(xs + (qr + 8 * i) * 32 + qc);
          if (qoff[i] >= 0) *reinterpret_cast<float4*>(g.C + qoff[i]) = v4;
        }
        wave_lds_turn();
      }
    }
  }
  if (!wide) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int col = n0 + wc * WN + nt * 32 + lr;
      cs[nt] = 0.f;
      cq[nt] = 0.f;
      if (col >= g.N) continue;
      const float bv = g.bias ? g.bias[col] : 0.f;
      float sc = 1.f, sh = 0.f, mu = 0.f, rs = 0.f;
      if (bwd) {
        if (g.bn_scale) { sc = g.bn_scale[col]; sh = g.bn_shift[col]; }
        if (g.bn_mean) { mu = g.bn_mean[col]; rs = g.bn_rstd[col]; }
      } else if (g.bn_pivot) {
        mu = g.bn_pivot[col];
      }
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = wr * WM + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
          const long long off = rowoff[row];
          if (off >= 0) {
            float* dst = g.C + off + col;
            float v = __builtin_fmaf(acc[mt][nt][r], oscale, bv);
            if (g.accumulate) v += *dst;
            *dst = v;
            epilogue_sums(v, bwd ? g.bn_x[off + col] : 0.f, bwd, th, slope, sc, sh, mu, rs, cs[nt], cq[nt], da);
          }
        }
      }
    }
  }
  if (g.stats == nullptr) return;  // uniform
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    cs[nt] += __shfl_xor(cs[nt], 32, 64);
    cq[nt] += __shfl_xor(cq[nt], 32, 64);
  }
  __syncthreads();  // every wave is past its last LDS operand read: the staging buffers are free
  if (h == 0) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int c = wc * WN + nt * 32 + lr;
      red[(0 * WR + wr) * BN + c] = cs[nt];
      red[(1 * WR + wr) * BN + c] = cq[nt];
    }
  }
  float* dred = red + 2 * WR * BN;  // one (hi, lo) slot per wave for the slope partial
  if (bwd && g.bn_dalpha) {
    da = wave_sum_d(da);
    if ((tid & 63) == 0) { const float hi = (float)da; dred[2 * (tid >> 6)] = hi; dred[2 * (tid >> 6) + 1] = (float)(da - (double)hi); }
  }
  __syncthreads();
  for (int i = tid; i < 2 * BN; i += nth) {
    const int k = i / BN, c = i - k * BN;
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < WR; ++w) t += red[(k * WR + w) * BN + c];
    if (n0 + c < g.N) g.stats[((long long)tile_x * 2 + k) * g.N + n0 + c] = t;
  }
  if (bwd && g.bn_dalpha && tid == 0) {  // the tile's partial leaves as a (hi, lo) float pair: the reduction kernels sum partials in fp64
    double t = 0.0;
    for (int w = 0; w < nth / 64; ++w) t += (double)dred[2 * w] + (double)dred[2 * w + 1];
    const float hi = (float)t;
    float* o = g.bn_dalpha + 2 * ((long long)tile_x * gridDim.y + tile_y);
    o[0] = hi;
    o[1] = (float)(t - (double)hi);
  }
}

// upper bound of the halo image rows over all BM-row tiles of both phases
inline int halo_rows(const GatherArgs& g, int bm) {
  int worst = 0;
  for (int p = 0; p < 2; ++p) {
    if (g.M[p] <= 0 || g.ntaps[p] <= 0) continue;
    int bmin = 1 << 30, bmax = -(1 << 30);
    for (int t = 0; t < g.ntaps[p]; ++t) {
      bmin = g.base[p][t] < bmin ? g.base[p][t] : bmin;
      bmax = g.base[p][t] > bmax ? g.base[p][t] : bmax;
    }
    const int nj = g.nj[p];
    int extra = g.Lin - nj * g.sj;  // additional anchor step at a sample boundary
    if (extra < 0) extra = 0;
    const int crossings = bm >= 2 ? (bm - 2) / nj + 1 : 0;
    const int span = (bm - 1) * g.sj + crossings * extra + (bmax - bmin) + 1;
    worst = span > worst ? span : worst;
  }
  return worst;
}

// raw staging ring of the 12-wave halo kernels (V = 16 .. 18): three slices of ceil(image rows / ntaps) rows (rounded up to 8) each
inline int ws4_slice_rows(const GatherArgs& g, int rmax) {
  int worst = 0;
  for (int p = 0; p < 2; ++p) {
    if (g.M[p] <= 0 || g.ntaps[p] <= 0) continue;
    const int sr = (((rmax + g.ntaps[p] - 1) / g.ntaps[p]) + 7) & ~7;
    worst = sr > worst ? sr : worst;
  }
  return worst;
}

// ---- The split forward / data-gradient launch of a tile code, resolved in ONE place: the launchers (launch_split_gather,
// launch_split_halo_ws) and the introspection calls (svae_conv_fwd_stats_tiles, svae_conv_dgrad_stats_tiles,
// svae_conv_split_tile) all read this.  A new variant is one case here and one launch line.
//
// Tile code V * 1000000 + BM * 1000 + BN (svae_conv_desc.tile[0 / 1]; BM, BN in {64, 128}); a code that does not decode (0) means
// the heuristic tile (pick_tile) on V = 1, and 8128NNN for a forward with the fused x2 upsample (g.up).  The variants:
//   0 / 1   gather_gemm_bf16s_kernel: 4 waves, double-buffered LDS / single LDS buffer
//   2 / 3   the same with 8 waves (4 x 2), single buffer / double-buffered (BM = 128)
//   4 / 5   gather_gemm_bf16s_ws_kernel: wave-specialised, 4 producer + 8 / 4 consumer waves, 2 tiles in flight (4: not 64 x 64)
//   6 / 7   as 4 / 5 with 3 tiles in flight
//   8       gather_halo_bf16s_kernel: the halo-image kernel, 8 waves, 128-row tiles; images of 160 / 264 rows; 2 or 3 pieces; up2
//   9       the same on 256-row tiles (8 waves of 64 x 64): half the weight-piece bytes per FLOP through the vector-memory path, pays
//           once the problem has >= 2 x 256 such row tiles; images of 320 / 528 rows (3 pieces and 528 rows: 64 columns only;
//           up2: 320 rows only -- 6-tap convs on 256-row tiles need 298)
//   10 / 11 gather_halo_ws_bf16s_kernel: wave-specialised halo kernel (8 consumer + 2 producer waves), 128- / 256-row tiles, where
//           two image buffers + two weight stages fit the 160 KiB of LDS: images of 160 / 264 rows; 264 / 320 (320: 2 pieces)
//   12 / 13 the same with three weight-tile buffers (the producers request two stages ahead): 3 pieces on 64 columns only;
//           images of 160 / 264 rows; 264 rows
//   14 / 15 FOUR consumer waves with 128 x 64 wave tiles (one per SIMD) + 2 producers on the 256 x 128 tile: 25 % fewer LDS
//           fragment bytes per MFMA; compiler-scheduled / pinned (sched_barrier) pipeline; 2 pieces; images of 264 / 320 rows
//   16 / 17 gather_halo_ws4_bf16s_kernel: 8 consumer + 4 DMA-only loader waves, 256-row tiles, with / without the quarter-stage
//           stagger of the consumers' second half; 2 pieces; images of 264 / 320 rows beside a raw ring of 3 x 88 / 3 x 64 rows
//   18      as 16 on v_mfma_f32_16x16x32 (gather_halo_ws4m_bf16s_kernel)
//   19      the 8-wave halo kernel on 256 x 160 tiles, 8 x 1 waves of 32 x 160 (19128128: the fields are placeholders).  For the
//           output conv (141 -> 144 channels): ONE column tile instead of three 64-wide ones -- 10 % instead of 25 % of the matrix
//           work on padding columns, the image of a channel block staged once instead of three times.  2 pieces; 320 / 528 rows
//   29      the 8-wave halo kernel on 256 x 256 tiles, 4 x 2 waves of 64 x 128 (29128128: placeholders): a quarter fewer operand
//           bytes per multiply through the CU's fetch path than 256 x 128.  2 pieces; images of <= 320 rows; up2
// "2 pieces" includes the two fp16 pieces (SVAE_PIECES_F16X2).  Variants 9, 11 and 13 .. 19 carry 128 in the row field of their
// code and run 256-row tiles; V >= 20 other than 29 are the diagnostic variants of the ablation build (256-row tiles).
struct SplitGeo {
  int v;               // kernel variant
  int bm, bn;          // workgroup tile really used
  int code_bm;         // row field of the code
  int blocks_m[2];     // row tiles per phase
  unsigned grid_x, grid_y;
  int rows;            // halo variants: upper bound of the image rows over all tiles of both phases, else 0
  int rmax;            // halo variants: image rows the kernel instance is built with, else 0
  int status;          // SVAE_OK, or SVAE_ERR_SHAPE: this variant does not exist for the code's tile / pieces / image rows --
  const char* why;     // -- with this message, a format that takes why_arg
  int why_arg;
};

// pieces: of the launch (the tile does not depend on it: the introspection calls pass 2, which every variant is built for)
inline SplitGeo split_gather_geometry(const GatherArgs& g, int code, int pieces) {
  SplitGeo s = {};
  Tile t;
  if (!decode_tile(code, t)) { t = pick_tile(g.M[0], g.M[1], g.N); t.dma = 1; if (g.up) { t.bm = 128; t.dma = 8; } }
  const int v = s.v = t.dma;
  const bool rows256 = v == 9 || v == 11 || v >= 13;
  s.code_bm = t.bm;
  s.bm = rows256 ? 256 : t.bm;
  s.bn = v == 19 ? 160 : (v == 29 ? 256 : t.bn);
  for (int p = 0; p < 2; ++p) s.blocks_m[p] = (int)((g.M[p] + s.bm - 1) / s.bm);
  s.grid_x = (unsigned)(s.blocks_m[0] + s.blocks_m[1]);
  s.grid_y = (unsigned)((g.N + s.bn - 1) / s.bn);
  int r0 = 0, r1 = 0;  // the image rows the variant's kernels are built with
  switch (v) {
    case 8: case 10: case 12: r0 = 160; r1 = 264; break;
    case 9: case 19: r0 = 320; r1 = 528; break;
    case 11: case 14: case 15: case 16: case 17: case 18: r0 = 264; r1 = 320; break;
    case 13: r0 = r1 = 264; break;
    case 29: r0 = r1 = 320; break;
    default: break;
  }
  if (r0) {
    s.rows = halo_rows(g, rows256 ? 256 : 128);
    s.rmax = s.rows <= r0 ? r0 : r1;
  }

  // does the combination exist?
  auto refuse = [&s](const char* why, int arg) { s.status = SVAE_ERR_SHAPE; s.why = why; s.why_arg = arg; return s; };
  static const char* const unsupported = "split gather: tile code %d unsupported";
  static const char* const not_affine = "split gather: tap tables are not arithmetic progressions";
  const bool two = pieces == 2 || pieces == SVAE_PIECES_F16X2, two_three = two || pieces == 3;
  const int rows = s.rows;
  if (g.up && v != 8 && v != 9 && v != 29)
    return refuse("split gather: the fused x2 upsample of the input exists in the halo kernels (tile codes 8 / 9 / 29), not in code %d", code);
  switch (v) {
    case 0: case 1: case 5: case 7: break;
    case 2: case 3:
      if (t.bm != 128) return refuse(unsupported, code);
      break;
    case 4: case 6:
      if (t.bm != 128 && t.bn != 128) return refuse(unsupported, code);
      break;
    case 8:
      if (t.bm != 128) return refuse(unsupported, code);
      if (!two_three) return refuse("split gather: the halo kernel is built for 2 or 3 pieces", 0);
      if (rows > 264) return refuse("split gather: halo image of %d rows does not fit", rows);
      break;
    case 9:
      if (t.bm != 128) return refuse(unsupported, code);
      if (!two_three) return refuse("split gather: the halo kernel is built for 2 or 3 pieces", 0);
      if (rows > 528 || (pieces == 3 && rows > 320 && t.bn > 64)) return refuse("split gather: 256-row halo image of %d rows does not fit", rows);
      if (g.up && rows > 320) return refuse("split gather: the fused upsample exists for 256-row halo images of <= 320 rows (%d)", rows);
      break;
    case 10: case 11:
      if (t.bm != 128) return refuse(unsupported, code);
      if (!plan_is_affine(g)) return refuse(not_affine, 0);
      if (!two_three) return refuse("split gather: the halo kernels are built for 2 or 3 pieces", 0);
      if (v == 10 && rows > 264) return refuse("split gather: halo image of %d rows does not fit", rows);
      if (v == 11 && (rows > 320 || (rows > 264 && pieces == 3))) return refuse("split gather: 256-row halo image of %d rows does not fit twice", rows);
      break;
    case 12: case 13:
      if (t.bm != 128) return refuse(unsupported, code);
      if (!plan_is_affine(g)) return refuse(not_affine, 0);
      if (!two_three) return refuse("split gather: the halo kernels are built for 2 or 3 pieces", 0);
      if (pieces == 3 && t.bn != 64) return refuse("split gather: three weight buffers with 3 pieces exist for 64-column tiles only", 0);
      if (rows > 264) return refuse("split gather: halo image of %d rows does not fit", rows);
      break;
    case 14: case 15:
      if (t.bm != 128 || t.bn != 128) return refuse(unsupported, code);
      if (!plan_is_affine(g)) return refuse(not_affine, 0);
      if (!two) return refuse("split gather: the 128 x 64 wave tiles are built for 2 pieces", 0);
      if (rows > 320) return refuse("split gather: 256-row halo image of %d rows does not fit", rows);
      break;
    case 16: case 17: case 18:
      if (t.bm != 128) return refuse(unsupported, code);
      if (!plan_is_affine(g)) return refuse(not_affine, 0);
      if (!two) return refuse("split gather: the 12-wave halo kernel is built for 2 pieces", 0);
      if (rows > 320 || ws4_slice_rows(g, s.rmax) > (s.rmax == 264 ? 88 : 64))
        return refuse("split gather: 256-row halo image of %d rows / its raw slices do not fit", rows);
      break;
    case 19:
      if (t.bm != 128 || t.bn != 128) return refuse(unsupported, code);
      if (!two) return refuse("split gather: the 256 x 160 halo tile is built for 2 pieces", 0);
      if (rows > 528) return refuse("split gather: 256-row halo image of %d rows does not fit", rows);
      break;
    case 29:
      if (t.bm != 128 || t.bn != 128) return refuse(unsupported, code);
      if (!two) return refuse("split gather: the 256 x 256 halo tile is built for 2 pieces", 0);
      if (rows > 320) return refuse("split gather: 256 x 256 halo tile: image of %d rows does not fit", rows);
      break;
    default: return refuse(unsupported, code);
  }
  return s;
}

// what a launcher answers when it has no instance for a geometry the resolver let through (they must agree: not reached)
inline int split_no_instance(const SplitGeo& s, int pieces) {
  set_error("split gather: no kernel instance of variant %d for a %d x %d tile, %d pieces, %d image rows", s.v, s.bm, s.bn, pieces, s.rmax);
  return SVAE_ERR_SHAPE;
}

// wave-specialised halo kernels (halo_ws_bf16s.hip): variants 10 .. 18 of a geometry that exists
int launch_split_halo_ws(const SplitGatherArgs& sa, const SplitGeo& geo, dim3 grid, hipStream_t st, int pieces);
#ifdef SVAE_ABLATION_KERNELS
// the diagnostic variants (V >= 20 other than 29; g.blocks_m set): true when the launch was one of theirs, its status in *e
bool launch_split_halo_diag(const SplitGatherArgs& sa, const SplitGeo& geo, hipStream_t st, int pieces, int* e);
#endif

}  // namespace svae
