// All-pairs squared distances of fp64 rows in 64 x 64 tiles, the shared layer of hdbscan.hip, mmd.hip, mmd_null.hip,
// silhouette.hip, hsic.hip and, through knn_buffer.h, knn.hip, mi.hip and rank.hip: a block of 256 threads holds 64 rows (lane =
// row, the same rows in each of the 4 waves) against 64 candidates (wave w takes candidates [16 w, 16 w + 16)), both staged
// through LDS 16 features at a time.  (density.hip takes only double4_t and the matrix-core lane layout from here.)
// s = ((x0 - y0)^2 + (x1 - y1)^2) + ... in feature order, every subtract, multiply and add rounded on its own: the pragma below
// is part of the contract.  A kernel builds its block's rows once (pair_rows) and asks for one tile of s at a time (pair_tile).
#pragma once

#pragma clang fp contract(off)

namespace svae {

typedef unsigned long long u64;
typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int HR = 64;        // query rows per block: lane = row, the same rows in each of the 4 waves
constexpr int HT = 64;        // candidates per tile: wave w takes candidates [16 w, 16 w + 16) of it
constexpr int HQ = HT / 4;    // candidates per lane
constexpr int HD = 16;        // features per staged chunk (zero-padded past d: adds +0 to s, which changes nothing)
constexpr int HQLD = HR + 1;  // qs[j][row] row stride: conflict-free staging writes
constexpr int HQCH = 4;       // feature chunks of the block's rows kept in LDS for the whole kernel (d <= 64); more: restaged per tile

static_assert(HR == HT, "row tiles and column tiles are counted alike");
__host__ __device__ inline int pair_tile_count(int n) { return (int)(((long long)n + HT - 1) / HT); }  // no int overflow near 2^31

// query rows [r0, r0 + 64), features [j0, j0 + HD), zero outside: qs[j][row]
__device__ __forceinline__ void pair_stage_rows(const double* __restrict__ X, int ld, int d, int n, long long r0, int j0, double* qs) {
  for (int e = threadIdx.x; e < HR * HD; e += 256) {
    const int r = e / HD, j = e - r * HD;
    const long long qr = r0 + r;
    qs[j * HQLD + r] = j0 + j < d && qr < n ? X[qr * ld + j0 + j] : 0.0;
  }
}

// candidates [c0, c0 + 64), features [j0, j0 + HD), zero outside: cs[cand][j]
__device__ __forceinline__ void pair_stage_cands(const double* __restrict__ X, int ld, int d, int n, long long c0, int j0, double* cs) {
  for (int e = threadIdx.x; e < HT * HD; e += 256) {
    const int r = e / HD, j = e - r * HD;
    const long long cr = c0 + r;
    cs[r * HD + j] = j0 + j < d && cr < n ? X[cr * ld + j0 + j] : 0.0;
  }
}

// s[q] += sum over the staged chunk of (row - cand_q)^2, feature by feature
__device__ __forceinline__ void pair_accumulate(const double* qs, const double* cs, int lane, int wave, double (&s)[HQ]) {
  const double* cw = cs + wave * HQ * HD;
#pragma unroll 4
  for (int j = 0; j < HD; ++j) {
    const double a = qs[j * HQLD + lane];
#pragma unroll
    for (int q = 0; q < HQ; ++q) {
      const double e = a - cw[q * HD + j];
      const double m = e * e;
      s[q] = s[q] + m;
    }
  }
}

// This block's 64 rows [r0, r0 + 64) of X [n] against the nc candidate rows of C (X itself unless a kernel searches one matrix
// against another, as knn_cross_lists_kernel): qs [HQCH * HD * HQLD] and cs [HT * HD] doubles of LDS
struct PairRows {
  const double* X;
  int ld, d, n, nch;  // nch feature chunks
  const double* C;    // the candidates [nc][ldc], of the same d features
  int ldc, nc;
  long long r0;
  bool resident;      // the rows stay in qs for the whole kernel; otherwise every tile restages them chunk by chunk
  double *qs, *cs;
  int lane, wave;
};

// stages the rows for the whole kernel when they fit (visible after the first barrier of the first pair_tile)
__device__ __forceinline__ PairRows pair_rows(const double* __restrict__ X, int ld, int d, int n, long long r0, double* qs, double* cs,
                                              const double* __restrict__ C = nullptr, int ldc = 0, int nc = 0) {
  const int nch = (d + HD - 1) / HD;
  bool resident = false;
  if (nch <= HQCH) {
#pragma unroll 1  // once per block: unrolled, this staging code is three times the size and nothing is faster
    for (int ch = 0; ch < nch; ++ch) pair_stage_rows(X, ld, d, n, r0, ch * HD, qs + ch * HD * HQLD);
    resident = true;
  }
  if (!C) C = X, ldc = ld, nc = n;
  return PairRows{X, ld, d, n, nch, C, ldc, nc, r0, resident, qs, cs, (int)(threadIdx.x & 63), (int)(threadIdx.x >> 6)};
}

// s[q] = the squared distance of row r0 + lane to candidate c0 + 16 wave + q.  Every thread of the block takes the two barriers
// of each chunk (the first one also ends whatever the block did with LDS before the call); a wave with live = false (wave-uniform)
// skips the arithmetic and gets zeros.
__device__ __forceinline__ void pair_tile(const PairRows& p, long long c0, double (&s)[HQ], bool live = true) {
#pragma unroll
  for (int q = 0; q < HQ; ++q) s[q] = 0.0;
  for (int ch = 0; ch < p.nch; ++ch) {
    __syncthreads();
    if (!p.resident) pair_stage_rows(p.X, p.ld, p.d, p.n, p.r0, ch * HD, p.qs);
    pair_stage_cands(p.C, p.ldc, p.d, p.nc, c0, ch * HD, p.cs);
    __syncthreads();
    if (live) pair_accumulate(p.resident ? p.qs + ch * HD * HQLD : p.qs, p.cs, p.lane, p.wave, s);
  }
}

// Block (x, y) takes row tile x against the column tiles [y ch, (y + 1) ch) of the n_cols candidates
struct PairTileRange {
  long long r0;
  int t_lo, t_hi;  // column tiles [t_lo, t_hi); empty (block-uniform) when t_lo >= t_hi
};
__device__ __forceinline__ PairTileRange pair_chunk_tiles(int n_cols, int ch) {
  return PairTileRange{(long long)blockIdx.x * HR, (int)blockIdx.y * ch, min(((int)blockIdx.y + 1) * ch, pair_tile_count(n_cols))};
}
// Upper triangle i < j: of that chunk, the tiles on or above the diagonal
__device__ __forceinline__ PairTileRange pair_upper_tiles(int n, int ch) {
  PairTileRange t;
  t.r0 = (long long)blockIdx.x * HR;
  t.t_lo = max((int)blockIdx.y * ch, (int)blockIdx.x);
  t.t_hi = min(((int)blockIdx.y + 1) * ch, pair_tile_count(n));
  return t;
}

// ---- a tile as the A operand of the fp64 matrix cores (mmd_null.hip, silhouette.hip) ---------------------------------------------
// Dynamic LDS, in doubles: the prefix every such kernel shares; its own regions follow from PAIR_LDS_END.
constexpr int PAIR_LDS_QS = 0;                                // the block's rows (PairRows::qs)
constexpr int PAIR_LDS_CS = PAIR_LDS_QS + HQCH * HD * HQLD;   // candidates of the tile (PairRows::cs)
constexpr int PAIR_LDS_KT = PAIR_LDS_CS + HT * HD;            // kt[j][i]: the tile of values, column-major
constexpr int PAIR_LDS_END = PAIR_LDS_KT + HT * HR;

// v_mfma_f64_16x16x4_f64: lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15] of each 16 x 16 x 4 step, and
// register r of C/D holds [row (l >> 4) + 4 r][col l & 15].  Wave w multiplies rows [16 w, 16 w + 16) of the tile with all of the
// kernel's columns; step ks covers the tile's columns j = 4 ks + k.
// the value of (row lane, candidate 16 wave + q), as pair_tile hands them out
__device__ __forceinline__ double& pair_kt_value(double* kt, int lane, int wave, int q) { return kt[(wave * HQ + q) * HR + lane]; }
// A of this lane for column j of the tile
__device__ __forceinline__ double pair_kt_a(const double* kt, int j, int wave, int l16) { return kt[j * HR + 16 * wave + l16]; }

}  // namespace svae
