// All-pairs squared distances of fp64 rows in 64 x 64 tiles, shared by hdbscan.hip and mmd.hip: a block of 256 threads holds 64 rows
// (lane = row, the same rows in each of the 4 waves) against 64 candidates (wave w takes candidates [16 w, 16 w + 16)), both staged
// through LDS 16 features at a time.  s = ((x0 - y0)^2 + (x1 - y1)^2) + ... in feature order, every subtract, multiply and add
// rounded on its own: the pragma below is part of the contract.
#pragma once

#pragma clang fp contract(off)

namespace svae {

constexpr int HR = 64;        // query rows per block: lane = row, the same rows in each of the 4 waves
constexpr int HT = 64;        // candidates per tile: wave w takes candidates [16 w, 16 w + 16) of it
constexpr int HQ = HT / 4;    // candidates per lane
constexpr int HD = 16;        // features per staged chunk (zero-padded past d: adds +0 to s, which changes nothing)
constexpr int HQLD = HR + 1;  // qs[j][row] row stride: conflict-free staging writes
constexpr int HQCH = 4;       // feature chunks of the block's rows kept in LDS for the whole kernel (d <= 64); more: restaged per tile

// query rows [r0, r0 + 64), features [j0, j0 + HD), zero outside: qs[j][row]
__device__ __forceinline__ void hdb_stage_rows(const double* __restrict__ X, int ld, int d, int n, long long r0, int j0, double* qs) {
  for (int e = threadIdx.x; e < HR * HD; e += 256) {
    const int r = e / HD, j = e - r * HD;
    const long long qr = r0 + r;
    qs[j * HQLD + r] = j0 + j < d && qr < n ? X[qr * ld + j0 + j] : 0.0;
  }
}

// candidates [c0, c0 + 64), features [j0, j0 + HD), zero outside: cs[cand][j]
__device__ __forceinline__ void hdb_stage_cands(const double* __restrict__ X, int ld, int d, int n, long long c0, int j0, double* cs) {
  for (int e = threadIdx.x; e < HT * HD; e += 256) {
    const int r = e / HD, j = e - r * HD;
    const long long cr = c0 + r;
    cs[r * HD + j] = j0 + j < d && cr < n ? X[cr * ld + j0 + j] : 0.0;
  }
}

// the block's rows for the whole kernel when they fit (visible after the first barrier of the tile loop)
__device__ __forceinline__ bool hdb_rows_resident(const double* __restrict__ X, int ld, int d, int n, long long r0, double* qs) {
  const int nch = (d + HD - 1) / HD;
  if (nch > HQCH) return false;
  for (int ch = 0; ch < nch; ++ch) hdb_stage_rows(X, ld, d, n, r0, ch * HD, qs + ch * HD * HQLD);
  return true;
}

// one feature chunk of a tile: the candidates (and the rows unless resident) staged, returns the rows' chunk
__device__ __forceinline__ const double* hdb_stage(const double* __restrict__ X, int ld, int d, int n, long long r0, long long c0,
                                                   int ch, bool resident, double* qs, double* cs) {
  __syncthreads();
  if (!resident) hdb_stage_rows(X, ld, d, n, r0, ch * HD, qs);
  hdb_stage_cands(X, ld, d, n, c0, ch * HD, cs);
  __syncthreads();
  return resident ? qs + ch * HD * HQLD : qs;
}

// s[q] += sum over the staged chunk of (row - cand_q)^2, feature by feature
__device__ __forceinline__ void hdb_accumulate(const double* qs, const double* cs, int lane, int wave, double (&s)[HQ]) {
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

}  // namespace svae
