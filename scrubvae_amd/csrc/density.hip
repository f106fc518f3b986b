// Gaussian kernel density of n fp64 points of the plane on a regular gx x gy grid, exact: no binning, no cutoff, no recurrence.
//     D[b][a] = (1 / n) sum_i c_i exp(-(x_a - Y[i][0])^2 s_i) exp(-(y_b - Y[i][1])^2 s_i),   s_i = 1 / (2 h_i^2), c_i = s_i / pi
// with the nodes x_a = x0 + a dx and y_b = y0 + b dy formed exactly so (one product, one sum, no fma).  The kernel is separable, so
// D = B^T A with A[i][a] = exp(-(x_a - Y[i][0])^2 s_i) and B[i][b] = c_i exp(-(y_b - Y[i][1])^2 s_i): a (gy x n) by (n x gx)
// product whose operands cost DEN_T + DEN_T exponentials per point and tile instead of DEN_T^2.  A block owns one 128 x 128 tile
// of D and one slice of the points.  Per stage of 16 points its 256 threads write the stage's 16 x 128 entries of A and of B to
// LDS (8 + 8 exponentials each), and wave w multiplies its 64 x 64 quarter on the fp64 matrix cores (v_mfma_f64_16x16x4_f64,
// lane layout: pair_tiles.h), 16 accumulator tiles of 4 doubles per lane.  Nothing of size n x G is stored.
// The order of every sum is fixed by the schedule: the MFMA's k order within a chunk, the chunks of a slice in order, the slices
// added by the finish kernel in order (compensated, fixed_sum.h).  The number of slices depends on (n, gx, gy) alone, not on the
// device, so D is bit-identical from run to run and from device to device.  A contribution that underflows is zero and stays zero.
// With one bandwidth for all points c is applied once per cell by the finish kernel; with per-point bandwidths a first kernel
// writes (s_i, c_i) to work, so that the division is done once per point and not once per exponential.
#include "svae_internal.h"

#include <algorithm>

#include "pair_tiles.h"  // double4_t, the f64 MFMA lane layout and #pragma clang fp contract(off): the exponent is formed as written
#include "fixed_sum.h"   // the compensated sum over the slices

namespace svae {

constexpr int DEN_T = 128;          // a tile of D is DEN_T x DEN_T cells; wave w owns rows [64 (w >> 1), +64) x columns [64 (w & 1), +64)
constexpr int DEN_CHUNK = 32;       // points per chunk: the unit the slices are counted in
constexpr int DEN_STAGE = 16;       // points generated and multiplied per step: half a chunk in each of the two LDS buffers
constexpr int DEN_LD = DEN_T + 16;  // row stride of the staged operands in doubles: the 4 k rows of an MFMA step fall on distinct banks
constexpr int DEN_BLOCKS = 512;     // the points are sliced only while the grid holds fewer blocks than this
constexpr int DEN_MAX_SLICES = 128;
constexpr int DEN_BUF = 2 * DEN_STAGE * DEN_LD;  // doubles per buffer: the stage's rows of A, then of B
constexpr size_t DEN_LDS = (size_t)2 * DEN_BUF * sizeof(double);  // 73,728 B: two blocks per CU
static_assert(2 * DEN_LDS <= 160 * 1024, "two workgroups per CU");
static_assert(DEN_CHUNK % DEN_STAGE == 0 && DEN_STAGE == 16 && 256 / DEN_T == 2, "a quarter of a stage is two rows per thread pair");

constexpr double DEN_INV_PI = 0.31830988618379067154;  // 1 / pi rounded to fp64

// sc[i] = (s_i, c_i) from h_i
__global__ __launch_bounds__(256) void den_rows_kernel(const double* __restrict__ h, int n, double2* __restrict__ sc) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double q = 2.0 * (h[i] * h[i]);
  const double s = 1.0 / q;
  sc[i] = make_double2(s, s * DEN_INV_PI);
}

// One quarter of a stage of DEN_STAGE points into buf: rows irow + 2 (2 part + j), j < 2, of A (first) and B (second half of buf).
// Branch-free: a row past n reads row n - 1 and writes 0, so the exponentials can be scheduled into the shadow of the MFMAs.
template <bool ROWS>
__device__ __forceinline__ void den_stage_part(const double* __restrict__ Y, int ld, int n, const double2* __restrict__ sc, double s1, double xa,
                                               double yb, int i0, int part, int irow, int col, double* buf) {
#pragma unroll
  for (int j = 0; j < DEN_STAGE / 8; ++j) {
    const int r = irow + (256 / DEN_T) * ((DEN_STAGE / 8) * part + j);
    const int i = i0 + r;
    const long long ic = min(i, n - 1);
    const double px = Y[ic * ld], py = Y[ic * ld + 1];
    double s = s1, c = 1.0;
    if (ROWS) {
      const double2 v = sc[ic];
      s = v.x;
      c = v.y;
    }
    const double ex = xa - px, ey = yb - py;
    const double qx = ex * ex, qy = ey * ey;
    const double ax = -(qx * s), ay = -(qy * s);
    const double av = exp(ax);
    const double by = exp(ay);
    const double bv = ROWS ? c * by : by;
    buf[r * DEN_LD + col] = i < n ? av : 0.0;  // a row past n adds nothing
    buf[(DEN_STAGE + r) * DEN_LD + col] = i < n ? bv : 0.0;
  }
}

// part[(slice * gy + b) * gx + a] = sum over the points of the slice of B[i][b] A[i][a]; ROWS: (s_i, c_i) from sc, else s and c = 1.
// Two LDS buffers: while the waves multiply the stage in one, they write the next stage to the other, a quarter of it between the
// four k steps, so that the exponentials (VALU) run beside the MFMAs of the same wave; one barrier per stage.
template <bool ROWS>
__global__ __launch_bounds__(256) void den_tile_kernel(const double* __restrict__ Y, int ld, int n, const double2* __restrict__ sc, double s1,
                                                       double x0, double dx, int gx, double y0, double dy, int gy, int cps,
                                                       double* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l16 = lane & 15, kg = lane >> 4;
  const int a0 = (int)blockIdx.x * DEN_T, b0 = (int)blockIdx.y * DEN_T;
  constexpr int SPC = DEN_CHUNK / DEN_STAGE;  // stages per chunk
  const int nstages = (n + DEN_STAGE - 1) / DEN_STAGE;
  const int s_lo = (int)blockIdx.z * cps * SPC, s_hi = min(s_lo + cps * SPC, nstages);
  // this thread's column of the staged operands and the node it belongs to (past the grid: computed, never stored)
  const int col = tid & (DEN_T - 1), irow = tid / DEN_T;
  const double pa = (double)(a0 + col) * dx;
  const double xa = x0 + pa;
  const double pb = (double)(b0 + col) * dy;
  const double yb = y0 + pb;
  const int wr = 64 * (wave >> 1), wc = 64 * (wave & 1);
  double4_t acc[4][4];
#pragma unroll
  for (int rb = 0; rb < 4; ++rb)
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) acc[rb][cb] = double4_t{0.0, 0.0, 0.0, 0.0};
  double* rd = lds;             // the stage being multiplied: A[i][a] then B[i][b]
  double* wt = lds + DEN_BUF;   // the stage being written
#pragma unroll
  for (int q = 0; q < 4; ++q) den_stage_part<ROWS>(Y, ld, n, sc, s1, xa, yb, s_lo * DEN_STAGE, q, irow, col, rd);
  for (int st = s_lo; st < s_hi; ++st) {
    __syncthreads();  // rd is written, and the reads of wt by the previous stage are done
    const int inext = (st + 1) * DEN_STAGE;  // past s_hi: written, never read
#pragma unroll
    for (int ks = 0; ks < DEN_STAGE / 4; ++ks) {
      const double* ar = rd + (4 * ks + kg) * DEN_LD + wc + l16;
      const double* br = rd + (DEN_STAGE + 4 * ks + kg) * DEN_LD + wr + l16;
      double bop[4], aop[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        bop[t] = br[16 * t];
        aop[t] = ar[16 * t];
      }
      // rows of D come from B (the MFMA's A operand), columns from A (its B operand)
#pragma unroll
      for (int rb = 0; rb < 4; ++rb)
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) acc[rb][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(bop[rb], aop[cb], acc[rb][cb], 0, 0, 0);
      den_stage_part<ROWS>(Y, ld, n, sc, s1, xa, yb, inext, ks, irow, col, wt);
    }
    double* t = rd;
    rd = wt;
    wt = t;
  }
  // acc[rb][cb][r] is [row wr + 16 rb + (l >> 4) + 4 r][col wc + 16 cb + (l & 15)] of the tile; cells past the grid are dropped
  double* out = part + (long long)blockIdx.z * gy * gx;
#pragma unroll
  for (int rb = 0; rb < 4; ++rb)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int b = b0 + wr + 16 * rb + kg + 4 * r;
      if (b >= gy) continue;
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) {
        const int a = a0 + wc + 16 * cb + l16;
        if (a < gx) out[(long long)b * gx + a] = acc[rb][cb][r];
      }
    }
}

// D[cell] = ((sum over the slices, in order, compensated) * c) / n
__global__ __launch_bounds__(256) void den_finish_kernel(const double* __restrict__ part, int slices, long long cells, double c, double n,
                                                         double* __restrict__ D) {
  const long long cell = (long long)blockIdx.x * 256 + threadIdx.x;
  if (cell >= cells) return;
  double sum = 0.0, comp = 0.0;
  for (int z = 0; z < slices; ++z) neumaier_add(sum, comp, part[z * cells + cell]);
  const double total = sum + comp;
  const double scaled = total * c;
  D[cell] = scaled / n;
}

}  // namespace svae

using namespace svae;

struct DenPlan {
  unsigned tx, ty, slices;
  int cps;  // chunks per slice
};

static bool den_sizes_ok(int n, int gx, int gy) {
  return n >= 1 && n <= (1 << 30) && gx >= 2 && gy >= 2 && gx <= SVAE_DENSITY_MAX_GRID && gy <= SVAE_DENSITY_MAX_GRID;
}

// a function of (n, gx, gy) alone: the sums, and so the bits of D, do not depend on the device
static DenPlan den_plan(int n, int gx, int gy) {
  DenPlan p;
  p.tx = (unsigned)((gx + DEN_T - 1) / DEN_T);
  p.ty = (unsigned)((gy + DEN_T - 1) / DEN_T);
  const int nchunks = (int)(((long long)n + DEN_CHUNK - 1) / DEN_CHUNK);
  const ChunkSplit s = chunk_split(nchunks, (long long)p.tx * p.ty, DEN_MAX_SLICES, DEN_BLOCKS);
  p.cps = s.per;
  p.slices = (unsigned)s.parts;
  return p;
}

extern "C" long long svae_density_work(int n, int gx, int gy) {
  if (!den_sizes_ok(n, gx, gy)) return 0;
  const DenPlan p = den_plan(n, gx, gy);
  return ((long long)p.slices * gy * gx + 2ll * n) * (long long)sizeof(double);
}

template <bool ROWS>
static int den_launch(const DenPlan& p, const double* Y, int ld, int n, const double2* sc, double s, double x0, double dx, int gx, double y0,
                      double dy, int gy, double* part, hipStream_t st) {
  static DeviceOnce once;
  if (int e = allow_lds(den_tile_kernel<ROWS>, once, (int)DEN_LDS, "density_grid")) return e;
  hipLaunchKernelGGL(den_tile_kernel<ROWS>, dim3(p.tx, p.ty, p.slices), dim3(256), DEN_LDS, st, Y, ld, n, sc, s, x0, dx, gx, y0, dy, gy, p.cps,
                     part);
  return check_launch("density_tiles");
}

extern "C" int svae_density_grid(const double* Y, int ld, int n, const double* h_rows, double h, double x0, double dx, int gx, double y0,
                                 double dy, int gy, void* work, double* D, void* stream) {
  SVAE_REQUIRE(Y && n >= 1 && n <= (1 << 30) && ld >= 2, SVAE_ERR_ARG, "density_grid: bad rows (n=%d ld=%d)", n, ld);
  SVAE_REQUIRE(gx >= 2 && gy >= 2 && gx <= SVAE_DENSITY_MAX_GRID && gy <= SVAE_DENSITY_MAX_GRID, SVAE_ERR_ARG,
               "density_grid: bad grid (gx=%d gy=%d, 2 to %d each)", gx, gy, SVAE_DENSITY_MAX_GRID);
  SVAE_REQUIRE(dx > 0.0 && dy > 0.0 && dx <= 1.79e308 && dy <= 1.79e308 && x0 - x0 == 0.0 && y0 - y0 == 0.0, SVAE_ERR_ARG,
               "density_grid: bad grid steps (x0=%g dx=%g y0=%g dy=%g)", x0, dx, y0, dy);
  const double s = 1.0 / (2.0 * (h * h));  // h^2 must neither underflow nor overflow
  SVAE_REQUIRE(h_rows || (h > 0.0 && s > 0.0 && s <= 1.79e308), SVAE_ERR_ARG, "density_grid: bad bandwidth (h=%g)", h);
  SVAE_REQUIRE(work && D, SVAE_ERR_ARG, "density_grid: null argument");
  SVAE_REQUIRE(aligned16(work) && (reinterpret_cast<uintptr_t>(D) & 7u) == 0, SVAE_ERR_ALIGN,
               "density_grid: work must be 16-byte aligned and D 8-byte aligned");
  const DenPlan p = den_plan(n, gx, gy);
  const long long cells = (long long)gy * gx;
  double2* sc = static_cast<double2*>(work);           // [n] (s_i, c_i), 16-byte aligned
  double* part = static_cast<double*>(work) + 2ll * n;  // [slices][gy][gx]
  int e;
  double c = 1.0;
  if (h_rows) {
    hipLaunchKernelGGL(den_rows_kernel, dim3((unsigned)(((long long)n + 255) / 256)), dim3(256), 0, ST(stream), h_rows, n, sc);
    if ((e = check_launch("density_rows"))) return e;
    e = den_launch<true>(p, Y, ld, n, sc, 0.0, x0, dx, gx, y0, dy, gy, part, ST(stream));
  } else {
    c = s * DEN_INV_PI;
    e = den_launch<false>(p, Y, ld, n, nullptr, s, x0, dx, gx, y0, dy, gy, part, ST(stream));
  }
  if (e) return e;
  hipLaunchKernelGGL(den_finish_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, ST(stream), part, (int)p.slices, cells, c,
                     (double)n, D);
  return check_launch("density_finish");
}
