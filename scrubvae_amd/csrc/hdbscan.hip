// HDBSCAN clustering of latents (reference eval/cluster.py::dbscan, which runs sklearn's HDBSCAN): core distances and the
// Boruvka rounds of the mutual-reachability minimum spanning tree on the device, in fp64; the single-linkage tree, the condensed
// tree, cluster selection, labels and probabilities in plain C++ on the host.
//
// Arithmetic contract (what makes the numpy restatement in tests/hdbscan_checks.py bit-equal): the squared distance of rows x, y
// is s = ((x0 - y0)^2 + (x1 - y1)^2) + ..., summed in feature order, every subtract, multiply and add rounded on its own (no FMA:
// the pragma below), the distance is the correctly rounded sqrt(s).  This is the arithmetic of sklearn's KD-tree euclidean metric.
// The core distance of a row is the k-th smallest of its n distances (itself included at 0).  Mutual reachability is
// max(core_i, core_j, d_ij / alpha).  MST edges are ordered by the strict key (w, min(i, j), max(i, j)), so the tree is unique
// and nothing depends on thread scheduling.
#include "svae_internal.h"

#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

#include "pair_tiles.h"  // the tile walk and #pragma clang fp contract(off)

namespace svae {

constexpr int HBINS = 256;
constexpr int HHLD = HBINS + 1;  // histogram row stride: a wave's 64 rows hitting one digit land in 64 different banks

__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// ---- core distances -----------------------------------------------------------------------------------------------------------
// Radix select of the k-th smallest squared distance per row over the uint64 bit pattern of s (non-negative doubles order like
// their bits), 8 bits per pass from the top, per-row 256-bin histograms in LDS.  Every pass recomputes the distances.  A row whose
// selected bin holds a single candidate fetches that candidate's s in the next pass and stops; after 8 passes the prefix is the
// value itself.  core[r] = sqrt(s_k).
__global__ __launch_bounds__(256) void hdb_core_kernel(const double* __restrict__ X, int ld, int d, int n, int k,
                                                       double* __restrict__ core) {
  __shared__ __attribute__((aligned(16))) double qs[HQCH * HD * HQLD];
  __shared__ __attribute__((aligned(16))) double cs[HT * HD];
  __shared__ unsigned hist[HR * HHLD];
  __shared__ unsigned long long st_pref[HR], st_mask[HR], st_val[HR];
  __shared__ unsigned st_krem[HR];
  __shared__ int st_shift[HR], st_mode[HR];  // mode 0: histogram, 1: fetch, 2: done
  __shared__ int any_left;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long r0 = (long long)blockIdx.x * HR;
  for (int e = threadIdx.x; e < HR * HHLD; e += 256) hist[e] = 0u;
  const PairRows rows = pair_rows(X, ld, d, n, r0, qs, cs);
  if (threadIdx.x < HR) {
    st_pref[lane] = 0ull;
    st_mask[lane] = 0ull;
    st_val[lane] = 0ull;
    st_krem[lane] = (unsigned)k;
    st_shift[lane] = 56;
    st_mode[lane] = r0 + lane < n ? 0 : 2;
  }
  __syncthreads();
  for (;;) {
    const unsigned long long pref = st_pref[lane], mask = st_mask[lane];
    const int shift = st_shift[lane], mode = st_mode[lane];
    for (long long c0 = 0; c0 < n; c0 += HT) {
      double s[HQ];
      pair_tile(rows, c0, s);
      if (mode != 2) {
#pragma unroll
        for (int q = 0; q < HQ; ++q) {
          const long long c = c0 + wave * HQ + q;
          const unsigned long long key = (unsigned long long)__double_as_longlong(s[q]);
          if (c < n && (key & mask) == pref) {
            if (mode == 1) st_val[lane] = key;  // the one candidate left in the bin
            else atomicAdd(&hist[lane * HHLD + (int)((key >> shift) & 255ull)], 1u);
          }
        }
      }
    }
    __syncthreads();
    if (wave == 0) {
      int m = st_mode[lane];
      if (m == 1) {
        m = 2;
      } else if (m == 0) {
        const unsigned krem = st_krem[lane];
        unsigned cum = 0u, below = 0u, cnt = 0u;
        int digit = -1;
        for (int b = 0; b < HBINS; ++b) {
          const unsigned h = hist[lane * HHLD + b];
          if (digit < 0 && cum + h >= krem) {
            digit = b;
            below = cum;
            cnt = h;
          }
          cum += h;
          hist[lane * HHLD + b] = 0u;
        }
        const int sh = st_shift[lane];
        st_krem[lane] = krem - below;
        st_pref[lane] |= (unsigned long long)digit << sh;
        st_mask[lane] |= 255ull << sh;
        if (sh == 0) {
          st_val[lane] = st_pref[lane];
          m = 2;
        } else {
          st_shift[lane] = sh - 8;
          if (cnt == 1u) m = 1;
        }
      }
      st_mode[lane] = m;
      const bool left = __any(m != 2);
      if (lane == 0) any_left = left;
    }
    __syncthreads();
    if (!any_left) break;
  }
  if (threadIdx.x < HR && r0 + lane < n) core[r0 + lane] = sqrt(__longlong_as_double((long long)st_val[lane]));
}

// ---- Boruvka ------------------------------------------------------------------------------------------------------------------
// Rows are in ascending order of core distance (X, core, id, comp all in that order; id = the row's index in the caller's order).
// Row i: the minimum key (w, min(id_i, id_j), max(id_i, id_j)) over j with comp[j] != comp[i], w = max(core_i, core_j, d_ij / alpha);
// wave v scans quarter v of every tile and the four minima are combined at the end.
// A candidate with core_j > best_i cannot win; candidates come in ascending core, so a block stops at the first tile whose first
// core exceeds every row's best, and a wave skips the arithmetic of a tile quarter whose first core exceeds all of its rows' best.
__global__ __launch_bounds__(256) void hdb_boruvka_kernel(const double* __restrict__ X, int ld, int d, int n,
                                                          const double* __restrict__ core, const int* __restrict__ id,
                                                          const int* __restrict__ comp, double alpha, double* __restrict__ bw,
                                                          unsigned long long* __restrict__ bp) {
  __shared__ __attribute__((aligned(16))) double qs[HQCH * HD * HQLD];
  __shared__ __attribute__((aligned(16))) double cs[HT * HD];
  __shared__ double ccore[HT];
  __shared__ int ccomp[HT], cid[HT];
  __shared__ double wmax[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long r0 = (long long)blockIdx.x * HR;
  const long long r = r0 + lane;
  const bool ok = r < n;
  const double ci = ok ? core[r] : 0.0;
  const int mycomp = ok ? comp[r] : -1;
  const unsigned myid = ok ? (unsigned)id[r] : 0u;
  double best = ok ? INFINITY : -INFINITY;
  const PairRows rows = pair_rows(X, ld, d, n, r0, qs, cs);
  unsigned long long bpk = ~0ull;
  for (long long c0 = 0; c0 < n; c0 += HT) {
    const double wm = wave_max_d(best);
    if (lane == 0) wmax[wave] = wm;
    __syncthreads();
    const double bmax = fmax(fmax(wmax[0], wmax[1]), fmax(wmax[2], wmax[3]));
    if (core[c0] > bmax) break;  // block-uniform
    if (threadIdx.x < HT) {
      const long long c = c0 + threadIdx.x;
      ccore[threadIdx.x] = c < n ? core[c] : INFINITY;
      ccomp[threadIdx.x] = c < n ? comp[c] : mycomp;
      cid[threadIdx.x] = c < n ? id[c] : 0;
    }
    double s[HQ];
    const long long cw0 = c0 + wave * HQ;
    const bool live = cw0 < n && !(core[cw0] > wm);  // wave-uniform
    pair_tile(rows, c0, s, live);
    if (live && ok) {
#pragma unroll
      for (int q = 0; q < HQ; ++q) {
        const int cl = wave * HQ + q;
        const double cj = ccore[cl];
        if (c0 + cl < n && ccomp[cl] != mycomp && !(cj > best)) {
          const double dist = sqrt(s[q]) / alpha;
          const double w = fmax(fmax(ci, cj), dist);
          const unsigned other = (unsigned)cid[cl];
          const unsigned lo = min(myid, other), hi = max(myid, other);
          const unsigned long long pk = ((unsigned long long)lo << 32) | hi;
          if (w < best || (w == best && pk < bpk)) {
            best = w;
            bpk = pk;
          }
        }
      }
    }
  }
  // each wave saw a quarter of every tile: the row's edge is the minimum key of the four
  __shared__ double fw[4 * HR];
  __shared__ unsigned long long fp[4 * HR];
  fw[wave * HR + lane] = best;
  fp[wave * HR + lane] = bpk;
  __syncthreads();
  if (wave == 0 && ok) {
    for (int v = 1; v < 4; ++v) {
      const double ow = fw[v * HR + lane];
      const unsigned long long op = fp[v * HR + lane];
      if (ow < best || (ow == best && op < bpk)) {
        best = ow;
        bpk = op;
      }
    }
    bw[r] = best;
    bp[r] = bpk;
  }
}

}  // namespace svae

namespace svae {

// cw[c] = min over rows of component c of the bits of bw (non-negative doubles order like their bits); cp[c] = min packed pair
// among the rows that reached that weight.  Both are order-independent atomic minima.
__global__ __launch_bounds__(256) void hdb_comp_init_kernel(unsigned long long* __restrict__ cw, unsigned long long* __restrict__ cp,
                                                            int C) {
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  if (c < C) {
    cw[c] = ~0ull;
    cp[c] = ~0ull;
  }
}

__global__ __launch_bounds__(256) void hdb_comp_weight_kernel(const double* __restrict__ bw, const int* __restrict__ comp, int n,
                                                              unsigned long long* __restrict__ cw) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r < n) atomicMin(cw + comp[r], (unsigned long long)__double_as_longlong(bw[r]));
}

__global__ __launch_bounds__(256) void hdb_comp_pair_kernel(const double* __restrict__ bw, const unsigned long long* __restrict__ bp,
                                                            const int* __restrict__ comp, int n, const unsigned long long* __restrict__ cw,
                                                            unsigned long long* __restrict__ cp) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r < n) {
    const int c = comp[r];
    if ((unsigned long long)__double_as_longlong(bw[r]) == cw[c]) atomicMin(cp + c, bp[r]);
  }
}

__global__ __launch_bounds__(256) void hdb_relabel_kernel(int* __restrict__ comp, int n, const int* __restrict__ map) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r < n) comp[r] = map[comp[r]];
}

// ---- host: union-find and the tree steps ---------------------------------------------------------------------------------------
struct Dsu {  // path halving; the caller picks the new root
  std::vector<long long> p;
  explicit Dsu(long long m) : p(m) { std::iota(p.begin(), p.end(), 0ll); }
  long long find(long long x) {
    while (p[x] != x) {
      p[x] = p[p[x]];
      x = p[x];
    }
    return x;
  }
};

// sklearn's TreeUnionFind (union by rank, ties to the first argument's root): labelling_at_cut numbers clusters by these roots
struct RankUnionFind {
  std::vector<long long> p;
  std::vector<long long> rank;
  explicit RankUnionFind(long long m) : p(m), rank(m, 0) { std::iota(p.begin(), p.end(), 0ll); }
  long long find(long long x) {
    long long r = x;
    while (p[r] != r) r = p[r];
    while (p[x] != r) {
      const long long nx = p[x];
      p[x] = r;
      x = nx;
    }
    return r;
  }
  void unite(long long x, long long y) {
    const long long xr = find(x), yr = find(y);
    if (rank[xr] < rank[yr]) p[xr] = yr;
    else if (rank[xr] > rank[yr]) p[yr] = xr;
    else {
      p[yr] = xr;
      rank[xr] += 1;
    }
  }
};

struct CondRow {
  long long parent, child;
  double lambda;
  long long size;
};

}  // namespace svae

using namespace svae;

static unsigned grid(int n, int per) { return (unsigned)(((long long)n + per - 1) / per); }  // no int overflow up to n = 2^31 - 1

extern "C" int svae_hdb_core(const double* X, int ld, int d, int n, int k, double* core, void* stream) {
  if (int e = check_pair_rows("hdb_core", X, ld, d, n, 1)) return e;
  SVAE_REQUIRE(core && k >= 1 && k <= n, SVAE_ERR_ARG, "hdb_core: bad args (k=%d n=%d)", k, n);
  if (k == 1) {  // the row itself, at distance 0
    const hipError_t e = hipMemsetAsync(core, 0, sizeof(double) * (size_t)n, ST(stream));
    SVAE_REQUIRE(e == hipSuccess, SVAE_ERR_LAUNCH, "hdb_core: hipMemsetAsync: %s", hipGetErrorString(e));
    return SVAE_OK;
  }
  hipLaunchKernelGGL(hdb_core_kernel, dim3((unsigned)pair_tile_count(n)), dim3(256), 0, ST(stream), X, ld, d, n, k, core);
  return check_launch("hdb_core");
}

extern "C" int svae_hdb_boruvka(const double* X, int ld, int d, int n, const double* core, const int* id, const int* comp, double alpha,
                                int n_comp, double* bw, unsigned long long* bp, unsigned long long* cw, unsigned long long* cp,
                                void* stream) {
  if (int e = check_pair_rows("hdb_boruvka", X, ld, d, n, 1)) return e;
  SVAE_REQUIRE(core && id && comp && bw && bp && cw && cp && n_comp >= 2 && n_comp <= n && alpha > 0.0, SVAE_ERR_ARG,
               "hdb_boruvka: bad args (n=%d n_comp=%d alpha=%g)", n, n_comp, alpha);
  const unsigned rb = grid(n, 256);
  hipLaunchKernelGGL(hdb_comp_init_kernel, dim3(grid(n_comp, 256)), dim3(256), 0, ST(stream), cw, cp, n_comp);
  if (int e = check_launch("hdb_comp_init")) return e;
  hipLaunchKernelGGL(hdb_boruvka_kernel, dim3((unsigned)pair_tile_count(n)), dim3(256), 0, ST(stream), X, ld, d, n, core, id, comp, alpha,
                     bw, bp);
  if (int e = check_launch("hdb_boruvka")) return e;
  hipLaunchKernelGGL(hdb_comp_weight_kernel, dim3(rb), dim3(256), 0, ST(stream), bw, comp, n, cw);
  if (int e = check_launch("hdb_comp_weight")) return e;
  hipLaunchKernelGGL(hdb_comp_pair_kernel, dim3(rb), dim3(256), 0, ST(stream), bw, bp, comp, n, cw, cp);
  return check_launch("hdb_comp_pair");
}

extern "C" int svae_hdb_relabel(int* comp, int n, const int* map, void* stream) {
  SVAE_REQUIRE(comp && map && n >= 1, SVAE_ERR_ARG, "hdb_relabel: bad args (n=%d)", n);
  hipLaunchKernelGGL(hdb_relabel_kernel, dim3(grid(n, 256)), dim3(256), 0, ST(stream), comp, n, map);
  return check_launch("hdb_relabel");
}

// host: one Boruvka merge.  cw / cp [n_comp] from svae_hdb_boruvka; comp [n] (caller's row order) in/out; map [n_comp] out; the new
// edges are appended to lo / hi / w at *n_edges.
extern "C" int svae_hdb_merge(int n, int n_comp, const unsigned long long* cw, const unsigned long long* cp, int* comp, int* map,
                              int* lo, int* hi, double* w, int* n_edges, int* n_comp_out) {
  SVAE_REQUIRE(cw && cp && comp && map && lo && hi && w && n_edges && n_comp_out && n >= 2 && n_comp >= 2 && n_comp <= n &&
                   *n_edges >= 0 && *n_edges <= n - 1, SVAE_ERR_ARG, "hdb_merge: bad args (n=%d n_comp=%d)", n, n_comp);
  std::vector<int> order(n_comp);
  std::iota(order.begin(), order.end(), 0);
  for (int c = 0; c < n_comp; ++c)
    SVAE_REQUIRE(cp[c] != ~0ull, SVAE_ERR_SHAPE, "hdb_merge: component %d found no outgoing edge", c);
  std::sort(order.begin(), order.end(), [&](int a, int b) { return cw[a] != cw[b] ? cw[a] < cw[b] : cp[a] < cp[b]; });
  Dsu u(n_comp);
  int ne = *n_edges;
  for (int t = 0; t < n_comp; ++t) {
    const int c = order[t];
    if (t > 0 && cw[c] == cw[order[t - 1]] && cp[c] == cp[order[t - 1]]) continue;  // the same edge, chosen from both sides
    const int a = (int)(cp[c] >> 32), b = (int)(cp[c] & 0xffffffffull);
    SVAE_REQUIRE(a >= 0 && a < n && b >= 0 && b < n, SVAE_ERR_SHAPE, "hdb_merge: bad edge (%d, %d)", a, b);
    const long long ra = u.find(comp[a]), rb = u.find(comp[b]);
    SVAE_REQUIRE(ra != rb && ne < n - 1, SVAE_ERR_SHAPE, "hdb_merge: edge (%d, %d) closes a cycle", a, b);
    u.p[std::max(ra, rb)] = std::min(ra, rb);
    lo[ne] = a;
    hi[ne] = b;
    double wv;
    std::memcpy(&wv, &cw[c], sizeof wv);
    w[ne] = wv;
    ++ne;
  }
  int next = 0;
  std::vector<int> root_id(n_comp, -1);
  for (int c = 0; c < n_comp; ++c) {
    const long long r = u.find(c);
    if (root_id[r] < 0) root_id[r] = next++;
    map[c] = root_id[r];
  }
  for (int i = 0; i < n; ++i) comp[i] = map[comp[i]];
  *n_edges = ne;
  *n_comp_out = next;
  return SVAE_OK;
}

extern "C" int svae_hdb_tree(int n, const int* lo, const int* hi, const double* w, int min_cluster_size, int leaf, int allow_single,
                             double epsilon, long long max_cluster_size, long long* sl_left, long long* sl_right, double* sl_value,
                             long long* sl_size, long long* labels, double* prob) {
  SVAE_REQUIRE(n >= 2 && lo && hi && w && sl_left && sl_right && sl_value && sl_size && labels && prob && min_cluster_size >= 2 &&
                   epsilon >= 0.0, SVAE_ERR_ARG, "hdb_tree: bad args (n=%d min_cluster_size=%d)", n, min_cluster_size);
  const long long N = n, m = N - 1, root = 2 * N - 2;
  // single linkage: edges in key order, the smaller endpoint's root on the left, internal node N + edge index
  std::vector<long long> eo(m);
  std::iota(eo.begin(), eo.end(), 0ll);
  std::sort(eo.begin(), eo.end(), [&](long long a, long long b) {
    if (w[a] != w[b]) return w[a] < w[b];
    if (lo[a] != lo[b]) return lo[a] < lo[b];
    return hi[a] < hi[b];
  });
  {
    Dsu u(2 * N - 1);
    for (long long e = 0; e < m; ++e) {
      const long long k = eo[e];
      SVAE_REQUIRE(lo[k] >= 0 && lo[k] < hi[k] && hi[k] < n, SVAE_ERR_ARG, "hdb_tree: bad edge (%d, %d)", lo[k], hi[k]);
      const long long L = u.find(lo[k]), R = u.find(hi[k]);
      SVAE_REQUIRE(L != R, SVAE_ERR_ARG, "hdb_tree: the edges are not a spanning tree");
      sl_left[e] = L;
      sl_right[e] = R;
      sl_value[e] = w[k];
      sl_size[e] = (L < N ? 1 : sl_size[L - N]) + (R < N ? 1 : sl_size[R - N]);
      u.p[L] = u.p[R] = N + e;
    }
  }
  auto count = [&](long long x) { return x < N ? 1ll : sl_size[x - N]; };
  // condensed tree: hierarchy nodes in breadth-first order (left before right)
  std::vector<long long> bfs;
  bfs.reserve(2 * N - 1);
  bfs.push_back(root);
  for (size_t t = 0; t < bfs.size(); ++t)
    if (bfs[t] >= N) {
      bfs.push_back(sl_left[bfs[t] - N]);
      bfs.push_back(sl_right[bfs[t] - N]);
    }
  std::vector<long long> relabel(2 * N - 1, 0), queue;
  std::vector<char> ignore(2 * N - 1, 0);
  std::vector<CondRow> rows;
  rows.reserve(2 * N);
  relabel[root] = N;
  long long next_label = N + 1;
  auto fall_out = [&](long long sub, long long parent, double lam) {  // the points under sub leave `parent` at lam, breadth-first
    queue.assign(1, sub);
    for (size_t t = 0; t < queue.size(); ++t) {
      const long long x = queue[t];
      ignore[x] = 1;
      if (x < N) rows.push_back({parent, x, lam, 1});
      else {
        queue.push_back(sl_left[x - N]);
        queue.push_back(sl_right[x - N]);
      }
    }
  };
  for (const long long node : bfs) {
    if (ignore[node] || node < N) continue;
    const long long e = node - N, left = sl_left[e], right = sl_right[e];
    const double dist = sl_value[e];
    const double lam = dist > 0.0 ? 1.0 / dist : INFINITY;
    const long long lc = count(left), rc = count(right), p = relabel[node];
    if (lc >= min_cluster_size && rc >= min_cluster_size) {
      relabel[left] = next_label++;
      rows.push_back({p, relabel[left], lam, lc});
      relabel[right] = next_label++;
      rows.push_back({p, relabel[right], lam, rc});
    } else if (lc < min_cluster_size && rc < min_cluster_size) {
      fall_out(left, p, lam);
      fall_out(right, p, lam);
    } else if (lc < min_cluster_size) {
      relabel[right] = p;
      fall_out(left, p, lam);
    } else {
      relabel[left] = p;
      fall_out(right, p, lam);
    }
  }
  // clusters N .. next_label - 1: births, stabilities in row order, the cluster tree
  const long long nc = next_label - N;
  std::vector<double> birth(nc, 0.0), stab(nc, 0.0), death(nc, 0.0);
  std::vector<long long> cparent(nc, -1), csize(nc, 0);
  std::vector<std::vector<long long>> kids(nc);
  std::vector<long long> point_row(N, -1);
  for (size_t t = 0; t < rows.size(); ++t) {
    const CondRow& q = rows[t];
    if (q.child >= N) {
      birth[q.child - N] = q.lambda;
      cparent[q.child - N] = q.parent;
      csize[q.child - N] = q.size;
      kids[q.parent - N].push_back(q.child);
    } else {
      point_row[q.child] = (long long)t;
    }
  }
  for (const CondRow& q : rows) stab[q.parent - N] += (q.lambda - birth[q.parent - N]) * (double)q.size;
  {  // deaths as sklearn's max_lambdas reads them: the maximum of the last run of consecutive rows of each parent
    long long cur = rows[0].parent;
    double mx = rows[0].lambda;
    for (size_t t = 1; t < rows.size(); ++t) {
      if (rows[t].parent == cur) mx = std::max(mx, rows[t].lambda);
      else {
        death[cur - N] = mx;
        cur = rows[t].parent;
        mx = rows[t].lambda;
      }
    }
    death[cur - N] = mx;
  }
  const long long max_cs = max_cluster_size > 0 ? max_cluster_size : N + 1;
  if (allow_single) {
    long long s = 0;
    for (const long long c : kids[0]) s += csize[c - N];
    csize[0] = s;
  }
  const bool has_tree = !kids[0].empty();
  std::vector<char> sel(nc, 0);
  auto mark_down = [&](long long top, std::vector<char>& flag) {  // flag every cluster strictly below top
    std::vector<long long> st(kids[top - N].begin(), kids[top - N].end());
    while (!st.empty()) {
      const long long c = st.back();
      st.pop_back();
      flag[c - N] = 1;
      for (const long long g : kids[c - N]) st.push_back(g);
    }
  };
  auto epsilon_search = [&](const std::vector<long long>& leaves) {
    std::vector<char> out(nc, 0), processed(nc, 0);
    for (const long long leaf : leaves) {
      if (1.0 / birth[leaf - N] < epsilon) {
        if (processed[leaf - N]) continue;
        long long x = leaf, top = -1;
        for (;;) {
          const long long par = cparent[x - N];
          if (par == N) {
            top = allow_single ? par : x;
            break;
          }
          if (1.0 / birth[par - N] > epsilon) {
            top = par;
            break;
          }
          x = par;
        }
        out[top - N] = 1;
        mark_down(top, processed);
      } else {
        out[leaf - N] = 1;
      }
    }
    return out;
  };
  if (!leaf) {  // excess of mass: children (larger ids) decide before parents
    std::vector<char> keep(nc, 0);
    for (long long c = nc - 1; c >= (allow_single ? 0 : 1); --c) {
      double sub = 0.0;
      for (const long long g : kids[c]) sub += stab[g - N];
      if (sub > stab[c] || csize[c] > max_cs) {
        stab[c] = sub;
      } else {
        keep[c] = 1;
      }
    }
    for (long long c = 0; c < nc; ++c) {  // selected: kept, with no kept ancestor
      if (c == 0 && !allow_single) continue;
      bool blocked = false;
      for (long long a = cparent[c]; a >= N && !blocked; a = cparent[a - N])
        if (a != N || allow_single) blocked = keep[a - N];
      sel[c] = keep[c] && !blocked;
    }
    if (epsilon != 0.0 && has_tree) {
      std::vector<long long> chosen;
      for (long long c = 0; c < nc; ++c)
        if (sel[c]) chosen.push_back(N + c);
      if (chosen.size() == 1 && chosen[0] == N) {
        if (!allow_single) sel[0] = 0;
      } else {
        sel = epsilon_search(chosen);
      }
    }
  } else {
    std::vector<long long> leaves;
    if (has_tree)
      for (long long c = 1; c < nc; ++c)
        if (kids[c].empty()) leaves.push_back(N + c);
    if (!leaves.empty()) sel = epsilon != 0.0 ? epsilon_search(leaves) : std::vector<char>(nc, 0);
    if (!leaves.empty() && epsilon == 0.0)
      for (const long long c : leaves) sel[c - N] = 1;
  }
  if (!allow_single) sel[0] = 0;
  // labels numbered in ascending cluster id; each point goes to the first selected cluster at or above its condensed parent
  std::vector<long long> label_of(nc, -1), top(nc, N);
  long long n_sel = 0;
  for (long long c = 0; c < nc; ++c)
    if (sel[c]) label_of[c] = n_sel++;
  for (long long c = 1; c < nc; ++c) top[c] = sel[c] ? N + c : top[cparent[c] - N];
  double root_max = -INFINITY;
  for (const CondRow& q : rows)
    if (q.parent == N) root_max = std::max(root_max, q.lambda);
  for (long long i = 0; i < N; ++i) {
    const CondRow& q = rows[point_row[i]];
    const long long t = top[q.parent - N];
    long long lab = -1;
    if (t != N) lab = label_of[t - N];
    else if (n_sel == 1 && allow_single) {
      const double threshold = epsilon != 0.0 ? 1.0 / epsilon : root_max;
      if (q.lambda >= threshold) lab = label_of[0];
    }
    labels[i] = lab;
  }
  std::vector<long long> cluster_of_label(n_sel);
  for (long long c = 0; c < nc; ++c)
    if (sel[c]) cluster_of_label[label_of[c]] = c;
  for (long long i = 0; i < N; ++i) {
    prob[i] = 0.0;
    if (labels[i] < 0) continue;
    const double ml = death[cluster_of_label[labels[i]]];
    const double lam = rows[point_row[i]].lambda;
    prob[i] = (ml == 0.0 || std::isinf(lam)) ? 1.0 : std::min(lam, ml) / ml;
  }
  return SVAE_OK;
}

extern "C" int svae_hdb_cut(long long n_nodes, const long long* left, const long long* right, const double* value, double cut,
                            long long min_cluster_size, long long* labels) {
  SVAE_REQUIRE(n_nodes >= 2 && left && right && value && labels, SVAE_ERR_ARG, "hdb_cut: bad args (n=%lld)", n_nodes);
  const long long N = n_nodes, m = N - 1;
  RankUnionFind u(2 * N - 1);
  for (long long e = 0; e < m; ++e)
    if (value[e] < cut) {
      SVAE_REQUIRE(left[e] >= 0 && left[e] < 2 * N - 1 && right[e] >= 0 && right[e] < 2 * N - 1, SVAE_ERR_ARG,
                   "hdb_cut: bad node %lld", e);
      u.unite(left[e], N + e);
      u.unite(right[e], N + e);
    }
  std::vector<long long> size(2 * N - 1, 0), lab(2 * N - 1, -1);
  for (long long i = 0; i < N; ++i) {
    labels[i] = u.find(i);
    size[labels[i]] += 1;
  }
  long long next = 0;
  for (long long r = 0; r < 2 * N - 1; ++r)  // ascending root id, as np.unique orders them
    if (size[r] > 0 && size[r] >= min_cluster_size) lab[r] = next++;
  for (long long i = 0; i < N; ++i) labels[i] = lab[labels[i]];
  return SVAE_OK;
}
