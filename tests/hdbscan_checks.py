"""numpy fp64 restatement of HDBSCAN's arithmetic contract (scrubvae_amd/eval/hdbscan.py, csrc/hdbscan.hip), independent of the
product: sequential-feature squared distances without FMA, np.partition core distances, a dense Prim's algorithm under the strict
edge key (w, min(i, j), max(i, j)), and sklearn 1.7's tree steps (single linkage, condensed tree, stabilities, EOM / leaf
selection with epsilon, max_cluster_size and allow_single_cluster, labels, probabilities, labelling at a cut)."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HIERARCHY_dtype = np.dtype([("left_node", np.intp), ("right_node", np.intp), ("value", np.float64), ("cluster_size", np.intp)])


def _threads():
    import os
    return max(1, min(16, len(os.sched_getaffinity(0))))


def sq_dists(Xt, x):
    """s[r, j] = ((x[r, 0] - X[j, 0])^2 + (x[r, 1] - X[j, 1])^2) + ..., Xt = X.T (features major); each op rounded on its own"""
    s = np.zeros((x.shape[0], Xt.shape[1]))
    e = np.empty_like(s)
    for f in range(Xt.shape[0]):
        np.subtract(x[:, f:f + 1], Xt[f][None, :], out=e)
        np.multiply(e, e, out=e)
        np.add(s, e, out=s)
    return s


def core_distances(X, k, rows=None, block=64):
    """sqrt of the k-th smallest squared distance of each row (or of X[rows]) to all rows of X, itself included"""
    X = np.ascontiguousarray(X, np.float64)
    Xt = np.ascontiguousarray(X.T)
    rows = np.arange(len(X)) if rows is None else np.asarray(rows)

    def one(b):
        r = rows[b:b + block]
        s = sq_dists(Xt, X[r])
        return np.sqrt(np.partition(s, k - 1, axis=1)[:, k - 1])

    with ThreadPoolExecutor(_threads()) as ex:
        parts = list(ex.map(one, range(0, len(rows), block)))
    return np.concatenate(parts) if parts else np.zeros(0)


def prim_mst(X, core, alpha=1.0):
    """(lo, hi, w) of the minimum spanning tree of max(core_i, core_j, d_ij / alpha) under the key (w, min(i, j), max(i, j)),
    dense Prim from row 0"""
    X = np.ascontiguousarray(X, np.float64)
    n = len(X)
    Xt = np.ascontiguousarray(X.T)
    out = np.ones(n, bool)
    bw = np.full(n, np.inf)
    blo = np.full(n, n, np.int64)
    bhi = np.full(n, n, np.int64)
    lo, hi, w = np.empty(n - 1, np.int64), np.empty(n - 1, np.int64), np.empty(n - 1)
    u = 0
    for t in range(n - 1):
        out[u] = False
        rest = np.nonzero(out)[0]
        s = sq_dists(Xt[:, rest], X[u:u + 1])[0]
        dist = np.sqrt(s) / alpha
        wv = np.maximum(np.maximum(core[u], core[rest]), dist)
        a = np.minimum(u, rest)
        b = np.maximum(u, rest)
        cw, ca, cb = bw[rest], blo[rest], bhi[rest]
        better = (wv < cw) | ((wv == cw) & ((a < ca) | ((a == ca) & (b < cb))))
        upd = rest[better]
        bw[upd], blo[upd], bhi[upd] = wv[better], a[better], b[better]
        cw, ca, cb = bw[rest], blo[rest], bhi[rest]
        m = cw == cw.min()
        cand = np.nonzero(m)[0]
        j = cand[np.lexsort((cb[cand], ca[cand]))[0]]
        v = rest[j]
        lo[t], hi[t], w[t] = ca[j], cb[j], cw[j]
        u = v
    return lo, hi, w


def edge_set(lo, hi, w):
    return set(zip(np.asarray(lo).tolist(), np.asarray(hi).tolist(), np.asarray(w).tolist()))


# ---- tree steps ----------------------------------------------------------------------------------------------------------------
def single_linkage(lo, hi, w):
    """edges in key order; left = root of lo, right = root of hi, internal node n + edge index"""
    n = len(lo) + 1
    order = np.lexsort((hi, lo, w))
    parent = list(range(2 * n - 1))
    size = [1] * n + [0] * (n - 1)

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    tree = np.zeros(n - 1, dtype=HIERARCHY_dtype)
    for e, k in enumerate(order.tolist()):
        L, R = find(int(lo[k])), find(int(hi[k]))
        size[n + e] = size[L] + size[R]
        parent[L] = parent[R] = n + e
        tree[e] = (L, R, w[k], size[n + e])
    return tree


def _bfs(tree, root, n):
    out, q = [], [root]
    while q:
        out.extend(q)
        nq = []
        for x in q:
            if x >= n:
                nq.extend([int(tree["left_node"][x - n]), int(tree["right_node"][x - n])])
        q = nq
    return out


def condense(tree, mcs):
    n = len(tree) + 1
    root = 2 * n - 2
    left, right, val, csz = (tree[f].tolist() for f in ("left_node", "right_node", "value", "cluster_size"))
    cnt = lambda x: 1 if x < n else csz[x - n]  # noqa: E731
    relabel = {root: n}
    nxt = n + 1
    ignore = set()
    rows = []
    for node in _bfs(tree, root, n):
        if node < n or node in ignore:
            continue
        l, r, dist = left[node - n], right[node - n], val[node - n]
        lam = 1.0 / dist if dist > 0.0 else np.inf
        lc, rc, p = cnt(l), cnt(r), relabel[node]

        def drop(sub):
            for x in _bfs(tree, sub, n):
                if x < n:
                    rows.append((p, x, lam, 1))
                ignore.add(x)

        if lc >= mcs and rc >= mcs:
            relabel[l] = nxt
            rows.append((p, nxt, lam, lc))
            relabel[r] = nxt + 1
            rows.append((p, nxt + 1, lam, rc))
            nxt += 2
        elif lc < mcs and rc < mcs:
            drop(l)
            drop(r)
        elif lc < mcs:
            relabel[r] = p
            drop(l)
        else:
            relabel[l] = p
            drop(r)
    return rows


def select(rows, n, method="eom", allow_single=False, eps=0.0, max_size=None):
    """(labels, probabilities) from the condensed rows"""
    root = n
    clusters = sorted({r[0] for r in rows} | {r[1] for r in rows if r[1] >= n})
    birth = {root: 0.0}
    par, size, kids = {}, {}, {c: [] for c in clusters}
    prow = {}
    for t, (p, c, lam, s) in enumerate(rows):
        if c >= n:
            birth[c], par[c], size[c] = lam, p, s
            kids[p].append(c)
        else:
            prow[c] = t
    stab = {c: 0.0 for c in clusters}
    for p, c, lam, s in rows:
        stab[p] += (lam - birth[p]) * s
    if allow_single:
        size[root] = sum(size[c] for c in kids[root])
    max_size = n + 1 if max_size is None else max_size
    nodes = sorted(clusters, reverse=True)
    if not allow_single:
        nodes = nodes[:-1]
    has_tree = len(kids[root]) > 0

    def below(c):
        out, st = [], list(kids[c])
        while st:
            x = st.pop()
            out.append(x)
            st.extend(kids[x])
        return out

    def eps_search(leaves):
        chosen, done = set(), set()
        for leaf in sorted(leaves):
            if 1.0 / birth[leaf] < eps:
                if leaf in done:
                    continue
                x = leaf
                while True:
                    p = par[x]
                    if p == root:
                        top = p if allow_single else x
                        break
                    if 1.0 / birth[p] > eps:
                        top = p
                        break
                    x = p
                chosen.add(top)
                done.update(below(top))
            else:
                chosen.add(leaf)
        return chosen

    is_cl = {c: True for c in nodes}
    if method == "eom":
        for c in nodes:
            sub = 0.0
            for g in kids[c]:
                sub += stab[g]
            if sub > stab[c] or size[c] > max_size:
                is_cl[c] = False
                stab[c] = sub
            else:
                for g in below(c):
                    is_cl[g] = False
        if eps != 0.0 and has_tree:
            eom = [c for c in is_cl if is_cl[c]]
            if len(eom) == 1 and eom[0] == root:
                sel = set(eom) if allow_single else set()
            else:
                sel = eps_search(eom)
            is_cl = {c: c in sel for c in is_cl}
    else:
        leaves = [c for c in clusters if c != root and not kids[c]] if has_tree else []
        sel = eps_search(leaves) if eps != 0.0 else set(leaves)
        is_cl = {c: c in sel for c in is_cl}
    chosen = sorted(c for c in is_cl if is_cl[c])
    cmap = {c: i for i, c in enumerate(chosen)}
    top = {root: root}
    for c in clusters:
        if c != root:
            top[c] = c if c in cmap else top[par[c]]
    root_max = max(lam for p, c, lam, s in rows if p == root)
    labels = np.full(n, -1, np.intp)
    for i in range(n):
        p, _, lam, _ = rows[prow[i]]
        t = top[p]
        if t != root:
            labels[i] = cmap[t]
        elif len(chosen) == 1 and allow_single:
            thr = 1.0 / eps if eps != 0.0 else root_max
            if lam >= thr and root in cmap:
                labels[i] = cmap[root]
    death, cur, mx = {}, rows[0][0], rows[0][2]
    for p, c, lam, s in rows[1:]:
        if p == cur:
            mx = max(mx, lam)
        else:
            death[cur], cur, mx = mx, p, lam
    death[cur] = mx
    prob = np.zeros(n)
    for i in range(n):
        if labels[i] < 0:
            continue
        ml = death[chosen[labels[i]]]
        lam = rows[prow[i]][2]
        prob[i] = 1.0 if (ml == 0.0 or np.isinf(lam)) else min(lam, ml) / ml
    return labels, prob


def cut_labels(tree, cut, mcs):
    """labelling at a cut with sklearn's union by rank (ties: the first argument's root), clusters numbered by ascending root"""
    n = len(tree) + 1
    parent = list(range(2 * n - 1))
    rank = [0] * (2 * n - 1)

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    def union(x, y):
        a, b = find(x), find(y)
        if rank[a] < rank[b]:
            parent[a] = b
        elif rank[a] > rank[b]:
            parent[b] = a
        else:
            parent[b] = a
            rank[a] += 1

    for e in range(n - 1):
        if tree["value"][e] < cut:
            union(int(tree["left_node"][e]), n + e)
            union(int(tree["right_node"][e]), n + e)
    roots = np.array([find(i) for i in range(n)])
    u, counts = np.unique(roots, return_counts=True)
    lab, nxt = {}, 0
    for r, c in zip(u.tolist(), counts.tolist()):
        if c >= mcs:
            lab[r] = nxt
            nxt += 1
    return np.array([lab.get(r, -1) for r in roots.tolist()], np.intp)


def fit(X, min_cluster_size=5, min_samples=None, alpha=1.0, method="eom", allow_single=False, eps=0.0, max_size=None):
    """the whole contract on finite rows: dict(core, lo, hi, w, tree, labels, probabilities)"""
    X = np.asarray(X, np.float64)
    k = min_cluster_size if min_samples is None else min_samples
    core = core_distances(X, k)
    lo, hi, w = prim_mst(X, core, alpha)
    tree = single_linkage(lo, hi, w)
    labels, prob = select(condense(tree, min_cluster_size), len(X), method, allow_single, eps, max_size)
    return dict(core=core, lo=lo, hi=hi, w=w, tree=tree, labels=labels, probabilities=prob)


def planted(n, d, n_blobs, seed, noise=0.05, spread=6.0):
    """float32 rows: n_blobs gaussian blobs and a share of uniform noise; returns (x, truth) with truth -1 on the noise"""
    g = np.random.default_rng(seed)
    centers = g.uniform(-spread, spread, size=(n_blobs, d))
    n_noise = int(noise * n)
    truth = np.concatenate([g.integers(0, n_blobs, n - n_noise), np.full(n_noise, -1)])
    x = centers[np.maximum(truth, 0)] + g.normal(size=(n, d)) * 0.5
    x[truth < 0] = g.uniform(-spread - 2, spread + 2, size=(n_noise, d))
    p = g.permutation(n)
    return x[p].astype(np.float32), truth[p]


def same_partition(a, b):
    """labels equal up to a renumbering of the clusters, with -1 (and -2, -3) fixed"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or not np.array_equal(a < 0, b < 0) or not np.array_equal(a[a < 0], b[b < 0]):
        return False
    pos = a >= 0
    pairs = set(zip(a[pos].tolist(), b[pos].tolist()))
    return len(pairs) == len({p[0] for p in pairs}) == len({p[1] for p in pairs})
