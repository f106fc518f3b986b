"""Dense numpy restatement of the entropic optimal transport of scrubvae_amd/eval/transport.py (csrc/ot.hip), stage by stage, in
fp64 and in np.longdouble, and the gates that test_ot_cpu.py (the restatement against itself, scipy's assignment) and
test_gpu_ot.py (the kernels and the solver against it) hold a value to.  u = 2^-53 throughout the derivations; the column offsets
are called `off` in the code.

The shared inputs.  The fp64 cost c_ij is fixed bit for bit by the contract of csrc/pair_tiles.h (s in feature order, every
operation rounded on its own, then the correctly rounded square root for the Euclidean cost), so the device, the fp64 restatement
and the long-double truth start from the same c: the roundings of s and of the square root count zero here, exactly as the
silhouette's gate takes its truth from the same fp64 distances.  The truth is the np.longdouble evaluation of
    v_ij = off_j - c_ij / eps,    L_i = log sum_j exp(v_ij),    cbar_i = sum_j pi_ij c_ij,    pi_ij = exp(v_ij - L_i)
from the same fp64 c, off and eps.

Single-pass gate, derived from the arithmetic and not measured.  Per pair the fp64 code forms
    inv_eps = fl(1 / eps) (1 rounding),  p = fl(c inv_eps) (1 more): 2 u p;   v = fl(off_j - p): 1 u |v|
so v is off by at most u (2 p + |v|).  A term enters the sum as exp(v - M) under the running maximum M of the moment and is later
multiplied by exp(M_old - M_new) at every rescale and merge above it.  Each of those exponents is one rounded subtraction, u |arg|,
and the arguments are all of one sign and telescope: along the chain of a term they add up to M_i - v_ij, the term's whole drop
below the row's maximum.  So the exponent of term j is off by at most u (2 p + |v| + (M_i - v)) in all, which is that relative
error of the term to first order ("1 u per unit of the exponent", the counterpart of density_checks' 6 u).  Per exponential the
device's exp is taken at 1 ulp <= 2 u (the maximum error the HIP math API documentation lists for the double-precision exp and
log of the device library; numpy's libm is at least as good), and the product with it is 1 u: 3 u for the term's own exp and sum,
and 3 u for each of the `steps` rescales and merges above it.  A thread rescales at most once per column tile, the waves merge in
3 steps and the chunks in at most 7, so steps <= ceil(n / 64) + 11 for any schedule.  All terms are positive, so ANY order of adding
the n of them is within (n - 1) u of their sum; the long-double sum is within n 2^-64 = n u / 2048 of the truth.  The logarithm adds
2 u |log S| (S in [1, n]) and the closing sum M + log S 1 u |L|.  Together
    |L_i - truth_i| <= 1.001 u (sum_j pi_ij A_ij + n + n / 2048 + 3 steps + 2 |log S_i| + |L_i|),   A_ij = 2 p + |v| + (M_i - v) + 3
with 1.001 for the second-order terms.  Terms that underflow lose at most DBL_MIN each against S >= 1: n DBL_MIN is added.
cbar = W / S with W = sum exp(.) c: a term of W carries the same A plus 1 u for its product with c, both sums their (n + 3 steps) u,
the quotient 1 u:
    |cbar_i - truth_i| <= 1.001 u (sum_j pi_ij c_ij (A_ij + 1) + cbar_i sum_j pi_ij A_ij + cbar_i (2 (n + n / 2048 + 3 steps) + 1))
apply: out_ic = sum_j w_ij V_jc, w_ij = exp(v_ij - L_i) from a given fp64 L.  One exponential per weight (u |v - L| for its argument,
2 u for exp), one rounding in the matrix core's multiply-add; the terms have mixed signs, so the order of the n additions (tiles,
chunks, at most 8 more) costs (n + 8) u of sum_j w |V|:
    |out_ic - truth_ic| <= 1.001 u (sum_j w_ij |V_jc| (2 p + |v| + |v - L_i| + 3) + (n + n / 2048 + 8) sum_j w_ij |V_jc|)

Whole-solve gate.  Softmin is non-expansive in the sup norm (|L(off) - L(off')| <= max_j |off_j - off'_j|), and so is its average
with the identity.  One pass maps a potential g to f = -(eps_t L(off)), off = g inv_eps + log b: forming off costs
u (2 |g_j| / eps_t + |off_j|), the pass its single-pass gate, the closing product 1 u |f|, so in units of the potential
    G_pass = eps_t (max_i gate_L_i + u max_j (2 |g_j| / eps_t + |off_j|)) + u max_i |f_i|     (+ u max |f| for the self update's mean)
and the device's potentials after t passes of a fixed schedule are within the sum of the t pass gates of the long-double run of
the same schedule.  That sum, accumulated by the long-double run itself, is the gate; no number is fixed in advance.  A value
sum a f + sum b g is then within (sum a + sum b) x that gate plus the (n + 4) u of its own summation."""
import functools
from collections import namedtuple

import numpy as np

EPS = 2.0 ** -53
DBL_MIN = np.finfo(np.float64).tiny
LD = np.longdouble
LONGDOUBLE = np.finfo(np.longdouble).nmant >= 63   # otherwise there is no truth to hold a value to

#         m,   n,  d     the smallest sizes that reach each path of csrc/ot.hip
SIZES = [(1, 1, 1),        # the minimum
         (3, 2, 2),        # smallest general
         (64, 65, 3),      # a last tile with one candidate: three waves see nothing
         (130, 65, 17),    # partial row tile, partial feature chunk
         (65, 700, 4),     # several column chunks and their merge
         (200, 300, 70)]   # rows not resident in LDS
APPLY_SIZES = [(130, 65, 17), (65, 700, 4)]
APPLY_COLS = [1, 16, 17, 64, 128]
SOLVE_SIZES = [(150, 130, 3), (70, 200, 20)]

Softmin = namedtuple("Softmin", ["L", "cbar", "v", "M", "S"])
Gate = namedtuple("Gate", ["truth", "tol_L", "tol_cbar"])
Solve = namedtuple("Solve", ["f", "g", "n_iter", "converged", "err", "gate", "eps_t"])
Closing = namedtuple("Closing", ["value", "transport_cost", "marginal_error", "r", "cbar", "L"])


# ---- cost, v, softmin, apply ------------------------------------------------------------------------------------------------------
def cost(A, B, kind):
    """c [len(A), len(B)] fp64 in the contract's arithmetic: s = ((a0 - b0)^2 + (a1 - b1)^2) + ... in feature order, every operation
    rounded on its own (numpy never fuses); kind 1: the correctly rounded sqrt"""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    s = np.zeros((len(A), len(B)))
    for j in range(A.shape[1]):
        e = A[:, j, None] - B[None, :, j]
        s = s + e * e
    return np.sqrt(s) if kind else s


def values(C, off, eps, dtype=np.float64):
    """v_ij = off_j - c_ij inv_eps with inv_eps = 1.0 / eps in fp64; in long double off_j - c_ij / eps"""
    if dtype is np.float64:
        inv = 1.0 / eps
        return np.asarray(off, np.float64)[None, :] - C * inv
    return np.asarray(off).astype(LD)[None, :] - C.astype(LD) / LD(eps)


def softmin(C, off, eps, dtype=np.float64):
    v = values(C, off, eps, dtype)
    M = v.max(axis=1)
    E = np.exp(v - M[:, None])
    S = E.sum(axis=1)
    return Softmin(M + np.log(S), (E * C.astype(dtype)).sum(axis=1) / S, v, M, S)


def steps(n):
    return -(-n // 64) + 11


def gate(C, off, eps):
    """the long-double truth of one pass and the derived tolerances of L and cbar (module docstring), fp64"""
    t = softmin(C, off, eps, LD)
    n = C.shape[1]
    p = C.astype(LD) / LD(eps)
    pi = np.exp(t.v - t.L[:, None])
    A = 2 * p + np.abs(t.v) + (t.M[:, None] - t.v) + 3
    order = n + n / 2048.0 + 3 * steps(n)
    piA = (pi * A).sum(axis=1)
    tol_L = LD(1.001 * EPS) * (piA + order + 2 * np.abs(np.log(t.S)) + np.abs(t.L)) + n * DBL_MIN
    tol_c = LD(1.001 * EPS) * ((pi * C * (A + 1)).sum(axis=1) + t.cbar * piA + t.cbar * (2 * order + 1)) + n * DBL_MIN
    return Gate(t, tol_L.astype(np.float64), tol_c.astype(np.float64))


def apply(C, off, eps, L, V, dtype=np.float64):
    """out = exp(v - L_i) V, from a given L"""
    w = np.exp(values(C, off, eps, dtype) - np.asarray(L).astype(dtype)[:, None])
    V = np.asarray(V).astype(dtype)
    if dtype is np.float64:
        return w @ V
    return np.stack([(w * V[None, :, c]).sum(axis=1) for c in range(V.shape[1])], axis=1)   # no long-double BLAS: sums per column


def apply_gate(C, off, eps, L, V):
    """(truth [m, c] long double, tolerance [m, c] fp64) of apply from the same fp64 L"""
    v = values(C, off, eps, LD)
    n = C.shape[1]
    d = v - np.asarray(L).astype(LD)[:, None]
    w = np.exp(d)
    B = w * (2 * C.astype(LD) / LD(eps) + np.abs(v) + np.abs(d) + 3)
    absV = np.abs(np.asarray(V)).astype(LD)
    V = np.asarray(V).astype(LD)
    truth = np.stack([(w * V[None, :, c]).sum(axis=1) for c in range(V.shape[1])], axis=1)
    tol = np.stack([(B * absV[None, :, c]).sum(axis=1) + (n + n / 2048.0 + 8) * (w * absV[None, :, c]).sum(axis=1)
                    for c in range(V.shape[1])], axis=1)
    return truth, (LD(1.001 * EPS) * tol + n * DBL_MIN).astype(np.float64)


def err(got, truth):
    return np.abs((np.asarray(got).astype(LD) - truth).astype(np.float64))


# ---- the sweep loop ---------------------------------------------------------------------------------------------------------------
def box_scale(X, Y, kind):
    """the squared length of the bounding-box diagonal of X and Y together (kind 0) or the length itself (kind 1)"""
    lo = np.minimum(X.min(axis=0), Y.min(axis=0))
    hi = np.maximum(X.max(axis=0), Y.max(axis=0))
    s = float(((hi - lo) ** 2).sum())
    return float(np.sqrt(s)) if kind else s


def eps_at(t, epsilon, D, scaling):
    return epsilon if scaling is None else max(epsilon, D * scaling ** t)


def median_epsilon(X, Y, kind, factor=0.05):
    """factor x np.median of the cost over the pairs i < j of the stacked rows (the median distance, squared for kind 0)"""
    Z = np.vstack([X, Y])
    d = np.sqrt(cost(Z, Z, 0))[np.triu_indices(len(Z), 1)]
    med = float(np.median(d))
    return factor * (med if kind else med * med)


def _uniform(w, n):
    return np.full(n, 1.0 / n) if w is None else np.asarray(w, np.float64)


def _pass(C, pot, logw, eps_t, dtype, want_gate):
    """one softmin pass: the potential of the rows of C from the potential `pot` and log weights of its columns, and the pass
    gate G_pass of the module docstring (long double only)"""
    if dtype is np.float64:
        inv = 1.0 / eps_t
        off = pot * inv + logw
        return -(eps_t * softmin(C, off, eps_t).L), 0.0
    off = pot / LD(eps_t) + logw.astype(LD)
    if not want_gate:
        return -(LD(eps_t) * softmin(C, off, eps_t, LD).L), 0.0
    g = gate(C, off.astype(np.float64), eps_t)   # the gate at the fp64 image of the offsets: the same to first order
    new = -(LD(eps_t) * softmin(C, off, eps_t, LD).L)
    form = EPS * float(np.max(2 * np.abs(pot) / LD(eps_t) + np.abs(off)))
    return new, float(eps_t * (g.tol_L.max() + form) + EPS * float(np.abs(new).max()))


def solve(X, Y, epsilon, kind=0, a=None, b=None, scaling=0.5, tol=1e-6, max_iter=1000, check_every=10, dtype=np.float64,
          want_gate=False):
    """the alternating sweeps of sinkhorn(): f from g over the rows of X, then g from the new f over the rows of Y, eps_t annealed,
    the error sum a |exp((f - f_new) / eps) - 1| read at every check_every-th sweep run at eps_t == epsilon; tol = 0 never stops early"""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    a, b = _uniform(a, len(X)), _uniform(b, len(Y))
    loga, logb = np.log(a), np.log(b)
    C = cost(X, Y, kind)
    CT = np.ascontiguousarray(C.T)
    D = box_scale(X, Y, kind)
    f, g = np.zeros(len(X), dtype), np.zeros(len(Y), dtype)
    acc, k, n_iter, converged, e, eps_list = 0.0, 0, 0, False, float("nan"), []
    for t in range(max_iter):
        eps_t = eps_at(t, epsilon, D, scaling)
        eps_list.append(eps_t)
        f_new, G = _pass(C, g, logb, eps_t, dtype, want_gate)
        acc += G
        check = False
        if eps_t == epsilon:
            k += 1
            check = k % check_every == 0
        if check:
            ratio = (f - f_new) * (1.0 / eps_t) if dtype is np.float64 else (f - f_new) / LD(eps_t)
            e = float((a * np.abs(np.exp(ratio) - 1)).sum())
        f = f_new
        g, G = _pass(CT, f, loga, eps_t, dtype, want_gate)
        acc += G
        n_iter = t + 1
        if check and tol > 0 and e <= tol:
            converged = True
            break
    return Solve(f, g, n_iter, converged, e, acc, eps_list)


def solve_self(X, epsilon, kind=0, a=None, scaling=0.5, tol=1e-6, max_iter=1000, check_every=10, dtype=np.float64, want_gate=False,
               box=None):
    """the symmetric problem of a set against itself: f <- (f + softmin(f)) / 2 on one potential, stopped at
    max |f_new - f| <= tol eps on the same check schedule; the value is 2 sum a f.  box: the annealing scale D (the divergence
    anneals its three problems from the box of X and Y together)"""
    X = np.asarray(X, np.float64)
    a = _uniform(a, len(X))
    loga = np.log(a)
    C = cost(X, X, kind)
    D = box_scale(X, X, kind) if box is None else box
    f = np.zeros(len(X), dtype)
    acc, k, n_iter, converged, delta, eps_list = 0.0, 0, 0, False, float("nan"), []
    for t in range(max_iter):
        eps_t = eps_at(t, epsilon, D, scaling)
        eps_list.append(eps_t)
        fs, G = _pass(C, f, loga, eps_t, dtype, want_gate)
        f_new = (f + fs) * dtype(0.5)
        acc += G + (EPS * float(np.abs(f_new).max()) if want_gate else 0.0)
        check = False
        if eps_t == epsilon:
            k += 1
            check = k % check_every == 0
        if check:
            delta = float(np.abs(f_new - f).max())
        f = f_new
        n_iter = t + 1
        if check and tol > 0 and delta <= tol * epsilon:
            converged = True
            break
    return Solve(f, f, n_iter, converged, delta, acc, eps_list)


def closing(X, Y, f, g, epsilon, kind=0, a=None, b=None, dtype=np.float64):
    """the pass after the loop: the row marginals r_i = a_i exp((f_i - f~_i) / eps) of the plan (f, g), the mean cost cbar of every
    row's plan, and from them the reported numbers"""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    a, b = _uniform(a, len(X)), _uniform(b, len(Y))
    C = cost(X, Y, kind)
    if dtype is np.float64:
        inv = 1.0 / epsilon
        sm = softmin(C, g * inv + np.log(b), epsilon)
        ratio = np.exp((f - -(epsilon * sm.L)) * inv)
    else:
        sm = softmin(C, g / LD(epsilon) + np.log(b).astype(LD), epsilon, LD)
        ratio = np.exp((f + LD(epsilon) * sm.L) / LD(epsilon))
    r = a * ratio
    return Closing(float((a * f).sum() + (b * g).sum()), float((r * sm.cbar).sum()), float((a * np.abs(ratio - 1)).sum()), r,
                   sm.cbar, sm.L)


def plan_rows(X, Y, g, epsilon, kind=0, b=None, dtype=np.float64):
    """(C, off, L): what apply needs for the row-normalised plan of the rows of X"""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    C = cost(X, Y, kind)
    logb = np.log(_uniform(b, len(Y)))
    off = g * (1.0 / epsilon) + logb if dtype is np.float64 else g / LD(epsilon) + logb.astype(LD)
    return C, off, softmin(C, off, epsilon, dtype).L


def flow(X, Y, g, epsilon, labels_y, kind=0, b=None):
    """(ids, share [nx, K]): the share of each X row's mass that lands in each label of Y, fp64"""
    ids, inv = np.unique(np.asarray(labels_y), return_inverse=True)
    C, off, L = plan_rows(X, Y, g, epsilon, kind, b)
    return ids, apply(C, off, epsilon, L, np.eye(len(ids))[inv.reshape(-1)])


def transport_flow(r, share, labels_x):
    """(ids_x, mass [Kx, Ky]): share weighted by the row marginals r and summed per label of X"""
    ids, inv = np.unique(np.asarray(labels_x), return_inverse=True)
    inv = inv.reshape(-1)
    return ids, np.stack([(r[inv == k, None] * share[inv == k]).sum(axis=0) for k in range(len(ids))])


def divergence(X, Y, epsilon, kind=0, **kw):
    """(value, ot_xy, ot_xx, ot_yy) of sinkhorn_divergence in fp64"""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    box = box_scale(X, Y, kind)
    s = solve(X, Y, epsilon, kind, **kw)
    xy = closing(X, Y, s.f, s.g, epsilon, kind).value
    sx, sy = solve_self(X, epsilon, kind, box=box, **kw), solve_self(Y, epsilon, kind, box=box, **kw)
    xx, yy = 2 * float(sx.f.mean()), 2 * float(sy.f.mean())
    return xy - xx / 2 - yy / 2, xy, xx, yy


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def rows(m, n, d, seed):
    """(Q [m, d], X [n, d]) standard normal, X shifted by 0.5, float32-representable"""
    g = np.random.default_rng(seed)
    q = g.normal(size=(m, d)).astype(np.float32).astype(np.float64)
    x = (g.normal(size=(n, d)) + 0.5).astype(np.float32).astype(np.float64)
    return q, x


def blobs(nx, ny, d, seed, shift=1.5):
    """two standard normal blobs `shift` apart along the first axis, float32-representable"""
    g = np.random.default_rng(seed)
    x = g.normal(size=(nx, d))
    y = g.normal(size=(ny, d))
    y[:, 0] += shift
    return x.astype(np.float32).astype(np.float64), y.astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def case(m, n, d, kind):
    """one of SIZES: (Q, X, off, eps, C, gate or None without a long double), computed once, read-only.  eps = 0.05 x the median
    cost (at least 0.01); off = a potential spread over +-50 eps times inv_eps, so that the running maximum changes often"""
    q, x = rows(m, n, d, 1000 * m + n + d)
    C = cost(q, x, kind)
    eps = max(0.05 * float(np.median(C)), 0.01)
    pot = np.random.default_rng(n + d).uniform(-50 * eps, 50 * eps, n)
    off = pot * (1.0 / eps)
    g = gate(C, off, eps) if LONGDOUBLE else None
    for v in (q, x, off, C):
        v.setflags(write=False)
    return q, x, off, eps, C, g


@functools.lru_cache(maxsize=None)
def solve_case(nx, ny, d, kind):
    """one of SOLVE_SIZES with its fixed schedule (tol = 0, 40 sweeps, annealing on): (X, Y, eps, the fp64 and long-double runs of
    the cross problem and of the two self problems; the long-double ones carry the accumulated gate)"""
    X, Y = blobs(nx, ny, d, nx + ny + d)
    eps = median_epsilon(X, Y, kind)
    box = box_scale(X, Y, kind)
    kw = dict(scaling=0.5, tol=0.0, max_iter=40, check_every=10)
    runs = {"xy": (solve(X, Y, eps, kind, **kw), solve(X, Y, eps, kind, dtype=LD, want_gate=True, **kw) if LONGDOUBLE else None),
            "xx": (solve_self(X, eps, kind, box=box, **kw),
                   solve_self(X, eps, kind, dtype=LD, want_gate=True, box=box, **kw) if LONGDOUBLE else None),
            "yy": (solve_self(Y, eps, kind, box=box, **kw),
                   solve_self(Y, eps, kind, dtype=LD, want_gate=True, box=box, **kw) if LONGDOUBLE else None)}
    X.setflags(write=False)
    Y.setflags(write=False)
    return X, Y, eps, runs


def value_gate(pot_gate, weights_and_pots, n):
    """the gate of a value sum_k sum w_k pot_k from the gate of its potentials"""
    return sum(float(np.sum(w)) for w, _ in weights_and_pots) * pot_gate + \
        (n + 4) * EPS * sum(float(np.sum(np.abs(w * np.asarray(p, np.float64)))) for w, p in weights_and_pots)
