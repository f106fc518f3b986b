"""Restatements and gates for the Gaussian HMM (scrubvae_amd/eval/hmm.py, csrc/hmm.hip), used by test_hmm_cpu.py and
test_gpu_hmm.py:

  (a) plain()      the plain scaled forward-backward recursion, frame by frame, and viterbi(), in numpy fp64
  (b) segmented()  the time-parallel pass in the structure of the kernels: transfer matrices of segments with power-of-two row
                   scales, the carry over the segments of a sequence relative to the largest exponent, the plain recursion inside
                   every segment from its boundary vector, the transition counts as A o sum_t alpha_{t-1} q_t^T.  Dot products are
                   numpy's (the matrix cores add in an order of their own; the gates hold for any order).
  (c) plain(..., dtype=np.longdouble)  the same plain recursion in 80-bit long double (unit roundoff 2^-64): the reference
  (d) gates()      how far (b) and the device may be from (c)

The gates.  u = 2^-53.  Every number in the pass is a sum of products of non-negative numbers: nothing cancels, so first-order
relative errors of the inputs of an operation pass through at their maximum and every rounding adds at most u.  A common factor of
a vector is removed by the next normalisation, so errors are counted up to a common factor ("projectively") until the last
normalisation, which doubles them (largest minus smallest).  With K states padded to KP, segments of L frames and at most S
segments in a sequence, counting the kernels' arithmetic:

  transfer   a step is a KP-term dot product (KP roundings at most, in any order), one product by b_t and a power-of-two scaling
             (exact): KP + 1 per step, so e_T = L (KP + 1) for an entry of a segment's matrix
  carry      per segment: weight by ldexp (exact), one product, a K-term sum and one division: the boundary vectors carry
             e_v = S (e_T + K + 1)
  fill       per frame: a K-term dot product (K), one product by b_t, one division: K + 2, so
             e_alpha = e_beta = e_v + L (K + 2)
  gamma      alpha beta / D: one product, the K-term sum D, one division; the last normalisation doubles the projective part:
             G_gamma = 2 (e_alpha + e_beta + 1) + K + 1
  Xi         a term alpha_{t-1}(i) q_t(j) with q_t = b_t beta_t / (c_t D_t): numerator e_alpha + e_beta + 3 roundings, the
             denominator is the same sum of numerators formed through c_t (K-term dot, product, K-term sum), alpha_t (a division),
             D_t (product, K-term sum) and one product: 3 K + 4 more; the terms are added one by one (at most n - 1 roundings), the
             blocks' partials in order (at most 1024) and the product by A: G_Xi = 2 (e_alpha + e_beta) + 3 K + 8 + n + 1025
  start_post G_gamma + number of sequences
  loglik     absolute: per frame the relative error of c_t, e_alpha + 2 K + 4, is the absolute error of log c_t; the log is
             taken within 2 u |log c_t| and the sum with lpn_t rounds once; the terms are added per segment one by one (L) and the
             segment sums by a compensated sum and a tree of depth 8 (16 at most):
             G_ll = u [n (e_alpha + 2 K + 4) + sum_t (2 |log c_t| + |log c_t + lpn_t|) + (L + 16) sum_t |log c_t + lpn_t|]
  floor      1e-290 absolute on everything: below it a value is close to the subnormal range (a row weight 2^-1022 below the
             largest is flushed by ldexp) and only its smallness is promised.

A fit adds the emissions in front of the pass (emission_bounds()).  A frame's log density w = cst - q / 2, q = |(x - mu) P|^2, is
formed with one subtraction, a d-term dot product per column, a d-term sum of squares, a halving and a subtraction: at most
2 d + 6 roundings on numbers no larger than |w| + |cst|; exp, log and the sum over states of the scaling add a few more: e_E(t) =
(2 d + 10) u max_k (|w_k(t)| + |cst_k|).  The likelihood is a sum of products with one emission factor per frame, so scaling the
factors of frame t by e^(+-e) moves the log-likelihood by at most e: the emissions add sum_t e_E(t) to G_ll, and a computed
log-likelihood is monotone over EM iterations up to the two evaluations' G_ll + sum e_E (an M-step that misses its maximiser by
a rounding costs second order).  Two fits whose parameters differ by delta (means by delta x max|x| per coordinate, every entry
of a precision factor by delta x its largest entry: the form of the mixture M-step's tolerance in test_gpu_gmm.py, delta = 1e-9)
differ in a frame's log density by at most delta s_t, s_t = max_k (sum_j |y_j| dy_j + pmax sum_j 1 / P_jj) with y = (x - mu) P and
dy_j = max|x| sum_i |P_ij| + pmax |x - mu|_1 (first order), hence in the log-likelihood by delta sum_t s_t; a relative difference
rho of the chain's entries moves it by at most n rho.

The bounds are worst cases, linear in the frames of a sequence; what (b) and the device actually use of them is recorded in
DESIGN.md.  The reference's own error, of the order of these counts times 2^-64, is 2^-11 of a gate and is ignored.
"""
import itertools

import numpy as np

U = 2.0 ** -53
FLOOR = 1e-290
SEGMENT = {16: 512, 32: 512, 64: 512}  # include/scrubvae_hip.h SVAE_HMM_SEGMENT_*


def padded(K):
    return 16 if K <= 16 else 32 if K <= 32 else 64


def segment_length(K):
    return SEGMENT[padded(K)]


def _bounds(lengths):
    ends = np.cumsum(lengths)
    return list(zip(ends - np.asarray(lengths), ends))


# ---- (a), (c): the plain recursion ----------------------------------------------------------------------------------------------
def plain(B, lpn, startprob, transmat, lengths=None, dtype=np.float64):
    """scaled forward-backward, frame by frame -> dict(alpha, gamma [K, n], c [n], Xi [K, K], start_post [K], loglik, ll_terms)"""
    B = np.asarray(B).astype(dtype)
    K, n = B.shape
    lengths = [n] if lengths is None else lengths
    pi, A = np.asarray(startprob).astype(dtype), np.asarray(transmat).astype(dtype)
    alpha, gamma, c = np.zeros((K, n), dtype), np.zeros((K, n), dtype), np.zeros(n, dtype)
    Xi, sp = np.zeros((K, K), dtype), np.zeros(K, dtype)
    for lo, hi in _bounds(lengths):
        for t in range(lo, hi):
            u = (pi if t == lo else alpha[:, t - 1] @ A) * B[:, t]
            c[t] = u.sum()
            alpha[:, t] = u / c[t]
        beta = np.ones(K, dtype)
        for t in range(hi - 1, lo - 1, -1):
            g = alpha[:, t] * beta
            gamma[:, t] = g / g.sum()
            if t > lo:
                y = B[:, t] * beta
                Xi += alpha[:, t - 1][:, None] * A * y[None, :] / c[t]
                beta = (A @ y) / c[t]
        sp += gamma[:, lo]
    terms = np.log(c) + np.asarray(lpn).astype(dtype)
    return dict(alpha=alpha, gamma=gamma, c=c, Xi=Xi, start_post=sp, loglik=terms.sum(), log_c=np.log(c), ll_terms=terms)


def viterbi(logB, log_startprob, log_transmat, lengths=None):
    """the max-sum recursion with np.argmax's ties (the lower state) -> (states [n], logprob per sequence)"""
    logB = np.asarray(logB, np.float64)
    K, n = logB.shape
    lengths = [n] if lengths is None else lengths
    states, logprob = np.zeros(n, np.int64), []
    for lo, hi in _bounds(lengths):
        delta = log_startprob + logB[:, lo]
        bp = np.zeros((hi - lo, K), np.int64)
        for t in range(lo + 1, hi):
            cand = delta[:, None] + log_transmat
            bp[t - lo] = cand.argmax(0)
            delta = cand.max(0) + logB[:, t]
        st = int(delta.argmax())
        logprob.append(delta[st])
        states[hi - 1] = st
        for t in range(hi - 1, lo, -1):
            st = bp[t - lo, st]
            states[t - 1] = st
    return states, np.array(logprob)


def viterbi_brute(logB, log_startprob, log_transmat):
    """every path of one short sequence -> (best log-probability, the lexicographically first best path)"""
    K, n = logB.shape
    best, arg = -np.inf, None
    for path in itertools.product(range(K), repeat=n):
        s = log_startprob[path[0]] + logB[path[0], 0]
        for t in range(1, n):
            s = s + log_transmat[path[t - 1], path[t]]
            s = s + logB[path[t], t]
        if s > best:
            best, arg = s, path
    return best, np.array(arg)


# ---- (b): the segmented pass ------------------------------------------------------------------------------------------------------
def segment_table(lengths, L):
    """as scrubvae_amd.eval.hmm.segment_table, written out sequence by sequence"""
    seg, seq, t = [], [], 0
    for s, ln in enumerate(lengths):
        first = len(seg)
        for off in range(0, ln, L):
            seg.append([t + off, min(L, ln - off), int(off == 0), s])
        seq.append([first, len(seg) - first, t, ln])
        t += ln
    return np.array(seg, np.int32), np.array(seq, np.int32)


DEAD = np.iinfo(np.int32).min


def _transfer(B, A, t0, ln, first):
    K = len(A)
    R, e, dead = np.eye(K), np.zeros(K, np.int64), np.zeros(K, bool)
    for f in range(ln):
        b = B[:, t0 + f]
        R = R * b[None, :] if first and f == 0 else (R @ A) * b[None, :]
        s = R.sum(1)
        live = s > 0
        ex = np.frexp(s)[1] - 1  # ilogb
        R[live] = np.ldexp(R[live], -ex[live][:, None])
        e[live] += ex[live]
        dead |= ~live
    R[dead] = 0.0
    return R, np.where(dead, DEAD, e)


def _norm(x):
    t = x.sum()
    return x / t if t > 0 else np.zeros_like(x)


def segmented(B, lpn, startprob, transmat, lengths=None, L=None):
    B = np.asarray(B, np.float64)
    K, n = B.shape
    lengths = [n] if lengths is None else lengths
    L = segment_length(K) if L is None else L
    A = np.asarray(transmat, np.float64)
    seg, seq = segment_table(lengths, L)
    trans = [_transfer(B, A, t0, ln, first) for t0, ln, first, _ in seg]
    vstart, wend = np.zeros((len(seg), K)), np.zeros((len(seg), K))
    for g0, cnt, _, _ in seq:
        v = np.asarray(startprob, np.float64)
        for g in range(g0, g0 + cnt):
            vstart[g] = v
            if g == g0 + cnt - 1:
                break
            R, e = trans[g]
            live = (v > 0) & (e != DEAD)
            me = e[live].max() if live.any() else 0
            w = np.where(live, np.ldexp(v, np.where(live, np.maximum(e - me, -4000), 0).astype(np.int64)), 0.0)
            v = _norm(w @ R)
        w = np.full(K, 1.0 / K)
        for g in range(g0 + cnt - 1, g0 - 1, -1):
            wend[g] = w
            if g == g0:
                break
            R, e = trans[g]
            x = R @ w
            live = (x > 0) & (e != DEAD)
            me = e[live].max() if live.any() else 0
            w = _norm(np.where(live, np.ldexp(x, np.where(live, np.maximum(e - me, -4000), 0).astype(np.int64)), 0.0))
    alpha, gamma, c = np.zeros((K, n)), np.zeros((K, n)), np.zeros(n)
    M, llseg = np.zeros((K, K)), []
    for g, (t0, ln, first, _) in enumerate(seg):
        a, ll = vstart[g], 0.0
        for f in range(ln):
            u = (a if first and f == 0 else a @ A) * B[:, t0 + f]
            c[t0 + f] = u.sum()
            a = u / c[t0 + f] if c[t0 + f] > 0 else np.zeros(K)
            alpha[:, t0 + f] = a
            ll = ll + (np.log(c[t0 + f]) + lpn[t0 + f])
        llseg.append(ll)
    for g, (t0, ln, first, _) in enumerate(seg):
        beta = wend[g]
        for f in range(ln - 1, -1, -1):
            t = t0 + f
            x = alpha[:, t] * beta
            D = x.sum()
            gamma[:, t] = x / D if D > 0 else 0.0
            y = B[:, t] * beta
            if not (first and f == 0):
                den = c[t] * D
                q = y / den if den > 0 else np.zeros(K)
                M += (alpha[:, t - 1] if f > 0 else vstart[g])[:, None] * q[None, :]
            if f > 0:
                beta = _norm(A @ y)
    sp = np.zeros(K)
    for _, _, t0, _ in seq:
        sp = sp + gamma[:, t0]
    return dict(alpha=alpha, gamma=gamma, c=c, Xi=A * M, start_post=sp, loglik=float(np.sum(llseg)))


# ---- (d): the gates ---------------------------------------------------------------------------------------------------------------
def gates(K, lengths, L, ref):
    """bounds on |value - reference|: relative ones for gamma, Xi, start_post (in units of the reference's entries, plus FLOOR) and
    the absolute one for loglik; `ref` is (c)'s result (its log c_t and lpn_t size the log-likelihood's)"""
    KP, n = padded(K), int(np.sum(lengths))
    S = max(-(-int(ln) // L) for ln in lengths)
    e_T = L * (KP + 1)
    e_v = S * (e_T + K + 1)
    e_ab = e_v + L * (K + 2)
    g_gamma = 2 * (2 * e_ab + 1) + K + 1
    g_xi = 2 * (2 * e_ab) + 3 * K + 8 + n + 1025
    log_c = np.abs(np.asarray(ref["log_c"], np.float64))
    terms = np.abs(np.asarray(ref["ll_terms"], np.float64))
    g_ll = U * (n * (e_ab + 2 * K + 4) + (2 * log_c + terms).sum() + (L + 16) * terms.sum())
    return dict(gamma=g_gamma * U, Xi=g_xi * U, start_post=(g_gamma + len(lengths)) * U, loglik=g_ll)


def share(got, ref, rel):
    """the largest |got - ref| / (rel |ref| + FLOOR): <= 1 inside the gate"""
    ref64 = np.asarray(ref, np.float64)
    err = np.abs(np.asarray(got).astype(np.longdouble) - np.asarray(ref).astype(np.longdouble)).astype(np.float64)
    return float((err / (rel * np.abs(ref64) + FLOOR)).max())


def check_pass(got, ref, K, lengths, L):
    """-> dict of the share of each gate that `got` uses against the reference `ref` (both dicts as plain() returns)"""
    g = gates(K, lengths, L, ref)
    out = {k: share(got[k], ref[k], g[k]) for k in ("gamma", "Xi", "start_post")}
    out["loglik"] = abs(float(np.longdouble(got["loglik"]) - ref["loglik"])) / g["loglik"]
    return out


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def chain(K, seed, sticky=0.8):
    """a start vector and a transition matrix with a heavy diagonal"""
    g = np.random.default_rng(seed)
    A = g.random((K, K)) + 1e-3
    A = (1 - sticky) * A / A.sum(1, keepdims=True) + sticky * np.eye(K)
    pi = g.random(K) + 0.1
    return pi / pi.sum(), A / A.sum(1, keepdims=True)


def overlapping(n, K, d, seed, sep=2.0):
    """rows from K unit Gaussians whose means lie within about `sep` sigma, drawn along a sticky chain -> (x fp32, means, states)"""
    g = np.random.default_rng(seed)
    means = g.normal(size=(K, d)) * sep / 2.0
    st = np.zeros(n, np.int64)
    st[0] = g.integers(K)
    stay = g.random(n) < 0.9
    jump = g.integers(0, K, n)
    for t in range(1, n):
        st[t] = st[t - 1] if stay[t] else jump[t]
    x = (means[st] + g.normal(size=(n, d))).astype(np.float32)
    return x, means, st


def emissions(x, means):
    """scaled emissions of unit Gaussians at `means`: B [K, n] with columns summing to 1, and lpn [n]"""
    x = np.asarray(x, np.float64)
    d = x.shape[1]
    w = -0.5 * ((x[None, :, :] - means[:, None, :]) ** 2).sum(2) - 0.5 * d * np.log(2 * np.pi)
    m = w.max(0)
    lpn = m + np.log(np.exp(w - m).sum(0))
    return np.exp(w - lpn), lpn


def emission_bounds(x, means, P, diag):
    """(sum_t e_E(t), sum_t s_t) of the module docstring for unit-weight Gaussians (means, precision factors P) on rows x"""
    x = np.asarray(x, np.float64)
    K, d = means.shape
    scale = np.abs(x).max()
    e_max, s_max = np.zeros(len(x)), np.zeros(len(x))
    for k in range(K):
        diff = x - means[k]
        if diag:
            y, colsum, pdiag = diff * P[k], np.abs(P[k]), P[k]
        else:
            y, colsum, pdiag = diff @ P[k], np.abs(P[k]).sum(0), np.diag(P[k])
        pmax = np.abs(P[k]).max()
        cst = np.log(pdiag).sum() - 0.5 * d * np.log(2 * np.pi)
        w = cst - 0.5 * (y ** 2).sum(1)
        dy = scale * colsum[None, :] + pmax * np.abs(diff).sum(1)[:, None]
        e_max = np.maximum(e_max, np.abs(w) + abs(cst))
        s_max = np.maximum(s_max, (np.abs(y) * dy).sum(1) + pmax * (1.0 / pdiag).sum())
    return (2 * d + 10) * U * e_max.sum(), s_max.sum()


# ---- the restated EM iteration and fit ------------------------------------------------------------------------------------------------
def em_iteration(x, lengths, startprob, transmat, means, P, diag, reg, tprior=1.0, sprior=1.0, dtype=np.float64):
    """one Baum-Welch iteration with the mixture's restated E- and M-step (tests/gmm_checks.py) around plain()"""
    from tests import gmm_checks as GC
    x64 = np.asarray(x, np.float64)
    K = len(means)
    lpn, resp = GC.estep(x64, np.ones(K), means, P, diag)
    fb = plain(resp.T, lpn, startprob, transmat, lengths, dtype)
    gamma = np.asarray(fb["gamma"], np.float64)
    _, means, cov, P = GC.mstep(x64, gamma.T.copy(), reg, diag)
    T = np.maximum(np.asarray(fb["Xi"], np.float64) + (tprior - 1.0), 0.0)
    tot = T.sum(1, keepdims=True)
    transmat = np.where(tot > 0, T / np.where(tot > 0, tot, 1.0), transmat)
    s = np.maximum(np.asarray(fb["start_post"], np.float64) + (sprior - 1.0), 0.0)
    startprob = s / s.sum() if s.sum() > 0 else startprob
    return float(fb["loglik"]), startprob, transmat, means, cov, P


def initial_transmat(labels, lengths, K):
    counts = np.ones((K, K))
    for lo, hi in _bounds(lengths):
        for t in range(lo, hi - 1):
            counts[labels[t], labels[t + 1]] += 1.0
    return counts / counts.sum(1, keepdims=True)


def fit(x, lengths, K, diag=False, n_iter=100, tol=1e-3, reg=1e-6, init_iter=10, random_state=None):
    """the restated fit: the restated mixture (gmm_checks.fit, max_iter = init_iter), then Baum-Welch with plain()"""
    from tests import gmm_checks as GC
    x64 = np.asarray(x, np.float64)
    n = len(x64)
    gm = GC.fit(x64, K, diag=diag, reg=reg, max_iter=init_iter, random_state=random_state)
    means, P = gm["means"], gm["precisions_cholesky"]
    startprob, transmat = np.full(K, 1.0 / K), initial_transmat(gm["labels"], lengths, K)
    prev, history, converged, it = -np.inf, [], False, 0
    own, sens, xi_gate = [], [], []
    for it in range(1, n_iter + 1):
        # the gates of this iteration's log-likelihood, at the parameters it is evaluated with
        lpn, resp = GC.estep(x64, np.ones(K), means, P, diag)
        g = gates(K, lengths, segment_length(K), plain(resp.T, lpn, startprob, transmat, lengths))
        e_tol, s_sum = emission_bounds(x64, means, P, diag)
        own.append(g["loglik"] + e_tol)
        sens.append(s_sum)
        xi_gate.append(g["Xi"])
        ll, startprob, transmat, means, cov, P = em_iteration(x64, lengths, startprob, transmat, means, P, diag, reg)
        history.append(ll)
        change = (ll - prev) / n
        prev = ll
        if abs(change) < tol:
            converged = True
            break
    lpn, resp = GC.estep(x64, np.ones(K), means, P, diag)
    with np.errstate(divide="ignore"):
        states, _ = viterbi(np.log(resp.T) + lpn[None, :], np.log(startprob), np.log(transmat), lengths)
    return dict(history=history, n_iter=it, converged=converged, startprob=startprob, transmat=transmat, means=means, states=states,
                initial_labels=gm["labels"], own_gate=np.array(own), sensitivity=np.array(sens), xi_gate=np.array(xi_gate))


def planted_sticky(seed=0, K=4, d=4, lengths=(1500, 1300, 1200), stay=0.97, sep=1.5):
    """rows of a planted sticky HMM with unit-variance states whose means are about `sep` sigma apart -> (x fp32, states)"""
    g = np.random.default_rng(seed)
    means = g.normal(size=(K, d))
    dist = np.sqrt(((means[:, None, :] - means[None, :, :]) ** 2).sum(2))
    means *= sep / dist[np.triu_indices(K, 1)].mean()  # the mean distance between two states' means is sep sigma
    n = int(np.sum(lengths))
    st = np.zeros(n, np.int64)
    t = 0
    for ln in lengths:
        st[t] = g.integers(K)
        for u in range(t + 1, t + ln):
            st[u] = st[u - 1] if g.random() < stay else (st[u - 1] + 1 + g.integers(K - 1)) % K
        t += ln
    return (means[st] + g.normal(size=(n, d))).astype(np.float32), st
