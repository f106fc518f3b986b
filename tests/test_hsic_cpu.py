"""HSIC without a GPU: the restatement of tests/hsic_checks.py pinned to the textbook matrix forms, the p-value cases it decides,
argument errors before any device work and the C-ABI exports."""
import numpy as np
import pytest
import torch

from tests import hsic_checks as HC

needs_longdouble = pytest.mark.skipif(np.finfo(np.longdouble).nmant < 63,
                                      reason="np.longdouble is no wider than fp64 here: no truth to hold the value to")


def textbook_biased(K, L):
    """tr(K H L H) / n^2 with an explicit centring matrix, in the dtype of K"""
    n = len(K)
    H = np.eye(n, dtype=K.dtype) - np.ones((n, n), dtype=K.dtype) / K.dtype.type(n)
    return np.trace(K @ H @ L @ H) / K.dtype.type(n * n)


def textbook_unbiased(K, L):
    """Song et al. 2012, eq. 4: [tr(K~ L~) + 1'K~1 1'L~1 / ((n - 1)(n - 2)) - 2 / (n - 2) 1'K~ L~1] / (n (n - 3))"""
    n = len(K)
    K, L = K.copy(), L.copy()
    np.fill_diagonal(K, 0)
    np.fill_diagonal(L, 0)
    one = np.ones(n, dtype=K.dtype)
    KL = K @ L
    return (np.trace(KL) + (one @ K @ one) * (one @ L @ one) / ((n - 1) * (n - 2)) - 2 * (one @ KL @ one) / (n - 2)) / (n * (n - 3))


@needs_longdouble
@pytest.mark.parametrize("n,d,q,labels", [(301, 3, 2, False), (130, 37, 1, False), (40, 5, 3, True), (4, 5, 1, False)])
def test_restatement_is_the_textbook_matrix_form(n, d, q, labels):
    z, y = HC.rows(n, d, q, seed=n + d)
    if labels:
        y = HC.labels_of(y)
    hz, hy = HC.bandwidth(z), (None if labels else HC.bandwidth(y))
    K, L = HC.kernel_matrices(z, y, hz, hy)
    Kl, Ll = HC.kernel_matrices(z, y, hz, hy, np.longdouble)
    perms = np.vstack([np.arange(n)[None], HC.numpy_permutations(n, 3, seed=n)])
    for estimator, textbook in (("biased", textbook_biased), ("unbiased", textbook_unbiased)):
        truth, tol, u, restated = HC.gate_of(K, L, Kl, Ll, perms, estimator)
        for p, perm in enumerate(perms):
            want = textbook(Kl, Ll[np.ix_(perm, perm)])
            print(f"n={n} {estimator} perm {p}: restated {HC.err_of(restated[p], want) / u[p]:.3f} u, truth "
                  f"{HC.err_of(truth[p], want) / u[p]:.2e} u from the textbook form (gate {tol[p] / u[p]:.2f} u)")
            assert HC.err_of(restated[p], want) <= tol[p] and HC.err_of(truth[p], want) <= tol[p]
        one = HC.gate_of(K, L, Kl, Ll, perms[2], estimator)  # one permutation: the same numbers as scalars
        assert one[0] == truth[2] and one[1] == tol[2] and one[3] == restated[2]


def test_restated_kernels_and_bandwidth():
    z, y = HC.rows(50, 7, 2, seed=1)
    K = HC.gauss_matrix(z, 3.0)
    assert np.array_equal(K, K.T) and (np.diag(K) == 1).all()
    from tests import mmd_checks as MC
    assert np.array_equal(np.sqrt(HC.sq_dist(z)), MC.pair_dist(z, z))  # pair_dist's sums, before its square root
    s = 0.0
    for j in range(7):
        s = s + (z[3, j] - z[11, j]) * (z[3, j] - z[11, j])
    assert HC.sq_dist(z)[3, 11] == s and K[3, 11] == np.exp(-s / 3.0)
    assert HC.bandwidth(z) == MC.bandwidth(z[:20], z[20:])  # the pooled rows of two sets are the one set
    assert HC.bandwidth(y[:, 0]) == HC.bandwidth(y[:, :1])
    c = HC.labels_of(y)
    assert set(c) == {0, 1, 2, 3}
    L = HC.delta_matrix(c)
    assert np.array_equal(L, HC.delta_matrix(7 - 2 * c)) and L.sum() == (np.bincount(c) ** 2).sum()
    # a permutation of y is a relabelling of L
    perm = HC.numpy_permutations(50, 1, 3)[0]
    Ly = HC.gauss_matrix(y, 2.0)
    assert np.array_equal(Ly[np.ix_(perm, perm)], HC.gauss_matrix(y[perm], 2.0))
    assert HC.hsic_value(K, Ly, perm, "biased") == HC.hsic_value(K, HC.gauss_matrix(y[perm], 2.0), np.arange(50), "biased")


@pytest.mark.parametrize("labels,table", [(False, HC.PVALUE_REAL), (True, HC.PVALUE_LABELS)])
def test_pvalue_cases_are_decided_by_the_restatement(labels, table):
    for a, (count, pvalue) in table.items():
        c = HC.pvalue_case(a, labels)
        assert int((c["restated"] >= c["t0"]).sum()) == count
        assert (1 + count) / 1000 == pvalue
        if np.finfo(np.longdouble).nmant >= 63:
            _, tol, u, _ = HC.hsic_gate(c["z"], c["y"], c["hz"], c["hy"], c["perms"], "biased", c["restated"])
            _, tol0, u0, _ = HC.hsic_gate(c["z"], c["y"], c["hz"], c["hy"], np.arange(301), "biased", c["t0"])
            margin = np.abs(c["restated"] - c["t0"]) - 2 * (tol + tol0)
            print(f"labels={labels} a={a}: nearest null value {np.min(np.abs(c['restated'] - c['t0'])) / u0:.3g} u from the statistic")
            assert (margin > 0).all(), "a restated null value lies within twice the summed gates of the statistic"


def test_closing_formulas_are_the_restated_ones():
    """the host-side formulas of the module on the restated sums give the restated statistic to rounding"""
    from scrubvae_amd.eval import independence as IN
    z, y = HC.rows(60, 4, 2, seed=5)
    K, L = HC.kernel_matrices(z, y, HC.bandwidth(z), HC.bandwidth(y))
    perm = HC.numpy_permutations(60, 1, 2)[0]
    Lp = L[np.ix_(perm, perm)]
    A = np.sum(np.triu(K * Lp, 1))
    k, l = K.sum(1), Lp.sum(1)
    for estimator, S in (("biased", np.sum(k * l)), ("unbiased", np.sum((k - 1) * (l - 1)))):
        got = IN.hsic_close(A, S, K.sum(), L.sum(), 60, estimator)
        t1, t2, t3 = HC.hsic_terms(K, L, perm, estimator)
        assert abs(got - (t1 - t2 + t3)) <= 8 * 2.0 ** -53 * (abs(t1) + abs(t2) + abs(t3))
    both = IN.hsic_close(np.array([A, A]), np.array([S, S]), K.sum(), L.sum(), 60, "unbiased")
    assert both[0].tobytes() == both[1].tobytes() == np.float64(got).tobytes()  # elementwise: a null value's bits are the statistic's


Z4 = np.arange(12.0).reshape(6, 2) ** 1.5
Y4 = np.arange(6.0) % 4.0
C4 = np.array([0, 1, 0, 1, 2, 2])


@pytest.mark.parametrize("z,y,kwargs", [
    (Z4, Y4[:5], {}),                                     # mismatched row counts
    (Z4, C4[:5], {}),
    (Z4[:1], Y4[:1], {}),                                 # n below the estimator's minimum
    (Z4[:3], Y4[:3], dict(estimator="unbiased")),
    (Z4[:3], C4[:3], dict(estimator="unbiased")),
    (Z4, Y4, dict(hz=0.0)),                               # bandwidths
    (Z4, Y4, dict(hz=-1.0)),
    (Z4, Y4, dict(hy=float("nan"))),
    (Z4, Y4, dict(hy=float("inf"))),
    (Z4, Y4, dict(hz=True)),
    (Z4, Y4, dict(estimator="u")),                        # unknown estimator
    (Z4, Y4, dict(estimator=None)),
    (Z4, np.zeros((6, 5)), {}),                           # too wide
    (Z4, np.zeros((6, 0)), {}),
    (Z4, np.zeros((6, 2, 1)), {}),
    (Z4, C4, dict(hy=1.0)),                               # hy with labels
    (Z4, np.zeros(6, dtype=np.int64), {}),                # one distinct label
    (Z4, np.stack([C4, C4], 1), {}),                      # labels must be 1-D
    (Z4, C4 > 0, {}),                                     # neither floating nor integer
    (Z4[:, 0], Y4, {}),                                   # z must be 2-D
    (Z4[:, :0], Y4, {}),
    (np.where(Z4 > 5, np.inf, Z4), Y4, {}),               # non-finite
    (Z4, np.where(Y4 > 2, np.nan, Y4), {}),
])
def test_argument_errors_before_device_work(z, y, kwargs, monkeypatch):
    """a ValueError before the library is touched: loading it fails the test"""
    from scrubvae_amd import _lib
    from scrubvae_amd.eval import hsic, hsic_permutation_test

    def touched():
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(_lib, "lib", touched)
    for fn, extra in ((hsic, {}), (hsic_permutation_test, dict(n_permutations=10))):
        with pytest.raises(ValueError):
            fn(z, y, **kwargs, **extra)
        with pytest.raises(ValueError):
            fn(torch.from_numpy(np.ascontiguousarray(z)), torch.from_numpy(np.ascontiguousarray(y)), **kwargs, **extra)


@pytest.mark.parametrize("kwargs", [
    dict(n_permutations=0),
    dict(n_permutations=65537),
    dict(n_permutations=10.0),
    dict(n_permutations=True),
    dict(permutations=np.zeros((3, 5), dtype=np.int64)),           # n is 6
    dict(permutations=np.arange(6)),                                # 1-D
    dict(permutations=np.zeros((0, 6), dtype=np.int64)),
    dict(permutations=np.tile(np.arange(6.0), (2, 1))),             # not integers
])
def test_permutation_errors_are_those_of_mmd_permutation_test(kwargs, monkeypatch):
    from scrubvae_amd import _lib
    from scrubvae_amd.eval import hsic_permutation_test
    from scrubvae_amd.eval import _permutation as PM
    from scrubvae_amd.eval import independence as IN
    from scrubvae_amd.eval import metrics as M
    assert IN._given_or_count is PM._given_or_count and IN._on_device_or_drawn is PM._on_device_or_drawn
    assert IN._pvalue is PM._pvalue and M.mmd_permutations is PM.mmd_permutations  # imported, not copied
    monkeypatch.setattr(_lib, "lib", lambda: (_ for _ in ()).throw(AssertionError("library loaded")))
    for y in (Y4, C4):
        with pytest.raises(ValueError):
            hsic_permutation_test(Z4, y, **kwargs)


def test_bandwidth_argument_errors(monkeypatch):
    from scrubvae_amd import _lib
    from scrubvae_amd.eval import hsic_bandwidth
    monkeypatch.setattr(_lib, "lib", lambda: (_ for _ in ()).throw(AssertionError("library loaded")))
    for a in (Z4[:1], Z4[:, :0], np.zeros((3, 2, 2)), np.array([1.0, np.nan, 2.0])):
        with pytest.raises(ValueError):
            hsic_bandwidth(a)


def test_variable_kinds():
    from scrubvae_amd.eval import _inputs as IN
    kind, v = IN._variable(Y4.astype(np.float32))
    assert kind == "real" and v.dtype == np.float64 and v.shape == (6, 1)
    kind, v = IN._variable(torch.from_numpy(np.stack([Y4, Y4], 1)))
    assert kind == "real" and v.dtype == torch.float64 and tuple(v.shape) == (6, 2)
    for c in (C4, C4.astype(np.uint8), torch.from_numpy(C4).to(torch.int32), 10 - 3 * C4):
        kind, v = IN._variable(c)
        assert kind == "labels" and v.dtype == np.int32 and v.flags.c_contiguous
        assert np.array_equal(v[:, None] == v[None, :], C4[:, None] == C4[None, :])


def test_new_exports_have_signatures():
    from scrubvae_amd import _lib
    from scrubvae_amd.eval import independence as IN
    lib = _lib.lib()
    work = lib.svae_hsic_work
    Pc, nmax = _lib.HSIC_PERMS, _lib.MMD_NULL_MAX
    assert work(1, 1) == 0 and work(0, 1) == 0 and work(-3, 1) == 0 and work(2 ** 26, 1) == 0
    assert work(10, 0) == 0 and work(10, -1) == 0 and work(10, nmax + 1) == 0
    # column chunks (at most 8) x row tiles x the larger of 2 x 64 (the moments' partials) and P padded to whole chunks of Pc
    assert work(2, 1) == 128 and work(64, 128) == 128 and work(64, 129) == 128 + Pc
    assert work(301, 256) == 5 * 5 * 256 and work(1030, 17) == 6 * 17 * 128   # 17 tiles: 6 chunks of 3
    assert work(100000, 256) == 8 * 1563 * 256
    assert work(2 ** 26 - 1, nmax) > 0
    # argument errors come before any device work (the pointers are never read)
    fake = 4096
    E = _lib.ERR_ARG

    def cross(Z=fake, ld=3, d=3, n=10, hz=fake, Y=fake, q=2, lab=None, hy=fake, perm=fake, P=3, w=fake, out=fake):
        return lib.svae_hsic_cross(Z, ld, d, n, hz, Y, q, lab, hy, perm, P, w, out, None)

    for bad in (dict(n=1), dict(n=2 ** 26), dict(d=0), dict(ld=2), dict(Z=None), dict(q=0), dict(q=_lib.HSIC_MAX_Y + 1), dict(hy=None),
                dict(Y=None), dict(lab=fake), dict(P=0), dict(P=nmax + 1), dict(perm=None), dict(hz=None), dict(w=None), dict(out=None)):
        assert cross(**bad) == E, bad
    assert "null" in _lib.last_error()
    assert cross(q=_lib.HSIC_MAX_Y + 1) == E and "at most" in _lib.last_error()

    def moments(X=fake, ld=3, d=3, lab=None, n=10, h=fake, w=fake, rowsum=fake, mom=fake):
        return lib.svae_hsic_moments(X, ld, d, lab, n, h, w, rowsum, mom, None)

    for bad in (dict(n=1), dict(d=0), dict(ld=2), dict(X=None), dict(lab=fake), dict(h=None), dict(w=None), dict(rowsum=None),
                dict(mom=None), dict(X=None, lab=fake, n=1)):
        assert moments(**bad) == E, bad

    def dots(k=fake, l=fake, n=10, perm=fake, P=3, tilde=0, out=fake):
        return lib.svae_hsic_dots(k, l, n, perm, P, tilde, out, None)

    for bad in (dict(k=None), dict(l=None), dict(out=None), dict(n=1), dict(P=0), dict(P=nmax + 1), dict(perm=None)):
        assert dots(**bad) == E, bad
    import scrubvae_amd.eval as EV
    for name in ("hsic", "hsic_bandwidth", "hsic_permutation_test", "HSICPermutationResult"):
        assert callable(getattr(EV, name))
    assert _lib.HSIC_MAX_Y >= 4 and IN._HSIC_CALLS.keys() >= {"select", "moments", "cross", "dots"}
    r = IN.HSICPermutationResult(1.0, 0.5, np.zeros(3), 2.0, None, 0.25)
    assert (r.statistic, r.pvalue, r.hz, r.hy, r.normalized) == (1.0, 0.5, 2.0, None, 0.25) and "normalized=0.25" in repr(r)
