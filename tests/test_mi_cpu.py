"""kNN mutual information without a GPU: the restatement of tests/mi_checks.py pinned to scipy's digamma and to sklearn's
estimators, the outcomes of the sanity pair that test_gpu_mi.py repeats on the device, argument errors before any device work and
the C-ABI exports."""
import math

import numpy as np
import pytest
import torch

from tests import mi_checks as MC

CPU_SIZES = [(301, 3), (130, 5), (1037, 3)]   # n, k of the sklearn comparisons
TOL = 4 * 2.0 ** -52


def test_psi_against_digamma():
    special = pytest.importorskip("scipy.special")
    from scrubvae_amd.eval import mutual_info as MI
    m = np.arange(1, 2 ** 20 + 1)
    got, want = MI.psi_int(m), special.digamma(m.astype(np.float64))
    dev = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print(f"largest deviation {dev.max() / 2.0 ** -53:.2f} x 2^-53 x max(1, |psi|) at m = {m[dev.argmax()]}")
    assert dev.max() <= 4 * 2.0 ** -53
    # the restatement's one-value-at-a-time recipe is the module's, bit for bit, on both sides of m = 16
    some = np.concatenate([np.arange(1, 40), [255, 1037, 50000, 2 ** 20, 2 ** 31 - 1]])
    assert MC.psi_int(some).tobytes() == MI.psi_int(some).tobytes()
    assert MI.psi_int(1) == -0.5772156649015329 and MI.psi_int(2) == -0.5772156649015329 + 1.0
    assert float(MI.psi_int(np.int64(20))) == MI.psi_int(np.array([20]))[0] and MI.psi_int(np.zeros(0, int)).shape == (0,)
    with pytest.raises(ValueError):
        MI.psi_int(np.array([3, 0]))


def test_gate_is_below_its_ceiling():
    for n in (2, 3, 30, 1037, 10 ** 6):
        L = max(1.0, math.log(n))
        assert 0 < MC.mi_gate(n) <= 64 * 2.0 ** -53 * L and MC.mi_gate(n) == 54 * 2.0 ** -53 * L


@pytest.mark.parametrize("n,k", CPU_SIZES)
def test_ksg_against_sklearn(n, k):
    mi = pytest.importorskip("sklearn.feature_selection._mutual_info")
    x, y = MC.cpu_rows(n, seed=n)
    # the preconditions under which sklearn's tree search and this contract must agree: no ties among the first k + 1 keys of
    # a row, and k small enough that sklearn keeps its KD-tree (its brute-force search takes dot-product distances)
    assert k < n // 2
    m = np.maximum(MC.sq_dist(x[:, None]), MC.sq_dist(y[:, None]))
    assert MC.tie_free([np.delete(m[i], i) for i in range(n)], k)
    I, rho2, nz, ny = MC.ksg(x[:, None], y, k)
    want = mi._compute_mi_cc(x, y, k)
    print(f"n={n} k={k}: restated {I!r}, sklearn {want!r}, apart {abs(max(I, 0.0) - want) / 2.0 ** -52:.2f} x 2^-52")
    assert abs(max(I, 0.0) - want) <= TOL
    assert (rho2 > 0).all() and (nz >= k - 1).all() and (ny >= k - 1).all()


@pytest.mark.parametrize("n,k", CPU_SIZES)
def test_ross_against_sklearn(n, k):
    mi = pytest.importorskip("sklearn.feature_selection._mutual_info")
    x, lab = MC.cpu_rows(n, seed=n, classes=4)
    count = np.bincount(lab)
    assert len(count) == 4 and k < n // 2 and (k < count // 2).all()
    s = MC.sq_dist(x[:, None])
    assert MC.tie_free([s[i, (lab == lab[i]) & (np.arange(n) != i)] for i in range(n)], k)
    I, rho2, nz, ki, c, kept = MC.ross(x[:, None], lab, k)
    want = mi._compute_mi_cd(x, lab, k)
    print(f"n={n} k={k}: restated {I!r}, sklearn {want!r}, apart {abs(max(I, 0.0) - want) / 2.0 ** -52:.2f} x 2^-52")
    assert abs(max(I, 0.0) - want) <= TOL
    assert kept.all() and (ki == k).all() and np.array_equal(c, count[lab]) and (nz >= k - 1).all()


def test_ross_drops_single_labels():
    z, lab, I, rho2, nz, ki, c, kept = MC.label_case()
    n, d, k = MC.LABEL_CASE
    assert len(z) == n + 2 and kept.sum() == n and set(lab[~kept]) == {100, -50}
    assert sorted(np.bincount(c)[list(MC.LABEL_SIZES)] // np.array(MC.LABEL_SIZES)) == [1] * 5
    assert set(ki) == {5, 2, 1} and np.array_equal(ki, np.minimum(k, c - 1))
    # the dropped rows change nothing: the same call on the kept rows alone
    again = MC.ross(z[kept], lab[kept], k)
    assert again[0] == I and np.array_equal(again[1], rho2) and np.array_equal(again[2], nz) and again[5].all()


def test_constant_y_and_one_class_give_the_knn_distance_on_the_restatements():
    """what test_gpu_mi.py holds the device's walks to each other with: under a constant y the joint key is s^z, and under one class
    every other row is a candidate, so rho2 is the square of the k-th neighbour distance of tests/knn_checks.py, bit for bit"""
    from tests import knn_checks as KC
    x, _, dist, _ = KC.case(301, 3, 5)
    rho2 = MC.ksg(x, np.zeros((301, 1)), 5)[1]
    assert np.sqrt(rho2).tobytes() == np.ascontiguousarray(dist[:, 4]).tobytes()
    x, _, dist, _ = KC.case(131, 128, 7)
    _, rho2, _, ki, _, kept = MC.ross(x, np.zeros(131, dtype=np.int64), 7)
    assert kept.all() and (ki == 7).all()
    assert np.sqrt(rho2).tobytes() == np.ascontiguousarray(dist[:, 6]).tobytes()
    # the arguments the device test builds for this case are shaped like the checked ones of a case that is accepted
    from scrubvae_amd.eval import mutual_info as MI
    ours, theirs = MC.one_class_arguments(x, 7), MI._mi_check(Z6, C6, 2)
    assert ours.keys() == theirs.keys() and all(np.asarray(ours[key]).dtype == np.asarray(theirs[key]).dtype for key in ours)


@pytest.mark.parametrize("n,d,k", MC.SCORES)
def test_latent_scores_against_sklearn(n, d, k):
    fs = pytest.importorskip("sklearn.feature_selection")
    from scrubvae_amd.eval import mutual_info as MI
    z, y, lab = MC.scores_rows(n, d, seed=n)
    for target, discrete, theirs in ((y, False, fs.mutual_info_regression), (lab, True, fs.mutual_info_classif)):
        got = MC.latent_scores(z, target, discrete, k, 0)
        want = theirs(z, target, n_neighbors=k, random_state=0)
        print(f"n={n} d={d} k={k} discrete={discrete}: apart {np.abs(got - want).max() / 2.0 ** -52:.2f} x 2^-52")
        assert got.shape == (d,) and np.abs(got - want).max() <= TOL and got[0] > 0.3
        a, b = MC.scores_inputs(z, target, discrete, 0), MI.mi_scores_inputs(z, target, discrete, 0)
        assert a[0].tobytes() == b[0].tobytes() and np.asarray(a[1]).tobytes() == np.asarray(b[1]).tobytes()
    const = z.copy()
    const[:, 1] = 3.0    # a zero deviation is read as 1: the column keeps its value and gets its noise
    assert np.abs(MC.scores_inputs(const, y, False, 0)[0][:, 1] - 3.0).max() < 1e-8


def test_sanity_pair_on_the_restatement():
    """what test_gpu_mi.py expects of the device is decided here first"""
    n, d, k, P = MC.SANITY
    for dependent in (True, False):
        z, y, perms = MC.sanity_case(dependent)
        stat = MC.ksg(z, y, k)[0]
        null = np.array([MC.ksg(z, y[p], k)[0] for p in perms])
        margin = np.abs(null - stat).min()
        print(f"dependent={dependent}: statistic {stat:.4f}, null in [{null.min():.4f}, {null.max():.4f}]")
        assert margin > 4 * MC.mi_gate(n)     # no null value close enough to the statistic for the gate to decide the count
        if dependent:
            assert (1 + int((null >= stat).sum())) / (1 + P) == 1 / (P + 1)
        else:
            assert null.min() < stat < null.max()


def test_closing_formulas_are_the_restated_ones():
    from scrubvae_amd.eval import mutual_info as MI
    n, d, q, k = MC.SIZES[0]
    z, y, I, rho2, nz, ny = MC.real_case(n, d, q, k)
    got = MI.mi_close_real(n, k, math.fsum(MC.psi_int(nz + 1)), math.fsum(MC.psi_int(ny + 1)))
    assert float(got) == I
    both = MI.mi_close_real(n, k, np.array([1.5, 1.5]), np.array([2.5, 2.5]))
    assert both[0].tobytes() == both[1].tobytes() == np.float64(MI.mi_close_real(n, k, 1.5, 2.5)).tobytes()  # elementwise
    z, lab, I, rho2, nz, ki, c, kept = MC.label_case()
    count = np.unique(lab[kept], return_counts=True)[1]
    mk, mc = MI.mi_class_terms(count, MC.LABEL_CASE[2])
    assert float(MI.mi_close_labels(len(nz), mk, mc, math.fsum(MC.psi_int(nz + 1)))) == I
    assert MI.mi_class_terms(count[::-1], MC.LABEL_CASE[2]) == (mk, mc)   # exactly rounded sums: the class order changes no bit
    assert abs(mk - MC.psi_int(ki).mean()) < 1e-12 and abs(mc - MC.psi_int(c).mean()) < 1e-12


Z6 = np.arange(24.0).reshape(8, 3) ** 1.5
Y6 = np.arange(8.0) % 5.0
C6 = np.array([0, 1, 0, 1, 2, 2, 0, 1])


@pytest.mark.parametrize("z,y,kwargs", [
    (Z6, Y6[:7], {}),                                       # mismatched row counts
    (Z6, C6[:7], {}),
    (np.where(Z6 > 50, np.inf, Z6), Y6, {}),                # non-finite rows
    (Z6, np.where(Y6 > 3, np.nan, Y6), {}),
    (Z6, Y6, dict(n_neighbors=0)),                          # n_neighbors
    (Z6, Y6, dict(n_neighbors=8)),                          # n - 1 = 7
    (Z6, Y6, dict(n_neighbors=3.0)),
    (Z6, Y6, dict(n_neighbors=True)),
    (Z6, Y6, dict(n_neighbors=None)),
    (np.zeros((40, 2)), np.zeros(40), dict(n_neighbors=33)),  # MI_MAX_K = 32
    (Z6, C6, dict(n_neighbors=8)),
    (Z6, np.array([0, 0, 0, 1, 1, 2, 3, 4]), dict(n_neighbors=5)),   # 5 rows kept: at most 4 neighbours
    (Z6, np.zeros((8, 5)), {}),                             # real y wider than 4
    (Z6, np.zeros((8, 0)), {}),
    (Z6, np.zeros((8, 2, 1)), {}),
    (Z6, np.stack([C6, C6], 1), {}),                        # labels must be 1-D
    (Z6, C6 > 0, {}),                                       # neither floating nor integer
    (Z6, np.zeros(8, dtype=np.int64), {}),                  # one class
    (Z6, np.array([0, 0, 0, 0, 0, 0, 1, 2]), {}),           # one class with two members or more
    (Z6, np.arange(8), {}),                                 # none
    (Z6[:1], Y6[:1], dict(n_neighbors=1)),                  # one row has no neighbour
    (Z6[:4], np.array([0, 0, 1, 2]), dict(n_neighbors=1)),  # fewer than 3 rows after the drop
    (Z6[:, 0], Y6, {}),                                     # z must be 2-D
    (Z6[:, :0], Y6, {}),
])
def test_argument_errors_before_device_work(z, y, kwargs, monkeypatch):
    """a ValueError before the library is touched: loading it fails the test"""
    from scrubvae_amd import _lib
    from scrubvae_amd.eval import mutual_information, mutual_information_permutation_test

    def touched():
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(_lib, "lib", touched)
    for fn, extra in ((mutual_information, {}), (mutual_information_permutation_test, dict(n_permutations=10))):
        with pytest.raises(ValueError):
            fn(z, y, **kwargs, **extra)
        with pytest.raises(ValueError):
            fn(torch.from_numpy(np.ascontiguousarray(z)), torch.from_numpy(np.ascontiguousarray(y)), **kwargs, **extra)


@pytest.mark.parametrize("z,y,kwargs", [
    (Z6, Y6[:7], {}),
    (Z6, C6, {}),                                           # labels without discrete_target
    (Z6, Y6, dict(discrete_target=True)),                   # and the reverse
    (Z6, np.stack([Y6, Y6], 1), {}),                        # one real target
    (Z6, Y6, dict(n_neighbors=8)),
    (Z6, np.zeros(8, dtype=np.int64), dict(discrete_target=True)),
    (np.where(Z6 > 50, np.nan, Z6), Y6, {}),
    (Z6[:, :0], Y6, {}),
])
def test_score_argument_errors_before_device_work(z, y, kwargs, monkeypatch):
    from scrubvae_amd import _lib
    from scrubvae_amd.eval import latent_mi_scores
    monkeypatch.setattr(_lib, "lib", lambda: (_ for _ in ()).throw(AssertionError("library loaded")))
    with pytest.raises(ValueError):
        latent_mi_scores(z, y, **kwargs)


@pytest.mark.parametrize("kwargs", [
    dict(n_permutations=0),
    dict(n_permutations=65537),
    dict(n_permutations=10.0),
    dict(n_permutations=True),
    dict(permutations=np.zeros((3, 7), dtype=np.int64)),           # n is 8
    dict(permutations=np.arange(8)),                                # 1-D
    dict(permutations=np.zeros((0, 8), dtype=np.int64)),
    dict(permutations=np.tile(np.arange(8.0), (2, 1))),             # not integers
])
def test_permutation_errors_are_those_of_mmd_permutation_test(kwargs, monkeypatch):
    from scrubvae_amd import _lib
    from scrubvae_amd.eval import _permutation as PM
    from scrubvae_amd.eval import metrics as M
    from scrubvae_amd.eval import mutual_info as MI
    assert MI._given_or_count is PM._given_or_count and MI._on_device_or_drawn is PM._on_device_or_drawn
    assert MI._pvalue is PM._pvalue and M.mmd_permutations is PM.mmd_permutations  # imported, not copied
    monkeypatch.setattr(_lib, "lib", lambda: (_ for _ in ()).throw(AssertionError("library loaded")))
    for y in (Y6, C6):
        with pytest.raises(ValueError):
            MI.mutual_information_permutation_test(Z6, y, **kwargs)


def test_checked_arguments():
    from scrubvae_amd.eval import mutual_info as MI
    c = MI._mi_check(Z6.astype(np.float32), np.stack([Y6, Y6], 1), 3)
    assert c["kind"] == "real" and c["n"] == 8 and c["k"] == 3 and c["kept"].all() and c["v"].shape == (8, 2) and c["x"].dtype == np.float64
    lab = np.array([5, 9, 5, 9, -2, 7, 5, 9])       # -2 and 7 occur once
    c = MI._mi_check(torch.from_numpy(Z6), torch.from_numpy(lab), 2)
    assert c["kind"] == "labels" and c["n"] == 6
    assert np.array_equal(c["kept"], (lab == 5) | (lab == 9)) and np.array_equal(c["lab"], [0, 1, 0, 1, 0, 1])
    assert np.array_equal(c["count"], [3, 3]) and np.array_equal(c["kk"], [2] * 6) and c["lab"].dtype == c["kk"].dtype == np.int32
    assert np.array_equal(MI._mi_check(Z6, np.array([0, 0, 0, 0, 0, 0, 1, 1]), 4)["kk"], [4] * 6 + [1] * 2)


def test_new_exports_have_signatures():
    from scrubvae_amd import _lib
    from scrubvae_amd.eval import mutual_info as MI
    lib = _lib.lib()
    work, K = lib.svae_mi_work, _lib.MI_MAX_K
    assert work(1, 1) == 0 and work(0, 1) == 0 and work(-3, 1) == 0 and work(10, 0) == 0 and work(10, 10) == 0 and work(100, K + 1) == 0
    # column chunks (at most 8, fewer once the grid holds 512 blocks) x rows padded to 64 x k x 12 bytes
    assert work(2, 1) == 64 * 12 and work(301, 3) == 5 * 320 * 3 * 12 and work(1037, 10) == 6 * 1088 * 10 * 12
    assert work(64 * 512 + 7, K) == (64 * 513) * K * 12 and work(2 ** 31 - 1, K) > 0
    fake, E = 4096, _lib.ERR_ARG

    def radius(Z=fake, ld=3, d=3, n=40, Y=fake, q=2, lab=None, kk=None, k=3, w=fake, rho2=fake):
        return lib.svae_mi_radius(Z, ld, d, n, Y, q, lab, kk, k, w, rho2, None)

    for bad, text in ((dict(k=0), "neighbour count"), (dict(k=K + 1), "neighbour count"), (dict(k=40), "neighbour count"),
                      (dict(n=30, k=30), "neighbour count"), (dict(q=_lib.MI_MAX_Y + 1), "at most"), (dict(q=0), "width"),
                      (dict(lab=fake, kk=fake), "exactly one"), (dict(Y=None), "exactly one"), (dict(w=None), "null"),
                      (dict(rho2=None), "null"), (dict(kk=fake), "kk"), (dict(Y=None, lab=fake), "kk"), (dict(n=1), "bad rows"),
                      (dict(Z=None), "bad rows"), (dict(ld=2), "bad rows"), (dict(d=0), "bad rows")):
        assert radius(**bad) == E and text in _lib.last_error(), (bad, _lib.last_error())
    assert radius(w=fake + 4) == _lib.ERR_ALIGN

    def counts_(Z=fake, ld=3, d=3, n=40, Y=fake, q=2, rho2=fake, nz=fake, ny=fake):
        return lib.svae_mi_counts(Z, ld, d, n, Y, q, rho2, nz, ny, None)

    for bad in (dict(n=1), dict(d=0), dict(ld=2), dict(Z=None), dict(q=0), dict(q=_lib.MI_MAX_Y + 1), dict(Y=None), dict(ny=None),
                dict(rho2=None), dict(nz=None), dict(Y=None, ny=None, nz=None)):
        assert counts_(**bad) == E, bad
    for bad in (dict(a=None), dict(out=None), dict(n=0)):
        args = dict(a=fake, b=fake, n=10, out=fake)
        args.update(bad)
        assert lib.svae_mi_psi_sums(args["a"], args["b"], args["n"], args["out"], None) == E, bad
    import scrubvae_amd.eval as EV
    for name in ("mutual_information", "mutual_information_permutation_test", "latent_mi_scores", "MIPermutationResult"):
        assert callable(getattr(EV, name))
    assert _lib.MI_MAX_K == 32 and _lib.MI_MAX_Y == 4
    assert MI._MI_CALLS.keys() >= {"radius", "counts", "psi_sums"}
    r = MI.MIPermutationResult(1.0, 0.5, np.zeros(3))
    assert (r.statistic, r.pvalue) == (1.0, 0.5) and "pvalue=0.5" in repr(r)


def test_constants_equal_the_header():
    from scrubvae_amd import _lib
    assert _lib.MI_MAX_K == MC.MAX_K and _lib.MI_MAX_Y == MC.MAX_Y
    from scrubvae_amd import build
    assert "mi.hip" in build.SOURCES and any(h.endswith("knn_buffer.h") for h in build.HEADERS)


def test_mutual_information_needs_the_built_library(monkeypatch, tmp_path):
    """no fallback: without the library the estimate fails at its first load, it does not compute on the host"""
    from scrubvae_amd import _lib
    from scrubvae_amd.eval import mutual_info as MI
    from scrubvae_amd.eval import mutual_information
    assert mutual_information is MI.mutual_information
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "libscrubvae_hip.so"))
    with pytest.raises(RuntimeError, match="not found"):
        MI._MiRun(MI._mi_check(Z6, Y6, 2), torch.device("cpu"))
