"""kNN conditional mutual information without a GPU: the restatement of tests/cmi_checks.py held to the unconditional one of
tests/mi_checks.py where the two must agree, the outcomes of the sanity pair that test_gpu_cmi.py repeats on the device, the
properties of the local permutation draw, argument errors before any device work and the C-ABI exports."""
import math

import numpy as np
import pytest
import torch

from tests import cmi_checks as CC
from tests import mi_checks as MC


def test_gate_is_below_its_ceiling():
    for n in (2, 3, 30, 1037, 10 ** 6):
        L = max(1.0, math.log(n))
        assert 0 < CC.cmi_gate(n) <= 96 * 2.0 ** -53 * L and CC.cmi_gate(n) == 78 * 2.0 ** -53 * L


def test_stratified_is_the_class_weighted_ksg():
    z, y, lab, I, rho2, nzc, nyc, kept = CC.label_case()
    k = CC.LABEL_K
    assert len(z) == sum(CC.LABEL_SIZES) and kept.sum() == sum(s for s in CC.LABEL_SIZES if s > k)
    assert sorted(np.unique(lab[~kept], return_counts=True)[1]) == [2, 3]
    zk, yk, lk = z[kept], y[kept], lab[kept]
    total, n = 0.0, int(kept.sum())
    for cl in np.unique(lk):
        rows = lk == cl
        value, r2, nz, ny = MC.ksg(zk[rows], yk[rows], k)
        total += rows.sum() / n * value
        assert r2.tobytes() == rho2[rows].tobytes() and np.array_equal(nz, nzc[rows]) and np.array_equal(ny, nyc[rows])
    assert abs(I - total) <= 1e-12
    # the class of 6 has exactly k other rows: the farthest of them sets rho2 in one of the two spaces and is not counted there
    six = np.unique(lk)[[int((lk == cl).sum()) == 6 for cl in np.unique(lk)]][0]
    assert (np.maximum(nzc, nyc)[lk == six] <= k).all() and (np.minimum(nzc, nyc)[lk == six] <= k - 1).all()
    # the dropped rows change nothing
    again = CC.cmi_strat(zk, yk, lk, k)
    assert again[0] == I and again[4].all() and again[1].tobytes() == rho2.tobytes()


@pytest.mark.parametrize("n,d,q,k", [(301, 3, 1, 3), (130, 37, 2, 5)])
def test_constant_c_gives_ksg(n, d, q, k):
    z, y, I, rho2, nz, ny = MC.real_case(n, d, q, k)
    got, r2, nzc, nyc, nc = CC.cmi_real(z, y, np.full((n, 2), 3.25), k)
    assert r2.tobytes() == rho2.tobytes() and np.array_equal(nzc, nz) and np.array_equal(nyc, ny)
    assert (rho2 > 0).all() and (nc == n - 1).all()
    assert abs(got - I) <= 1e-12          # psi(k) + psi(n) - ... in another order of the same terms


def test_constant_c_on_duplicates():
    z, y, I, rho2, nz, ny = MC.grid_case(False)
    got, r2, nzc, nyc, nc = CC.cmi_real(z, y, np.zeros(len(z)), MC.GRID_K)
    assert r2.tobytes() == rho2.tobytes() and np.array_equal(nzc, nz) and np.array_equal(nyc, ny)
    assert (rho2 == 0).any() and np.array_equal(nc, np.where(rho2 > 0, len(z) - 1, 0))


def test_sanity_pair_on_the_restatement():
    """what test_gpu_cmi.py expects of the device is decided here first"""
    n, k, P, donors = CC.SANITY
    z, y, y2, c = CC.sanity_case()
    unconditional, confounded, direct = MC.ksg(z, y, k)[0], CC.cmi_real(z, y, c, k)[0], CC.cmi_real(z, y2, c, k)[0]
    print(f"I(z; y) {unconditional:.4f}, I(z; y | c) {confounded:.4f}, I(z; y2 | c) {direct:.4f}")
    assert unconditional >= 0.5 and abs(confounded) <= 0.05 and direct >= 0.25


def test_local_null_of_the_direct_case_on_the_restatement():
    """19 local permutations at 8 donors: the null of the direct case stays far below its statistic"""
    n, k, P, donors = CC.SANITY
    z, y, y2, c = CC.sanity_case()
    direct = CC.cmi_real(z, y2, c, k)[0]
    nbr, order, scan = CC.draw_inputs(n, donors, P, seed=3, values=c)
    maps = CC.local_permutation(nbr, order, scan)
    null = np.array([CC.cmi_real(z, y2[m], c, k)[0] for m in maps])
    print(f"direct {direct:.4f}, null in [{null.min():.4f}, {null.max():.4f}]")
    assert null.max() < 0.04 < direct


@pytest.mark.parametrize("n,kp,P", CC.DRAWS)
def test_local_permutation_properties(n, kp, P):
    nbr, order, scan = CC.draw_inputs(n, kp, P, seed=n + kp)
    out = CC.local_permutation(nbr, order, scan)
    assert out.shape == (P, n)
    for p in range(P):
        assert all(out[p, i] in nbr[i] for i in range(n))                      # every image is a donor of its row
        first = order[p, 0]
        assert out[p, first] == nbr[first, scan[p, first, 0]]                  # the first visit finds everything unused
    one = CC.local_permutation(nbr[:, :1], order, np.zeros((P, n, 1), np.uint8))
    assert np.array_equal(one, np.tile(np.arange(n), (P, 1)))                  # kp = 1: the row itself


def test_local_permutation_repeats_a_donor_when_all_are_used():
    nbr = np.array([[0, 1], [1, 0], [2, 0]])
    order, scan = np.array([[0, 1, 2]]), np.array([[[1, 0], [1, 0], [1, 0]]])
    # row 0 takes 1; row 1 takes 0; row 2 finds 0 and 2... scan (1, 0): donor nbr[2][1] = 0 is used, then nbr[2][0] = 2 is free
    assert CC.local_permutation(nbr, order, scan).tolist() == [[1, 0, 2]]
    nbr = np.array([[0, 1], [1, 0], [0, 1]])
    # row 2 finds both of its donors used and keeps the last one tried, nbr[2][scan = 0] = 0: used twice
    assert CC.local_permutation(nbr, order, scan).tolist() == [[1, 0, 0]]


Z6 = np.arange(24.0).reshape(8, 3) ** 1.5
Y6 = np.arange(8.0) % 5.0
C6 = np.array([0, 1, 0, 1, 2, 2, 0, 1])
R6 = np.cos(np.arange(8.0))


@pytest.mark.parametrize("z,y,c,kwargs", [
    (Z6, Y6[:7], R6, {}),                                      # mismatched row counts
    (Z6, Y6, R6[:7], {}),
    (Z6, Y6, C6[:7], dict(n_neighbors=1)),
    (Z6, C6[:7], R6, dict(n_neighbors=1)),
    (np.where(Z6 > 50, np.inf, Z6), Y6, R6, {}),               # non-finite rows
    (Z6, np.where(Y6 > 3, np.nan, Y6), R6, {}),
    (Z6, Y6, np.where(R6 > 0.9, np.nan, R6), {}),
    (Z6, np.zeros((8, 5)), R6, {}),                            # widths above the caps
    (Z6, Y6, np.zeros((8, 5)), {}),
    (Z6, Y6, np.zeros((8, 0)), {}),
    (Z6, C6, np.zeros((8, 5)), dict(n_neighbors=1)),
    (Z6, Y6, R6, dict(n_neighbors=0)),                         # n_neighbors
    (Z6, Y6, R6, dict(n_neighbors=8)),                         # n - 1 = 7
    (Z6, Y6, R6, dict(n_neighbors=3.0)),
    (Z6, Y6, R6, dict(n_neighbors=True)),
    (np.zeros((40, 2)), np.zeros(40), np.zeros(40), dict(n_neighbors=33)),   # MI_MAX_K = 32
    (Z6, Y6, C6, dict(n_neighbors=8)),
    (Z6, Y6, C6, dict(n_neighbors=3)),                         # no class has more than 3 rows
    (Z6[:4], Y6[:4], np.array([0, 0, 1, 2]), dict(n_neighbors=1)),      # fewer than 3 rows after the drop
    (Z6, C6, C6, dict(n_neighbors=1)),                         # labels for both
    (Z6, C6, R6, dict(n_neighbors=8)),                         # label y: the checks of mutual_information
    (Z6, np.arange(8), R6, dict(n_neighbors=1)),               # no class of y with two members
    (Z6[:, 0], Y6, R6, {}),                                    # z must be 2-D
    (Z6[:, :0], Y6, R6, {}),
    (Z6, Y6, C6 > 0, {}),                                      # c neither floating nor integer
    (Z6, Y6, np.stack([C6, C6], 1), {}),                       # labels must be 1-D
    (Z6, Y6, np.zeros(8, dtype=np.int64), {}),                 # one class
])
def test_argument_errors_before_device_work(z, y, c, kwargs, monkeypatch):
    """a ValueError before the library is touched: loading it fails the test"""
    from scrubvae_amd import _lib
    from scrubvae_amd.eval import conditional_mutual_information, conditional_mutual_information_permutation_test

    def touched():
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(_lib, "lib", touched)
    for fn, extra in ((conditional_mutual_information, {}), (conditional_mutual_information_permutation_test, dict(n_permutations=10))):
        with pytest.raises(ValueError):
            fn(z, y, c, **kwargs, **extra)
        with pytest.raises(ValueError):
            fn(*(torch.from_numpy(np.ascontiguousarray(a)) for a in (z, y, c)), **kwargs, **extra)


@pytest.mark.parametrize("kwargs", [
    dict(n_permutations=0),
    dict(n_permutations=65537),
    dict(n_permutations=10.0),
    dict(n_permutations=True),
    dict(n_donors=1),                                               # 2 .. min(n, 64)
    dict(n_donors=9),                                               # n is 8
    dict(n_donors=4.0),
    dict(n_donors=True),
    dict(permutations=np.zeros((3, 7), dtype=np.int64)),            # n is 8
    dict(permutations=np.arange(8)),                                # 1-D
    dict(permutations=np.zeros((0, 8), dtype=np.int64)),
    dict(permutations=np.tile(np.arange(8.0), (2, 1))),             # not integers
    dict(permutations=np.tile(np.arange(1, 9), (2, 1))),            # 8 is out of range
    dict(permutations=np.tile(np.arange(-1, 7), (2, 1))),
])
def test_permutation_argument_errors(kwargs, monkeypatch):
    from scrubvae_amd import _lib
    from scrubvae_amd.eval import _permutation as PM
    from scrubvae_amd.eval import conditional_mi as CM
    from scrubvae_amd.eval import metrics as M
    assert CM._given_or_count is PM._given_or_count and CM._count is PM._count   # imported, not copied
    assert CM.mmd_permutations is M.mmd_permutations
    monkeypatch.setattr(_lib, "lib", lambda: (_ for _ in ()).throw(AssertionError("library loaded")))
    with pytest.raises(ValueError):
        CM.conditional_mutual_information_permutation_test(Z6, Y6, R6, n_neighbors=2, **kwargs)
    if "n_donors" not in kwargs:                                    # the class draw reads no donor count
        with pytest.raises(ValueError):
            CM.conditional_mutual_information_permutation_test(Z6, Y6, C6, n_neighbors=1, **kwargs)
    if "permutations" not in kwargs:
        args = dict(n_permutations=5)
        args.update(kwargs)
        with pytest.raises(ValueError):
            CM.conditional_permutations(R6, args.pop("n_permutations"), **args)
    for bad in (np.zeros((8, 5)), C6 > 0, np.where(R6 > 0.9, np.inf, R6)):
        with pytest.raises(ValueError):
            CM.conditional_permutations(bad, 5)
    # a row of a given table need not be a permutation: the checks let a repeated donor through (and then look for a device)
    repeated = np.zeros((2, 8), dtype=np.int64)
    assert CM._cmi_given_permutations(repeated, 8).shape == (2, 8)
    with pytest.raises(ValueError):
        CM._donor_count(8, 2 ** 19 + 1)                             # the used-bitmap of the draw
    assert CM._donor_count(64, 2 ** 19) == 64


def test_checked_arguments():
    from scrubvae_amd.eval import conditional_mi as CM
    c = CM._cmi_check(Z6.astype(np.float32), np.stack([Y6, Y6], 1), R6, 3)
    assert c["kind"] == "real" and c["n"] == 8 and c["k"] == 3 and c["kept"].all()
    assert c["v"].shape == (8, 2) and c["w"].shape == (8, 1) and c["x"].dtype == np.float64
    lab = np.array([5, 9, 5, 9, -2, 7, 5, 9])            # -2 and 7 occur once
    c = CM._cmi_check(torch.from_numpy(Z6), Y6, torch.from_numpy(lab), 2)
    assert c["kind"] == "strat" and c["n"] == 6 and np.array_equal(c["kept"], (lab == 5) | (lab == 9))
    assert np.array_equal(c["lab"], [0, 1, 0, 1, 0, 1]) and np.array_equal(c["count"], [3, 3]) and c["lab"].dtype == np.int32
    c = CM._cmi_check(Z6, np.array([0, 0, 0, 0, 0, 1, 1, 2]), torch.from_numpy(np.stack([R6, Y6], 1)), 2)
    assert c["kind"] == "chain" and c["n"] == 7 and c["k"] == 2 and torch.is_tensor(c["x"]) and c["x"].shape == (8, 5)
    assert np.array_equal(c["x"][:, :3].numpy(), Z6) and np.array_equal(c["x"][:, 3:].numpy(), np.stack([R6, Y6], 1))   # z first
    assert c["joint"]["n"] == c["marginal"]["n"] == 7 and not c["kept"][7]
    assert CM.cmi_class_term([3, 3]) == float(CM.psi_int(3)) and CM.cmi_class_term([150, 7]) == CM.cmi_class_term([7, 150])
    # the closing formula is the restated one
    z, y, cc, I, rho2, nzc, nyc, nc = CC.real_case(*CC.SIZES[0])
    n, k = CC.SIZES[0][0], CC.SIZES[0][4]
    sums = [math.fsum(MC.psi_int(v + 1)) for v in (nzc, nyc, nc)]
    assert float(CM.cmi_close(n, k, sums[2] / np.float64(n), sums[0], sums[1])) == I


def test_label_y_under_an_index_map_takes_its_classes_from_the_mapped_labels():
    """the host side of the chain-rule null: k_i, the class sizes and the dropped rows are those of y[map], as ross has them"""
    from scrubvae_amd.eval import conditional_mi as CM
    from scrubvae_amd.eval.mutual_info import mi_class_terms
    z, lab, c, maps = CC.chain_case()
    k, n = CC.CHAIN_K, len(lab)
    checked = CM._cmi_check(z, lab, c, k)
    assert checked["kind"] == "chain" and checked["n"] == n
    run = object.__new__(CM._ChainRun)       # no device: only the host side is used
    run.c, run.k = checked, k
    for m, index in enumerate(maps):
        keep, mapped, kk, count = run._pairing(index)
        I, rho2, nz, ki, ci, kept = CC.ross(c[:, None], lab[index], k)
        assert np.array_equal(keep, kept) and np.array_equal(kk, ki) and kk.dtype == mapped.dtype == np.int32
        assert np.array_equal(np.unique(mapped, return_counts=True)[1], count) and count.sum() == keep.sum() and (count > 1).all()
        assert np.array_equal(count[np.unique(mapped, return_inverse=True)[1].reshape(-1)], ci)
        assert (mapped[:, None] == mapped[None, :]).tolist() == (lab[index][keep][:, None] == lab[index][keep][None, :]).tolist()
        if m < 2:                            # a true permutation leaves what the observed pairing has
            assert keep.all() and np.array_equal(kk, checked["joint"]["kk"][index])
            assert mi_class_terms(count, k) == mi_class_terms(checked["joint"]["count"], k)
    keep, mapped, kk, count = run._pairing(maps[3])
    assert keep.sum() == n - 1 and sorted(count) == [4, 70, 128] and set(kk[mapped == mapped[kk == 3][0]]) == {3}
    for bad in (np.zeros(n, np.int64), np.where(np.arange(n) < 1, np.flatnonzero(lab == 2)[0], np.flatnonzero(lab == -3)[0])):
        with pytest.raises(ValueError):      # one class; two classes of which one is a single row: neither is an estimate
            run._pairing(bad)
    assert 1 <= CM._local_chunk(2 ** 19, 64) * 2 ** 19 * 64 <= CM._CMI_SCAN and CM._local_chunk(20000, 8) == 64
    assert CM._local_chunk(2 ** 19, 2) == 32 and CM._local_chunk(1, 1) == 64


def test_new_exports_have_signatures():
    from scrubvae_amd import _lib
    from scrubvae_amd.eval import conditional_mi as CM
    lib = _lib.lib()
    fake, E, K = 4096, _lib.ERR_ARG, _lib.MI_MAX_K

    def radius(Z=fake, ld=3, d=3, n=40, Y=fake, q=2, C=fake, p=2, clab=None, k=3, w=fake, rho2=fake):
        return lib.svae_cmi_radius(Z, ld, d, n, Y, q, C, p, clab, k, w, rho2, None)

    for bad, text in ((dict(k=0), "neighbour count"), (dict(k=K + 1), "neighbour count"), (dict(k=40), "neighbour count"),
                      (dict(q=_lib.MI_MAX_Y + 1), "width of y"), (dict(q=0), "width of y"), (dict(p=_lib.CMI_MAX_C + 1), "width of c"),
                      (dict(p=0), "width of c"), (dict(clab=fake), "exactly one"), (dict(C=None), "exactly one"), (dict(Y=None), "null"),
                      (dict(w=None), "null"), (dict(rho2=None), "null"), (dict(n=1), "bad rows"), (dict(Z=None), "bad rows"),
                      (dict(ld=2), "bad rows"), (dict(d=0), "bad rows")):
        assert radius(**bad) == E and text in _lib.last_error(), (bad, _lib.last_error())
    assert radius(w=fake + 4) == _lib.ERR_ALIGN

    def counts(Z=fake, ld=3, d=3, n=40, Y=fake, q=2, C=fake, p=2, clab=None, rho2=fake, nzc=fake, nyc=fake, nc=fake):
        return lib.svae_cmi_counts(Z, ld, d, n, Y, q, C, p, clab, rho2, nzc, nyc, nc, None)

    for bad in (dict(n=1), dict(d=0), dict(ld=2), dict(Z=None), dict(Y=None), dict(q=0), dict(q=5), dict(p=0), dict(p=5), dict(C=None),
                dict(clab=fake), dict(C=None, clab=fake), dict(nc=None), dict(rho2=None), dict(nzc=None), dict(nyc=None)):
        assert counts(**bad) == E, bad
    assert "nc belongs" in (counts(C=None, clab=fake) and _lib.last_error())     # nc given with clab

    def draw(nbr=fake, n=10, kp=4, order=fake, scan=fake, P=3, out=fake):
        return lib.svae_local_permutations(nbr, n, kp, order, scan, P, out, None)

    for bad in (dict(nbr=None), dict(order=None), dict(scan=None), dict(out=None), dict(n=0), dict(n=2 ** 19 + 1), dict(kp=0),
                dict(kp=_lib.CMI_MAX_DONORS + 1), dict(P=0), dict(P=_lib.MMD_NULL_MAX + 1)):
        assert draw(**bad) == E, bad
    import scrubvae_amd.eval as EV
    for name in ("conditional_mutual_information", "conditional_permutations", "conditional_mutual_information_permutation_test"):
        assert getattr(EV, name) is getattr(CM, name)
    assert _lib.CMI_MAX_C == CC.MAX_C == 4 and _lib.CMI_MAX_DONORS == CC.MAX_DONORS == 64
    assert CM._CMI_CALLS.keys() >= {"radius", "counts", "psi_sums"}
    from scrubvae_amd.eval import mutual_info as MI
    assert MI._MI_CALLS.keys() == {"radius", "counts", "psi_sums"} and CM.MIPermutationResult is MI.MIPermutationResult


def test_conditional_mutual_information_needs_the_built_library(monkeypatch, tmp_path):
    """no fallback: without the library the estimate fails at its first load, it does not compute on the host"""
    from scrubvae_amd import _lib
    from scrubvae_amd.eval import conditional_mi as CM
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "libscrubvae_hip.so"))
    with pytest.raises(RuntimeError, match="not found"):
        CM._CmiRun(CM._cmi_check(Z6, Y6, R6, 2), torch.device("cpu"))
