"""conditional_mutual_information / conditional_permutations / conditional_mutual_information_permutation_test (csrc/mi.hip) on the
device against the numpy restatement of tests/cmi_checks.py.

Every kernel output is an integer or one order statistic, so rho2 is held to equal bytes and nzc, nyc, nc to exact equality, and the
local permutation draw to exact equality with the plain Python loop; only the estimate itself, which passes through a log and three
floating-point means, is held to cmi_checks.cmi_gate.  The sizes are those of test_gpu_mi.py: partial row and column tiles, a
partial feature chunk, rows not resident in LDS, k at its maximum and at n - 1, several column chunks per row tile."""
import numpy as np
import pytest
import torch

from tests import cmi_checks as CC
from tests import mi_checks as MC

pytestmark = pytest.mark.gpu

OBSERVED = {"worst": 0.0}   # the largest |I_device - I_restated| / cmi_gate(n) seen by this run


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def within_gate(got, want, n, what):
    ratio = abs(got - want) / CC.cmi_gate(n)
    OBSERVED["worst"] = max(OBSERVED["worst"], ratio)
    print(f"{what}: device {got!r}, restated {want!r}, apart {abs(got - want) / 2.0 ** -53:.2f} x 2^-53 = {ratio:.3f} of the gate"
          f" (largest so far {OBSERVED['worst']:.3f})")
    assert ratio <= 1.0


def check_real(z, y, c, k, want, what):
    from scrubvae_amd.eval import conditional_mutual_information
    I, rho2, nzc, nyc, nc = want
    got, parts = conditional_mutual_information(z, y, c, n_neighbors=k, return_parts=True)
    assert isinstance(got, float) and parts["rho2"].dtype == np.float64
    assert parts["nzc"].dtype == parts["nyc"].dtype == parts["nc"].dtype == np.int32
    assert bits(parts["rho2"]) == bits(rho2), int(np.argmax(parts["rho2"] != rho2))
    assert np.array_equal(parts["nzc"], nzc) and np.array_equal(parts["nyc"], nyc) and np.array_equal(parts["nc"], nc)
    assert parts["kept"].all()
    within_gate(got, I, len(z), what)
    return got, parts


@pytest.mark.parametrize("n,d,q,p,k", CC.SIZES)
def test_equal_to_the_restatement(n, d, q, p, k):
    z, y, c, *want = CC.real_case(n, d, q, p, k)
    check_real(z, y if q > 1 else y[:, 0], c if p > 1 else c[:, 0], k, want, f"n={n} d={d} q={q} p={p} k={k}")


def test_two_rows():
    z, y, c = np.array([[0.0, 0.0], [3.0, 4.0]]), np.array([0.0, 1.0]), np.array([0.0, 2.0])
    got, parts = check_real(z, y, c, 1, CC.cmi_real(z, y, c, 1), "two rows")
    assert np.array_equal(parts["rho2"], [25.0, 25.0])                     # max(25, 1, 4)
    assert np.array_equal(parts["nzc"], [0, 0]) and np.array_equal(parts["nyc"], [1, 1]) and np.array_equal(parts["nc"], [1, 1])


def test_constant_c_gives_the_parts_of_mutual_information():
    from scrubvae_amd.eval import conditional_mutual_information, mutual_information
    for (n, d, q, k), c in ((MC.SIZES[0], np.full(301, 3.25)), (MC.SIZES[5], np.zeros((1037, 4)))):
        z, y = MC.real_case(n, d, q, k)[:2]
        _, mine = conditional_mutual_information(z, y, c, n_neighbors=k, return_parts=True)
        _, theirs = mutual_information(z, y, n_neighbors=k, return_parts=True)
        assert bits(mine["rho2"]) == bits(theirs["rho2"]) and bits(mine["nzc"]) == bits(theirs["nz"]) and bits(mine["nyc"]) == bits(theirs["ny"])
        assert (mine["nc"] == n - 1).all()


def test_label_c_drops_small_classes():
    from scrubvae_amd.eval import conditional_mutual_information
    z, y, lab, I, rho2, nzc, nyc, kept = CC.label_case()
    k = CC.LABEL_K
    got, parts = conditional_mutual_information(z, y, lab, n_neighbors=k, return_parts=True)
    assert np.array_equal(parts["kept"], kept) and kept.sum() == 302 == len(parts["nzc"])
    assert bits(parts["rho2"]) == bits(rho2) and np.array_equal(parts["nzc"], nzc) and np.array_equal(parts["nyc"], nyc)
    size = np.unique(lab, return_counts=True)[1][np.unique(lab, return_inverse=True)[1]]
    assert np.array_equal(parts["nc"] + 1, size[kept]) and parts["nc"].dtype == np.int32
    within_gate(got, I, int(kept.sum()), "label c")
    # renumbering the labels changes nothing, whatever it does to their order
    for other in (50 - 3 * lab, torch.from_numpy(lab.copy()).cuda() + 7):
        again, p2 = conditional_mutual_information(z, y, other, n_neighbors=k, return_parts=True)
        assert again == got and all(bits(p2[key]) == bits(parts[key]) for key in parts)


def test_ties_and_duplicates():
    z, y, c, *want = CC.grid_case()
    rho2, nzc, nyc, nc = want[1:]
    assert (rho2 == 0).any() and (rho2 > 0).any() and not (nzc[rho2 == 0].any() or nyc[rho2 == 0].any() or nc[rho2 == 0].any())
    check_real(z, y, c, CC.GRID_K, want, "grid")


def test_views_give_the_bits_of_the_contiguous_copy():
    from scrubvae_amd.eval import conditional_mutual_information
    n, d, q, p, k = CC.SIZES[1]
    z, y, c, *want = CC.real_case(n, d, q, p, k)
    got, parts = check_real(z, y, c, k, want, "contiguous")
    wide, wide_c = np.zeros((n, 2 * d)), np.zeros((n, 2 * p))
    wide[:, ::2], wide_c[:, ::2] = z, c
    for zv, cv in ((wide[:, ::2], wide_c[:, ::2]), (torch.from_numpy(wide).cuda()[:, ::2], torch.from_numpy(wide_c).cuda()[:, ::2]),
                   (z.astype(np.float32), c.astype(np.float32)), (torch.from_numpy(z.copy()).cuda(), c)):
        a, pv = conditional_mutual_information(zv, y, cv, n_neighbors=k, return_parts=True)
        assert a == got and all(bits(pv[key]) == bits(parts[key]) for key in parts)


def test_two_calls_give_the_same_bits():
    from scrubvae_amd.eval import conditional_mutual_information
    for size in (CC.SIZES[0], CC.SIZES[5]):
        z, y, c = CC.real_case(*size)[:3]
        a, b = (conditional_mutual_information(z, y, c, n_neighbors=size[4], return_parts=True) for _ in range(2))
        assert bits(np.float64(a[0])) == bits(np.float64(b[0])) and all(bits(a[1][key]) == bits(b[1][key]) for key in a[1])
    z, y, lab = CC.label_case()[:3]
    assert conditional_mutual_information(z, y, lab, n_neighbors=5) == conditional_mutual_information(z, y, lab, n_neighbors=5)


def test_chain_rule_for_label_y():
    from scrubvae_amd.eval import conditional_mutual_information, mutual_information
    z, lab = MC.label_case()[:2]
    c = np.random.default_rng(4).normal(size=(len(z), 2)) + 0.3 * (lab[:, None] % 3)
    k = MC.LABEL_CASE[2]
    got, parts = conditional_mutual_information(z, lab, c, n_neighbors=k, return_parts=True)
    joint, marginal = mutual_information(np.hstack([z, c]), lab, n_neighbors=k), mutual_information(c, lab, n_neighbors=k)
    assert bits(np.float64(got)) == bits(np.float64(joint - marginal)) and parts["joint"] == joint and parts["marginal"] == marginal
    assert np.array_equal(parts["kept"], MC.label_case()[7])
    assert conditional_mutual_information(torch.from_numpy(z.copy()).cuda(), lab, c, n_neighbors=k) == got
    with pytest.raises(ValueError):
        conditional_mutual_information(z, lab, lab, n_neighbors=k)


def device_draw(nbr, order, scan):
    from scrubvae_amd.eval import conditional_mi as CM
    return CM._local_draw(*(torch.from_numpy(a).cuda() for a in (nbr, order, scan))).cpu().numpy()


@pytest.mark.parametrize("n,kp,P", CC.DRAWS)
def test_local_permutations_against_the_loop(n, kp, P):
    nbr, order, scan = CC.draw_inputs(n, kp, P, seed=n + kp)
    assert np.array_equal(device_draw(nbr, order, scan), CC.local_permutation(nbr, order, scan))


def test_local_permutations_with_exhausted_donors():
    n, kp, P = 301, 2, 3
    values = np.random.default_rng(8).integers(0, 10, n).astype(np.float64)      # ten distinct values of c
    nbr, order, scan = CC.draw_inputs(n, kp, P, seed=12, values=values)
    want = CC.local_permutation(nbr, order, scan)
    assert any(len(np.unique(row)) < n for row in want)                           # at least one donor repeats
    assert np.array_equal(device_draw(nbr, order, scan), want)


def test_conditional_permutations_of_labels():
    from scrubvae_amd.eval import conditional_permutations
    lab = CC.label_case()[2]
    perms = conditional_permutations(lab, 7, seed=3)
    assert perms.is_cuda and perms.dtype == torch.int64 and perms.shape == (7, len(lab))
    got = perms.cpu().numpy()
    assert all(np.array_equal(np.sort(row), np.arange(len(lab))) for row in got) and (lab[got] == lab[None, :]).all()
    assert len({bits(row) for row in got}) == 7 and not np.array_equal(got[0], np.arange(len(lab)))
    assert torch.equal(perms, conditional_permutations(torch.from_numpy(lab.copy()).cuda(), 7, seed=3, n_donors=999))


def test_conditional_permutations_of_a_real_c():
    from scrubvae_amd.eval import conditional_mi as CM
    from scrubvae_amd.eval import conditional_permutations, kneighbors
    n, P, donors, seed = 301, 70, 8, 5          # two launches of the draw
    c = np.random.default_rng(2).normal(size=(n, 2))
    before = CM._CMI_CALLS["local_permutations"]
    perms = conditional_permutations(c, P, n_donors=donors, seed=seed)
    assert CM._CMI_CALLS["local_permutations"] == before + 2
    assert perms.is_cuda and perms.dtype == torch.int64 and perms.shape == (P, n)
    nbr = np.concatenate([np.arange(n)[:, None], kneighbors(c, donors - 1, return_distance=False)], axis=1)
    order, scan_of = CM._local_inputs(n, donors, P, seed, perms.device)
    scan = torch.cat([scan_of(64), scan_of(P - 64)])
    assert scan.dtype == torch.uint8 and (scan.sort(dim=2).values == torch.arange(donors, device=scan.device, dtype=torch.uint8)).all()
    want = CC.local_permutation(nbr, order.cpu().numpy(), scan.cpu().numpy())
    assert np.array_equal(perms.cpu().numpy(), want)
    assert torch.equal(perms, conditional_permutations(torch.from_numpy(c).cuda(), P, n_donors=donors, seed=seed, device="cuda"))


def test_permutation_test():
    from scrubvae_amd.eval import MIPermutationResult, conditional_mutual_information, conditional_mutual_information_permutation_test
    from scrubvae_amd.eval import conditional_mi as CM
    from scrubvae_amd.eval import mutual_info as MI
    n, d, q, p, k, P = CC.PERM_CASE
    z, y, c, maps = CC.perm_case()
    assert len(np.unique(maps[-1])) < n          # the last row repeats rows
    before, before_mi = dict(CM._CMI_CALLS), dict(MI._MI_CALLS)
    r = conditional_mutual_information_permutation_test(z, y, c, n_neighbors=k, permutations=maps)
    assert all(CM._CMI_CALLS[key] == before[key] + P + 1 for key in ("radius", "counts", "psi_sums"))
    assert CM._CMI_CALLS["local_permutations"] == before["local_permutations"] and MI._MI_CALLS == before_mi
    assert isinstance(r, MIPermutationResult) and r.null_distribution.shape == (P,) and r.null_distribution.dtype == np.float64
    stat = conditional_mutual_information(z, y, c, n_neighbors=k)
    assert bits(np.float64(r.statistic)) == bits(np.float64(stat)) == bits(r.null_distribution[0])   # row 0 is the identity
    for m in range(P):
        within_gate(r.null_distribution[m], CC.cmi_real(z, y[maps[m]], c, k)[0], n, f"index map {m}")
    assert r.pvalue == (1 + int((r.null_distribution >= r.statistic).sum())) / (1 + P)
    # a null value depends on its row alone: two calls, and a device tensor of another integer dtype
    a = conditional_mutual_information_permutation_test(z, y, c, n_neighbors=k, permutations=maps[:30])
    b = conditional_mutual_information_permutation_test(torch.from_numpy(z.copy()).cuda(), y, c, n_neighbors=k,
                                                        permutations=torch.from_numpy(maps[30:].astype(np.int32)).cuda())
    assert bits(np.concatenate([a.null_distribution, b.null_distribution])) == bits(r.null_distribution)
    # drawn maps are those of conditional_permutations
    from scrubvae_amd.eval import conditional_permutations
    drawn = conditional_mutual_information_permutation_test(z, y, c, n_neighbors=k, n_permutations=5, seed=3, n_donors=6)
    given = conditional_mutual_information_permutation_test(z, y, c, n_neighbors=k,
                                                            permutations=conditional_permutations(c, 5, n_donors=6, seed=3))
    assert bits(drawn.null_distribution) == bits(given.null_distribution) and drawn.pvalue == given.pvalue
    bad = maps[:3].copy()
    bad[1, 0] = n
    with pytest.raises(ValueError):
        conditional_mutual_information_permutation_test(z, y, c, n_neighbors=k, permutations=torch.from_numpy(bad).cuda())


def test_permutation_test_with_label_c():
    from scrubvae_amd.eval import conditional_mutual_information, conditional_mutual_information_permutation_test, conditional_permutations
    z, y, lab, I, rho2, nzc, nyc, kept = CC.label_case()
    k, n = CC.LABEL_K, int(kept.sum())
    r = conditional_mutual_information_permutation_test(z, y, lab, n_neighbors=k, n_permutations=3, seed=1)
    assert bits(np.float64(r.statistic)) == bits(np.float64(conditional_mutual_information(z, y, lab, n_neighbors=k)))
    zk, yk, lk = z[kept], y[kept], lab[kept]
    maps = conditional_permutations(lk, 3, seed=1).cpu().numpy()       # n counts the kept rows
    assert maps.shape == (3, n)
    for m in range(3):
        within_gate(r.null_distribution[m], CC.cmi_strat(zk, yk[maps[m]], lk, k)[0], n, f"label c, permutation {m}")
    ident = conditional_mutual_information_permutation_test(z, y, lab, n_neighbors=k, permutations=np.arange(n)[None, :])
    assert bits(ident.null_distribution[0]) == bits(np.float64(ident.statistic)) and ident.pvalue == 1.0


def test_permutation_test_with_label_y():
    """under an index map that repeats rows the class sizes, k_i and the dropped labels are those of y[map]"""
    from scrubvae_amd.eval import conditional_mutual_information, conditional_mutual_information_permutation_test, conditional_permutations
    z, lab, c, maps = CC.chain_case()
    k, n = CC.CHAIN_K, len(lab)
    sizes = lambda m: sorted(np.unique(lab[m], return_counts=True)[1])
    assert sizes(maps[1]) == sizes(maps[0]) and all(sizes(m) != sizes(maps[0]) for m in maps[2:])
    assert sizes(maps[3])[:2] == [1, 4] and 4 <= k      # one class is left a single row, another at most k rows
    r = conditional_mutual_information_permutation_test(z, lab, c, n_neighbors=k, permutations=maps)
    stat = conditional_mutual_information(z, lab, c, n_neighbors=k)
    assert bits(np.float64(r.statistic)) == bits(np.float64(stat)) == bits(r.null_distribution[0])   # row 0 is the identity
    for m, index in enumerate(maps):
        want, kept = CC.cmi_chain(z, lab[index], c, k)
        assert kept.sum() == n - 1 if m == 3 else kept.all() or m == 2
        within_gate(r.null_distribution[m], want, int(kept.sum()), f"label y, index map {m}")
        # and it is the plain estimate of the mapped labels, to the bit
        assert bits(r.null_distribution[m]) == bits(np.float64(conditional_mutual_information(z, lab[index], c, n_neighbors=k)))
    assert r.pvalue == (1 + int((r.null_distribution >= r.statistic).sum())) / (1 + len(maps))
    # a null value depends on its row alone
    again = conditional_mutual_information_permutation_test(z, lab, torch.from_numpy(c.copy()).cuda(), n_neighbors=k,
                                                            permutations=torch.from_numpy(maps[[3, 5, 2]]).cuda())
    assert bits(again.null_distribution) == bits(r.null_distribution[[3, 5, 2]])
    # drawn local maps repeat donors, and are held to the same restatement
    drawn = conditional_permutations(c, 3, n_donors=8, seed=2).cpu().numpy()
    assert any(len(np.unique(row)) < n for row in drawn)
    d = conditional_mutual_information_permutation_test(z, lab, c, n_neighbors=k, n_permutations=3, n_donors=8, seed=2)
    for m, index in enumerate(drawn):
        want, kept = CC.cmi_chain(z, lab[index], c, k)
        within_gate(d.null_distribution[m], want, int(kept.sum()), f"label y, drawn map {m}")
    with pytest.raises(ValueError):      # every row receives the label of row 0: one class is no estimate
        conditional_mutual_information_permutation_test(z, lab, c, n_neighbors=k, permutations=np.zeros((1, n), np.int64))


@pytest.mark.parametrize("direct", [True, False])
def test_sanity_pair(direct):
    """the outcomes that test_cmi_cpu.py decides on the restatement"""
    from scrubvae_amd.eval import conditional_mutual_information_permutation_test, mutual_information
    n, k, P, donors = CC.SANITY
    z, y, y2, c = CC.sanity_case()
    r = conditional_mutual_information_permutation_test(z, y2 if direct else y, c, n_neighbors=k, n_donors=donors, n_permutations=P, seed=0)
    print(f"direct={direct}: statistic {r.statistic:.4f}, null in [{r.null_distribution.min():.4f}, {r.null_distribution.max():.4f}]")
    if direct:
        assert r.pvalue == 1 / 20
    else:
        assert abs(r.statistic) <= 0.05 and mutual_information(z, y, n_neighbors=k) >= 0.5


def test_argument_errors_launch_nothing():
    from scrubvae_amd import _lib, ops
    lib, st, E = _lib.lib(), ops._stream(), _lib.ERR_ARG
    n, d = 40, 3
    Z = torch.zeros(n, d, dtype=torch.float64, device="cuda")
    Y, C = (torch.zeros(n, 4, dtype=torch.float64, device="cuda") for _ in range(2))
    lab = torch.ones(n, dtype=torch.int32, device="cuda")
    work = torch.zeros((lib.svae_mi_work(n, 32) + 7) // 8, dtype=torch.int64, device="cuda")
    rho2 = torch.full((n,), -1.0, dtype=torch.float64, device="cuda")
    cnt = torch.full((3, n), -7, dtype=torch.int32, device="cuda")

    def radius(k=3, q=2, p=2, Y=Y, C=C, lab=None, w=work, n=n):
        return lib.svae_cmi_radius(Z.data_ptr(), d, d, n, ops._p(Y), q, ops._p(C), p, ops._p(lab), k, ops._p(w), rho2.data_ptr(), st)

    def counts(q=2, p=2, C=C, lab=None, nc=cnt[2], r=rho2):
        return lib.svae_cmi_counts(Z.data_ptr(), d, d, n, Y.data_ptr(), q, ops._p(C), p, ops._p(lab), ops._p(r), cnt[0].data_ptr(),
                                   cnt[1].data_ptr(), ops._p(nc), st)

    for bad, text in ((dict(k=0), "neighbour count"), (dict(k=33), "neighbour count"), (dict(k=30, n=30), "neighbour count"),
                      (dict(q=5), "at most 4"), (dict(p=5), "at most 4"), (dict(lab=lab), "exactly one"), (dict(C=None), "exactly one"),
                      (dict(Y=None), "null"), (dict(w=None), "null")):
        assert radius(**bad) == E and text in _lib.last_error(), (bad, _lib.last_error())
    for bad, text in ((dict(q=0), "width of y"), (dict(p=0), "width of c"), (dict(lab=lab), "exactly one"), (dict(C=None), "exactly one"),
                      (dict(C=None, lab=lab), "nc belongs"), (dict(nc=None), "nc belongs"), (dict(r=None), "null")):
        assert counts(**bad) == E and text in _lib.last_error(), (bad, _lib.last_error())
    nbr = torch.zeros(n, 4, dtype=torch.int32, device="cuda")
    order = torch.arange(n, dtype=torch.int32, device="cuda").view(1, n)
    scan = torch.zeros(1, n, 4, dtype=torch.uint8, device="cuda")
    out = torch.full((1, n), -7, dtype=torch.int32, device="cuda")
    for kp, rows, P in ((0, n, 1), (65, n, 1), (4, 0, 1), (4, 2 ** 19 + 1, 1), (4, n, 0), (4, n, 65537)):
        assert lib.svae_local_permutations(nbr.data_ptr(), rows, kp, order.data_ptr(), scan.data_ptr(), P, out.data_ptr(), st) == E
    torch.cuda.synchronize()
    assert (rho2 == -1.0).all() and (work == 0).all() and (cnt == -7).all() and (out == -7).all()    # nothing was launched
    assert radius() == 0 and counts() == 0 and radius(C=None, lab=lab) == 0 and counts(C=None, lab=lab, nc=None) == 0
    torch.cuda.synchronize()
    assert (rho2 == 0.0).all() and (cnt[:2] == 0).all()        # 40 equal rows: every radius is 0 and nothing is below it
