"""mutual_information / mutual_information_permutation_test / latent_mi_scores (csrc/mi.hip) on the device against the numpy
restatement of tests/mi_checks.py.

Every kernel output is an integer or one order statistic, so rho2 is held to equal bytes and nz, ny to exact equality, with no
tolerance; only the estimate itself, which passes through a log and two floating-point means, is held to mi_checks.mi_gate.  The
sizes are the smallest that reach each path of the kernels: partial row and column tiles, a partial feature chunk, rows not
resident in LDS, k at its maximum and at n - 1, several column chunks per row tile, per-row k with labels, exact ties and
duplicate rows."""
import numpy as np
import pytest
import torch

from tests import mi_checks as MC

pytestmark = pytest.mark.gpu

OBSERVED = {"worst": 0.0}   # the largest |I_device - I_restated| / mi_gate(n) seen by this run


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def within_gate(got, want, n, what):
    ratio = abs(got - want) / MC.mi_gate(n)
    OBSERVED["worst"] = max(OBSERVED["worst"], ratio)
    print(f"{what}: device {got!r}, restated {want!r}, apart {abs(got - want) / 2.0 ** -53:.2f} x 2^-53 = {ratio:.3f} of the gate"
          f" (largest so far {OBSERVED['worst']:.3f})")
    assert ratio <= 1.0


def check_real(z, y, k, want, what):
    from scrubvae_amd.eval import mutual_information
    I, rho2, nz, ny = want
    got, parts = mutual_information(z, y, n_neighbors=k, return_parts=True)
    assert isinstance(got, float) and parts["rho2"].dtype == np.float64 and parts["nz"].dtype == parts["ny"].dtype == np.int32
    assert bits(parts["rho2"]) == bits(rho2), int(np.argmax(parts["rho2"] != rho2))
    assert np.array_equal(parts["nz"], nz) and np.array_equal(parts["ny"], ny) and parts["kept"].all()
    within_gate(got, I, len(z), what)
    return got, parts


def check_labels(z, lab, k, want, what):
    from scrubvae_amd.eval import mutual_information
    I, rho2, nz, ki, c, kept = want
    got, parts = mutual_information(z, lab, n_neighbors=k, return_parts=True)
    assert bits(parts["rho2"]) == bits(rho2) and np.array_equal(parts["nz"], nz) and "ny" not in parts
    assert np.array_equal(parts["k"], ki) and np.array_equal(parts["count"], c) and np.array_equal(parts["kept"], kept)
    within_gate(got, I, int(kept.sum()), what)
    return got, parts


@pytest.mark.parametrize("n,d,q,k", MC.SIZES)
def test_equal_to_the_restatement(n, d, q, k):
    z, y, *want = MC.real_case(n, d, q, k)
    check_real(z, y if q > 1 else y[:, 0], k, want, f"n={n} d={d} q={q} k={k}")


def test_two_rows():
    z, y = np.array([[0.0, 0.0], [3.0, 4.0]]), np.array([0.0, 1.0])
    got, parts = check_real(z, y, 1, MC.ksg(z, y, 1), "two rows")
    assert np.array_equal(parts["rho2"], [25.0, 25.0]) and np.array_equal(parts["nz"], [0, 0]) and np.array_equal(parts["ny"], [1, 1])


def test_column_chunks():
    from scrubvae_amd import _lib
    work = _lib.lib().svae_mi_work
    assert [work(n, k) // (-(-n // 64) * 64 * k * 12) for n, k in ((30, 29), (301, 3), (1037, 10))] == [1, 5, 6]


def test_labels_with_per_row_k_and_single_labels():
    z, lab, *want = MC.label_case()
    got, parts = check_labels(z, lab, MC.LABEL_CASE[2], want, "labels")
    assert parts["kept"].sum() == MC.LABEL_CASE[0] == len(parts["nz"]) and set(parts["k"]) == {5, 2, 1}
    # renumbering the labels changes nothing, whatever it does to their order
    for other in (50 - 3 * lab, (lab * lab) % 1009, torch.from_numpy(lab.copy()).cuda() + 7):
        again, p2 = check_labels(z, other, MC.LABEL_CASE[2], want, "labels renumbered")
        assert again == got and all(bits(p2[key]) == bits(parts[key]) for key in parts)


@pytest.mark.parametrize("labels", [False, True])
def test_ties_and_duplicates(labels):
    z, y, *want = MC.grid_case(labels)
    rho2, nz = want[1], want[2]
    assert (rho2 == 0).any() and (rho2 > 0).any() and (nz[rho2 == 0] == 0).all()   # a zero radius counts nothing
    if labels:
        check_labels(z, y, MC.GRID_K, want, "grid labels")
    else:
        check_real(z, y, MC.GRID_K, want, "grid real")


def test_constant_y_gives_the_knn_distances():
    """the walk with the key max(s, s^y) against the walk of the neighbour search: 5 partial row and column tiles, 5 column chunks,
    so both merges run (decided on the restatements in test_mi_cpu.py)"""
    from tests import knn_checks as KC
    from scrubvae_amd.eval import kneighbors, mutual_information
    x = KC.case(301, 3, 5)[0]
    _, parts = mutual_information(x, np.zeros((301, 1)), n_neighbors=5, return_parts=True)
    assert bits(np.sqrt(parts["rho2"])) == bits(kneighbors(x, 5)[0][:, 4])


def test_one_class_gives_the_knn_distances():
    """the walk that admits the row's own label, with every label equal: rows not resident in LDS, 3 column chunks.  One class is
    no estimate, so mutual_information refuses it: the checked arguments are written out here"""
    from tests import knn_checks as KC
    from scrubvae_amd.eval import kneighbors
    from scrubvae_amd.eval import mutual_info as MI
    n, d, k = 131, 128, 7
    x = KC.case(n, d, k)[0]
    dev = torch.device("cuda", torch.cuda.current_device())
    run = MI._MiRun(MC.one_class_arguments(x, k), dev)
    run.run(torch.zeros(2, dtype=torch.float64, device=dev))
    assert bits(np.sqrt(run.parts()["rho2"])) == bits(kneighbors(x, k)[0][:, k - 1])


def test_views_give_the_bits_of_the_contiguous_copy():
    from scrubvae_amd import _lib, ops
    from scrubvae_amd.eval import mutual_information
    n, d, q, k = MC.SIZES[0]
    z, y, *want = MC.real_case(n, d, q, k)
    got, parts = check_real(z, y, k, want, "contiguous")
    wide = np.zeros((n, 2 * d))
    wide[:, ::2] = z
    for view in (wide[:, ::2], torch.from_numpy(wide).cuda()[:, ::2], z.astype(np.float32), torch.from_numpy(z.copy()).cuda()):
        a, p = mutual_information(view, y, n_neighbors=k, return_parts=True)
        assert a == got and all(bits(p[key]) == bits(parts[key]) for key in parts)
    # the C ABI on strided rows: ld > d, and a column view (d = 1, ld = 6)
    lib, st = _lib.lib(), ops._stream()
    six = np.random.default_rng(6).normal(size=(n, 6))
    Z6 = torch.from_numpy(six).cuda()
    Y = torch.from_numpy(y.copy()).cuda()

    def run(Z, offset, ld, dd):
        work = torch.empty((lib.svae_mi_work(n, k) + 7) // 8, dtype=torch.int64, device="cuda")
        rho2 = torch.empty(n, dtype=torch.float64, device="cuda")
        nz, ny = (torch.full((n,), -7, dtype=torch.int32, device="cuda") for _ in range(2))
        out = torch.zeros(2, dtype=torch.float64, device="cuda")
        zp = Z.data_ptr() + 8 * offset
        _lib.check(lib.svae_mi_radius(zp, ld, dd, n, Y.data_ptr(), q, None, None, k, work.data_ptr(), rho2.data_ptr(), st), "mi_radius")
        _lib.check(lib.svae_mi_counts(zp, ld, dd, n, Y.data_ptr(), q, rho2.data_ptr(), nz.data_ptr(), ny.data_ptr(), st), "mi_counts")
        _lib.check(lib.svae_mi_psi_sums(nz.data_ptr(), ny.data_ptr(), n, out.data_ptr(), st), "mi_psi_sums")
        return [t.cpu().numpy() for t in (rho2, nz, ny, out)]

    for offset, dd in ((0, 4), (2, 1), (5, 1)):
        strided = run(Z6, offset, 6, dd)
        copy = run(torch.from_numpy(six[:, offset:offset + dd].copy()).cuda(), 0, dd, dd)
        assert all(bits(a) == bits(b) for a, b in zip(strided, copy))
        want_v = MC.ksg(six[:, offset:offset + dd], y, k)
        assert bits(strided[0]) == bits(want_v[1]) and np.array_equal(strided[1], want_v[2]) and np.array_equal(strided[2], want_v[3])


def test_two_calls_give_the_same_bits():
    from scrubvae_amd.eval import mutual_information
    for n, d, q, k in (MC.SIZES[0], MC.SIZES[5]):
        z, y = MC.real_case(n, d, q, k)[:2]
        a, b = (mutual_information(z, y, n_neighbors=k, return_parts=True) for _ in range(2))
        assert bits(np.float64(a[0])) == bits(np.float64(b[0])) and all(bits(a[1][key]) == bits(b[1][key]) for key in a[1])
        assert mutual_information(z, y, n_neighbors=k) == a[0]
    z, lab = MC.label_case()[:2]
    assert mutual_information(z, lab, n_neighbors=5) == mutual_information(z, lab, n_neighbors=5)


def test_permuted_rows_give_the_permuted_counts():
    from scrubvae_amd.eval import mutual_information
    n, d, q, k = MC.SIZES[0]
    z, y, I, rho2, nz, ny = MC.real_case(n, d, q, k)
    perm = np.random.default_rng(1).permutation(n)
    got, p = mutual_information(z[perm], y[perm], n_neighbors=k, return_parts=True)   # row a of the permuted input is row perm[a]
    assert bits(p["rho2"]) == bits(rho2[perm]) and np.array_equal(p["nz"], nz[perm]) and np.array_equal(p["ny"], ny[perm])
    within_gate(got, I, n, "rows permuted")
    z, lab, I, rho2, nz, ki, c, kept = MC.label_case()
    perm = np.random.default_rng(2).permutation(len(z))
    inv = np.argsort(perm)
    got, p = mutual_information(z[perm], lab[perm], n_neighbors=5, return_parts=True)
    order = inv[np.flatnonzero(kept)]                # where each kept row went
    back = np.argsort(np.argsort(order))             # its position among the kept rows of the permuted input
    assert np.array_equal(p["kept"], kept[perm])
    assert bits(p["rho2"][back]) == bits(rho2) and np.array_equal(p["nz"][back], nz) and np.array_equal(p["k"][back], ki)
    within_gate(got, I, int(kept.sum()), "labelled rows permuted")


def test_permutation_test():
    from scrubvae_amd.eval import MIPermutationResult, mutual_information, mutual_information_permutation_test
    from scrubvae_amd.eval import mutual_info as MI
    n, d, q, k, P = MC.PERM_CASE
    z, y, perms = MC.perm_case()
    before = dict(MI._MI_CALLS)
    r = mutual_information_permutation_test(z, y, n_neighbors=k, permutations=perms)
    assert all(MI._MI_CALLS[key] == before[key] + P + 1 for key in before)      # the three launches per pairing, nothing else
    assert isinstance(r, MIPermutationResult) and r.null_distribution.shape == (P,) and r.null_distribution.dtype == np.float64
    stat = mutual_information(z, y, n_neighbors=k)
    assert bits(np.float64(r.statistic)) == bits(np.float64(stat)) == bits(r.null_distribution[0])   # row 0 is the identity
    for p in (1, 2, 17, P - 1):
        assert bits(np.float64(mutual_information(z, y[perms[p]], n_neighbors=k))) == bits(r.null_distribution[p])
    within_gate(r.null_distribution[5], MC.ksg(z, y[perms[5]], k)[0], n, "permutation 5")
    assert r.pvalue == (1 + int((r.null_distribution >= r.statistic).sum())) / (1 + P)
    # a null value depends on its permutation row alone: two calls, and a device tensor of another integer dtype
    a = mutual_information_permutation_test(z, y, n_neighbors=k, permutations=perms[:30])
    b = mutual_information_permutation_test(torch.from_numpy(z.copy()).cuda(), y, n_neighbors=k,
                                            permutations=torch.from_numpy(perms[30:].astype(np.int32)).cuda())
    assert bits(np.concatenate([a.null_distribution, b.null_distribution])) == bits(r.null_distribution)
    assert a.statistic == b.statistic == r.statistic
    # drawn permutations are those of mmd_permutations
    from scrubvae_amd.eval import mmd_permutations
    drawn = mutual_information_permutation_test(z, y, n_neighbors=k, n_permutations=5, seed=3)
    given = mutual_information_permutation_test(z, y, n_neighbors=k, permutations=mmd_permutations(n, 5, 3, "cuda"))
    assert bits(drawn.null_distribution) == bits(given.null_distribution) and drawn.pvalue == given.pvalue
    bad = perms[:3].copy()
    bad[1, 0] = bad[1, 1]
    with pytest.raises(ValueError):
        mutual_information_permutation_test(z, y, n_neighbors=k, permutations=bad)


def test_permutation_test_with_labels():
    from scrubvae_amd.eval import mutual_information, mutual_information_permutation_test
    z, lab, I, rho2, nz, ki, c, kept = MC.label_case()
    n, _, k = MC.LABEL_CASE
    g = np.random.default_rng(9)
    perms = np.stack([np.arange(n)] + [g.permutation(n) for _ in range(3)])
    r = mutual_information_permutation_test(z, lab, n_neighbors=k, permutations=perms)
    assert bits(np.float64(r.statistic)) == bits(np.float64(mutual_information(z, lab, n_neighbors=k))) == bits(r.null_distribution[0])
    zk, lk = z[kept], lab[kept]
    for p in (1, 3):        # k_i and c_i follow the label
        assert bits(np.float64(mutual_information(zk, lk[perms[p]], n_neighbors=k))) == bits(r.null_distribution[p])
        within_gate(r.null_distribution[p], MC.ross(zk, lk[perms[p]], k)[0], n, f"labels, permutation {p}")


@pytest.mark.parametrize("dependent", [True, False])
def test_sanity_pair(dependent):
    """the outcomes that test_mi_cpu.test_sanity_pair_on_the_restatement decides on the restatement"""
    from scrubvae_amd.eval import mutual_information_permutation_test
    n, d, k, P = MC.SANITY
    z, y, perms = MC.sanity_case(dependent)
    r = mutual_information_permutation_test(z, y, n_neighbors=k, permutations=perms)
    print(f"dependent={dependent}: statistic {r.statistic:.4f}, null in [{r.null_distribution.min():.4f}, {r.null_distribution.max():.4f}]")
    if dependent:
        assert r.pvalue == 1 / (P + 1) and r.statistic > 0.3
    else:
        assert r.null_distribution.min() < r.statistic < r.null_distribution.max()


@pytest.mark.parametrize("discrete", [False, True])
def test_latent_scores(discrete):
    from scrubvae_amd.eval import latent_mi_scores
    n, d, k = MC.SCORES[0]
    z, y, lab = MC.scores_rows(n, d, seed=n)
    target = lab if discrete else y
    want = MC.latent_scores(z, target, discrete, k, 0)
    got = latent_mi_scores(z, target, discrete_target=discrete, n_neighbors=k, random_state=0)
    assert got.shape == (d,) and got.dtype == np.float64 and (got >= 0).all() and got[0] > 0.3
    for col in range(d):
        within_gate(got[col], want[col], n, f"discrete={discrete} column {col}")
    again = latent_mi_scores(torch.from_numpy(z).cuda().float().double(), torch.from_numpy(target).cuda(), discrete_target=discrete,
                             n_neighbors=k, random_state=0)
    assert bits(again) == bits(latent_mi_scores(z.astype(np.float32), target, discrete_target=discrete, n_neighbors=k, random_state=0))


def test_argument_errors_launch_nothing():
    from scrubvae_amd import _lib, ops
    lib, st, E = _lib.lib(), ops._stream(), _lib.ERR_ARG
    n, d, q = 40, 3, 2
    Z = torch.zeros(n, d, dtype=torch.float64, device="cuda")
    Y = torch.zeros(n, 4, dtype=torch.float64, device="cuda")
    lab, kk = (torch.ones(n, dtype=torch.int32, device="cuda") for _ in range(2))
    work = torch.zeros((lib.svae_mi_work(n, 32) + 7) // 8, dtype=torch.int64, device="cuda")
    rho2 = torch.full((n,), -1.0, dtype=torch.float64, device="cuda")

    def radius(k=3, q=q, Y=Y, lab=None, kk=None, w=work, n=n):
        return lib.svae_mi_radius(Z.data_ptr(), d, d, n, ops._p(Y), q, ops._p(lab), ops._p(kk), k, ops._p(w), rho2.data_ptr(), st)

    for bad, text in ((dict(k=0), "neighbour count"), (dict(k=33), "neighbour count"), (dict(k=30, n=30), "neighbour count"),
                      (dict(q=5), "at most 4"), (dict(lab=lab, kk=kk), "exactly one"), (dict(Y=None), "exactly one"),
                      (dict(w=None), "null")):
        assert radius(**bad) == E and text in _lib.last_error(), (bad, _lib.last_error())
    torch.cuda.synchronize()
    assert (rho2 == -1.0).all() and (work == 0).all()    # nothing was launched
    assert radius() == 0 and radius(Y=None, lab=lab, kk=kk) == 0
    torch.cuda.synchronize()
    assert (rho2 == 0.0).all()                           # 40 equal rows: every radius is 0
