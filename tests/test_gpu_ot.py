"""svae_ot_softmin / svae_ot_apply (csrc/ot.hip) and sinkhorn / sinkhorn_divergence / transport_flow on the device against the numpy
restatement of tests/ot_checks.py.

Every L, cbar and applied value is held to the single-pass gates derived in ot_checks' docstring (truth in np.longdouble from the
same offsets), a whole solve with a fixed schedule to the gate its long-double run accumulates; the sizes are the smallest that
reach each path of the kernels: one row and one candidate, a last tile with one candidate, partial row tiles and feature chunks,
several column chunks and their merge, rows not resident in LDS, the 16-, 64- and 128-column instantiations of apply."""
import warnings

import numpy as np
import pytest
import torch

from tests import ot_checks as OC
from tests.test_gpu_mmd import needs_longdouble

pytestmark = pytest.mark.gpu

FIXED = dict(scaling=0.5, tol=0.0, max_iter=40, check_every=10)   # the schedule of OC.solve_case
COSTS = {0: "sqeuclidean", 1: "euclidean"}


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def sets(q, x, kind):
    from scrubvae_amd.eval import transport as T
    return T._Sets(q, x, np.full(len(q), 1.0 / len(q)), np.full(len(x), 1.0 / len(x)), kind)


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float64)).cuda()


def softmin(S, off, eps, cbar=True):
    with torch.cuda.device(S.dev):
        out = S.softmin(S.X, S.Y, dev(off), eps, cbar)
    return tuple(t.cpu().numpy() for t in out) if cbar else out.cpu().numpy()


@needs_longdouble
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("m,n,d", OC.SIZES)
def test_every_value_within_the_derived_gate(m, n, d, kind):
    q, x, off, eps, _, g = OC.case(m, n, d, kind)
    S = sets(q, x, kind)
    L, cbar = softmin(S, off, eps)
    assert L.shape == cbar.shape == (m,) and L.dtype == np.float64
    eL, ec = OC.err(L, g.truth.L), OC.err(cbar, g.truth.cbar)
    worst = int(np.argmax(eL / g.tol_L))
    print(f"ot softmin m={m} n={n} d={d} kind={kind}: worst device error of L {eL[worst] / OC.EPS:.2f} u (gate {g.tol_L[worst] / OC.EPS:.0f} u),"
          f" largest error / gate L {np.max(eL / g.tol_L):.4f} cbar {np.max(ec / g.tol_cbar):.4f}")
    assert (eL <= g.tol_L).all(), (worst, float(eL[worst] / OC.EPS))
    assert (ec <= g.tol_cbar).all(), int(np.argmax(ec / g.tol_cbar))
    assert bits(softmin(S, off, eps, cbar=False)) == bits(L)   # asking for cbar changes no bit of L


@needs_longdouble
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("c", OC.APPLY_COLS)
@pytest.mark.parametrize("m,n,d", OC.APPLY_SIZES)
def test_every_applied_value_within_the_derived_gate(m, n, d, c, kind):
    q, x, off, eps, C, _ = OC.case(m, n, d, kind)
    S = sets(q, x, kind)
    L = softmin(S, off, eps, cbar=False)
    V = np.random.default_rng(m + c).normal(size=(n, c))
    got = apply_with_offsets(S, off, eps, L, V)
    truth, tol = OC.apply_gate(C, off, eps, L, V)
    e = OC.err(got, truth)
    print(f"ot apply m={m} n={n} d={d} c={c} kind={kind}: largest error / gate {np.max(e / tol):.4f}")
    assert got.shape == (m, c) and (e <= tol).all(), float(np.max(e / tol))


def apply_with_offsets(S, off, eps, L, V):
    """svae_ot_apply with the offsets as given"""
    from scrubvae_amd import ops
    from scrubvae_amd._lib import check
    m, n, c = S.nx, S.ny, V.shape[1]
    offd, Ld, Vd = dev(off), dev(L), dev(V)
    out = torch.empty((m, c), dtype=torch.float64, device=S.dev)
    work = torch.empty(S.lib.svae_ot_apply_work(m, n, c), dtype=torch.float64, device=S.dev)
    check(S.lib.svae_ot_apply(S.X.data_ptr(), S.d, m, S.Y.data_ptr(), S.d, n, S.d, offd.data_ptr(), 1.0 / eps, S.kind, Ld.data_ptr(),
                              Vd.data_ptr(), c, c, work.data_ptr(), out.data_ptr(), c, ops._stream()), "ot_apply")
    return out.cpu().numpy()


@needs_longdouble
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("nx,ny,d", OC.SOLVE_SIZES)
def test_whole_solve_within_the_accumulated_gate(nx, ny, d, kind):
    from scrubvae_amd.eval import sinkhorn, sinkhorn_divergence, transport as T
    X, Y, eps, runs = OC.solve_case(nx, ny, d, kind)
    res = sinkhorn(X, Y, epsilon=eps, cost=COSTS[kind], **FIXED)
    _, truth = runs["xy"]
    a, b = np.full(nx, 1.0 / nx), np.full(ny, 1.0 / ny)
    ef, eg = OC.err(res.f, truth.f).max(), OC.err(res.g, truth.g).max()
    value = float((a * truth.f).sum() + (b * truth.g).sum())
    vgate = OC.value_gate(truth.gate, [(a, truth.f), (b, truth.g)], max(nx, ny))
    print(f"ot solve nx={nx} ny={ny} d={d} kind={kind}: potentials {max(ef, eg) / truth.gate:.4f} of the accumulated gate {truth.gate:.3e}, "
          f"value {abs(res.value - value) / vgate:.4f} of its gate")
    assert res.n_iter == 40 and not res.converged and res.epsilon == eps
    assert ef <= truth.gate and eg <= truth.gate and abs(res.value - value) <= vgate
    # the two self problems: potentials through the solver's own loop, values through sinkhorn_divergence
    div = sinkhorn_divergence(X, Y, epsilon=eps, cost=COSTS[kind], **FIXED)
    assert bits(div.cross.f) == bits(res.f) and bits(div.cross.g) == bits(res.g) and div.ot_xy == res.value
    box = OC.box_scale(X, Y, kind)
    for name, rows, w, got_value in (("xx", X, a, div.ot_xx), ("yy", Y, b, div.ot_yy)):
        _, t = runs[name]
        S = T._Sets(rows, rows, w, w, kind, same=True)
        with torch.cuda.device(S.dev):
            f, v, n_iter, converged = T._solve_self(S, eps, box, FIXED["scaling"], 0.0, 40, 10)
        e = OC.err(f.cpu().numpy(), t.f).max()
        tv = 2 * float((w * t.f).sum())
        tg = 2 * OC.value_gate(t.gate, [(w, t.f)], len(rows))
        print(f"ot solve {name}: potential {e / t.gate:.4f} of the accumulated gate {t.gate:.3e}, value {abs(v - tv) / tg:.4f} of its gate")
        assert n_iter == 40 and not converged and e <= t.gate
        assert v == got_value and abs(v - tv) <= tg
    assert div.value == div.ot_xy - div.ot_xx / 2 - div.ot_yy / 2


def test_two_calls_give_the_same_bits():
    from scrubvae_amd.eval import sinkhorn
    for size in [(65, 700, 4), (200, 300, 70)]:
        q, x, off, eps, _, _ = OC.case(*size, 0)
        S = sets(q, x, 0)
        one, two = softmin(S, off, eps), softmin(S, off, eps)
        assert bits(one[0]) == bits(two[0]) and bits(one[1]) == bits(two[1])
    X, Y, eps, _ = OC.solve_case(150, 130, 3, 0)
    r1, r2 = sinkhorn(X, Y, epsilon=eps, **FIXED), sinkhorn(X, Y, epsilon=eps, **FIXED)
    assert bits(r1.f) == bits(r2.f) and bits(r1.g) == bits(r2.g)
    assert (r1.value, r1.transport_cost, r1.marginal_error) == (r2.value, r2.transport_cost, r2.marginal_error)
    assert bits(r1.barycentric_map()) == bits(r2.barycentric_map())


@needs_longdouble
@pytest.mark.parametrize("m,n,d", [(130, 65, 17), (65, 700, 4)])
def test_permuting_rows_changes_no_bit_and_columns_stay_within_twice_the_gate(m, n, d):
    q, x, off, eps, _, g = OC.case(m, n, d, 0)
    L, cbar = softmin(sets(q, x, 0), off, eps)
    p = np.random.default_rng(m).permutation(m)
    Lp, cp = softmin(sets(q[p], x, 0), off, eps)
    assert bits(Lp) == bits(L[p]) and bits(cp) == bits(cbar[p])     # a row's sums do not depend on the other rows of Q
    c = np.random.default_rng(n).permutation(n)
    Lc, cc = softmin(sets(q, x[c], 0), off[c], eps)
    assert (np.abs(Lc - L) <= 2 * g.tol_L).all() and (np.abs(cc - cbar) <= 2 * g.tol_cbar).all()


def test_input_kinds_give_the_same_bits():
    from scrubvae_amd.eval import sinkhorn
    X, Y, eps, _ = OC.solve_case(150, 130, 3, 0)    # float32-representable values
    base = sinkhorn(X, Y, epsilon=eps, **FIXED)
    xt, yt = torch.from_numpy(X.copy()), torch.from_numpy(Y.copy())     # the cached case is read-only
    for x, y in ((X.astype(np.float32), Y.astype(np.float32)), (xt, yt), (xt.cuda(), yt.cuda()), (xt.float().cuda(), Y),
                 (X, yt.float())):
        got = sinkhorn(x, y, epsilon=eps, **FIXED)
        assert bits(got.f) == bits(base.f) and bits(got.g) == bits(base.g) and got.value == base.value
    w = np.full(150, 1.0 / 150)
    got = sinkhorn(X, Y, epsilon=eps, a=torch.from_numpy(w).cuda(), b=np.full(130, 1.0 / 130), **FIXED)
    assert bits(got.f) == bits(base.f) and got.value == base.value


def test_sinkhorn_equals_the_restated_solve_inside_the_assignment_sandwich():
    so = pytest.importorskip("scipy.optimize")
    from scrubvae_amd.eval import sinkhorn
    n, d = 150, 3
    X, Y = OC.blobs(n, n, d, 6)
    eps = OC.median_epsilon(X, Y, 0)
    ref = OC.solve(X, Y, eps, 0, tol=1e-9)
    res = sinkhorn(X, Y, tol=1e-9)               # epsilon=None: 0.05 x the exact median of svae_mmd_select
    C = OC.cost(X, Y, 0)
    i, j = so.linear_sum_assignment(C)
    exact = float(C[i, j].sum()) / n
    print(f"ot sinkhorn n={n} d={d}: {res.n_iter} sweeps (restated {ref.n_iter}), exact {exact:.4f} <= cost {res.transport_cost:.4f} <= value "
          f"{res.value:.4f} <= {exact + eps * np.log(n):.4f}, marginal error {res.marginal_error:.2e}")
    assert res.epsilon == eps
    assert res.n_iter == ref.n_iter and res.converged and ref.converged
    assert res.marginal_error <= 1e-9
    assert exact <= res.transport_cost + res.marginal_error * float(C.max())
    assert res.transport_cost <= res.value <= exact + eps * np.log(n)


def test_stopping_at_max_iter_warns():
    from scrubvae_amd.eval import sinkhorn
    from scrubvae_amd.eval.metrics import ConvergenceWarning
    X, Y = OC.blobs(40, 30, 3, 2)
    with pytest.warns(ConvergenceWarning):
        res = sinkhorn(X, Y, tol=1e-12, max_iter=12, check_every=1)
    assert res.n_iter == 12 and not res.converged
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        sinkhorn(X, Y, **FIXED)                  # a fixed schedule is no failure to converge


def test_divergence_of_a_set_against_itself_is_zero():
    from scrubvae_amd.eval import sinkhorn_divergence
    X = torch.from_numpy(OC.blobs(70, 70, 3, 3)[0]).cuda()
    got = sinkhorn_divergence(X, X)
    assert got.value == 0.0 and got.cross is None


@needs_longdouble
def test_barycentric_map_of_a_translated_copy():
    from scrubvae_amd.eval import sinkhorn
    X, _ = OC.blobs(140, 1, 3, 9)
    shift = np.array([0.75, -0.5, 0.25])
    Y = X + shift                                 # float32-representable rows, quarter steps: exact in fp64
    eps = 0.02 * OC.median_epsilon(X, Y, 0) / 0.05
    res = sinkhorn(X, Y, epsilon=eps, scaling=0.5, tol=0.0, max_iter=60)
    got = res.barycentric_map()
    C = OC.cost(X, Y, 0)
    off = res.g * (1.0 / eps) + np.log(np.full(140, 1.0 / 140))
    L = res._L.cpu().numpy()
    truth, tol = OC.apply_gate(C, off, eps, L, Y)
    e = OC.err(got, truth)
    print(f"ot barycentric map of a translated copy: largest error / gate {np.max(e / tol):.4f}; mean distance to x + t "
          f"{np.sqrt(((got - Y) ** 2).sum(1)).mean():.3f}, to x {np.sqrt(((got - X) ** 2).sum(1)).mean():.3f}")
    assert got.shape == X.shape and (e <= tol).all()
    assert bits(res.apply(Y)) == bits(got)
    assert np.sqrt(((got - Y) ** 2).sum(1)).mean() < 0.5 * np.sqrt(((got - X) ** 2).sum(1)).mean()   # the map follows the translation
    back = res.barycentric_map_transposed()
    assert back.shape == Y.shape and bits(res.apply_transposed(X)) == bits(back)
    assert np.sqrt(((back - X) ** 2).sum(1)).mean() < 0.5 * np.sqrt(((back - Y) ** 2).sum(1)).mean()


def labelled_blobs(n, seed, offset):
    g = np.random.default_rng(seed)
    lab = g.integers(0, 3, n)
    mu = 6.0 * np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    return (mu[lab] + offset + g.normal(size=(n, 3))).astype(np.float32).astype(np.float64), lab


@needs_longdouble
def test_transport_flow_puts_the_restated_mass_in_each_cell():
    from scrubvae_amd.eval import sinkhorn, transport_flow
    X, lx = labelled_blobs(150, 1, 0.0)
    Y, ly = labelled_blobs(170, 2, 0.4)
    names_x, names_y = np.array([-1, 7, 10 ** 9]), np.array([3, 2 ** 40, 11])     # non-contiguous ids
    res = sinkhorn(X, Y, tol=1e-7)
    assert res.converged
    ids_y, share = res.flow(torch.from_numpy(names_y[ly]).cuda())
    ids_x, ids_y2, mass = transport_flow(res, names_x[lx], names_y[ly])
    assert np.array_equal(ids_x, np.sort(names_x)) and np.array_equal(ids_y, np.sort(names_y)) and np.array_equal(ids_y2, ids_y)
    assert share.shape == (150, 3) and mass.shape == (3, 3)
    # the restated cells from the device's g, L and row marginals
    eps = res.epsilon
    C = OC.cost(X, Y, 0)
    off = res.g * (1.0 / eps) + np.log(np.full(170, 1.0 / 170))
    inv_y = np.searchsorted(ids_y, names_y[ly])
    inv_x = np.searchsorted(ids_x, names_x[lx])
    truth, tol = OC.apply_gate(C, off, eps, res._L.cpu().numpy(), np.eye(3)[inv_y])
    assert (OC.err(share, truth) <= tol).all()
    r = res.row_marginals()
    for k in range(3):
        rows = inv_x == k
        cell = (r[rows, None].astype(OC.LD) * truth[rows]).sum(axis=0)
        gate = (r[rows, None] * tol[rows]).sum(axis=0) + (rows.sum() + 4) * OC.EPS * cell.astype(np.float64)
        assert (OC.err(mass[k], cell) <= gate).all(), k
    print("ot transport_flow mass:\n", mass)
    assert abs(mass.sum() - 1) <= res.marginal_error + 1e-12
    assert (np.abs(share.sum(axis=1) - 1) <= tol.sum(axis=1) + 1e-13).all()
    # blob k of X carries names_x[k], blob k of Y names_y[k]: the largest cell of every row and column is the matching blob
    order_x, order_y = np.argsort(names_x), np.argsort(names_y)
    for k in range(3):
        row, col = int(np.flatnonzero(order_x == k)[0]), int(np.flatnonzero(order_y == k)[0])
        assert np.argmax(mass[row]) == col and np.argmax(mass[:, col]) == row


def test_launch_counts_and_work_buffers():
    from scrubvae_amd import _lib
    from scrubvae_amd.eval import sinkhorn, transport as T
    lib = _lib.lib()
    X, Y, eps, _ = OC.solve_case(70, 200, 20, 0)
    before = dict(T._OT_CALLS)
    res = sinkhorn(X, Y, epsilon=eps, **FIXED)
    # 40 sweeps of two passes and the closing pass; the error at sweeps 10 x k of those at eps_t == eps; cost and error, a f, b g
    at_eps = sum(1 for t in range(40) if OC.eps_at(t, eps, OC.box_scale(X, Y, 0), 0.5) == eps)
    assert T._OT_CALLS == {"softmin": before["softmin"] + 81, "apply": before["apply"], "select": before["select"],
                           "sums": before["sums"] + at_eps // 10 + 3}
    assert T._OT_LAST["softmin_work"] == lib.svae_ot_softmin_work(70, 200) == 3 * 4 * 128
    res.barycentric_map()
    assert T._OT_CALLS["apply"] == before["apply"] + 1 and T._OT_LAST["apply_work"] == lib.svae_ot_apply_work(70, 200, 20)
    res.barycentric_map_transposed()                                   # one more softmin for the columns' L, once
    res.apply_transposed(np.ones((70, 130)))                           # 128 + 2 columns: two launches
    assert T._OT_CALLS["softmin"] == before["softmin"] + 82 and T._OT_CALLS["apply"] == before["apply"] + 4
    assert T._OT_LAST["softmin_work"] == lib.svae_ot_softmin_work(200, 70)
    assert T._OT_LAST["apply_work"] == lib.svae_ot_apply_work(200, 70, 128)
    sinkhorn(X, Y, **FIXED)
    assert T._OT_CALLS["select"] == before["select"] + 1
