"""Entropic optimal transport without a GPU: the fp64 restatement of tests/ot_checks.py inside both derived gates of the long-double
one (which checks the gates themselves here), the solved problem inside the sandwich around scipy's exact assignment, the
divergence against the shift between two blobs, the flows' sums, argument errors raised before any device work, and the C-ABI
exports."""
import inspect

import numpy as np
import pytest
import torch

from tests import ot_checks as OC

needs_longdouble = pytest.mark.skipif(not OC.LONGDOUBLE, reason="np.longdouble is no wider than fp64 here: no truth to hold the value to")


@needs_longdouble
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("m,n,d", OC.SIZES)
def test_restated_pass_sits_inside_the_single_pass_gate(m, n, d, kind):
    _, _, off, eps, C, g = OC.case(m, n, d, kind)
    s = OC.softmin(C, off, eps)
    eL, ec = OC.err(s.L, g.truth.L), OC.err(s.cbar, g.truth.cbar)
    print(f"ot m={m} n={n} d={d} kind={kind}: restated L {np.max(eL / g.tol_L):.4f} of its gate ({np.max(g.tol_L) / OC.EPS:.0f} u), cbar "
          f"{np.max(ec / g.tol_cbar):.4f} of its gate")
    assert (eL <= g.tol_L).all() and (ec <= g.tol_cbar).all()
    assert np.isfinite(g.tol_L).all() and np.isfinite(g.tol_cbar).all() and (g.tol_L > 0).all()
    # the offsets spread over +-50: the running maximum of a row moves
    assert off.max() - off.min() > 50 or n < 3


@needs_longdouble
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("m,n,d", OC.APPLY_SIZES)
def test_restated_apply_sits_inside_its_gate(m, n, d, kind):
    _, _, off, eps, C, g = OC.case(m, n, d, kind)
    L = OC.softmin(C, off, eps).L
    V = np.random.default_rng(m).normal(size=(n, 17))
    truth, tol = OC.apply_gate(C, off, eps, L, V)
    e = OC.err(OC.apply(C, off, eps, L, V), truth)
    print(f"ot apply m={m} n={n} d={d} kind={kind}: restated {np.max(e / tol):.4f} of its gate")
    assert (e <= tol).all()
    # the plan is row-normalised: applied to a column of ones it returns 1 within the same gate
    ones_truth, ones_tol = OC.apply_gate(C, off, eps, L, np.ones((n, 1)))
    assert (np.abs((ones_truth - 1).astype(np.float64)) <= ones_tol + g.tol_L[:, None]).all()


@needs_longdouble
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("nx,ny,d", OC.SOLVE_SIZES)
def test_restated_solve_sits_inside_the_accumulated_gate(nx, ny, d, kind):
    X, Y, eps, runs = OC.solve_case(nx, ny, d, kind)
    for name, (got, truth) in runs.items():
        assert got.n_iter == truth.n_iter == 40 and not got.converged and got.eps_t == truth.eps_t
        assert got.eps_t[0] > eps and got.eps_t[-1] == eps      # the schedule anneals and arrives
        ef, eg = OC.err(got.f, truth.f).max(), OC.err(got.g, truth.g).max()
        print(f"ot solve {name} nx={nx} ny={ny} d={d} kind={kind}: potentials {max(ef, eg) / truth.gate:.4f} of the accumulated gate "
              f"{truth.gate:.3e}")
        assert ef <= truth.gate and eg <= truth.gate


def assignment_sandwich(n, d, seed):
    so = pytest.importorskip("scipy.optimize")
    X, Y = OC.blobs(n, n, d, seed)
    eps = OC.median_epsilon(X, Y, 0)
    s = OC.solve(X, Y, eps, 0, tol=1e-9)
    c = OC.closing(X, Y, s.f, s.g, eps, 0)
    C = OC.cost(X, Y, 0)
    i, j = so.linear_sum_assignment(C)
    return s, c, float(C[i, j].sum()) / n, float(C.max()), eps


@pytest.mark.parametrize("n,d,seed", [(150, 3, 6), (300, 8, 308)])
def test_solved_problem_sits_inside_the_assignment_sandwich(n, d, seed):
    """exact <= transport_cost + eta Cmax (the plan is within eta of a feasible one), transport_cost <= value (the entropy term is
    not negative), value <= exact + epsilon log n (the optimal permutation plan has KL = log n against the product measure)"""
    s, c, exact, cmax, eps = assignment_sandwich(n, d, seed)
    print(f"ot sandwich n={n} d={d}: {s.n_iter} sweeps, exact {exact:.4f} <= cost {c.transport_cost:.4f} <= value {c.value:.4f} <= "
          f"{exact + eps * np.log(n):.4f}, marginal error {c.marginal_error:.2e}")
    assert s.converged and s.n_iter < 1000 and c.marginal_error <= 1e-9
    assert exact <= c.transport_cost + c.marginal_error * cmax
    assert c.transport_cost <= c.value
    assert c.value <= exact + eps * np.log(n)


def test_divergence_is_positive_and_grows_with_the_shift():
    values = []
    for shift in (0.0, 0.25, 0.5, 1.0, 2.0):
        X, Y = OC.blobs(150, 130, 3, 7, shift=shift)
        values.append(OC.divergence(X, Y, OC.median_epsilon(X, Y, 0), 0)[0])
    print("ot divergence at shifts 0, 0.25, 0.5, 1, 2:", " ".join(f"{v:.3f}" for v in values))
    assert values[0] > 0 and all(b > a for a, b in zip(values, values[1:]))


@needs_longdouble
def test_flows_sum_to_one():
    X, Y = OC.blobs(90, 70, 3, 11)
    lx, ly = np.arange(90) % 3, np.array([-1, 7, 10 ** 9, 12])[np.arange(70) % 4]
    eps = OC.median_epsilon(X, Y, 0)
    s = OC.solve(X, Y, eps, 0, tol=1e-9)
    c = OC.closing(X, Y, s.f, s.g, eps, 0)
    ids, share = OC.flow(X, Y, s.g, eps, ly)
    assert np.array_equal(ids, [-1, 7, 12, 10 ** 9]) and share.shape == (90, 4) and (share >= 0).all()
    C, off, L = OC.plan_rows(X, Y, s.g, eps, 0)
    _, tol = OC.apply_gate(C, off, eps, L, np.ones((70, 1)))
    row_tol = tol[:, 0] + OC.gate(C, off, eps).tol_L + 8 * OC.EPS   # the weights, L itself, the sum over the four labels
    assert (np.abs(share.sum(axis=1) - 1) <= row_tol).all()
    ids_x, mass = OC.transport_flow(c.r, share, lx)
    assert np.array_equal(ids_x, [0, 1, 2]) and mass.shape == (3, 4)
    assert abs(mass.sum() - 1) <= c.marginal_error + row_tol.max() + (90 + 4) * OC.EPS
    assert (np.abs(mass.sum(axis=1) - 1 / 3) <= c.marginal_error + row_tol.max() + (90 + 4) * OC.EPS).all()


XS, YS = OC.blobs(12, 9, 2, 0)


@pytest.mark.parametrize("X,Y,kwargs", [
    (XS[0], YS, {}),                                          # 1-D
    (XS[None], YS, {}),                                       # 3-D
    (XS, YS[:, :1], {}),                                      # feature counts differ
    (XS[:0], YS, {}),                                         # no rows
    (np.where(np.arange(24).reshape(12, 2) == 5, np.nan, XS), YS, {}),
    (XS, np.where(np.arange(18).reshape(9, 2) == 5, np.inf, YS), {}),
    (XS, YS, dict(cost="cosine")),
    (XS, YS, dict(epsilon=0.0)),
    (XS, YS, dict(epsilon=-1.0)),
    (XS, YS, dict(epsilon=float("nan"))),
    (XS, YS, dict(epsilon="1")),
    (XS, YS, dict(scaling=1.0)),
    (XS, YS, dict(scaling=0.0)),
    (XS, YS, dict(tol=-1e-3)),
    (XS, YS, dict(max_iter=0)),
    (XS, YS, dict(max_iter=2.5)),
    (XS, YS, dict(check_every=0)),
    (XS, YS, dict(a=np.full(11, 1 / 11))),                    # wrong length
    (XS, YS, dict(a=np.full(12, 1 / 11))),                    # does not sum to 1
    (XS, YS, dict(b=np.array([1.0] + [0.0] * 8))),            # not positive
    (XS, YS, dict(b=np.full((9, 1), 1 / 9))),                 # not 1-D
    (torch.from_numpy(XS), torch.from_numpy(YS), dict(cost="l1")),
])
def test_argument_errors_before_device_work(X, Y, kwargs):
    """this machine has no device: a ValueError, not the "no device is available" RuntimeError, shows the order"""
    import scrubvae_amd.eval as E
    for fn in (E.sinkhorn, E.sinkhorn_divergence):
        with pytest.raises(ValueError):
            fn(X, Y, **kwargs)


def test_divergence_of_a_set_against_itself_is_zero_without_device_work():
    from scrubvae_amd.eval import sinkhorn_divergence, transport as T
    before = dict(T._OT_CALLS)
    for X in (XS, torch.from_numpy(XS), XS.astype(np.float32)):
        got = sinkhorn_divergence(X, X, epsilon=0.3)
        assert got.value == 0.0 and isinstance(got.value, float) and got.cross is None
    assert T._OT_CALLS == before
    with pytest.raises(ValueError):
        sinkhorn_divergence(XS, XS, a=np.full(12, 1 / 12), b=np.linspace(1, 2, 12) / np.linspace(1, 2, 12).sum())


def test_interface_defaults_are_the_documented_ones():
    import scrubvae_amd.eval as E
    for fn in (E.sinkhorn, E.sinkhorn_divergence):
        p = inspect.signature(fn).parameters
        assert [k for k in p][:2] == ["X", "Y"] and all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[2:])
        assert {k: p[k].default for k in list(p)[2:]} == dict(epsilon=None, cost="sqeuclidean", a=None, b=None, scaling=0.5, tol=1e-6,
                                                              max_iter=1000, check_every=10)
    assert "not a measured optimum" in E.sinkhorn.__doc__
    for name in ("apply", "apply_transposed", "barycentric_map", "barycentric_map_transposed", "flow"):
        assert callable(getattr(E.SinkhornResult, name))


def test_new_exports_have_signatures():
    from scrubvae_amd import _lib, build
    from scrubvae_amd.eval import transport as T
    assert "ot.hip" in build.SOURCES
    lib = _lib.lib()   # the library cross-compiled with ot.hip in it
    work, awork = lib.svae_ot_softmin_work, lib.svae_ot_apply_work
    assert work(0, 5) == 0 and work(5, 0) == 0 and work(-1, 5) == 0 and work(1 << 26, 5) == 0 and work(5, 1 << 26) == 0
    # 3 x column chunks x rows padded to 64
    assert work(1, 1) == 3 * 1 * 64
    assert work(64, 65) == 3 * 2 * 64                 # 2 column tiles, one chunk each
    assert work(130, 65) == 3 * 2 * 192
    assert work(65, 700) == 3 * 6 * 128               # 11 column tiles, at most 8 chunks: 6 of 2
    assert work(200, 300) == 3 * 5 * 256
    assert work(100000, 100000) == 3 * 1 * 100032     # 1563 row tiles: no split
    assert awork(5, 5, 0) == 0 and awork(5, 5, _lib.OT_MAX_COLS + 1) == 0 and awork(0, 5, 1) == 0 and awork(5, 0, 1) == 0
    # column chunks x rows padded to 64 x columns padded to 16, 64 or 128
    assert awork(130, 65, 1) == awork(130, 65, 16) == 2 * 192 * 16
    assert awork(130, 65, 17) == awork(130, 65, 64) == 2 * 192 * 64
    assert awork(65, 700, 65) == awork(65, 700, 128) == 6 * 128 * 128
    import scrubvae_amd.eval as E
    for name in ("sinkhorn", "sinkhorn_divergence", "transport_flow", "SinkhornResult", "SinkhornDivergence"):
        assert callable(getattr(E, name))
    assert _lib.OT_MAX_COLS == 128
    assert T._OT_CALLS.keys() >= {"softmin", "apply", "sums", "select"} and T._OT_LAST.keys() >= {"softmin_work", "apply_work"}
