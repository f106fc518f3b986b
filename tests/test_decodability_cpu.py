"""CPU checks of the decodability metrics: the fold split and the fp64 restatements of tests/decode_checks.py against sklearn,
the C ABI declarations, and train()'s key selection."""
import warnings

import numpy as np
import pytest

from tests import decode_checks as DC


@pytest.mark.parametrize("n", [5, 7, 100, 20011])
def test_fold_split_equals_kfold(n):
    skm = pytest.importorskip("sklearn.model_selection")
    from scrubvae_amd.eval.metrics import kfold_assign
    fold = kfold_assign(n, 5)
    mine = DC.kfold_split(n, 5)
    for f, (tr, te) in enumerate(skm.KFold(n_splits=5, shuffle=True, random_state=100).split(np.zeros((n, 1)))):
        assert np.array_equal(np.nonzero(fold == f)[0], te)
        assert np.array_equal(mine[f][0], tr) and np.array_equal(mine[f][1], te)


def test_fold_split_raises_below_folds():
    from scrubvae_amd.eval.metrics import kfold_assign
    with pytest.raises(ValueError):
        kfold_assign(4, 5)
    with pytest.raises(ValueError):
        DC.kfold_split(4, 5)


def test_linear_restatement_matches_sklearn():
    lm = pytest.importorskip("sklearn.linear_model")
    from sklearn.metrics import r2_score
    g = np.random.default_rng(0)
    x = g.normal(size=(500, 6)) + 30.0
    x[:, 5] = x[:, 4]  # duplicated column: minimum-norm solution, same predictions
    y = x @ g.normal(size=(6, 2)) + g.normal(size=(500, 2))
    for tr, te in DC.kfold_split(500, 5):
        ref = r2_score(y[te], lm.LinearRegression().fit(x[tr], y[tr]).predict(x[te]))
        assert abs(DC.linear_r2(x[tr], y[tr], x[te], y[te]) - ref) < 1e-9


def test_qda_restatement_matches_sklearn():
    da = pytest.importorskip("sklearn.discriminant_analysis")
    g = np.random.default_rng(1)
    y = g.integers(0, 3, 600)
    x = g.normal(size=(3, 4))[y] + g.normal(size=(600, 4)) * (1 + y[:, None])
    tr, te = np.arange(450), np.arange(450, 600)
    clf = da.QuadraticDiscriminantAnalysis().fit(x[tr], y[tr])
    sc = DC.qda_scores(x[tr], y[tr], x[te], np.arange(3))
    assert np.abs(sc - clf.decision_function(x[te])).max() < 1e-8
    assert np.array_equal(sc.argmax(1), clf.predict(x[te]))


@pytest.mark.parametrize("K", [2, 3])
def test_logreg_restatement_matches_sklearn_saga(K):
    lm = pytest.importorskip("sklearn.linear_model")
    g = np.random.default_rng(2)
    y = g.integers(0, K, 400)
    x = g.normal(size=(K, 5))[y] + g.normal(size=(400, 5))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        clf = lm.LogisticRegression(penalty="elasticnet", l1_ratio=0.5, multi_class="ovr", solver="saga", tol=1e-10,
                                    max_iter=200000).fit(x, y)
    for c in range(1 if K == 2 else K):
        s = np.where(y == (1 if K == 2 else c), 1.0, -1.0)
        w, b = DC.logreg_fit(x, s)
        assert DC.kkt_residual(x, s, w, b) < 1e-8
        scale = np.abs(clf.coef_[c]).max()
        assert np.abs(w - clf.coef_[c]).max() <= 1e-4 * scale and abs(b - clf.intercept_[c]) <= 1e-4 * max(scale, abs(b))


def test_mlp_restatement_runs_in_fp64():
    import torch
    torch.manual_seed(0)
    init = [(l.weight.detach(), l.bias.detach()) for l in (torch.nn.Linear(4, 4), torch.nn.Linear(4, 4), torch.nn.Linear(4, 1))]
    x = np.random.default_rng(3).normal(size=(50, 4))
    p = DC.mlp_predict(x[:40], x[:40, :1], x[40:], init, steps=5)
    assert p.shape == (10, 1) and p.dtype == np.float64


def test_decode_exports_are_declared():
    import scrubvae_amd.eval as E
    assert all(callable(getattr(E, f)) for f in ("linear_rand_cv", "mlp_rand_cv", "log_class_rand_cv", "qda_rand_cv"))


@pytest.mark.parametrize("cfg", [{"train": {}, "data": {}}, {"train": {"minimal_test": True}, "data": {"dataset": "4_mice"}},
                                 {"train": {}, "data": {"dataset": "other"}}])
def test_decodability_keys_off_without_a_known_dataset(cfg):
    from scrubvae_amd.train.trainer import decodability_metrics
    assert decodability_metrics(cfg, None, None, None) == {}


def test_limits_raise():
    from scrubvae_amd.eval import metrics as M
    with pytest.raises(ValueError):
        M._check_dims(100, 129, 5)
    with pytest.raises(ValueError):
        M._check_dims(100, 8, 5, ny=9)
    with pytest.raises(ValueError):
        M._check_dims(100, 8, 5, k=65)
    M._check_dims(100, 8, 5, k=36)  # the 36 subjects of the Parkinson's data set
    with pytest.raises(ValueError):
        M._check_dims(100, 8, 11)


def test_logreg_problems_are_the_classes_of_each_training_fold():
    from scrubvae_amd.eval.metrics import logreg_problems
    cnt = np.array([[5, 5, 0], [5, 5, 0], [0, 0, 9]])  # class 2 lives in fold 2 only
    pfold, pos, pstart, neg = logreg_problems(cnt)
    assert list(pstart) == [0, 3, 6, 7]
    assert list(pfold) == [0, 0, 0, 1, 1, 1, 2] and list(pos) == [0, 1, 2, 0, 1, 2, 1]
    assert list(neg) == [-1, -1, 0]                       # fold 2 trains on {0, 1}: binary, classes_[1] positive
    with pytest.raises(ValueError):
        logreg_problems(np.array([[5, 0], [5, 0], [0, 5]]))  # fold 2 trains on class 0 only


def test_r2_from_stats_matches_r2_score():
    skm = pytest.importorskip("sklearn.metrics")
    from scrubvae_amd.eval.metrics import _r2_from_stats
    g = np.random.default_rng(4)
    cases = []
    y = g.normal(size=(40, 3)) + 5.0
    p = y + g.normal(size=(40, 3)) * 0.3
    cases.append((y, p))
    yc = np.tile(np.array([[2.0, 1.0]]), (30, 1))          # constant targets: force_finite -> 1 (exact) and 0 (not)
    pc = yc.copy()
    pc[:, 1] += 0.5
    cases.append((yc, pc))
    for y, p in cases:
        st = np.stack([((y - p) ** 2).sum(0), y.sum(0), (y ** 2).sum(0), np.full(y.shape[1], len(y))], 1)[None]
        assert abs(_r2_from_stats(st)[0] - skm.r2_score(y, p)) < 1e-12


def test_mlp_init_draws_the_reference_mlp():
    import torch
    from scrubvae_amd.eval.metrics import mlp_init
    torch.manual_seed(11)
    got = mlp_init(6, 2)
    torch.manual_seed(11)
    ref = torch.nn.Sequential(torch.nn.Linear(6, 6), torch.nn.ReLU(), torch.nn.Linear(6, 6), torch.nn.ReLU(), torch.nn.Linear(6, 2))
    lins = [m for m in ref if isinstance(m, torch.nn.Linear)]
    for (w, b), l in zip(got, lins):
        assert torch.equal(w, l.weight) and torch.equal(b, l.bias)


class _Data:
    def __getitem__(self, i):
        import torch
        return {k: torch.zeros(10, 1) for k in ("avg_speed_3d", "heading", "ids", "pd_label")}


class _Loader:
    dataset = _Data()


def test_decodability_metrics_skip_an_unsupported_metric_with_a_warning(monkeypatch):
    import scrubvae_amd.eval as E
    from scrubvae_amd.train.trainer import decodability_metrics

    def ok(z, y_true, window, folds):
        return [0.5, 0.7]

    def bad(z, y_true, window, folds):
        raise ValueError("y has only 1 sample in class 3")

    for name in ("linear_rand_cv", "mlp_rand_cv", "log_class_rand_cv"):
        monkeypatch.setattr(E, name, ok)
    monkeypatch.setattr(E, "qda_rand_cv", bad)

    class Model:
        window = 1

    with pytest.warns(UserWarning, match="acc_ids_qda skipped"):
        out = decodability_metrics({"train": {}, "data": {"dataset": "parkinsons"}}, Model(), _Loader(), None)
    assert set(out) == {"acc_ids_log_mean", "acc_ids_log_std", "acc_pd_label_log_mean", "acc_pd_label_log_std"}
    assert out["acc_ids_log_mean"] == 0.6 and abs(out["acc_ids_log_std"] - 0.1) < 1e-12
