"""train()'s latent decodability metrics on the device (scrubvae_amd/eval/metrics.py, csrc/decode.hip) against the fp64
restatements of tests/decode_checks.py."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

from tests import decode_checks as DC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def planted(n, d, ny, seed, offset=50.0):
    g = np.random.default_rng(seed)
    x = g.normal(size=(n, d)) * np.exp(g.normal(size=d)) + offset  # |mean| >> std in some columns
    x[:, 0] = 3.0                     # a constant column
    x[:, 1] = x[:, 2]                 # a duplicated column
    B = g.normal(size=(d, ny))
    y = (x - x.mean(0)) @ B * 0.1 + g.normal(size=(n, ny))
    return x.astype(np.float32), y.astype(np.float32)


def test_moments_match_fp64_and_are_bit_reproducible():
    from scrubvae_amd.eval import metrics as M
    g = np.random.default_rng(0)
    n, d, ny = 3000, 32, 3
    x = (g.normal(size=(n, d)) + 100.0).astype(np.float32)
    y = g.normal(size=(n, ny)).astype(np.float32)
    fold = M.kfold_assign(n, 5)
    cls = g.integers(0, 4, n)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    R = M._Rows(xd, fold, cls, 4, yd, xd.device)
    D = d + 1 + ny
    out1 = R.moments(D, R.glo, R.ghi).cpu().numpy()
    out2 = R.moments(D, R.glo, R.ghi).cpu().numpy()
    assert np.array_equal(out1, out2)
    x64, y64 = x.astype(np.float64)[R.perm], y.astype(np.float64)[R.perm]
    mean = np.concatenate([x.astype(np.float64).mean(0), y.astype(np.float64).mean(0)])
    A = np.hstack([x64 - mean[:d], np.ones((n, 1)), y64 - mean[d:]])
    for gi in range(20):
        a = A[R.glo[gi]:R.ghi[gi]]
        ref = a.T @ a
        bound = np.abs(a).T @ np.abs(a)
        assert (np.abs(out1[gi] - ref) <= 1e-12 * bound + 1e-300).all(), gi


@pytest.mark.parametrize("d,ny", [(32, 2), (128, 3)])
def test_linear_rand_cv_matches_lstsq(d, ny):
    from scrubvae_amd.eval import linear_rand_cv
    x, y = planted(20000, d, ny, seed=d)
    got = linear_rand_cv(torch.from_numpy(x).cuda(), y, window=1, folds=5)
    ref = [DC.linear_r2(x[tr], y[tr], x[te], y[te]) for tr, te in DC.kfold_split(len(x), 5)]
    assert len(got) == 5 and all(isinstance(v, float) for v in got)
    assert np.abs(np.array(got) - ref).max() <= 1e-8, (got, ref)
    got_np = linear_rand_cv(np.repeat(x, 3, axis=0), np.repeat(y, 3, axis=0), window=3, folds=5)  # the window downsample
    assert np.abs(np.array(got_np) - ref).max() <= 1e-8


def class_data(n, d, K, seed):
    g = np.random.default_rng(seed)
    y = g.integers(0, K, n)
    mus = g.normal(size=(K, d)) * 0.7
    As = g.normal(size=(K, d, d)) / np.sqrt(d) + np.eye(d)[None]
    x = mus[y] + np.einsum("nij,nj->ni", As[y], g.normal(size=(n, d)))
    return x.astype(np.float32), y


def test_qda_rand_cv_matches_restatement():
    from scrubvae_amd.eval import metrics as M
    x, y = class_data(20000, 32, 4, seed=1)
    out = M._qda(torch.from_numpy(x).cuda(), y, 1, 5, want_rows=True)
    near, rows = 0, 0
    accs = []
    for f, (tr, te) in enumerate(DC.kfold_split(len(x), 5)):
        sc = DC.qda_scores(x[tr], y[tr], x[te], np.arange(4))
        pred = sc.argmax(1)
        srt = np.sort(sc, 1)
        clear = (srt[:, -1] - srt[:, -2]) > 1e-6
        near += (~clear).sum()
        rows += len(te)
        assert np.array_equal(out["pred"][te][clear], pred[clear]), f
        accs.append((pred == y[te]).mean())
    assert near < 1e-3 * rows
    assert np.abs(np.array(out["acc"]) - accs).max() <= near / 4000 + 1e-12
    assert M.qda_rand_cv(x, y, window=1, folds=5) == out["acc"]


@pytest.mark.parametrize("K", [4, 2])
def test_log_class_rand_cv_reaches_the_optimum(K):
    from scrubvae_amd.eval import metrics as M
    x, y = class_data(4000, 16, K, seed=K)
    x[:, 3] += 20.0
    with warnings.catch_warnings():
        warnings.simplefilter("error", M.ConvergenceWarning)
        out = M._logreg(torch.from_numpy(x).cuda(), y, 1, 5, want_rows=True)
    KP = 1 if K == 2 else K
    X64 = x.astype(np.float64)
    for f, (tr, te) in enumerate(DC.kfold_split(len(x), 5)):
        dec = []
        assert out["pstart"][f + 1] - out["pstart"][f] == KP
        for c in range(KP):
            pos = 1 if K == 2 else c
            p = out["pstart"][f] + c
            assert out["pfold"][p] == f and out["pos"][p] == pos
            s = np.where(y[tr] == pos, 1.0, -1.0)
            w, b = out["coef"][p], out["intercept"][p]
            g0 = max(np.abs(DC.logreg_grad(X64[tr], s, np.zeros(16), 0.0)[0]).max(), abs(DC.logreg_grad(X64[tr], s, np.zeros(16), 0.0)[1]))
            assert DC.kkt_residual(X64[tr], s, w, b) <= 1e-6 * g0, (f, c)
            wr, br = DC.logreg_fit(X64[tr], s)
            scale = max(np.abs(wr).max(), abs(br))
            assert np.abs(w - wr).max() <= 1e-5 * scale and abs(b - br) <= 1e-5 * scale, (f, c)
            dec.append(X64[te] @ wr + br)
        dec = np.stack(dec, 1)
        pred = (dec[:, 0] > 0).astype(int) if K == 2 else dec.argmax(1)
        srt = np.sort(dec, 1)
        clear = np.abs(dec[:, 0]) > 1e-6 if K == 2 else (srt[:, -1] - srt[:, -2]) > 1e-6
        assert np.array_equal(out["pred"][te][clear], pred[clear])
    assert M.log_class_rand_cv(x, y, window=1, folds=5) == out["acc"]


def test_log_class_rand_cv_fits_the_classes_present_in_each_training_fold():
    """A class that lives in one fold only is absent from that fold's training rows: sklearn fits the remaining classes
    there (two left -> one binary problem), and so does the device."""
    from scrubvae_amd.eval import metrics as M
    x, y = class_data(3000, 8, 3, seed=7)
    split = DC.kfold_split(len(x), 5)
    rare = np.isin(np.arange(len(y)), split[2][1][:40])  # 40 rows of fold 2 only
    y3 = np.where(rare, 3, y)
    y2 = np.where(rare, 3, np.minimum(y, 1))             # fold 2 then trains on classes {0, 1}: binary
    X64 = x.astype(np.float64)
    for labels in (y3, y2):
        out = M._logreg(torch.from_numpy(x).cuda(), labels, 1, 5, want_rows=True)
        for f, (tr, te) in enumerate(split):
            present = np.unique(labels[tr])
            ps = present[1:] if len(present) == 2 else present
            p0, p1 = out["pstart"][f], out["pstart"][f + 1]
            assert list(out["pos"][p0:p1]) == list(ps), (f, out["pos"][p0:p1], ps)
            dec = []
            for i, c in enumerate(ps):
                s = np.where(labels[tr] == c, 1.0, -1.0)
                g = DC.logreg_grad(X64[tr], s, np.zeros(8), 0.0)
                w, b = out["coef"][p0 + i], out["intercept"][p0 + i]
                assert DC.kkt_residual(X64[tr], s, w, b) <= 1e-6 * max(np.abs(g[0]).max(), abs(g[1])), (f, c)
                dec.append(X64[te] @ w + b)
            dec = np.stack(dec, 1)
            if len(present) == 2:
                pred, clear = np.where(dec[:, 0] > 0, ps[0], present[0]), np.abs(dec[:, 0]) > 1e-6
            else:
                srt = np.sort(dec, 1)
                pred, clear = ps[dec.argmax(1)], (srt[:, -1] - srt[:, -2]) > 1e-6
            assert np.array_equal(out["pred"][te][clear], pred[clear]), f


def test_mlp_rand_cv_matches_torch_recipe():
    from scrubvae_amd.eval import metrics as M
    x, y = planted(2000, 16, 2, seed=5, offset=0.0)
    torch.manual_seed(123)
    init = [M.mlp_init(16, 2) for _ in range(5)]
    got = M.mlp_rand_cv(torch.from_numpy(x).cuda(), y, window=1, folds=5, init=init)
    for f, (tr, te) in enumerate(DC.kfold_split(len(x), 5)):
        r64 = DC.r2(y[te].astype(np.float64), DC.mlp_predict(x[tr], y[tr], x[te], init[f], torch.float64))
        r32 = DC.r2(y[te].astype(np.float64), DC.mlp_predict(x[tr], y[tr], x[te], init[f], torch.float32).astype(np.float64))
        assert abs(got[f] - r64) <= max(1e-3, 4 * abs(r32 - r64)), (f, got[f], r64, r32)
    torch.manual_seed(123)
    assert M.mlp_rand_cv(x, y, window=1, folds=5) == got  # default draws: the same order from the global generator


def test_mlp_rand_cv_repeats_bitwise_above_the_autotune_size():
    """n = 20 000, z = 128 is above the GEMM autotune threshold: the first call fixes the tiles of the cached geometry, a second
    call from the same initial weights gives the same R^2 bit for bit."""
    from scrubvae_amd.eval import metrics as M
    x, y = planted(20000, 128, 3, seed=9, offset=0.0)
    xd = torch.from_numpy(x).cuda()
    torch.manual_seed(5)
    init = [M.mlp_init(128, 3) for _ in range(5)]
    first = M.mlp_rand_cv(xd, y, window=1, folds=5, init=init)
    assert M.mlp_rand_cv(xd, y, window=1, folds=5, init=init) == first
    assert np.isfinite(first).all()


class _ValSet:
    def __init__(self, n, seed, n_ids):
        g = torch.Generator().manual_seed(seed)
        self.d = {"avg_speed_3d": torch.randn(n, 3, generator=g), "heading": torch.randn(n, 2, generator=g),
                  "ids": torch.randint(0, n_ids, (n, 1), generator=g), "pd_label": torch.randint(0, 2, (n, 1), generator=g)}

    def __getitem__(self, i):
        return {k: v[i] for k, v in self.d.items()}

    def __len__(self):
        return len(self.d["ids"])


KEYS_4MICE = {"r2_{}_{}_{}".format(k, m, s) for k in ("avg_speed_3d", "heading") for m in ("lin", "mlp") for s in ("mean", "std")} | \
    {"acc_ids_{}_{}".format(m, s) for m in ("log", "qda") for s in ("mean", "std")}
KEYS_PD = {"acc_{}_{}_{}".format(k, m, s) for k in ("ids", "pd_label") for m in ("log", "qda") for s in ("mean", "std")}


@pytest.mark.parametrize("case", ["4_mice", "parkinsons", "minimal", "none"])
def test_train_logs_decodability_from_epoch_50(case, monkeypatch):
    from scrubvae_amd.train import trainer
    window, n = 8, 8 * 2000
    # parkinsons: the reference folds the raw subject ids into 36 (data/dataset.py:346)
    val = torch.utils.data.DataLoader(_ValSet(n, 0, 36 if case == "parkinsons" else 4), batch_size=64)
    logged = []

    class Run:
        def log(self, metrics, epoch):
            logged.append((epoch, dict(metrics)))

    class Model:
        device = "cuda"
        disentangle = {}

    model = Model()
    model.window = window
    z = torch.randn(n, 16, generator=torch.Generator().manual_seed(1))
    monkeypatch.setattr(trainer, "get_optimizer_and_lr_scheduler", lambda *a: (None, None))
    monkeypatch.setattr(trainer, "train_epoch", lambda *a: {"total": 1.0})
    monkeypatch.setattr(trainer, "test_epoch", lambda *a: ({"total": 2.0}, z))
    config = {"train": {"num_epochs": 50}, "model": {"start_epoch": 48}, "loss": {}, "data": {"batch_size": 64}}
    if case in ("4_mice", "parkinsons", "minimal"):
        config["data"]["dataset"] = "4_mice" if case == "minimal" else case
    if case == "minimal":
        config["train"]["minimal_test"] = True
    with warnings.catch_warnings():
        warnings.simplefilter("error", UserWarning)  # no metric may be skipped on this data
        trainer.train(config, model, {"train": None, "val": val}, run=Run())
    assert [e for e, _ in logged] == [49, 50]
    new = set(logged[1][1]) - {"total_train", "time", "total_test"}
    assert new == {"4_mice": KEYS_4MICE, "parkinsons": KEYS_PD}.get(case, set())
    assert all(isinstance(logged[1][1][k], float) for k in new)


def test_product_path_does_not_need_sklearn():
    code = (
        "import sys; sys.modules['sklearn'] = None\n"
        "import numpy as np, torch\n"
        "from scrubvae_amd.eval import linear_rand_cv, mlp_rand_cv, log_class_rand_cv, qda_rand_cv\n"
        "g = np.random.default_rng(0); x = g.normal(size=(400, 8)).astype(np.float32)\n"
        "y = g.normal(size=(400, 2)).astype(np.float32); c = g.integers(0, 3, 400)\n"
        "for f, t in ((linear_rand_cv, y), (mlp_rand_cv, y), (log_class_rand_cv, c), (qda_rand_cv, c)):\n"
        "    r = f(x, t, window=1, folds=5); assert len(r) == 5, r\n"
        "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
