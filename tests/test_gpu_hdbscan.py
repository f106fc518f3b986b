"""HDBSCAN on the device (scrubvae_amd/eval/hdbscan.py, csrc/hdbscan.hip) against the fp64 restatement of
tests/hdbscan_checks.py."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import hdbscan_checks as H

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _data(n, d, seed):
    """planted blobs with a constant column and a duplicated column (where d allows)"""
    x, _ = H.planted(n, d, max(2, min(25, n // 200)), seed)
    if d >= 3:
        x[:, 0] = 1.5
        x[:, 1] = x[:, 2]
    return x


def _check(m, ref, x64):
    assert np.array_equal(m._core_distances_, ref["core"])
    got = H.edge_set(*_edges(m))
    assert got == H.edge_set(ref["lo"], ref["hi"], ref["w"])
    assert np.array_equal(m._single_linkage_tree_, ref["tree"])
    assert m.labels_.dtype == np.intp and np.array_equal(m.labels_, ref["labels"])
    assert np.array_equal(m.probabilities_, ref["probabilities"])
    assert m.n_features_in_ == x64.shape[1]


def _edges(m):
    return m._mst_


@pytest.mark.parametrize("n,d,k", [(20011, 32, 500), (5003, 128, 7), (4099, 1, 16), (3001, 37, 1), (1000, 3, 1000)])
def test_fit_matches_restatement(n, d, k):
    from scrubvae_amd.eval import HDBSCAN
    x = _data(n, d, seed=n + d)
    x64 = x.astype(np.float64)
    mcs = min(k, 50) if k > 1 else 5
    m = HDBSCAN(min_cluster_size=max(2, mcs), min_samples=k).fit(torch.from_numpy(x).cuda())
    ref = H.fit(x64, max(2, mcs), k)
    _check(m, ref, x64)


@pytest.mark.parametrize("kw", [dict(cluster_selection_method="leaf"), dict(cluster_selection_epsilon=2.5),
                                dict(max_cluster_size=300), dict(allow_single_cluster=True), dict(alpha=0.7, min_samples=20),
                                dict(cluster_selection_method="leaf", cluster_selection_epsilon=2.5, allow_single_cluster=True)])
def test_selection_options_match_restatement(kw):
    from scrubvae_amd.eval import HDBSCAN
    x = _data(4001, 16, seed=11)
    x64 = x.astype(np.float64)
    m = HDBSCAN(min_cluster_size=40, **kw).fit(x)
    ref = H.fit(x64, 40, kw.get("min_samples"), kw.get("alpha", 1.0), kw.get("cluster_selection_method", "eom"),
                kw.get("allow_single_cluster", False), kw.get("cluster_selection_epsilon", 0.0), kw.get("max_cluster_size"))
    _check(m, ref, x64)


def test_duplicated_rows_zero_core_distance():
    """600 copies of one row: core distance 0 and merges at w = 0 (lambda = inf)"""
    from scrubvae_amd.eval import HDBSCAN
    x = _data(3000, 8, seed=5)
    x[:600] = x[700]
    x64 = x.astype(np.float64)
    m = HDBSCAN(min_cluster_size=100).fit(x)
    ref = H.fit(x64, 100)
    assert (ref["core"][:600] == 0.0).all() and (ref["w"] == 0.0).sum() >= 599
    _check(m, ref, x64)


def test_inputs_and_determinism():
    from scrubvae_amd.eval import HDBSCAN
    x = _data(6007, 32, seed=3)
    fits = [HDBSCAN(min_cluster_size=60).fit(a) for a in (x, x.astype(np.float64), torch.from_numpy(x),
                                                           torch.from_numpy(x).cuda(), torch.from_numpy(x).cuda().double())]
    for f in fits[1:]:
        assert np.array_equal(f.labels_, fits[0].labels_)
        assert np.array_equal(f.probabilities_, fits[0].probabilities_)
        assert np.array_equal(f._single_linkage_tree_, fits[0]._single_linkage_tree_)
    again = HDBSCAN(min_cluster_size=60).fit(x)
    assert np.array_equal(again._single_linkage_tree_.view(np.uint8), fits[0]._single_linkage_tree_.view(np.uint8))
    ref = H.fit(x.astype(np.float64), 60)
    for cut in (1.5, 4.0):
        assert np.array_equal(fits[0].dbscan_clustering(cut, 5), H.cut_labels(ref["tree"], cut, 5))
    m = pickle.loads(pickle.dumps(fits[0]))
    assert np.array_equal(m.labels_, fits[0].labels_)


def test_non_finite_rows():
    from scrubvae_amd.eval import HDBSCAN
    x = _data(2000, 8, seed=9).astype(np.float64)
    x[[5, 77]] = np.nan
    x[[10, 1999]] = np.inf
    x[300, 2] = -np.inf
    m = HDBSCAN(min_cluster_size=30).fit(x)
    fin = np.isfinite(x.sum(1))
    ref = H.fit(x[fin], 30)
    assert np.array_equal(m.labels_[fin], ref["labels"]) and m.labels_.dtype == np.int32
    assert (m.labels_[[5, 77]] == -3).all() and (m.labels_[[10, 1999, 300]] == -2).all()
    assert np.isnan(m.probabilities_[[5, 77]]).all() and (m.probabilities_[[10, 1999, 300]] == 0).all()
    assert np.array_equal(m.probabilities_[fin], ref["probabilities"])
    lab = m.dbscan_clustering(2.0, 5)
    assert (lab[[5, 77]] == -3).all() and (lab[[10, 1999, 300]] == -2).all()


def test_dbscan_wrapper(tmp_path):
    from scrubvae_amd.eval import HDBSCAN, dbscan
    x = _data(3000, 16, seed=4)
    got = dbscan(x, min_samples=50, label="z", path=str(tmp_path) + "/")
    assert np.array_equal(got, HDBSCAN(min_cluster_size=50).fit_predict(x))
    assert np.array_equal(np.load(tmp_path / "z_sc_pred.npy"), got)


def test_product_path_without_sklearn(tmp_path):
    code = ("import sys; sys.modules['sklearn'] = None; sys.path.insert(0, %r)\n"
            "import numpy as np\n"
            "from tests import hdbscan_checks as H\n"
            "from scrubvae_amd.eval import HDBSCAN, dbscan\n"
            "x, _ = H.planted(2000, 8, 4, 0)\n"
            "m = HDBSCAN(min_cluster_size=40).fit(x)\n"
            "k = dbscan(x, min_samples=40, path=%r)\n"
            "assert (k == m.labels_).all() and k.max() >= 1\n"
            "print('ok', k.max() + 1)\n") % (ROOT, str(tmp_path) + "/")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout


def test_full_size_planted_partition():
    from scrubvae_amd.eval import HDBSCAN
    n, d = 1 << 17, 32
    x, truth = H.planted(n, d, 25, seed=17, noise=0.0)
    m = HDBSCAN(min_cluster_size=500).fit(torch.from_numpy(x).cuda())
    lab = m.labels_
    agree = 0
    for t in np.unique(truth):
        vals, counts = np.unique(lab[truth == t], return_counts=True)
        agree += counts[vals >= 0].max() if (vals >= 0).any() else 0
    assert agree / n >= 0.99, agree / n
    assert len(np.unique(lab[lab >= 0])) == 25
    rows = np.random.default_rng(0).choice(n, 256, replace=False)
    assert np.array_equal(m._core_distances_[rows], H.core_distances(x.astype(np.float64), 500, rows=rows))


def test_launches_on_the_input_device(monkeypatch):
    """The C ABI launches on the current device's stream: a tensor on another device than the current one must be fitted with
    its own device made current.  The stream lookup is checked before every launch (raising there, nothing runs on the wrong
    device); with one GPU the input and current devices coincide."""
    from scrubvae_amd import ops
    from scrubvae_amd.eval import HDBSCAN
    x = _data(3000, 16, seed=6)
    want = HDBSCAN(min_cluster_size=40).fit(x)
    dev = torch.cuda.device_count() - 1
    seen = []
    real = ops._stream

    def stream():
        seen.append(torch.cuda.current_device())
        assert seen[-1] == dev, f"launch on cuda:{seen[-1]} for a tensor on cuda:{dev}"
        return real()

    monkeypatch.setattr(ops, "_stream", stream)
    with torch.cuda.device(0):
        m = HDBSCAN(min_cluster_size=40).fit(torch.from_numpy(x).to(f"cuda:{dev}"))
    assert seen and set(seen) == {dev}
    assert torch.cuda.current_device() == 0
    assert np.array_equal(m.labels_, want.labels_) and np.array_equal(m.probabilities_, want.probabilities_)
