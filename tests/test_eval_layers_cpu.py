"""The layering of scrubvae_amd/eval, read from the source with ast (nothing heavy is imported for it): _device, _inputs and
_permutation sit below the feature modules, the import graph has no cycle, and a feature takes a private name from another feature
only where it reuses that feature.  Then the helpers the layers hold, on host tensors, and the no-device sentence of the modules
that used to borrow the decodability metrics' one."""
import ast
from pathlib import Path

import numpy as np
import pytest
import torch

EVAL = Path(__file__).resolve().parents[1] / "scrubvae_amd" / "eval"
SHARED = ["_device", "_inputs", "_permutation"]   # each may import only the ones before it

# (importing feature, feature imported from): the private names taken.  Every entry reuses a feature: the neighbour search, the
# EM machinery of the mixture, the MI estimator inside the conditional one, the t-SNE affinities inside the map.
ALLOWED = {
    ("metrics", "neighbors"): {"_knn_check", "_knn_device"},
    ("embed", "neighbors"): {"_knn_device"},
    ("embed_quality", "neighbors"): {"_knn_device"},
    ("embed_transform", "neighbors"): {"_knn_cross_device"},
    ("density", "neighbors"): {"_knn_device"},
    ("conditional_mi", "neighbors"): {"_knn_device"},
    ("embed_transform", "embed"): {"_search_device", "_tsne_neighbors"},
    ("conditional_mi", "mutual_info"): {"_MI_CALLS", "_mi_check", "_mi_neighbors", "_MiRun"},
    ("hmm", "cluster"): {"_EM", "_NOT_PD", "_check_model_exists", "_Rows", "_rows32"},
}


def _sibling_imports(path, top_level_only):
    """[(sibling module, name imported, line)] of `from .sibling import name` and `from . import sibling` in one eval module"""
    tree = ast.parse(path.read_text())
    nodes = tree.body if top_level_only else list(ast.walk(tree))
    out = []
    for node in nodes:
        if isinstance(node, ast.ImportFrom) and node.level == 1:
            for a in node.names:
                out.append((node.module, a.name, node.lineno) if node.module else (a.name, None, node.lineno))
    return out


def _modules():
    return {p.stem: p for p in sorted(EVAL.glob("*.py")) if p.stem != "__init__"}


def test_shared_modules_import_only_the_ones_below_them():
    mods = _modules()
    assert set(SHARED) <= set(mods)
    for i, name in enumerate(SHARED):
        siblings = {m for m, _, _ in _sibling_imports(mods[name], top_level_only=False)}
        assert siblings <= set(SHARED[:i]), (name, siblings)


def test_import_graph_has_no_cycle_and_metrics_imports_at_the_top():
    mods = _modules()
    graph = {name: {m for m, _, _ in _sibling_imports(path, top_level_only=True) if m in mods} for name, path in mods.items()}
    done, on_path = set(), []

    def visit(name):
        assert name not in on_path, "import cycle: " + " -> ".join(on_path[on_path.index(name):] + [name])
        if name in done:
            return
        on_path.append(name)
        for m in sorted(graph[name]):
            visit(m)
        on_path.pop()
        done.add(name)

    for name in sorted(graph):
        visit(name)
    top = _sibling_imports(mods["metrics"], top_level_only=True)
    assert set(_sibling_imports(mods["metrics"], top_level_only=False)) == set(top)   # none inside a function
    assert ("neighbors", "_knn_device") in {(m, n) for m, n, _ in top}


def test_private_names_cross_features_only_where_a_feature_is_reused():
    mods = _modules()
    found = {}
    for name, path in mods.items():
        if name in SHARED:
            continue
        for m, imported, line in _sibling_imports(path, top_level_only=False):
            if m in SHARED or m not in mods or imported is None or not imported.startswith("_"):
                continue
            found.setdefault((name, m), set()).add(imported)
    assert found == ALLOWED


# ---- the no-device sentence -------------------------------------------------------------------------------------------------------
_G = np.random.default_rng(0)
Z8, Q5, LAB8, E8 = _G.standard_normal((8, 3)), _G.standard_normal((5, 3)), np.array([0, 1] * 4), _G.standard_normal((8, 2))


@pytest.mark.parametrize("call,source", [
    (lambda E: E.kneighbors(Z8, 2), "csrc/knn.hip"),
    (lambda E: E.kneighbors_cross(Z8, Q5, 2), "csrc/knn.hip"),
    (lambda E: E.silhouette_samples(Z8, LAB8), "csrc/silhouette.hip"),
    (lambda E: E.tsne(Z8, perplexity=2.0), "csrc/tsne.hip"),
    (lambda E: E.TSNEMap(Z8, E8, perplexity=2.0).transform(Q5), "csrc/tsne.hip"),
    (lambda E: E.tsne_transform(Z8, E8, Q5, perplexity=2.0), "csrc/tsne.hip"),
], ids=["kneighbors", "kneighbors_cross", "silhouette_samples", "tsne", "TSNEMap", "tsne_transform"])
def test_no_device_sentence_names_the_modules_own_source(call, source, monkeypatch):
    import scrubvae_amd.eval as E
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError) as err:
        call(E)
    text = str(err.value)
    assert source in text and "decode.hip" not in text and text.endswith("; no device is available")


# ---- the merged helpers, on the host ------------------------------------------------------------------------------------------------
def test_on_device_gives_contiguous_tensors_and_copies_a_read_only_array():
    from scrubvae_amd.eval._device import _on_device
    cpu = torch.device("cpu")
    a = np.arange(12.0).reshape(4, 3)
    a.setflags(write=False)
    t = _on_device(a, cpu)
    assert t.is_contiguous() and np.array_equal(t.numpy(), a)
    assert not np.shares_memory(t.numpy(), a)
    t[0, 0] = -1.0                                   # the copy is writable, the caller's array is untouched
    assert a[0, 0] == 0.0
    base = torch.arange(24.0).reshape(4, 6)
    view = base[:, ::2]
    assert not view.is_contiguous()
    t = _on_device(view, cpu)
    assert t.is_contiguous() and torch.equal(t, view)
    whole = torch.arange(6.0).reshape(2, 3)
    t = _on_device(whole, cpu)
    assert t.is_contiguous() and torch.equal(t, whole)


def test_device_of_takes_any_number_of_candidates(monkeypatch):
    from scrubvae_amd.eval import _device
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for args in ((Z8,), (Z8, torch.zeros(2)), (None, Z8, None), ()):
        with pytest.raises(RuntimeError, match="^nobody home$"):
            _device._device_of(*args, who="nobody home")


def test_pvalue():
    from scrubvae_amd.eval._permutation import _pvalue
    null = np.array([0.5, 2.0, 1.0, 1.0, -3.0])
    assert _pvalue(1.0, null) == (1 + 3) / (1 + 5)    # ties count: >=
    assert _pvalue(1.0000000000000002, null) == (1 + 1) / (1 + 5)
    assert _pvalue(9.0, null) == 1 / 6 and _pvalue(-9.0, null) == 1.0
    for s in (-3.0, 0.0, 0.5, 0.75, 2.0):
        assert _pvalue(s, null) == (1 + sum(1 for v in null if v >= s)) / (1 + len(null))
    assert _pvalue(0.0, np.array([0.0])) == 1.0 and _pvalue(0.1, np.array([0.0])) == 0.5   # P = 1
    assert np.isnan(_pvalue(float("nan"), null))
    assert isinstance(_pvalue(1.0, null), float)
