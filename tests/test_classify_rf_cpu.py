"""CPU checks of the random-forest surface: the entry is declared, exported and bound, the restatement's pieces hold on their own,
and every message comes before any device work.  No GPU needed."""
import os
import re

import numpy as np
import pytest

import classify_rf_ref as RF
from rcppml_amd import _abi, classify as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_is_declared_exported_and_bound():
    import rcppml_amd
    src = open(os.path.join(ROOT, "include", "rcppml_gpu.h")).read()
    m = re.search(r"RCPPML_GPU_API void rcppml_gpu_classify_rf_ex\((.*?)\);", src, flags=re.S)
    assert m and m.group(1).count("*") == 31 and len(m.group(1).split(",")) == 31
    assert "rcppml_gpu_classify_rf_ex" in _abi.EXPORTED_SYMBOLS and hasattr(_abi.lib(), "rcppml_gpu_classify_rf_ex")
    assert "ops_classify_rf.hip" in open(os.path.join(ROOT, "rcppml_amd", "csrc", "Makefile")).read()
    assert rcppml_amd.classify_rf is K.classify_rf


def test_restatement_bins_and_a_separable_tree():
    lo, hi = np.array([0.0, 2.0]), np.array([1.0, 2.0])
    x = np.array([[0.0, 2.0], [1.0, 2.0], [0.5, 9.0], [-3.0, 2.0], [7.0, 2.0], [1.0 / 256, 2.0], [np.nextafter(1.0 / 256, 0), 2.0]])
    assert RF.bins(x, lo, hi).tolist() == [[0, 0], [255, 0], [128, 0], [0, 0], [255, 0], [1, 0], [0, 0]]
    train = np.array([[0.0], [0.1], [0.2], [0.8], [0.9], [1.0]])
    y = np.array([0, 0, 0, 1, 1, 1])
    f = RF.forest(train, np.array([[0.05], [0.95]]), y, 2, ntree=4, seed=1)
    assert f["votes"].tolist() == [[4, 0], [0, 4]] and f["predictions"].tolist() == [0, 1] and np.all(f["n_nodes"] <= 3)
    assert np.all(f["leaf_class"][f["feature"] >= 0] >= 0) and np.all(f["left"][:, 0] == np.where(f["n_nodes"] == 3, 1, -1))


def test_messages_come_before_device_work(monkeypatch):
    seen = []
    monkeypatch.setattr(_abi, "classify_rf", lambda *a, **kw: seen.append((a, kw)) or dict(status=-1, error="stub"))
    emb, lab = np.random.default_rng(0).standard_normal((30, 9)), np.arange(30) % 3
    with pytest.raises(ValueError, match=re.escape("length(labels) must equal nrow(embedding)")):
        K.classify_rf(emb, lab[:29])
    with pytest.raises(ValueError, match="ntree must be >= 1"):
        K.classify_rf(emb, lab, ntree=0)
    with pytest.raises(ValueError, match=re.escape("mtry must be in [1, ncol(embedding)]")):
        K.classify_rf(emb, lab, mtry=10)
    assert seen == []
    with pytest.raises(_abi.BackendError, match="stub"):
        K.classify_rf(emb, lab, test_idx=[0, 1, 2], ntree=7)
    a, kw = seen[-1]
    assert a[0].shape == (27, 9) and a[4:] == (3, 7, 3, 0) and kw == dict(forest=False)          # mtry = floor(sqrt(9)), seed None = 0


@pytest.mark.parametrize("kw, msg", [(dict(p=129), "dim must be in [1, 128]"), (dict(C=1), "n_classes must be in [2, 64]"),
                                     (dict(C=65), "n_classes must be in [2, 64]"), (dict(ntree=4097), "ntree must be in [1, 4096]"),
                                     (dict(mtry=4), "mtry must be in [1, dim] (0: floor(sqrt(dim)))"),
                                     (dict(label=3), "train_labels holds a label outside [0, n_classes)")])
def test_abi_refusals_hold_without_a_device(kw, msg):
    p, C = kw.get("p", 3), kw.get("C", 3)
    ltr = np.arange(20) % 3
    ltr[5] = kw.get("label", ltr[5])
    r = _abi.classify_rf(np.ones((20, p)), np.ones((4, p)), ltr, np.arange(4) % 3, C, kw.get("ntree", 5), kw.get("mtry", 0))
    assert (r["status"], r["error"]) == (-1, msg) and all(np.all(b == -7) for b in r["buffers"].values())


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_no_device_is_loud():
    emb, lab = np.random.default_rng(1).standard_normal((30, 4)), np.arange(30) % 3
    with pytest.raises(_abi.BackendError, match="no HIP device"):
        K.classify_rf(emb, lab, ntree=3)
