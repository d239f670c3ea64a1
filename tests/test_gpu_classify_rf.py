"""GPU checks of the histogram random forest (csrc/ops_classify_rf.hip) against its numpy restatement, tests/classify_rf_ref.py.
Everything is integer work after two fixed fp64 expressions, so every comparison is np.array_equal: no tolerance."""
import functools

import numpy as np
import pytest

import classify_ref as CR
import classify_rf_ref as RF
from rcppml_amd import _abi, classify as K

pytestmark = pytest.mark.gpu

FOREST_KEYS = ("feature", "threshold", "left", "leaf_class", "n_nodes", "lo", "hi", "votes", "predictions")
# n_train, p, C, ntree, mtry (None: floor(sqrt(p))), flavour.  63 / 65 / 257 rows cross the one-wave boundary; 257 rows leave about
# 162 in-bag rows at the root, above the 128-entry switch to the workgroup search, and the lower levels fall below it.
CASES = [
    (63, 1, 2, 1, None, "blobs"),
    (65, 17, 7, 33, 4, "blobs"),
    (257, 128, 7, 3, None, "blobs"),
    (128, 5, 64, 5, 2, "blobs"),             # two rows per class
    (257, 6, 3, 9, 2, "blobs"),
    (120, 4, 3, 7, 2, "dup"),                # a constant feature; duplicated rows with conflicting labels: impure leaves, tied votes
    (9000, 6, 5, 1, 2, "noise"),             # random labels: a tree of more than 4096 nodes, which prediction reads from global memory
]


@functools.lru_cache(maxsize=None)
def case(i):
    n, p, C, ntree, mtry, flavour = CASES[i]
    x, lab = CR.blobs(n + 40, p, C, 1.0, 100 + i)
    if flavour == "dup":
        x[:, 1] = 3.0
        x[20:40], lab[20:40] = x[0:20], (lab[0:20] + 1) % C
        x[n:n + 5, 0] = [-50.0, 50.0, x[:n, 0].min(), x[:n, 0].max(), 0.0]          # test rows outside and on the bin range
    if flavour == "noise":
        lab = np.random.default_rng(i).integers(0, C, n + 40).astype(np.int32)
    tr, te, ltr, lte = x[:n], x[n:], lab[:n], lab[n:]
    return tr, te, ltr, lte, RF.forest(tr, te, ltr, C, ntree, mtry, seed=7 + i)


def device(i, **kw):
    n, p, C, ntree, mtry, _ = CASES[i]
    tr, te, ltr, lte, _ = case(i)
    return _abi._check(_abi.classify_rf(tr, te, ltr, lte, C, ntree, 0 if mtry is None else mtry, 7 + i, forest=True, **kw), "rf")


@pytest.mark.parametrize("i", range(len(CASES)))
def test_forest_is_the_restatement_exactly(i):
    ref, got = case(i)[4], device(i)
    for key in FOREST_KEYS:
        assert np.array_equal(got[key], ref[key]), key
    assert np.array_equal(got["prob"], ref["prob"]) and got["launches"] > 0
    if CASES[i][5] == "dup":
        leaves = (ref["feature"] < 0) & (ref["leaf_class"] >= 0)
        assert np.all(ref["lo"][1] == ref["hi"][1]) and not np.any(ref["feature"] == 1) and leaves.any()
    if CASES[i][5] == "noise":
        assert ref["n_nodes"][0] > 4096


@pytest.mark.parametrize("i", [1, 4])
def test_one_tree_per_batch_changes_nothing(i):
    whole, single = device(i), device(i, tree_batch=1)
    for key in FOREST_KEYS + ("prob", "confusion", "auc"):
        assert whole[key].tobytes() == single[key].tobytes(), key


def test_public_function_matches_the_restatement():
    x, lab = CR.blobs(240, 6, 4, 1.0, 11)
    levels = np.array(["a", "b", "c", "d"])
    out = K.classify_rf(x, levels[lab], test_fraction=0.25, ntree=15, seed=3, return_forest=True)
    tr, te = out["train_idx"], out["test_idx"]
    ref = RF.forest(x[tr], x[te], lab[tr], 4, 15, None, seed=3)
    m = CR.metrics(ref["predictions"], lab[te], ref["prob"], 4)
    assert out["method"] == "random_forest" and (out["ntree"], out["mtry"]) == (15, 2)
    assert out["accuracy"] == m["accuracy"] and np.array_equal(out["confusion"], m["confusion"])
    assert np.array_equal(out["per_class_auc"], m["auc"]) and np.array_equal(out["votes"], ref["votes"])
    assert np.array_equal(out["feature"], ref["feature"]) and np.array_equal(out["predictions"], levels[ref["predictions"]])


@pytest.mark.parametrize("kw, msg", [(dict(p=129), "dim must be in [1, 128]"), (dict(C=65), "n_classes must be in [2, 64]"),
                                     (dict(ntree=0), "ntree must be in [1, 4096]")])
def test_refusals_name_the_argument_and_leave_outputs_untouched(kw, msg):
    p, C, ntree = kw.get("p", 3), kw.get("C", 3), kw.get("ntree", 5)
    r = _abi.classify_rf(np.ones((20, p)), np.ones((4, p)), np.arange(20) % 3, np.arange(4) % 3, C, ntree, forest=True)
    assert (r["status"], r["error"]) == (-1, msg)
    assert len(r["buffers"]) == 16 and all(np.all(b == -7) for b in r["buffers"].values())
