"""CPU checks of the embedding assessment feature: the ABI declarations and exports, the std::mt19937 / std::shuffle restatement
against the library's host-only plan entry, ARI / NMI, the refusals (all decided before any device work) and the Python surface's
R messages, class filter and metric keys.  No GPU needed."""
import os
import re

import numpy as np
import pytest

import assess_ref as R
from rcppml_amd import _abi
from rcppml_amd import assess as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rcppml_gpu_assess", "rcppml_gpu_assess_ex", "rcppml_gpu_knn_float", "rcppml_gpu_assess_plan")


def test_header_declares_the_reference_pointer_list():
    src = open(os.path.join(ROOT, "include", "rcppml_gpu.h")).read()
    m = re.search(r"RCPPML_GPU_API void rcppml_gpu_assess\((.*?)\);", src, flags=re.S)
    assert m
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 26 and all("*" in a for a in args)
    assert args[0].startswith("const double*") and args[-1] == "int* out_status"
    names = [a.split("*")[-1].strip() for a in args]
    assert names[18:25] == ["out_ari", "out_nmi", "out_silhouette", "out_knn_accuracy", "out_knn_f1", "out_batch_sil",
                            "out_batch_entropy"]


def test_library_exports_the_entries():
    L = _abi.lib()
    for name in NEW:
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(L, name), name


def test_mt19937_standard_value():
    g = R.MT19937()
    for _ in range(9999):
        g()
    assert g() == 4123659995


@pytest.mark.parametrize("n", [1, 2, 7, 1000, 65535, 65536, 70000])
def test_kmeans_init_matches_the_library(n):
    labels = np.arange(n) % 3
    r = _abi.assess_plan(labels, 3, nstart=3, spc=5, folds=2, seed=42)
    assert r["status"] == 0, r["error"]
    assert np.array_equal(r["init"], R.kmeans_init(n, 3, 3, 42))


def test_shuffle_takes_both_branches():
    # (2^32 - 1) // n >= n up to n = 65535: one engine draw per two positions; above it one draw per position (plus rejections)
    class Counting(R.MT19937):
        draws = 0

        def __call__(self):
            self.draws += 1
            return super().__call__()

    for n, lo, hi in ((65535, 32767, 49000), (65536, 65535, 70000)):
        g = Counting(1)
        R.shuffle(list(range(n)), g)
        assert lo <= g.draws <= hi, (n, g.draws)


@pytest.mark.parametrize("n,seed", [(1000, 42), (70000, 7), (1000, -1)])
def test_plan_matches_restatement(n, seed):
    rng = np.random.default_rng(n)
    labels = rng.integers(0, 12, n)
    labels[labels >= 10] = 0
    labels[:3] = 11                       # class 11: fewer points than spc
    labels[5] = 10                        # class 10: a class of size 1
    spc = 200
    r = _abi.assess_plan(labels, 12, nstart=4, spc=spc, folds=5, seed=seed)
    assert r["status"] == 0, r["error"]
    assert np.array_equal(r["init"], R.kmeans_init(n, 12, 4, seed))
    smp, cnt = R.sil_plan(labels, 12, spc, seed)
    assert np.array_equal(r["sil_counts"], cnt)
    assert cnt[10] == 1 and cnt[11] < spc
    assert np.array_equal(r["sil_samples"], smp)
    assert np.array_equal(r["fold_ids"], R.fold_plan(labels, 12, 5, seed))


def test_plan_small_spc_and_negative_spc():
    labels = np.array([0, 0, 0, 1, 1, 2])
    for spc in (0, 1, 2, -3):
        r = _abi.assess_plan(labels, 3, nstart=1, spc=spc, folds=3, seed=3)
        assert r["status"] == 0
        smp, cnt = R.sil_plan(labels, 3, spc, 3)
        assert np.array_equal(r["sil_counts"], cnt) and np.array_equal(r["sil_samples"], smp)


def test_plan_refusals_write_nothing():
    labels = np.array([0, 1, 2, 3])
    r = _abi.assess_plan(labels, 3)
    assert r["status"] == -1 and "label" in r["error"]
    assert all(np.all(b == -7) for b in r["buffers"])
    r = _abi.assess_plan(np.array([0, 1, 1]), 2, nstart=2, capacity=(3, 10, 3))
    assert r["status"] == -1 and "init_capacity" in r["error"]
    assert all(np.all(b == -7) for b in r["buffers"])


def test_ari_nmi_restatement():
    a = np.array([0, 0, 1, 1, 2, 2, 2])
    assert R.ari(a, a) == pytest.approx(1.0) and R.nmi(a, a) == pytest.approx(1.0)
    perm = np.array([2, 0, 1])[a]
    assert R.ari(a, perm) == pytest.approx(1.0) and R.nmi(a, perm) == pytest.approx(1.0)
    # truth [0,0,1,1], pred [0,1,0,1]: table [[1,1],[1,1]] -> sum_ij 0, rows 2, cols 2, expected 2*2/6, max 2 -> ARI -0.5
    t, p = np.array([0, 0, 1, 1]), np.array([0, 1, 0, 1])
    assert R.ari(t, p) == pytest.approx(-0.5)
    assert R.nmi(t, p) == pytest.approx(0.0, abs=1e-15)
    # truth [0,0,0,1,1,1], pred [0,0,1,1,1,1]: table [[2,1],[0,3]]
    t, p = np.array([0, 0, 0, 1, 1, 1]), np.array([0, 0, 1, 1, 1, 1])
    sij, si, sj, cn = 1 + 0 + 0 + 3, 3 + 3, 1 + 6, 15
    exp = si * sj / cn
    assert R.ari(t, p) == pytest.approx((sij - exp) / (0.5 * (si + sj) - exp))
    pij = np.array([[2, 1], [0, 3]]) / 6
    pi, pj = pij.sum(1), pij.sum(0)
    mi = sum(pij[i, j] * np.log(pij[i, j] / (pi[i] * pj[j])) for i in range(2) for j in range(2) if pij[i, j] > 0)
    h = lambda q: -sum(x * np.log(x) for x in q if x > 0)
    assert R.nmi(t, p) == pytest.approx(mi / np.sqrt(h(pi) * h(pj)))


def _call(**kw):
    base = dict(emb=np.ones((6, 2)), labels=np.array([0, 0, 0, 1, 1, 1]), n_classes=2, batch=np.array([0, 1] * 3), n_batch=2)
    base.update(kw)
    return _abi.assess_raw(base.pop("emb"), base.pop("labels"), base.pop("n_classes"), base.pop("batch"), base.pop("n_batch"),
                           init=-7.0, **base)


@pytest.mark.parametrize("kw,msg", [
    (dict(emb=np.ones((0, 2))), "n must be"),
    (dict(emb=np.ones((6, 0))), "dim must be"),
    (dict(maxiter=0), "kmeans_maxiter"),
    (dict(n_classes=0, silhouette=False, classify=False), "n_classes must be"),
    (dict(knn_k=0), "knn_k"),
    (dict(folds=0), "knn_folds"),
    (dict(batch_k=0), "batch_knn_k"),
    (dict(labels=np.array([0, 0, 0, 1, 1, 2])), "label lies outside"),
    (dict(labels=np.array([0, 0, 0, 1, 1, -1]), clustering=False, classify=False), "label lies outside"),
    (dict(batch=np.array([0, 1, 0, 1, 0, 2])), "batch label"),
])
def test_refusals(kw, msg):
    r = _call(**kw)
    assert r["status"] == -1 and msg in r["error"], r["error"]
    assert all(r[k] == -7.0 for k in ("ari", "nmi", "silhouette", "knn_accuracy", "knn_f1", "batch_sil", "batch_entropy"))


# a 3 x 2 embedding with one defect each (the assessment takes no CSC: these are its own argument checks)
@pytest.mark.parametrize("kw, msg", [
    (dict(labels=np.array([0, 1, 2])), "a label lies outside [0, n_classes)"),
    (dict(batch=np.array([0, 1, 2])), "a batch label lies outside [0, n_batch)"),
    (dict(maxiter=0), "kmeans_maxiter must be >= 1 for clustering"),
    (dict(knn_k=0), "knn_k must be >= 1 for classification"),
    (dict(folds=0), "knn_folds must be >= 1 for classification"),
    (dict(batch_k=0), "batch_knn_k must be >= 1 for batch mixing"),
])
def test_refusals_are_exact(kw, msg):
    """Refused before any device work (so with or without a GPU): status -1, this message, nothing written."""
    base = dict(emb=np.arange(6.0).reshape(3, 2), labels=np.array([0, 1, 1]), n_classes=2, batch=np.array([0, 1, 0]), n_batch=2)
    base.update(kw)
    emb, labels, nc, batch, nb = (base.pop(k) for k in ("emb", "labels", "n_classes", "batch", "n_batch"))
    r = _abi.assess_raw(emb, labels, nc, batch, nb, init=-7.0, **base)
    assert (r["status"], r["error"]) == (-1, msg)
    assert all(r[k] == -7.0 for k in ("ari", "nmi", "silhouette", "knn_accuracy", "knn_f1", "batch_sil", "batch_entropy"))
    r = _abi.assess_ex(emb, labels, nc, batch, nb, init=-7.0, **base)
    assert (r["status"], r["error"]) == (-1, msg)
    assert all(r[k] == -7.0 for k in ("ari", "nmi", "silhouette", "knn_accuracy", "knn_f1", "batch_sil", "batch_entropy"))
    b = r["buffers"]
    assert all(np.all(b[k] == -7) for k in ("assignments", "fold_ids", "fold_accuracy", "fold_f1"))
    assert all(np.all(np.isnan(b[k])) for k in ("restart_ari", "restart_nmi", "sil_point", "batch_entropy_point", "batch_sil_point"))


def test_refusal_messages_are_distinct():
    msgs = {_call(**kw)["error"] for kw in (dict(maxiter=0), dict(knn_k=0), dict(folds=0), dict(batch_k=0),
                                            dict(emb=np.ones((6, 0))), dict(emb=np.ones((0, 2))))}
    assert len(msgs) == 6


def test_knn_refusals_write_nothing():
    q = np.zeros((4, 2), np.float32)
    for kw, msg in ((dict(k=0), "k must"), (dict(k=2, capacity=7), "out_capacity"), (dict(k=2, mask="self", train=q), "train = NULL"),
                    (dict(k=2, mask="group", group=np.array([0, 0, 1, 1]), group_k=np.array([1, 3])), "group_k")):
        r = _abi.knn_float(q, **kw)
        assert r["status"] == -1 and msg in r["error"], r["error"]
        assert np.all(r["buffers"][0] == -7) and np.all(np.isnan(r["buffers"][1]))


def test_surface_messages():
    x = np.zeros((20, 3))
    with pytest.raises(ValueError, match=r"length\(labels\) must equal nrow of embedding \(20\)"):
        A.assess(x, np.zeros(19))
    with pytest.raises(ValueError, match="Fewer than 2 classes with >= 10 samples"):
        A.assess(x, np.array(["a"] * 15 + ["b"] * 5))
    with pytest.raises(ValueError, match="lr"):
        A.assess(x, np.array(["a"] * 10 + ["b"] * 10), classifiers=("knn", "lr"))


def test_surface_filter_keys_and_extraction(monkeypatch, capsys):
    seen = {}

    def fake(emb, codes, n_classes, batch, n_batch, **kw):
        seen.update(emb=emb, codes=codes, n_classes=n_classes, batch=batch, n_batch=n_batch, **kw)
        return dict(status=0, error="", ari=0.5, nmi=0.6, silhouette=0.1, knn_accuracy=0.9, knn_f1=0.8, batch_sil=0.2,
                    batch_entropy=0.7)

    monkeypatch.setattr(_abi, "assess_raw", fake)
    labels = np.array(["t"] * 12 + ["b"] * 3 + ["a"] * 11)
    x = np.arange(26 * 2, dtype=float).reshape(26, 2)
    batch = np.array(["y", "x"] * 13)
    r = A.assess(x, labels, batch=batch)
    assert "Dropped 3 samples from 1 small classes (min_class_size=10)" in capsys.readouterr().err
    assert seen["n_classes"] == 2 and seen["emb"].shape == (23, 2)
    assert np.array_equal(seen["codes"], np.array([1] * 12 + [0] * 11))          # sorted levels a < t
    assert seen["n_batch"] == 2 and seen["batch"][0] == 1                          # "y" -> 1
    assert seen["nstart"] == 10 and seen["maxiter"] == 100 and seen["batch_mixing"]
    m = r["metrics"]
    assert list(m) == ["ari", "nmi", "silhouette", "accuracy_knn", "f1_knn", "precision_knn", "recall_knn", "auroc_knn",
                       "accuracy_mean", "f1_mean", "precision_mean", "recall_mean", "auroc_mean", "batch_silhouette",
                       "batch_knn_entropy"]
    assert m["accuracy_knn"] == 0.9 and np.isnan(m["precision_mean"]) and np.isnan(m["auroc_knn"])
    assert r["params"]["backend"] == "gpu"
    r = A.assess(x, labels, metrics=("ari", "sil"))
    assert list(r["metrics"]) == ["ari", "silhouette"] and not seen["classify"] and not seen["batch_mixing"]
    # nmf() result t(d * h) and svd() result u * d
    h = np.arange(6.0).reshape(2, 3)
    assert np.array_equal(A._embedding(dict(w=None, d=np.array([2.0, 3.0]), h=h)), (np.array([[2.0], [3.0]]) * h).T)
    u = np.ones((3, 2))
    assert np.array_equal(A._embedding(dict(u=u, d=np.array([2.0, 5.0]), v=None)), u * [2.0, 5.0])
