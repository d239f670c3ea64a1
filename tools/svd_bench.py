#!/usr/bin/env python3
"""tools/svd_bench.py -- truncated SVD / PCA on the GPU path (rcppml_gpu_svd_pca_{float,double}, csrc/ops_svd.hip).

Workloads, all of pbmc3k (tests/golden/pbmc3k.spz, 13714 x 2700, 2.28 M nonzeros):
  pca(k = 10) with Lanczos (R's GPU default below k = 32; maxit 0: the 3k / k + 50 step cap, tol 1e-5)
  svd(k = 5, nonneg) with deflation (R's choice for constrained k < 8; maxit 200, tol 1e-5)
each in fp32 and fp64.  Per workload, after one warm-up call: the best and all of three wall times of the whole entry call (host CSC
checks, upload, device transpose, the solve, the download), iterations (deflation: per factor; Lanczos: steps), and the entry's own
out_wall_time_ms.  --cpu also times the numpy restatement of the reference's CPU deflation (tests/svd_ref.py, dense numpy on the
machine's BLAS threads -- not the reference's C++) and, for Lanczos, numpy's dense LAPACK SVD of the centered matrix; both are
labelled as such.  Prints one JSON line per workload.

--auto runs one leg only: pca(k = "auto") through the Python surface (rcppml_gpu_svd_cv_ex: cross-validated deflation, k_max 50,
test_fraction 0.05, patience 3, fp64), and prints one JSON line with the call's wall time (best of three after a warm-up),
k_selected, the factors computed, and the time and rank of the numpy restatement (tests/svd_cv_ref.py; not the reference's C++).

--krylov runs one leg only: svd(k = 16, nonneg) in fp32 with the constrained block method KSPR (rcppml_gpu_svd_krylov_ex, default
pass limit, tol 1e-5), with deflation under the same constraints on the same device (what the fit cost before KSPR), and with the
numpy restatement of KSPR from the device's Lanczos seed (tests/svd_krylov_ref.py; not the reference's C++).  One JSON line: wall
times (best of three after a warm-up), the pass count, ms per pass (the call with the default limit minus a one-pass call, over the
passes in between: the seed and the transfers cancel) and the relative Frobenius error of both fits.

--reg runs one leg only: pca(k = 6, method = "deflation") in fp32 through the Python surface, three times: plain; with L21 and
angular; with those plus a banded Laplacian on the cell side (every cell joined to its next two, graph_lambda * lambda_max <= 0.25)
-- the last two through rcppml_gpu_svd_reg_ex.  One JSON line: per run the wall ms (best of three after a warm-up), the total
iterations and the ms per iteration, and the marginal ms per iteration from two fixed iteration counts (tol = 0, maxit 10 and 30:
uploads, transposes and the per-factor work cancel), which is the figure to hold the on-terms against the plain run with.

--randomized runs one leg only: pca(k = 40, method = "randomized") through the Python surface (rcppml_gpu_svd_randomized_ex, 3 power
iterations, sketch dimension 50) in fp32 and fp64, beside pca(k = 40, method = "lanczos") and beside the reference entry with
algorithm 3 (Lanczos under the name randomized: what the same call ran before the block method existed, and what method = "auto"
still runs at this k).  The calls alternate within one process, best of three after a warm-up each.  One JSON line: the wall times,
the kernel launches of the randomized fit (10 q + 10: the sketch, 2 q + 2 products, 2 q + 1 orthonormalisations of four launches,
the final Gram and two rotations), the Lanczos steps, the largest relative deviation of each d from the true singular values' top
40 where --cpu computes them, and under --cpu the time of the numpy restatement (tests/svd_rand_ref.py; not the reference's C++)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from rcppml_amd import _abi, data  # noqa: E402


def pbmc3k():
    from oracle import oracle as O
    buf = np.fromfile(os.path.join(ROOT, "tests", "golden", "pbmc3k.spz"), dtype=np.uint8)
    st, m, n, nnz, vt = O.spz_info(buf)
    p, i, x = O.spz_decode(buf)
    return data.CSC((m, n), np.asarray(p, np.int32), np.asarray(i, np.int32), np.asarray(x, np.float64))


def timed(fn, reps=3):
    fn()
    out, ts = None, []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return out, ts


def auto_leg(A):
    import scipy.sparse as sp
    import svd_cv_ref
    from rcppml_amd import svd as S
    r, ts = timed(lambda: S.pca(A, k="auto", precision="double"))
    mi = r["misc"]
    M = sp.csc_matrix((A.x, A.i, A.p), shape=(A.rows, A.cols))
    t0 = time.perf_counter()
    ref = svd_cv_ref.cv_deflation_svd(M.toarray(), min(50, A.rows, A.cols), stored=(M != 0).toarray(), center=True,
                                      test_fraction=0.05, patience=3)
    cpu_s = time.perf_counter() - t0
    print(json.dumps(dict(workload="pca k=auto deflation cv", precision="double", m=A.rows, n=A.cols, nnz=int(A.x.shape[0]),
                          wall_s=min(ts), wall_s_all=ts, entry_wall_ms=mi["wall_time_ms"], k_selected=int(mi["k_selected"]),
                          k_computed=int(len(mi["test_loss"])), n_test=int(mi["n_test"]), test_loss=mi["test_loss"].tolist(),
                          cpu_s=cpu_s, cpu_k_selected=int(ref["k_selected"]), cpu_k_computed=int(ref["k_computed"]),
                          cpu_label="numpy restatement of the reference CPU deflation with CV (tests/svd_cv_ref.py), not the "
                                    "reference's C++")), flush=True)


def krylov_leg(A):
    import scipy.sparse as sp
    import svd_krylov_ref
    parts = (A.p, A.i, A.x, A.rows, A.cols)
    k, kw = 16, dict(precision="float", tol=1e-5, seed=0, nonneg=(True, True))
    r, ts = timed(lambda: _abi.svd_krylov(parts, k, max_iter=0, **kw))
    assert r["status"] == 0, r["error"]
    one, t1 = timed(lambda: _abi.svd_krylov(parts, k, max_iter=1, **kw))
    assert one["status"] == 0, one["error"]
    dfl, td = timed(lambda: _abi.svd_pca(parts, k, algorithm=0, max_iter=200, **kw))
    assert dfl["status"] == 0, dfl["error"]
    lz = _abi.svd_pca(parts, k, algorithm=2, max_iter=0, precision="float", tol=1e-5, seed=0)
    assert lz["status"] == 0, lz["error"]
    M = sp.csc_matrix((A.x, A.i, A.p), shape=(A.rows, A.cols))
    dense = M.toarray()
    t0 = time.perf_counter()
    ref = svd_krylov_ref.kspr(dense, lz["V"][:, :lz["k"]], 0, 1e-5, nonneg=(True, True), dtype=np.float32)
    cpu_s = time.perf_counter() - t0
    fro = np.linalg.norm(dense)

    def err(x):
        kk = x["k"]
        return float(np.linalg.norm(dense - (x["U"][:, :kk] * x["d"][:kk]) @ x["V"][:, :kk].T) / fro)
    passes = int(r["passes"])
    print(json.dumps(dict(workload="svd k=16 nonneg krylov (KSPR)", precision="float", m=A.rows, n=A.cols, nnz=int(A.x.shape[0]),
                          wall_s=min(ts), wall_s_all=ts, entry_wall_ms=r["wall_ms"], passes=passes,
                          ms_per_pass=(min(ts) - min(t1)) * 1e3 / max(passes - 1, 1), one_pass_wall_s=min(t1), dw_last=float(r["dw"][-1]),
                          rel_error=err(r), deflation_wall_s=min(td), deflation_wall_s_all=td,
                          deflation_iterations=int(np.sum(dfl["iters"][:dfl["k"]])), deflation_rel_error=err(dfl),
                          cpu_s=cpu_s, cpu_passes=int(ref["passes"]),
                          cpu_label="numpy restatement of KSPR in float32 from the device's Lanczos seed (tests/svd_krylov_ref.py), "
                                    "not the reference's C++")), flush=True)


def reg_leg(A):
    import scipy.sparse as sp
    from rcppml_amd import svd as S
    M = sp.csc_matrix((A.x, A.i, A.p), shape=(A.rows, A.cols))
    n = A.cols
    W = sp.diags([np.ones(n - 1), np.ones(n - 2)], [1, 2], format="csc")
    W = W + W.T
    L = (sp.diags(np.asarray(W.sum(axis=1)).ravel()) - W).tocsc()
    lam = 0.25 / float(np.max(np.abs(L).sum(axis=1)))            # the row-sum bound of lambda_max
    runs = [("plain", dict()), ("L21+angular", dict(L21=0.1, angular=0.2)),
            ("L21+angular+graph_V", dict(L21=0.1, angular=0.2, graph_V=L, graph_lambda=(0, lam)))]
    rec = dict(workload="pca k=6 deflation, regularisers", precision="float", m=A.rows, n=A.cols, nnz=int(A.x.shape[0]),
               graph_lambda=lam, runs=[])
    for name, kw in runs:
        call = lambda **extra: S.pca(M, k=6, method="deflation", precision="float", **kw, **extra)
        r, ts = timed(call)
        its = int(np.sum(r["misc"]["iters_per_factor"]))
        (ra, ta), (rb, tb) = timed(lambda: call(tol=0.0, maxit=10)), timed(lambda: call(tol=0.0, maxit=30))
        ia, ib = (int(np.sum(x["misc"]["iters_per_factor"])) for x in (ra, rb))
        rec["runs"].append(dict(run=name, wall_ms=min(ts) * 1e3, wall_ms_all=[t * 1e3 for t in ts], iterations=its,
                                ms_per_iteration=min(ts) * 1e3 / max(its, 1),
                                marginal_ms_per_iteration=(min(tb) - min(ta)) * 1e3 / max(ib - ia, 1), d=r["d"].tolist()))
    print(json.dumps(rec), flush=True)


def randomized_leg(A, cpu):
    import scipy.sparse as sp
    from rcppml_amd import svd as S
    M = sp.csc_matrix((A.x, A.i, A.p), shape=(A.rows, A.cols))
    parts = (A.p, A.i, A.x, A.rows, A.cols)
    k = 40
    q = _abi.randomized_sizes(A.rows, A.cols, k)[2]
    rec = dict(workload="pca k=40 randomized", m=A.rows, n=A.cols, nnz=int(A.x.shape[0]), sketch=_abi.randomized_sizes(A.rows, A.cols, k)[1],
               power_iterations=q, launches=10 * q + 10, runs=[])
    sv = None
    if cpu:
        import svd_rand_ref
        dense = M.toarray()
        t0 = time.perf_counter()
        ref = svd_rand_ref.randomized_svd(dense, k, center=True)
        rec["cpu_s"] = time.perf_counter() - t0
        rec["cpu_label"] = "numpy restatement of the reference's randomized SVD in float64 (tests/svd_rand_ref.py), not the reference's C++"
        sv = np.linalg.svd(dense - dense.mean(axis=1, keepdims=True), compute_uv=False)[:k]
        rec["cpu_tail_below_true"] = float(1 - ref["d"][-1] / sv[-1])
    for prec in ("float", "double"):
        legs = [("randomized", lambda: S.pca(M, k=k, method="randomized", precision=prec)),
                ("lanczos", lambda: S.pca(M, k=k, method="lanczos", precision=prec)),
                ("algorithm 3 on the reference entry (Lanczos)",
                 lambda: _abi.svd_pca(parts, k, precision=prec, tol=1e-5, max_iter=3, center=True, seed=0, algorithm=3))]
        for _, fn in legs:
            fn()                                                # warm-up
        ts, out = {name: [] for name, _ in legs}, {}
        for _ in range(3):                                      # alternate the three calls
            for name, fn in legs:
                t0 = time.perf_counter()
                out[name] = fn()
                ts[name].append(time.perf_counter() - t0)
        for name, _ in legs:
            r = out[name]
            d = r["d"] if "misc" in r else r["d"][:r["k"]]
            run = dict(run=name, precision=prec, wall_ms=min(ts[name]) * 1e3, wall_ms_all=[t * 1e3 for t in ts[name]],
                       entry_wall_ms=r["misc"]["wall_time_ms"] if "misc" in r else r["wall_ms"],
                       iterations=int((r["misc"]["iters_per_factor"] if "misc" in r else r["iters"])[0]), d_first=float(d[0]),
                       d_last=float(d[-1]))
            if sv is not None:
                run["max_rel_d_from_true"] = float(np.max(np.abs(d - sv) / sv))
            rec["runs"].append(run)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu", action="store_true", help="also time the numpy restatements (slow)")
    ap.add_argument("--auto", action="store_true", help="only the pca(k = \"auto\") leg")
    ap.add_argument("--krylov", action="store_true", help="only the svd(k = 16, nonneg, method = \"krylov\") leg")
    ap.add_argument("--reg", action="store_true", help="only the pca(k = 6, deflation) leg with L21 / angular / graph regularisation")
    ap.add_argument("--randomized", action="store_true", help="only the pca(k = 40, method = \"randomized\") leg")
    args = ap.parse_args()
    A = pbmc3k()
    if args.randomized:
        randomized_leg(A, args.cpu)
        return
    if args.reg:
        reg_leg(A)
        return
    if args.auto:
        auto_leg(A)
        return
    if args.krylov:
        krylov_leg(A)
        return
    parts = (A.p, A.i, A.x, A.rows, A.cols)
    work = [("pca k=10 lanczos", dict(k=10, center=True, algorithm=2, max_iter=0)),
            ("svd k=5 nonneg deflation", dict(k=5, center=False, algorithm=0, max_iter=200, nonneg=(True, True)))]
    dense = None
    for name, w in work:
        for prec in ("float", "double"):
            kw = dict(w)
            k = kw.pop("k")
            r, ts = timed(lambda: _abi.svd_pca(parts, k, precision=prec, tol=1e-5, seed=0, **kw))
            assert r["status"] == 0, r["error"]
            rec = dict(workload=name, precision=prec, m=A.rows, n=A.cols, nnz=int(A.x.shape[0]), wall_s=min(ts), wall_s_all=ts,
                       entry_wall_ms=r["wall_ms"], iterations=r["iters"][:r["k"]].tolist() if kw["algorithm"] == 0 else int(r["iters"][0]),
                       d=r["d"][:r["k"]].tolist())
            if args.cpu and prec == "double":
                import svd_ref
                if dense is None:
                    import scipy.sparse as sp
                    dense = sp.csc_matrix((A.x, A.i, A.p), shape=(A.rows, A.cols)).toarray()
                if kw["algorithm"] == 0:
                    t0 = time.perf_counter()
                    ref = svd_ref.deflation_svd(dense, k, tol=1e-5, maxit=200, nonneg=(True, True))
                    rec["cpu_s"] = time.perf_counter() - t0
                    rec["cpu_label"] = "numpy restatement of the reference CPU deflation (tests/svd_ref.py), not the reference's C++"
                    rec["cpu_same_iterations"] = ref["iters"].tolist() == rec["iterations"]
                    rec["cpu_max_rel_d"] = float(np.max(np.abs(ref["d"] - r["d"][:k]) / ref["d"]))
                else:
                    t0 = time.perf_counter()
                    sv = np.linalg.svd(dense - dense.mean(axis=1, keepdims=True), compute_uv=False)
                    rec["cpu_s"] = time.perf_counter() - t0
                    rec["cpu_label"] = "numpy dense LAPACK SVD of the centered matrix (all singular values), not the reference's C++"
                    rec["cpu_max_rel_d"] = float(np.max(np.abs(sv[:k] - r["d"][:k]) / sv[:k]))
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
