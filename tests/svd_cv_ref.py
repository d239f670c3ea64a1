"""numpy restatement of the reference's cross-validated / auto-rank and obs-masked CPU deflation SVD -- the parity target of
rcppml_gpu_svd_cv_ex / rcppml_gpu_svd_cv_dense_ex (rcppml_amd/csrc/ops_svd.hip, kernels_svd_cv.hip.h).  Test infrastructure only:
the product path never imports it.  With test_fraction = 0 and no mask it is svd_ref.deflation_svd, operation for operation.

Sources restated (reference tree, inst/include/FactorNet/):
  rng/rng.hpp:129-170            SplitMix64::hash(seed, i, j) and is_holdout: hash < UINT64_MAX // inv_prob
  nmf/speckled_cv.hpp:121        inv_prob = (uint64)(1.0 / test_fraction)
  core/svd_config.hpp:149-151    effective_cv_seed
  svd/test_entries.hpp:84-141    test entries: held-out stored entries (sparse, either mask_zeros) or every held-out (i, j) (dense),
                                 column-major, value minus row mean when centred; :43-65 update and compute_mse
  svd/test_entries.hpp:264-315   training matrix: same pattern, held-out values 0
  svd/deflation.hpp:377-417      row means and the norm from the full A
  svd/deflation.hpp:452-487      obs_mask zeroes training values first
  svd/deflation.hpp:552-559      the denominator correction;  :713-784 where it applies;  :869-911 test loss, patience, sigma stop
"""
import numpy as np

from rcppml_amd.data import splitmix64_uniform
from svd_ref import regularize

M64 = (1 << 64) - 1


def cv_hash(seed, i, j):
    """SplitMix64::hash over arrays of row / column indices (uint64 arithmetic wraps)."""
    with np.errstate(over="ignore"):
        h = (np.uint64(seed & M64) + np.asarray(i, np.uint64) * np.uint64(0x9e3779b97f4a7c15)
             + np.asarray(j, np.uint64) * np.uint64(0x6c62272e07bb0142))
        h = (h ^ (h >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
        h = (h ^ (h >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
        return h ^ (h >> np.uint64(31))


def is_holdout(seed, i, j, inv_prob):
    if inv_prob == 0:
        return np.zeros(np.broadcast(i, j).shape, bool)
    return cv_hash(seed, i, j) < np.uint64(M64 // int(inv_prob))


def effective_cv_seed(seed, cv_seed):
    seed, cv_seed = int(seed) & 0xFFFFFFFF, int(cv_seed) & 0xFFFFFFFF
    return cv_seed if cv_seed != 0 else ((seed ^ 0xBEEF) if seed != 0 else 42)


def holdout_grid(m, n, seed, test_fraction):
    """(m, n) bool: the hold-out rule over the whole grid."""
    if not test_fraction > 0:
        return np.zeros((m, n), bool)
    ii, jj = np.meshgrid(np.arange(m), np.arange(n), indexing="ij")
    return is_holdout(seed, ii, jj, int(1.0 / test_fraction))


def cv_deflation_svd(A, k, stored=None, tol=1e-5, maxit=200, center=False, seed=0, L1=(0, 0), L2=(0, 0), nonneg=(False, False),
                     ub=(0, 0), test_fraction=0.0, cv_seed=0, patience=3, mask_zeros=False, obs_mask=None, dtype=np.float64):
    """A: dense (m, n) array.  stored: (m, n) bool pattern of the stored entries of a sparse input, None for a dense input.
    obs_mask: (m, n) bool pattern or None.  Returns dict(u, d, v, iters, frob, row_means, k_selected, k_computed, test_loss, n_test,
    n_masked, stopped_by_patience, rows, cols)."""
    A = np.asarray(A, np.float64)
    m, n = A.shape
    Ad = A.astype(dtype)
    mu = A.mean(axis=1).astype(dtype) if center else None
    frob = float(np.sum(A * A)) - (n * float(np.sum(A.mean(axis=1) ** 2)) if center else 0.0)
    eps100 = np.finfo(dtype).eps * 100
    rs = 42 if seed == 0 else int(seed)
    drawn = [0]
    do_cv = test_fraction > 0
    pattern = np.ones((m, n), bool) if stored is None else np.asarray(stored, bool)
    # ---- obs_mask, test entries from the original A, training matrix
    At = Ad.copy()
    n_masked = 0
    if obs_mask is not None:
        hit = np.asarray(obs_mask, bool) & pattern
        At[hit] = 0
        n_masked = int(hit.sum())
    rows = cols = np.zeros(0, np.int64)
    res = np.zeros(0, dtype)
    dc = dtype(1)
    if do_cv:
        held = holdout_grid(m, n, effective_cv_seed(seed, cv_seed), test_fraction) & pattern
        cols, rows = np.nonzero(held.T)                  # column-major order
        res = Ad[rows, cols] - (mu[rows] if center else dtype(0))
        At[held] = 0
        nnz = int(pattern.sum())
        dens = dtype(nnz) / (dtype(m) * dtype(n))
        dc = dtype(1) - dtype(test_fraction) * (dens if mask_zeros else dtype(1))

    def rand_u():
        r = splitmix64_uniform(rs, drawn[0], m).astype(dtype)
        drawn[0] += m
        return r

    def at(u):
        y = At.T @ u
        return y - mu @ u if center else y

    def ax(v):
        y = At @ v
        return y - mu * v.sum() if center else y

    U = np.zeros((m, k), dtype)
    V = np.zeros((n, k), dtype)
    d = np.zeros(k, dtype)
    iters, losses = [], []
    kcomp = best_k = waited = 0
    best = np.finfo(dtype).max
    by_patience = False
    for f in range(k):
        Uk, Vk, dk = U[:, :f], V[:, :f], d[:f]
        corr_v = lambda y, x: y - Vk @ (dk * (Uk.T @ x))           # deflation_correct, v side
        corr_u = lambda y, x: y - Uk @ (dk * (Vk.T @ x))
        if f == 0:
            u = rand_u()
        else:
            u = U[:, f - 1].copy()
            for r in range(f):
                u = u - (u @ U[:, r]) * U[:, r]
            ni = np.sqrt(u @ u)
            if ni > eps100:
                u = u / ni
                v = corr_v(at(u), u)
                nv = np.sqrt(v @ v)
                if nv > 0:
                    v = v / nv
                u = corr_u(ax(v), v)
                for r in range(f):
                    u = u - (u @ U[:, r]) * U[:, r]
            else:
                u = rand_u()
        nu = np.sqrt(u @ u)
        if nu > 0:
            u = u / nu
        tol_k = dtype(tol)
        if f > 0 and d[0] > 0 and d[f - 1] > 0:
            tol_k = min(dtype(tol) * d[0] / d[f - 1], dtype(tol) * dtype(100))
        u_prev = u.copy()
        v = np.zeros(n, dtype)
        it = 0
        while it < maxit:
            u_old = u
            beta = dtype(it - 1) / dtype(it + 2) if it > 1 else dtype(0)
            uh = u + beta * (u - u_prev)
            u_prev = u
            usq = (uh @ uh) * dc
            if not usq > 0:
                v = np.zeros(n, dtype)
                break
            v = corr_v(at(uh), uh) / usq
            v = regularize(v, L1[1], L2[1], nonneg[1], ub[1], usq)
            sv = np.sqrt(v @ v)
            if not sv > 0:
                break
            v = v / sv
            vsq = (v @ v) * dc
            u = corr_u(ax(v), v) / vsq
            u = regularize(u, L1[0], L2[0], nonneg[0], ub[0], vsq)
            su = np.sqrt(u @ u)
            if not su > 0:
                break
            u = u / su
            if 1 - abs(u @ u_old) < tol_k:
                it += 1
                break
            it += 1
        if f > 0:
            for _ in range(2):
                u = u - Uk @ (Uk.T @ u)
            nn = np.sqrt(u @ u)
            if nn > eps100:
                u = u / nn
            for _ in range(2):
                v = v - Vk @ (Vk.T @ v)
            nn = np.sqrt(v @ v)
            if nn > eps100:
                v = v / nn
        sigma = abs(u @ corr_u(ax(v), v))
        U[:, f], V[:, f], d[f] = u, v, sigma
        iters.append(it)
        kcomp = f + 1
        if do_cv:
            res = res - sigma * u[rows] * v[cols]
            mse = (np.sum(res * res, dtype=dtype) / dtype(res.size)) if res.size else dtype(0)
            losses.append(mse)
            if mse < best:
                best, best_k, waited = mse, f + 1, 0
            else:
                waited += 1
                if waited >= patience:
                    by_patience = True
                    break
        else:
            best_k = f + 1
        if sigma < eps100:
            break
    return dict(u=U[:, :best_k], d=d[:best_k], v=V[:, :best_k], iters=np.array(iters), frob=frob,
                row_means=A.mean(axis=1) if center else None, k_selected=best_k, k_computed=kcomp,
                test_loss=np.array(losses, dtype), n_test=int(rows.size), n_masked=n_masked, stopped_by_patience=by_patience,
                rows=rows, cols=cols)


# ------------------------------------------------------------------------------------------------ the parity inputs
def planted(m, n, sig, seed, noise=0.05):
    """As test_gpu_svd.ground_truth: QR factors times singular values, plus Gaussian noise."""
    rng = np.random.default_rng(seed)
    Uq, _ = np.linalg.qr(rng.standard_normal((m, len(sig))))
    Vq, _ = np.linalg.qr(rng.standard_normal((n, len(sig))))
    return (Uq * np.asarray(sig, float)) @ Vq.T + noise * rng.standard_normal((m, n))


DENSE_SEED, SPARSE_SEED = 1, 1
CV_KW = dict(test_fraction=0.1, patience=3, tol=1e-5, maxit=200)
K_MAX = 12


def dense_input():
    return planted(60, 40, (50.0, 30, 15, 8, 4), DENSE_SEED)


def sparse_input():
    """(A with unstored entries 0, stored pattern): 96 x 72 kept at density 0.5."""
    A = planted(96, 72, (80.0, 50, 30, 20), SPARSE_SEED)
    keep = np.random.default_rng(SPARSE_SEED + 1000).random(A.shape) < 0.5
    return A * keep, keep
