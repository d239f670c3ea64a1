"""numpy restatement of the reference's CPU deflation SVD -- the parity target of the GPU deflation path
(rcppml_amd/csrc/ops_svd.hip, algorithm 0).  Test infrastructure only: the product path never imports it.

Sources restated (reference tree, inst/include/FactorNet/svd/):
  deflation.hpp:192-236  apply_regularization(): L2 shrink, L1 soft threshold, nonneg, upper bound (in that order)
  deflation.hpp:306-321  deflation_correct(): raw -= F diag(sigma) (PX' x)
  deflation.hpp:600-915  deflation_svd(): SplitMix64(seed, 0 -> 42) start, power-step warm start of later factors (random again
                         when the orthogonalised previous u vanishes), Nesterov momentum (iter - 1) / (iter + 2) from iter 2,
                         adaptive tol_k, 1 - |u . u_old| < tol_k, two-pass Gram-Schmidt after each factor, Rayleigh-quotient sigma,
                         early stop when sigma < 100 eps
  spmv.hpp:236-435       centering as scalar corrections: A'u - (mu . u) 1, A v - mu sum(v)
"""
import numpy as np

from rcppml_amd.data import splitmix64_uniform


def regularize(x, L1, L2, nonneg, ub, nsq):
    if L2 > 0:
        x = x * (1.0 / (1.0 + L2 / nsq))
    if L1 > 0:
        th = L1 / (2.0 * nsq)
        x = np.where(x > th, x - th, np.where(x < -th, x + th, 0.0))
    if nonneg:
        x = np.maximum(x, 0.0)
    if ub > 0:
        x = np.minimum(x, ub)
    return x


def deflation_svd(A, k, tol=1e-5, maxit=200, center=False, seed=0, L1=(0, 0), L2=(0, 0), nonneg=(False, False), ub=(0, 0),
                  dtype=np.float64):
    """A: dense (m, n) array (densified CSC).  Returns dict(u, d, v, iters, frob, row_means)."""
    A = np.asarray(A, np.float64)
    m, n = A.shape
    Ad = A.astype(dtype)
    mu = A.mean(axis=1).astype(dtype) if center else None
    frob = float(np.sum(A * A)) - (n * float(np.sum(A.mean(axis=1) ** 2)) if center else 0.0)
    eps100 = np.finfo(dtype).eps * 100
    rs = 42 if seed == 0 else int(seed)
    drawn = [0]

    def rand_u():
        r = splitmix64_uniform(rs, drawn[0], m).astype(dtype)
        drawn[0] += m
        return r

    def at(u):
        y = Ad.T @ u
        return y - mu @ u if center else y

    def ax(v):
        y = Ad @ v
        return y - mu * v.sum() if center else y

    U = np.zeros((m, k), dtype)
    V = np.zeros((n, k), dtype)
    d = np.zeros(k, dtype)
    iters = []
    ksel = 0
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
            usq = uh @ uh
            if not usq > 0:
                v = np.zeros(n, dtype)
                break
            v = corr_v(at(uh), uh) / usq
            v = regularize(v, L1[1], L2[1], nonneg[1], ub[1], usq)
            sv = np.sqrt(v @ v)
            if not sv > 0:
                break
            v = v / sv
            vsq = v @ v
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
        ksel = f + 1
        if sigma < eps100:
            break
    return dict(u=U[:, :ksel], d=d[:ksel], v=V[:, :ksel], iters=np.array(iters), frob=frob,
                row_means=A.mean(axis=1) if center else None)
