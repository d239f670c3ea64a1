"""numpy restatement of the reference's randomized SVD (randomized_svd, inst/include/FactorNet/svd/randomized.hpp:59-241,
Halko-Martinsson-Tropp): the parity target of tests/test_gpu_svd_rand.py, checked on its own in tests/test_svd_rand_cpu.py.

The sketch is the reference's SplitMix64 stream (rng/rng.hpp:89-104, :213-219: column-major, one draw per element), the QR steps
are numpy's Householder QR and the small SVD is LAPACK's.  A thin QR is unique up to column signs, and those signs cancel in
U diag(d) V', so the factors are defined up to one sign per column pair; compare after align()."""
import numpy as np

GOLDEN = 0x9E3779B97F4A7C15
MASK = (1 << 64) - 1


def sizes(m, n, k, maxit=0):
    """randomized.hpp:73-76: oversampling p, sketch dimension l, power iterations q."""
    p = min(max(10, k // 5), min(m, n) - k)
    return p, k + max(p, 0), 3 if maxit <= 0 else min(int(maxit), 10)


def splitmix_uniform(seed, start, count, dtype=np.float64):
    """uniform<dtype>() of draws start .. start + count - 1 of the stream of `seed`: static_cast<T>(next()) / static_cast<T>(UINT64_MAX)."""
    idx = np.arange(start + 1, start + count + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed & MASK) + idx * np.uint64(GOLDEN)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return z.astype(dtype) / dtype(2.0 ** 64)          # UINT64_MAX rounds to 2^64 in both formats


def omega(n, l, seed=0, dtype=np.float64):
    """randomized.hpp:145-151: n x l, filled column by column, shifted to [-0.5, 0.5).  Seed 0 means 42."""
    s = 42 if seed == 0 else int(seed)
    return (splitmix_uniform(s, 0, n * l, dtype) - dtype(0.5)).reshape(l, n).T.copy()


def randomized_svd(A, k, maxit=0, center=False, seed=0, dtype=np.float64):
    """A: dense m x n.  Returns dict(u, d, v, iters, row_means, frob, p, l, q) in `dtype` arithmetic."""
    A = np.asarray(A, np.float64)
    m, n = A.shape
    p, l, q = sizes(m, n, k, maxit)
    mu = A.mean(axis=1)
    frob = float(np.sum(A * A) - (n * np.sum(mu * mu) if center else 0.0))
    At = (A - mu[:, None] if center else A).astype(dtype)
    Y = At @ omega(n, l, seed, dtype)
    for _ in range(q):
        Y = np.linalg.qr(Y)[0]
        Z = np.linalg.qr(At.T @ Y)[0]
        Y = At @ Z
    Q = np.linalg.qr(Y)[0]
    Bt = At.T @ Q
    Ub, sv, Vbt = np.linalg.svd(Bt, full_matrices=False)
    kk = min(k, sv.size)
    return dict(u=Q @ Vbt.T[:, :kk], d=sv[:kk], v=Ub[:, :kk], iters=np.array([q], np.int32), row_means=mu, frob=frob, p=p, l=l, q=q)


def align(u_ref, u, v):
    """u and v with each column's sign flipped where u_ref . u is negative."""
    sg = np.sign(np.sum(u_ref * u, axis=0))
    sg[sg == 0] = 1.0
    return u * sg, v * sg
