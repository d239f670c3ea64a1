"""numpy restatement of the reference's initialize_lanczos / initialize_irlba (nmf/nmf_init.hpp:45-158) given the truncated SVD they
run: W_T(c, :) = |U(:, c)| sqrt(d_c) and H(c, :) = |V(:, c)| sqrt(d_c) for the k_svd triplets delivered, in the fit's Scalar, and the
rows the SVD did not deliver filled from one sequential SplitMix64 stream (:82-90)."""
import numpy as np

from rcppml_amd.data import splitmix64_uniform


def fill_seed(seed):
    """rng::SplitMix64 rng(seed == 0 ? 54321U : seed + 999), uint32 arithmetic."""
    seed = int(seed) & 0xFFFFFFFF
    return 54321 if seed == 0 else (seed + 999) & 0xFFFFFFFF


def initialize_lanczos(U, d, V, k, m, n, seed, dtype=np.float64):
    """U (m x k_svd), d (k_svd), V (n x k_svd): the SVD result, k_svd <= k.  Returns W_T as (m, k) and H as (n, k) arrays of
    `dtype`, C-order: the column-major k x m and k x n matrices of the reference."""
    dtype = np.dtype(dtype)
    U, d, V = (np.asarray(a).astype(dtype) for a in (U, d, V))
    ks = min(k, d.shape[0])
    W_T, H = np.zeros((m, k), dtype), np.zeros((n, k), dtype)
    sq = np.sqrt(d[:ks])
    W_T[:, :ks] = np.abs(U[:, :ks]) * sq
    H[:, :ks] = np.abs(V[:, :ks]) * sq
    if ks < k:
        rows = k - ks
        # fill_uniform(data, rows, cols) walks the rows x cols block column by column (rng.hpp:195-201): W first, then H goes on
        # in the same stream
        draws = splitmix64_uniform(fill_seed(seed), 0, rows * (m + n), dtype)
        W_T[:, ks:] = draws[:rows * m].reshape(m, rows)
        H[:, ks:] = draws[rows * m:].reshape(n, rows)
    return W_T, H
