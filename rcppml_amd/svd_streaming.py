"""svd_streaming() / pca_streaming(): the reference's out-of-core SVD -- svd("file.spz") through svd/streaming.hpp:683-773 and
svd_streaming_gateway -- for the randomized block method, on the HIP streaming path (csrc/ops_stream_svd.hip).  In the reference
the streamed fit is svd() on a path; here it is a function of its own and svd() is unchanged.

The algorithm is svd(method = "randomized")'s, step for step: the same sketch, power iterations, CholeskyQR2 and small stage, with
the two block products taken one column panel at a time, so the result agrees with it up to the order of the floating-point sums
of the product in the scatter direction.  What differs is memory: neither the matrix nor its transpose lies on the device, only
the two l-wide blocks and one panel buffer do.  A fit costs 2 maxit + 2 passes over the matrix, one more when centred.
"""
import os

import numpy as np

from . import _abi
from .nmf import _as_csc

# what the streamed fit does not carry, by argument of svd(): refused before anything runs
_REFUSED = dict(tol=1e-5, L1=0, L2=0, nonneg=False, upper_bound=0, method="randomized", test_fraction=0, mask=None, cv_seed=None,
                patience=3, k_max=50, L21=0, angular=0, graph_U=None, graph_V=None, graph_lambda=0, devices=1)


def svd_streaming(data, k=10, center=False, seed=None, maxit=3, precision="float", panel_cols=0, **unsupported):
    """Randomized block SVD with the matrix streamed through the device one panel of `panel_cols` columns at a time.

    `data`: a scipy sparse matrix, a CSC, a 2-D array (taken as sparse), or the path of an .spz file (StreamPress v2, not
    row-sorted; st_write() produces one), whose chunks are decoded on the device panel by panel.  `panel_cols` = 0 chooses panels of about 64 MiB of CSC in
    whole multiples of 256 columns; for an .spz file it is rounded up to whole chunks.  k, center, seed, maxit (the power
    iterations, at most 10) and precision ("float" / "double") are svd(method = "randomized")'s; l = k + max(10, k / 5) must be at
    most 128 and at most min(m, n).  Any other svd() argument (tol, L1, L2, nonneg, upper_bound, another method, k = "auto",
    test_fraction, mask, cv_seed, patience, k_max, L21, angular, graph_U, graph_V, graph_lambda, devices) set to anything but its
    default raises NotImplementedError naming it.

    Returns dict(u, d, v, misc) as svd() does; misc holds method = "randomized", row_means (or None), iters_per_factor = [the
    power iterations run], passes, panels, panel_cols, panel_bytes_peak, range_table_bytes, device_ops and entry."""
    for name, value in unsupported.items():
        if name not in _REFUSED:
            raise TypeError("svd_streaming() got an unexpected keyword argument '%s'" % name)
        default = _REFUSED[name]
        same = value is default if default is None else (value is not None and np.ndim(value) == 0 and value == default)
        if not same:
            raise NotImplementedError("svd_streaming(): '%s' is not carried by the streamed fit; use svd()" % name)
    if isinstance(k, str):
        raise NotImplementedError("svd_streaming(): 'k' = %r (auto-rank) is not carried by the streamed fit; use svd()" % k)
    if precision not in ("float", "double"):
        raise ValueError("precision must be 'float' or 'double'")
    k = int(k)
    if k < 1:
        raise ValueError("'k' must be >= 1")
    if int(panel_cols) < 0:
        raise ValueError("'panel_cols' must be >= 0")
    path = os.fspath(data) if isinstance(data, (str, bytes)) or hasattr(data, "__fspath__") else None
    if path is not None:
        st, m, n, _, _ = _abi.spz_info(np.fromfile(path, np.uint8, 128))
        if st != 0:
            raise ValueError("data: %s is not a v2 .spz file" % (path,))
        csc = None
    else:
        A = _as_csc(data)
        m, n = A.shape
        csc = (A.p, A.i, A.x)
    r = _abi.svd_streaming(csc, path, m, n, k, center=center, seed=0 if seed is None else int(seed), max_iter=int(maxit),
                           precision=_abi.F32 if precision == "float" else _abi.F64, panel_cols=int(panel_cols))
    if r["status"] != 0:
        raise _abi.BackendError("GPU streamed SVD/PCA failed: %s" % r["error"])
    misc = dict(method="randomized", row_means=r["row_means"].copy() if center else None,
                iters_per_factor=np.array([r["power_iterations"]], np.int32), k_selected=k, precision=precision,
                entry="rcppml_gpu_svd_streaming_ex",
                **{key: r[key] for key in ("passes", "panels", "panel_cols", "panel_bytes_peak", "range_table_bytes", "device_ops", "sketch")})
    return dict(u=r["U"].copy(), d=r["d"][:k].copy(), v=r["V"].copy(), misc=misc)


def pca_streaming(data, k=10, **kw):
    """svd_streaming(data, k, center = True, ...)."""
    kw["center"] = True
    return svd_streaming(data, k=k, **kw)
