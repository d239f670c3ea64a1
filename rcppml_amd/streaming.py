"""nmf_streaming(): the reference's out-of-core fit -- nmf(data, streaming = TRUE, panel_cols = ...) of R/nmf_thin.R:442-610, built
there from nmf/fit_chunked.hpp and nmf/fit_streaming_spz.hpp -- on the HIP streaming path (csrc/ops_stream.hip).  In the reference
`streaming` is an argument of nmf(); here it is a function of its own and nmf() is unchanged.

The model is nmf()'s: the same update order, penalties, scaling, loss and convergence rule, with the columns regrouped into panels,
so the factors agree with nmf() up to the order of the floating-point sums.  What differs is memory: the matrix and its transpose
never lie on the device, only W, H, the right-hand sides and one panel buffer do.
"""
import os

import numpy as np

from . import _abi
from .data import r_runif, splitmix64_uniform
from .nmf import NMFModel, _as_csc, _pair, select_solver

# what the streamed fit does not carry, by argument: refused before anything runs
_REFUSED = dict(mask=None, loss="mse", robust=False, test_fraction=0, projective=False, symmetric=False, zi="none", L21=(0.0, 0.0),
                angular=(0.0, 0.0), graph_W=None, graph_H=None, target_H=None, devices=1)


def nmf_streaming(data, k, panel_cols=0, tol=1e-4, maxit=100, L1=(0.0, 0.0), L2=(0.0, 0.0), seed=None, nonneg=(True, True), *,
                  solver="auto", upper_bound=(0.0, 0.0), cd_maxit=100, cd_tol=1e-8, norm="L1", sort_model=True, patience=5,
                  h_init=None, precision="fp32", **unsupported):
    """A ~ w diag(d) h by alternating NNLS with the matrix streamed through the device one panel of `panel_cols` columns at a time.

    `data`: a scipy sparse matrix, a CSC, a 2-D array (taken as sparse), or the path of an .spz file (StreamPress v2, not
    row-sorted; st_write() produces one), whose chunks are decoded on the device panel by panel: the matrix then never exists
    uncompressed, on either side.
    `panel_cols` = 0 chooses panels of about 64 MiB of CSC at the matrix's mean column size, in whole multiples of 256 columns,
    never more than n and never more than the W-side kernel's range table allows (2 GiB); a value above n means one panel.  For an
    .spz file `panel_cols` is rounded up to whole chunks.  The other arguments are nmf()'s; `seed` is None,
    an int or a W matrix.  MSE loss, CD or Cholesky + clip, 1 <= k <= 64.  Any other nmf() argument (mask, loss, robust,
    test_fraction, projective, symmetric, zi, L21, angular, graph_W, graph_H, target_H, devices, a string seed) set to anything but
    its default raises NotImplementedError naming it.
    misc gains panels, panel_cols, panel_bytes_peak (bytes of the panel buffer), range_table_bytes (the W-side kernel's scratch
    table), device_ops_per_iter and entry."""
    for name, value in unsupported.items():
        if name not in _REFUSED:
            raise TypeError("nmf_streaming() got an unexpected keyword argument '%s'" % name)
        default = _REFUSED[name]
        same = value is default if default is None else (value is not None and np.ndim(value) == np.ndim(default) and np.all(np.asarray(value) == np.asarray(default)))
        if not same:
            raise NotImplementedError("nmf_streaming(): '%s' is not carried by the streamed fit; use nmf()" % name)
    if isinstance(seed, str):
        raise NotImplementedError("nmf_streaming(): 'seed' = %r (an SVD start) is not carried by the streamed fit; use nmf()" % seed)
    if precision not in ("fp32", "fp64"):
        raise ValueError("precision must be 'fp32' or 'fp64'")
    if norm not in ("L1", "L2", "none", "None"):
        raise ValueError("'arg' should be one of 'L1', 'L2', 'none'")
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
    k = int(k)
    if k < 1:
        raise ValueError("k must be a positive integer")
    if int(panel_cols) < 0:
        raise ValueError("'panel_cols' must be >= 0")
    L1p, L2p, ubp = _pair(L1, "L1"), _pair(L2, "L2"), _pair(upper_bound, "upper_bound")
    if max(L1p) >= 1 or min(L1p) < 0:
        raise ValueError("L1 penalties must be strictly in the range [0,1)")
    if min(L2p) < 0:
        raise ValueError("L2 penalties must be strictly >= 0")
    if min(ubp) < 0:
        raise ValueError("'upper_bound' values must be non-negative")
    nn = np.atleast_1d(np.asarray(nonneg))
    if nn.dtype != np.bool_ or nn.shape[0] not in (1, 2):
        raise ValueError("'nonneg' must be logical, of length 1 or 2")
    solver = select_solver(solver, k, L1p, "mse", use_gpu=True)
    # ---- the start, as nmf() draws it
    if seed is not None and np.ndim(seed) == 2:
        s = np.asarray(seed, dtype=np.float64)
        if s.shape not in ((m, k), (k, m)):
            raise ValueError("Custom init matrix dimensions incompatible with data")
        W_T = np.array(s if s.shape == (m, k) else s.T, order="C")          # a copy: the entry updates it in place
        seed_int = int(abs(int(np.sum(s * 1e6) % (2 ** 31 - 1))))
    else:
        seed_int = int(seed) if seed is not None else int(np.random.SeedSequence().generate_state(1)[0] % (2 ** 31 - 1)) + 1
        W_T = np.ascontiguousarray(r_runif(seed_int, m * k).reshape(k, m).T)
    if h_init is not None:
        H = np.array(np.asarray(h_init, dtype=np.float64).T, order="C")
        if H.shape != (n, k):
            raise ValueError("h_init must be k x n")
    else:
        sdt = np.float32 if precision == "fp32" else np.float64
        H = splitmix64_uniform(seed_int & 0xFFFFFFFF, 0, k * n, sdt).astype(np.float64).reshape(n, k)
    res = _abi._check(_abi.nmf_streaming(csc, path, m, n, k, W_T, H, panel_cols=int(panel_cols), max_iter=int(maxit),
                                         tol=float(tol), L1=L1p, L2=L2p, upper_bound=ubp, nonneg=(int(nn[0]), int(nn[-1])),
                                         norm_type={"L1": 0, "L2": 1, "none": 2, "None": 2}[norm], solver_mode=0 if solver == "cd" else 1,
                                         cd_maxit=int(cd_maxit), cd_tol=float(cd_tol), patience=int(patience), sort_model=int(bool(sort_model)),
                                         precision=_abi.F32 if precision == "fp32" else _abi.F64), "streamed NMF")
    misc = dict(tol=res["tol"], iter=res["iter"], loss=res["loss"], loss_history=res["loss_history"], converged=res["converged"],
                solver=solver, solver_mode=0 if solver == "cd" else 1, L1=L1p, L2=L2p, seed=seed_int, precision=precision, resource="gpu",
                loss_type="mse", panels=res["panels"], panel_cols=res["panel_cols"], panel_bytes_peak=res["panel_bytes_peak"],
                range_table_bytes=res["range_table_bytes"], device_ops_per_iter=res["ops_per_iter"],
                entry="rcppml_gpu_nmf_streaming_ex")
    return NMFModel(w=W_T.copy(), d=res["d"], h=H.T.copy(), misc=misc)
