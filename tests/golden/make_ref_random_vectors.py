#!/usr/bin/env python3
"""tests/golden/make_ref_random_vectors.py -- the reference's outputs for the randomised draws of tests/test_oracle_ref.py.

The two live tests there (SplitMix64 factor initialisation at 20 random seeds and shapes; NB IRLS weight and NB negative
log-likelihood at 500 random points) call oracle/_ref/libref_rng.so and libref_loss.so (built by `make -C oracle ref` from the
reference tree, sources never copied).  This script runs the same draws through those libraries once and stores inputs +
outputs in tests/golden/ref_random_vectors.npz, so that the tests compare against the reference where the tree does not exist.
Data only: seeds, shapes, arguments and the reference's numeric outputs."""
import ctypes as C
import os

import numpy as np

here = os.path.dirname(os.path.abspath(__file__))
root = os.path.dirname(os.path.dirname(here))
rng = C.CDLL(os.path.join(root, "oracle", "_ref", "libref_rng.so"))
loss = C.CDLL(os.path.join(root, "oracle", "_ref", "libref_loss.so"))
for f, t in ((loss.ref_irls_weight_nb_f64, C.c_double), (loss.ref_loss_nb_f64, C.c_double),
             (loss.ref_irls_weight_nb_f32, C.c_float), (loss.ref_loss_nb_f32, C.c_float)):
    f.restype = t

out = {}
# factor initialisation: W (m x k) then H (n x k) of every draw, flattened one after the other per precision
rs = np.random.default_rng(7)
seeds, shapes, flat = [], [], {"f64": [], "f32": []}
for _ in range(20):
    seed = int(rs.integers(0, 2 ** 63)) * 2 + int(rs.integers(0, 2))
    k, m, n = (int(v) for v in rs.integers(1, 40, size=3))
    seeds.append(seed)
    shapes.append((k, m, n))
    for name, dt, fn in (("f64", np.float64, rng.ref_init_factors_f64), ("f32", np.float32, rng.ref_init_factors_f32)):
        W = np.zeros((m, k), dt)
        H = np.zeros((n, k), dt)
        fn(C.c_uint64(seed), k, m, n, W.ctypes.data_as(C.c_void_p), H.ctypes.data_as(C.c_void_p))
        flat[name] += [W.ravel(), H.ravel()]
out["init_seeds"] = np.array(seeds, dtype=np.uint64)
out["init_shapes"] = np.array(shapes, dtype=np.int64)
for name in ("f64", "f32"):
    out["init_" + name] = np.concatenate(flat[name])
# NB IRLS weight (pred, size) and NB negative log-likelihood (obs, pred, size)
rs = np.random.default_rng(11)
pts = np.array([(float(10 ** rs.uniform(-14, 6)), float(10 ** rs.uniform(-12, 6)), float(rs.integers(0, 2000))) for _ in range(500)])
out["nb_pred"], out["nb_size"], out["nb_obs"] = pts[:, 0], pts[:, 1], pts[:, 2]
out["nb_weight_f64"] = np.array([loss.ref_irls_weight_nb_f64(C.c_double(p), C.c_double(r)) for p, r, y in pts])
out["nb_weight_f32"] = np.array([loss.ref_irls_weight_nb_f32(C.c_float(p), C.c_float(r)) for p, r, y in pts], dtype=np.float32)
out["nb_nll_f64"] = np.array([loss.ref_loss_nb_f64(C.c_double(y), C.c_double(p), C.c_double(r)) for p, r, y in pts])
out["nb_nll_f32"] = np.array([loss.ref_loss_nb_f32(C.c_float(y), C.c_float(p), C.c_float(r)) for p, r, y in pts], dtype=np.float32)
np.savez_compressed(os.path.join(here, "ref_random_vectors.npz"), **out)
print("wrote", {k: v.shape for k, v in out.items()})
