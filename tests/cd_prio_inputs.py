"""Shared inputs of tests/test_gpu_cd_prio.py and tests/test_cd_prio_cpu.py: early-exit CD problems whose columns need anything from
a handful of sweeps to the cap.  numpy only: no torch, no GPU code, no oracle.

G = F F^T + 1e-3 I of a seeded non-negative F (k x 3k: one dominant direction, so coordinate descent on many coupled
coordinates is slow).  Column j starts at a non-negative x0_j with m_j nonzeros (m_j from 0 to k, mostly small) and has the
right-hand side b_j = G x0_j + s_j * noise_j, s_j log-uniform over four decades, the noise non-positive off the support of x0_j
(those coordinates stay at zero) and a tenth as large on it: how many sweeps a column needs follows the size of its support --
1 for an empty one, the cap of 100 for a large one.  The stop rule is relative (mean |step| / |x| < 1e-8), so a plain
b = G x0 + noise on a full support leaves every column at the cap whatever the noise level."""
import numpy as np

MAXIT, TOL = 100, 1e-8
KS = (64, 40, 24)                               # 32-column tiles: RT = 2, RT = 2 padded, RT = 1; 16-column: NT = 4, 3 (padded), 2
PLACED_SHAPES = ((32, 1573), (32, 2100), (16, 389))      # (tile width, columns) on 4 CUs = 16 SIMDs: see the GPU test's docstring
TILE_PER_WAVE_NS = (200, 70)
_CACHE = {}


def problem(n, k):
    """(G, B, X0) in float32, formed once per (n, k) and left unchanged."""
    if (n, k) not in _CACHE:
        rs = np.random.default_rng(7000 * k + n)
        F = rs.uniform(size=(k, 3 * k))
        G = F @ F.T + 1e-3 * np.eye(k)
        m = np.minimum(k, (k * rs.uniform(size=(n, 1)) ** 3).astype(int))          # support sizes 0 .. k, mostly small
        on = np.argsort(rs.uniform(size=(n, k)), axis=1) < m
        X0 = np.where(on, rs.uniform(0.5, 1.5, size=(n, k)), 0.0)
        scale = 10.0 ** rs.uniform(-4.0, 0.0, size=(n, 1)) * np.mean(np.diag(G))
        z = rs.standard_normal((n, k))
        B = X0 @ G + scale * np.where(on, 0.1 * z, -np.abs(z))
        _CACHE[(n, k)] = (G.astype(np.float32), B.astype(np.float32), X0.astype(np.float32))
    return _CACHE[(n, k)]
