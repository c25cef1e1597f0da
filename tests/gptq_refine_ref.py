"""Shared by tests/test_gptq_refine_{cpu,gpu}.py: a correlated Gram system that host and device hold alike, the cases of the
kernel test, and the margin below which two fp64 walks may decide differently."""
import functools

import numpy as np

ETA = 8.0
# (n, bias, c2, levels, per-row scales, passes).  n = 64: one block, no outside columns; 130 with bias: the bias alone in a
# padded last block; 193: a block with columns on both sides (mirrored and direct tiles).  c2 = 1: a partial group of four
# rows; 5: a padded 16-row tile; 70: a second 64-row group in the update's grid.  The last case ends at a fixed point.
CASES = [(64, False, 1, 4, False, 1), (64, False, 5, 2, True, 3), (130, True, 5, 256, False, 1), (130, True, 70, 4, True, 3),
         (130, True, 1, 2, False, 3), (193, True, 70, 2, False, 1), (193, True, 1, 256, True, 3), (193, True, 5, 4, False, 3),
         (193, True, 70, 256, True, 1), (65, True, 5, 16, False, 16)]
EXCUSED = 0.1          # the share of rows that may meet a decision inside the margin


@functools.lru_cache(maxsize=None)
def system(n, bias, c2, per_row):
    """(A0 fp32, H fp64, u, alpha): A0 = 2 X^T X rounded to fp32, X the rectified mixtures of 2 n normal samples (dense
    off-diagonal entries, not diagonally dominant; a ones column for the bias), and H = A0 + eta I from that fp32 matrix;
    u dyadic, exact in fp32."""
    rng = np.random.default_rng(100 * n + c2)
    X = np.maximum(rng.standard_normal((2 * n, n)) @ (np.eye(n) + rng.standard_normal((n, n)) * (2.0 / np.sqrt(n))), 0.0)
    if bias:
        X[:, -1] = 1.0
    A0 = (2.0 * X.T @ X).astype(np.float32)
    A0 = np.triu(A0) + np.triu(A0, 1).T            # exactly symmetric: the kernels read the upper triangle
    u = rng.integers(-511, 512, (c2, n)) / 1024.0
    alpha = 0.3 + 0.04 * (np.arange(c2) % 6) if per_row else np.array([0.4])
    return A0, A0.astype(np.float64) + ETA * np.eye(n), u, alpha


def quad(H, q, u):
    return np.einsum("ri,ij,rj->r", q - u, H, q - u)


def threshold(H, q, u, alpha, passes):
    """Per row, in units of alpha^2: g_j is a sum of n products that every pass adds to again, so its fp64 error is within
    (passes + 1) n 2^-52 sum_k |q_k - u_k| |H_kj|; t_j moves by that over H_jj, and a difference of squared distances to two
    grid values, which lie at most 2 alpha apart, by 4 alpha times as much.  Twice that."""
    dt = ((passes + 1) * H.shape[0] * 2.0 ** -52 * (np.abs(q - u) @ np.abs(H)) / H.diagonal()).max(axis=1)
    return 8.0 * dt / np.broadcast_to(np.asarray(alpha, dtype=np.float64).reshape(-1), dt.shape)
