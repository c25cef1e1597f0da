"""The rule of efficientq_amd/gptq.py in plain numpy fp64, column by column (no blocks, no reversal)."""
import numpy as np


def gptq_ref(H, u, alpha, levels, has_bias):
    """(P, q, ids, err, margin) for H (n, n), u (c2, n) and alpha (a scalar or c2 scales); margin: per row the smallest
    distance of an unclipped t_j to a rounding boundary of its grid."""
    c2, n = u.shape
    P = np.linalg.cholesky(H[::-1, ::-1])[::-1, ::-1]
    a = np.broadcast_to(np.asarray(alpha, dtype=np.float64).reshape(-1), (c2,))
    d = 2.0 / (levels - 1)
    q, ids, err, margin = np.zeros((c2, n)), np.zeros((c2, n)), np.zeros(c2), np.full(c2, np.inf)
    for r in range(c2):
        s = np.zeros(n)
        for j in range(n):
            t = u[r, j] - s[j] / P[j, j]
            if has_bias and j == n - 1:
                q[r, j] = t
            else:
                x = (t / a[r] + 1.0) / d
                if 0.0 < x < levels - 1:
                    margin[r] = min(margin[r], abs(abs(x - np.floor(x)) - 0.5) * d * a[r])
                ids[r, j] = np.rint((min(max(t / a[r], -1.0), 1.0) + 1.0) / d)
                q[r, j] = a[r] * (ids[r, j] * d - 1.0)
            s[j + 1:] += (q[r, j] - u[r, j]) * P[j, j + 1:]
            err[r] += (P[j, j] * (q[r, j] - t)) ** 2
    return P, q, ids, err, margin
