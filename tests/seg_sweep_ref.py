"""numpy restatement of effq_seg_sweep, written from its definition (include/effq_hip.h), not from
the kernel: scores in np.float32, edges built here, bins by np.searchsorted on the edges, the argmax pin from a
restatement of torch.max's rule, the histogram by np.add.at."""
import numpy as np

BINS = 4096
MID = 2048


def edges(mode: str, thresh=0.0) -> np.ndarray:
    """The 4096 fp32 edges: -inf, then (k - 2048) / 128 for k = 1 .. 4095, with edge 2048 = `thresh` in sigmoid mode and
    0 in argmax mode."""
    e = ((np.arange(BINS, dtype=np.float64) - MID) / 128.0).astype(np.float32)
    assert np.array_equal(e.astype(np.float64) * 128.0, np.arange(BINS) - MID)       # every edge is exact in fp32
    e[0] = -np.inf
    e[MID] = np.float32(thresh) if mode == "sigmoid" else np.float32(0.0)
    assert e[MID - 1] < e[MID] < e[MID + 1]
    return e


def bins_of(s: np.ndarray, e: np.ndarray) -> np.ndarray:
    """The number of k >= 1 with e_k <= s; NaN -> 0."""
    s = np.asarray(s, dtype=np.float32)
    b = np.searchsorted(e[1:], s, side="right")
    return np.where(np.isnan(s), 0, b).astype(np.int64)


def torch_max_winner(x: np.ndarray) -> np.ndarray:
    """torch.max over axis 0 of C x S: the first maximum wins, NaN counts as the largest value."""
    C, S = x.shape
    best = np.zeros(S, dtype=np.int64)
    bv = x[0].copy()
    for c in range(1, C):
        v = x[c]
        take = (v > bv) | (np.isnan(v) & ~np.isnan(bv))
        bv = np.where(take, v, bv)
        best = np.where(take, c, best)
    return best


def scores(x: np.ndarray, mode: str, fuse=None) -> np.ndarray:
    """C x S fp32 scores of C x S fp32 logits."""
    x = np.asarray(x, dtype=np.float32)
    C = x.shape[0]
    with np.errstate(invalid="ignore"):
        if mode == "argmax":
            assert fuse is None
            if C == 1:
                return x.copy()
            out = np.empty_like(x)
            for c in range(C):
                others = np.delete(x, c, axis=0)
                m = np.max(others, axis=0)                       # np.max hands a NaN on: NaN is the largest
                out[c] = x[c] - m                                # one fp32 subtraction
            return out
        if fuse in ("agg", "aggressive"):
            # np.fmax keeps the value that is not NaN: NaN only when all of x_c .. x_{C-1} are
            return np.stack([np.fmax.reduce(x[c:], axis=0) for c in range(C)])
        if fuse in ("con", "conservative"):
            # np.min hands a NaN on: NaN when any of x_0 .. x_c is
            return np.stack([np.min(x[:c + 1], axis=0) for c in range(C)])
        assert fuse is None
        return x.copy()


def truth(label: np.ndarray, mode: str, C: int) -> np.ndarray:
    """C x S bool: class ids (S) in argmax mode (a value >= C belongs to no class), C x S 0/1 planes in sigmoid mode."""
    label = np.asarray(label)
    if mode == "argmax":
        return np.stack([label == c for c in range(C)])
    return label != 0


def bins(x, mode: str, fuse=None, thresh=0.0) -> np.ndarray:
    """C x S bins of logits C x S, in argmax mode pinned to torch.max's decision."""
    x = np.asarray(x, dtype=np.float32)
    C = x.shape[0]
    b = bins_of(scores(x, mode, fuse), edges(mode, thresh))
    if mode == "argmax":
        win = torch_max_winner(x)
        is_win = np.stack([win == c for c in range(C)])
        b = np.where(is_win, np.maximum(b, MID), np.minimum(b, MID - 1))
    return b


def sweep(x, label, mode: str, fuse=None, thresh=0.0) -> np.ndarray:
    """hist (C, 2, 4096) int64 of logits C x S and their label."""
    x = np.asarray(x, dtype=np.float32)
    x = x.reshape(x.shape[0], -1)
    C, S = x.shape
    b = bins(x, mode, fuse, thresh)
    g = truth(np.asarray(label).reshape(-1, S) if mode == "sigmoid" else np.asarray(label).reshape(S), mode, C)
    hist = np.zeros((C, 2, BINS), dtype=np.int64)
    for c in range(C):
        np.add.at(hist[c], (g[c].astype(np.int64), b[c]), 1)
    return hist


def decision_counts(hist: np.ndarray, k: int) -> np.ndarray:
    """C x 4 = TP, FP, FN, TN of the decision "score >= edge k"."""
    h = np.asarray(hist, dtype=np.int64)
    return np.stack([h[:, 1, k:].sum(1), h[:, 0, k:].sum(1), h[:, 1, :k].sum(1), h[:, 0, :k].sum(1)], axis=1)
