"""The rule of crf.py in numpy fp64: plain loops over the offsets with slicing, nothing borrowed from the kernel."""
import itertools
import math

import numpy as np


def radii(spacing, theta_p, theta_s):
    return tuple(min(3, int(math.floor(2.0 * max(theta_p, theta_s) / s))) for s in spacing)


def offsets(r):
    return [t for t in itertools.product(*[range(-n, n + 1) for n in r]) if any(t)]


def _shifted(a, t):
    """(the part of the last three axes of `a` that has a neighbour at offset t, that neighbour's part)."""
    here = tuple(slice(max(0, -d), max(0, a.shape[-3 + k] - max(0, d))) for k, d in enumerate(t))
    there = tuple(slice(max(0, d), max(0, a.shape[-3 + k] - max(0, -d))) for k, d in enumerate(t))
    return (Ellipsis,) + here, (Ellipsis,) + there


def decide(h, mode, thresh=0.0):
    """The decision of every voxel: the first largest channel, or the channels at or above the threshold as bits."""
    if mode == "softmax":
        return np.argmax(h, axis=0)
    return ((h >= np.float32(thresh)).astype(np.int64) << np.arange(h.shape[0]).reshape(-1, 1, 1, 1)).sum(0)


def margin(h, mode, thresh=0.0):
    """How far every voxel is from deciding otherwise: top two, or the nearest channel's distance to the threshold."""
    if mode == "softmax":
        top = np.sort(h, axis=0)
        return top[-1] - top[-2]
    return np.abs(h - float(np.float32(thresh))).min(0)


def crf(v, x, spacing, mode, w_a, w_s, theta_p, theta_i, theta_s, iters, thresh=0.0):
    """(H after `iters` iterations in fp64, changed, the voxels that are all finite) of logits v (C, D, H, W) and images x
    (M, D, H, W)."""
    v64, x64 = v.astype(np.float64), x.astype(np.float64)
    ok = np.isfinite(v64).all(0) & np.isfinite(x64).all(0)
    vz, xz = np.where(ok, v64, 0.0), np.where(ok, x64, 0.0)
    ts = offsets(radii(spacing, theta_p, theta_s))
    d2 = [sum((s * d) ** 2 for s, d in zip(spacing, t)) for t in ts]
    gp = np.array([math.exp(-d / (2 * theta_p ** 2)) for d in d2])
    gs = np.array([math.exp(-d / (2 * theta_s ** 2)) for d in d2])
    gp, gs = gp / gp.sum(), gs / gs.sum()
    h = vz.copy()
    for _ in range(iters):
        if mode == "softmax":
            e = np.exp(h - h.max(0))
            msg = e / e.sum(0)
        else:
            msg = 2.0 / (1.0 + np.exp(-h)) - 1.0
        msg = msg * ok                                                    # a voxel that is not finite sends nothing
        new = vz.copy()
        for t, a, b in zip(ts, gp, gs):
            here, there = _shifted(h, t)
            k = w_a * a * np.exp(-((xz[here] - xz[there]) ** 2).sum(0) / (2 * theta_i ** 2)) + w_s * b
            new[here] += k * msg[there]
        h = new
    h = np.where(ok, h, v64)                                              # ... and keeps H = v
    changed = int((ok & (decide(h, mode, thresh) != decide(v64, mode, thresh))).sum())
    return h, changed, ok
