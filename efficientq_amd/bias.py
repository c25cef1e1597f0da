"""Correction of the smooth multiplicative intensity inhomogeneity of an MRI scan (--prep_bias n4 of the ``prep`` and
``predict`` missions): N4 (Tustison et al. 2010) on Sled's N3 sharpening, as this package defines it.
The one definition of the rule; the sharpening runs on the host in fp64, everything per voxel on the device
(ops_bias; csrc/prep_bias.hip).  Agreement with ITK's filter is not claimed.

Per modality, on the scan's own grid, before every other step; the label is never touched.

Fit mask    M: the voxels of the modality's --prep_mask whose value is finite and > 0.  u = fp32(log(v)) there.
Samples     along an axis of length X the full-grid indices x = s q + s // 2 < X with s = SHRINK; an axis with fewer than
            MIN_AXIS_SAMPLES such indices uses s = 1 (sample_rule).  Coordinates are always those of the full grid.
Field       f = sum over the levels l = 0 .. LEVELS - 1 of a tensor-product uniform cubic B-spline with n = 2^l spans and
            n + 3 control points per axis: for index x, t = (x + 0.5) / X * n, span k = floor(t), the four basis values at
            t - k on control points k .. k + 3 (formed on the device: bias_weights of csrc/prep_bias.hip).  Each level
            keeps one accumulated lattice (fp64).  On the samples f is carried in fp32: f <- fp32(f + fp32(df)).
Iteration   at level l, over the samples in M:  r = u - f (fp32);  the histogram of r, BINS bins whose centres run from
            min r to max r, each sample split linearly between the two nearest centres, the fraction quantised to
            1 / 65536 and counted in integers (max r == min r ends the level);  E = sharpen(histogram);
            e = r - lerp(E, r), clamped to the end bins;  phi_c = sum w_c^3 e / S / sum w_c^2 with S the sum of the 64
            squared weights of a sample, 0 where no sample reaches c;  the level's lattice += phi;  df = eval(phi),
            f += df;  cv = population std / mean of exp(df) over the samples in M.  The level ends when cv < CV_STOP or
            after MAX_ITERS iterations.
Output      every voxel becomes fp32(v / exp(f)), f from the four lattices in fp64: an exact 0 stays 0, a negative value is
            divided like any other, a NaN or an Inf stays what it is.
Refusals    fewer than MIN_SAMPLES samples in M, or a field that is not finite, stops the run naming subject and modality.
"""
from __future__ import annotations

import math
from collections import namedtuple
from functools import partial

import numpy as np
import torch

from . import ops_bias
from . import prep

BINS, LEVELS, LATTICE_OFFSETS = ops_bias.BINS, ops_bias.LEVELS, ops_bias.LATTICE_OFFSETS
SHRINK = 4
MIN_AXIS_SAMPLES = 8
FWHM = 0.15                 # of the Gaussian the histogram is deconvolved with, log-units
WIENER = 0.01
PADDED = 512
CV_STOP = 0.001
MAX_ITERS = 50
MIN_SAMPLES = 1000
FRACTION = 65536
BIAS_KINDS = ("n4",)

# per level the iterations, the last cv, and min and max of exp(f) over M
Corrected = namedtuple("Corrected", "iters cv field_min field_max")


def bias_switch(args):
    """--prep_bias of `args` (or the YAML key): 'n4', None when absent; any other value is refused by name."""
    kind = getattr(args, "prep_bias", None)
    if kind is None:
        return None
    if not isinstance(kind, str) or kind.strip().lower() not in BIAS_KINDS:
        raise prep.PrepError(f"--prep_bias {kind!r}: n4")
    return kind.strip().lower()


def sample_rule(extent: int) -> tuple:
    """(stride, offset) of an axis: SHRINK and SHRINK // 2, or 1 and 0 when that leaves fewer than MIN_AXIS_SAMPLES."""
    s = SHRINK
    if (extent - s // 2 + s - 1) // s < MIN_AXIS_SAMPLES:
        s = 1
    return s, s // 2


def sharpen(hist, lo: float, hi: float) -> np.ndarray:
    """E, the expected true value of every bin centre (Sled's form): the histogram (BINS floats over [lo, hi]) padded to
    PADDED bins, deconvolved by the Wiener filter of a Gaussian of FWHM log-units, clipped at 0, and the ratio of the
    blurred first moment to the blurred density; 0 where that density is 0."""
    h = np.asarray(hist, dtype=np.float64)
    slope = (float(hi) - float(lo)) / (BINS - 1)
    start = (PADDED - BINS) // 2
    v = np.zeros(PADDED)
    v[start:start + BINS] = h
    width = FWHM / slope                                            # in bins
    i = np.arange(PADDED, dtype=np.float64)
    i = np.minimum(i, PADDED - i)
    kernel = 2.0 * math.sqrt(math.log(2.0) / math.pi) / width * np.exp(-i * i * (4.0 * math.log(2.0) / (width * width)))
    kf = np.fft.fft(kernel)
    wiener = np.conj(kf) / (np.abs(kf) ** 2 + WIENER)
    u = np.maximum(np.fft.ifft(np.fft.fft(v) * wiener).real, 0.0)
    centre = float(lo) + (np.arange(PADDED, dtype=np.float64) - start) * slope
    num = np.fft.ifft(np.fft.fft(u * centre) * kf).real
    den = np.fft.ifft(np.fft.fft(u) * kf).real
    e = np.zeros(PADDED)
    np.divide(num, den, out=e, where=den != 0.0)
    return e[start:start + BINS].copy()


def cv_of(s1: float, s2: float, n: int) -> float:
    """Population std / mean from the sum, the sum of squares and the count."""
    mean = s1 / n
    return math.sqrt(max(s2 / n - mean * mean, 0.0)) / mean


def correct(ops, subject: str, name: str, v, mask: str = "nonzero"):
    """(corrected float32 device volume, Corrected) of the D x H x W float32 device volume `v` by the rule above."""
    who = f"subject {subject}: modality {name}: --prep_bias"
    call = {k: getattr(ops, k, None) or partial(getattr(ops_bias, k), ops)
            for k in ("prep_bias_log", "prep_bias_hist", "prep_bias_fit", "prep_bias_apply")}
    dims = tuple(int(n) for n in v.shape)
    stride, offset = zip(*(sample_rule(n) for n in dims))
    u, m = call["prep_bias_log"](v, mask)
    f = torch.zeros(ops_bias.sample_shape(dims, stride, offset), dtype=torch.float32, device=v.device)
    lattices = torch.zeros(LATTICE_OFFSETS[-1], dtype=torch.float64, device=v.device)
    iters, cv = [], 0.0
    for level in range(LEVELS):
        lattice = lattices[LATTICE_OFFSETS[level]:LATTICE_OFFSETS[level + 1]]
        phi = torch.empty_like(lattice)
        done = 0
        while done < MAX_ITERS:
            counters, lo, hi, n = call["prep_bias_hist"](u, m, f, stride, offset)
            if n < MIN_SAMPLES:
                raise prep.PrepError(f"{who}: {n} samples inside the mask are finite and above 0, the fit needs "
                                     f"{MIN_SAMPLES}")
            if not hi > lo:
                break
            table = sharpen(counters / float(FRACTION), lo, hi)
            if not np.all(np.isfinite(table)):
                raise prep.PrepError(f"{who}: the sharpened histogram is not finite at level {level}")
            s1, s2 = call["prep_bias_fit"](u, m, f, stride, offset, level, lo, hi, table, phi, lattice)
            done += 1
            cv = cv_of(s1, s2, n)
            if not math.isfinite(cv):
                raise prep.PrepError(f"{who}: the field is not finite at level {level}, iteration {done}")
            if cv < CV_STOP:
                break
        iters.append(done)
    if not bool(torch.isfinite(lattices).all()):
        raise prep.PrepError(f"{who}: the field is not finite")
    y, lo, hi = call["prep_bias_apply"](v, m, lattices)
    if not (math.isfinite(lo) and math.isfinite(hi)):
        raise prep.PrepError(f"{who}: the field is not finite")
    return y, Corrected(tuple(iters), cv, lo, hi)
