"""Removal of thermal noise from an MRI scan by non-local means (--prep_denoise nlmM of the ``prep`` and ``predict``
missions): Buades' filter in the 3-D form of Coupe et al. 2008, as this package defines it.  The one
definition of the rule; everything per voxel runs on the device (ops_denoise; csrc/prep_denoise.hip), the noise level is
finished on the host in fp64.  Agreement with another tool's numbers is not claimed.

Per modality, on the scan's own grid, before --prep_bias and every other step; the label is never touched.

Omega       the voxels that are finite and, with --prep_mask nonzero, not exactly 0 (with ``all`` every finite voxel).  A
            voxel outside Omega leaves the filter bit for bit as it came: a zero keeps its sign, a NaN its payload.
Noise       one sigma per modality.  For every voxel of Omega whose six face neighbours are inside the volume and in
            Omega, e = fp32((double)v - ((((((d-) + (d+)) + (h-)) + (h+)) + (w-)) + (w+)) / 6), the sum in fp64 in that
            order, and r = |e|; every other voxel gets r = +0.  n and the median come from the exact radix select over the
            non-zero r (a constant background would otherwise pull the median to 0):  sigma = MAD_SCALE * median.
Filter      patch radius 1 (27 voxels), search radius M; patch reads outside the volume clamp to the edge.  For i in Omega
            and every j = i + t, t != 0, |t|inf <= M, j inside the volume and in Omega:
                d2 = (1 / 27) * sum over o in {-1, 0, 1}^3 of (v[clamp(i + o)] - v[clamp(j + o)])^2
                w  = exp(-max(d2 - 2 sigma^2, 0) / (H2 sigma^2)),     0 for a d2 that is not finite
                wmax = max w, or 1 when no candidate has w > 0
                y_i = (sum w_j v_j + wmax v_i) / (sum w_j + wmax)
Report      rms = sqrt(sum over Omega of (y - v)^2 / |Omega|), the noise that was removed; it should come out near sigma.
Refusals    fewer than MIN_SAMPLES residuals, or a sigma that is not finite and positive, stops the run naming subject
            and modality.
Not built   Rician bias correction, a spatially varying sigma, other patch radii, block-wise NLM.
"""
from __future__ import annotations

import math
import re
from collections import namedtuple
from functools import partial

from . import ops_denoise
from . import prep

H2 = 1.0                                        # the filter strength, in units of sigma^2 (csrc/prep_denoise.hip: NLM_H2)
MAD_SCALE = 1.4826 * math.sqrt(6.0 / 7.0)       # MAD to sigma, and the variance 7 / 6 sigma^2 of the pseudo-residual
MIN_SAMPLES = 1000
DEFAULT_RADIUS = 3
MAX_RADIUS = ops_denoise.MAX_RADIUS
DENOISE_FORMS = "nlm or nlmM, M = 1 ... %d" % MAX_RADIUS

# the search radius, the noise level, the residuals it was found from, and the rms of what the filter removed
Denoised = namedtuple("Denoised", "radius sigma samples rms")


def denoise_switch(args):
    """--prep_denoise of `args` (or the YAML key): the search radius, None when absent; any other value is refused."""
    kind = getattr(args, "prep_denoise", None)
    if kind is None:
        return None
    m = re.fullmatch(r"nlm([1-9]?)", kind.strip().lower()) if isinstance(kind, str) else None
    radius = (int(m.group(1)) if m.group(1) else DEFAULT_RADIUS) if m else 0
    if not 1 <= radius <= MAX_RADIUS:
        raise prep.PrepError(f"--prep_denoise {kind!r}: {DENOISE_FORMS}")
    return radius


def sigma_of(n: int, a, b) -> float:
    """The host half of the noise level: MAD_SCALE times the median of n residuals from their two middle order
    statistics (prep.percentile_value)."""
    return MAD_SCALE * prep.percentile_value(n, 50.0, a, b)


def noise_sigma(ops, sn: str, m: str, v, mask: str = "nonzero"):
    """(sigma, n) of the D x H x W float32 device volume `v` by the rule above."""
    residual = getattr(ops, "prep_denoise_residual", None) or partial(ops_denoise.prep_denoise_residual, ops)
    count, stats = ops.prep_quantiles(residual(v, mask).reshape(1, -1), [50.0], "nonzero")
    n = int(count.cpu()[0])
    a, b = (float(x) for x in stats.cpu()[0, 0]) if n else (math.nan, math.nan)
    sigma = sigma_of(n, a, b) if n else math.nan
    if n < MIN_SAMPLES or not (math.isfinite(sigma) and sigma > 0.0):
        raise prep.PrepError(f"subject {sn}: modality {m}: --prep_denoise: {n} residuals and a noise level of {sigma!r}, "
                             f"the filter needs {MIN_SAMPLES} and a finite level above 0")
    return sigma, n


def denoise(ops, sn: str, m: str, v, mask: str = "nonzero", radius: int = DEFAULT_RADIUS):
    """(denoised float32 device volume, Denoised) of the D x H x W float32 device volume `v` by the rule above."""
    sigma, n = noise_sigma(ops, sn, m, v, mask)
    nlm = getattr(ops, "prep_denoise_nlm", None) or partial(ops_denoise.prep_denoise_nlm, ops)
    y, sumsq, count = nlm(v, mask, radius, sigma)
    return y, Denoised(radius, sigma, n, math.sqrt(sumsq / count) if count else 0.0)
