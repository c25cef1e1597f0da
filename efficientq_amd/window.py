"""The sliding window of the validation and of the ``predict`` mission: the window grid, the host split and stitch of the
reference (``utils/transforms.py:784-852``, ``utils/validate.py:236-245``) and the HIP path, stitched_window_logits
(batched gather, un-mirrored put, stitch: DESIGN.md section 13, with --blend and --tta_mirror).  evaluate.py imports
every name: ``evaluate.X`` is the object defined here."""
from __future__ import annotations

from typing import List, Sequence

import torch

from .ops_base import _triple
from .ops_window import BLEND_KINDS      # --blend: the window weights of the stitch (ops_window.blend_weights_host)

WINDOW_BATCH_MAX = 16     # windows per forward at most (a BraTS case has 8 of 128^3)


def window_starts(size: int, patch: int, overlap: int) -> List[int]:
    """Start offsets along one axis (transforms.py:797-800): a step of patch-overlap while a whole patch still
    ends strictly before the border, then one patch flush with the border."""
    if patch > size:
        raise RuntimeError(f"patch {patch} larger than the image extent {size}")
    if overlap >= patch:
        raise RuntimeError("overlap must be smaller than the patch")
    return list(range(0, size - patch, patch - overlap)) + [size - patch]


def image_to_patch3d(images: torch.Tensor, patch_sz, overlap) -> List[torch.Tensor]:
    """Overlapped patches of an N x C x D x H x W batch in (d, h, w) raster order (transforms.py:784-810)."""
    if patch_sz is None or overlap is None:
        return images
    p, o = _triple(patch_sz), _triple(overlap)
    d, h, w = images.shape[-3:]
    return [images[..., i:i + p[0], j:j + p[1], k:k + p[2]]
            for i in window_starts(d, p[0], o[0]) for j in window_starts(h, p[1], o[1])
            for k in window_starts(w, p[2], o[2])]


def patch_to_image3d(images: torch.Tensor, patch_list: Sequence[torch.Tensor], patch_sz, overlap) -> torch.Tensor:
    """Stitch per-patch outputs (any leading dims, e.g. heads x batch x channels) back to the image grid: sum of
    the patches over the number of patches covering each voxel (transforms.py:812-852)."""
    if patch_sz is None or overlap is None:
        return images
    p, o = _triple(patch_sz), _triple(overlap)
    d, h, w = images.shape[-3:]
    first = patch_list[0]
    acc = torch.zeros(tuple(first.shape[:-3]) + (d, h, w), dtype=first.dtype, device=first.device)
    cnt = torch.zeros((d, h, w), dtype=torch.int32, device=first.device)
    n = 0
    for i in window_starts(d, p[0], o[0]):
        for j in window_starts(h, p[1], o[1]):
            for k in window_starts(w, p[2], o[2]):
                acc[..., i:i + p[0], j:j + p[1], k:k + p[2]] += patch_list[n]
                cnt[i:i + p[0], j:j + p[1], k:k + p[2]] += 1
                n += 1
    if n != len(patch_list):
        raise RuntimeError(f"{len(patch_list)} patches for a grid of {n}")
    return acc / cnt


@torch.no_grad()
def sliding_window_forward(model, images: torch.Tensor, patch_size=64, overlap=16) -> torch.Tensor:
    """validate_seg's inner loop (validate.py:236-245): split, run the model on every patch, stitch.
    `model(patch)` may return one tensor or a list of heads; the result is heads x N x C x D x H x W."""
    patches = image_to_patch3d(images, patch_size, overlap)
    preds = []
    for pt in patches:
        out = model(pt.contiguous())
        if isinstance(out, (list, tuple)):
            out = torch.stack(list(out))
        elif out.dim() == images.dim():          # a single head
            out = out.unsqueeze(0)
        preds.append(out)                        # heads x N x C x d x h x w (UResQ returns its heads stacked)
    return patch_to_image3d(images, preds, patch_size, overlap)


def _last_head(out) -> torch.Tensor:
    """The last head of a model output: a list of heads, heads stacked in front (UResQ), or one N x C x ... tensor."""
    if isinstance(out, (list, tuple)):
        return out[-1]
    return out[-1] if out.dim() == 6 else out


MIRROR_AXES = "dhw"                      # --tta_mirror: bit i of a flip mask mirrors axis MIRROR_AXES[i]


def mirror_flips(axes) -> tuple:
    """The flip masks of --tta_mirror `axes`, ascending: every subset of the named axes, the empty one (mask 0, the
    un-mirrored pass) included - "w" -> (0, 4), "hw" -> (0, 2, 4, 6), "dhw" -> (0, ..., 7).  None: (0,).  `axes` is a
    non-empty string over d, h, w with no letter twice; anything else is a ValueError."""
    if axes is None:
        return (0,)
    if not isinstance(axes, str) or not axes or any(a not in MIRROR_AXES for a in axes) or len(set(axes)) != len(axes):
        raise ValueError(f"{axes!r}: a non-empty string over the letters d, h, w, each at most once (w, hw, dhw, ...)")
    bits = sum(1 << MIRROR_AXES.index(a) for a in axes)
    return tuple(m for m in range(8) if m & ~bits == 0)


def check_flips(flips) -> tuple:
    """`flips` as a tuple of distinct masks 0..7 in ascending order; a ValueError otherwise."""
    f = tuple(flips)
    if not f or any(isinstance(m, bool) or not isinstance(m, int) or not 0 <= m <= 7 for m in f) or \
            list(f) != sorted(set(f)):
        raise ValueError(f"flips {flips!r}: distinct flip masks 0..7 in ascending order, at least one")
    return f


@torch.no_grad()
def stitched_window_logits(ops, nets, vol: torch.Tensor, patch, overlap, window_batch=None, blend="uniform",
                           flips=(0,)):
    """The sliding-window forward of validate_seg and of the `predict` mission: the windows of `vol` (N x C x D x H x W
    fp32 on the device of `ops`) gathered into batches of `window_batch`, once per mask of `flips` and mirrored by it
    (effq_window_gather); every network of `nets` run on each; its last head un-mirrored into the network's window
    buffer, the first pass stored and the others added, so the buffer keeps its size (effq_window_put); and the buffer
    stitched and divided by the number of passes (effq_window_stitch): the logits are averaged, not the probabilities.
    window_batch=None: the first window runs alone and its peak memory - over all the forwards of `nets` - sizes the
    batches, half the free device memory at most WINDOW_BATCH_MAX windows.  Returns (one stitched N x classes x D x H x
    W tensor per network, the number of windows, the window batch in use): a caller hands the last back in for its next
    volume.
    blend: "uniform" (every covering window counts alike) or "gauss" (a window's voxels are weighted by a separable
    Gaussian of sigma = patch / 8 around its centre, hip_ops.blend_weights_host).  flips: the flip masks of mirror
    test-time augmentation (mirror_flips), ascending."""
    from .hip_ops import from_ndhwc
    if blend not in BLEND_KINDS:
        raise ValueError(f"blend {blend!r}: one of {', '.join(BLEND_KINDS)}")
    flips = check_flips(flips)
    dev = vol.device
    p, o = _triple(patch), _triple(overlap)
    bsz = window_batch
    N = int(vol.shape[0])
    nwin = 1
    for n in ops.window_grid(vol.shape[-3:], p, o):
        nwin *= n
    bufs = [None] * len(nets)
    first = 0
    while first < nwin:
        cnt = min(bsz or 1, nwin - first)
        if bsz is None:
            torch.cuda.synchronize(dev)
            base = torch.cuda.memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
        for m in flips:                         # the peak below covers every forward of every pass
            x = from_ndhwc(ops.window_gather(vol, p, o, first, cnt, m))
            for k, net in enumerate(nets):
                last = _last_head(net(x))
                if bufs[k] is None:
                    bufs[k] = torch.empty(nwin * N, *p, int(last.shape[1]), dtype=torch.float32, device=dev)
                ops.window_put(last, bufs[k][first * N:(first + cnt) * N], m, m != flips[0])
                del last
            del x
        if bsz is None:
            per = max(1, torch.cuda.max_memory_allocated(dev) - base)
            free, _ = torch.cuda.mem_get_info(dev)
            bsz = int(max(1, min(WINDOW_BATCH_MAX, free // 2 // per)))
        first += cnt
    full = (N,) + tuple(bufs[0].shape[-1:]) + tuple(vol.shape[-3:])
    weights = None if blend == "uniform" else ops.blend_weights(p, blend)
    return [ops.window_stitch(b, full, p, o, weights, len(flips)) for b in bufs], nwin, bsz
