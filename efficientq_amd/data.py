"""Labelled volumes in the reference's data layout (README "Dataset preparation", src/dataloader/{datahub,datasets}.py,
src/definer.py:get_data_cube):

    data_dir/<modality>/<subject>.npy      (--access_type npy; .npz holds the array under the key arr_0)
    split_dir/round<R>/train.txt, val.txt  (one subject per line)

With ``--src_geom`` two more files of the reference's layout are read (datahub.py:51, definer.py:113-123):

    data_dir/sn_fn.txt                      ``subject,path`` per line: the subject's source NIfTI image
    data_dir/restore_shape_infokw.pickle    optional: {subject: {pmin, pmax, shape}}, how the arrays were cropped

Modalities are flair, t1, t1ce, t2 for brats and ct for lits; the label is the modality ``seg`` (never opened with
``--unlabelled``: every subject then carries an empty label).  Subjects are
taken in sorted order, as the reference's Dataset_SEG loads them.  Images are used as stored: the reference's README
asks for volumes already standardised to zero mean and unit variance, and no augmentation or random crop is applied.
The returned cube has the interface ``calibrate.get_calibration_data`` and the validation tester use:
``trainseqloader`` (train split, batch 1, no shuffle, ``dataset.use_fix_transform()``), ``valloader`` and the
subject names ``train_sn`` / ``val_sn``.
"""
from __future__ import annotations

import math
import os.path as P
import pickle
from zlib import error as zlib_error
from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

MODALITIES = {"brats": ("flair", "t1", "t1ce", "t2"), "lits": ("ct",)}
LABEL_MODALITY = "seg"
ACCESS_TYPES = ("npy", "npz")
# sliding-window defaults of get_data_cube: window extent and overlap per task
PATCH_DEFAULT = {"brats": (128, 128, 128), "lits": (128, 128, 64)}
OVERLAP_DEFAULT = 16


def read_split(path: str) -> List[str]:
    """Subject names of a split file, sorted; blank lines are ignored."""
    with open(path, "r") as f:
        return sorted(line.strip() for line in f.read().splitlines() if line.strip())


def load_array(data_dir: str, modality: str, subject: str, access_type: str, dtype) -> np.ndarray:
    if access_type == "npy":
        a = np.load(P.join(data_dir, modality, f"{subject}.npy"))
    elif access_type == "npz":
        with np.load(P.join(data_dir, modality, f"{subject}.npz")) as z:
            a = z["arr_0"]
    else:
        raise RuntimeError(f"Unknown access type {access_type} (one of {', '.join(ACCESS_TYPES)})")
    return a.astype(dtype, copy=False)


# ---- source geometry (--src_geom, --spacing) --------------------------------------------------------------------------
SN_FN_FILE = "sn_fn.txt"
RESTORE_FILE = "restore_shape_infokw.pickle"


def read_sn_fn(data_dir: str) -> dict:
    """{subject: path of its source NIfTI image} from data_dir/sn_fn.txt, ``subject,path`` per line (the reference's
    file_to_dict); a relative path is taken relative to `data_dir`.  Blank lines are ignored."""
    out = {}
    with open(P.join(data_dir, SN_FN_FILE), "r") as f:
        for line in f.read().splitlines():
            if not line.strip():
                continue
            if line.count(",") != 1:
                raise RuntimeError(f"{SN_FN_FILE}: line {line!r} is not `subject,path`")
            sn, path = (s.strip() for s in line.split(","))
            out[sn] = path if P.isabs(path) else P.join(data_dir, path)
    return out


def read_restore_info(data_dir: str) -> Optional[dict]:
    """{subject: {pmin, pmax, shape}} - the keyword arguments of restore_crop - from
    data_dir/restore_shape_infokw.pickle, or None when the file does not exist.  Unpickling runs code: this is called
    under --src_geom only, on the user's own data_dir."""
    path = P.join(data_dir, RESTORE_FILE)
    if not P.isfile(path):
        return None
    with open(path, "rb") as f:
        return pickle.load(f)


def restore_crop(crop: np.ndarray, pmin, pmax, shape) -> np.ndarray:
    """`crop` put back into a volume of zeros of extent `shape` at pmin:pmax (misc.restore_crop for three axes)."""
    out = np.zeros(tuple(int(n) for n in shape), dtype=crop.dtype)
    out[pmin[0]:pmax[0], pmin[1]:pmax[1], pmin[2]:pmax[2]] = crop
    return out


def array_shape(data_dir: str, modality: str, subject: str, access_type: str) -> tuple:
    if access_type == "npy":
        return tuple(np.load(P.join(data_dir, modality, f"{subject}.npy"), mmap_mode="r").shape)
    return tuple(load_array(data_dir, modality, subject, access_type, np.uint8).shape)


def read_source_geometry(data_dir: str, subjects: Sequence[str], access_type: str = "npy",
                         modality: str = LABEL_MODALITY) -> List[dict]:
    """One entry per subject for --src_geom: `affine`, `spacing`, `source_shape` and `header` (nifti.read_geometry of the
    image sn_fn.txt names) and, when the subject's array is a crop of it, `pmin` / `pmax`.  Every failure names the
    subject.  `modality` is the array whose shape is compared with the source's (an image modality when there are no
    labels)."""
    from .nifti import read_geometry
    if not P.isfile(P.join(data_dir, SN_FN_FILE)):
        raise RuntimeError(f"--src_geom: {P.join(data_dir, SN_FN_FILE)} is missing (needed for {', '.join(subjects)})")
    sn_fn = read_sn_fn(data_dir)
    restore = read_restore_info(data_dir) or {}
    out = []
    for sn in subjects:
        if sn not in sn_fn:
            raise RuntimeError(f"--src_geom: subject {sn} has no line in {SN_FN_FILE}")
        try:
            hdr = read_geometry(sn_fn[sn])
        except (OSError, ValueError, EOFError, zlib_error) as e:
            raise RuntimeError(f"--src_geom: subject {sn}: cannot read the geometry of {sn_fn[sn]}: {e}") from e
        src = tuple(hdr["shape"][:3])
        entry = {"affine": hdr["affine"], "spacing": hdr["spacing"], "source_shape": src, "header": hdr}
        have = array_shape(data_dir, modality, sn, access_type)
        if have != src:
            kw = restore.get(sn)
            ok = kw is not None and tuple(int(n) for n in kw["shape"]) == src and \
                tuple(int(b) - int(a) for a, b in zip(kw["pmin"], kw["pmax"])) == have
            if not ok:
                raise RuntimeError(f"--src_geom: subject {sn}: array of shape {have}, source image of shape {src}"
                                   + (f", restore entry pmin {tuple(kw['pmin'])} pmax {tuple(kw['pmax'])} shape "
                                      f"{tuple(kw['shape'])}" if kw is not None else f", no entry in {RESTORE_FILE}"))
            entry["pmin"] = tuple(int(v) for v in kw["pmin"])
            entry["pmax"] = tuple(int(v) for v in kw["pmax"])
        out.append(entry)
    return out


def parse_spacing(s) -> tuple:
    """--spacing d,h,w: three finite positive numbers (millimetres per voxel along D, H, W)."""
    try:
        v = tuple(float(x) for x in (s.split(",") if isinstance(s, str) else s))
    except (TypeError, ValueError):
        v = ()
    if len(v) != 3 or not all(math.isfinite(x) and x > 0 for x in v):
        raise RuntimeError(f"--spacing {s!r}: needs three finite positive numbers d,h,w")
    return v


# ---- label transforms (definer.py: --bin_label / --multi_label; misc.split_label_*) -----------------------------------
def label_binary(label: torch.Tensor) -> torch.Tensor:
    return (label > 0).long()


def label_split_brats(label: torch.Tensor) -> torch.Tensor:
    """BraTS class ids 0 / 1 (necrosis) / 2 (oedema) / 3 (enhancing, after the usual 4 -> 3 remap) to three nested
    0/1 channels: whole tumour (> 0), tumour core (1 or 3), enhancing tumour (3)."""
    return torch.stack([label > 0, (label == 1) | (label == 3), label == 3]).float()


def label_split_lits(label: torch.Tensor) -> torch.Tensor:
    """LiTS class ids 0 / 1 (liver) / 2 (tumour) to two nested 0/1 channels: liver incl. tumour (> 0), tumour (2)."""
    return torch.stack([label > 0, label == 2]).float()


def label_transform(bin_label=None, multi_label=None) -> Optional[Callable]:
    """The label transform get_data_cube selects: --multi_label wins over --bin_label."""
    fn = None
    if bin_label:
        fn = label_binary
    if multi_label:
        key = multi_label.lower()
        if key == "brats":
            fn = label_split_brats
        elif key == "lits":
            fn = label_split_lits
        else:
            raise RuntimeError(f"Unknown multi_label {multi_label}")
    return fn


class SegVolumes(torch.utils.data.Dataset):
    """(image C x D x H x W float32, label) per subject, read from disk when indexed.  labels=False: seg/ is never
    opened and the label is an empty uint8 tensor (evaluate.validate_seg takes such a case as unlabelled)."""

    def __init__(self, data_dir: str, subjects: Sequence[str], modalities: Sequence[str], access_type: str = "npy",
                 label_fn: Optional[Callable] = None, labels: bool = True):
        if access_type not in ACCESS_TYPES:
            raise RuntimeError(f"Unknown access type {access_type} (one of {', '.join(ACCESS_TYPES)})")
        self.data_dir, self.subjects, self.modalities = data_dir, list(subjects), tuple(modalities)
        self.access_type, self.label_fn, self.labels = access_type, label_fn, labels

    def __len__(self):
        return len(self.subjects)

    def __getitem__(self, i):
        sn = self.subjects[i]
        img = np.stack([load_array(self.data_dir, m, sn, self.access_type, np.float32) for m in self.modalities])
        if not self.labels:
            return torch.from_numpy(img), torch.empty(0, dtype=torch.uint8)
        label = torch.from_numpy(load_array(self.data_dir, LABEL_MODALITY, sn, self.access_type, np.uint8)).long()
        if self.label_fn is not None:
            label = self.label_fn(label)
        return torch.from_numpy(img), label

    def use_fix_transform(self):
        """There is only the fixed transform (no augmentation, no random crop)."""


class DataCube:
    def __init__(self, data_dir, split_dir, round_, task, access_type="npy", bin_label=None, multi_label=None,
                 merge_type=None, patch_size=None, src_geom=False, spacing=None, labels=True):
        task = task.lower()
        if task not in MODALITIES:
            raise RuntimeError(f"Unknown task: {task}")
        split = P.join(split_dir, f"round{round_}")
        self.train_sn = read_split(P.join(split, "train.txt"))
        self.val_sn = read_split(P.join(split, "val.txt")) if P.isfile(P.join(split, "val.txt")) else []
        fn = label_transform(bin_label, multi_label)
        mk = lambda names: SegVolumes(data_dir, names, MODALITIES[task], access_type, fn, labels)
        self.trainseqloader = torch.utils.data.DataLoader(mk(self.train_sn), 1, shuffle=False)
        self.valloader = torch.utils.data.DataLoader(mk(self.val_sn), 1, shuffle=False) if self.val_sn else None
        self.multi_label = multi_label
        self.labelled = labels
        self.multilabel_fusetype = merge_type
        self.patch_size = parse_patch(patch_size) if patch_size else PATCH_DEFAULT[task]
        self.overlap = OVERLAP_DEFAULT
        # where the val subjects lie in space: one entry per subject (--src_geom), or one spacing for all (--spacing)
        self.geometry = self.spacing = None
        if src_geom and spacing:
            raise RuntimeError("--src_geom and --spacing exclude each other: the source images carry their own spacing")
        if src_geom:
            self.geometry = read_source_geometry(data_dir, self.val_sn, access_type,
                                                 LABEL_MODALITY if labels else MODALITIES[task][0])
        elif spacing:
            self.spacing = parse_spacing(spacing)


def parse_patch(s) -> tuple:
    if isinstance(s, (tuple, list)):
        return tuple(int(v) for v in s)
    s = str(s)
    return tuple(int(v) for v in s.split(",")) if "," in s else (int(s),) * 3


def get_data_cube(args) -> DataCube:
    """The data cube of `args` (--data_dir, --split_dir, --round, --task, --access_type, --bin_label, --multi_label,
    --merge_type, --patch_size, --src_geom, --spacing, --unlabelled)."""
    return DataCube(args.data_dir, args.split_dir, args.round, args.task, getattr(args, "access_type", "npy"),
                    getattr(args, "bin_label", None), getattr(args, "multi_label", None),
                    getattr(args, "merge_type", None), getattr(args, "patch_size", None),
                    getattr(args, "src_geom", False), getattr(args, "spacing", None),
                    not getattr(args, "unlabelled", False))
