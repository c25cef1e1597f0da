"""Labelled volumes in the reference's data layout (README "Dataset preparation", src/dataloader/{datahub,datasets}.py,
src/definer.py:get_data_cube):

    data_dir/<modality>/<subject>.npy      (--access_type npy; .npz holds the array under the key arr_0)
    split_dir/round<R>/train.txt, val.txt  (one subject per line)

Modalities are flair, t1, t1ce, t2 for brats and ct for lits; the label is the modality ``seg``.  Subjects are
taken in sorted order, as the reference's Dataset_SEG loads them.  Images are used as stored: the reference's README
asks for volumes already standardised to zero mean and unit variance, and no augmentation or random crop is applied.
The returned cube has the interface ``calibrate.get_calibration_data`` and the validation tester use:
``trainseqloader`` (train split, batch 1, no shuffle, ``dataset.use_fix_transform()``), ``valloader`` and the
subject names ``train_sn`` / ``val_sn``.
"""
from __future__ import annotations

import os.path as P
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
    """(image C x D x H x W float32, label) per subject, read from disk when indexed."""

    def __init__(self, data_dir: str, subjects: Sequence[str], modalities: Sequence[str], access_type: str = "npy",
                 label_fn: Optional[Callable] = None):
        if access_type not in ACCESS_TYPES:
            raise RuntimeError(f"Unknown access type {access_type} (one of {', '.join(ACCESS_TYPES)})")
        self.data_dir, self.subjects, self.modalities = data_dir, list(subjects), tuple(modalities)
        self.access_type, self.label_fn = access_type, label_fn

    def __len__(self):
        return len(self.subjects)

    def __getitem__(self, i):
        sn = self.subjects[i]
        img = np.stack([load_array(self.data_dir, m, sn, self.access_type, np.float32) for m in self.modalities])
        label = torch.from_numpy(load_array(self.data_dir, LABEL_MODALITY, sn, self.access_type, np.uint8)).long()
        if self.label_fn is not None:
            label = self.label_fn(label)
        return torch.from_numpy(img), label

    def use_fix_transform(self):
        """There is only the fixed transform (no augmentation, no random crop)."""


class DataCube:
    def __init__(self, data_dir, split_dir, round_, task, access_type="npy", bin_label=None, multi_label=None,
                 merge_type=None, patch_size=None):
        task = task.lower()
        if task not in MODALITIES:
            raise RuntimeError(f"Unknown task: {task}")
        split = P.join(split_dir, f"round{round_}")
        self.train_sn = read_split(P.join(split, "train.txt"))
        self.val_sn = read_split(P.join(split, "val.txt")) if P.isfile(P.join(split, "val.txt")) else []
        fn = label_transform(bin_label, multi_label)
        mk = lambda names: SegVolumes(data_dir, names, MODALITIES[task], access_type, fn)
        self.trainseqloader = torch.utils.data.DataLoader(mk(self.train_sn), 1, shuffle=False)
        self.valloader = torch.utils.data.DataLoader(mk(self.val_sn), 1, shuffle=False) if self.val_sn else None
        self.multi_label = multi_label
        self.multilabel_fusetype = merge_type
        self.patch_size = parse_patch(patch_size) if patch_size else PATCH_DEFAULT[task]
        self.overlap = OVERLAP_DEFAULT


def parse_patch(s) -> tuple:
    if isinstance(s, (tuple, list)):
        return tuple(int(v) for v in s)
    s = str(s)
    return tuple(int(v) for v in s.split(",")) if "," in s else (int(s),) * 3


def get_data_cube(args) -> DataCube:
    """The data cube of `args` (--data_dir, --split_dir, --round, --task, --access_type, --bin_label, --multi_label,
    --merge_type, --patch_size)."""
    return DataCube(args.data_dir, args.split_dir, args.round, args.task, getattr(args, "access_type", "npy"),
                    getattr(args, "bin_label", None), getattr(args, "multi_label", None),
                    getattr(args, "merge_type", None), getattr(args, "patch_size", None))
