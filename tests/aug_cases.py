"""Fixed inputs of the augmentation tests (tests/test_augment_cpu.py, tests/test_gpu_augment.py): images uniform in [0, 1),
labels random uint8 in 0..3, six matrices per rank whose angles span +-0.26 and scales 0.8 .. 1.2, every flip subset."""
from __future__ import annotations

import numpy as np
import torch

import aug_ref as R

SHAPE3, SHAPE2 = (2, 3, 20, 24, 28), (3, 2, 33, 47)

# (angles, scales, flip) of the drawn samples
MATS3 = [
    ((0.26, 0.26, 0.26), (1.2, 1.2, 1.2), (0, 0, 0)),
    ((-0.26, 0.1, -0.2), (0.8, 1.1, 1.2), (1, 0, 0)),
    ((0.13, -0.26, 0.05), (1.2, 0.8, 1.0), (0, 1, 0)),
    ((-0.2, -0.15, 0.26), (0.9, 1.2, 0.8), (0, 0, 1)),
    ((0.26, -0.26, -0.26), (0.8, 0.8, 0.8), (1, 1, 0)),
    ((0.05, 0.2, -0.1), (1.1, 0.9, 1.15), (1, 0, 1)),
]
IDENT_FLIPS3 = [(0, 1, 1), (1, 1, 1), (0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)]   # flips of the identity sample of case i
MATS2 = [
    ((0.26,), (1.2, 1.2), (0, 0)),
    ((-0.26,), (0.8, 1.15), (1, 0)),
    ((0.13,), (1.2, 0.8), (0, 1)),
    ((-0.26,), (0.8, 1.2), (1, 1)),
    ((0.26,), (0.9, 1.2), (0, 1)),
    ((-0.07,), (1.1, 1.0), (1, 0)),
]
IDENT_FLIPS2 = [(1, 1), (0, 0), (1, 0)]


def image(shape, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g).to(dtype)


def label(shape, seed, channels=1):
    g = torch.Generator().manual_seed(seed + 1000)
    return torch.randint(0, 4, (shape[0], channels, *shape[2:]), generator=g, dtype=torch.uint8)


def resample_cases(nd):
    """list of (shape, affine (B, nd, nd) fp32 tensor, flip (B, nd) bool tensor): one identity sample per batch, at a
    position that moves with the case"""
    out = []
    if nd == 3:
        for i, (ang, sc, fl) in enumerate(MATS3):
            A = np.stack([R.matrix(ang, sc, 3), np.eye(3)])
            F = np.array([fl, IDENT_FLIPS3[i]], dtype=bool)
            if i % 2:
                A, F = A[::-1].copy(), F[::-1].copy()
            out.append((SHAPE3, torch.tensor(A, dtype=torch.float32), torch.tensor(F)))
    else:
        for i in range(3):
            (a0, s0, f0), (a1, s1, f1) = MATS2[2 * i], MATS2[2 * i + 1]
            A = [R.matrix(a0, s0, 2), R.matrix(a1, s1, 2)]
            F = [f0, f1]
            A.insert(i, np.eye(2))
            F.insert(i, IDENT_FLIPS2[i])
            out.append((SHAPE2, torch.tensor(np.stack(A), dtype=torch.float32), torch.tensor(np.array(F, dtype=bool))))
    return out


def all_flip_subsets_appear(nd):
    seen = set()
    for _, _, F in resample_cases(nd):
        seen |= {tuple(int(v) for v in row) for row in F.tolist()}
    return len(seen) == 2 ** nd
