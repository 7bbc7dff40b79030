"""Independent float64 / int64 numpy restatement of the batch augmentations (factorizer_amd/augment.py states the contract;
this file shares no code with it).  Shared by tests/test_augment_cpu.py and tests/test_gpu_augment.py.

A batch: image (B, C, *S), label (B, L, *S); per sample a matrix A (nd x nd), flips (nd), noise std, sigma (nd), gain, offset.
Steps per sample: gather at p = A (o' - c) + c clamped to the image (image: multilinear, label: floor(p + 0.5)); += std * z;
separable zero-padded convolution with erf-difference taps; * gain + offset.  Everything here is float64 on the fp32 values of
the records; the taps are rounded to fp32 as the contract says."""
from __future__ import annotations

import itertools
import math

import numpy as np

from philox_ref import MASK32, philox4x32_10

NOISE_STREAM = 0x41554731


# ---- noise: Philox words -> normals (the Box-Muller step restated on the host) ----------------------------------------------
def box_muller(words):
    """words: four arrays of 32-bit values (one Philox output per entry) -> float64 array (..., 4) of normals:
    u_i = ((w_i >> 8) + 0.5) 2^-24; (z0, z1) = sqrt(-2 ln u0) (cos, sin)(2 pi u1); (z2, z3) likewise from (u2, u3)"""
    u = [((np.asarray(w, dtype=np.uint64) >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24 for w in words]
    out = []
    for i in (0, 2):
        r = np.sqrt(-2.0 * np.log(u[i]))
        a = 2.0 * np.pi * u[i + 1]
        out += [r * np.cos(a), r * np.sin(a)]
    return np.stack(out, axis=-1)


def noise_field(shape, seed):
    """float64 (B, C, *S): element (b, c, v) = normal v & 3 of counter (v >> 2, c, b, NOISE_STREAM), key (seed lo, seed hi)"""
    B, C = shape[:2]
    V = int(np.prod(shape[2:]))
    seed = int(seed)
    k0, k1 = seed & MASK32, (seed >> 32) & MASK32
    nq = (V + 3) // 4
    b, c, q = np.meshgrid(np.arange(B), np.arange(C), np.arange(nq), indexing="ij")
    z = box_muller(philox4x32_10(q, c, b, np.full_like(q, NOISE_STREAM), k0, k1))
    return z.reshape(B, C, 4 * nq)[..., :V].reshape(shape)


# ---- taps ---------------------------------------------------------------------------------------------------------------
def tail_of(sigma):
    return int(max(4.0 * sigma, 0.5) + 0.5)


def taps(sigma):
    """float64 array of the fp32-rounded taps for x = -tail .. tail"""
    t = 0.70710678 / sigma
    n = tail_of(sigma)
    w = [max(0.0, 0.5 * (math.erf(t * (x + 0.5)) - math.erf(t * (x - 0.5)))) for x in range(-n, n + 1)]
    return np.asarray(w, dtype=np.float64).astype(np.float32).astype(np.float64)


# ---- geometry ---------------------------------------------------------------------------------------------------------------
def rotation(angles, nd):
    if nd == 2:
        c, s = math.cos(angles[0]), math.sin(angles[0])
        return np.array([[c, -s], [s, c]])
    (c0, s0), (c1, s1), (c2, s2) = [(math.cos(a), math.sin(a)) for a in angles]
    rx = np.array([[1, 0, 0], [0, c0, -s0], [0, s0, c0]], dtype=np.float64)
    ry = np.array([[c1, 0, s1], [0, 1, 0], [-s1, 0, c1]], dtype=np.float64)
    rz = np.array([[c2, -s2, 0], [s2, c2, 0], [0, 0, 1]], dtype=np.float64)
    return rx @ ry @ rz


def matrix(angles, scales, nd):
    """A = R diag(s), rounded to fp32 (the precision of a record), as float64"""
    return (rotation(angles, nd) * np.asarray(scales, dtype=np.float64)[None, :]).astype(np.float32).astype(np.float64)


def positions(A, flip, spatial):
    """(unclamped, clamped) source positions, each (nd, *S) float64"""
    nd = len(spatial)
    axes = []
    for k, n in enumerate(spatial):
        o = np.arange(n, dtype=np.float64)
        if flip[k]:
            o = (n - 1) - o
        axes.append(o - (n - 1) / 2.0)
    d = np.stack(np.meshgrid(*axes, indexing="ij"))                        # (nd, *S)
    p = np.tensordot(np.asarray(A, dtype=np.float64), d, axes=(1, 0))
    for k, n in enumerate(spatial):
        p[k] += (n - 1) / 2.0
    pc = np.stack([np.clip(p[k], 0.0, n - 1.0) for k, n in enumerate(spatial)])
    return p, pc


def clamp_share(A, flip, spatial):
    """fraction of output voxels whose source position is clamped on at least one axis"""
    p, pc = positions(A, flip, spatial)
    return float(np.any(p != pc, axis=0).mean())


def near_half(A, flip, spatial, eps=1e-3):
    """bool (*S): the clamped position lies within eps of a half-integer on some axis (nearest may round either way in fp32)"""
    _, pc = positions(A, flip, spatial)
    frac = pc - np.floor(pc)
    return np.any(np.abs(frac - 0.5) <= eps, axis=0)


def resample_image(x, A, flip):
    """x (C, *S) -> float64 (C, *S), multilinear at the clamped positions"""
    x = np.asarray(x, dtype=np.float64)
    spatial = x.shape[1:]
    nd = len(spatial)
    _, pc = positions(A, flip, spatial)
    i0 = np.floor(pc).astype(np.int64)
    f = pc - i0
    i1 = np.stack([np.minimum(i0[k] + 1, n - 1) for k, n in enumerate(spatial)])
    out = np.zeros(x.shape, dtype=np.float64)
    for corner in itertools.product((0, 1), repeat=nd):
        w = np.ones(spatial, dtype=np.float64)
        idx = []
        for k, hi in enumerate(corner):
            w = w * (f[k] if hi else 1.0 - f[k])
            idx.append(i1[k] if hi else i0[k])
        out += w[None] * x[(slice(None),) + tuple(idx)]
    return out


def resample_label(l, A, flip):
    l = np.asarray(l)
    _, pc = positions(A, flip, l.shape[1:])
    idx = tuple(np.floor(pc + 0.5).astype(np.int64))
    return l[(slice(None),) + idx]


def smooth(x, sigma):
    """x (C, *S) float64; zero padding; one pass per axis with sigma > 0"""
    x = np.asarray(x, dtype=np.float64)
    for k, s in enumerate(sigma):
        if s <= 0:
            continue
        w = taps(float(s))
        n = (len(w) - 1) // 2
        ax = 1 + k
        N = x.shape[ax]
        pad = [(0, 0)] * x.ndim
        pad[ax] = (n, n)
        xp = np.pad(x, pad)
        acc = np.zeros_like(x)
        for j, wj in enumerate(w):
            acc += wj * np.take(xp, np.arange(j, j + N), axis=ax)
        x = acc
    return x


def augment(image, label, affine, flip, noise_std, sigma, gain, offset, noise=None):
    """the whole contract; image (B, C, *S) / label (B, L, *S) numpy (either None); the records as arrays over the batch
    (fp32 values, used as float64); noise (B, C, *S) float64 = the field.  Returns float64 image, label."""
    out_i = None if image is None else np.zeros(image.shape, dtype=np.float64)
    out_l = None if label is None else np.zeros_like(label)
    B = (image if image is not None else label).shape[0]
    for b in range(B):
        A = np.asarray(affine[b], dtype=np.float64)
        fl = [bool(v) for v in flip[b]]
        if label is not None:
            out_l[b] = resample_label(label[b], A, fl)
        if image is None:
            continue
        x = resample_image(image[b], A, fl)
        if float(noise_std[b]) > 0:
            x = x + float(noise_std[b]) * noise[b]
        x = smooth(x, [float(s) for s in sigma[b]])
        out_i[b] = x * float(gain[b]) + float(offset[b])
    return out_i, out_l
