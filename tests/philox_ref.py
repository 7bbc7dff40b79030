"""Pure-numpy reference of the block dropout masks (csrc/dropout.hip, include/factorizer_hip.h "block dropout"):
Philox4x32-10, the keep rule and the packed bit layout.  Shared by tests/test_dropout_cpu.py and tests/test_gpu_dropout.py."""
from __future__ import annotations

import numpy as np

MASK32 = 0xFFFFFFFF
M0, M1 = 0xD2511F53, 0xCD9E8D57   # Philox4x32 multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85   # Weyl key increments

# Random123 known-answer vectors (kat_vectors, philox4x32 with 10 rounds): (counter, key, output)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((MASK32,) * 4, (MASK32,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """elementwise over numpy arrays (or ints) of 32-bit values; returns four uint64 arrays holding 32-bit words"""
    c0, c1, c2, c3, k0, k1 = (np.asarray(v, dtype=np.uint64) for v in (c0, c1, c2, c3, k0, k1))
    m = np.uint64(MASK32)
    for _ in range(10):
        p0 = np.uint64(M0) * c0
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m
        k0 = (k0 + np.uint64(W0)) & m
        k1 = (k1 + np.uint64(W1)) & m
    return c0, c1, c2, c3


def keep_threshold(p):
    """floor((1 - p) 2^32) with p rounded to float32 first, as the library receives it"""
    return int((1.0 - float(np.float32(p))) * 4294967296.0)


def keep_mask(seed, site, B, ch, V, p):
    """bool array (B, ch, V): element (b, c, v) kept iff word v & 3 of Philox((v >> 2, c, b, site), (seed lo, seed hi)) < thr"""
    seed = int(seed)
    k0, k1 = seed & MASK32, (seed >> 32) & MASK32
    nq = (V + 3) // 4
    b, c, q = np.meshgrid(np.arange(B), np.arange(ch), np.arange(nq), indexing="ij")
    r = philox4x32_10(q, c, b, np.full_like(q, site), k0, k1)
    words = np.stack(r, axis=-1).reshape(B, ch, 4 * nq)[..., :V]
    return words < np.uint64(keep_threshold(p))


def pack_bits(keep):
    """bool (B, ch, V) -> int32 (B, ch, ceil(V / 32)): bit v & 31 of word v >> 5, padding bits 0"""
    B, ch, V = keep.shape
    nw = (V + 31) // 32
    pad = np.zeros((B, ch, nw * 32), dtype=np.uint64)
    pad[..., :V] = keep
    w = (pad.reshape(B, ch, nw, 32) << np.arange(32, dtype=np.uint64)).sum(-1)
    return w.astype(np.uint32).view(np.int32)


def keep_bits(seed, site, B, ch, V, p):
    return pack_bits(keep_mask(seed, site, B, ch, V, p))
