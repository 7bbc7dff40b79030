"""Independent float64 restatement, in numpy, of the orientation / spacing / pad chain and its inverse that
factorizer_amd/respace.py runs — written from the contract (the module docstring there), not from the implementation: the
geometry goes through explicit affines, the sampling through explicit per-axis index / weight tables and a weighted sum over
the corners (no nested lerp), mirrored axes through np.flip of the array.  Shared by tests/test_respace_cpu.py and
tests/test_gpu_respace.py; also the shapes both use."""
import itertools
import math

import numpy as np

WORLD = {"L": (0, -1), "R": (0, 1), "P": (1, -1), "A": (1, 1), "I": (2, -1), "S": (2, 1)}
NAMES = (("L", "R"), ("P", "A"), ("I", "S"))


def all_codes(nd=3):
    """the 48 (nd = 3) signed axis permutations as code strings"""
    out = []
    for perm in itertools.permutations(range(nd)):
        for signs in itertools.product((0, 1), repeat=nd):
            out.append("".join(NAMES[w][s] for w, s in zip(perm, signs)))
    return out


def rotation(deg, nd):
    """a rotation by `deg` degrees about the axis (1, 2, 3) / sqrt(14) (3-D), in the plane (2-D), none (1-D)"""
    t = math.radians(deg)
    if nd == 1:
        return np.eye(1)
    if nd == 2:
        return np.array([[math.cos(t), -math.sin(t)], [math.sin(t), math.cos(t)]])
    k = np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(t) * K + (1 - math.cos(t)) * (K @ K)


def make_affine(code, zooms, deg=0.0, origin=None):
    """the affine of a grid whose voxel axis i grows towards code[i], `zooms[i]` mm per voxel, the whole rotated by `deg`"""
    nd = len(code)
    M = np.zeros((nd, nd))
    for i, c in enumerate(code):
        w, s = WORLD[c]
        M[w, i] = s * zooms[i]
    A = np.eye(nd + 1)
    A[:nd, :nd] = rotation(deg, nd) @ M
    A[:nd, nd] = np.arange(1, nd + 1) * 7.25 if origin is None else origin
    return A


def orientation(A):
    """[(world axis, sign)] per voxel axis"""
    nd = A.shape[0] - 1
    M = A[:nd, :nd].astype(np.float64)
    ln = np.sqrt((M * M).sum(0))
    ln[ln == 0] = 1.0
    U, S, Vt = np.linalg.svd(M / ln)
    keep = S > S.max() * nd * np.finfo(np.float64).eps
    R = U[:, keep] @ Vt[keep]
    free, out = list(range(nd)), []
    for i in range(nd):
        w = max(free, key=lambda r: abs(R[r, i]))
        free.remove(w)
        out.append((w, 1 if R[w, i] >= 0 else -1))
    return out


def code_of(A):
    return "".join(NAMES[w][s > 0] for w, s in orientation(A))


def half_even(v):
    f = math.floor(v)
    d = v - f
    if d > 0.5 or (d == 0.5 and f % 2 == 1):
        return int(f) + 1
    return int(f)


def geometry(size, A, pixdim, axcodes="RAS", box_start=None, roi=None, orig_size=None):
    """dict: perm / flip (output axis w reads voxel axis perm[w], mirrored or not), n_or (oriented extents), zoom, res, pad,
    out, affine (of the resampled grid), start, orig"""
    nd = len(size)
    start = [0] * nd if box_start is None else list(box_start)
    Ac = np.array(A, dtype=np.float64)
    Ac[:nd, nd] = (Ac @ np.array(start + [1.0]))[:nd]                       # crop
    if axcodes is None:
        perm, flip = list(range(nd)), [False] * nd
    else:
        src = orientation(Ac)
        perm, flip = [], []
        for c in axcodes[:nd]:
            w, s = WORLD[c]
            i = [k for k, (ww, _) in enumerate(src) if ww == w][0]
            perm.append(i)
            flip.append(src[i][1] != s)
    n_or = [size[i] for i in perm]
    Ao = np.eye(nd + 1)
    Ao[:nd, nd] = Ac[:nd, nd]
    for w in range(nd):                                                      # orient
        col = Ac[:nd, perm[w]]
        if flip[w]:
            Ao[:nd, nd] += col * (n_or[w] - 1)
            col = -col
        Ao[:nd, w] = col
    zoom = [float(np.linalg.norm(Ao[:nd, w])) for w in range(nd)]
    pix = zoom if pixdim is None else ([float(pixdim)] * nd if np.isscalar(pixdim) else [float(p) for p in pixdim])
    res = [n if pixdim is None else half_even((n - 1) * z / p + 1) for n, z, p in zip(n_or, zoom, pix)]
    As = Ao.copy()
    for w in range(nd):                                                      # space
        As[:nd, w] = Ao[:nd, w] * (pix[w] / zoom[w])
    roi = res if roi is None else list(roi)
    out = [max(a, b) for a, b in zip(res, roi)]
    return dict(nd=nd, size=tuple(size), perm=perm, flip=flip, n_or=n_or, zoom=zoom, pix=pix, res=res,
                pad=[(o - r) // 2 for o, r in zip(out, res)], out=out, affine=As, start=start,
                orig=tuple(orig_size) if orig_size is not None else tuple(s + n for s, n in zip(start, size)))


def table(count, step, n):
    """positions step·o (o < count) clamped to [0, n − 1]: (p, i0, i1, weight of i1, rounded index)"""
    p = np.clip(np.arange(count, dtype=np.float64) * step, 0.0, n - 1.0)
    i0 = np.floor(p).astype(np.int64)
    i1 = np.minimum(i0 + 1, n - 1)
    return p, i0, i1, p - i0, np.rint(p).astype(np.int64)                     # np.rint: half to even


def _oriented(x, g):
    """x (C, *size) in the oriented axis order, mirrored axes flipped"""
    xo = np.transpose(x, [0] + [1 + i for i in g["perm"]])
    mirrored = [1 + w for w in range(g["nd"]) if g["flip"][w]]
    return np.flip(xo, mirrored) if mirrored else xo


def _interp(x, tabs):
    """x (C, *n) float64 sampled at the product of the per-axis tables: the weighted sum over the 2^nd corners"""
    nd = len(tabs)
    out = 0.0
    for corner in itertools.product((0, 1), repeat=nd):
        v, wgt = x, 1.0
        for ax, c in enumerate(corner):
            _, i0, i1, f, _ = tabs[ax]
            v = np.take(v, i1 if c else i0, axis=1 + ax)
            shape = [1] * (nd + 1)
            shape[1 + ax] = -1
            wgt = wgt * (f if c else 1.0 - f).reshape(shape)
        out = out + wgt * v
    return out


def _nearest(x, tabs):
    for ax, t in enumerate(tabs):
        x = np.take(x, t[4], axis=1 + ax)
    return x


def _padded(v, g):
    out = np.zeros((v.shape[0],) + tuple(g["out"]), dtype=v.dtype)
    out[(slice(None),) + tuple(slice(b, b + n) for b, n in zip(g["pad"], g["res"]))] = v
    return out


def forward(x, g, mode="bilinear"):
    """x (C, *size) -> (C, *out): float64 for bilinear, x's dtype for nearest"""
    tabs = [table(g["res"][w], g["pix"][w] / g["zoom"][w], g["n_or"][w]) for w in range(g["nd"])]
    if mode == "nearest":
        return _padded(_nearest(_oriented(x, g), tabs), g)
    return _padded(_interp(_oriented(x, g).astype(np.float64), tabs), g)


def forward_positions(g):
    """per output axis the float64 position each unpadded output index reads, on the oriented grid"""
    return [table(g["res"][w], g["pix"][w] / g["zoom"][w], g["n_or"][w])[0] for w in range(g["nd"])]


def near_ties(g, tol=1e-9):
    """bool (res): output voxels whose position lies within tol of a half-integer on an axis whose scale is no dyadic rational"""
    nd = g["nd"]
    bad = np.zeros(g["res"], dtype=bool)
    for w in range(nd):
        s = g["pix"][w] / g["zoom"][w]
        m, e = math.frexp(s)
        if m * 2.0 ** 53 % 2.0 ** 33 == 0:       # at most 20 significant bits: s·o is exact for every index in use
            continue
        p = forward_positions(g)[w]
        near = np.abs(np.abs(p - np.floor(p)) - 0.5) <= tol
        shape = [1] * nd
        shape[w] = -1
        bad |= near.reshape(shape)
    return bad


def unclamped(g):
    """bool (size): voxels of the resampled box whose way back reads inside the resampled grid, through samples whose own
    positions were inside the box — the voxels a round trip of a linear field reproduces"""
    nd = g["nd"]
    keep = np.ones(g["size"], dtype=bool)
    for w in range(nd):
        n, m = g["n_or"][w], g["res"][w]
        back = np.arange(n) * (g["zoom"][w] / g["pix"][w])
        ok = back <= m - 1
        upper = np.minimum(np.floor(back).astype(np.int64) + 1, m - 1)       # the further of the two samples it reads
        ok &= upper * (g["pix"][w] / g["zoom"][w]) <= n - 1
        if g["flip"][w]:
            ok = ok[::-1]
        shape = [1] * nd
        shape[g["perm"][w]] = -1
        keep &= ok.reshape(shape)
    return keep


def sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


def inverse(logits, g, use_sigmoid=True):
    """logits: list of (C, *out) arrays (any float dtype, values taken as they are) -> float64 (C, *orig): the ensemble mean,
    the sigmoid, the bilinear resampling back, un-mirror, un-permute, paste"""
    nd = g["nd"]
    v = sum(l.astype(np.float64) for l in logits) / len(logits)
    if use_sigmoid:
        v = sigmoid(v)
    v = v[(slice(None),) + tuple(slice(b, b + n) for b, n in zip(g["pad"], g["res"]))]
    tabs = [table(g["n_or"][w], g["zoom"][w] / g["pix"][w], g["res"][w]) for w in range(nd)]
    v = _interp(v, tabs)
    mirrored = [1 + w for w in range(nd) if g["flip"][w]]
    if mirrored:
        v = np.flip(v, mirrored)
    v = np.transpose(v, [0] + [1 + g["perm"].index(i) for i in range(nd)])
    out = np.zeros((v.shape[0],) + tuple(g["orig"]))
    lo = [max(s, 0) for s in g["start"]]
    hi = [min(s + n, m) for s, n, m in zip(g["start"], g["size"], g["orig"])]
    out[(slice(None),) + tuple(slice(a, b) for a, b in zip(lo, hi))] = \
        v[(slice(None),) + tuple(slice(a - s, b - s) for a, b, s in zip(lo, hi, g["start"]))]
    return out


# ---- the shapes of the value tests (CPU and GPU) ---------------------------------------------------------------------------
# name: (C, size), code of the file's axes, zooms, pixdim, rotation in degrees, roi, (box_start, orig_size) or None
CASES = {
    "shrink_identity": ((2, (9, 14, 11)), "RAS", (1, 1, 1), 2, 0, None, None),
    "grow_transposed_mirror": ((2, (9, 14, 11)), "ALS", (3, 3, 3), 2, 0, (8, 18, 8), None),      # roi larger on one axis, odd pad
    "mixed_cyclic_two_mirrors": ((1, (16, 12, 20)), "PIR", (0.9, 1.2, 5.0), 2, 15, (56, 12, 12), None),
    "grow_reversed_three_mirrors": ((1, (16, 12, 20)), "IPL", (3, 3, 3), 2, 0, None, None),
    "border_clamp": ((1, (10, 6, 10)), "RAS", (1, 1, 1), 2, 0, None, None),
    "half_ties": ((1, (9, 8, 11)), "RAS", (4, 4, 1), 2, 0, (20, 16, 8), None),                   # scale 0.5: exact ties
    "unit_axis": ((2, (6, 1, 9)), "LAS", (1.2, 5.0, 0.9), 2, 0, None, None),
    "boxed": ((2, (9, 14, 11)), "PIR", (0.9, 1.2, 5.0), 2, 10, (30, 8, 8), ((2, 3, 1), (12, 20, 15))),
    # rows that read a strided axis, with more than one 16 x 16 tile of lanes along the row and along the other axis
    "tiles_middle_axis": ((1, (5, 40, 70)), "RSA", (1.0, 3.0, 2.2), 2, 0, (3, 77, 72), None),
    "tiles_slow_axis": ((1, (40, 6, 70)), "IPL", (3.0, 1.0, 2.2), 2, 0, None, None),
    "2d": ((3, (13, 18)), "AL", (3, 0.9), 2, 5, (10, 20), None),
    "1d": ((2, (17,)), "L", (3,), 2, 0, (30,), None),
}


def make_case(name, seed=3):
    """(x float32 (C, *size), label uint8 (2, *size), affine, dict of keywords for geometry())"""
    (C, size), code, zooms, pix, deg, roi, box = CASES[name]
    rng = np.random.default_rng(seed + len(name))
    x = rng.standard_normal((C,) + size).astype(np.float32) * 3.0
    lab = rng.integers(0, 4, (2,) + size).astype(np.uint8)
    kw = dict(pixdim=pix, roi=roi)
    if box is not None:
        kw.update(box_start=box[0], orig_size=box[1])
    return x, lab, make_affine(code, zooms, deg), kw


def make_logits(C, out, K, seed=11):
    """K float32 arrays (C, *out) drawn as 4·N(0, 1)"""
    rng = np.random.default_rng(seed)
    return [(4.0 * rng.standard_normal((C,) + tuple(out))).astype(np.float32) for _ in range(K)]
