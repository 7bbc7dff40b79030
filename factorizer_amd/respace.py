"""Resampling of a volume to the recipe's voxel spacing, and of a prediction back onto the file's grid: the two transforms of
the bundles' chains that `volume.py` leaves out, on device.

What the recipe runs (model_zoo/factorizer_isles22/configs; deconver_isles22 has the same chain):

* ``deterministic_transforms`` (train.yaml:90-113): ``CropForegroundd`` → ``Orientationd(axcodes="RAS")`` →
  ``NormalizeIntensityd`` → ``Spacingd(pixdim=pix_size, mode=[bilinear, nearest], align_corners=True)`` → ``SpatialPadd``,
  with ``pix_size: [2.0, 2.0, 2.0]`` (train.yaml:36) on files of mixed, often anisotropic spacing and mixed axis order;
* ``postprocessing`` (inference.yaml:103-121): ``MeanEnsembled`` → ``Activationsd(sigmoid)`` →
  ``Invertd(nearest_interp=false)``, which resamples the **probabilities** back to the file's grid bilinearly, → and only then
  ``AsDiscreted(threshold)``.

MONAI and nibabel are third-party and absent here, so their semantics are **restated**, not pinned against them.  With the
image ``(C, *S)`` of 1 to 3 spatial axes and ``A`` the ``(nd+1)×(nd+1)`` voxel-index → world affine of its grid (host geometry
is float64 throughout, never fp32):

* **Crop.**  A box that starts at ``start`` has the affine ``A`` with the translation ``A·[start; 1]``.
* **Orientation to ``axcodes``** (nibabel's ``io_orientation``).  The direction matrix ``A[:nd, :nd]`` with its columns
  normalised (a zero column counts as length 1) is replaced by its closest orthogonal matrix ``R`` — the polar factor
  ``P·Qᵀ`` of its SVD, singular values at or below ``S.max()·nd·eps`` dropped.  For source axes 0, 1, 2 in this order the
  world axis with the largest ``|R|`` entry of that column among those not yet taken is the axis' direction, the sign of the
  entry its sense (letters ``L/R``, ``P/A``, ``I/S``; the second is the positive sense).  The result is a signed permutation:
  output axis ``w`` reads source axis ``π(w)``, mirrored or not; the output affine has column ``w`` = ± column ``π(w)`` of
  ``A``, and each mirrored axis adds ``column π(w)·(n_π(w) − 1)`` to the translation.
* **Spacing to ``pixdim``** on the oriented grid with affine ``A'``: ``zoom_a`` is the length of column ``a`` of ``A'``,
  ``n_out_a = round_half_even((n_a − 1)·zoom_a / pixdim_a + 1)``, and the output affine has column ``a`` scaled by
  ``pixdim_a / zoom_a`` and ``A'``'s translation.  In voxel space that is a scaling per axis, also for oblique affines: output
  index ``o_a`` reads the oriented position ``p_a = o_a·(pixdim_a / zoom_a)``.
* **Sampling** (``align_corners=True``, ``padding_mode="border"``): ``p`` is clamped to ``[0, n − 1]``; ``bilinear`` takes
  ``i0 = floor(p)``, ``i1 = min(i0 + 1, n − 1)`` and the weight ``p − i0`` rounded to fp32, and lerps as
  ``fma(f, v1 − v0, v0)`` in fp32 along the contiguous axis of the sampled grid first, then the middle, then the slow one;
  ``nearest`` takes ``round_half_even(p)``.  Positions are float64 on every path.
* **Pad.**  ``SpatialPad(roi)`` as in `prepare_volume`: symmetric, constant 0, ``w // 2`` voxels in front.
* **Inverse** (``Invertd``, ``nearest_interp=False``): the pad is stripped; the spaced grid is resampled onto the oriented
  grid of its pre-spacing size at ``p_a = q_a·(zoom_a / pixdim_a)``, bilinear, border; the axes are un-mirrored and
  un-permuted; the box is pasted into zeros of the file's size.

Crop ∘ orient ∘ space ∘ pad is a **monomial** map — each output axis reads one source axis at ``p = s·o + t`` — and so is its
inverse; `ResampleGeometry` carries it and one gather per direction does all of it (csrc/respace.hip).

**Two differences from MONAI**, both on purpose: positions are formed in float64 (``grid_sample`` builds an fp32 grid, which
moves samples by up to ``n·2⁻²⁴`` voxels and decides ties of the nearest mode by rounding noise), and a composite map whose
scales are all 1 is a copy, bit-identical to indexing (the interpolation there would turn an infinite neighbour into NaN).

Device tensors of the native kinds (image fp32 in, fp32 / bf16 out; labels uint8; logits fp32 / bf16) run the kernels; CPU
tensors run composed framework ops — index arithmetic from float64 positions, no ``grid_sample`` — silently; device tensors of
other kinds, with more than 65535 planes or a plane of 2^30 voxels or more run them too and say why, once per reason.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from . import _native as N
from . import composed
from . import functional as Fn
from .volume import MAX_CHANNELS, MAX_PLANE, MAX_SETS, _pad, _per_axis, _voxels, prepare_volume

F64 = torch.float64
_LETTERS = {"L": (0, -1), "R": (0, 1), "P": (1, -1), "A": (1, 1), "I": (2, -1), "S": (2, 1)}
_CODES = (("L", "R"), ("P", "A"), ("I", "S"))


@dataclass
class ResampleGeometry:
    """The monomial map of crop → orient → space → pad and what its inverse needs.  Index ``o`` of resampled axis ``w`` (in
    front of the pad) reads position ``scale[w]·o + offset[w]`` of axis ``src_axis[w]`` of the grid that is resampled — the
    crop box, ``src_size``, which starts at ``box_start`` of the file's grid ``orig_size``; a negative scale is a mirrored
    axis.  On the way back oriented index ``i`` reads resampled position ``inv_scale[w]·i``."""
    src_axis: tuple
    scale: tuple                   # float, signed: ± pixdim / zoom
    offset: tuple                  # float: n − 1 on a mirrored axis, else 0
    inv_scale: tuple               # float, positive: zoom / pixdim
    src_size: tuple
    res_size: tuple                # the resampled grid, n_out
    pad_before: tuple
    out_size: tuple                # the padded grid
    dst_affine: torch.Tensor       # (nd+1, nd+1) float64: the affine of the unpadded resampled grid
    orig_size: tuple
    box_start: tuple

    @property
    def flip(self):
        return tuple(s < 0 for s in self.scale)

    def native(self):
        return Fn.respace_geom(self.src_size, self.src_axis, [int(f) for f in self.flip], [abs(s) for s in self.scale],
                               self.inv_scale, self.res_size, self.pad_before, self.out_size, self.orig_size, self.box_start)


@dataclass
class SpacedVolume:
    """What `prepare_spaced_volume` returns: the network input, the fields of `PreparedVolume`, and the geometry
    `restore_spaced_prediction` inverts."""
    image: torch.Tensor            # (1, C, *P)
    label: torch.Tensor | None     # (1, K, *P) uint8
    box_start: tuple
    box_end: tuple
    pad_before: tuple              # zero voxels in front of the resampled box in `image`
    orig_size: tuple
    mean: torch.Tensor
    std: torch.Tensor
    geometry: ResampleGeometry


# ---- host geometry (float64) -------------------------------------------------------------------------------------------------
def _affine(affine, nd):
    A = torch.as_tensor(affine).detach().to("cpu", F64)
    if A.dim() != 2 or A.shape[0] != A.shape[1] or not 2 <= A.shape[0] <= 4:
        raise ValueError(f"an affine is (nd+1, nd+1) with 1 to 3 spatial axes, got {tuple(A.shape)}")
    if nd is not None and A.shape[0] != nd + 1:
        raise ValueError(f"{nd} spatial axes need a ({nd + 1}, {nd + 1}) affine, got {tuple(A.shape)}")
    if not bool(torch.isfinite(A).all()):
        raise ValueError("the affine holds a value that is not finite")
    return A


def _io_orientation(A):
    """per source axis (world axis, sense ±1) of the grid with affine A"""
    nd = A.shape[0] - 1
    rzs = A[:nd, :nd]
    zooms = rzs.pow(2).sum(0).sqrt()
    zooms = torch.where(zooms == 0, torch.ones_like(zooms), zooms)
    P, S, Qt = torch.linalg.svd(rzs / zooms)
    keep = S > S.max() * nd * torch.finfo(F64).eps
    R = P[:, keep] @ Qt[keep]
    taken, ornt = [], []
    for i in range(nd):
        col = R[:, i].abs().clone()
        col[taken] = -1.0
        w = int(col.argmax())
        taken.append(w)
        ornt.append((w, -1 if float(R[w, i]) < 0 else 1))
    return ornt


def _parse_axcodes(axcodes, nd):
    codes = [str(c).upper() for c in axcodes][:nd]      # a code longer than the grid has axes names its first nd axes
    if len(codes) != nd or any(c not in _LETTERS for c in codes):
        raise ValueError(f"axcodes needs {nd} letters out of L/R, P/A, I/S, got {axcodes!r}")
    ornt = [_LETTERS[c] for c in codes]
    if sorted(w for w, _ in ornt) != list(range(nd)):
        raise ValueError(f"axcodes {axcodes!r} must name each of the first {nd} world axes once")
    return ornt


def orientation_of(affine, nd=None) -> str:
    """The axis codes of a grid: one letter per voxel axis saying towards which world direction it grows (``"RAS"``: right,
    anterior, superior), by the rule restated in the module docstring."""
    A = _affine(affine, nd)
    return "".join(_CODES[w][s > 0] for w, s in _io_orientation(A))


def _floats(v, nd, what):
    v = (float(v),) * nd if isinstance(v, (int, float)) else tuple(float(a) for a in v)
    if len(v) != nd:
        raise ValueError(f"{what} needs one value per spatial axis ({nd}), got {v}")
    return v


def spacing_geometry(size, affine, pixdim, *, axcodes="RAS", box_start=None, roi_size=None,
                     orig_size=None) -> ResampleGeometry:
    """The geometry of ``Orientation(axcodes)`` → ``Spacing(pixdim)`` → ``SpatialPad(roi_size)`` of the grid ``size`` (1 to 3
    axes) that starts at ``box_start`` (default: the origin) of the file's grid ``orig_size`` (default: ``box_start + size``)
    with the voxel → world ``affine``.  ``axcodes=None`` skips the reorientation, ``pixdim=None`` the spacing, ``roi_size=None``
    the pad.  Host only, float64 throughout."""
    size = tuple(int(n) for n in size)
    nd = len(size)
    if not 1 <= nd <= 3 or any(n < 1 for n in size):
        raise ValueError(f"size needs 1 to 3 positive extents, got {size}")
    A = _affine(affine, nd)
    start = (0,) * nd if box_start is None else _per_axis(box_start, nd, "box_start")
    orig = tuple(s + n for s, n in zip(start, size)) if orig_size is None else _per_axis(orig_size, nd, "orig_size")
    if any(n < 1 for n in orig):
        raise ValueError(f"orig_size must be positive, got {orig}")
    M, t = A[:nd, :nd], A[:nd, nd] + A[:nd, :nd] @ torch.tensor(start, dtype=F64)
    # orientation: output axis w reads source axis perm[w], mirrored where the senses differ
    if axcodes is None:
        perm, flip = list(range(nd)), [False] * nd
    else:
        src, dst = _io_orientation(A), _parse_axcodes(axcodes, nd)
        where = {w: (i, s) for i, (w, s) in enumerate(src)}
        perm = [where[w][0] for w, _ in dst]
        flip = [where[w][1] != s for w, s in dst]
    n_or = [size[a] for a in perm]
    cols = []
    for w in range(nd):
        col = M[:, perm[w]]
        if flip[w]:
            t = t + col * (n_or[w] - 1)
            col = -col
        cols.append(col)
    # spacing
    if pixdim is None:
        ratio, inv, res = [1.0] * nd, [1.0] * nd, list(n_or)
    else:
        pix = _floats(pixdim, nd, "pixdim")
        if any(not (p > 0.0) or p == float("inf") for p in pix):
            raise ValueError(f"pixdim must be positive and finite, got {pix}")
        zoom = [float(c.pow(2).sum().sqrt()) for c in cols]
        if any(z == 0.0 for z in zoom):
            raise ValueError("the affine has an axis of zero length: its spacing is undefined")
        ratio = [p / z for p, z in zip(pix, zoom)]
        inv = [z / p for p, z in zip(pix, zoom)]
        res = [max(1, round((n - 1) * z / p + 1)) for n, z, p in zip(n_or, zoom, pix)]     # round(): half to even
    dst_affine = torch.eye(nd + 1, dtype=F64)
    for w in range(nd):
        dst_affine[:nd, w] = cols[w] * ratio[w]
    dst_affine[:nd, nd] = t
    roi = res if roi_size is None else _per_axis(roi_size, nd, "roi_size")
    out = tuple(max(n, r) for n, r in zip(res, roi))
    return ResampleGeometry(src_axis=tuple(perm), scale=tuple(-r if f else r for r, f in zip(ratio, flip)),
                            offset=tuple(float(n - 1) if f else 0.0 for n, f in zip(n_or, flip)), inv_scale=tuple(inv),
                            src_size=size, res_size=tuple(res), pad_before=tuple((o - n) // 2 for o, n in zip(out, res)),
                            out_size=out, dst_affine=dst_affine, orig_size=orig, box_start=start)


# ---- gate ----------------------------------------------------------------------------------------------------------------------
def _gate(what, on_device, kinds_ok, dtypes, planes, voxels):
    """True when the call runs the kernels (`volume._native_gate` for this module's kinds)"""
    if not on_device:
        return False
    if not kinds_ok:
        names = ", ".join(str(d) for d in dtypes)
        key, why = names.replace(" ", ""), f"{names} is outside the native kernel set (image fp32 in, fp32 / bf16 out; " \
            "labels uint8; logits fp32 / bf16)"
    elif planes > MAX_CHANNELS:
        key, why = "channels", f"{planes} planes, the kernels take up to {MAX_CHANNELS}"
    elif max(voxels) >= MAX_PLANE:
        key, why = "plane", f"a plane of {max(voxels)} voxels, the kernels take fewer than 2^30"
    else:
        return True
    composed.warn_once(f"respace:{what}:{key}", f"{what}: {why}: composed framework ops")
    return False


# ---- composed pieces -----------------------------------------------------------------------------------------------------------
def _taps(count, scale, n, nearest, device):
    """indices (and the fp32 weight of the second) that positions ``scale·o``, o < count, read on an axis of extent n"""
    p = (torch.arange(count, dtype=F64) * scale).clamp(max=float(n - 1))
    if nearest:
        return torch.round(p).to(torch.int64).to(device), None, None          # torch.round: half to even
    i0 = p.floor()
    f = (p - i0).to(torch.float32)
    i0 = i0.to(torch.int64)
    return i0.to(device), (i0 + 1).clamp(max=n - 1).to(device), f.to(device)


def _sample_axis(x, dim, i0, i1, f):
    v0 = x.index_select(dim, i0)
    if i1 is None:
        return v0
    shape = [1] * x.dim()
    shape[dim] = -1
    return torch.addcmul(v0, f.view(shape), x.index_select(dim, i1) - v0)


def _resample_composed(x, g, nearest):
    """x (C, *src_size) -> (C, *res_size): the oriented view sampled axis by axis, the contiguous axis first"""
    nd = len(g.src_size)
    x = x.permute(0, *(1 + a for a in g.src_axis))
    for w in reversed(range(nd)):
        n = g.src_size[g.src_axis[w]]
        i0, i1, f = _taps(g.res_size[w], abs(g.scale[w]), n, nearest, x.device)
        if g.scale[w] < 0:
            i0, i1 = n - 1 - i0, None if i1 is None else n - 1 - i1
        x = _sample_axis(x, 1 + w, i0, i1, f)
    return x


def _unspace_composed(ls, g, sigmoid, threshold):
    x0 = ls[0]
    nd = len(g.src_size)
    acc = torch.zeros(x0.shape[1:], dtype=torch.float32, device=x0.device)
    for t in ls:
        acc = acc + t[0].to(torch.float32)
    v = acc * torch.tensor(1.0 / len(ls), dtype=torch.float32, device=x0.device)
    if sigmoid:
        v = torch.sigmoid(v)
    v = v[(slice(None),) + tuple(slice(b, b + n) for b, n in zip(g.pad_before, g.res_size))]      # the pad stripped
    for w in reversed(range(nd)):
        i0, i1, f = _taps(g.src_size[g.src_axis[w]], g.inv_scale[w], g.res_size[w], False, v.device)
        v = _sample_axis(v, 1 + w, i0, i1, f)
    mirrored = [1 + w for w in range(nd) if g.scale[w] < 0]
    if mirrored:
        v = v.flip(mirrored)
    v = v.permute(0, *(1 + g.src_axis.index(a) for a in range(nd)))                               # back in source axis order
    out = torch.zeros((v.shape[0],) + g.orig_size, dtype=torch.float32, device=v.device)
    lo = [max(s, 0) for s in g.box_start]
    hi = [min(s + n, m) for s, n, m in zip(g.box_start, g.src_size, g.orig_size)]
    if all(b > a for a, b in zip(lo, hi)):
        out[(slice(None),) + tuple(slice(a, b) for a, b in zip(lo, hi))] = \
            v[(slice(None),) + tuple(slice(a - s, b - s) for a, b, s in zip(lo, hi, g.box_start))]
    if threshold is None:
        return out
    return (out >= torch.tensor(threshold, dtype=torch.float32, device=out.device)).to(torch.uint8)


# ---- public ------------------------------------------------------------------------------------------------------------------------
_MODES = {"bilinear": N.RESPACE_BILINEAR, "nearest": N.RESPACE_NEAREST}


def resample_volume(image, geometry: ResampleGeometry, *, label=None, mode: str = "bilinear", out_dtype=None):
    """``Orientation`` → ``Spacing`` → ``SpatialPad`` of ``image`` (C, *S) fp32 through ``geometry`` (`spacing_geometry` of the
    same S), ``bilinear`` or ``nearest``; ``label`` (K, *S) uint8 goes through the same map, always nearest.  Returns
    ``(image_out, label_out)``: (C, *P) in ``out_dtype`` (fp32 by default; bf16 is rounded to nearest even from the fp32
    value) and (K, *P) uint8 or None.  Pad voxels are 0.  A map whose scales are all 1 is a copy, bit-identical to indexing."""
    g = geometry
    nd = len(g.src_size)
    if mode not in _MODES:
        raise ValueError(f"mode is 'bilinear' or 'nearest', got {mode!r}")
    if image.dim() != nd + 1 or tuple(image.shape[1:]) != g.src_size or image.shape[0] < 1:
        raise ValueError(f"the geometry resamples (C, *{g.src_size}), got {tuple(image.shape)}")
    if not image.dtype.is_floating_point:
        raise ValueError(f"the resampler takes a floating-point image (the chain normalises first), got {image.dtype}")
    if label is not None:
        if label.dim() != nd + 1 or tuple(label.shape[1:]) != g.src_size:
            raise ValueError(f"a channel-first label is (K, *S) with S = {g.src_size}, got {tuple(label.shape)}")
        if label.dtype != torch.uint8:
            raise ValueError(f"a channel-first label is uint8, got {label.dtype}")
        if label.device != image.device:
            raise ValueError("image and label live on different devices")
    out_dtype = out_dtype or torch.float32
    nearest = mode == "nearest" or all(abs(s) == 1.0 for s in g.scale)    # unit scales: every position is an index
    K = 0 if label is None else label.shape[0]
    kinds_ok = image.dtype == torch.float32 and out_dtype in (torch.float32, torch.bfloat16)
    if _gate("resample_volume", image.is_cuda, kinds_ok, [image.dtype, out_dtype], image.shape[0] + K,
             [_voxels(g.src_size), _voxels(g.out_size)]):
        return Fn.vol_respace(image.contiguous(), None if label is None else label.contiguous(), g.native(),
                              N.RESPACE_NEAREST if nearest else N.RESPACE_BILINEAR, out_dtype)
    img = _pad(_resample_composed(image.to(torch.float32), g, nearest), g.pad_before, g.out_size).to(out_dtype)
    lab = None if label is None else _pad(_resample_composed(label, g, True), g.pad_before, g.out_size)
    return img.contiguous(), None if lab is None else lab.contiguous()


def prepare_spaced_volume(image, affine, label=None, *, pixdim, axcodes="RAS", margin=10, roi_size=None,
                          nonzero: bool = True, channel_wise: bool = True, classes=None, out_dtype=None) -> SpacedVolume:
    """The ISLES recipe's ``deterministic_transforms`` in their order: `prepare_volume` without a pad (foreground box with
    ``margin``, crop, `normalize_intensity`, class encoding) → `spacing_geometry` of the box (``Orientation(axcodes)`` →
    ``Spacing(pixdim)`` → ``SpatialPad(roi_size)``) → `resample_volume`, the image bilinear, the label nearest.  The recipe
    normalises behind the reorientation and here it runs in front of it: the same statistic over the same elements, in another
    float64 summation order.  ``affine`` is the file's voxel → world matrix; the other arguments are `prepare_volume`'s.
    Returns a `SpacedVolume`: the tensors with a leading batch axis, `PreparedVolume`'s fields (``pad_before`` is the pad of the
    resampled grid) and the geometry for `restore_spaced_prediction`."""
    p = prepare_volume(image, label, margin=margin, roi_size=None, nonzero=nonzero, channel_wise=channel_wise, classes=classes)
    bsize = tuple(e - s for s, e in zip(p.box_start, p.box_end))
    g = spacing_geometry(bsize, affine, pixdim, axcodes=axcodes, box_start=p.box_start, roi_size=roi_size,
                         orig_size=p.orig_size)
    img, lab = resample_volume(p.image[0], g, label=None if p.label is None else p.label[0], out_dtype=out_dtype)
    return SpacedVolume(image=img[None], label=None if lab is None else lab[None], box_start=p.box_start, box_end=p.box_end,
                        pad_before=g.pad_before, orig_size=p.orig_size, mean=p.mean, std=p.std, geometry=g)


def restore_spaced_prediction(logits, geometry, *, sigmoid: bool = True, threshold: float | None = 0.5):
    """The ISLES inference ``postprocessing``: ``logits`` is one (1, C, *P) tensor or a list of up to 8 (one per fold model),
    fp32 or bf16, on the padded resampled grid of ``geometry`` (a `ResampleGeometry` or a `SpacedVolume`).  Per voxel of that
    grid the ensemble value is the fp32 mean (the sum in list order times ``1 / K``), through the sigmoid unless
    ``sigmoid=False``; the **values** are interpolated bilinearly through the inverse map onto the file's grid and only then
    compared: returns ``value >= threshold`` as uint8 (C, *orig_size), zeros outside the crop box, or with ``threshold=None``
    the fp32 values themselves (``Invertd``'s output in front of ``AsDiscreted``)."""
    g = geometry.geometry if isinstance(geometry, SpacedVolume) else geometry
    ls = [logits] if torch.is_tensor(logits) else list(logits)
    if not 1 <= len(ls) <= MAX_SETS:
        raise ValueError(f"restore_spaced_prediction takes 1 to {MAX_SETS} logit tensors, got {len(ls)}")
    nd = len(g.src_size)
    x0 = ls[0]
    if x0.dim() != nd + 2 or x0.shape[0] != 1 or tuple(x0.shape[2:]) != g.out_size or x0.shape[1] < 1:
        raise ValueError(f"logits are (1, C, *{g.out_size}), got {tuple(x0.shape)}")
    for t in ls:
        if t.shape != x0.shape or t.dtype != x0.dtype or t.device != x0.device:
            raise ValueError("all logit tensors share one shape, dtype and device")
    if threshold is not None:
        threshold = float(threshold)
        if threshold != threshold:
            raise ValueError("threshold is NaN")
    C = x0.shape[1]
    if _gate("restore_spaced_prediction", x0.is_cuda, x0.dtype in (torch.float32, torch.bfloat16), [x0.dtype], C,
             [_voxels(g.orig_size), _voxels(g.out_size)]):
        return Fn.vol_unspace([t[0].contiguous() for t in ls], g.native(), sigmoid, threshold)
    return _unspace_composed(ls, g, sigmoid, threshold)
