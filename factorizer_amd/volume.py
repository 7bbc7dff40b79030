"""Volume preparation in front of the network and prediction restore behind it: the `deterministic_transforms` and the
inference `postprocessing` of the bundles, on device.

What the recipe runs (model_zoo/factorizer_brats23/configs; factorizer_isles22 has the same chain without the encoder):

* ``deterministic_transforms`` (train.yaml:86-116, inference.yaml:57-83) on the raw volume:
  ``BraTSOneHotEncoderd`` (train.yaml:91-92; a per-voxel map, so it commutes with the crop and runs here in the write pass)
  → ``CropForegroundd(source_key="image", margin=10)`` (train.yaml:93-96, inference.yaml:64-67) →
  ``NormalizeIntensityd(nonzero=True, channel_wise=True)`` (train.yaml:100-103, inference.yaml:71-74) →
  ``SpatialPadd(spatial_size=roi)`` (train.yaml:113-116; not in inference.yaml);
* ``postprocessing`` (inference.yaml:104-125) on the stitched logits: ``MeanEnsembled`` over the fold checkpoints
  (inference.yaml:107-109) → ``Activationsd(sigmoid=True)`` (110-112) → ``Invertd`` (113-119; undoes the crop) →
  ``AsDiscreted(threshold=0.5)`` (120-122) → the BraTS label-map lambda (inference.yaml:123-125).

``Orientationd`` and ``Spacingd`` (train.yaml:97-99, 104-108) need the file's affine and are not part of this module: the BraTS
bundles run them at 1 mm on 1 mm RAS data, where they are the identity; the ISLES22 bundles resample to 2 mm from files of
mixed spacing and axis order, which is `respace.py` (`prepare_spaced_volume`, `restore_spaced_prediction`).

MONAI (pinned 1.4.0) is third-party and absent here, so its semantics are **restated**, not pinned against it:

* ``CropForeground``: a voxel is foreground iff any channel is ``> 0``; per axis ``start = first − margin``,
  ``end = last + 1 + margin``; ``allow_smaller=True`` (the 1.4 default) clips the box to the image, ``False`` lets it reach
  outside, where the crop reads zeros.  **Difference:** for an image without a foreground voxel MONAI returns an empty box
  that nothing downstream can consume; here the box is the whole image.
* ``NormalizeIntensity``: per channel (``channel_wise``) or over the tensor, mean and population standard deviation
  (``unbiased=False``) over the selected elements — ``!= 0`` with ``nonzero``, else all; the selected elements become
  ``(x − mean) / std``, the others stay; ``std == 0`` divides by 1; nothing selected: unchanged.  The statistics are formed in
  float64 and rounded once to fp32; the elementwise arithmetic is fp32 with an IEEE division.
* ``BraTSOneHotEncoder``: channel k = 1 where the class id is in set k; `BRATS_CLASSES` ``((3,), (1, 3), (1, 2, 3))`` are
  the bundle's three channels (enhancing tumour, tumour core, whole tumour).
* ``SpatialPad(method="symmetric", mode="constant")``: per axis ``w = max(roi − size, 0)``, ``w // 2`` zero voxels in front,
  the rest behind.
* ``MeanEnsemble`` + ``Activations(sigmoid)`` + ``AsDiscrete(threshold)``: the fp32 mean of the K logit tensors (sum in list
  order times ``1 / K``) is foreground iff it is ``>= log(t / (1 − t))`` — the bound of `metrics._bound`, decided on the logit
  (``MeanEnsembled`` runs in front of ``Activationsd`` in the recipe as well: the mean is taken over logits).
* ``Invertd``: the pad is stripped and the box pasted into zeros of the original size; box parts outside the image are dropped.
* label map: the first channel, in channel order, that is foreground writes its value; `BRATS_LABEL_VALUES` ``(3, 1, 2)``
  over the channels (ET, TC, WT) reproduces the lambda's nesting.

Device tensors of the native kinds (image fp32 / int16 in, fp32 / bf16 out; labels uint8 / int16; logits fp32 / bf16) run
the kernels of csrc/volprep.hip; CPU tensors run composed framework ops; device tensors of other kinds,
with more than 65535 channels, with a plane of 2^30 voxels or more, or a label map over more than 8 channels do too and say
why once (`_native_gate`).
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from . import _native as N
from . import composed
from . import functional as Fn
from .metrics import _bound

BRATS_CLASSES = ((3,), (1, 3), (1, 2, 3))
BRATS_LABEL_VALUES = (3, 1, 2)
MAX_SETS = 8       # class sets of prepare_volume, logit tensors of restore_prediction
MAX_CLASS_ID = 31  # the sets travel as 32-bit membership masks


@dataclass
class PreparedVolume:
    """What `prepare_volume` returns: the network input and the geometry `restore_prediction` inverts."""
    image: torch.Tensor            # (1, C, *P)
    label: torch.Tensor | None     # (1, K, *P) uint8
    box_start: tuple               # the crop box in the original image, may reach outside it (allow_smaller=False)
    box_end: tuple
    pad_before: tuple              # zero voxels in front of the box in `image`
    orig_size: tuple
    mean: torch.Tensor             # (C,) fp32
    std: torch.Tensor              # (C,) fp32: the divisor (1 where the deviation is 0 or nothing was selected)


def _per_axis(v, nd, what):
    if isinstance(v, int):
        return (v,) * nd
    v = tuple(int(a) for a in v)
    if len(v) != nd:
        raise ValueError(f"{what} needs one value per spatial axis ({nd}), got {v}")
    return v


def _check_image(image):
    if image.dim() < 2 or image.dim() > 4:
        raise ValueError(f"expected a channel-first image (C, *S) with 1, 2 or 3 spatial axes, got {tuple(image.shape)}")
    if image.numel() == 0:
        raise ValueError("empty image")


MAX_CHANNELS = 65535   # planes of one launch grid
MAX_PLANE = 1 << 30    # voxels per plane the native gate lets through (the entry points index planes with 31 bits)


def _native_gate(what, on_device, kinds_ok, dtypes, channels, planes, other=None):
    """True when the call runs the kernels.  CPU tensors are composed silently; a device call outside the native set — element
    kinds, more than MAX_CHANNELS channels, a plane of MAX_PLANE voxels or more, or `other` (a reason in words) — is composed
    too and says why, once per reason."""
    if not on_device:
        return False
    names = ", ".join(str(d) for d in dtypes)
    if not kinds_ok:
        key, why = names.replace(" ", ""), f"{names} is outside the native kernel set (image fp32 / int16 in, fp32 / bf16 " \
            "out; labels uint8 / int16; logits fp32 / bf16)"
    elif channels > MAX_CHANNELS:
        key, why = "channels", f"{channels} channels, the kernels take up to {MAX_CHANNELS}"
    elif max(planes) >= MAX_PLANE:
        key, why = "plane", f"a plane of {max(planes)} voxels, the kernels take fewer than 2^30"
    elif other:
        key, why = "other", other
    else:
        return True
    composed.warn_once(f"volume:{what}:{key}", f"{what}: {why}: composed framework ops")
    return False


def _voxels(size):
    n = 1
    for v in size:
        n *= int(v)
    return n


# ---- bounding box ----------------------------------------------------------------------------------------------------------
def _first_last(image):
    """(first, last) foreground index per spatial axis, or None when no voxel is foreground"""
    nd = image.dim() - 1
    if _native_gate("foreground_bbox", image.is_cuda, Fn.vol_kind_ok(N.VOL_IMAGE_IN, image.dtype), [image.dtype],
                    image.shape[0], [_voxels(image.shape[1:])]):
        box = Fn.vol_bbox(image.contiguous()).tolist()   # the one host read: the output shape depends on it
        if box[5] < 0:
            return None
        return tuple(box[3 - nd:3]), tuple(box[6 - nd:6])
    return _first_last_composed(image)


def _first_last_composed(image):
    nd = image.dim() - 1
    fg = (image > 0).any(0)
    if not bool(fg.any()):
        return None
    first, last = [], []
    for ax in range(nd):
        idx = torch.nonzero(fg.any(tuple(a for a in range(nd) if a != ax)) if nd > 1 else fg).flatten()
        first.append(int(idx[0]))
        last.append(int(idx[-1]))
    return tuple(first), tuple(last)


def foreground_bbox(image, margin=0, allow_smaller: bool = True):
    """``CropForeground``'s box of a channel-first image (C, *S): (start, end) as tuples of Python ints, per axis
    ``first − margin`` and ``last + 1 + margin`` over the voxels where any channel is ``> 0``.  ``allow_smaller=True`` clips
    the box to the image; otherwise it may reach outside (the crop zero-fills there).  ``margin``: an int or one per axis.
    **An image with no foreground voxel gives the whole image** (start 0, end S) — MONAI returns an empty box there, which
    nothing downstream can consume."""
    _check_image(image)
    size = tuple(image.shape[1:])
    nd = len(size)
    m = _per_axis(margin, nd, "margin")
    fl = _first_last(image)
    if fl is None:
        return (0,) * nd, size
    start = tuple(f - a for f, a in zip(fl[0], m))
    end = tuple(l + 1 + a for l, a in zip(fl[1], m))
    if allow_smaller:
        start = tuple(max(s, 0) for s in start)
        end = tuple(min(e, n) for e, n in zip(end, size))
    return start, end


# ---- composed pieces ---------------------------------------------------------------------------------------------------------
def _crop(x, start, end):
    """x (C, *S) cut to the box [start, end), zeros where the box leaves the image"""
    size = tuple(x.shape[1:])
    lo = [max(s, 0) for s in start]
    hi = [min(e, n) for e, n in zip(end, size)]
    inner = x[(slice(None),) + tuple(slice(a, b) for a, b in zip(lo, hi))]
    if all(a == s for a, s in zip(lo, start)) and all(b == e for b, e in zip(hi, end)):
        return inner
    out = torch.zeros((x.shape[0],) + tuple(e - s for s, e in zip(start, end)), dtype=x.dtype, device=x.device)
    out[(slice(None),) + tuple(slice(a - s, b - s) for a, b, s in zip(lo, hi, start))] = inner
    return out


def _pad(x, before, out_size):
    """x (C, *B) placed `before` voxels into zeros (C, *out_size)"""
    if tuple(x.shape[1:]) == tuple(out_size):
        return x
    out = torch.zeros((x.shape[0],) + tuple(out_size), dtype=x.dtype, device=x.device)
    out[(slice(None),) + tuple(slice(b, b + n) for b, n in zip(before, x.shape[1:]))] = x
    return out


def _normalize_composed(x, nonzero, channel_wise):
    """(fp32 result, mean (C,), std (C,)) of x (C, *S): float64 statistics rounded once, fp32 elementwise arithmetic"""
    C = x.shape[0]
    x32 = x.to(torch.float32)
    sel = (x32 != 0) if nonzero else torch.ones_like(x32, dtype=torch.bool)
    x64 = x32.to(torch.float64)
    dims = tuple(range(1, x.dim())) if channel_wise else tuple(range(x.dim()))
    cnt = sel.sum(dims, keepdim=True).to(torch.float64)
    safe = cnt.clamp_min(1.0)
    mean = torch.where(sel, x64, torch.zeros_like(x64)).sum(dims, keepdim=True) / safe
    sq = torch.where(sel, (x64 - mean) ** 2, torch.zeros_like(x64)).sum(dims, keepdim=True)
    mean32 = torch.where(cnt > 0, mean, torch.zeros_like(mean)).to(torch.float32)
    std32 = torch.where(cnt > 0, (sq / safe).sqrt(), torch.ones_like(sq)).to(torch.float32)
    std32 = torch.where(std32 == 0, torch.ones_like(std32), std32)
    out = torch.where(sel, (x32 - mean32) / std32, x32)
    return out, mean32.reshape(-1).expand(C).contiguous(), std32.reshape(-1).expand(C).contiguous()


def _encode_composed(label, classes):
    """label (*S) integer class map -> (K, *S) uint8"""
    lab = label.to(torch.int64)
    planes = []
    for cs in classes:
        m = torch.zeros_like(lab, dtype=torch.bool)
        for v in cs:
            m |= lab == int(v)
        planes.append(m)
    return torch.stack(planes).to(torch.uint8)


def _prepare_composed(image, label, start, end, before, out_size, nonzero, channel_wise, classes, out_dtype):
    """crop -> normalise -> encode -> pad in framework ops: (image (C, *P), label (K, *P) or None, mean, std)"""
    x, mean, std = _normalize_composed(_crop(image, start, end), nonzero, channel_wise)
    img = _pad(x, before, out_size).to(out_dtype)
    lab = None
    if label is not None:
        lc = _crop(label[None] if classes is not None else label, start, end)
        lab = _pad(_encode_composed(lc[0], classes) if classes is not None else lc, before, out_size)
    return img, lab, mean, std


# ---- normalisation -----------------------------------------------------------------------------------------------------------
def _whole_geom(size):
    nd = len(size)
    return Fn.vol_geom(size, (0,) * nd, size, (0,) * nd, size)


def normalize_intensity(image, nonzero: bool = True, channel_wise: bool = True, batched: bool | None = None):
    """``NormalizeIntensity(nonzero, channel_wise)`` of (C, *S) or (B, C, *S), fp32 result: per channel (or per tensor — per
    sample of a batch) the mean and the population standard deviation over the elements ``!= 0`` (``nonzero``) or over all;
    those elements become ``(x − mean) / std``, zeros stay zeros.  ``std == 0`` divides by 1; a channel with no selected
    element is returned unchanged.  The statistics are accumulated in float64 and rounded once to fp32.  ``batched``: None
    takes a 5-D tensor as a batch and everything else as one channel-first image; pass True for a 1-D / 2-D batch."""
    if batched is None:
        batched = image.dim() == 5
    if batched:
        if image.dim() < 3:
            raise ValueError(f"a batch is (B, C, *S), got {tuple(image.shape)}")
        if image.shape[0] == 0:
            return image.to(torch.float32)
        return torch.stack([normalize_intensity(x, nonzero, channel_wise, False) for x in image])
    _check_image(image)
    if _native_gate("normalize_intensity", image.is_cuda, Fn.vol_kind_ok(N.VOL_IMAGE_IN, image.dtype), [image.dtype],
                    image.shape[0], [_voxels(image.shape[1:])]):
        return Fn.vol_prepare(image.contiguous(), None, _whole_geom(tuple(image.shape[1:])), nonzero, channel_wise, None,
                              torch.float32)[0]
    return _normalize_composed(image, nonzero, channel_wise)[0]


# ---- the chain -------------------------------------------------------------------------------------------------------------------
def _check_classes(classes):
    classes = tuple(tuple(int(v) for v in cs) for cs in classes)
    if not 1 <= len(classes) <= MAX_SETS:
        raise ValueError(f"classes needs 1 to {MAX_SETS} class-id sets, got {len(classes)}")
    for cs in classes:
        for v in cs:
            if not 0 <= v <= MAX_CLASS_ID:
                raise ValueError(f"class ids must lie in 0 .. {MAX_CLASS_ID}, got {v}")
    return classes


def prepare_volume(image, label=None, *, margin=10, roi_size=None, nonzero: bool = True, channel_wise: bool = True,
                   allow_smaller: bool = True, classes=None, out_dtype=None) -> PreparedVolume:
    """The recipe's ``deterministic_transforms`` in their order: `foreground_bbox` of ``image`` (C, *S) with ``margin`` → crop
    of image and label → `normalize_intensity` over the cropped box → class encoding of the label → symmetric constant pad to
    ``roi_size`` (per axis ``w = max(roi − size, 0)``, ``w // 2`` voxels in front, the rest behind; None: no pad, the
    inference recipe).  ``label``: with ``classes`` (1 to 8 sets of class ids below 32; `BRATS_CLASSES` is
    ``BraTSOneHotEncoder``) an integer class map (*S) or (1, *S), uint8 or int16 — output channel k is 1 where the label is in
    ``classes[k]``; with ``classes=None`` an already channel-first uint8 (K, *S), cropped and padded as it is.  Returns a
    `PreparedVolume`: ``image`` (1, C, *P) in ``out_dtype`` (fp32 by default; bf16 is rounded to nearest even from the fp32
    value), ``label`` (1, K, *P) uint8 or None, the geometry and the (C,) fp32 ``mean`` / ``std`` that were applied.
    ``Orientationd`` / ``Spacingd`` need the file's affine: the identity at the BraTS bundles' 1 mm, `prepare_spaced_volume`
    otherwise."""
    _check_image(image)
    size = tuple(image.shape[1:])
    nd = len(size)
    out_dtype = out_dtype or torch.float32
    if classes is not None:
        classes = _check_classes(classes)
    if label is not None:
        if classes is not None:
            if label.dim() == nd + 1 and label.shape[0] == 1:
                label = label[0]
            if tuple(label.shape) != size:
                raise ValueError(f"class map {tuple(label.shape)} does not match the image's spatial size {size}")
            if label.dtype not in (torch.uint8, torch.int16, torch.int32, torch.int64):
                raise ValueError(f"a class map is an integer tensor, got {label.dtype}")
        else:
            if label.dim() != nd + 1 or tuple(label.shape[1:]) != size:
                raise ValueError(f"a channel-first label is (K, *S) with S = {size}, got {tuple(label.shape)}")
            if label.dtype != torch.uint8:
                raise ValueError(f"a channel-first label is uint8, got {label.dtype}")
        if label.device != image.device:
            raise ValueError("image and label live on different devices")
    start, end = foreground_bbox(image, margin, allow_smaller)
    bsize = tuple(e - s for s, e in zip(start, end))
    roi = bsize if roi_size is None else _per_axis(roi_size, nd, "roi_size")
    out_size = tuple(max(b, r) for b, r in zip(bsize, roi))
    before = tuple((o - b) // 2 for o, b in zip(out_size, bsize))

    kinds = [image.dtype] + ([label.dtype] if label is not None else [])
    kinds_ok = Fn.vol_kind_ok(N.VOL_IMAGE_IN, image.dtype) and Fn.vol_kind_ok(N.VOL_IMAGE_OUT, out_dtype) \
        and (label is None or Fn.vol_kind_ok(N.VOL_LABEL_IN, label.dtype))
    planes = image.shape[0] + (0 if label is None else (len(classes) if classes is not None else label.shape[0]))
    if _native_gate("prepare_volume", image.is_cuda, kinds_ok, kinds + [out_dtype], planes,
                    [_voxels(size), _voxels(out_size)]):
        img, lab, mean, std = Fn.vol_prepare(image.contiguous(), None if label is None else label.contiguous(),
                                             Fn.vol_geom(size, start, end, before, out_size), nonzero, channel_wise, classes,
                                             out_dtype)
    else:
        img, lab, mean, std = _prepare_composed(image, label, start, end, before, out_size, nonzero, channel_wise, classes,
                                                out_dtype)
    return PreparedVolume(image=img[None], label=None if lab is None else lab[None], box_start=start, box_end=end,
                          pad_before=before, orig_size=size, mean=mean, std=std)


# ---- restore ---------------------------------------------------------------------------------------------------------------------
def _geometry_of(prepared):
    if isinstance(prepared, dict):
        get = prepared.__getitem__
    else:
        get = lambda k: getattr(prepared, k)   # noqa: E731
    return tuple(tuple(int(v) for v in get(k)) for k in ("box_start", "box_end", "pad_before", "orig_size"))


def restore_prediction(logits, prepared, *, sigmoid: bool = True, threshold: float = 0.5, label_values=None):
    """The inference ``postprocessing``: ``logits`` is one (1, C, *P) tensor or a list of up to 8 (one per fold model), fp32
    or bf16.  The ensemble value is their fp32 mean (the sum in list order times ``1 / K``); it is foreground iff
    ``sigmoid(mean) >= threshold``, decided on the logit with the bound of `metrics.discretize`.  The decision is inverted
    through ``prepared`` (a `PreparedVolume`, or a dict with ``box_start``, ``box_end``, ``pad_before``, ``orig_size``): the
    pad is stripped, the box pasted into zeros of ``orig_size``, box parts outside the image dropped.  Returns the uint8 mask
    (C, *orig_size), or with ``label_values`` (one value per channel) the uint8 label map (*orig_size) in which the first
    foreground channel in channel order writes its value and no foreground channel leaves 0 — `BRATS_LABEL_VALUES` gives
    the BraTS map."""
    ls = [logits] if torch.is_tensor(logits) else list(logits)
    if not 1 <= len(ls) <= MAX_SETS:
        raise ValueError(f"restore_prediction takes 1 to {MAX_SETS} logit tensors, got {len(ls)}")
    start, end, before, size = _geometry_of(prepared)
    nd = len(size)
    if nd < 1 or nd > 3 or not (len(start) == len(end) == len(before) == nd):
        raise ValueError("the geometry needs 1 to 3 spatial axes, the same number in every field")
    x0 = ls[0]
    if x0.dim() != nd + 2 or x0.shape[0] != 1:
        raise ValueError(f"logits are (1, C, *P) with {nd} spatial axes, got {tuple(x0.shape)}")
    for t in ls:
        if t.shape != x0.shape or t.dtype != x0.dtype or t.device != x0.device:
            raise ValueError("all logit tensors share one shape, dtype and device")
    C = x0.shape[1]
    P = tuple(x0.shape[2:])
    bsize = tuple(e - s for s, e in zip(start, end))
    for a in range(nd):
        if bsize[a] < 1 or before[a] < 0 or before[a] + bsize[a] > P[a] or start[a] >= size[a] or end[a] <= 0:
            raise ValueError(f"box [{start}, {end}) with pad {before} does not fit logits {P} / image {size}")
    if label_values is not None:
        label_values = tuple(int(v) for v in label_values)
        if len(label_values) != C or any(not 0 <= v <= 255 for v in label_values):
            raise ValueError(f"label_values needs one byte value per channel ({C}), got {label_values}")
    bound = _bound(sigmoid, threshold)
    many = None if label_values is None or C <= MAX_SETS else \
        f"a label map over {C} channels, the kernel takes up to {MAX_SETS}"
    if _native_gate("restore_prediction", x0.is_cuda, Fn.vol_kind_ok(N.VOL_LOGITS, x0.dtype), [x0.dtype], C,
                    [_voxels(size), _voxels(P)], many):
        return Fn.vol_restore([t[0].contiguous() for t in ls], Fn.vol_geom(size, start, end, before, P), bound, label_values)
    return _restore_composed(ls, start, end, before, size, bound, label_values)


def _restore_composed(ls, start, end, before, size, bound, label_values):
    x0 = ls[0]
    C = x0.shape[1]
    bsize = tuple(e - s for s, e in zip(start, end))
    acc = torch.zeros(x0.shape[1:], dtype=torch.float32, device=x0.device)
    for t in ls:
        acc = acc + t[0].to(torch.float32)
    fg = acc * torch.tensor(1.0 / len(ls), dtype=torch.float32, device=x0.device) >= bound
    fg = fg[(slice(None),) + tuple(slice(b, b + n) for b, n in zip(before, bsize))]      # the pad stripped
    lo = [max(s, 0) for s in start]
    hi = [min(e, n) for e, n in zip(end, size)]
    mask = torch.zeros((C,) + size, dtype=torch.bool, device=x0.device)
    mask[(slice(None),) + tuple(slice(a, b) for a, b in zip(lo, hi))] = \
        fg[(slice(None),) + tuple(slice(a - s, b - s) for a, b, s in zip(lo, hi, start))]
    if label_values is None:
        return mask.to(torch.uint8)
    out = torch.zeros(size, dtype=torch.uint8, device=x0.device)
    for c in reversed(range(C)):                                                          # channel 0 is written last: it wins
        out[mask[c]] = label_values[c]
    return out
