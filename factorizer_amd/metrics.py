"""Segmentation metrics of the training recipe: thresholded Dice and the percentile Hausdorff distance.

Every bundle's ``train.yaml`` reports the same two numbers (model_zoo/factorizer_brats23/configs/train.yaml):

* every training iteration ``Activationsd(sigmoid)`` → ``AsDiscreted(threshold=0.5)`` →
  ``MeanDice(include_background=True, ignore_empty=False)`` (train.yaml:215-243);
* every validation pass the same Dice per channel on the stitched sliding-window prediction — ``val_mean_dice`` selects the
  checkpoint — and ``MeanHausdorffDistance(percentile=95)`` (train.yaml:245-287).

MONAI (pinned 1.4.0, docs/requirements.txt:11) is third-party and absent here, so its semantics are **restated**, not pinned
against it:

* ``discretize``: foreground iff ``sigmoid(x) >= threshold``, decided on the logit: ``x >= log(t / (1 − t))``, the bound
  formed in float64 and rounded to fp32 (``t = 0.5``: ``x >= 0``, so a logit of exactly 0 is foreground, as in the
  composed form ``sigmoid(0) = 0.5 >= 0.5``);
* ``DiceMetric``: per (sample, channel) plane ``2 |P∧Y| / (|P| + |Y|)`` when the label plane is not empty; an empty label
  plane gives NaN with ``ignore_empty=True``, otherwise 1.0 when the prediction is empty too and 0.0 when it is not;
* ``get_mask_edges``: ``mask ^ binary_erosion(mask)`` with the cross structuring element and a zero border (MONAI's crop
  to the bounding box changes nothing: the border of the crop is background or the image border either way);
* ``HausdorffDistanceMetric``: the directed distance d(P→Y) is the ``percentile / 100`` quantile (linear interpolation;
  the maximum for ``percentile=None``) of the distances from every edge voxel of P to the nearest edge voxel of Y, in units
  of ``spacing``; NaN when P has no edge, +inf when only Y has none; the undirected value is the NaN-propagating maximum of
  the two directions (``torch.max``), so it is NaN whenever either edge set is empty;
* reductions (``do_metric_reduction``): NaN entries are left out of every mean; a mean over nothing is 0.0.

Mutually exclusive classes (``argmax=True``; the bundle chain ``AsDiscreted(pred, argmax=True, to_onehot=C)`` +
``AsDiscreted(label, to_onehot=C)`` + ``DiceMetric``), restated the same way:

* argmax over channels with **ties to the lowest index**; the comparison is strict (``z_c > best``, the best starting at
  −inf with class 0), so a NaN never wins and an all-NaN voxel gives class 0; the decision is taken on the stored values —
  bf16 logits are compared as stored.  This equals ``AsDiscrete(argmax=True)`` on the CPU for NaN-free input.  The composed
  branch implements lowest-index explicitly (``where(z == amax, arange, C).amin(1)``), it does not trust ``torch.argmax``;
* multi-class Dice: per (sample, class) the three exact integer counts ``|P=c ∧ Y=c|``, ``|P=c|`` and ``|Y=c|`` of the
  predicted and the labelled class maps go through the same `_dice_from_counts` (``include_background``, ``ignore_empty``);
* labels follow the loss's conventions (factorizer_amd/losses.py): converted as ``.long()`` does, a label outside [0, C)
  matches no class.

Native (`fz_seg_argmax`: one streaming pass, any V) for fp32 / bf16 device logits with 2 <= C <= 16 and uint8 / int64 / fp32
label maps; a label map given as the *prediction* (or to `one_hot_mask`) is native as uint8.  fp16 / fp64 logits, C > 16 and
other label types run composed ops on device and say so once.  A multi-class ``restore_prediction`` and surface Dice are
not built.

Device tensors run the kernels of csrc/segmetric.hip: one streaming pass for the three integer counts (and the mask), one for
the edges, and a brute-force nearest-edge search over the two SURFACE lists (DESIGN.md §3.11 says why that beats a
separable distance transform here).  CPU tensors run composed framework ops; device tensors outside the native gate (fp16 /
fp64 logits, an image axis longer than 2048 for the distance search) run composed ops on device and say so once.
"""
from __future__ import annotations

import math

import torch

from . import _native as N
from . import composed
from . import functional as Fn

MAX_AXIS = 2048   # the distance kernel is exact in fp32 while 3 · (axis − 1)² < 2²⁴


def _bound(sigmoid: bool, threshold: float) -> float:
    """the fp32 decision bound on the stored value: foreground iff x >= bound"""
    t = float(threshold)
    if not sigmoid:
        b = t
    elif t <= 0.0:
        b = -math.inf
    elif t >= 1.0:
        b = math.inf
    else:
        b = math.log(t / (1.0 - t))   # float64
    return float(torch.tensor(b, dtype=torch.float64).to(torch.float32))


def _is_mask(x) -> bool:
    return x.dtype in (torch.uint8, torch.bool)


def _check(pred, label=None):
    if pred.dim() < 3 or pred.dim() > 5:
        raise ValueError("segmentation metrics take (B, C, *S) tensors with 1, 2 or 3 spatial axes")
    if label is not None and tuple(label.shape) != tuple(pred.shape):
        raise ValueError(f"prediction {tuple(pred.shape)} and label {tuple(label.shape)} differ in shape")


def _native(*ts) -> bool:
    """every tensor on device, non-empty and of a kind the kernels read"""
    return all(t.is_cuda and t.numel() > 0 and Fn.seg_kind_ok(t) for t in ts)


def _warn(what, *ts):
    if any(t.is_cuda and t.numel() for t in ts):
        composed.warn_once(f"metrics:{what}:" + ",".join(str(t.dtype) for t in ts),
                           f"{what}: {', '.join(str(t.dtype) for t in ts)} is outside the native kernel set (fp32 / bf16 "
                           "values, uint8 / bool masks): composed framework ops")


def _decide(x, sigmoid, threshold):
    """bool foreground of a prediction tensor, composed"""
    if _is_mask(x):
        return x != 0
    b = _bound(sigmoid, threshold)
    return (x.float() if x.dtype in (torch.bfloat16, torch.float16) else x) >= b


# ---- mutually exclusive classes: argmax, one-hot, counts -------------------------------------------------------------------
MAX_CLASSES = 16   # channel slots of fz_seg_argmax


def _argmax_only(argmax, sigmoid, threshold):
    if argmax and (not sigmoid or threshold != 0.5):
        raise ValueError("argmax=True decides by the largest logit: it takes neither sigmoid=False nor a threshold")


def _argmax_composed(x):
    """int64 (B, *S): argmax over dim 1, ties to the lowest index, a NaN never wins (all NaN: class 0)"""
    z = x.float() if x.dtype in (torch.bfloat16, torch.float16) else x
    z = torch.where(torch.isnan(z), torch.full_like(z, -math.inf), z)
    C = z.shape[1]
    cls = torch.arange(C, device=z.device).view(1, C, *([1] * (z.dim() - 2)))
    return torch.where(z == z.amax(1, keepdim=True), cls, C).amin(1)


def _one_hot_composed(idx, valid, C):
    """uint8 (B, C, *S) from int64 classes (B, *S); all-zero rows where not valid"""
    cls = torch.arange(C, device=idx.device).view(1, C, *([1] * (idx.dim() - 1)))
    hit = idx.unsqueeze(1) == cls
    return (hit if valid is None else hit & valid.unsqueeze(1)).to(torch.uint8)


def _logits_native(x) -> bool:
    return x.is_cuda and x.numel() > 0 and x.dtype in (torch.float32, torch.bfloat16) and 2 <= x.shape[1] <= MAX_CLASSES \
        and x.shape[0] <= 65535


def _warn_mc(what, why, *ts):
    if any(t.is_cuda and t.numel() for t in ts):
        composed.warn_once(f"metrics:{what}:{why}", f"{what}: {why} is outside the native argmax kernel (fp32 / bf16 logits, "
                           f"2 <= C <= {MAX_CLASSES}, uint8 / int64 / float32 label maps): composed framework ops")


def _mc_why(x):
    return f"{x.dtype} logits" if x.dtype not in (torch.float32, torch.bfloat16) else f"C = {x.shape[1]}"


def _check_mc(pred, labels=None):
    if pred.dim() < 3 or pred.dim() > 5:
        raise ValueError("segmentation metrics take (B, C, *S) tensors with 1, 2 or 3 spatial axes")
    if labels is not None and (labels.dim() != pred.dim() or labels.shape[1] != 1 or labels.shape[0] != pred.shape[0]
                               or labels.shape[2:] != pred.shape[2:]):
        raise ValueError(f"prediction {tuple(pred.shape)} needs a label map (B, 1, *S), got {tuple(labels.shape)}")


def _discretize_argmax(x, to_onehot):
    _check_mc(x)
    if x.shape[1] < 2:
        raise ValueError(f"argmax=True needs at least two channels, got {tuple(x.shape)}")
    if _logits_native(x):
        cmap, onehot, _ = Fn.seg_argmax(x.contiguous(), None, x.shape[1], want_map=not to_onehot, want_onehot=to_onehot)
        return onehot if to_onehot else cmap
    _warn_mc("discretize", _mc_why(x), x)
    idx = _argmax_composed(x)
    return _one_hot_composed(idx, None, x.shape[1]) if to_onehot else idx.unsqueeze(1).to(torch.uint8)


def one_hot_mask(labels, num_classes: int):
    """``AsDiscrete(to_onehot=num_classes)`` of a class-index label map (B, 1, *S): the uint8 mask (B, C, *S) that
    `mask_edges` / `hausdorff_distance` take.  A label outside [0, C) gives an all-zero row (the loss's convention)."""
    _check_mc(labels)
    C = int(num_classes)
    if labels.shape[1] != 1 or C < 1:
        raise ValueError(f"one_hot_mask takes a label map (B, 1, *S) and num_classes >= 1, got {tuple(labels.shape)}, {C}")
    if labels.is_cuda and labels.numel() and labels.dtype == torch.uint8 and 2 <= C <= MAX_CLASSES and labels.shape[0] <= 65535:
        return Fn.seg_argmax(labels.contiguous(), None, C, want_onehot=True)[1]
    _warn_mc("one_hot_mask", f"a {labels.dtype} label map" if labels.dtype != torch.uint8 else f"C = {C}", labels)
    from .losses import _label_classes
    return _one_hot_composed(*_label_classes(labels, C), C)


def multiclass_counts(pred, labels, num_classes: int | None = None):
    """int64 (B, C, 3): per (sample, class) |P = c ∧ Y = c|, |P = c| and |Y = c| as exact integers.  ``pred`` holds logits
    (B, C, *S) — P is their argmax, see the module docstring — or an already discrete label map (B, 1, *S), which needs
    ``num_classes``; ``labels`` is the class-index label map (B, 1, *S)."""
    _check_mc(pred, labels)
    is_map = pred.shape[1] == 1
    if is_map and num_classes is None:
        raise ValueError("multiclass_counts: a label map as the prediction needs num_classes")
    C = int(num_classes) if num_classes is not None else pred.shape[1]
    if not is_map and C != pred.shape[1]:
        raise ValueError(f"multiclass_counts: num_classes = {C} against logits {tuple(pred.shape)}")
    pred_ok = (pred.is_cuda and pred.numel() > 0 and pred.dtype == torch.uint8 and 2 <= C <= MAX_CLASSES
               and pred.shape[0] <= 65535) if is_map else _logits_native(pred)
    if pred_ok and labels.is_cuda and labels.dtype in Fn.LABEL_KIND:
        return Fn.seg_argmax(pred.contiguous(), labels.contiguous(), C, want_counts=True)[2]
    why = (f"a {pred.dtype} label map" if is_map and pred.dtype != torch.uint8 else
           _mc_why(pred) if not is_map and not _logits_native(pred) else
           f"a {labels.dtype} label map" if labels.dtype not in Fn.LABEL_KIND else f"C = {C}")
    _warn_mc("multiclass_counts", why, pred, labels)
    from .losses import _label_classes
    if is_map:
        p, pv = _label_classes(pred, C)
    else:
        p, pv = _argmax_composed(pred), None
    y, yv = _label_classes(labels, C)
    P, Y = _one_hot_composed(p, pv, C).bool(), _one_hot_composed(y, yv, C).bool()
    dims = tuple(range(2, P.dim()))
    return torch.stack([(P & Y).sum(dims), P.sum(dims), Y.sum(dims)], dim=-1).to(torch.int64)


def discretize(x, sigmoid: bool = True, threshold: float = 0.5, argmax: bool = False, to_onehot: bool = False):
    """``Activations(sigmoid)`` + ``AsDiscrete(threshold)``: uint8 mask, 1 iff ``sigmoid(x) >= threshold`` (decided on the
    logit, see the module docstring); with ``sigmoid=False`` ``x`` is a probability or mask and the test is
    ``x >= threshold``.  A uint8 / bool ``x`` is already discrete: non-zero is foreground.
    ``argmax=True``: ``AsDiscrete(argmax=True)`` — the uint8 class map (B, 1, *S), ties to the lowest index — or, with
    ``to_onehot=True``, ``AsDiscrete(argmax=True, to_onehot=C)``: the uint8 mask (B, C, *S)."""
    _argmax_only(argmax, sigmoid, threshold)
    if argmax:
        return _discretize_argmax(x, to_onehot)
    if to_onehot:
        raise ValueError("to_onehot=True belongs to argmax=True (a label map goes through one_hot_mask)")
    _check(x)
    if _native(x):
        return Fn.seg_counts(x.contiguous(), None, _bound(sigmoid, threshold), want_mask=True, want_counts=False)[1]
    _warn("discretize", x)
    return _decide(x, sigmoid, threshold).to(torch.uint8)


def _counts_and_mask(pred, label, sigmoid, threshold, want_mask):
    _check(pred, label)
    if _native(pred, label):
        return Fn.seg_counts(pred.contiguous(), label.contiguous(), _bound(sigmoid, threshold), want_mask=want_mask)
    _warn("segmentation_counts", pred, label)
    p = _decide(pred, sigmoid, threshold)
    y = label != 0
    dims = tuple(range(2, pred.dim()))
    counts = torch.stack([(p & y).sum(dims), p.sum(dims), y.sum(dims)], dim=-1).to(torch.int64)
    return counts, (p.to(torch.uint8) if want_mask else None)


def segmentation_counts(pred, label, sigmoid: bool = True, threshold: float = 0.5):
    """int64 (B, C, 3): per (sample, channel) plane |P ∧ Y|, |P| and |Y| as exact integers.  ``pred`` holds logits (fp32 or
    bf16; P as in `discretize`) or an already discrete uint8 / bool mask; ``label`` is binary, stored as uint8, bool, fp32
    or bf16 — **a non-zero label element counts as 1**, whatever its value."""
    return _counts_and_mask(pred, label, sigmoid, threshold, False)[0]


def _dice_from_counts(counts, include_background, ignore_empty):
    inter, p, y = (counts[..., k].to(torch.float64) for k in range(3))
    dice = 2.0 * inter / (p + y)                       # 0 / 0 = NaN where both are empty: replaced below
    empty = y == 0
    if ignore_empty:
        fill = torch.full_like(dice, math.nan)
    else:
        fill = (p == 0).to(torch.float64)              # 1.0 when the prediction is empty too, else 0.0
    dice = torch.where(empty, fill, dice).to(torch.float32)
    return dice if include_background else dice[:, 1:]


def dice_metric(pred, label, *, sigmoid: bool = True, threshold: float = 0.5, include_background: bool = True,
                ignore_empty: bool = False, argmax: bool = False):
    """MONAI 1.4 ``DiceMetric`` values, float32 (B, C): ``2 |P∧Y| / (|P| + |Y|)`` where |Y| > 0; where the label plane is
    empty NaN (``ignore_empty=True``), else 1.0 if the prediction is empty as well and 0.0 if not.  The quotient is formed
    from the exact counts in float64 and rounded once.  ``include_background=False`` drops channel 0.
    ``argmax=True``: mutually exclusive classes — ``pred`` logits (B, C, *S), ``label`` a class-index map (B, 1, *S), the
    counts those of `multiclass_counts`."""
    _argmax_only(argmax, sigmoid, threshold)
    if argmax:
        return _dice_from_counts(multiclass_counts(pred, label), include_background, ignore_empty)
    return _dice_from_counts(segmentation_counts(pred, label, sigmoid, threshold), include_background, ignore_empty)


# ---- reductions (monai.metrics.utils.do_metric_reduction) ----------------------------------------------------------------
REDUCTIONS = ("mean", "mean_batch", "mean_channel", "none")


def _nanmean(f, dim):
    ok = ~torch.isnan(f)
    n = ok.sum(dim)
    s = torch.where(ok, f, torch.zeros_like(f)).sum(dim)
    return torch.where(n > 0, s / n.clamp_min(1).to(f.dtype), torch.zeros_like(s)), n


def reduce_metric(f, reduction: str = "mean"):
    """NaN-aware reduction of (N, C) metric values: "mean" first over the channels of a sample, then over the samples that
    had a valid channel; "mean_batch" over samples per channel (C,); "mean_channel" over channels per sample (N,); "none"
    the values themselves.  A mean over no valid entry is 0.0."""
    if reduction not in REDUCTIONS:
        raise ValueError(f"reduction must be one of {REDUCTIONS}, got {reduction!r}")
    if reduction == "none":
        return f
    if reduction == "mean_batch":
        return _nanmean(f, 0)[0]
    m, n = _nanmean(f, 1)
    if reduction == "mean_channel":
        return m
    valid = n > 0
    k = valid.sum()
    return torch.where(k > 0, torch.where(valid, m, torch.zeros_like(m)).sum() / k.clamp_min(1).to(m.dtype),
                       torch.zeros((), dtype=m.dtype, device=m.device))


class _Cumulative:
    """the accumulating side of MONAI's CumulativeIterationMetric: every call appends its (B, C) values"""

    def __init__(self, reduction):
        if reduction not in REDUCTIONS:
            raise ValueError(f"reduction must be one of {REDUCTIONS}, got {reduction!r}")
        self.reduction = reduction
        self._buffer = []

    def _compute(self, pred, label):
        raise NotImplementedError

    def __call__(self, pred, label):
        v = self._compute(pred, label)
        self._buffer.append(v)
        return v

    def get_buffer(self):
        """all values seen since the last reset, (N, C); None before the first call"""
        return torch.cat(self._buffer, dim=0) if self._buffer else None

    def aggregate(self, reduction: str | None = None):
        buf = self.get_buffer()
        if buf is None:
            raise ValueError("aggregate() before any call: the buffer is empty")
        return reduce_metric(buf, reduction or self.reduction)

    def reset(self):
        self._buffer = []


class DiceMetric(_Cumulative):
    """``DiceMetric(include_background, reduction, ignore_empty)`` of the recipe behind the bundle's post-processing
    (``sigmoid`` / ``threshold``: the ``Activationsd`` / ``AsDiscreted`` in front of it; pass ``sigmoid=False`` or masks for
    already discrete predictions; ``argmax=True``: logits of mutually exclusive classes against a class-index label map,
    `multiclass_counts`).  ``metric(pred, label)`` returns the (B, C) values and keeps them; ``aggregate()`` reduces
    everything kept since ``reset()``."""

    def __init__(self, include_background: bool = True, reduction: str = "mean", ignore_empty: bool = False,
                 sigmoid: bool = True, threshold: float = 0.5, argmax: bool = False):
        super().__init__(reduction)
        _argmax_only(argmax, sigmoid, threshold)
        self.include_background, self.ignore_empty = include_background, ignore_empty
        self.sigmoid, self.threshold, self.argmax = sigmoid, threshold, argmax

    def _compute(self, pred, label):
        return dice_metric(pred, label, sigmoid=self.sigmoid, threshold=self.threshold,
                           include_background=self.include_background, ignore_empty=self.ignore_empty, argmax=self.argmax)


# ---- edges and the Hausdorff distance --------------------------------------------------------------------------------------
def _edges_composed(m):
    """bool edges of a bool mask (B, C, *S): foreground with a background or out-of-image face neighbour"""
    nd = m.dim() - 2
    inner = m.clone()
    for ax in range(2, 2 + nd):
        n = m.shape[ax]
        zero = torch.zeros_like(m.narrow(ax, 0, 1))
        inner &= torch.cat([zero, m.narrow(ax, 0, n - 1)], dim=ax)    # neighbour at −1 (outside: background)
        inner &= torch.cat([m.narrow(ax, 1, n - 1), zero], dim=ax)    # neighbour at +1
    return m & ~inner


def _edges_and_counts(mask):
    _check(mask)
    if _native(mask) and _is_mask(mask):
        return Fn.mask_edges(mask.contiguous())
    if not _is_mask(mask):
        _warn("mask_edges", mask)
    e = _edges_composed(mask != 0)
    return e.to(torch.uint8), e.sum(tuple(range(2, mask.dim()))).to(torch.int64)


def mask_edges(mask):
    """uint8 edge mask: 1 where ``mask`` is foreground (non-zero) and at least one of its 2·nd face neighbours is background
    or lies outside the image — ``mask ^ binary_erosion(mask)`` with the cross element and a zero border (MONAI's
    ``get_mask_edges``, with or without its crop)."""
    return _edges_and_counts(mask)[0]


def _spacing(spacing, nd):
    if spacing is None:
        return (1.0,) * nd
    if isinstance(spacing, (int, float)):
        return (float(spacing),) * nd
    s = tuple(float(v) for v in spacing)
    if len(s) != nd:
        raise ValueError(f"spacing needs one value per spatial axis ({nd}), got {s}")
    return s


def _min_dist_composed(q, t, spacing):
    """float64 distances from every row of q (nq, nd) to the nearest row of t (nt, nd) — all pairs, in chunks"""
    s = torch.tensor(spacing, dtype=torch.float64, device=q.device)
    qs, ts = q.to(torch.float64) * s, t.to(torch.float64) * s
    step = max(1, (1 << 22) // max(1, ts.shape[0]))
    out = [((qs[i:i + step, None, :] - ts[None, :, :]) ** 2).sum(-1).min(dim=1).values
           for i in range(0, qs.shape[0], step)]
    return torch.cat(out).sqrt()


def _coords4(idx):
    """(n, nd) int64 voxel indices -> (n, 4) fp32, axis k in column k, zeros behind"""
    c = torch.zeros((idx.shape[0], 4), dtype=torch.float32, device=idx.device)
    c[:, :idx.shape[1]] = idx.to(torch.float32)
    return c


def _quantile(d, percentile):
    if percentile is None:
        return d.max()
    return torch.quantile(d, float(percentile) / 100.0)


def hausdorff_distance(pred_mask, label_mask, *, percentile=95, spacing=None, directed: bool = False,
                       include_background: bool = True):
    """MONAI 1.4 ``compute_hausdorff_distance`` values, float32 (B, C), of two discrete masks (B, C, *S) (non-zero is
    foreground).  Per plane d(P→Y) is the ``percentile / 100`` quantile (linear interpolation; ``None``: the maximum) of
    ``min_y ‖s ∘ (p − y)‖₂`` over the edge voxels p of P, y of Y; NaN when P has no edge, +inf when only Y has none.
    ``directed=False`` returns the NaN-propagating maximum of d(P→Y) and d(Y→P).  ``spacing``: None (unit), a scalar, or one
    value per spatial axis.  The square roots and the quantile are taken in float64 and rounded once."""
    _check(pred_mask, label_mask)
    if percentile is not None and not 0 <= percentile <= 100:
        raise ValueError(f"percentile must be in [0, 100] or None, got {percentile}")
    nd = pred_mask.dim() - 2
    sp = _spacing(spacing, nd)
    if not include_background:
        pred_mask, label_mask = pred_mask[:, 1:], label_mask[:, 1:]
    B, C = pred_mask.shape[:2]
    dev = pred_mask.device
    out = torch.full((B, C), math.nan, dtype=torch.float32, device=dev)
    if B * C == 0:
        return out
    ep, np_ = _edges_and_counts(pred_mask)
    ey, ny_ = _edges_and_counts(label_mask)
    native = ep.is_cuda
    if native and max(pred_mask.shape[2:]) > MAX_AXIS:
        composed.warn_once("metrics:hausdorff_distance:axis",
                           f"hausdorff_distance: an image axis of {max(pred_mask.shape[2:])} voxels is longer than "
                           f"{MAX_AXIS}, the exact range of the native distance kernel: composed framework ops")
        native = False
    w = [s * s for s in sp] + [1.0] * (3 - nd)           # float64 squares, rounded to fp32 at the call
    np_, ny_ = np_.tolist(), ny_.tolist()                # one sync: the list lengths size the launches
    for b in range(B):
        for c in range(C):
            n_p, n_y = np_[b][c], ny_[b][c]
            vals = []
            for (nq, nt, eq, et) in ((n_p, n_y, ep, ey),) + (() if directed else ((n_y, n_p, ey, ep),)):
                if nq == 0:
                    vals.append(math.nan)
                elif nt == 0:
                    vals.append(math.inf)
                else:
                    qi, ti = torch.nonzero(eq[b, c]), torch.nonzero(et[b, c])
                    if native:
                        d = Fn.edge_min_dist2(_coords4(qi), _coords4(ti), w).to(torch.float64).sqrt()
                    else:
                        d = _min_dist_composed(qi, ti, sp)
                    vals.append(_quantile(d, percentile))
            if any(isinstance(v, float) and math.isnan(v) for v in vals):
                continue                                  # NaN propagates through the maximum
            vals = [v if torch.is_tensor(v) else torch.tensor(v, dtype=torch.float64, device=dev) for v in vals]
            out[b, c] = torch.stack(vals).max().to(torch.float32)
    return out


class HausdorffDistanceMetric(_Cumulative):
    """``HausdorffDistanceMetric(include_background, percentile, directed, reduction)`` over discrete masks, accumulating as
    `DiceMetric` does; ``spacing`` as in `hausdorff_distance`.  The defaults are MONAI's — ``include_background=False``,
    ``percentile=None`` — and the bundles pass ``include_background=True, percentile=95`` (train.yaml:279-287).
    ``argmax=True``: ``pred`` is logits (B, C, *S) and ``label`` a class-index map (B, 1, *S); both become one-hot masks
    (`discretize(argmax=True, to_onehot=True)`, `one_hot_mask`) in front of the same `hausdorff_distance`."""

    def __init__(self, include_background: bool = False, percentile=None, directed: bool = False, reduction: str = "mean",
                 spacing=None, argmax: bool = False):
        super().__init__(reduction)
        self.include_background, self.percentile, self.directed, self.spacing = include_background, percentile, directed, spacing
        self.argmax = argmax

    def _compute(self, pred, label):
        if self.argmax:
            _check_mc(pred, label)
            pred, label = discretize(pred, argmax=True, to_onehot=True), one_hot_mask(label, pred.shape[1])
        return hausdorff_distance(pred, label, percentile=self.percentile, spacing=self.spacing, directed=self.directed,
                                  include_background=self.include_background)
