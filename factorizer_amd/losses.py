"""Segmentation loss of the training step: the reference bundle's
``DiceCELoss(sigmoid=True, squared_pred=True)`` (model_zoo/factorizer_brats23/configs/train.yaml:67-70).
MONAI (pinned 1.4.0, docs/requirements.txt:11) is third-party and absent here; its published
evaluation is restated:

* Dice term: ``DiceLoss(sigmoid=True, squared_pred=True)`` — per (b, c) plane
  ``1 − (2 Σ p t + 1e-5) / (Σ p² + Σ t² + 1e-5)`` with ``p = sigmoid(z)``, mean over (b, c);
* cross-entropy term: for **one** prediction channel ``BCEWithLogitsLoss``; for C > 1 channels (the
  3-channel BraTS head) ``nn.CrossEntropyLoss`` over the channel softmax with the float multi-label
  target as class probabilities: ``mean_{b,v} −Σ_c t_c · log_softmax(z)_c`` — `dice_ce_loss`.

`dice_bce_loss` (sigmoid Dice + per-channel BCE for any C) is NOT the recipe's objective for C > 1; it
is kept as a separate, documented loss.

Device tensors: one fused reduction pass + one fused gradient pass (csrc/loss.hip) behind ONE autograd Function,
`DiceLossFn`, whatever the kind (Dice + BCE, Dice + CE) and the way the target is read; CPU tensors: composed ATen ops.

`DeepSupervisionLoss` / `deep_supervision_loss` (MONAI 1.4 semantics, restated below) sum that loss over the head list
of a ``num_deep_supr`` network; coarse levels read the full-resolution target through an index map (the same kernels with
their level reader).

The class-index form (mutually exclusive classes, e.g. the 16 classes of AMOS22 with uint8 label maps):
``DiceCELoss(softmax=True, to_onehot_y=True, include_background=ib, squared_pred=sq, smooth_nr=s, smooth_dr=s)(z, y)`` —
`dice_ce_softmax_loss`.  ``z`` is logits (B, C, *S) with 2 <= C, ``y`` a class-index label map (B, 1, *S).
With ``p = softmax(z, dim=1)``, ``t_c = [y == c]`` (the one-hot target, never stored) and ``c0 = 0`` if ``ib`` else 1, the sums
over the voxels of each plane (b, c >= c0) are ``inter = Σ p_c t_c``, ``pred = Σ p_c²`` if ``sq`` else ``Σ p_c`` and
``ground = Σ t_c`` (one-hot: t² = t), and

* Dice term: mean over (b, c >= c0) of ``1 − (2·inter + s) / (pred + ground + s)``;
* CE term: ``nn.CrossEntropyLoss()`` on class indices, always over all C classes, background included:
  mean over (b, v) of ``logsumexp_c(z) − z_y``;
* loss = Dice term + CE term.

Gradient, with ``g`` the upstream scalar, ``num = 2·inter + s``, ``den = pred + ground + s``, ``cd = 1/(B·(C − c0))``,
``cb = 1/(B·V)``: ``a_c = cd·(−2 t_c/den_c + num_c·(2 p_c if sq else 1)/den_c²)`` for ``c >= c0``, otherwise 0, and
``dL/dz_k = g·[ p_k·(a_k − Σ_c a_c p_c) + cb·(p_k − t_k) ]`` — the CE part ``cb·(p_k − t_k)`` is absent at a voxel whose
label matches no class (checked against float64 autograd for all four (sq, ib):
tests/test_softmax_loss_cpu.py).

Label conventions (this build's): a label is converted as ``.long()`` does — a float label truncates toward zero; a label
outside [0, C) (a NaN float label included) matches no class: its one-hot row is all zero and its CE contribution is zero,
but it is still counted in the CE mean's B·V.  No device-side assert, ever: an abort on a shared GPU is worse than a
documented convention.  The composed paths implement the same rule: they mask, they do not call ``F.one_hot`` on bad values.

Native for fp32 (bf16 / fp16: cast once) device logits with 2 <= C <= 16 and V a positive multiple of 4, and a contiguous
uint8 / int64 / fp32 label map, read in its own type; anything else runs composed framework ops, on a device with one
warning per reason.  Not built, and not accepted as arguments: ``ce_weight`` / ``weight``, ``label_smoothing``, ``jaccard``,
``batch=True``, ``lambda_dice`` / ``lambda_ce``, ``other_act``, ``reduction != "mean"``; a soft (B, C, *S) target with
``softmax=True`` has no native path (composed).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import _native as N
from . import functional as Fn


def dice_bce_loss_composed(logits, target, smooth: float = 1e-5):
    p = torch.sigmoid(logits)
    dims = tuple(range(2, logits.ndim))
    inter = (p * target).sum(dims)
    den = (p * p).sum(dims) + (target * target).sum(dims)
    dice = 1.0 - (2.0 * inter + smooth) / (den + smooth)
    return dice.mean() + F.binary_cross_entropy_with_logits(logits, target)


def _bce_finish(part, planes, V, smooth):
    """(loss, coef (planes, 2) = {2·inter + smooth, den + smooth}) from the partials (planes, nchunk, 4) of a Dice + BCE sums pass"""
    s = part.sum(dim=1)  # (planes, 4) — tiny
    num = 2.0 * s[:, 0] + smooth
    den = s[:, 1] + s[:, 2] + smooth
    loss = (1.0 - num / den).mean() + s[:, 3].sum() / (planes * V)
    return loss, torch.stack([num, den], dim=1).contiguous()


def _ce_finish(part, B, C, V, smooth):
    """(loss, coef (B·C, 2)) from the partials (B, nchunk, 3C + 1) of a Dice + CE sums pass"""
    if B <= 8:   # one finish launch instead of a dozen framework kernels (chunk sum, num, den, means)
        loss = torch.empty((), dtype=part.dtype, device=part.device)
        coef = torch.empty((B * C, 2), dtype=part.dtype, device=part.device)
        with torch.cuda.device(part.device):
            rc = N.lib().fz_dice_ce_finish(part.data_ptr(), B, C, V, float(smooth), loss.data_ptr(), coef.data_ptr(), N.stream_ptr(part))
        N.check(rc, "fz_dice_ce_finish")
        return loss, coef
    s = part.sum(dim=1)  # (B, 3C+1) — tiny
    d = s[:, :3 * C].reshape(B, C, 3)
    num = 2.0 * d[..., 0] + smooth
    den = d[..., 1] + d[..., 2] + smooth
    loss = (1.0 - num / den).mean() + s[:, 3 * C].sum() / (B * V)
    return loss, torch.stack([num, den], dim=-1).reshape(B * C, 2).contiguous()


def _sce_finish(part, B, C, V, c0, smooth):
    """(loss, coef (B·C, 2)) from the partials (B, nchunk, 3C + 1) of a class-index sums pass; the Dice mean runs over the
    channels c >= c0, the planes below get the inert coefficients {0, 1}"""
    if B <= 8:
        loss = torch.empty((), dtype=part.dtype, device=part.device)
        coef = torch.empty((B * C, 2), dtype=part.dtype, device=part.device)
        with torch.cuda.device(part.device):
            rc = N.lib().fz_dice_sce_finish(part.data_ptr(), B, C, V, c0, float(smooth), loss.data_ptr(), coef.data_ptr(),
                                            N.stream_ptr(part))
        N.check(rc, "fz_dice_sce_finish")
        return loss, coef
    s = part.sum(dim=1)  # (B, 3C+1) — tiny
    d = s[:, :3 * C].reshape(B, C, 3)
    num = 2.0 * d[..., 0] + smooth
    den = d[..., 1] + d[..., 2] + smooth
    loss = (1.0 - num / den)[:, c0:].mean() + s[:, 3 * C].sum() / (B * V)
    if c0:
        num = torch.cat([torch.zeros_like(num[:, :c0]), num[:, c0:]], dim=1)
        den = torch.cat([torch.ones_like(den[:, :c0]), den[:, c0:]], dim=1)
    return loss, torch.stack([num, den], dim=-1).reshape(B * C, 2).contiguous()


_DS_TKIND = {torch.float32: N.SEG_F32, torch.bfloat16: N.SEG_BF16, torch.uint8: N.SEG_U8, torch.bool: N.SEG_U8}


def _lift3(spatial):
    return (1,) * (3 - len(spatial)) + tuple(int(s) for s in spatial)


class DiceLossFn(torch.autograd.Function):
    """The native loss of every path: one sums pass and a finish forward, one gradient pass backward — the entry points
    fz_dice_{bce,ce}[_ds]_{sums,grad} of csrc/loss.hip, timed under their names without the fz_.
    kind: "bce" — every (b, c) plane on its own, partials (B·C, nchunk, 4), `_bce_finish` — "ce" — the C channels of a
    batch item together, partials (B, nchunk, 3C + 1), `_ce_finish` — or "sce" — the class-index form: softmax over the
    channels, target a label map (B, 1, *S) of uint8 / int64 / fp32 read in its own type, opts = (squared_pred,
    c0 = first Dice channel), partials as "ce", `_sce_finish`; the entry points take the label kind behind the sizes and
    (sq[, c0]) behind that.
    level: False — the target is fp32 at the logits' extents — or True — ONE coarse deep-supervision level against the
    full-resolution target as the caller holds it (fp32 / bf16 / uint8 / bool, contiguous): saved as given, never resampled,
    read through the index map (the fz_dice_*_ds_* entry points).  logits: fp32, contiguous or not."""

    @staticmethod
    def forward(ctx, logits, target, smooth, kind, level, opts=None):
        z = logits.contiguous()
        B, C = z.shape[:2]
        V = z.numel() // (B * C)
        sce = kind == "sce"
        if level:
            t = target.view(torch.uint8) if target.dtype == torch.bool else target
            where = (*_lift3(t.shape[2:]), *_lift3(z.shape[2:]), Fn.LABEL_KIND[t.dtype] if sce else _DS_TKIND[target.dtype])
        else:
            t = target.contiguous()
            where = (V, Fn.LABEL_KIND[t.dtype]) if sce else (V,)
        sq, c0 = (int(bool(opts[0])), int(opts[1])) if sce else (None, 0)
        fwd_x, bwd_x = ((sq,), (sq, c0)) if sce else ((), ())
        rows = (B * C,) if kind == "bce" else (B, C)      # how the entry points take the planes
        name = f"dice_{kind}_ds" if level else f"dice_{kind}"
        tbytes = (B * V if sce else z.numel()) * t.element_size()   # the level's voxels, not the target's
        lib = N.lib()
        part = torch.empty((rows[0], lib.fz_dice_bce_chunks(V), 4 if kind == "bce" else 3 * C + 1), dtype=z.dtype, device=z.device)
        with torch.cuda.device(z.device):
            rc = Fn._timed(name + "_sums", 4 * z.numel() + tbytes, lambda: getattr(lib, f"fz_{name}_sums")(
                z.data_ptr(), t.data_ptr(), part.data_ptr(), *rows, *where, *fwd_x, N.stream_ptr(z)), cols=B * V)
        N.check(rc, f"fz_{name}_sums")
        if sce:
            loss, coef = _sce_finish(part, B, C, V, c0, smooth)
        else:
            loss, coef = _bce_finish(part, B * C, V, smooth) if kind == "bce" else _ce_finish(part, B, C, V, smooth)
        ctx.save_for_backward(z, t, coef)
        ctx.call = (name, rows, where + bwd_x, 1.0 / (B * (C - c0)), 1.0 / (rows[0] * V), tbytes, B * V)
        return loss

    @staticmethod
    def backward(ctx, g):
        z, t, coef = ctx.saved_tensors
        name, rows, where, cd, cb, tbytes, cols = ctx.call
        gz = torch.empty_like(z)
        gs = g.reshape(1).to(z.dtype).contiguous()
        with torch.cuda.device(z.device):
            rc = Fn._timed(name + "_grad", 8 * z.numel() + tbytes, lambda: getattr(N.lib(), f"fz_{name}_grad")(
                z.data_ptr(), t.data_ptr(), coef.data_ptr(), gz.data_ptr(), *rows, *where, cd, cb, gs.data_ptr(),
                N.stream_ptr(z)), cols=cols)
        N.check(rc, f"fz_{name}_grad")
        return (gz,) + (None,) * (len(ctx.needs_input_grad) - 1)


def _shape_gate(logits, c_min, c_max, v_end=None):
    """The shape conditions of the native passes, stated here only: c_min <= C <= c_max channels and V voxels per plane a
    positive multiple of 4 (below v_end).  None, or (key, reason) of the first one missed, worded for the warning of a
    deep-supervision level — the dense losses only ask whether there is one."""
    B, C = logits.shape[:2]
    if not (c_min <= C and (c_max is None or C <= c_max)):
        return "channels", f"C = {C} (native: {c_min} <= C <= {c_max})"
    V = logits.numel() // max(B * C, 1)
    if V == 0 or V % 4 or (v_end is not None and V >= v_end):
        return "voxels", f"{V} level voxels (native: a multiple of 4 below 2^31)"
    return None


def _fp32_logits(logits, target):
    """The loss is evaluated in fp32 whatever the storage type of the network's activations (the head of a
    mixed-precision run emits bf16 logits: one cast of a (B, out_channels, V) tensor)."""
    if logits.dtype in (torch.bfloat16, torch.float16):
        logits = logits.float()
    if target.dtype != logits.dtype:
        target = target.to(logits.dtype)
    return logits, target


def _dense_loss(name, kind, composed, c_min, c_max, logits, target, smooth):
    """the loss of a target at the logits' extents: native for fp32 device tensors that pass `_shape_gate`, else `composed`"""
    logits, target = _fp32_logits(logits, target)
    if logits.is_cuda and logits.dtype == torch.float32 and _shape_gate(logits, c_min, c_max) is None:
        return DiceLossFn.apply(logits, target, smooth, kind, False)
    if logits.is_cuda and logits.numel():
        from .composed import warn_once
        warn_once(name, f"no native kernel for shape {tuple(logits.shape)} / {logits.dtype}: composed framework ops")
    return composed(logits, target, smooth)


def dice_bce_loss(logits, target, smooth: float = 1e-5):
    return _dense_loss("dice_bce_loss", "bce", dice_bce_loss_composed, 1, None, logits, target, smooth)


# ---- the recipe's loss: DiceCELoss(sigmoid=True, squared_pred=True), MONAI 1.4 semantics -------------------
def _dice_term(logits, target, smooth):
    p = torch.sigmoid(logits)
    dims = tuple(range(2, logits.ndim))
    inter = (p * target).sum(dims)
    den = (p * p).sum(dims) + (target * target).sum(dims)
    return (1.0 - (2.0 * inter + smooth) / (den + smooth)).mean()


def dice_ce_loss_composed(logits, target, smooth: float = 1e-5):
    if logits.shape[1] == 1:
        return dice_bce_loss_composed(logits, target, smooth)
    target = target.to(logits.dtype)
    return _dice_term(logits, target, smooth) + F.cross_entropy(logits, target)


def dice_ce_loss(logits, target, smooth: float = 1e-5):
    """``DiceCELoss(sigmoid=True, squared_pred=True)(logits, target)`` of the training recipe."""
    if logits.shape[1] == 1:
        return dice_bce_loss(logits, target, smooth)
    return _dense_loss("dice_ce_loss", "ce", dice_ce_loss_composed, 2, 8, logits, target, smooth)


class DiceCELoss(torch.nn.Module):
    """Drop-in for MONAI 1.4 ``DiceCELoss`` in its two forms:

    * the recipe's ``DiceCELoss(sigmoid=True, squared_pred=True)`` (train.yaml:67-70) — the default: independent sigmoid
      channels against a multi-label float target (`dice_ce_loss`);
    * ``DiceCELoss(softmax=True, to_onehot_y=True, include_background=..., squared_pred=...)``: mutually exclusive classes
      against a class-index label map (B, 1, *S) (`dice_ce_softmax_loss`); ``squared_pred`` defaults to MONAI's False here.

    ``sigmoid=None`` means ``not softmax``, ``squared_pred=None`` the form's default.  ``softmax=True, to_onehot_y=False``
    takes a (B, C, *S) target and runs composed framework ops.  ``ce_weight`` / ``weight``, ``label_smoothing``, ``jaccard``,
    ``batch``, ``lambda_dice`` / ``lambda_ce``, ``other_act`` and ``reduction`` are not arguments of this class."""

    def __init__(self, sigmoid: bool | None = None, squared_pred: bool | None = None, smooth_nr: float = 1e-5,
                 smooth_dr: float = 1e-5, softmax: bool = False, to_onehot_y: bool = False, include_background: bool = True):
        super().__init__()
        sigmoid = (not softmax) if sigmoid is None else bool(sigmoid)
        if sigmoid and softmax:
            raise ValueError("DiceCELoss: sigmoid=True and softmax=True exclude each other")
        if not (sigmoid or softmax):
            raise NotImplementedError("DiceCELoss: one of sigmoid=True / softmax=True is needed (no other activation is built)")
        if smooth_nr != smooth_dr:
            raise NotImplementedError("DiceCELoss: only smooth_nr == smooth_dr is implemented")
        if sigmoid:
            squared_pred = True if squared_pred is None else bool(squared_pred)
            if not squared_pred or to_onehot_y or not include_background:
                raise NotImplementedError("DiceCELoss: the sigmoid form is implemented as the recipe has it (squared_pred=True, "
                                          "to_onehot_y=False, include_background=True)")
        else:
            squared_pred = False if squared_pred is None else bool(squared_pred)
        self.sigmoid, self.softmax, self.to_onehot_y = sigmoid, bool(softmax), bool(to_onehot_y)
        self.squared_pred, self.include_background = squared_pred, bool(include_background)
        self.smooth = float(smooth_nr)

    @property
    def class_index(self) -> bool:
        """the target is a class-index label map (B, 1, *S)"""
        return self.softmax and self.to_onehot_y

    def forward(self, input, target):
        if self.sigmoid:
            return dice_ce_loss(input, target, self.smooth)
        if input.ndim < 3 or input.shape[1] < 2:
            raise ValueError(f"DiceCELoss(softmax=True): a one-channel input {tuple(input.shape)} has no softmax")
        if self.to_onehot_y:
            return dice_ce_softmax_loss(input, target, include_background=self.include_background,
                                        squared_pred=self.squared_pred, smooth=self.smooth)
        if target.shape != input.shape:
            raise ValueError(f"DiceCELoss(softmax=True, to_onehot_y=False): target {tuple(target.shape)} must have the "
                             f"logits' shape {tuple(input.shape)}")
        if input.dtype in (torch.bfloat16, torch.float16):
            input = input.float()
        if input.is_cuda and input.numel():
            from .composed import warn_once
            warn_once("dice_ce_softmax_loss:soft", "softmax DiceCE with a (B, C, *S) target has no native kernel: composed "
                      "framework ops")
        return _softmax_soft_target_composed(input, target, self.include_background, self.squared_pred, self.smooth)


# ---- the class-index form: DiceCELoss(softmax=True, to_onehot_y=True), MONAI 1.4 semantics (module docstring) ----------
def _label_classes(labels, C):
    """(idx int64 (B, *S) in [0, C), valid bool (B, *S)) of a label map (B, 1, *S): converted as .long() does (a float label
    truncates toward zero); a label outside [0, C), a NaN included, is not valid and names no class (idx 0 there)"""
    lab = labels[:, 0]
    if lab.dtype == torch.bool:
        lab = lab.to(torch.uint8)
    if lab.is_floating_point():
        valid = (lab > -1) & (lab < C)          # truncation maps (-1, 1) to class 0; a NaN fails both tests
        idx = torch.where(valid, lab, torch.zeros_like(lab)).long()
    else:
        idx = lab.long()
        valid = (idx >= 0) & (idx < C)
        idx = torch.where(valid, idx, torch.zeros_like(idx))
    return idx, valid


def _masked_one_hot(idx, valid, C, dtype):
    """(B, C, *S) one-hot of idx with all-zero rows where not valid — no F.one_hot on bad values"""
    cls = torch.arange(C, device=idx.device).view(1, C, *([1] * (idx.dim() - 1)))
    return ((idx.unsqueeze(1) == cls) & valid.unsqueeze(1)).to(dtype)


def _softmax_dice_term(p, t, include_background, squared_pred, smooth):
    dims = tuple(range(2, p.ndim))
    c0 = 0 if include_background else 1
    inter = (p * t).sum(dims)[:, c0:]
    pred = ((p * p) if squared_pred else p).sum(dims)[:, c0:]
    ground = t.sum(dims)[:, c0:]
    return (1.0 - (2.0 * inter + smooth) / (pred + ground + smooth)).mean()


def _check_label_map(logits, labels):
    if logits.ndim < 3 or logits.shape[1] < 2:
        raise ValueError(f"softmax DiceCE: logits {tuple(logits.shape)} need at least two channels (B, C >= 2, *S)")
    if labels.ndim != logits.ndim or labels.shape[1] != 1:
        raise ValueError(f"softmax DiceCE with to_onehot_y: the label map must be (B, 1, *S), got {tuple(labels.shape)}")
    if labels.shape[0] != logits.shape[0]:
        raise ValueError(f"softmax DiceCE: logits {tuple(logits.shape)} against labels {tuple(labels.shape)}")


def dice_ce_softmax_loss_composed(logits, labels, *, include_background: bool = True, squared_pred: bool = False,
                                  smooth: float = 1e-5):
    _check_label_map(logits, labels)
    if labels.shape[2:] != logits.shape[2:]:
        raise ValueError(f"softmax DiceCE: logits {tuple(logits.shape)} against labels {tuple(labels.shape)}")
    C = logits.shape[1]
    idx, valid = _label_classes(labels, C)
    t = _masked_one_hot(idx, valid, C, logits.dtype)
    dice = _softmax_dice_term(torch.softmax(logits, dim=1), t, include_background, squared_pred, smooth)
    nll = torch.logsumexp(logits, dim=1) - logits.gather(1, idx.unsqueeze(1))[:, 0]
    ce = torch.where(valid, nll, torch.zeros_like(nll)).sum() / valid.numel()    # the mean counts every voxel
    return dice + ce


def _softmax_soft_target_composed(logits, target, include_background, squared_pred, smooth):
    """softmax=True, to_onehot_y=False: a (B, C, *S) target of class probabilities / a stored one-hot — composed only"""
    target = target.to(logits.dtype)
    dice = _softmax_dice_term(torch.softmax(logits, dim=1), target, include_background, squared_pred, smooth)
    return dice + F.cross_entropy(logits, target)


def _sce_gate(logits, labels, v_end=None, dtypes=(torch.float32,)):
    """None when the class-index kernels of csrc/loss.hip take these logits and this label map, else (key, reason)"""
    if logits.dtype not in dtypes:
        return "logits", f"{logits.dtype} logits"
    why = _shape_gate(logits, 2, 16, v_end)
    if why is not None:
        return why
    if labels.dtype not in Fn.LABEL_KIND:
        return "labels", f"a {labels.dtype} label map (native: uint8 / int64 / float32)"
    if not Fn.label_kind_ok(labels):
        return "layout", "a label map that is not contiguous and 16-byte aligned"
    return None


def dice_ce_softmax_loss(logits, labels, *, include_background: bool = True, squared_pred: bool = False,
                         smooth: float = 1e-5):
    """``DiceCELoss(softmax=True, to_onehot_y=True, include_background, squared_pred, smooth_nr=smooth_dr=smooth)(logits,
    labels)``: logits (B, C >= 2, *S), labels a class-index map (B, 1, *S) — the module docstring has the formulas and the
    label conventions."""
    _check_label_map(logits, labels)
    if labels.shape[2:] != logits.shape[2:]:
        raise ValueError(f"softmax DiceCE: logits {tuple(logits.shape)} against labels {tuple(labels.shape)}")
    if logits.dtype in (torch.bfloat16, torch.float16):
        logits = logits.float()                  # one cast, as `_fp32_logits`
    if logits.is_cuda and logits.numel():
        why = _sce_gate(logits, labels)
        if why is None:
            return DiceLossFn.apply(logits, labels, smooth, "sce", False, (squared_pred, 0 if include_background else 1))
        from .composed import warn_once
        warn_once("dice_ce_softmax_loss:" + why[0], f"no native kernel for {why[1]}: composed framework ops")
    return dice_ce_softmax_loss_composed(logits, labels, include_background=include_background, squared_pred=squared_pred,
                                         smooth=smooth)


# ---- deep supervision: MONAI 1.4 DeepSupervisionLoss over the head list of num_deep_supr networks --------------------
# ushape.UNet returns one logits tensor per decoder level, finest first.  The loss of the list is Σ_l w_l · loss(z_l, t_l)
# (not normalised) with t_l the target itself where the level has its extents and its nearest-exact down-sampling otherwise.
# For an integer ratio r on an axis nearest-exact is the strided pick index = r·i + r//2, which csrc/loss.hip applies as
# an index map while it reads the full-resolution target: a coarse level then costs the launches of a dense one and writes
# no target of its own.  (For non-integer ratios torch's float arithmetic and the integer formula floor((2i+1)·S_t/(2·S_l))
# disagree — 26 -> 11 is the first case — so those are never computed natively.)
_DS_MODES = ("same", "exp", "two")


def _ds_check_mode(weight_mode):
    if weight_mode not in _DS_MODES:
        raise ValueError(f"deep supervision: weight_mode must be one of {_DS_MODES}, got {weight_mode!r}")


def ds_weights(levels: int, weight_mode: str = "exp", weights=None):
    """the level weights w_0 .. w_{levels-1}: explicit `weights` when there are enough of them, else by `weight_mode`"""
    _ds_check_mode(weight_mode)
    if weights is not None and len(weights) >= levels:
        return [float(w) for w in weights[:levels]]
    if weight_mode == "same":
        return [1.0] * levels
    if weight_mode == "exp":
        return [max(0.5 ** l, 0.0625) for l in range(levels)]
    return [1.0 if l == 0 else 0.5 for l in range(levels)]


def ds_target_composed(target, size, dtype):
    """the target of a level of spatial `size` in `dtype`: the target itself at its own size, else nearest-exact"""
    if tuple(target.shape[2:]) == tuple(size):
        return target
    if target.dtype == torch.bool:
        target = target.view(torch.uint8)
    return F.interpolate(target, size=tuple(size), mode="nearest-exact").to(dtype)


def ds_level_launches(B: int, C: int, backward: bool = False) -> int:
    """native launches of one sampled level: the sums pass, plus fz_dice_ce_finish where the dense loss runs it too (C >= 2 and
    B <= 8; the other finishes are framework reductions of the partials); the backward is one gradient pass"""
    if backward:
        return 1
    return 2 if (C >= 2 and B <= 8) else 1


def _ds_level_gate(loss, logits, target):
    """None when csrc/loss.hip takes this coarse level, else (key, reason) of the composed branch"""
    if not isinstance(loss, DiceCELoss):
        return "loss", f"{type(loss).__name__} is not ft.DiceCELoss"
    if not loss.sigmoid:   # softmax with a (B, C, *S) target: the level kernels of this gate are the sigmoid form's
        return "loss", "ft.DiceCELoss(softmax=True) with a (B, C, *S) target"
    if logits.dtype not in (torch.float32, torch.bfloat16):
        return "logits", f"{logits.dtype} logits"
    why = _shape_gate(logits, 1, 8, 2 ** 31)
    if why is not None:
        return why
    if len(logits.shape) > 5 or any(st % sl for st, sl in zip(target.shape[2:], logits.shape[2:])):
        return "ratio", f"target {tuple(target.shape[2:])} over level {tuple(logits.shape[2:])} is not an integer ratio"
    if target.dtype not in _DS_TKIND or not target.is_contiguous():
        return "target", f"{target.dtype} target, contiguous = {target.is_contiguous()}"
    return None


def ds_labels_composed(labels, size):
    """the label map of a level of spatial `size`: the map itself at its own size, else its nearest-exact pick, in its type"""
    if tuple(labels.shape[2:]) == tuple(size):
        return labels
    lab = labels.view(torch.uint8) if labels.dtype == torch.bool else labels
    src = lab if lab.is_floating_point() and lab.dtype != torch.float16 else lab.to(torch.float32)   # a pick: no arithmetic
    return F.interpolate(src, size=tuple(size), mode="nearest-exact").to(lab.dtype)


def _ds_label_gate(loss, logits, labels):
    """`_ds_level_gate` for the class-index form: None when csrc/loss.hip takes this coarse level"""
    if len(logits.shape) > 5 or any(st % sl for st, sl in zip(labels.shape[2:], logits.shape[2:])):
        return "ratio", f"target {tuple(labels.shape[2:])} over level {tuple(logits.shape[2:])} is not an integer ratio"
    return _sce_gate(logits, labels, 2 ** 31, (torch.float32, torch.bfloat16))


def deep_supervision_loss(inputs, target, loss=None, weight_mode: str = "exp", weights=None):
    """MONAI 1.4 ``DeepSupervisionLoss(loss, weight_mode, weights)(inputs, target)``: Σ_l w_l · loss(inputs[l], target_l) over a
    list of logits (B, C, *S_l), finest first — what ``Factorizer(..., num_deep_supr=k)`` / ``Deconver(..., num_deep_supr=k)``
    return.  A tensor, or a list of one tensor whose weight is 1 (every mode gives that), is ``loss(input, target)`` itself.
    On a device, with ``ft.DiceCELoss``, a coarse level reads the full-resolution target through the nearest-exact index map
    (csrc/loss.hip); a level the kernels do not take (`_ds_level_gate`) interpolates the target and calls `loss`.
    With the class-index form, ``ft.DiceCELoss(softmax=True, to_onehot_y=True)``, `target` is the label map (B, 1, *S_target)
    and a coarse level reads it through the same index map in its own type (`_ds_label_gate`)."""
    loss = DiceCELoss() if loss is None else loss
    _ds_check_mode(weight_mode)   # a bad mode is refused whatever the input is
    if isinstance(inputs, torch.Tensor):
        if inputs.ndim == target.ndim + 1:
            raise ValueError(f"deep supervision: the stacked form (B, L, C, *S) {tuple(inputs.shape)} is not supported; "
                             "pass the list of level logits")
        return loss(inputs, target)
    levels = list(inputs)
    if not levels:
        raise ValueError("deep supervision: an empty list of logits")
    w = ds_weights(len(levels), weight_mode, weights)
    if len(levels) == 1 and w[0] == 1.0:
        return loss(levels[0], target)
    total = None
    labels = isinstance(loss, DiceCELoss) and loss.class_index and target.ndim >= 3 and target.shape[1] == 1
    for wl, z in zip(w, levels):
        if z.ndim != target.ndim or (z.shape[0] != target.shape[0] if labels else z.shape[:2] != target.shape[:2]):
            raise ValueError(f"deep supervision: logits {tuple(z.shape)} against target {tuple(target.shape)}")
        if z.shape[2:] == target.shape[2:]:
            term = loss(z, target)
        elif labels:
            why = _ds_label_gate(loss, z, target) if z.is_cuda else ("cpu", "")
            if why is None:
                term = DiceLossFn.apply(z.float() if z.dtype != torch.float32 else z, target, loss.smooth, "sce", True,
                                        (loss.squared_pred, 0 if loss.include_background else 1))
            else:
                if z.is_cuda:
                    from .composed import warn_once
                    warn_once("deep_supervision_loss:labels:" + why[0], f"no native deep-supervision level for {why[1]}: "
                              "composed framework ops (interpolate the label map, then the loss)")
                term = loss(z, ds_labels_composed(target, z.shape[2:]))
        else:
            why = _ds_level_gate(loss, z, target) if z.is_cuda else ("cpu", "")
            if why is None:
                term = DiceLossFn.apply(z.float() if z.dtype != torch.float32 else z, target, loss.smooth,
                                        "bce" if z.shape[1] == 1 else "ce", True)
            else:
                if z.is_cuda:
                    from .composed import warn_once
                    warn_once("deep_supervision_loss:" + why[0], f"no native deep-supervision level for {why[1]}: "
                              "composed framework ops (interpolate, then the loss)")
                arith = torch.float32 if z.dtype in (torch.bfloat16, torch.float16) else z.dtype
                term = loss(z, ds_target_composed(target, z.shape[2:], arith))
        total = wl * term if total is None else total + wl * term
    return total


class DeepSupervisionLoss(torch.nn.Module):
    """Drop-in for MONAI 1.4 ``DeepSupervisionLoss(loss, weight_mode="exp", weights=None)`` on the head lists of this package's
    ``num_deep_supr`` networks (`deep_supervision_loss`)."""

    def __init__(self, loss, weight_mode: str = "exp", weights=None):
        super().__init__()
        _ds_check_mode(weight_mode)
        self.loss = loss
        self.weight_mode = weight_mode
        self.weights = None if weights is None else [float(v) for v in weights]

    def forward(self, input, target):
        return deep_supervision_loss(input, target, self.loss, self.weight_mode, self.weights)
