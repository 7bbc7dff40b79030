"""CPU side of the class-index DiceCE (ft.DiceCELoss(softmax=True, to_onehot_y=True), ft.dice_ce_softmax_loss): the
constructor matrix, the composed form against the independent float64 reference of tests/softmax_loss_cases.py, the
closed-form gradient the kernels evaluate against float64 autograd, the label conventions, and deep supervision with a label
map."""
import warnings

import pytest
import torch
import torch.nn.functional as F

import factorizer_amd as ft
from factorizer_amd import losses
import loss_adamw_cases as L
import softmax_loss_cases as S

SQ_IB = [(False, True), (False, False), (True, True), (True, False)]


# ---- constructor -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,sq", [
    (dict(softmax=True, to_onehot_y=True), False),
    (dict(softmax=True, to_onehot_y=True, squared_pred=True), True),
    (dict(softmax=True, to_onehot_y=True, squared_pred=False, include_background=False), False),
    (dict(softmax=True, to_onehot_y=True, squared_pred=True, include_background=False, smooth_nr=1e-3, smooth_dr=1e-3), True),
    (dict(sigmoid=False, softmax=True, to_onehot_y=True), False),
    (dict(softmax=True, to_onehot_y=False), False),
    (dict(), True), (dict(sigmoid=True), True), (dict(sigmoid=True, squared_pred=True), True),
])
def test_accepted_constructions(kw, sq):
    m = ft.DiceCELoss(**kw)
    assert m.squared_pred is sq
    assert m.sigmoid is (not kw.get("softmax", False)) and m.softmax is kw.get("softmax", False)
    assert m.smooth == kw.get("smooth_nr", 1e-5)


@pytest.mark.parametrize("kw,err", [
    (dict(sigmoid=True, softmax=True), ValueError),
    (dict(include_background=False), NotImplementedError),
    (dict(sigmoid=True, include_background=False), NotImplementedError),
    (dict(to_onehot_y=True), NotImplementedError),
    (dict(sigmoid=True, squared_pred=False), NotImplementedError),
    (dict(smooth_nr=1e-5, smooth_dr=1e-4), NotImplementedError),
    (dict(softmax=True, to_onehot_y=True, smooth_nr=0.0, smooth_dr=1e-5), NotImplementedError),
    (dict(sigmoid=False), NotImplementedError),
])
def test_refused_constructions(kw, err):
    with pytest.raises(err):
        ft.DiceCELoss(**kw)


def test_refused_inputs():
    m = ft.DiceCELoss(softmax=True, to_onehot_y=True)
    with pytest.raises(ValueError, match="one-channel"):
        m(torch.zeros(2, 1, 8), torch.zeros(2, 1, 8, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"\(B, 1, \*S\)"):
        m(torch.zeros(2, 3, 8), torch.zeros(2, 3, 8, dtype=torch.uint8))
    with pytest.raises(ValueError):
        m(torch.zeros(2, 3, 8), torch.zeros(2, 1, 12, dtype=torch.uint8))
    with pytest.raises(ValueError, match="one-channel"):
        ft.DiceCELoss(softmax=True)(torch.zeros(2, 1, 8), torch.zeros(2, 1, 8))
    with pytest.raises(TypeError):
        ft.DiceCELoss(softmax=True, to_onehot_y=True, label_smoothing=0.1)   # not an argument of this class


def test_default_and_explicit_sigmoid_forms_equal_dice_ce_loss_bit_for_bit():
    z, t = L.make_inputs("randn3", 2, 3, 64)
    want = ft.dice_ce_loss(z, t)
    for m in (ft.DiceCELoss(), ft.DiceCELoss(sigmoid=True, squared_pred=True), ft.DiceCELoss(True, True, 1e-5, 1e-5)):
        assert torch.equal(m(z, t), want)
    z1, t1 = L.make_inputs("randn3", 2, 1, 64)
    assert torch.equal(ft.DiceCELoss()(z1, t1), ft.dice_ce_loss(z1, t1))


def test_soft_target_form_runs_composed_silently_on_the_cpu():
    z, y = S.make_inputs("randn3", 2, 4, 40)
    t = F.one_hot(y[:, 0].long(), 4).movedim(-1, 1).float()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = ft.DiceCELoss(softmax=True, to_onehot_y=False, squared_pred=True)(z, t)
    l64, _ = S.reference(z, y, True, True)
    assert abs(got.item() - l64.item()) <= L.LOSS_REL * abs(l64.item()) + L.LOSS_FLOOR


# ---- composed against the reference -------------------------------------------------------------------------------------------
def _labels_as(y, C, kind, seed=0):
    g = torch.Generator().manual_seed(seed)
    if kind == "uint8":
        return y
    if kind == "int64":
        return y.long()
    if kind == "int32":
        return y.int()
    if kind == "float32":
        return y.float()
    if kind == "fraction":                       # a float label truncates toward zero: c + [0, 1) is class c
        return y.float() + torch.rand(y.shape, generator=g) * 0.98
    if kind == "oob":                            # values C and 255 name no class
        r = torch.rand(y.shape, generator=g)
        y = torch.where(r < 0.1, torch.full_like(y, C), y)
        return torch.where(r > 0.9, torch.full_like(y, 255), y)
    if kind == "negative":                       # int64 −1 names no class; float −0.5 truncates to class 0
        return torch.where(torch.rand(y.shape, generator=g) < 0.1, torch.full_like(y.long(), -1), y.long())
    raise KeyError(kind)


@pytest.mark.parametrize("sq,ib", SQ_IB)
@pytest.mark.parametrize("C,shape", [(2, (12,)), (3, (5, 7)), (16, (3, 4, 5))])
@pytest.mark.parametrize("kind", ["uint8", "int64", "int32", "float32", "fraction", "oob", "negative"])
def test_composed_matches_the_reference(sq, ib, C, shape, kind):
    V = 1
    for s in shape:
        V *= s
    z, y = S.make_inputs("randn3", 2, C, V, seed=3)
    z, y = z.reshape(2, C, *shape).double(), _labels_as(y, C, kind).reshape(2, 1, *shape)
    zc = z.clone().requires_grad_(True)
    loss = ft.dice_ce_softmax_loss(zc, y, include_background=ib, squared_pred=sq)
    (g,) = torch.autograd.grad(loss * 1.7, zc)
    l64, g64 = S.reference(z, y, sq, ib, 1.7)
    assert abs(loss.item() - l64.item()) <= 1e-12 * abs(l64.item())
    assert (g - g64).abs().max().item() <= 1e-12 * g64.abs().max().item()
    lm = ft.DiceCELoss(softmax=True, to_onehot_y=True, squared_pred=sq, include_background=ib)(z, y)
    assert torch.equal(lm, loss.detach())
    assert torch.equal(ft.dice_ce_softmax_loss_composed(z, y, include_background=ib, squared_pred=sq), lm)


def test_label_conventions():
    """float −0.5 and 0.9 are class 0, C − 0.5 is class C − 1, C, −1, NaN and 255 name no class: zero one-hot row, zero CE, yet
    counted in the CE mean's B·V"""
    C = 3
    z = torch.randn(1, C, 8, generator=torch.Generator().manual_seed(0)).double()
    yf = torch.tensor([-0.5, 0.9, 2.5, 1.0, 3.0, -1.0, float("nan"), 255.0]).view(1, 1, 8)
    yi = torch.tensor([0, 0, 2, 1, 3, -1, 77, 255]).view(1, 1, 8)
    lf = ft.dice_ce_softmax_loss(z, yf)
    li = ft.dice_ce_softmax_loss(z, yi)
    assert torch.equal(lf, li)
    # by hand: the CE of the four valid voxels over all eight
    logp = torch.log_softmax(z, 1)[0]
    ce = -(logp[0, 0] + logp[0, 1] + logp[2, 2] + logp[1, 3]) / 8
    p = torch.softmax(z, 1)[0]
    t = torch.zeros(C, 8, dtype=torch.float64)
    t[0, 0] = t[0, 1] = t[2, 2] = t[1, 3] = 1
    dice = (1 - (2 * (p * t).sum(1) + 1e-5) / (p.sum(1) + t.sum(1) + 1e-5)).mean()
    assert abs(li.item() - (ce + dice).item()) <= 1e-13


# ---- the closed-form gradient ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sq,ib", SQ_IB)
@pytest.mark.parametrize("regime", ["randn3", "oob_1pct", "absent"])
def test_closed_form_gradient_is_float64_autograd(sq, ib, regime):
    """pins the FORMULA stated in the docstring of factorizer_amd/losses.py — two helpers of softmax_loss_cases against each
    other, no product code: the kernels that evaluate it are held by tests/test_gpu_softmax_loss.py"""
    z, y = S.make_inputs(regime, 2, 5, 400, seed=1)
    _, g64 = S.reference(z, y, sq, ib, 1.7)
    gc = S.closed_form_grad(z, y, sq, ib, 1.7)
    assert (gc - g64).abs().max().item() <= 1e-13 * g64.abs().max().item()


def test_only_the_saturated_regime_needs_the_kink_allowance():
    """the float32 evaluation of the reference holds GRAD_REL of every plane maximum in all regimes but S.KINK's (C = 16)"""
    for regime in S.REGIMES:
        z, y = S.make_inputs(regime, 2, 16, 4096, seed=1)
        zz = S.unshifted(z) if regime == "shift1e4" else z
        _, g64 = S.reference(zz, y, False, True)
        _, g32 = S.reference(z, y, False, True, dtype=torch.float32)
        d, s = L.plane_errors(g32, g64)
        assert bool((d <= L.GRAD_REL * s).all()) is (regime not in S.KINK), regime


# ---- deep supervision -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.uint8, torch.int64, torch.float32])
@pytest.mark.parametrize("St,levels", [((8, 12, 8), [(8, 12, 8), (4, 6, 4), (2, 3, 2)]), ((16, 12), [(16, 12), (8, 4), (5, 5)])])
def test_deep_supervision_with_a_label_map_is_the_sum_of_dense_losses_on_nearest_exact_labels(dt, St, levels):
    g = torch.Generator().manual_seed(5)
    C = 4
    y = torch.randint(0, C, (2, 1, *St), generator=g).to(dt)
    zs = [torch.randn(2, C, *s, generator=g).double() for s in levels]
    base = ft.DiceCELoss(softmax=True, to_onehot_y=True, include_background=False)
    got = ft.DeepSupervisionLoss(base, weight_mode="exp")(zs, y)
    w = losses.ds_weights(len(zs), "exp")
    want = sum(wl * base(z, F.interpolate(y.float(), size=z.shape[2:], mode="nearest-exact").to(dt) if z.shape[2:] != y.shape[2:]
                         else y) for wl, z in zip(w, zs))
    assert torch.equal(got, want)
    # an integer ratio is the strided pick r·i + r//2
    z1 = zs[1]
    r = [a // b for a, b in zip(St, z1.shape[2:])]
    sl = (slice(None), slice(None)) + tuple(slice(k // 2, None, k) for k in r)
    assert torch.equal(base(z1, losses.ds_labels_composed(y, z1.shape[2:])), base(z1, y[sl]))


def test_deep_supervision_with_a_soft_target_is_the_sum_of_dense_losses_on_the_interpolated_target():
    """ft.DiceCELoss(softmax=True) (to_onehot_y=False) takes a (B, C, *S) target: every level is that softmax loss on the
    nearest-exact target — none of them the sigmoid form"""
    g = torch.Generator().manual_seed(6)
    C = 3
    t = F.one_hot(torch.randint(0, C, (2, 16, 8), generator=g), C).movedim(-1, 1).float().contiguous()
    zs = [torch.randn(2, C, *s, generator=g) for s in ((16, 8), (8, 4), (4, 4))]
    base = ft.DiceCELoss(softmax=True, squared_pred=True, include_background=False)
    got = ft.DeepSupervisionLoss(base)(zs, t)
    w = losses.ds_weights(3, "exp")
    want = sum(wl * base(z, t if z.shape[2:] == t.shape[2:] else F.interpolate(t, size=z.shape[2:], mode="nearest-exact"))
               for wl, z in zip(w, zs))
    assert torch.equal(got, want)
    sig = sum(wl * ft.dice_ce_loss(z, losses.ds_target_composed(t, z.shape[2:], torch.float32)) for wl, z in zip(w, zs))
    assert abs(got.item() - sig.item()) > 1e-3          # the sigmoid form of the same levels is another number
    assert losses._ds_level_gate(base, zs[1], t) is not None and losses._ds_level_gate(ft.DiceCELoss(), zs[1], t) is None


def test_deep_supervision_shape_check_of_the_sigmoid_form_stays_strict():
    zs = [torch.zeros(2, 3, 8, 8), torch.zeros(2, 3, 4, 4)]
    with pytest.raises(ValueError, match="deep supervision"):
        ft.deep_supervision_loss(zs, torch.zeros(2, 1, 8, 8), ft.DiceCELoss())
    with pytest.raises(ValueError, match="deep supervision"):   # the class-index form wants ONE label channel
        ft.deep_supervision_loss(zs, torch.zeros(2, 2, 8, 8), ft.DiceCELoss(softmax=True, to_onehot_y=True))
