"""ft.DeepSupervisionLoss / ft.deep_supervision_loss on the CPU (no GPU needed): the level weights, the target of a coarse
level (nearest-exact = the strided pick for integer ratios, F.interpolate otherwise), the single-input forms, the tiny
num_deep_supr models end to end, and the condition under tests/test_gpu_deep_supervision.py: for every case that file
runs, the fp32 composed evaluation on the CPU is within HALF of the GPU test's bounds against float64 (tests/ds_cases.py),
so the reference alone is inside them."""
import pytest
import torch
import torch.nn.functional as F

import factorizer_amd as ft
from factorizer_amd import losses
import ds_cases as D
import loss_adamw_cases as L


# ---- weights --------------------------------------------------------------------------------------------------------------
def test_weight_modes():
    assert losses.ds_weights(3, "same") == [1.0, 1.0, 1.0]
    assert losses.ds_weights(6, "exp") == [1.0, 0.5, 0.25, 0.125, 0.0625, 0.0625]      # the 0.0625 floor at the sixth level
    assert losses.ds_weights(4, "two") == [1.0, 0.5, 0.5, 0.5]
    assert losses.ds_weights(1, "two") == [1.0]


def test_explicit_weights_and_their_fallback():
    assert losses.ds_weights(2, "exp", [0.3, 0.2, 0.1]) == [0.3, 0.2]
    assert losses.ds_weights(3, "exp", [0.3, 0.2, 0.1]) == [0.3, 0.2, 0.1]
    assert losses.ds_weights(4, "exp", [0.3, 0.2, 0.1]) == [1.0, 0.5, 0.25, 0.125]      # too few: the mode decides
    assert losses.ds_weights(4, "two", (0.3,)) == [1.0, 0.5, 0.5, 0.5]


def test_bad_weight_mode_raises():
    z = [torch.randn(1, 2, 8), torch.randn(1, 2, 4)]
    t = torch.rand(1, 2, 8)
    with pytest.raises(ValueError, match="weight_mode"):
        ft.DeepSupervisionLoss(ft.DiceCELoss(), weight_mode="linear")
    with pytest.raises(ValueError, match="weight_mode"):
        ft.deep_supervision_loss(z, t, loss=ft.DiceCELoss(), weight_mode="linear")
    with pytest.raises(ValueError, match="weight_mode"):
        ft.deep_supervision_loss(z[0], t, loss=ft.DiceCELoss(), weight_mode="")


@pytest.mark.parametrize("mode,explicit", [("same", None), ("exp", None), ("two", None), ("exp", (0.7, 0.2, 0.1))])
def test_total_is_the_weighted_sum_of_the_level_losses(mode, explicit):
    zs, t = D.make_case("3d", 2, 3)
    w = D.weights_of(mode, len(zs), explicit)
    base = ft.DiceCELoss()
    got = ft.DeepSupervisionLoss(base, weight_mode=mode, weights=explicit)(zs, t)
    want = sum(wl * base(z, D.slice_target(t, z.shape[2:])) for wl, z in zip(w, zs))
    assert got.dtype == torch.float32 and got.shape == ()
    assert abs(got.item() - want.item()) <= 3 * 2.0 ** -23 * want.item()
    other = ft.deep_supervision_loss(zs, t, loss=lambda a, b: (a - b).square().mean(), weight_mode=mode, weights=explicit)
    want = sum(wl * (z - D.slice_target(t, z.shape[2:])).square().mean() for wl, z in zip(w, zs))
    assert abs(other.item() - want.item()) <= 3 * 2.0 ** -23 * want.item()


# ---- the target of a level ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.uint8, torch.bool])
@pytest.mark.parametrize("St,S", [((64,), (16,)), ((12,), (4,)), ((32, 24), (8, 12)), ((16, 12, 8), (4, 3, 2)),
                                  ((12, 3, 16), (4, 3, 4))])
def test_composed_target_is_the_strided_pick(dt, St, S):
    g = torch.Generator().manual_seed(3)
    t = (torch.rand(2, 3, *St, generator=g) > 0.5).to(dt)
    got = losses.ds_target_composed(t, S, torch.float32)
    assert got.dtype == torch.float32 and torch.equal(got, D.slice_target(t, S).float())
    assert losses.ds_target_composed(t, St, torch.float32) is t        # at its own size: the target itself, untouched


def test_nearest_exact_is_r_i_plus_half_r_for_integer_ratios_only():
    """what the level reader of csrc/loss.hip relies on: torch's nearest-exact picks r·i + r//2 for every integer ratio, and NOT
    floor((2i+1)·S_t / (2·S_l)) for the others (first at 26 -> 11) — those are never computed natively"""
    for r in range(1, 17):
        for S in range(1, 129):
            src = torch.arange(r * S, dtype=torch.float32).reshape(1, 1, -1)
            got = F.interpolate(src, size=S, mode="nearest-exact").reshape(-1).long()
            assert torch.equal(got, r * torch.arange(S) + r // 2), (r, S)
    src = torch.arange(26, dtype=torch.float32).reshape(1, 1, -1)
    got = F.interpolate(src, size=11, mode="nearest-exact").reshape(-1).long()
    assert not torch.equal(got, ((2 * torch.arange(11) + 1) * 26) // 22)
    assert losses._ds_level_gate(ft.DiceCELoss(), torch.zeros(1, 1, 11, 4), torch.zeros(1, 1, 26, 8))[0] == "ratio"
    assert losses._ds_level_gate(ft.DiceCELoss(), torch.zeros(1, 1, 13, 4), torch.zeros(1, 1, 26, 8)) is None


def test_composed_target_keeps_soft_values():
    t = torch.rand(1, 2, 12, 8, generator=torch.Generator().manual_seed(4))
    assert torch.equal(losses.ds_target_composed(t, (4, 4), torch.float32), D.slice_target(t, (4, 4)))
    tb = t.to(torch.bfloat16)
    assert torch.equal(losses.ds_target_composed(tb, (4, 4), torch.float32), D.slice_target(tb, (4, 4)).float())


@pytest.mark.parametrize("St,S", [((10,), (4,)), ((26,), (11,)), ((26, 10), (11, 4))])
@pytest.mark.parametrize("dt", [torch.float32, torch.uint8, torch.bool])
def test_non_integer_ratios_are_torch_nearest_exact(St, S, dt):
    g = torch.Generator().manual_seed(5)
    t = (torch.rand(2, 2, *St, generator=g) > 0.5).to(dt)
    z = [torch.randn(2, 2, *St, generator=g), torch.randn(2, 2, *S, generator=g)]
    tl = F.interpolate(t.float(), size=S, mode="nearest-exact")
    assert torch.equal(losses.ds_target_composed(t, S, torch.float32), tl)
    base = ft.DiceCELoss()
    got = ft.deep_supervision_loss(z, t, loss=base, weight_mode="same")
    assert torch.equal(got, base(z[0], t.float()) + base(z[1], tl))


# ---- single inputs, the stacked form --------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("mode", ["same", "exp", "two"])
def test_tensor_and_one_entry_list_are_the_base_loss(C, mode):
    g = torch.Generator().manual_seed(6)
    z = torch.randn(2, C, 8, 6, 4, generator=g).requires_grad_(True)
    t = (torch.rand(2, C, 8, 6, 4, generator=g) > 0.5).float()
    base = ft.DiceCELoss()
    want = base(z, t)
    (gw,) = torch.autograd.grad(want, z)
    ds = ft.DeepSupervisionLoss(base, weight_mode=mode)
    for inp in (z, [z], (z,)):
        got = ds(inp, t)
        (gg,) = torch.autograd.grad(got, z)
        assert torch.equal(got, want) and torch.equal(gg, gw)
    assert torch.equal(ft.deep_supervision_loss(z, t), want)          # the default base loss is ft.DiceCELoss()
    assert torch.equal(ft.deep_supervision_loss([z], t, weights=[0.25]), 0.25 * want)


def test_stacked_form_raises():
    z = torch.randn(2, 3, 2, 8, 8)          # (B, L, C, H, W) against a (B, C, H, W) target
    t = torch.rand(2, 2, 8, 8)
    with pytest.raises(ValueError, match="stacked"):
        ft.DeepSupervisionLoss(ft.DiceCELoss())(z, t)
    with pytest.raises(ValueError):
        ft.deep_supervision_loss([torch.randn(2, 2, 8, 8), torch.randn(2, 3, 4, 4)], t)   # a level's channels against the target's
    with pytest.raises(ValueError):
        ft.deep_supervision_loss([], t)


# ---- the num_deep_supr networks --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,shapes", [
    ("factorizer", [(1, 3, 16, 16, 16), (1, 3, 8, 8, 8), (1, 3, 4, 4, 4)]),
    ("deconver2d", [(2, 1, 32, 32), (2, 1, 16, 16)]),
    ("one_head", [(1, 3, 16, 16, 16)])])
def test_tiny_models_train_through_the_loss(which, shapes):
    torch.manual_seed(0)
    if which == "deconver2d":
        model, x = D.tiny_deconver2d(), torch.randn(2, 3, 32, 32)
    else:
        model = D.tiny_factorizer(num_deep_supr=True if which == "one_head" else 3)
        x = torch.rand(1, 2, 16, 16, 16)
    t = torch.rand(shapes[0]) > 0.5                                    # a bool mask, as a label pipeline holds it
    for mod in (model.train(), model.eval()):                         # eval() returns the list too
        out = mod(x)
        assert isinstance(out, list) and [tuple(o.shape) for o in out] == shapes
    out = model.train()(x)
    loss = ft.DeepSupervisionLoss(ft.DiceCELoss())(out, t)
    assert loss.shape == () and torch.isfinite(loss)
    loss.backward()
    assert len(model.heads) == len(shapes)
    for j, head in enumerate(model.heads):
        for n, p in head.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, (j, n)
    if which == "one_head":
        assert torch.equal(loss, ft.DiceCELoss()(out[0], t))


# ---- the condition under the GPU tests ------------------------------------------------------------------------------------
def _composed_fp32(zs, t, mode="exp", scale=D.SCALE):
    zr = [z.clone().requires_grad_(True) for z in zs]
    loss = ft.deep_supervision_loss(zr, t, loss=ft.DiceCELoss(), weight_mode=mode)
    return loss.detach(), torch.autograd.grad(loss * scale, zr)


@pytest.mark.parametrize("geom,B,C", D.MATRIX)
def test_composed_fp32_within_half_of_the_gpu_bounds_shape_matrix(geom, B, C):
    zs, t = D.make_case(geom, B, C)
    w = D.weights_of("exp", len(zs))
    loss, grads = _composed_fp32(zs, t)
    D.check(f"cpu fp32 {geom} B={B} C={C}", zs, t, w, loss, grads, frac=0.5, ref=D.case_reference(geom, B, C))


@pytest.mark.parametrize("C,regime", D.REGIME_CASES)
def test_composed_fp32_within_half_of_the_gpu_bounds_regimes(C, regime):
    """KINK regimes (loss_adamw_cases.KINK: ("bce", "saturated")) carry their kink term, as in tests/test_gpu_loss.py"""
    zs, t = D.make_case("regimes", 2, C, regime, 1)
    w = D.weights_of("exp", len(zs))
    loss, grads = _composed_fp32(zs, t)
    D.check(f"cpu fp32 regime {regime} C={C}", zs, t, w, loss, grads, regime=regime, frac=0.5,
            ref=D.case_reference("regimes", 2, C, regime, 1))


def test_kink_regimes_are_the_listed_ones():
    assert set(L.KINK) == {("bce", "saturated")}
    for C, regime in D.REGIME_CASES:
        if (D.kind_of(C), regime) in L.KINK:
            zs, t = D.make_case("regimes", 2, C, regime, 1)
            assert all(((2 * D.slice_target(t, z.shape[2:]) - 1) * z >= 20).all() for z in zs)   # saturated AND correct, per level


# ---- the C ABI's host-side checks (no device is touched) --------------------------------------------------------------------
def test_host_side_argument_checks_of_the_level_entry_points():
    from factorizer_amd import _native
    lib = _native.lib()
    E_ARG, E_SHAPE, E_UNSUPPORTED = -4, -1, -2
    p8 = 8   # a non-null pointer value the host code never dereferences
    ok = (16, 12, 8, 8, 6, 4)
    assert lib.fz_dice_ce_ds_sums(None, p8, p8, 2, 3, *ok, _native.SEG_U8, None) == E_ARG
    assert lib.fz_dice_bce_ds_sums(p8, None, p8, 2, *ok, _native.SEG_U8, None) == E_ARG
    for geom, word in (((16, 12, 8, 8, 5, 4), b"multiple"), ((16, 12, 8, 0, 6, 4), b"positive"), ((6, 6, 6, 3, 3, 3), b"multiple of 4"),
                       ((16, 12, 8, 8, 6, 4, 7), b"kind")):
        geom, kind = geom[:6], (geom[6] if len(geom) > 6 else _native.SEG_F32)
        assert lib.fz_dice_ce_ds_sums(p8, p8, p8, 2, 3, *geom, kind, None) == E_SHAPE and word in lib.fz_last_error_string()
        assert lib.fz_dice_ce_ds_grad(p8, p8, p8, p8, 2, 3, *geom, kind, 0.5, 0.5, None, None) == E_SHAPE
        assert lib.fz_dice_bce_ds_sums(p8, p8, p8, 2, *geom, kind, None) == E_SHAPE
        assert lib.fz_dice_bce_ds_grad(p8, p8, p8, p8, 2, *geom, kind, 0.5, 0.5, None, None) == E_SHAPE
    for C in (1, 9):
        assert lib.fz_dice_ce_ds_sums(p8, p8, p8, 2, C, *ok, _native.SEG_BF16, None) == E_UNSUPPORTED
        assert lib.fz_dice_ce_ds_grad(p8, p8, p8, p8, 2, C, *ok, _native.SEG_BF16, 0.5, 0.5, None, None) == E_UNSUPPORTED
    assert losses.ds_level_launches(2, 3) == 2 and losses.ds_level_launches(9, 3) == 1 and losses.ds_level_launches(2, 1) == 1
    assert losses.ds_level_launches(2, 3, backward=True) == losses.ds_level_launches(9, 1, backward=True) == 1
