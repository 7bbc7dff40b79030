"""-m gpu: the level kernels of csrc/loss.hip behind ft.DeepSupervisionLoss / ft.deep_supervision_loss against the float64 reference of
tests/ds_cases.py (strided slices of the target, then the composed loss), at the smallest shapes at which the index map
can go wrong: 1-D, 2-D and 3-D levels, ratios 1 .. 4 mixed over the axes, level rows shorter than the 4 elements a thread
walks, the kernel finish at B <= 8 and the framework finish at B = 9, one chunk and two.  Bounds: ds_cases.check."""
import warnings

import pytest
import torch
import torch.nn.functional as F

import factorizer_amd as ft
from factorizer_amd import _native, losses
from factorizer_amd import composed as CO
from factorizer_amd import functional as Fn
import ds_cases as D
import loss_adamw_cases as L
import parity as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -8   # bf16 unit roundoff, as in tests/test_gpu_loss.py


def device_run(zs, t, scale=D.SCALE, mode="exp", weights=None, strict=True, loss=None):
    """(total loss, [d(scale·loss)/dz_l], native launches forward, backward, kernel names); zs, t: CPU tensors.  strict: no
    composed device branch may be taken (those warn)"""
    zd = [z.to(DEV).requires_grad_(True) for z in zs]
    td = t.to(DEV) if t.device.type == "cpu" else t
    timer = Fn.KernelTimer()
    Fn.set_timer(timer)
    try:
        with warnings.catch_warnings():
            if strict:
                warnings.simplefilter("error", RuntimeWarning)
            torch.cuda.synchronize()
            n0 = _native.launch_count()
            out = ft.DeepSupervisionLoss(loss or ft.DiceCELoss(), weight_mode=mode, weights=weights)(zd, td)
            n1 = _native.launch_count()
            grads = torch.autograd.grad(out * scale, zd)
            torch.cuda.synchronize()
            n2 = _native.launch_count()
    finally:
        Fn.set_timer(None)
    return out.detach(), grads, n1 - n0, n2 - n1, set(timer.summary())


def dense_launches(B, C, S):
    """(forward, backward) native launches of ft.DiceCELoss on one dense level, counted"""
    z = torch.zeros(B, C, *S, device=DEV, requires_grad=True)
    n0 = _native.launch_count()
    out = ft.DiceCELoss()(z, torch.zeros(B, C, *S, device=DEV))
    n1 = _native.launch_count()
    torch.autograd.grad(out, z)
    torch.cuda.synchronize()
    return n1 - n0, _native.launch_count() - n1


def ds_names(C):
    return {"dice_bce_ds_sums", "dice_bce_ds_grad"} if C == 1 else {"dice_ce_ds_sums", "dice_ce_ds_grad"}


# ---- the shape matrix -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom,B,C", D.MATRIX)
def test_shape_matrix_vs_float64(geom, B, C):
    zs, t = D.make_case(geom, B, C)
    w = D.weights_of("exp", len(zs))
    loss, grads, nf, nb, ran = device_run(zs, t)
    assert ds_names(C) <= ran, sorted(ran)
    D.check(f"ds {geom} B={B} C={C}", zs, t, w, loss, grads, ref=D.case_reference(geom, B, C))
    for z, g in zip(zs, grads):
        assert g.shape == z.shape and g.dtype == torch.float32


# ---- sampling offsets ---------------------------------------------------------------------------------------------------------
def _level_only(z1, t, St):
    """loss and gradient of the coarse level alone: weights (0, 1) over a zero level 0 (0·l_0 + 1·l_1 = l_1 exactly)"""
    z0 = torch.zeros(z1.shape[0], z1.shape[1], *St)
    loss, grads, *_ = device_run([z0, z1], t, scale=1.0, weights=[0.0, 1.0])
    return loss, grads[1]


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("ratios", [(2, 1, 1), (1, 2, 1), (1, 1, 2), (3, 1, 1), (1, 3, 1), (1, 1, 3), (4, 1, 1), (1, 4, 1),
                                    (1, 1, 4), (2, 3, 4), (4, 2, 3)])
def test_sampled_positions_are_r_i_plus_half_r(ratios, C):
    """a target that is 1 exactly at the positions r·i + r//2 and 0 elsewhere IS an all-ones target to the level, bit for
    bit, and its complement an all-zeros one: any other offset on any axis reads a 0 (resp. a 1) and changes the bits"""
    S = (4, 3, 2)      # level rows of 2 elements: a thread's 4 elements span two rows and, every third time, two slices
    St = tuple(s * r for s, r in zip(S, ratios))
    z1 = torch.randn(2, C, *S, generator=torch.Generator().manual_seed(11)) * 3
    hit = torch.zeros(2, C, *St)
    hit[(slice(None), slice(None)) + tuple(slice(r // 2, None, r) for r in ratios)] = 1.0
    assert hit.sum().item() == 2 * C * D.prod(S)
    l1, g1 = _level_only(z1, torch.ones(2, C, *St), St)
    l0, g0 = _level_only(z1, torch.zeros(2, C, *St), St)
    assert not torch.equal(l1, l0)
    lh, gh = _level_only(z1, hit, St)
    lc, gc = _level_only(z1, 1.0 - hit, St)
    assert torch.equal(lh, l1) and torch.equal(gh, g1)
    assert torch.equal(lc, l0) and torch.equal(gc, g0)


@pytest.mark.parametrize("geom,B,C", [("3d", 2, 3), ("3d", 9, 2), ("2d", 2, 1), ("mixed_1_2_4", 1, 8), ("two_chunks", 1, 2)])
def test_sampled_level_equals_the_dense_kernels_on_the_sliced_target(geom, B, C):
    """the per-voxel arithmetic, the chunking and the order of the sums are csrc/loss.hip's: a level through the index map and
    the same level through ft.DiceCELoss on a target sliced beforehand give the same bits"""
    zs, t = D.make_case(geom, B, C)
    St = zs[0].shape[2:]
    for z in zs[1:]:
        ls, gs = _level_only(z, t, St)
        zd = z.to(DEV).requires_grad_(True)
        ld = ft.DiceCELoss()(zd, D.slice_target(t, z.shape[2:]).contiguous().to(DEV))
        (gd,) = torch.autograd.grad(ld, zd)
        assert torch.equal(ls, ld) and torch.equal(gs, gd), (geom, tuple(z.shape))


@pytest.mark.parametrize("C,St", [(2, (2048, 1280, 1024)), (1, (2048, 1280, 1024))])
def test_target_offsets_past_2_to_31(C, St):
    """a uint8 target of 2.5 Gi elements per (b, c) plane: the offsets inside a plane pass 2^31 from z = 1638 on and 2^32 in
    the second channel, so an offset held in 32 bits reads another element.  Both levels are coarse (ratios 128 and 256); the
    target is 0 except at the sampled positions, which carry each level's own random 0 / 1 target — a read anywhere else
    sees 0 and fails the float64 bounds.  Nothing of the target's size exists on the host or in fp32."""
    levels = [(16, 10, 8), (8, 5, 4)]
    g = torch.Generator().manual_seed(17)
    zs = [torch.randn(1, C, *S, generator=g) * 3 for S in levels]
    tls = [(torch.rand(1, C, *S, generator=g) > 0.5).to(torch.uint8) for S in levels]
    t = torch.zeros(1, C, *St, dtype=torch.uint8, device=DEV)
    for S, tl in zip(levels, tls):
        r = [a // b for a, b in zip(St, S)]
        t[:, :, r[0] // 2::r[0], r[1] // 2::r[1], r[2] // 2::r[2]] = tl.to(DEV)      # (128·i + 64 and 256·i + 128 never meet)
    assert t[0, C - 1, St[0] - 64, St[1] - 64, St[2] - 64].item() == tls[0][0, C - 1, -1, -1, -1].item()
    try:
        loss, grads, _, _, ran = device_run(zs, t)
    finally:
        del t
        torch.cuda.empty_cache()
    assert ds_names(C) <= ran
    w = D.weights_of("exp", 2)
    ref = [L.reference(D.kind_of(C), z, tl.double(), wl * D.SCALE) for z, tl, wl in zip(zs, tls, w)]
    l64s = [r[0] for r in ref]
    assert abs(loss.item() - sum(wl * l.item() for wl, l in zip(w, l64s))) <= D.loss_bound(l64s, w)
    for l, (gd, r) in enumerate(zip(grads, ref)):
        P.close(f"ds 2^31 C={C} level {l} dL/dz", gd, r[1], rel=L.GRAD_REL, floor=0.0)
        d, s = L.plane_errors(gd, r[1])
        assert (d <= L.GRAD_REL * s).all()


# ---- target types -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom,C", [("3d", 3), ("2d", 1), ("ratio3", 2)])
def test_target_types_give_the_same_bits(geom, C):
    zs, t = D.make_case(geom, 2, C)
    lf, gf, *_ = device_run(zs, t)
    for dt in (torch.uint8, torch.bool, torch.bfloat16):
        ld, gd, _, _, ran = device_run(zs, t.to(dt))
        assert ds_names(C) <= ran
        assert torch.equal(ld, lf) and all(torch.equal(a, b) for a, b in zip(gd, gf)), dt


@pytest.mark.parametrize("C", [3, 1])
def test_non_contiguous_target_equals_its_contiguous_copy(C):
    """a label cut out of a wider one without a copy: outside the native gate (the index map reads a dense target), so its
    coarse levels interpolate and run the dense kernels — same values, same bits (see above), one warning"""
    zs, t = D.make_case("3d", 2, C)
    wide = torch.ones(*t.shape[:-1], t.shape[-1] + 3, dtype=torch.uint8)
    wide[..., :t.shape[-1]] = t.to(torch.uint8)
    tl = wide.to(DEV)[..., :t.shape[-1]]
    assert not tl.is_contiguous() and torch.equal(tl.cpu(), t.to(torch.uint8))
    CO._warned.discard("deep_supervision_loss:target")
    with pytest.warns(RuntimeWarning, match="no native deep-supervision level"):
        ln, gn, _, _, ran = device_run(zs, tl, strict=False)
    assert not (ds_names(C) & ran)
    lc, gc, *_ = device_run(zs, t.to(torch.uint8))
    assert torch.equal(ln, lc) and all(torch.equal(a, b) for a, b in zip(gn, gc))


# ---- input regimes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,regime", D.REGIME_CASES)
def test_input_regimes_vs_float64(C, regime):
    zs, t = D.make_case("regimes", 2, C, regime, 1)
    w = D.weights_of("exp", len(zs))
    loss, grads, _, _, ran = device_run(zs, t)
    assert ds_names(C) <= ran
    D.check(f"ds regime {regime} C={C}", zs, t, w, loss, grads, regime=regime, ref=D.case_reference("regimes", 2, C, regime, 1))


# ---- interface ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [3, 1])
def test_bf16_logits(C):
    """bf16 logits are evaluated in fp32, per level: the loss is that of the same values held in fp32, bit for bit; every
    gradient comes back in bf16, one rounding away from the fp32 gradient (bound 2 x u = 2^-8, as tests/test_gpu_loss.py)"""
    zs, t = D.make_case("3d", 2, C, "randn3", 3)
    zb = [z.to(torch.bfloat16) for z in zs]
    l32, g32, *_ = device_run([z.float() for z in zb], t.to(torch.uint8))
    lb, gb, _, _, ran = device_run(zb, t.to(torch.uint8))
    assert ds_names(C) <= ran
    assert lb.dtype == torch.float32 and torch.equal(lb, l32)
    for l, (a, b) in enumerate(zip(gb, g32)):
        assert a.dtype == torch.bfloat16
        P.close(f"ds C={C} level {l}: bf16 gradient vs fp32 gradient", a.float(), b, rel=2 * U, floor=0.0,
                why="bf16 storage: the gradient is rounded to bf16 once, bound 2 x u = 2^-8 as in test_gpu_bf16.py")
    w = D.weights_of("exp", len(zs))
    l64s, _, l64 = D.reference([z.float() for z in zb], t, w)
    assert abs(lb.item() - l64) <= D.loss_bound(l64s, w)


@pytest.mark.parametrize("mode,explicit", [("same", None), ("exp", None), ("two", None), ("exp", (0.7, 0.2, 0.1)),
                                           ("two", (0.7, 0.2))])
def test_weight_modes_vs_float64(mode, explicit):
    zs, t = D.make_case("3d", 2, 3)
    w = D.weights_of(mode, len(zs), explicit)
    loss, grads, *_ = device_run(zs, t, mode=mode, weights=explicit)
    D.check(f"ds weights {mode} {explicit}", zs, t, w, loss, grads)


@pytest.mark.parametrize("C", [3, 1])
def test_upstream_gradient_scales(C):
    zs, t = D.make_case("2d", 2, C)
    _, g1, *_ = device_run(zs, t, scale=1.0)
    _, g17, *_ = device_run(zs, t, scale=1.7)
    _, g64k, *_ = device_run(zs, t, scale=65536.0)
    for l, (a, b, c) in enumerate(zip(g1, g17, g64k)):
        P.close(f"ds C={C} level {l}: gradient at scale 1.7 vs 1.7 x gradient at scale 1", b, a * 1.7, rel=L.GRAD_REL, floor=0.0)
        assert torch.equal(c, a * 65536.0)       # a power of two: exactly linear


@pytest.mark.parametrize("geom,B,C", [("3d", 2, 3), ("3d", 9, 3), ("2d", 2, 1), ("1d", 8, 8), ("mixed_1_2_4", 9, 1)])
def test_launch_counts(geom, B, C):
    """level 0 launches what ft.DiceCELoss launches; every sampled level losses.ds_level_launches, and its own kernels"""
    zs, t = D.make_case(geom, B, C)
    df, db = dense_launches(B, C, zs[0].shape[2:])
    _, _, nf, nb, ran = device_run(zs, t.to(torch.uint8))
    nl = len(zs) - 1
    assert nf == df + nl * losses.ds_level_launches(B, C), (nf, df)
    assert nb == db + nl * losses.ds_level_launches(B, C, backward=True), (nb, db)
    assert losses.ds_level_launches(B, C) == df and losses.ds_level_launches(B, C, backward=True) == db   # a level costs a dense one
    assert ds_names(C) <= ran


@pytest.mark.parametrize("St,S,C", [((26, 8), (11, 4), 3), ((20,), (8,), 1)])
def test_non_integer_ratio_level_is_composed_warns_once_and_meets_the_bounds(St, S, C):
    """26 -> 11 is the first extent at which the integer formula and torch's nearest-exact disagree: such a level adds no launch
    of the level kernels of csrc/loss.hip — it interpolates the target (framework kernels) and runs the dense loss kernels on the result"""
    g = torch.Generator().manual_seed(13)
    zs = [torch.randn(2, C, *St, generator=g) * 3, torch.randn(2, C, *S, generator=g) * 3]
    t = (torch.rand(2, C, *St, generator=g) > 0.5).float()
    CO._warned.discard("deep_supervision_loss:ratio")
    with pytest.warns(RuntimeWarning, match="not an integer ratio"):
        loss, grads, nf, nb, ran = device_run(zs, t, strict=False)
    loss2, grads2, nf2, nb2, ran2 = device_run(zs, t)             # ... once: strict turns a second warning into an error
    assert torch.equal(loss, loss2) and not any("_ds_" in k for k in ran | ran2)
    (f0, b0), (f1, b1) = dense_launches(2, C, St), dense_launches(2, C, S)
    assert (nf, nb) == (nf2, nb2) == (f0 + f1, b0 + b1)
    w = D.weights_of("exp", 2)
    kind = D.kind_of(C)
    t64 = [t.double(), F.interpolate(t.double(), size=S, mode="nearest-exact")]
    ref = [L.reference(kind, z, tl, wl * D.SCALE) for z, tl, wl in zip(zs, t64, w)]
    l64s = [r[0] for r in ref]
    assert abs(loss.item() - sum(wl * l.item() for wl, l in zip(w, l64s))) <= D.loss_bound(l64s, w)
    for l, (gd, r) in enumerate(zip(grads, ref)):
        P.close(f"ds non-integer {St}->{S} level {l} dL/dz", gd, r[1], rel=L.GRAD_REL, floor=0.0)
        d, s = L.plane_errors(gd, r[1])
        assert (d <= L.GRAD_REL * s).all()


def test_other_base_loss_is_composed_on_the_device():
    zs, t = D.make_case("2d", 2, 3)
    CO._warned.discard("deep_supervision_loss:loss")
    with pytest.warns(RuntimeWarning, match="is not ft.DiceCELoss"):
        loss, grads, nf, nb, ran = device_run(zs, t, strict=False, loss=ft.dice_bce_loss)
    assert not any("_ds_" in k for k in ran)
    want = sum(wl * ft.dice_bce_loss(z.to(DEV), D.slice_target(t, z.shape[2:]).contiguous().to(DEV))
               for wl, z in zip(D.weights_of("exp", len(zs)), zs))
    assert torch.equal(loss, want)


def test_three_replays_are_bitwise_equal():
    zs, t = D.make_case("two_chunks", 1, 2)
    runs = [device_run(zs, t.to(torch.bool)) for _ in range(3)]
    for ld, gd, *_ in runs[1:]:
        assert torch.equal(ld, runs[0][0]) and all(torch.equal(a, b) for a, b in zip(gd, runs[0][1]))


def test_tensor_and_one_entry_list_launch_what_the_base_loss_launches():
    zs, t = D.make_case("3d", 2, 3)
    z = zs[0].to(DEV).requires_grad_(True)
    td = t.to(DEV)
    base = ft.DiceCELoss()
    n0 = _native.launch_count()
    want = base(z, td)
    n1 = _native.launch_count()
    for inp in (z, [z]):
        m0 = _native.launch_count()
        got = ft.DeepSupervisionLoss(base)(inp, td)
        assert _native.launch_count() - m0 == n1 - n0 and torch.equal(got, want)
        assert type(got.grad_fn).__name__ == type(want.grad_fn).__name__


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def _composed_on_device(out, t, w):
    return sum(wl * losses.dice_ce_loss_composed(z.float(), losses.ds_target_composed(t, z.shape[2:], torch.float32).float())
               for wl, z in zip(w, out))


@pytest.mark.parametrize("which", ["factorizer", "deconver2d"])
def test_models_train_through_the_native_levels(which):
    from factorizer_amd import pointwise as PW
    torch.manual_seed(0)
    if which == "factorizer":
        model = D.tiny_factorizer((32, 64, 128), (32, 32, 32)).to(DEV)
        x, shapes = torch.rand(1, 2, 32, 32, 32, device=DEV), [(1, 3, 32, 32, 32), (1, 3, 16, 16, 16), (1, 3, 8, 8, 8)]
    else:
        model = D.tiny_deconver2d((32, 64, 128)).to(DEV)
        x, shapes = torch.randn(2, 3, 64, 64, device=DEV), [(2, 1, 64, 64), (2, 1, 32, 32)]
    t = torch.rand(shapes[0], device=DEV) > 0.5
    crit = ft.DeepSupervisionLoss(ft.DiceCELoss())
    heads = [p for h in model.heads for p in h.parameters()]
    timer = Fn.KernelTimer()
    Fn.set_timer(timer)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            out = model(x)
            assert [tuple(o.shape) for o in out] == shapes
            loss = crit(out, t)
            got = torch.autograd.grad(loss, heads, retain_graph=True)
    finally:
        Fn.set_timer(None)
    assert ds_names(shapes[0][1]) <= set(timer.summary())
    want = torch.autograd.grad(_composed_on_device(out, t, D.weights_of("exp", len(out))), heads)
    for j, (a, b) in enumerate(zip(got, want)):
        assert torch.isfinite(a).all() and a.abs().max() > 0
        P.close(f"{which}: head parameter {j} gradient, native levels vs composed loss", a, b, rel=L.GRAD_REL, floor=0.0)
    del out, loss, got, want
    try:
        opt = ft.FlatAdamW(model, lr=1e-3)                        # default: deferred finishes
        opt.zero_grad()
        loss = crit(model(x), t)
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
    finally:
        PW.defer_finishes(False)
    assert torch.isfinite(loss).item() and all(torch.isfinite(p).all() for p in model.parameters())
