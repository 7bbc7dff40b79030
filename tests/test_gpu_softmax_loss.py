"""-m gpu: the class-index kernels of csrc/loss.hip (dice_sce_*) behind ft.dice_ce_softmax_loss /
ft.DiceCELoss(softmax=True, to_onehot_y=True) / ft.DeepSupervisionLoss against the independent float64 reference of
tests/softmax_loss_cases.py, each shape the smallest that reaches its seam.  Bounds: the sigmoid kernels' (loss_adamw_cases):
|l − l64| <= LOSS_REL·|l64| + LOSS_FLOOR, the gradient GRAD_REL of max|g64| over the tensor AND over every (b, c) plane.
Every native case asserts that kernels were launched and that no composed device branch (those warn) was taken.

The gradient kernel runs one batch item per blockIdx.y and caps blockIdx.x at 4096 blocks of 1024 voxels: its grid-stride
loop starts past V = 4 Mi voxels per item, whatever B and C (test_past_the_gradient_grid_cap)."""
import functools
import warnings

import pytest
import torch

import factorizer_amd as ft
from factorizer_amd import _native
from factorizer_amd import composed as CO
from factorizer_amd import functional as Fn
import loss_adamw_cases as L
import parity as P
import softmax_loss_cases as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SQ_IB = [(False, True), (False, False), (True, True), (True, False)]
SCALE = 1.7


class Native:
    """the body must launch native kernels and may not take a composed device branch (those warn) — tests/test_gpu_loss.py"""

    def __enter__(self):
        self.n0 = _native.launch_count()
        self.w = warnings.catch_warnings()
        self.w.__enter__()
        warnings.simplefilter("error", RuntimeWarning)
        return self

    def __exit__(self, *exc):
        self.w.__exit__(*exc)
        if exc[0] is None:
            torch.cuda.synchronize()
            assert _native.launch_count() > self.n0, "native kernels were not launched"


def device_loss(z, y, sq, ib, scale=SCALE):
    """(loss, d(scale·loss)/dz) on the device; z, y: CPU (or device) tensors"""
    zd = z.to(DEV).requires_grad_(True)
    with Native():
        loss = ft.dice_ce_softmax_loss(zd, y.to(DEV), include_background=ib, squared_pred=sq)
        (g,) = torch.autograd.grad(loss * scale, zd)
    return loss.detach(), g


def compare(name, regime, z, y, sq, ib, ld, gd, l64, g64, scale=SCALE):
    P.close(f"{name}: loss", ld, l64, rel=L.LOSS_REL, floor=L.LOSS_FLOOR)
    why, k, kp = S.KINK.get(regime), 0.0, None
    if why:
        _, g32 = S.reference(z, y, sq, ib, scale, dtype=torch.float32)     # measured from the REFERENCE in fp32
        k, kp = L.kink(g32, g64)
    gd = gd.detach().cpu()
    P.close(f"{name}: dL/dz", gd, g64, rel=L.GRAD_REL, floor=0.0, extra=k, why=why)
    d, s = L.plane_errors(gd, g64)
    P.note(f"{name}: worst plane", loss_rel_err=abs(ld.item() - l64.item()) / (abs(l64.item()) + 1e-300),
           rel_err_of_plane_max=(d / (s + 1e-300)).max().item(), smallest_plane_max=s.min().item())
    bound = L.GRAD_REL * s + (kp if why else 0.0)
    bad = (d > bound).nonzero()
    assert not len(bad), f"{name}: planes {bad.tolist()} err {d[d > bound].tolist()} > bound {bound[d > bound].tolist()}"


@functools.lru_cache(maxsize=4)
def case(regime, B, C, V, sq, ib, seed=0):
    z, y = S.make_inputs(regime, B, C, V, seed)
    l64, g64 = S.reference(S.unshifted(z) if regime == "shift1e4" else z, y, sq, ib, SCALE)
    return z, y, l64, g64


def run_case(regime, B, C, V, sq, ib, seed=0):
    z, y, l64, g64 = case(regime, B, C, V, sq, ib, seed)
    ld, gd = device_loss(z, y, sq, ib)
    compare(f"sce {regime} ({B},{C},{V}) sq={sq} ib={ib}", regime, z, y, sq, ib, ld, gd, l64, g64)
    return ld, gd


# ---- shapes -------------------------------------------------------------------------------------------------------------------
def chunk_seams():
    """(last one-chunk V, first two-chunk V, a three-chunk V whose `per` is no multiple of 1024 and whose last chunk is
    short), asked from the library"""
    chunks = _native.lib().fz_dice_bce_chunks

    def first_with(n):
        lo, hi = 4, 1 << 24            # smallest multiple of 4 with chunks(V) >= n (chunks is monotonic)
        while lo < hi:
            mid = ((lo + hi) // 2) // 4 * 4
            if chunks(mid) >= n:
                hi = mid
            else:
                lo = mid + 4
        return lo

    two, three = first_with(2), first_with(3) + 4
    per = ((three // 4 + 2) // 3) * 4
    assert chunks(two - 4) == 1 and chunks(two) == 2 and chunks(three) == 3
    assert per % 1024 and three - 2 * per < per
    return two - 4, two, three


@pytest.mark.parametrize("C", [2, 16])
def test_one_float4_per_row(C):
    run_case("randn3", 2, C, 4, False, True)


@pytest.mark.parametrize("sq,ib", SQ_IB)
@pytest.mark.parametrize("which", [0, 1, 2])
def test_chunk_seams(which, sq, ib):
    run_case("randn3", 2, 3, chunk_seams()[which], sq, ib)


@pytest.mark.parametrize("C", list(range(2, 17)))
def test_every_channel_count(C):
    """the exact instances (C = 2, 3, 4, 8, 16) and every padded size of the 8- and 16-slot ones; the kernels that ran are the
    class-index ones"""
    z, y, l64, g64 = case("randn3", 2, C, 4096, C % 2 == 0, C % 3 != 0)
    timer = Fn.KernelTimer()
    Fn.set_timer(timer)
    try:
        ld, gd = device_loss(z, y, C % 2 == 0, C % 3 != 0)
    finally:
        Fn.set_timer(None)
    ran = {k for k in timer.summary() if k.startswith("dice_")}
    assert ran == {"dice_sce_sums", "dice_sce_grad"}, sorted(ran)
    compare(f"sce C={C}", "randn3", z, y, C % 2 == 0, C % 3 != 0, ld, gd, l64, g64)
    with Native():
        lm = ft.DiceCELoss(softmax=True, to_onehot_y=True, squared_pred=C % 2 == 0, include_background=C % 3 != 0)(
            z.to(DEV), y.to(DEV))
    assert torch.equal(lm, ld)


def test_past_the_gradient_grid_cap():
    """V = 4 Mi + 2048 voxels in one item: the last two blocks' worth of voxels is written by the second trip of the loop"""
    run_case("randn3", 1, 2, 4096 * 1024 + 2048, False, True)


@pytest.mark.parametrize("ib", [True, False])
def test_finish_kernel_at_B8_and_framework_finish_at_B9(ib):
    z, y = S.make_inputs("randn3", 9, 3, 4096, seed=2)
    out = {}
    for B in (8, 9):
        l64, g64 = S.reference(z[:B], y[:B], True, ib, SCALE)
        n0 = _native.launch_count()
        ld, gd = device_loss(z[:B], y[:B], True, ib)
        assert _native.launch_count() - n0 == (3 if B == 8 else 2)     # sums, [finish,] gradient
        compare(f"sce finish B={B} ib={ib}", "randn3", z[:B], y[:B], True, ib, ld, gd, l64, g64)
        out[B] = gd
    # the ninth item leaves the first eight planes' coefficients as they are: the gradients differ by the means' 9/8 only
    P.close(f"sce finish ib={ib}: B=9 gradient x 9/8 vs B=8", out[9][:8] * (9.0 / 8.0), out[8], floor=0.0)


@pytest.mark.parametrize("B,C,V", [(2, 5, 4096), (2, 16, 32 ** 3)])
@pytest.mark.parametrize("regime", S.REGIMES)
def test_input_regimes_vs_float64(regime, B, C, V):
    """shift1e4: the float64 reference is evaluated on the UNSHIFTED logits — the result may not depend on the shift"""
    run_case(regime, B, C, V, C == 16, C != 16, seed=1)


# ---- interface ------------------------------------------------------------------------------------------------------------------
def test_label_kinds_give_the_same_bits():
    z, y, l64, g64 = case("oob_1pct", 2, 3, 8192, False, True)
    lu, gu = device_loss(z, y, False, True)
    compare("sce uint8 labels", "oob_1pct", z, y, False, True, lu, gu, l64, g64)
    frac = y.float() + 0.75 * (y < 255).float()          # a float label truncates toward zero
    for yy in (y.long(), y.float(), frac):
        ld, gd = device_loss(z, yy, False, True)
        assert torch.equal(ld, lu) and torch.equal(gd, gu), yy.dtype


def test_spatial_rank_1_2_3_bitwise_equal():
    z, y, l64, g64 = case("randn3", 2, 3, 4096, True, False)
    got = []
    for s in ((4096,), (64, 64), (16, 16, 16)):
        ld, gd = device_loss(z.reshape(2, 3, *s), y.reshape(2, 1, *s), True, False)
        assert gd.shape == (2, 3, *s)
        got.append((ld, gd.reshape(2, 3, 4096)))
    compare("sce rank 1", "randn3", z, y, True, False, got[0][0], got[0][1], l64, g64)
    for ld, gd in got[1:]:
        assert torch.equal(ld, got[0][0]) and torch.equal(gd, got[0][1])


def test_non_contiguous_logits_equal_contiguous():
    g = torch.Generator().manual_seed(6)
    zl = torch.randn(2, 8, 8, 20, 5, generator=g) * 3          # (B, D, H, W, C): a channels-last head output
    y = torch.randint(0, 5, (2, 1, 8, 8, 20), generator=g).to(torch.uint8)
    zd = zl.to(DEV).permute(0, 4, 1, 2, 3).requires_grad_(True)
    assert not zd.is_contiguous()
    with Native():
        ln = ft.dice_ce_softmax_loss(zd, y.to(DEV))
        (gn,) = torch.autograd.grad(ln * SCALE, zd)
    zc = zl.permute(0, 4, 1, 2, 3).contiguous()
    lc, gc = device_loss(zc, y, False, True)
    assert torch.equal(ln, lc) and torch.equal(gn, gc)
    l64, g64 = S.reference(zc, y, False, True, SCALE)
    compare("sce permuted view", "randn3", zc, y, False, True, ln, gn, l64, g64)


def test_bf16_logits_equal_the_fp32_call_on_the_upcast_values():
    z, y = S.make_inputs("randn3", 2, 5, 4096, seed=3)
    zb = z.to(torch.bfloat16)
    l32, g32 = device_loss(zb.float(), y, False, True)
    lb, gb = device_loss(zb, y, False, True)
    assert lb.dtype == torch.float32 and torch.equal(lb, l32)
    assert gb.dtype == torch.bfloat16 and torch.equal(gb, g32.to(torch.bfloat16))   # the cast's backward rounds once
    l64, g64 = S.reference(zb.float(), y, False, True, SCALE)
    compare("sce bf16 values", "randn3", zb.float(), y, False, True, l32, g32, l64, g64)


def test_three_replays_are_bitwise_equal():
    z, y, l64, g64 = case("randn3", 2, 16, 32 ** 3, True, False, 1)
    runs = [device_loss(z, y, True, False) for _ in range(3)]
    for ld, gd in runs[1:]:
        assert torch.equal(ld, runs[0][0]) and torch.equal(gd, runs[0][1])


def test_upstream_gradient_scales():
    z, y = S.make_inputs("randn3", 2, 3, 8192, seed=5)
    g = {}
    for s in (1.0, 1.7, 65536.0):
        l64, g64 = S.reference(z, y, False, True, s)
        ld, g[s] = device_loss(z, y, False, True, s)
        compare(f"sce scale {s:g}", "randn3", z, y, False, True, ld, g[s], l64, g64, s)
    assert torch.equal(g[65536.0], g[1.0] * 65536.0)
    P.close("sce: gradient at scale 1.7 vs 1.7 x gradient at scale 1", g[1.7], g[1.0] * 1.7, floor=0.0)


# ---- deep supervision -----------------------------------------------------------------------------------------------------------
def _slice(y, size):
    r = [a // b for a, b in zip(y.shape[2:], size)]
    return y[(slice(None), slice(None)) + tuple(slice(k // 2, None, k) for k in r)].contiguous()


def _alloc():
    st = torch.cuda.memory_stats(DEV)
    return st["allocation.all.allocated"], st["allocated_bytes.all.allocated"]


@pytest.mark.parametrize("dt", [torch.uint8, torch.int64])
@pytest.mark.parametrize("St,Sl", [((16, 24, 16), (8, 12, 8)), ((16, 16, 16), (4, 4, 4)), ((8, 24, 32), (8, 6, 16)),
                                   ((64, 48), (32, 24)), ((64, 48), (16, 12)), ((4096,), (1024,))])
def test_coarse_level_equals_the_dense_loss_on_the_presliced_label_map(St, Sl, dt):
    """ratios 2 and 4, an anisotropic ratio (1, 4, 2), 2-D, 1-D: the level through the index map and the dense kernels on the
    label map sliced beforehand give the same bits; the level call allocates what the dense call allocates — no tensor of
    the label map's level size (nor any other but the weighted scalar) is created for it"""
    g = torch.Generator().manual_seed(11)
    B, C = 2, 5
    y = torch.randint(0, C + 1, (B, 1, *St), generator=g).to(dt).to(DEV)      # value C: no class
    z1 = torch.randn(B, C, *Sl, generator=g) * 3
    base = ft.DiceCELoss(softmax=True, to_onehot_y=True, squared_pred=True, include_background=False)
    ys = _slice(y, Sl)
    zd = z1.to(DEV).requires_grad_(True)
    torch.cuda.synchronize()
    with Native():
        a0 = _alloc()
        ld = base(zd, ys)
        a1 = _alloc()
        (gd,) = torch.autograd.grad(ld, zd)
    zl = z1.to(DEV).requires_grad_(True)
    timer = Fn.KernelTimer()
    Fn.set_timer(timer)
    try:
        with Native():
            b0 = _alloc()
            ll = ft.deep_supervision_loss([zl], y, base, weights=[0.5])      # the coarse level alone: 0.5 · l_1, exactly
            b1 = _alloc()
            (gl,) = torch.autograd.grad(ll, zl)
    finally:
        Fn.set_timer(None)
    assert {"dice_sce_ds_sums", "dice_sce_ds_grad"} <= set(timer.summary())
    assert torch.equal(ll.detach(), 0.5 * ld.detach()) and torch.equal(gl, 0.5 * gd)
    # one allocation more than the dense call — the scalar 0.5 · l_1, one minimum block — and nothing else
    assert b1[0] - b0[0] == a1[0] - a0[0] + 1, (a0, a1, b0, b1)
    assert (b1[1] - b0[1]) - (a1[1] - a0[1]) <= 512, (a0, a1, b0, b1)
    l64, g64 = S.reference(z1, ys.cpu(), True, False, 1.0)
    compare(f"sce ds {St}->{Sl} {dt}", "randn3", z1, ys.cpu(), True, False, ld.detach(), gd, l64, g64, 1.0)


# ---- composed device branches ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("why,key,B,C,V,zdt,ydt", [
    ("C = 17", "channels", 2, 17, 4096, torch.float32, torch.uint8),
    ("V % 4 != 0", "voxels", 2, 3, 4098, torch.float32, torch.uint8),
    ("float64 logits", "logits", 2, 3, 4096, torch.float64, torch.uint8),
    ("int32 labels", "labels", 2, 3, 4096, torch.float32, torch.int32),
    ("non-contiguous label map", "layout", 2, 3, 4096, torch.float32, torch.uint8)])
def test_composed_device_branch_warns_once_and_matches_float64(why, key, B, C, V, zdt, ydt):
    z, y = S.make_inputs("randn3", B, C, V, seed=7)
    l64, g64 = S.reference(z, y, False, True, SCALE)
    CO._warned.discard("dice_ce_softmax_loss:" + key)
    zd = z.to(DEV).to(zdt).requires_grad_(True)
    yd = y.to(ydt).to(DEV)
    if key == "layout":
        wide = torch.zeros(B, 1, V + 4, dtype=ydt, device=DEV)
        wide[..., :V] = yd
        yd = wide[..., :V]
        assert not yd.is_contiguous()
    n0 = _native.launch_count()
    with pytest.warns(RuntimeWarning, match="no native kernel"):
        ld = ft.dice_ce_softmax_loss(zd, yd)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)      # ... once
        ld2 = ft.dice_ce_softmax_loss(zd, yd)
    (gd,) = torch.autograd.grad(ld * SCALE, zd)
    torch.cuda.synchronize()
    assert _native.launch_count() == n0, "the composed branch launched a native kernel"
    assert torch.equal(ld, ld2)
    compare(f"sce composed on device ({why})", "randn3", z, y, False, True, ld, gd, l64, g64)


def test_deep_supervision_with_a_soft_target_runs_the_softmax_loss_on_every_level():
    """ft.DiceCELoss(softmax=True) with a (B, C, *S) target has no native kernel: a coarse level that the sigmoid level
    kernels would take (C = 3, integer ratio, V % 4 == 0, contiguous fp32 target) must not reach them — it interpolates the
    target and calls the softmax loss, warning once, and equals the CPU sum of the dense losses"""
    import torch.nn.functional as F
    from factorizer_amd import losses
    g = torch.Generator().manual_seed(14)
    C = 3
    t = F.one_hot(torch.randint(0, C, (2, 16, 16, 16), generator=g), C).movedim(-1, 1).float().contiguous()
    zs = [torch.randn(2, C, *s, generator=g) * 3 for s in ((16, 16, 16), (8, 8, 8))]
    base = ft.DiceCELoss(softmax=True, squared_pred=True)
    w = losses.ds_weights(2, "exp")
    want = sum(wl * base(z.double(), (t if z.shape[2:] == t.shape[2:] else F.interpolate(t, size=z.shape[2:], mode="nearest-exact")).double())
               for wl, z in zip(w, zs))
    for k in ("deep_supervision_loss:loss", "dice_ce_softmax_loss:soft"):
        CO._warned.discard(k)
    timer = Fn.KernelTimer()
    Fn.set_timer(timer)
    try:
        with pytest.warns(RuntimeWarning, match="no native deep-supervision level"):
            got = ft.DeepSupervisionLoss(base)([z.to(DEV) for z in zs], t.to(DEV))
    finally:
        Fn.set_timer(None)
    assert not [k for k in timer.summary() if k.startswith("dice_")], sorted(timer.summary())
    assert abs(got.item() - want.item()) <= L.LOSS_REL * abs(want.item()) + L.LOSS_FLOOR


def test_deep_supervision_composed_level_warns_once():
    """a non-integer ratio interpolates the label map (nearest-exact) and calls the dense loss"""
    g = torch.Generator().manual_seed(13)
    y = torch.randint(0, 3, (2, 1, 26, 20), generator=g).to(torch.uint8)
    zs = [torch.randn(2, 3, 26, 20, generator=g), torch.randn(2, 3, 11, 12, generator=g)]
    base = ft.DiceCELoss(softmax=True, to_onehot_y=True)
    want = ft.DeepSupervisionLoss(base)([z.double() for z in zs], y)
    CO._warned.discard("deep_supervision_loss:labels:ratio")
    with pytest.warns(RuntimeWarning, match="no native deep-supervision level"):
        got = ft.DeepSupervisionLoss(base)([z.to(DEV) for z in zs], y.to(DEV))
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        ft.DeepSupervisionLoss(base)([z.to(DEV) for z in zs], y.to(DEV))
    assert abs(got.item() - want.item()) <= L.LOSS_REL * abs(want.item()) + L.LOSS_FLOOR
