"""-m gpu: csrc/loss.hip behind ft.dice_ce_loss / ft.dice_bce_loss / ft.DiceCELoss against the composed form evaluated on the
CPU in FLOAT64, at training sizes: one chunk and many, the grid-stride loops past the 4096-block cap, the finish kernel at
B = 8 and the ATen finish at B = 9, every channel count, and the numerical regimes a training run produces
(tests/loss_adamw_cases.py).  The loss is held to |l − l64| ≤ 1e-5·|l64| + 1e-6, the gradient to 1e-4 of max|g64| over the
tensor AND over every (b, c) plane on its own (an error confined to a small-gradient plane — an empty one — is invisible
under the global maximum).  Every case asserts that native kernels ran and that no composed device branch was taken."""
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

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FN = {"ce": ft.dice_ce_loss, "bce": ft.dice_bce_loss}
V128 = 128 ** 3
U = 2.0 ** -8   # bf16 unit roundoff, as in tests/test_gpu_bf16.py


class Native:
    """the body must launch native kernels and may not take a composed-ATen device branch (those warn)"""

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


def device_loss(kind, z, t, scale=1.0, fn=None):
    """(loss, d(scale·loss)/dz) on the device; z, t: CPU tensors of any shape"""
    zd = z.to(DEV).requires_grad_(True)
    with Native():
        loss = (fn or FN[kind])(zd, t.to(DEV))
        (g,) = torch.autograd.grad(loss * scale, zd)
    return loss.detach(), g


@functools.lru_cache(maxsize=2)
def case(kind, regime, B, C, V, scale=1.7, seed=0):
    """inputs and the float64 reference of one parametrised shape, built once"""
    z, t = L.make_inputs(regime, B, C, V, seed)
    l64, g64 = L.reference(kind, z, t, scale)
    return z, t, l64, g64


def compare(name, kind, regime, z, t, ld, gd, l64, g64, scale):
    P.close(f"{name}: loss", ld, l64, rel=L.LOSS_REL, floor=L.LOSS_FLOOR)
    why, k, kp = L.KINK.get((kind, regime)), 0.0, None
    if why:
        _, g32 = L.reference(kind, z, t, scale, dtype=torch.float32)
        k, kp = L.kink(g32, g64)
    gd = gd.detach().cpu()
    P.close(f"{name}: dL/dz", gd, g64, floor=0.0, extra=k, why=why)
    B, C = g64.shape[:2]
    d, s = L.plane_errors(gd, g64)
    P.note(f"{name}: worst plane", rel_err_of_plane_max=(d / (s + 1e-300)).max().item(), smallest_plane_max=s.min().item())
    for b in range(B):
        for c in range(C):
            P.close(f"{name}: dL/dz plane ({b},{c})", gd[b, c], g64[b, c], floor=0.0,
                    extra=kp[b, c].item() if why else 0.0, why=why)


def run_case(kind, regime, B, C, V, scale=1.7, seed=0):
    z, t, l64, g64 = case(kind, regime, B, C, V, scale, seed)
    ld, gd = device_loss(kind, z, t, scale)
    compare(f"{kind} {regime} ({B},{C},{V})", kind, regime, z, t, ld, gd, l64, g64, scale)
    return ld, gd


SHAPES = [
    ("ce", 2, 3, 4),                  # the minimum: one float4 per row
    ("ce", 2, 3, 32768 * 2 - 4),      # the last one-chunk size
    ("ce", 2, 3, 65536),              # two chunks
    ("ce", 2, 3, 32768 * 3 + 4),      # three chunks, `per` = 32772 (not a multiple of 1024), short last chunk
    ("ce", 1, 3, V128),               # 64 chunks
    ("ce", 2, 3, V128),               # the gradient grid exactly at its 4096-block cap
    ("ce", 4, 3, V128),               # past the cap: the grid-stride loop runs twice
    ("bce", 2, 3, 4),
    ("bce", 2, 1, 32768 * 2 - 4),
    ("bce", 2, 3, 32768 * 3 + 4),
    ("bce", 1, 3, V128),              # planes·V = 6 Mi > 4 Mi: dice_bce_grad's grid-stride loop
    ("bce", 2, 9, 4096),              # C = 9: no multi-channel CE kernel, but the per-plane BCE kernels take any C
]


@pytest.mark.parametrize("kind,B,C,V", SHAPES)
def test_loss_shape_matrix_vs_float64(kind, B, C, V):
    run_case(kind, "randn3", B, C, V)


@pytest.mark.parametrize("C", [8, 2])
def test_finish_kernel_at_B8_and_aten_finish_at_B9(C):
    """B = 8 fills the finish kernel's column table (8 x (3C + 1)); B = 9 composes the finish in ATen.  Both against float64,
    and against each other: the ninth item changes nothing in the first eight planes' Dice coefficients, so the gradients
    of the first eight items differ by the factor 9/8 of the two means only."""
    V = 32768 * 3 + 4
    z, t = L.make_inputs("randn3", 9, C, V, seed=2)
    out = {}
    for B in (8, 9):
        l64, g64 = L.reference("ce", z[:B], t[:B], 1.7)
        ld, gd = device_loss("ce", z[:B], t[:B], 1.7)
        compare(f"ce finish B={B} C={C}", "ce", "randn3", z[:B], t[:B], ld, gd, l64, g64, 1.7)
        out[B] = gd
    P.close(f"ce finish C={C}: B=9 gradient x 9/8 vs B=8", out[9][:8] * (9.0 / 8.0), out[8], floor=0.0)


@pytest.mark.parametrize("C", [1, 2, 3, 4, 5, 6, 7, 8])
def test_every_channel_count_runs_its_own_kernels(C):
    V = 32768 * 3 + 4
    z, t, l64, g64 = case("ce", "randn3", 2, C, V)
    timer = Fn.KernelTimer()
    Fn.set_timer(timer)
    try:
        ld, gd = device_loss("ce", z, t, 1.7)
    finally:
        Fn.set_timer(None)
    ran = set(timer.summary())
    want = {"dice_bce_sums", "dice_bce_grad"} if C == 1 else {"dice_ce_sums", "dice_ce_grad"}
    assert want <= ran and not any(k.startswith("dice_") for k in ran - want), sorted(ran)
    compare(f"ce C={C}", "ce", "randn3", z, t, ld, gd, l64, g64, 1.7)
    with Native():
        lm = ft.DiceCELoss(sigmoid=True, squared_pred=True)(z.to(DEV), t.to(DEV))
    assert torch.equal(lm, ld)


@pytest.mark.parametrize("kind", ["ce", "bce"])
@pytest.mark.parametrize("V,shapes", [(4096, ((4096,), (64, 64), (16, 16, 16))), (65536, ((65536,), (256, 256), (32, 32, 64)))])
def test_spatial_rank_1_2_3_bitwise_equal(kind, V, shapes):
    """the kernels see (B, C, V) only: (B, C, L), (B, C, H, W) and (B, C, D, H, W) of equal V give the same bits"""
    z, t, l64, g64 = case(kind, "randn3", 2, 3, V)
    got = []
    for s in shapes:
        ld, gd = device_loss(kind, z.reshape(2, 3, *s), t.reshape(2, 3, *s), 1.7)
        assert gd.shape == (2, 3, *s)
        got.append((ld, gd.reshape(2, 3, V)))
    compare(f"{kind} rank-1 V={V}", kind, "randn3", z, t, got[0][0], got[0][1], l64, g64, 1.7)
    for ld, gd in got[1:]:
        assert torch.equal(ld, got[0][0]) and torch.equal(gd, got[0][1])


@pytest.mark.parametrize("V", [20000, 32768 * 3 + 4])
@pytest.mark.parametrize("regime", L.REGIMES)
@pytest.mark.parametrize("kind,C", [("ce", 3), ("bce", 1), ("bce", 3)])
def test_input_regimes_vs_float64(kind, C, regime, V):
    run_case(kind, regime, 2, C, V, seed=1)


# ---- interface ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ce", "bce"])
def test_bf16_logits(kind):
    """bf16 logits are evaluated in fp32: the loss is the loss of the same values as fp32, bit for bit; the gradient comes
    back in bf16, one rounding away from the fp32 gradient"""
    z, t = L.make_inputs("randn3", 2, 3, 32768 * 3 + 4, seed=3)
    zb = z.to(torch.bfloat16)
    l32, g32 = device_loss(kind, zb.float(), t, 1.7)
    lb, gb = device_loss(kind, zb, t, 1.7)
    assert lb.dtype == torch.float32 and torch.equal(lb, l32)
    assert gb.dtype == torch.bfloat16
    P.close(f"{kind}: bf16 gradient vs fp32 gradient", gb.float(), g32, rel=2 * U, floor=0.0,
            why="bf16 storage: the gradient is rounded to bf16 once, bound 2 x u = 2^-8 as in test_gpu_bf16.py")
    l64, g64 = L.reference(kind, zb.float(), t, 1.7)
    P.close(f"{kind}: bf16 loss vs float64", lb, l64, rel=L.LOSS_REL, floor=L.LOSS_FLOOR)


@pytest.mark.parametrize("kind", ["ce", "bce"])
def test_bool_and_uint8_targets_equal_float_targets(kind):
    z, t = L.make_inputs("randn3", 2, 3, 32768 * 3 + 4, seed=4)
    lf, gf = device_loss(kind, z, t, 1.7)
    for dt in (torch.bool, torch.uint8):
        ld, gd = device_loss(kind, z, t.to(dt), 1.7)
        assert torch.equal(ld, lf) and torch.equal(gd, gf), dt
    l64, g64 = L.reference(kind, z, t, 1.7)
    compare(f"{kind} float targets", kind, "randn3", z, t, lf, gf, l64, g64, 1.7)


@pytest.mark.parametrize("kind", ["ce", "bce"])
def test_non_contiguous_logits_equal_contiguous(kind):
    """a channels-last head output, permuted into (B, C, D, H, W) without a copy"""
    g = torch.Generator().manual_seed(6)
    zl = torch.randn(2, 16, 16, 260, 3, generator=g) * 3        # (B, D, H, W, C)
    t = (torch.rand(2, 3, 16, 16, 260, generator=g) > 0.5).float()
    zp = zl.permute(0, 4, 1, 2, 3)
    assert not zp.is_contiguous()
    zd = zl.to(DEV).permute(0, 4, 1, 2, 3).requires_grad_(True)
    assert not zd.is_contiguous()
    with Native():
        ln = FN[kind](zd, t.to(DEV))
        (gn,) = torch.autograd.grad(ln * 1.7, zd)
    lc, gc = device_loss(kind, zp.contiguous(), t, 1.7)
    assert torch.equal(ln, lc) and torch.equal(gn, gc)
    l64, g64 = L.reference(kind, zp.contiguous(), t, 1.7)
    compare(f"{kind} permuted view", kind, "randn3", zp.reshape(2, 3, -1), t.reshape(2, 3, -1), ln,
            gn.reshape(2, 3, -1), l64, g64.reshape(2, 3, -1), 1.7)


@pytest.mark.parametrize("kind", ["ce", "bce"])
def test_upstream_gradient_scales(kind):
    """1, 1.7 and an AMP loss scale of 65536: the gradient is linear in the upstream scalar, exactly so for a power of two"""
    z, t = L.make_inputs("randn3", 2, 3, 32768 * 3 + 4, seed=5)
    g = {}
    for s in (1.0, 1.7, 65536.0):
        l64, g64 = L.reference(kind, z, t, s)
        ld, g[s] = device_loss(kind, z, t, s)
        compare(f"{kind} scale {s:g}", kind, "randn3", z, t, ld, g[s], l64, g64, s)
    assert torch.equal(g[65536.0], g[1.0] * 65536.0)
    P.close(f"{kind}: gradient at scale 1.7 vs 1.7 x gradient at scale 1", g[1.7], g[1.0] * 1.7, floor=0.0)


def test_three_replays_at_128_cubed_are_bitwise_equal():
    z, t, l64, g64 = case("ce", "randn3", 2, 3, V128)
    runs = [device_loss("ce", z, t, 1.7) for _ in range(3)]
    for ld, gd in runs[1:]:
        assert torch.equal(ld, runs[0][0]) and torch.equal(gd, runs[0][1])
    P.close("replay 128^3: loss", runs[0][0], l64, rel=L.LOSS_REL, floor=L.LOSS_FLOOR)
    P.close("replay 128^3: dL/dz", runs[0][1], g64, floor=0.0)


@pytest.mark.parametrize("kind,why,B,C,V,dt", [
    ("ce", "V % 4 != 0", 2, 3, 4098, torch.float32), ("ce", "C = 9", 2, 9, 4096, torch.float32),
    ("ce", "float64 logits", 2, 3, 4096, torch.float64),
    # (the dice_bce kernels work on B·C planes and take any C: C = 9 is native there, tested in the shape matrix)
    ("bce", "V % 4 != 0", 2, 3, 4098, torch.float32), ("bce", "float64 logits", 2, 3, 4096, torch.float64)])
def test_composed_device_branch_warns_once_and_matches_float64(kind, why, B, C, V, dt):
    """shapes and types outside the kernel set run as composed framework ops on the device, and say so (once per process)"""
    z, t = L.make_inputs("randn3", B, C, V, seed=7)
    l64, g64 = L.reference(kind, z, t, 1.7)
    key = {"ce": "dice_ce_loss", "bce": "dice_bce_loss"}[kind]
    CO._warned.discard(key)
    zd = z.to(DEV).to(dt).requires_grad_(True)
    n0 = _native.launch_count()
    with pytest.warns(RuntimeWarning, match="no native kernel"):
        ld = FN[kind](zd, t.to(DEV))
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)      # ... once
        ld2 = FN[kind](zd, t.to(DEV))
    (gd,) = torch.autograd.grad(ld * 1.7, zd)
    torch.cuda.synchronize()
    assert _native.launch_count() == n0, "the composed branch launched a native kernel"
    assert torch.equal(ld, ld2)
    compare(f"{kind} composed on device ({why})", kind, "randn3", z, t, ld, gd, l64, g64, 1.7)
