"""CPU-side companions of tests/test_gpu_loss.py and tests/test_gpu_adamw.py (no GPU needed).

1. The references of the GPU tests stay well inside the GPU tests' own bounds: for every input regime of
   tests/loss_adamw_cases.py the composed fp32 loss and gradient are within ONE TENTH of the bound against the composed
   float64 form, and the fp32 CPU branch of FlatAdamW is within one tenth of the AdamW bounds against `adamw64` (moments, and the
   relative term of the parameter bound; its ulp term is what any fp32 update spends, and is kept whole).  An input
   regime edited into an ill-conditioned one fails here, before a kernel gets blamed on the device.
2. `adamw64` is torch.optim.AdamW (checked on float64 tensors).
3. The host-side argument checks of csrc/loss.hip and csrc/optim.hip."""
import ctypes

import pytest
import torch

import factorizer_amd as ft
import loss_adamw_cases as L


@pytest.fixture(scope="module")
def built_lib():
    from factorizer_amd import build
    return build.build(verbose=False)


CASES = [(kind, C, regime, V) for kind, C in (("ce", 3), ("bce", 1), ("bce", 3)) for regime in L.REGIMES
         for V in (4096, 32768 + 4)]


@pytest.mark.parametrize("kind,C,regime,V", CASES)
def test_composed_fp32_within_a_tenth_of_the_gpu_bound(kind, C, regime, V):
    z, t = L.make_inputs(regime, 2, C, V, seed=1)
    l64, g64 = L.reference(kind, z, t, 1.7)
    l32, g32 = L.reference(kind, z, t, 1.7, dtype=torch.float32)
    assert abs(l32.item() - l64.item()) <= 0.1 * (L.LOSS_REL * abs(l64.item()) + L.LOSS_FLOOR)
    d, s = L.plane_errors(g32, g64)
    worst, worst_plane = (d.max() / s.max()).item(), (d / s).max().item()
    print(f"{kind} C={C} {regime} V={V}: fp32 vs float64 gradient {worst:.2e} of max, {worst_plane:.2e} of a plane's max")
    if (kind, regime) in L.KINK:
        # the one listed reason a bound carries `kink`: no fp32 evaluation of THIS regime holds 1e-4 (the composed path is
        # off by the whole plane maximum), so the GPU bound is 1e-4·max + 30 x this distance — a tenth of which it meets
        assert worst_plane > L.GRAD_REL, "this regime no longer needs its kink term: drop it from loss_adamw_cases.KINK"
        k, kp = L.kink(g32, g64)
        assert d.max().item() <= 0.1 * (L.GRAD_REL * s.max().item() + k)
        assert (d <= 0.1 * (L.GRAD_REL * s + kp)).all()
    else:
        assert worst <= 0.1 * L.GRAD_REL and worst_plane <= 0.1 * L.GRAD_REL


def test_adamw64_is_torch_adamw():
    """the ten-line float64 restatement against torch.optim.AdamW on float64 tensors: 6 steps, changing lr, loaded step count"""
    gen = torch.Generator().manual_seed(5)
    for betas, eps, wd, t0 in (((0.9, 0.999), 1e-8, 1e-2, 0), ((0.8, 0.99), 1e-6, 0.0, 1000)):
        p0, m0, v0 = (x.double() for x in L.make_state(1001, gen))
        ref = torch.nn.Parameter(p0.clone())
        opt = torch.optim.AdamW([ref], lr=1e-3, betas=betas, eps=eps, weight_decay=wd)
        p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
        if t0:
            m, v = m0.clone(), v0.clone()
            sd = opt.state_dict()
            sd["state"] = {0: {"step": torch.tensor(float(t0)), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}}
            opt.load_state_dict(sd)
        for k in range(1, 7):
            lr = 1e-3 / k
            opt.param_groups[0]["lr"] = lr
            g = L.make_grad("zeros10", 1001, gen).double()
            ref.grad = g.clone()
            opt.step()
            p, m, v = L.adamw64(p, g, m, v, t0 + k, lr, betas, eps, wd)
            st = opt.state[ref]
            assert float(st["step"]) == t0 + k
            for a, b in ((ref.detach(), p), (st["exp_avg"], m), (st["exp_avg_sq"], v)):
                assert (a - b).abs().max().item() <= 1e-12 * b.abs().max().item()


@pytest.mark.parametrize("regime", L.GRAD_REGIMES)
@pytest.mark.parametrize("t0", [0, 1000, 100000])
def test_flat_adamw_fp32_cpu_within_a_tenth_of_the_gpu_bound(regime, t0):
    gen = torch.Generator().manual_seed(11)
    n, steps = 4099, 3
    p0, m0, v0 = L.make_state(n, gen)
    par = torch.nn.Parameter(p0.clone())
    opt = ft.FlatAdamW([par], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, deferred_finishes=False)
    p, m, v = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    if t0:
        m, v = m0.double(), v0.double()
        sd = opt.state_dict()
        sd["state"] = {0: {"step": torch.tensor(float(t0)), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}}
        opt.load_state_dict(sd)
    sched = ft.WarmupCosineSchedule(opt, warmup_steps=2, t_total=10, warmup_multiplier=0.1)
    for k in range(1, steps + 1):
        g = L.make_grad(regime, n, gen)
        par.grad = g.clone()
        lr = opt.lr
        opt.step()
        sched.step()
        p, m, v = L.adamw64(p, g.double(), m, v, t0 + k, lr, (0.9, 0.999), 1e-8, 1e-2)
        dp, dp64 = par.detach().double() - p0.double(), p - p0.double()
        rel, ulp = L.param_bound_terms(dp64, p, k)
        # a tenth of the relative term; the ulp term is kept whole — it is no slack but the two roundings of p that ANY fp32
        # update makes per step (this one reaches half of it), so no fp32 run can stay inside a tenth of it
        assert (dp - dp64).abs().max().item() <= 0.1 * rel + ulp
        for a, b in ((opt.exp_avg[:n], m), (opt.exp_avg_sq[:n], v)):
            assert (a.double() - b).abs().max().item() <= 0.1 * 1e-4 * b.abs().max().item()


def test_loss_and_adamw_host_side_argument_checks(built_lib):
    """csrc/loss.hip and csrc/optim.hip validate their arguments before touching the device."""
    from factorizer_amd import _native
    lib = _native.lib()
    p8 = ctypes.c_void_p(8)   # (a non-null pointer value the host code never dereferences)
    E_SHAPE, E_UNSUPPORTED, E_ARG = -1, -2, -4
    for V in (0, 3, 6, 4097):
        assert lib.fz_dice_bce_sums(p8, p8, p8, 2, V, None) == E_SHAPE and b"fz_dice_bce_sums" in lib.fz_last_error_string()
        assert lib.fz_dice_bce_grad(p8, p8, p8, p8, 2, V, 0.5, 0.5, None, None) == E_SHAPE
        assert b"fz_dice_bce_grad" in lib.fz_last_error_string()
        assert lib.fz_dice_ce_sums(p8, p8, p8, 2, 3, V, None) == E_SHAPE and b"fz_dice_ce_sums" in lib.fz_last_error_string()
        assert lib.fz_dice_ce_grad(p8, p8, p8, p8, 2, 3, V, 0.5, 0.5, None, None) == E_SHAPE
        assert b"fz_dice_ce_grad" in lib.fz_last_error_string()
    for C in (1, 9):
        assert lib.fz_dice_ce_sums(p8, p8, p8, 2, C, 64, None) == E_UNSUPPORTED
        assert lib.fz_dice_ce_grad(p8, p8, p8, p8, 2, C, 64, 0.5, 0.5, None, None) == E_UNSUPPORTED
        assert lib.fz_dice_ce_finish(p8, 2, C, 64, 1e-5, p8, p8, None) == E_UNSUPPORTED
    assert lib.fz_dice_ce_finish(p8, 9, 3, 64, 1e-5, p8, p8, None) == E_UNSUPPORTED
    assert lib.fz_dice_ce_finish(p8, 0, 3, 64, 1e-5, p8, p8, None) == E_UNSUPPORTED
    assert lib.fz_dice_bce_sums(None, p8, p8, 2, 64, None) == E_ARG
    hp = (1e-3, 0.9, 0.999, 1e-8, 1e-2)
    assert lib.fz_adamw_step(p8, p8, p8, p8, 16, *hp, 0, 1.0, None) == E_ARG and b"step >= 1" in lib.fz_last_error_string()
    assert lib.fz_adamw_step(p8, p8, p8, p8, -1, *hp, 1, 1.0, None) == E_ARG
    assert lib.fz_adamw_step(None, p8, p8, p8, 16, *hp, 1, 1.0, None) == E_ARG
    assert lib.fz_adamw_step(p8, p8, p8, p8, 0, *hp, 1, 1.0, None) == 0          # nothing to do: FZ_OK, no launch
    got = [lib.fz_dice_bce_chunks(V) for V in (4, 65535, 65536, 98308, 2 ** 21, 2 ** 21 + 4, 256 ** 3)]
    assert got == [1, 1, 2, 3, 64, 64, 64]
