"""-m gpu: csrc/optim.hip (fz_adamw_step) and ft.FlatAdamW.step against `adamw64`, the float64 restatement of
torch.optim.AdamW's update (tests/loss_adamw_cases.py; checked against torch itself in tests/test_loss_adamw_cpu.py).
After EVERY step three buffers are compared: the parameter update p − p0, exp_avg and exp_avg_sq — at gradient magnitudes
real training produces (1e-8 .. 1e-2, exact zeros), late step counts, a changing lr, grad_scale, and buffers past the
2048-block grid cap with a scalar tail.

Bounds.  Moments: 1e-4 of max|ref| (no absolute floor: exp_avg_sq is 1e-7 and below).  Parameter:
max|Δp − Δp64| ≤ 1e-4·max|Δp64| + steps·2^-23·max|p| — the kernel rounds p twice per step (decay multiply, subtract), half
an ulp of p each; parameters start at weight-like scale (randn·0.05) so that term stays small next to the update."""
import pytest
import torch

import factorizer_amd as ft
from factorizer_amd import _native
import loss_adamw_cases as L
import parity as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MI = 1 << 20
HP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, wd=1e-2)


def compare(name, k, p, m, v, p0, p64, m64, v64):
    """after step k: device fp32 (p, m, v) against the float64 run"""
    P.close(f"{name} step {k}: exp_avg", m, m64, floor=0.0)
    P.close(f"{name} step {k}: exp_avg_sq", v, v64, floor=0.0)
    dp64 = p64 - p0.double()
    dp = p.detach().cpu().double() - p0.double()
    rel, ulp = L.param_bound_terms(dp64, p64, k)
    P.note(f"{name} step {k}: parameter bound terms", rel_term=rel, ulp_term=ulp, max_dp=dp64.abs().max().item())
    # (parity.close works in fp32: Δp of both sides is formed in float64 first, so the cast costs 2^-24 of Δp, not of p)
    P.close(f"{name} step {k}: p - p0", dp, dp64, floor=0.0, extra=ulp)


def run_kernel(name, n, regime, steps=3, t0=0, grad_scale=1.0, lrs=None, seed=0, **hp):
    """fz_adamw_step called directly on n-element buffers (the only way to reach the scalar tail: FlatAdamW pads every
    parameter to a multiple of four); returns the final device (p, m, v)"""
    hp = {**HP, **hp}
    gen = torch.Generator().manual_seed(seed)
    p0, m0, v0 = L.make_state(n, gen)
    if not t0:
        m0, v0 = torch.zeros(n), torch.zeros(n)
    p, m, v = p0.to(DEV), m0.to(DEV), v0.to(DEV)
    p64, m64, v64 = p0.double(), m0.double(), v0.double()
    lib = _native.lib()
    for k in range(1, steps + 1):
        lr = lrs[k - 1] if lrs else hp["lr"]
        g = L.make_grad(regime, n, gen)
        gd = (g * (1.0 / grad_scale)).to(DEV)      # grad_scale is a power of two wherever it is not 1: exact
        assert gd.numel() == p.numel() == m.numel() == v.numel() == n
        n0 = _native.launch_count()
        with torch.cuda.device(0):
            rc = lib.fz_adamw_step(p.data_ptr(), gd.data_ptr(), m.data_ptr(), v.data_ptr(), n, lr, *hp["betas"], hp["eps"],
                                   hp["wd"], t0 + k, grad_scale, _native.stream_ptr(p))
        _native.check(rc, "fz_adamw_step")
        torch.cuda.synchronize()
        assert _native.launch_count() == n0 + 1
        p64, m64, v64 = L.adamw64(p64, g.double(), m64, v64, t0 + k, lr, hp["betas"], hp["eps"], hp["wd"])
        compare(name, k, p, m, v, p0, p64, m64, v64)
    return p, m, v


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1023, 1024, 2 * MI, 2 * MI + 3, 5_860_003])
def test_adamw_kernel_sizes(n):
    """vector body only, tail only, both; exactly the grid cap (2048 blocks x 256 threads x 4), past it with a tail (the
    grid-stride loop), and the README model's 5.86 M parameters"""
    run_kernel(f"n={n}", n, "loguniform", seed=n % 97)


@pytest.mark.parametrize("regime", L.GRAD_REGIMES)
@pytest.mark.parametrize("t0", [0, 1000])
def test_adamw_kernel_gradient_regimes(regime, t0):
    n = 2 * MI + 3
    p, m, v = run_kernel(f"{regime} t0={t0}", n, regime, t0=t0, seed=3)
    if regime == "allzero" and not t0:
        # m / (0 + eps) with m = 0: the parameter sits at its decayed value, the moments at zero
        p0 = L.make_state(n, torch.Generator().manual_seed(3))[0]
        want = p0.double() * (1.0 - HP["lr"] * HP["wd"]) ** 3
        assert not m.any() and not v.any()
        assert (p.cpu().double() - want).abs().max().item() <= 3 * 2.0 ** -23 * want.abs().max().item()   # 2 roundings a step


@pytest.mark.parametrize("regime", ["randn", "loguniform"])
def test_adamw_kernel_grad_scale(regime):
    """gradients pre-multiplied by 1/grad_scale (an unscaled AMP run): against float64, and for the power-of-two scales
    bit for bit the unscaled run"""
    n = 1024 + 3
    base = run_kernel(f"{regime} grad_scale=1", n, regime, t0=10, seed=4)
    for gs in (0.5, 1.0 / 65536):
        got = run_kernel(f"{regime} grad_scale={gs:g}", n, regime, t0=10, grad_scale=gs, seed=4)
        for a, b in zip(got, base):
            assert torch.equal(a, b), gs


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("betas,eps", [((0.9, 0.999), 1e-8), ((0.8, 0.99), 1e-6)])
def test_adamw_kernel_hyperparameters(betas, eps, wd):
    run_kernel(f"betas={betas} eps={eps:g} wd={wd:g}", 4 * MI + 1, "zeros10", t0=2, betas=betas, eps=eps, wd=wd, seed=5,
               lrs=[1e-3, 3e-4, 1e-5])


@pytest.mark.parametrize("t0", [0, 1, 9, 999, 99999])
@pytest.mark.parametrize("shapes", [((5_860_003,),), ((3,), (5, 7), (1031,), (2 * MI + 1,))])
def test_flat_adamw_step_counts_and_schedule(t0, shapes):
    """ft.FlatAdamW end to end: a torch-layout state_dict with non-trivial moments sets the step count (the three steps taken
    are t0+1 .. t0+3: t = 1, 2, 10, 1000, 100000 are all among them), WarmupCosineSchedule changes lr before every step,
    grad_scale = 0.5 with doubled gradients.  Every parameter's slice of the flat buffers against float64."""
    gen = torch.Generator().manual_seed(7)
    st = [L.make_state(int(torch.Size(s).numel()), gen) for s in shapes]
    params = torch.nn.ParameterList([torch.nn.Parameter(p0.reshape(s).to(DEV)) for s, (p0, _, _) in zip(shapes, st)])
    opt = ft.FlatAdamW(params, lr=1e-3, weight_decay=1e-2, deferred_finishes=False)
    ref = [(p0.double(), torch.zeros_like(p0).double(), torch.zeros_like(p0).double()) for p0, _, _ in st]
    if t0:
        sd = opt.state_dict()
        sd["state"] = {i: {"step": torch.tensor(float(t0)), "exp_avg": m0.reshape(s).clone(), "exp_avg_sq": v0.reshape(s).clone()}
                       for i, (s, (_, m0, v0)) in enumerate(zip(shapes, st))}
        opt.load_state_dict(sd)
        ref = [(p0.double(), m0.double(), v0.double()) for p0, m0, v0 in st]
    sched = ft.WarmupCosineSchedule(opt, warmup_steps=2, t_total=10, warmup_multiplier=0.1)
    lrs = []
    for k in range(1, 4):
        gs = [L.make_grad("loguniform" if i % 2 == 0 else "zeros10", p.numel(), gen) for i, p in enumerate(params)]
        for p, g in zip(params, gs):
            p.grad = (g * 2.0).reshape(p.shape).to(DEV)
        lrs.append(opt.lr)
        n0 = _native.launch_count()
        opt.step(grad_scale=0.5)
        sched.step()
        torch.cuda.synchronize()
        assert _native.launch_count() == n0 + 1 and opt.t == t0 + k      # one launch over the whole flat buffer
        ref = [L.adamw64(p64, g.double(), m64, v64, t0 + k, lrs[-1], (0.9, 0.999), 1e-8, 1e-2)
               for (p64, m64, v64), g in zip(ref, gs)]
        for i, (p, (p0, _, _), (p64, m64, v64)) in enumerate(zip(params, st, ref)):
            lo, n = opt.offsets[p], p.numel()
            compare(f"FlatAdamW t0={t0} param {i} ({n})", k, p.detach().reshape(-1), opt.exp_avg[lo:lo + n],
                    opt.exp_avg_sq[lo:lo + n], p0, p64, m64, v64)
    assert len(set(lrs)) == 3, lrs
    sd = opt.state_dict()
    assert all(float(sd["state"][i]["step"]) == t0 + 3 for i in range(len(shapes)))
