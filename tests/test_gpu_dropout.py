"""-m gpu: FactorizerBlock in training mode with live dropout runs as the one-node native block (pointwise.FactorizerBlockFn;
csrc/dropout.hip).  The masks are not torch's (nn.Dropout draws from another stream); the contract is: the keep probability is
exactly floor((1 - p) 2^32) / 2^32, the bits are reproducible from the seed (tests/philox_ref.py), and the forward and the
backward use the same masks.  The oracle is the composed CPU block with those masks applied at the reference's three sites
(factorizer.py:53-56,69,72; mlp.py:54-60)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import factorizer_amd as ft
import parity as P
import philox_ref as R
from factorizer_amd import _native
from factorizer_amd import functional as Fn
from factorizer_amd import pointwise as PW
from factorizer_amd.training import FlatAdamW
from oracle import cpu_ref as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
U = 2.0 ** -8   # unit roundoff of bf16 storage


class Launches:
    """Asserts that the native library actually launched kernels inside the block."""

    def __enter__(self):
        self.n0 = _native.launch_count()
        return self

    def __exit__(self, *a):
        torch.cuda.synchronize()
        assert _native.launch_count() > self.n0, "native kernels were not launched"


def unpack(bits, V):
    """int32 (B, ch, nw) keep-bit words -> float mask (B, ch, V)"""
    w = bits.to(torch.int64) & 0xFFFFFFFF
    m = (w.unsqueeze(-1) >> torch.arange(32, device=bits.device)) & 1
    return m.reshape(*bits.shape[:2], -1)[..., :V].float()


def _block(C, S, reshape_kw, nmf_kw, mlp_ratio=2, ps=(0.1, 0.1, 0.1)):
    torch.manual_seed(0)
    blk = ft.FactorizerBlock(channels=C, spatial_size=S, norm=ft.LayerNorm, reshape=(ft.SWMatricize, reshape_kw),
                             act=nn.ReLU, factorize=ft.NMF, init="uniform", mlp_ratio=mlp_ratio, dropout=0.0, **nmf_kw)
    blk.fact.dropout.p, blk.mlp.block[2].p, blk.mlp.block[4].p = ps
    return blk


README = dict(C=32, S=(32, 32, 32), reshape_kw=dict(head_dim=8, patch_size=8), nmf_kw=dict(rank=1, num_iters=5, solver="hals"))


# ---------------------------------------------------------------- mask generator ------------------------------------
@pytest.mark.parametrize("V", [8 * 8 * 12, 5 * 6 * 7])
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
def test_keep_bits_bit_exact(V, p):
    B, ch = 2, 5
    seed_val = 0x0123456789ABCDE
    seed = torch.tensor([seed_val], dtype=torch.int64, device=DEV)
    for site in range(3):
        with Launches():
            got = Fn.dropout_keep_bits(seed, site, B, ch, V, p)
        ref = R.keep_bits(seed_val, site, B, ch, V, p)
        assert got.shape == (B, ch, (V + 31) // 32)
        assert np.array_equal(got.cpu().numpy(), ref), (site, p, V)
        if p == 0:
            assert bool((unpack(got, V) == 1).all())


def test_keep_rate_is_exact_threshold():
    B, ch, V, p = 2, 5, 1 << 20, 0.1          # 1.05e7 elements
    seed = Fn.dropout_seed(DEV)
    bits = Fn.dropout_keep_bits(seed, 1, B, ch, V, p)
    n = B * ch * V
    kept = int(unpack(bits, V).sum().item())
    q = R.keep_threshold(p) / 2.0 ** 32
    sigma = math.sqrt(n * q * (1 - q))
    P.note("dropout keep rate", kept=kept, n=n, expected=n * q, sigma=sigma)
    assert abs(kept - n * q) <= 5 * sigma, (kept, n * q, sigma)


# ---------------------------------------------------------------- the block -------------------------------------------
def test_readme_block_with_dropout_runs_as_one_node():
    blk = _block(**README).to(DEV).train()
    x = torch.rand(2, 32, 32, 32, 32, device=DEV, requires_grad=True)
    with Launches():
        y = blk(x)
    assert type(y.grad_fn).__name__ == "FactorizerBlockFnBackward", type(y.grad_fn).__name__
    y.sum().backward()
    assert torch.isfinite(x.grad).all()


def test_readme_block_dropout_takes_the_fused_launches():
    """(C, hidden) = (32, 64): the forward runs its three masks inside the out-projection + MLP chain launch (no elementwise
    dropout pass, no separate fc layer); in the backward fz_gemm_dw reads g as M0 s0 g (the one remaining site-0/2 pass is
    g_f = M2 s2 g2 for the MLP's separate layers)"""
    blk = _block(32, (16, 16, 16), dict(head_dim=8, patch_size=8), dict(rank=1, num_iters=5, solver="hals")).to(DEV).train()
    x = torch.rand(2, 32, 16, 16, 16, device=DEV, requires_grad=True)

    def launches(fn):
        tm = Fn.KernelTimer()
        Fn.set_timer(tm)
        try:
            out = fn()
        finally:
            Fn.set_timer(None)
        return out, {k: v["calls"] for k, v in tm.summary().items()}
    y, fwd = launches(lambda: blk(x))
    assert "outproj_mlp_chain_fwd_32" in fwd, fwd
    assert not any(k.startswith(("dropout_apply", "linear_", "ln_linear_32->64", "act_linear_res")) for k in fwd), fwd
    _, bwd = launches(lambda: y.sum().backward())
    assert bwd.get("dgrad_wgrad_32") == 1 and bwd.get("dropout_apply0_32") == 1, bwd


def _oracle(x, sd, cfg, masks, ps):
    """FactorizerBlock.forward (factorizer.py:74-77) with the three dropout sites applied by the given masks"""
    def drop(t, m, p):
        return t if p == 0 else t * (m * (1.0 / (1.0 - p)))
    y = O.layernorm_cf(x, sd["norm1.norm.weight"], sd["norm1.norm.bias"])
    x1 = x + drop(O.fact_mixer(y, sd, "fact.", cfg), masks[0], ps[0])
    y = O.layernorm_cf(x1, sd["norm2.norm.weight"], sd["norm2.norm.bias"])
    h = drop(F.gelu(O.linear_cf(y, sd["mlp.block.0.linear.weight"], sd["mlp.block.0.linear.bias"])), masks[1], ps[1])
    return x1 + drop(O.linear_cf(h, sd["mlp.block.3.linear.weight"], sd["mlp.block.3.linear.bias"]), masks[2], ps[2])


def _masks(blk, B, S, ps, seed_call):
    """the three masks of the forward that ran right after torch.cuda.manual_seed(seed_call), rebuilt through the documented
    seed helper (functional.dropout_seed: the block forward's first use of the device generator)"""
    C, Hd = blk.norm1.norm.weight.shape[0], blk.mlp.block[0].linear.weight.shape[0]
    V = math.prod(S)
    torch.cuda.manual_seed(seed_call)
    seed = Fn.dropout_seed(DEV)
    return [None if p == 0 else unpack(Fn.dropout_keep_bits(seed, s, B, ch, V, p), V).reshape(B, ch, *S).cpu()
            for s, (ch, p) in enumerate(zip((C, Hd, C), ps))]


def _run_device(blk, x, gy, seed_call):
    xd = x.to(DEV).requires_grad_(True)
    torch.cuda.manual_seed(seed_call)
    with Launches():
        yd = blk(xd)
        assert type(yd.grad_fn).__name__ == "FactorizerBlockFnBackward"
        gd = torch.autograd.grad(yd, [xd] + list(blk.parameters()), gy.to(DEV, x.dtype))
    return yd, gd


def _parity(C, S, reshape_kw, nmf_kw, mlp_ratio=2, ps=(0.1, 0.1, 0.1), B=2, tol=1e-4, why=None):
    blk = _block(C, S, reshape_kw, nmf_kw, mlp_ratio, ps).train()
    sd = {k: v.clone() for k, v in blk.state_dict().items()}
    x = torch.rand(B, C, *S)
    gy = torch.rand_like(x)
    blk = blk.to(DEV)
    names = [k for k, _ in blk.named_parameters()]
    yd, gd = _run_device(blk, x, gy, 1234)
    masks = _masks(blk, B, S, ps, 1234)
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items() if not k.endswith(("u0", "v0"))}
    assert list(params) == names
    full = dict(sd)
    full.update(params)
    xo = x.clone().requires_grad_(True)
    cfg = dict(reshape=reshape_kw, num_iters=nmf_kw.get("num_iters", 5), solver=nmf_kw.get("solver", "hals"))
    yo = _oracle(xo, full, cfg, masks, ps)
    go = torch.autograd.grad(yo, [xo] + list(params.values()), gy)
    P.close("y", yd, yo, rel=tol, why=why)
    P.close("gx", gd[0], go[0], rel=tol, why=why)
    for k, a, b in zip(names, gd[1:], go[1:]):
        P.close(f"grad:{k}", a, b, rel=tol, why=why)


@pytest.mark.parametrize("C,mlp_ratio", [(32, 2), (32, 4), (64, 2), (16, 2)])
def test_block_dropout_vs_masked_oracle(C, mlp_ratio):
    """(C, hidden) = (32, 64): the forward's masks inside the out-projection + MLP chain launch, site 0's backward inside
    fz_gemm_dw, the MLP backward as separate layers; (32, 128), (64, 128) and C = 16: separate layers with the elementwise dropout
    kernels between them (C = 32: site 0's backward in fz_gemm_dw).  All on the fused core."""
    _parity(C, (16, 16, 16), dict(head_dim=8, patch_size=8), dict(rank=1, num_iters=5, solver="hals"), mlp_ratio)


def test_block_dropout_cfg5_patch_generic_core():
    _parity(16, (10, 12, 20), dict(head_dim=8, patch_size=(5, 6, 5)), dict(rank=2, num_iters=10, solver="hals"))


def test_block_dropout_mu_rank2():
    _parity(16, (16, 16, 16), dict(head_dim=8, patch_size=8), dict(rank=2, num_iters=3, solver="mu"))


def test_block_dropout_independent_sites():
    _parity(32, (16, 16, 16), dict(head_dim=8, patch_size=8), dict(rank=1, num_iters=5, solver="hals"), ps=(0.1, 0.0, 0.3))


def test_block_dropout_deterministic_per_seed_and_fresh_per_call():
    blk = _block(32, (16, 16, 16), dict(head_dim=8, patch_size=8), dict(rank=1, num_iters=5, solver="hals")).to(DEV).train()
    torch.manual_seed(5)
    x = torch.rand(2, 32, 16, 16, 16)
    gy = torch.rand_like(x)
    y1, g1 = _run_device(blk, x, gy, 77)
    y2, g2 = _run_device(blk, x, gy, 77)
    assert torch.equal(y1, y2)
    for a, b in zip(g1, g2):
        assert torch.equal(a, b)
    # consecutive forwards draw new seeds, hence new bits and new outputs
    torch.cuda.manual_seed(77)
    s1, s2 = Fn.dropout_seed(DEV), Fn.dropout_seed(DEV)
    b1, b2 = Fn.dropout_keep_bits(s1, 0, 2, 32, 4096, 0.1), Fn.dropout_keep_bits(s2, 0, 2, 32, 4096, 0.1)
    assert not torch.equal(s1, s2) and not torch.equal(b1, b2)
    with torch.no_grad():
        xd = x.to(DEV)
        assert not torch.equal(blk(xd), blk(xd))


def test_dropout_zero_and_eval_unchanged():
    """p = 0 in training mode and any p in eval mode: bitwise the block built with dropout=0.0"""
    kw = dict(C=32, S=(16, 16, 16), reshape_kw=dict(head_dim=8, patch_size=8), nmf_kw=dict(rank=1, num_iters=5, solver="hals"))
    ref = _block(**kw, ps=(0.0, 0.0, 0.0)).to(DEV)
    torch.manual_seed(3)
    x = torch.rand(2, 32, 16, 16, 16)
    gy = torch.rand_like(x)
    for train, ps in ((True, (0.0, 0.0, 0.0)), (False, (0.1, 0.1, 0.1)), (False, (0.5, 0.0, 0.3))):
        blk = _block(**kw, ps=ps).to(DEV).train(train)
        ref.train(train)
        outs = []
        for m in (ref, blk):
            xd = x.to(DEV).requires_grad_(True)
            y = m(xd)
            outs.append((y, torch.autograd.grad(y, [xd] + list(m.parameters()), gy.to(DEV))))
        (ya, ga), (yb, gb) = outs
        assert torch.equal(ya, yb), (train, ps)
        for a, b in zip(ga, gb):
            assert torch.equal(a, b), (train, ps)


def _train(defer, steps=3):
    blk = _block(32, (16, 16, 16), dict(head_dim=8, patch_size=8), dict(rank=1, num_iters=5, solver="hals")).to(DEV).train()
    p0 = [p.detach().clone() for p in blk.parameters()]
    torch.manual_seed(11)
    x = torch.rand(2, 32, 16, 16, 16, device=DEV)
    w = torch.rand_like(x)
    opt = FlatAdamW(blk, lr=1e-3, deferred_finishes=defer)
    grads, losses = [], []
    for i in range(steps):
        opt.zero_grad()
        torch.cuda.manual_seed(100 + i)
        loss = (blk(x) * w).mean()
        loss.backward()
        torch.cuda.synchronize()
        grads.append([p.grad.detach().clone() for p in blk.parameters()])
        losses.append(loss.item())
        opt.step()
    torch.cuda.synchronize()
    moved = [not torch.equal(a, b.detach()) for a, b in zip(p0, blk.parameters())]
    return grads, losses, moved


def test_flat_adamw_with_deferred_finishes_on_dropout_block():
    try:
        g_def, l_def, moved = _train(True)
        assert all(math.isfinite(v) for v in l_def)
        assert all(moved)
        PW.defer_finishes(False)
        g_imm, l_imm, _ = _train(False)
        for sa, sb in zip(g_def, g_imm):
            for a, b in zip(sa, sb):
                assert torch.equal(a, b)
    finally:
        PW.defer_finishes(False)


def test_block_dropout_bf16_vs_masked_fp32_oracle():
    """bf16 activations (fp32 parameters) at (C, hidden) = (32, 64) — the fused dropout launches — against the masked fp32 oracle
    on the same rounded input.  The bound is the p = 0 block's empirical one (tests/test_gpu_bf16.py: 4 u of max|ref|, u = 2^-8),
    not a count of stores (measured about 1.3 u)."""
    C, S, B, ps = 32, (16, 16, 16), 2, (0.1, 0.1, 0.1)
    reshape_kw, nmf_kw = dict(head_dim=8, patch_size=8), dict(rank=1, num_iters=5, solver="hals")
    blk = _block(C, S, reshape_kw, nmf_kw, 2, ps).train()
    sd = {k: v.clone() for k, v in blk.state_dict().items()}
    x = torch.rand(B, C, *S).to(BF).float()
    gy = torch.rand_like(x).to(BF).float()
    blk = blk.to(DEV)
    names = [k for k, _ in blk.named_parameters()]
    yd, gd = _run_device(blk, x.to(BF), gy, 4321)
    assert yd.dtype == BF and gd[0].dtype == BF
    masks = _masks(blk, B, S, ps, 4321)
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items() if not k.endswith(("u0", "v0"))}
    full = dict(sd)
    full.update(params)
    xo = x.clone().requires_grad_(True)
    yo = _oracle(xo, full, dict(reshape=reshape_kw, num_iters=5, solver="hals"), masks, ps)
    go = torch.autograd.grad(yo, [xo] + list(params.values()), gy)
    n = 4
    why = f"bf16 storage: {n} stored tensor(s) x u = 2^-8 between input and this result"
    P.close("y (bf16) vs masked fp32 oracle", yd.float(), yo, rel=n * U, why=why)
    P.close("gx (bf16) vs masked fp32 oracle", gd[0].float(), go[0], rel=n * U, why=why)
    for k, a, b in zip(names, gd[1:], go[1:]):
        assert a.dtype == torch.float32, k
        P.close(f"grad:{k} (bf16) vs masked fp32 oracle", a, b, rel=n * U, why=why)


# ---------------------------------------------------------------- registers ------------------------------------------
def test_dropout_kernels_do_not_spill():
    """the kernels of csrc/dropout.hip and the dropout instantiations of csrc/mlp_chain32.hip and csrc/gemm_dw.hip exist in the built objects and own no
    scratch (tools/scratch_audit.py)"""
    import importlib.util
    import os
    from factorizer_amd import build as Bld
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    Bld.build(verbose=False)
    spec = importlib.util.spec_from_file_location("scratch_audit", os.path.join(root, "tools", "scratch_audit.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ks = {name: (scratch, spills) for o in ("dropout.o", "mlp_chain32.o", "gemm_dw.o") for name, scratch, spills, _v in
          mod.kernels_of(os.path.join(root, "factorizer_amd", "csrc", "build", o))}
    want = ["dropout_bits_kernel"] + [f"dropout_apply_kernelI{t}Li{k}E" for t in ("f", "DF16b") for k in range(3)]
    # the fused launches' dropout instantiations (one trailing DropArgs argument)
    want += [f"gemm_chain_kernelILb0ELi2ELi2E{t}Lb1ELb1EJNS_8DropArgsE" for t in ("f", "DF16b")]
    want += [f"gemm_dw_kernelILb0E{t}JNS_8DropArgsE" for t in ("f", "DF16b")]
    for frag in want:
        hits = {k: v for k, v in ks.items() if frag in k}
        assert hits, (frag, sorted(ks))
        for name, (scratch, spills) in hits.items():
            assert scratch == 0 and spills == 0, (name, scratch, spills)
