"""-m gpu: every layer node of factorizer_amd/pointwise.py under DEFERRED finishes (pointwise._Defer), node by node, then at
block and model level through FlatAdamW at its defaults.

A deferred finish reads its partial-row workspace at the end-of-backward flush, long after the node returned: a buffer the
node's `_finish_scope` does not hold goes back to the caching allocator and is handed to the next node of the backward.  So
every node-level graph here is  y = node_b(node_a(x))  of two instances of the SAME Function with their own parameters:
node_b runs first in the backward and queues its finishes, node_a then allocates workspaces of the same sizes.

Assertions per configuration (fp32 and bf16 activations, one shape per kernel the wrapper dispatches to at small size, every
combination of optional arguments the device call accepts):
  bitwise   every gradient of the armed run `torch.equal`s the run with defer_finishes(False) — same arithmetic, no tolerance;
  deferred  `_Defer.flushed` grew by >= 1 job per node, `_Defer.refused` did not move, nothing is pending or kept afterwards;
  float64   every gradient of the armed run against the same two layers in float64 torch ops on the host, through
            parity.close at rel = 1e-4 (max-norm).  bf16 activations: the rule of tests/test_gpu_bf16.py — n stored tensors
            between input and result x u = 2^-8 — with that file's factors for the single layer (linear 1 / 1,
            LayerNorm+Linear 3 for the input gradient and 2 for the parameters, the convolutions 1 / 1; the other dense
            layers are linear layers in its sense) and the chain's own stores counted on top: node_b reads a stored y_a
            (+1), node_a receives node_b's input gradient (+ that gradient's own count).  The reference rounds y_a to
            bf16 where the device stores it (that file's rule for maps that are not of unit gain: node_b's ReLU gates;
            against the unrounded float64 chain the ReLU cases miss the count by 3-7x, through gates that the rounding of
            y_a flips).  The decoder node has no bf16 factor there;
            tests/test_gpu_upcat_bwd.py::test_bf16_storage_takes_the_old_launches states 2e-2 (5 u) for it.

Shapes are the small ones already proven in tests/test_gpu_dense.py, tests/test_gpu_bx.py and tests/test_gpu_upcat_bwd.py."""
import copy
import functools
import itertools
import warnings

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import factorizer_amd as ft
import parity as P
from factorizer_amd import _native as N
from factorizer_amd import blocks as BL
from factorizer_amd import pointwise as PW
from factorizer_amd.training import FlatAdamW

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
U = 2.0 ** -8   # bf16 unit roundoff


def _lin(x, w, b=None):
    return F.conv1d(x.flatten(2), w.reshape(w.shape[0], -1, 1), b).reshape(x.shape[0], w.shape[0], *x.shape[2:])


def _ln(x, g, bt, eps=1e-5):
    return F.layer_norm(x.movedim(1, -1), (x.shape[1],), g, bt, eps).movedim(-1, 1)


class Case:
    """one Function in one configuration: x0(r) the chain input, extra(r) a node's further activations, params(r) a node's
    parameters (None = the optional argument is absent), dev / ref (x, extras, params) -> y on the device through the public
    wrapper / in torch ops (any dtype), adapt(y) the cheap op between node_a and node_b where the shapes demand one.
    n_bf = (stores behind the input gradient, stores behind a parameter gradient) of the single layer in bf16."""

    def __init__(self, name, x0, params, dev, ref, extra=None, adapt=None, n_bf=(1, 1), share="w"):
        self.name, self.x0, self.params, self.dev, self.ref = name, x0, params, dev, ref
        self.extra = extra or (lambda r: {})
        self.adapt = adapt or (lambda y: y)
        self.n_bf, self.share = n_bf, share

    def __repr__(self):
        return self.name


def _on(names, p):
    """drop the parameters not in `names` (the optional arguments passed as None)"""
    return {k: (v if k in names else None) for k, v in p.items()}


def _dense_cases():
    out = []
    for C, B, S in ((32, 2, (8, 8, 8)), (64, 2, (8, 8, 8))):   # the C = 32 kernels | reduction length 64: the split-bf16 family
        x0 = lambda r, C=C, B=B, S=S: r(B, C, *S) * 2 + 0.5   # noqa: E731
        act = lambda r, C=C, B=B, S=S: r(B, C, *S)   # noqa: E731
        for bias, a in itertools.product((True, False), ("relu", "none")):   # ("relu_out" is "relu" whose gradient arrives gated)
            keep = {"g", "bt", "w"} | ({"b"} if bias else set())
            out.append(Case(
                f"ln_linear-{C}-{a}-{'b' if bias else 'nob'}", x0,
                lambda r, C=C, keep=keep: _on(keep, dict(g=r(C).abs() + 0.5, bt=r(C) * 0.3, w=r(C, C, 1) / C ** 0.5, b=r(C))),
                lambda x, e, p, a=a: PW.ln_linear(x, p["g"], p["bt"], 1e-5, p["w"], p["b"], a),
                lambda x, e, p, a=a: (torch.relu if a == "relu" else (lambda t: t))(_lin(_ln(x, p["g"], p["bt"]), p["w"], p["b"])),
                n_bf=(3, 2)))
        for bias, res, a in itertools.product((True, False), (True, False), ("gelu", "none")):
            out.append(Case(
                f"act_linear_res-{C}-{a}-{'b' if bias else 'nob'}-{'res' if res else 'nores'}", act,
                lambda r, C=C, bias=bias: _on({"w"} | ({"b"} if bias else set()), dict(w=r(C, C, 1) / C ** 0.5, b=r(C))),
                lambda x, e, p, a=a: PW.act_linear_res(x, p["w"], p["b"], e.get("res"), a),
                lambda x, e, p, a=a: _lin(F.gelu(x) if a == "gelu" else x, p["w"], p["b"]) + (e["res"] if "res" in e else 0),
                extra=(lambda r, C=C, B=B, S=S: {"res": r(B, C, *S)}) if res else None))
        for bias in (True, False):
            out.append(Case(
                f"cat_linear-{C}-{'b' if bias else 'nob'}", act,
                lambda r, C=C, bias=bias: _on({"w"} | ({"b"} if bias else set()), dict(w=r(C, 2 * C, 1) / (2 * C) ** 0.5, b=r(C))),
                lambda x, e, p: PW.cat_linear(x, e["x2"], p["w"], p["b"]),
                lambda x, e, p: _lin(torch.cat([x, e["x2"]], 1), p["w"], p["b"]),
                extra=lambda r, C=C, B=B, S=S: {"x2": r(B, C, *S)}))
            out.append(Case(
                f"linear-{C}-{'b' if bias else 'nob'}", act,
                lambda r, C=C, bias=bias: _on({"w"} | ({"b"} if bias else set()), dict(w=r(C, C, 1) / C ** 0.5, b=r(C))),
                lambda x, e, p: PW.linear_cf(x, p["w"], p["b"]),
                lambda x, e, p: _lin(x, p["w"], p["b"])))
        out.append(Case(
            f"layernorm-{C}", lambda r, C=C, B=B, S=S: r(B, C, *S) * 3 + 1,
            lambda r, C=C: dict(g=r(C).abs() + 0.5, bt=r(C)),
            lambda x, e, p: PW.layernorm_cf(x, p["g"], p["bt"], 1e-5),
            lambda x, e, p: _ln(x, p["g"], p["bt"]), share="g"))
    # the head (32 -> 3, no activation): input, weight and bias gradient in one pass (csrc/headbwd.hip), its rows reduced by two jobs
    for bias in (True, False):
        out.append(Case(
            f"act_linear_res-head3-{'b' if bias else 'nob'}", lambda r: r(1, 32, 8, 8, 8),
            lambda r, bias=bias: _on({"w"} | ({"b"} if bias else set()), dict(w=r(3, 32, 1) / 32 ** 0.5, b=r(3))),
            lambda x, e, p: PW.act_linear_res(x, p["w"], p["b"], None, "none"),
            lambda x, e, p: _lin(x, p["w"], p["b"]),
            adapt=lambda y: y.repeat(1, 11, 1, 1, 1)[:, :32]))
    return out


def _conv_cases():
    out = []
    up2 = lambda y: F.interpolate(y, scale_factor=2)   # noqa: E731  (nearest: a copy of each value, exact in every dtype)
    for bias in (True, False):
        kb = {"w"} | ({"b"} if bias else set())
        for Ci, Co, S in ((32, 64, (8, 8, 8)), (16, 16, (4, 6, 4))):
            prm = lambda r, Ci=Ci, Co=Co, kb=kb: _on(kb, dict(w=r(Co, Ci, 2, 2, 2) / (8 * Ci) ** 0.5, b=r(Co)))   # noqa: E731
            out.append(Case(
                f"conv_k2s2-{Ci}-{Co}-{'b' if bias else 'nob'}", lambda r, Ci=Ci, S=S: r(2, Ci, *S), prm,
                lambda x, e, p: PW.ConvK2S2Fn.apply(x, p["w"], p["b"]),
                lambda x, e, p: F.conv3d(x, p["w"], p["b"], stride=2),
                adapt=lambda y, Ci=Ci: up2(y[:, :Ci])))

            def skip_dev(x, e, p, Ci=Ci):
                skip, y = PW.SkipConvK2S2Fn.apply(x * 1.0, p["w"], p["b"])   # (a non-leaf, as in the encoder)
                return skip + up2(y[:, :Ci])
            out.append(Case(
                f"skip_conv_k2s2-{Ci}-{Co}-{'b' if bias else 'nob'}", lambda r, Ci=Ci, S=S: r(2, Ci, *S), prm, skip_dev,
                lambda x, e, p, Ci=Ci: x + up2(F.conv3d(x, p["w"], p["b"], stride=2)[:, :Ci])))
        for Ci, Co, S in ((64, 32, (4, 4, 4)), (32, 16, (2, 4, 2))):
            out.append(Case(
                f"tconv_k2s2-{Ci}-{Co}-{'b' if bias else 'nob'}", lambda r, Ci=Ci, S=S: r(2, Ci, *S),
                lambda r, Ci=Ci, Co=Co, kb=kb: _on(kb, dict(w=r(Ci, Co, 2, 2, 2) / Ci ** 0.5, b=r(Co))),
                lambda x, e, p: PW.TConvK2S2Fn.apply(x, p["w"], p["b"]),
                lambda x, e, p: F.conv_transpose3d(x, p["w"], p["b"], stride=2),
                adapt=lambda y: y[..., ::2, ::2, ::2].repeat(1, 2, 1, 1, 1)))
        # the stem: W % 32 == 0 takes the direct weight-gradient kernel (its own partial rows), W = 8 the generic tap loader
        for S in ((8, 8, 32), (8, 8, 8)):
            out.append(Case(
                f"conv_k3-4-32-W{S[2]}-{'b' if bias else 'nob'}", lambda r, S=S: r(2, 4, *S),
                lambda r, kb=kb: _on(kb, dict(w=r(32, 4, 3, 3, 3) / 5, b=r(32))),
                lambda x, e, p: PW.ConvK3Fn.apply(x, p["w"], p["b"]),
                lambda x, e, p: F.conv3d(x, p["w"], p["b"], padding=1),
                adapt=lambda y: y[:, :4]))
    return out


def _upcat_cases():
    """(3, 2, 64), B = 2 (SMALL[1] of tests/test_gpu_upcat_bwd.py): the one-pass backward in fp32, the three launches in bf16;
    (1, 2, 32) with 16 / 16 / 32 channels: outside the predicate, the three launches with their `_no_defer` site"""
    out = []
    for (S, C1, Cd), (bt, bad) in itertools.product((((3, 2, 64), 32, 64), ((1, 2, 32), 16, 32)), itertools.product((True, False), repeat=2)):
        fine = tuple(2 * d for d in S)
        keep = {"w_t", "w"} | ({"b_t"} if bt else set()) | ({"b"} if bad else set())
        out.append(Case(
            f"up_cat_linear-{C1}-{Cd}-{'bt' if bt else 'nobt'}-{'bad' if bad else 'nobad'}", lambda r, C1=C1, fine=fine: r(2, C1, *fine),
            lambda r, C1=C1, Cd=Cd, keep=keep: _on(keep, dict(w_t=r(Cd, C1, 2, 2, 2) * 0.2, b_t=r(C1) * 0.1, w=r(C1, 2 * C1, 1) * 0.2, b=r(C1) * 0.1)),
            lambda x, e, p: PW.up_cat_linear(x, e["deep"], p["w_t"], p["b_t"], p["w"], p["b"]),
            lambda x, e, p: _lin(torch.cat([x, F.conv_transpose3d(e["deep"], p["w_t"], p["b_t"], stride=2)], 1), p["w"], p["b"]),
            extra=lambda r, Cd=Cd, S=S: {"deep": r(2, Cd, *S)}, n_bf=(5, 5)))
    return out


DENSE, CONV, UPCAT = _dense_cases(), _conv_cases(), _upcat_cases()
CASES = DENSE + CONV + UPCAT


@functools.lru_cache(maxsize=None)
def _host(case, dt):
    """seeded host tensors of one chain (never modified): x0, per node extras and parameters, the output gradient; activations
    hold bf16-representable values when dt is bf16"""
    gen = torch.Generator().manual_seed(sum(map(ord, case.name)))
    r = lambda *sh: torch.randn(*sh, generator=gen)   # noqa: E731
    rd = (lambda t: t.to(BF).float()) if dt == BF else (lambda t: t)
    h = {"x0": rd(case.x0(r)), "ea": {k: rd(v) for k, v in case.extra(r).items()}, "eb": {k: rd(v) for k, v in case.extra(r).items()},
         "pa": case.params(r), "pb": case.params(r)}
    with torch.no_grad():
        y = case.ref(case.adapt(case.ref(h["x0"], h["ea"], h["pa"])), h["eb"], h["pb"])
    h["g"] = rd(torch.randn(y.shape, generator=gen))
    return h


def _leaves(h, to):
    """fresh leaves of a chain's tensors: {name: leaf}, names 'x0', 'a.<extra>', 'a.<param>', 'b....'"""
    lv = {"x0": to(h["x0"], True)}
    for n in "ab":
        lv.update({f"{n}.{k}": to(v, True) for k, v in h["e" + n].items()})
        lv.update({f"{n}.{k}": to(v, False) for k, v in h["p" + n].items() if v is not None})
    return lv


def _chain(case, fn, h, lv, shared=False, junction=lambda t: t):
    ea, eb = ({k: lv[f"{n}.{k}"] for k in h["e" + n]} for n in "ab")
    pa, pb = ({k: lv.get(f"{n}.{k}") for k in h["p" + n]} for n in "ab")
    if shared:
        pb[case.share] = pa[case.share]
    return fn(junction(case.adapt(fn(lv["x0"], ea, pa))), eb, pb)


def _stored_bf16(t):
    """the value a bf16 tensor holds, gradient passed straight through"""
    return t + (t.to(BF).to(t.dtype) - t).detach()


def _device_run(case, dt, defer, shared=False):
    """gradients of the chain on the device, deferral armed for its parameters (as FlatAdamW.zero_grad arms it) or off:
    ({name: gradient}, finishes flushed, nodes refused, finishes pending afterwards, buffers kept afterwards)"""
    h = _host(case, dt)
    lv = _leaves(h, lambda t, is_act: t.to(DEV, dt if is_act else torch.float32).requires_grad_(True))
    if shared:
        del lv["b." + case.share]
    params = [v for k, v in lv.items() if k != "x0" and k.split(".")[1] in h["pa"]]
    d = PW._Defer
    f0, r0 = d.flushed, d.refused
    PW.defer_finishes(defer)
    try:
        if defer:
            PW.arm_deferred_finishes(params)
        _chain(case, case.dev, h, lv, shared).backward(h["g"].to(DEV, dt))
        torch.cuda.synchronize()
        left = (N.lib().fz_finish_pending(), len(d.keep))
    finally:
        PW.defer_finishes(False)
    assert all(v.grad is not None for v in lv.values()), [k for k, v in lv.items() if v.grad is None]
    return {k: v.grad.detach().clone() for k, v in lv.items()}, d.flushed - f0, d.refused - r0, *left


@functools.lru_cache(maxsize=None)
def _float64(case, dt):
    h = _host(case, dt)
    lv = _leaves(h, lambda t, is_act: t.double().requires_grad_(True))
    # bf16: node_b's input is a STORED tensor.  The reference rounds it as the device does, so that node_b's ReLU gates (and
    # GELU) sit on the same values — tests/test_gpu_bf16.py's rule where the map between two stored tensors is not of unit gain
    _chain(case, case.ref, h, lv, junction=_stored_bf16 if dt == BF else (lambda t: t)).backward(h["g"].double())
    return {k: v.grad for k, v in lv.items()}


def _bound(case, dt, name):
    """(rel, why) of one gradient of the chain against float64"""
    if dt != BF:
        return 1e-4, None
    n_gx, n_par = case.n_bf
    # the junction costs one store on top of the single layer's: the device rounds y_a from its fp32 result and, where the op
    # between the nodes computes (skip + up(y)), a second time; the reference rounds a float64 value once
    if name == "x0" or name.startswith("a.") and name[2:] in _host(case, dt)["ea"]:
        n = 2 * n_gx + 1        # node_b's input gradient (n_gx, + the junction) feeds node_a's (n_gx)
    elif name.startswith("a."):
        n = n_par + n_gx + 1    # node_a's parameters see node_b's input gradient
    elif name[2:] in _host(case, dt)["eb"]:
        n = n_gx + 1
    else:
        n = n_par + 1           # node_b's parameters see the junction
    return n * U, f"bf16 storage: {n} stored tensor(s) x u = 2^-8 between input and this result (tests/test_gpu_bf16.py)"


@pytest.mark.parametrize("dt", [torch.float32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_node_deferred_behind_a_node_of_its_kind(case, dt):
    n0 = N.launch_count()
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)   # (a composed-ATen branch would warn: every case runs natively)
        g_def, flushed, refused, pending, kept = _device_run(case, dt, True)
        g_imm, flushed0, _, _, _ = _device_run(case, dt, False)
    assert N.launch_count() > n0
    print(f"{case} {dt}: {flushed} finishes flushed, {refused} nodes refused")
    for k in g_def:
        assert torch.equal(g_def[k], g_imm[k]), f"{case} {k}: the deferred bits differ from the immediate ones"
    assert flushed >= 2 and refused == 0 and flushed0 == 0, (flushed, refused, flushed0)   # >= one job per node
    assert pending == 0 and kept == 0, (pending, kept)
    ref = _float64(case, dt)
    for k in g_def:
        rel, why = _bound(case, dt, k)
        P.close(f"{case} {'bf16' if dt == BF else 'fp32'} d{k}", g_def[k], ref[k].reshape(g_def[k].shape), rel=rel, why=why)


SHARED = [next(c for c in DENSE if c.name == "ln_linear-64-relu-b"), next(c for c in CONV if c.name == "conv_k3-4-32-W32-b"),
          next(c for c in UPCAT if c.name == "up_cat_linear-32-64-nobt-bad")]


@pytest.mark.parametrize("case", SHARED, ids=repr)
def test_parameter_shared_by_both_nodes(case):
    """one parameter feeds node_a and node_b: node_a — second in the backward — is refused, the queue is flushed before the
    engine adds its gradient to node_b's, and the sum has the bits of the immediate run"""
    g_def, flushed, refused, pending, kept = _device_run(case, torch.float32, True, shared=True)
    g_imm, _, _, _, _ = _device_run(case, torch.float32, False, shared=True)
    assert refused == 1 and flushed >= 1 and pending == 0 and kept == 0, (refused, flushed, pending, kept)
    for k in g_def:
        assert torch.equal(g_def[k], g_imm[k]), (case, k)
    # ... and the sum is the right one: node_b's and node_a's gradient of the shared parameter in float64
    h = _host(case, torch.float32)
    lv = _leaves(h, lambda t, is_act: t.double().requires_grad_(True))
    del lv["b." + case.share]
    _chain(case, case.ref, h, lv, shared=True).backward(h["g"].double())
    k = "a." + case.share
    P.close(f"{case} shared d{k}", g_def[k], lv[k].grad.reshape(g_def[k].shape))


# ---------------------------------------------------------------- blocks --------------------------------------------------
def _graph_nodes(y):
    seen, todo, names = set(), [y.grad_fn], []
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.append(type(fn).__name__)
        todo.extend(f for f, _ in fn.next_functions)
    return names


def _armed_vs_immediate(params, step):
    """gradients of `step()` with deferral armed for `params` and switched off: (armed, immediate, flushed, refused)"""
    d = PW._Defer
    out = []
    try:
        for defer in (True, False):
            for p in params:
                p.grad = None
            f0, r0 = d.flushed, d.refused
            PW.defer_finishes(defer)
            if defer:
                PW.arm_deferred_finishes(params)
            extra = step()
            torch.cuda.synchronize()
            assert N.lib().fz_finish_pending() == 0 and not d.keep
            out.append(([p.grad.detach().clone() for p in params] + list(extra), d.flushed - f0, d.refused - r0))
    finally:
        PW.defer_finishes(False)
    return out[0][0], out[1][0], out[0][1], out[0][2]


def _swm_block(**kw):
    cfg = dict(channels=32, spatial_size=(8, 8, 8), norm=ft.LayerNorm, reshape=(ft.SWMatricize, {"head_dim": 8, "patch_size": 4}), act=nn.ReLU,
               factorize=ft.NMF, rank=1, num_iters=5, init="uniform", solver="hals", mlp_ratio=2, dropout=0.0)
    cfg.update(kw)
    return ft.FactorizerBlock(**cfg)


def _wide():
    """the configuration of tests/test_gpu_wide_nmf.py::test_num_heads_8_block_m_not_8: the reference's own Matricize, M = 16, N = 4096"""
    return _swm_block(spatial_size=(16, 16, 16), reshape=(ft.Matricize, {"num_heads": 2, "grid_size": 1}))


def _biased_in_proj():
    """FactMixer's constructor fixes in_proj to bias=False and FactorizerBlock hands MLP no `bias`, so the constructors cannot
    produce these layouts; a user gets them by replacing the sub-modules, as here: in_proj WITH a bias, an MLP without"""
    blk = _swm_block()
    blk.fact.in_proj = ft.Linear(32, 32, bias=True)
    blk.mlp = ft.MLP(32, ratio=2, bias=False)
    return blk


def _mu_one_factor():
    """solver "mu-0" updates one factor only: no native kernel takes it (nmf.MatrixFactorization._native_solver wants factor =
    (0, 1)), the NMF runs composed, the dense layers stay native and the block still passes _fusable.  (Every rank of the
    native solvers has a modular kernel at this size, so there is no rank that leaves the one-node path.)  A multiplicative
    update has no gate that a rounding could flip between host and device."""
    return _swm_block(solver="mu-0")


@pytest.mark.parametrize("make", [_wide, _biased_in_proj, _mu_one_factor], ids=lambda f: f.__name__.strip("_"))
def test_per_layer_block_defers(make):
    """blocks that are fusable but not one node run FactorizerBlock._per_layer: LNLinearFn (a float eps in front of its weight)
    twice, ActLinearResFn twice.  Host reference: the block's composed fp32 path on the CPU, as the neighbouring block tests
    use (tests/test_gpu_wide_nmf.py; the composed NMF is pinned against the reference's goldens in fp32)."""
    torch.manual_seed(1)
    blk = make()
    sp = (16, 16, 16) if make is _wide else (8, 8, 8)
    x, gy = torch.rand(2, 32, *sp), torch.rand(2, 32, *sp)
    xc = x.clone().requires_grad_(True)
    ref = torch.autograd.grad(blk(xc), [*blk.parameters(), xc], gy)
    blk = blk.to(DEV)
    names = [n for n, _ in blk.named_parameters()] + ["x"]
    params = list(blk.parameters())
    kinds = []

    def step():
        xd = x.to(DEV).requires_grad_(True)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")    # (a composed NMF on the device says so once)
            y = blk(xd)
        kinds.append(_graph_nodes(y))
        y.backward(gy.to(DEV))
        return [xd.grad]

    g_def, g_imm, flushed, refused = _armed_vs_immediate(params, step)
    assert kinds[0].count("LNLinearFnBackward") == 2 and kinds[0].count("ActLinearResFnBackward") == 2, kinds[0]
    assert "FactorizerBlockFnBackward" not in kinds[0]
    assert flushed >= 4 and refused == 0, (flushed, refused)   # one job or more per dense layer
    for n, a, b in zip(names, g_def, g_imm):
        assert torch.equal(a, b), n
    for n, a, b in zip(names, g_def, ref):
        P.close(f"{make.__name__} d{n}", a, b)


@pytest.mark.parametrize("dt", [torch.float32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("head", [False, True], ids=["plain", "fused-head"])
def test_one_node_blocks_defer(head, dt):
    """FactorizerBlockFn behind FactorizerBlockFn, without and with the network's head applied inside the second block's last
    launch (HeadOfBlockFn carries the head's gradients, with and without a head bias).  Host reference (fp32 activations): the
    blocks' composed fp32 path on the CPU, as tests/test_gpu_wide_nmf.py and tests/test_gpu_model.py use for blocks.  bf16: the
    bitwise comparison only — tests/test_gpu_bf16.py explains why a block in bf16 needs the oracle with storage roundings
    inserted (the gradient through the HALS iterations is not of unit gain), and holds that comparison."""
    for bias in ((True, False) if head else (True,)):
        torch.manual_seed(2)
        a, b = _swm_block(), _swm_block()
        hd = ft.Conv3d(32, 3, kernel_size=1, bias=bias)
        x, gy = torch.rand(2, 32, 8, 8, 8), torch.rand(2, 3 if head else 32, 8, 8, 8)
        mods = [a, b] + ([hd] if head else [])
        xc = x.clone().requires_grad_(True)
        yc = b(a(xc))
        ref = torch.autograd.grad(hd(yc) if head else yc, [p for m in mods for p in m.parameters()] + [xc], gy)
        for m in mods:
            m.to(DEV)
        params = [p for m in mods for p in m.parameters()]
        names = [f"{i}.{n}" for i, m in enumerate(mods) for n, _ in m.named_parameters()] + ["x"]
        kinds = []

        def step():
            xd = x.to(DEV, dt).requires_grad_(True)
            if head:
                with PW.HeadFusion(b, (hd.weight, hd.bias)) as slot:
                    b(a(xd))
                y = slot.logits
                assert y is not None
            else:
                y = b(a(xd))
            kinds.append(_graph_nodes(y))
            y.backward(gy.to(DEV, y.dtype))
            return [xd.grad]

        g_def, g_imm, flushed, refused = _armed_vs_immediate(params, step)
        assert kinds[0].count("FactorizerBlockFnBackward") == 2 and kinds[0].count("HeadOfBlockFnBackward") == int(head), kinds[0]
        assert flushed >= 2 + int(head) and refused == 0, (flushed, refused)
        for n, u, v in zip(names, g_def, g_imm):
            assert torch.equal(u, v), n
        if dt == torch.float32:
            for n, u, v in zip(names, g_def, ref):
                P.close(f"one-node blocks{' + head' if head else ''}{'' if bias else ' (no head bias)'} d{n}", u, v)


# ---------------------------------------------------------------- model ---------------------------------------------------
def _matricize_model(tconv_bias=True):
    return ft.Factorizer(in_channels=4, out_channels=3, spatial_size=(16, 16, 16), encoder_depth=(1, 1), encoder_width=(32, 64),
                         strides=(1, 2), decoder_depth=(1,), norm=ft.LayerNorm, reshape=(ft.Matricize, {"num_heads": 2, "grid_size": 1}),
                         upsample=(ft.ConvTranspose3d, {"kernel_size": 2, "bias": tconv_bias}),
                         act=nn.ReLU, factorize=ft.NMF, rank=1, num_iters=5, init="uniform", solver="hals", mlp_ratio=2, dropout=0.0)


def _data():
    gen = torch.Generator().manual_seed(5)
    return torch.rand(2, 4, 16, 16, 16, generator=gen), (torch.rand(2, 3, 16, 16, 16, generator=gen) > 0.5).float()


def _train_two_steps(host_model, deferred, amp=False, hook_on=None):
    """(gradients of step 1, parameters after step 2, finishes flushed, nodes refused, what the hook saw) under FlatAdamW"""
    model = copy.deepcopy(host_model).to(DEV)
    x, t = (v.to(DEV) for v in _data())
    d = PW._Defer
    PW.defer_finishes(False)    # (the switch is process-wide: an optimizer built with deferred_finishes=False leaves it as it is)
    saw = []
    try:
        opt = FlatAdamW(model, lr=1e-3, deferred_finishes=deferred)
        assert d.enabled == deferred
        if hook_on is not None:
            dict(model.named_parameters())[hook_on].register_post_accumulate_grad_hook(lambda p: saw.append(p.grad.clone()))
        f0, r0 = d.flushed, d.refused
        g1 = None
        for _ in range(2):
            opt.zero_grad()
            with torch.autocast("cuda", dtype=BF, enabled=amp):
                loss = ft.dice_ce_loss(model(x), t)
            loss.backward()
            torch.cuda.synchronize()
            assert N.lib().fz_finish_pending() == 0 and not d.keep
            if g1 is None:
                g1 = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
                kinds = _graph_nodes(loss)
            opt.step()
        torch.cuda.synchronize()
        return g1, {n: p.detach().clone() for n, p in model.named_parameters()}, d.flushed - f0, d.refused - r0, saw, kinds
    finally:
        PW.defer_finishes(False)


@pytest.mark.parametrize("variant", ["tconv-bias", "tconv-nobias", "tconv-nobias-one-node-level"])
def test_matricize_model_trains_under_flat_adamw_defaults(variant, monkeypatch):
    """a two-stage Factorizer whose every block uses the reference's own ft.Matricize (so every block takes _per_layer), two
    steps under FlatAdamW(model) at its defaults against deferred_finishes=False; with a bias-less transposed convolution in
    the decoder, and with the decoder level as ONE node (UpCatLinearFn with b_t = None: its size threshold lowered to reach
    it at 16^3).  Host reference of the step-1 gradients: the same model's composed fp32 path on the CPU (the path
    tests/test_gpu_model.py compares models with; the composed NMF is not written for float64 buffers)."""
    if variant.endswith("one-node-level"):
        monkeypatch.setattr(BL, "_UP_FUSED_MIN", 1)
    torch.manual_seed(3)
    host = _matricize_model(tconv_bias=variant == "tconv-bias")
    g_def, p_def, flushed, refused, _, kinds = _train_two_steps(host, True)
    g_imm, p_imm, flushed0, _, _, _ = _train_two_steps(host, False)
    assert kinds.count("LNLinearFnBackward") == 6 and "FactorizerBlockFnBackward" not in kinds, kinds   # 3 blocks x 2
    assert ("UpCatLinearFnBackward" in kinds) == variant.endswith("one-node-level"), kinds
    assert flushed >= 12 and refused == 0 and flushed0 == 0, (flushed, refused, flushed0)
    for n in g_def:
        assert torch.equal(g_def[n], g_imm[n]), n
        assert torch.equal(p_def[n], p_imm[n]), n
    x, t = _data()
    ft.dice_ce_loss(host(x), t).backward()
    for n, p in host.named_parameters():
        P.close(f"Matricize model [{variant}] d{n}", g_def[n], p.grad)


def test_matricize_model_under_autocast_is_bit_identical():
    torch.manual_seed(3)
    host = _matricize_model(tconv_bias=False)
    g_def, p_def, flushed, refused, _, _ = _train_two_steps(host, True, amp=True)
    g_imm, p_imm, _, _, _, _ = _train_two_steps(host, False, amp=True)
    assert flushed >= 12 and refused == 0, (flushed, refused)
    for n in g_def:
        assert torch.equal(g_def[n], g_imm[n]), n
        assert torch.equal(p_def[n], p_imm[n]), n


def test_post_accumulate_grad_hook_sees_the_finished_gradient():
    """a stranger's post-accumulate-grad hook clones p.grad inside the backward: its node must not defer"""
    torch.manual_seed(3)
    host = _matricize_model()
    name = "encoder.blocks.1.block.blocks.0.fact.in_proj.linear.weight"
    assert name in dict(host.named_parameters())
    g1, _, flushed, refused, saw, _ = _train_two_steps(host, True, hook_on=name)
    assert len(saw) == 2 and refused >= 2 and flushed > 0, (len(saw), refused, flushed)   # (one refusal per step)
    g_imm, _, _, _, _, _ = _train_two_steps(host, False)
    assert torch.equal(saw[0], g1[name]) and torch.equal(saw[0], g_imm[name])
