"""No GPU, no library: the launches of the FactorizerBlock node and of the launch wrappers under it, pinned.

(a) Node level.  FactorizerBlockFn.forward / backward run on CPU tensors against a stand-in ctx; the launch layer below them
(`_gemm`, `_wgrad`, `_wgrad_group`, `_gemm_dw`, `_dgrad_lnbwd`, the four MLP-chain wrappers, the core and the dropout passes) is
replaced by recorders, and the branch predicates are monkeypatched through the combinations a device allows.  Every call is
recorded as (kind, operands by role, keyword arguments), with the tuple handed to save_for_backward and the returned gradients.

(b) Descriptor level.  The four MLP-chain wrappers, `_dgrad_lnbwd` and the head backward run against a fake `N.lib()` whose entry
points record their arguments: every field of every descriptor at the moment of the call, pointers replaced by the role of the
tensor they point into, and the (name, bytes, columns, flops) of every timed launch — bench.py keys its stage table on them.

The kernels see only what these layers put into their descriptors, so equal records are equal device results.  EXPECTED was
written down from these recorders run on pointwise.py as it stood BEFORE the block node's branches and the wrappers' descriptor
blocks were folded, and is not to be regenerated from the code under test.

Tensors: a role name is an operand the test passed in or a stand-in's output ("<kind><call>.<output>"); "new<k>[shape,dtype]" is
a tensor the code under test allocated, numbered by first appearance in the record; "role+n" is n bytes into it; "role@shape" is
a view of another shape."""
import contextlib
import ctypes
import inspect
import weakref

import pytest
import torch

from factorizer_amd import _native as N
from factorizer_amd import functional as Fn
from factorizer_amd import pointwise as PW

B, C, HD, SP = 1, 32, 64, (2, 2, 4)
V = 16


_DT = {torch.float32: "f32", torch.bfloat16: "bf16", torch.int32: "i32", torch.int64: "i64"}


def _dims(t):
    return "x".join(str(n) for n in t.shape)


class _Geo:
    nshift = 2


GEO = _Geo()


class _Names:
    """tensor / pointer -> role.  Everything torch.empty / empty_like / zeros / zeros_like hands out while the code under test runs
    is registered (and kept alive, so no address is used twice); it gets its number when a record first mentions it."""

    def __init__(self, monkeypatch):
        self.reg = []   # [tensor, name or None, given]
        self.new = 0
        for fn in ("empty", "empty_like", "zeros", "zeros_like"):
            monkeypatch.setattr(torch, fn, self._hook(getattr(torch, fn)))

    def _hook(self, orig):
        def alloc(*a, **kw):
            t = orig(*a, **kw)
            self.reg.append([t, None, False])
            return t
        return alloc

    def add(self, name, t):
        if t is not None:
            self.reg.append([t, name, True])
        return t

    def ptr(self, p):
        """(role of the address p, the registered tensor it lies in)"""
        if p is None:
            return None, None
        for e in self.reg:
            lo = e[0].data_ptr()
            if lo <= p < lo + max(e[0].numel() * e[0].element_size(), 1):
                if e[1] is None:
                    self.new += 1
                    e[1] = f"new{self.new}"
                base = e[1] if e[2] else f"{e[1]}[{_dims(e[0])},{_DT[e[0].dtype]}]"
                return (base if p == lo else f"{base}+{p - lo}"), e[0]
        return "unregistered", None

    def d(self, v):
        if isinstance(v, torch.Tensor):
            r, t = self.ptr(v.data_ptr())
            if t is None:
                return f"{r}[{_dims(v)},{_DT[v.dtype]}]"
            return r if v.shape == t.shape else f"{r}@{_dims(v)}"
        if v is GEO:
            return "geo"
        if isinstance(v, PW._Ctx):
            return "ctx"
        if isinstance(v, weakref.ref):
            return self.d(v())
        if isinstance(v, torch.Size):
            return tuple(v)
        if isinstance(v, (tuple, list)):
            return type(v)(self.d(e) for e in v)
        if isinstance(v, dict):
            return {k: self.d(e) for k, e in v.items()}
        if isinstance(v, (torch.dtype, torch.device)):
            return str(v)
        return v


# ---- (a) node level ------------------------------------------------------------------------------------------------------------
class _NodeCtx(PW._Ctx):
    needs_input_grad = (True,) * 19

    def __init__(self):
        self.marks = []

    def mark_non_differentiable(self, *ts):
        self.marks.append(("mark_non_differentiable", ts))

    def set_materialize_grads(self, flag):
        self.marks.append(("set_materialize_grads", flag))


# the defaults of `_gemm` / `_wgrad`: a keyword passed with its default value is the same launch as one not passed, and is not recorded
_GEMM_DEFAULTS = dict(w_t=False, ldw=None, bias=None, ln=None, stats_out=None, bact=0, bmul=None, bmul_kind=0, eact=0, res=None, emul=None,
                      emul_kind=0, src_mode=0, c0=0, loader=0, epilogue=0, Di=0, Hi=0, Wi=0, Ho=0, Wo=0, name="gemm", tune=0)
_WGRAD_DEFAULTS = dict(gbias=None, pmul=None, pmul_kind=0, src_mode=0, c0=0, stats=None, qact=0, ln=None, loader=0, D=0, H=0, W=0, Ho=0,
                       Wo=0, accumulate=False, name="wgrad")
_STUB_DEFAULTS = {   # of the stand-ins' originals, written down here so that a changed default shows
    "gemm_dw": dict(ln=None, stats=None, gadd=None, want_bias=False, name="dgrad_wgrad", gw_out=None, gb_out=None, drop=None),
    "outproj_mlp_fwd_chain": dict(head=None, drop=None), "swm_fwd_raw": dict(relu=False, div=1),
    "swm_inv_raw": dict(average=True, gate=None), "nmf_fwd_raw": dict(want_uv=False), "dropout_apply": dict(aux=None),
}


def _passed(kw, defaults):
    return {k: v for k, v in kw.items() if not (k in defaults and (v is defaults[k] or (not isinstance(v, torch.Tensor) and v == defaults[k])))}


class _NodeRecorder:
    def __init__(self, monkeypatch, names):
        self.calls, self.names, self.n = [], names, {}
        self.empty = torch.empty   # (hooked: what a stand-in returns is registered, then named below)
        mp = monkeypatch
        mp.setattr(PW, "_gemm", self.gemm)
        mp.setattr(PW, "_wgrad", self.wgrad)
        mp.setattr(PW, "_wgrad_group", self.wgrad_group)
        for name, outs in (("_gemm_dw", self.o_gemm_dw), ("_dgrad_lnbwd", self.o_dgrad_lnbwd), ("_mlp_fwd_chain", self.o_mlp_fwd),
                           ("_outproj_mlp_fwd_chain", self.o_outproj), ("_mlp_bwd_chain", self.o_mlp_bwd),
                           ("_mlp_bwd_chain_wgrad", self.o_mlp_bwd_wg)):
            mp.setattr(PW, name, self.stub(name.lstrip("_"), getattr(PW, name), outs))
        for name, outs in (("_swm_fwd_raw", self.o_swm_fwd), ("_swm_inv_raw", self.o_swm_inv), ("_nmf_fwd_raw", self.o_nmf_fwd),
                           ("_nmf_bwd_raw", self.o_nmf_bwd), ("dropout_seed", self.o_seed), ("dropout_keep_bits", self.o_bits),
                           ("dropout_apply", self.o_apply)):
            mp.setattr(Fn, name, self.stub(name.lstrip("_"), getattr(Fn, name), outs))
        mp.setattr(Fn.FactCoreFn, "forward", staticmethod(self.stub("core_fwd", Fn.FactCoreFn.forward, self.o_core_fwd)))
        mp.setattr(Fn.FactCoreFn, "backward", staticmethod(self.stub("core_bwd", Fn.FactCoreFn.backward, self.o_core_bwd)))
        mp.setattr(torch.cuda, "current_stream", lambda dev=None: "stream")

    def gemm(self, xs, w, y, **kw):
        d = self.names.d
        self.calls.append(("gemm", d(list(xs)), d(w), d(y), d(_passed(kw, _GEMM_DEFAULTS))))
        return y

    def wgrad(self, p, qs, gw, **kw):
        d = self.names.d
        self.calls.append(("wgrad", d(p), d(list(qs)), d(gw), d(_passed(kw, _WGRAD_DEFAULTS))))
        return gw

    def wgrad_group(self, problems, name):
        d = self.names.d
        self.calls.append(("wgrad_group", [(d(p), d(list(qs)), d(gw), d(_passed(kw, _WGRAD_DEFAULTS))) for p, qs, gw, kw in problems], name))

    def stub(self, kind, orig, outs):
        """a stand-in of `orig`: records the arguments by parameter name (those that differ from the parameter's default), returns
        what `outs` makes of them — {output name: tensor}, registered as '<kind><call number>.<output name>'"""
        sig = inspect.signature(orig)
        defaults = _STUB_DEFAULTS.get(kind, {})

        def call(*a, **kw):
            args = _passed(dict(sig.bind(*a, **kw).arguments), defaults)
            k = self.n[kind] = self.n.get(kind, 0) + 1
            if kind == "core_bwd":   # what the block handed over in the stand-in ctx
                args["ctx"] = {"saved_tensors": args["ctx"].saved_tensors, "cfg": args["ctx"].cfg}
            self.calls.append((kind, self.names.d(args)))
            res = outs(**args)
            for e in self.names.reg:
                for name, t in res.items():
                    if e[0] is t:
                        e[1], e[2] = f"{kind}{k}.{name}", True
            vals = tuple(res.values())
            return vals[0] if len(vals) == 1 and kind not in ("core_bwd",) else vals
        return call

    def like(self, t, ch=None, dtype=None):
        return self.empty((t.shape[0], t.shape[1] if ch is None else ch, *t.shape[2:]), dtype=dtype or t.dtype)

    def f32(self, *shape):
        return self.empty(shape, dtype=torch.float32)

    def o_gemm_dw(self, g, w2, q, ln=None, want_bias=False, **kw):
        return dict(y=self.like(q), gw=self.f32(C, C), gb=self.f32(C) if want_bias else None,
                    gg=self.f32(C) if ln is not None else None, gbt=self.f32(C) if ln is not None else None)

    def o_dgrad_lnbwd(self, gz, w2, x, stats, ln_w, gadd):
        return dict(gx=self.like(x), gg=self.f32(x.shape[1]), gbt=self.f32(x.shape[1]))

    def o_mlp_fwd(self, x1, w12, **kw):
        return dict(x2=self.like(x1), z1=self.like(x1, w12.shape[0]), st=self.f32(B, 2, V))

    def o_outproj(self, a, w12, head=None, **kw):
        out = dict(x1=self.like(a), x2=self.like(a), z1=self.like(a, w12.shape[0]), st=self.f32(B, 2, V))
        if head is not None:
            out["logits"] = self.like(a, head[0].shape[0])
        return out

    def o_mlp_bwd(self, g2, z1, w12, w22, x1, st, ln_w):
        return dict(gz1=self.like(z1), gx1=self.like(x1), gg=self.f32(C), gbt=self.f32(C))

    def o_mlp_bwd_wg(self, g2, z1, w12, w22, x1, st, ln_w, ln_b):
        return dict(gx1=self.like(x1), gg=self.f32(C), gbt=self.f32(C), gw1=self.f32(HD, C), gb1=self.f32(HD),
                    gw2=self.f32(C, HD), gb2=self.f32(C))

    def o_swm_fwd(self, x, geo, **kw):
        return dict(m=self.empty((B, 4, 8, 16), dtype=x.dtype))

    def o_swm_inv(self, y, geo, **kw):
        return dict(out=self.empty((B, C, *SP), dtype=y.dtype))

    def o_nmf_fwd(self, x, **kw):
        return dict(y=self.empty(x.shape, dtype=x.dtype), u=None, v=None)

    def o_nmf_bwd(self, x, **kw):
        return dict(gx=self.empty(x.shape, dtype=x.dtype))

    def o_seed(self, device):
        return dict(seed=self.empty((1,), dtype=torch.int64))

    def o_bits(self, seed, site, B, ch, V, p):
        return dict(bits=self.empty((B, ch, (V + 31) // 32), dtype=torch.int32))

    def o_apply(self, kind, bits, p, t, aux=None):
        return dict(out=self.like(t))

    def o_core_fwd(self, ctx, t, **kw):
        return dict(a=self.like(t))

    def o_core_bwd(self, ctx, ga):
        return dict(gt=self.like(ga))


# predicates: chain = _mlp_chain_ok, outproj = _outproj_mlp_ok, dropok = _mlp_drop_ok, wgf = _mlp_wgrad_fused_ok, dw = _dw_fused_ok.
# Only what a device allows: dropok implies outproj implies chain; wgf implies chain; a head comes with outproj, the fused core and
# no dropout; t_pre comes with the fused core.  P = the dropout probability of a live site (three different ones in "ppp").
NODE_DEFAULTS = dict(chain=False, outproj=False, dropok=False, wgf=False, dw=False, group=True, core=True, drop=None, head=False,
                     t_pre=False, G=1, g2_none=False)
P = 0.25
NODE_CASES = {
    # (arms as they stood before the fold: five in the forward's steps 3 + 4, three in the backward's MLP section)
    # case                forward arm (steps 3 + 4)                        backward MLP section                          rest of the backward
    # plain               two plain GEMMs (the last arm)                   no-dropout arm without the chain              GEMMs, one grouped wgrad launch
    # chain               out-projection GEMM + _mlp_fwd_chain             no-dropout arm with _mlp_bwd_chain            fz_gemm_dw pair, single wgrad launches
    # chain-wgf           out-projection GEMM + _mlp_fwd_chain             _mlp_bwd_chain_wgrad arm                      GEMMs, grouped launch of the other two
    # outproj             _outproj_mlp_fwd_chain                           no-dropout arm with _mlp_bwd_chain            GEMMs, one grouped wgrad launch
    # outproj-head        _outproj_mlp_fwd_chain with head=, t_pre         _mlp_bwd_chain_wgrad arm                      fz_gemm_dw pair, no wgrad launch left
    # drop-ppp-fused      _outproj_mlp_fwd_chain with drop=                dropout arm (wgf holds too), all sites        m0 inside fz_gemm_dw
    # drop-p00            unfused dropout tail, site 0                     dropout arm, no site of the MLP live          m0 as a pass of its own
    # drop-0p0            unfused dropout tail, site 1                     dropout arm, m1: dgrad + two dropout passes   fz_gemm_dw pair
    # drop-00p            unfused dropout tail, site 2; modular core       dropout arm, m2                               modular core, single wgrad launches
    # G0-modular-g2none   two plain GEMMs; modular core                    a missing output gradient is a zero one       G = 0: no core backward
    "plain": dict(),
    "chain": dict(chain=True, dw=True, group=False),
    "chain-wgf": dict(chain=True, wgf=True),
    "outproj": dict(chain=True, outproj=True),
    "outproj-head": dict(chain=True, outproj=True, dropok=True, wgf=True, dw=True, t_pre=True, head=True),
    "drop-ppp-fused": dict(chain=True, outproj=True, dropok=True, wgf=True, dw=True, drop=(0.1, 0.2, 0.3)),
    "drop-p00": dict(drop=(P, 0, 0)),
    "drop-0p0": dict(chain=True, outproj=True, dw=True, drop=(0, P, 0)),
    "drop-00p": dict(drop=(0, 0, P), group=False, core=False),
    "G0-modular-g2none": dict(core=False, G=0, g2_none=True),
}


def _node_operands(c):
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    ops = dict(x=r(B, C, *SP), n1w=r(C), n1b=r(C), win=r(C, C, 1, 1, 1), u0=r(4, 8, 1), v0=r(4, 16, 1), wout=r(C, C, 1, 1, 1), bout=r(C),
               n2w=r(C), n2b=r(C), w1=r(HD, C, 1, 1, 1), b1=r(HD), w2=r(C, HD, 1, 1, 1), b2=r(C))
    ops["head_w"], ops["head_b"] = (r(3, C, 1, 1, 1), r(3)) if c["head"] else (None, None)
    ops["t_pre"], ops["st_pre"] = (r(B, C, *SP), r(B, 2, V)) if c["t_pre"] else (None, None)
    return ops


def _patch_predicates(monkeypatch, c):
    for name, key in (("_mlp_chain_ok", "chain"), ("_outproj_mlp_ok", "outproj"), ("_mlp_drop_ok", "dropok"),
                      ("_mlp_wgrad_fused_ok", "wgf"), ("_dw_fused_ok", "dw")):
        monkeypatch.setattr(PW, name, lambda *a, _v=c[key]: _v)
    monkeypatch.setattr(PW, "_WGRAD_GROUP", c["group"])
    monkeypatch.delenv("FZ_SIDE_WGRAD", raising=False)
    monkeypatch.setattr(PW._Defer, "armed", False)   # (whatever an earlier test of the process left behind)


def _trace_node(monkeypatch, case):
    c = dict(NODE_DEFAULTS, **NODE_CASES[case])
    ops = _node_operands(c)
    g2 = None if c["g2_none"] else torch.randn(B, C, *SP)
    _patch_predicates(monkeypatch, c)
    names = _Names(monkeypatch)
    for k, t in ops.items():
        names.add(k, t)
    names.add("g2", g2)
    rec = _NodeRecorder(monkeypatch, names)
    cfg = dict(geo=GEO, T=5, G=c["G"], solver=1, nmf_eps=1e-16, eps1=1e-5, eps2=1e-6, core=c["core"])
    if c["drop"] is not None:
        cfg["drop"] = c["drop"]
    ctx = _NodeCtx()
    o = ops
    res = PW.FactorizerBlockFn.forward(ctx, o["x"], o["n1w"], o["n1b"], o["win"], o["u0"], o["v0"], o["wout"], o["bout"], o["n2w"],
                                       o["n2b"], o["w1"], o["b1"], o["w2"], o["b2"], cfg, o["head_w"], o["head_b"], o["t_pre"],
                                       o["st_pre"])
    d = names.d
    out = dict(fwd=rec.calls, out=d(res if isinstance(res, tuple) else (res,)), saved=d(tuple(ctx.saved_tensors)), marks=d(ctx.marks),
               shapes=d(ctx.shapes), prm=d(ctx.prm))
    rec.calls = []
    grads = PW.FactorizerBlockFn.backward(ctx, g2, None) if c["head"] else PW.FactorizerBlockFn.backward(ctx, g2)
    out.update(bwd=rec.calls, grads=d(grads))
    return out


@pytest.mark.parametrize("case", list(NODE_CASES))
def test_block_node_launches_are_the_recorded_ones(monkeypatch, case):
    assert _trace_node(monkeypatch, case) == EXPECTED_NODE[case]


def test_a_head_outside_the_out_projection_chain_is_refused(monkeypatch):
    c = dict(NODE_DEFAULTS, chain=True, dw=True, head=True)
    o = _node_operands(c)
    _patch_predicates(monkeypatch, c)
    _NodeRecorder(monkeypatch, _Names(monkeypatch))
    cfg = dict(geo=GEO, T=5, G=1, solver=1, nmf_eps=1e-16, eps1=1e-5, eps2=1e-6, core=True)
    with pytest.raises(RuntimeError, match="head fusion asked for a configuration outside fz_mlp_pre_supported"):
        PW.FactorizerBlockFn.forward(_NodeCtx(), o["x"], o["n1w"], o["n1b"], o["win"], o["u0"], o["v0"], o["wout"], o["bout"], o["n2w"],
                                     o["n2b"], o["w1"], o["b1"], o["w2"], o["b2"], cfg, o["head_w"], o["head_b"], None, None)


# ---- (b) descriptor level ------------------------------------------------------------------------------------------------------
_RETURNS = {"fz_mlp_partials": 3, "fz_gemm_lnbwd_partials": 5, "fz_mlp_wgrad_workspace_bytes": 4096, "fz_head_bwd_rows": 7,
            "fz_head_bwd_workspace_bytes": 7 * 132 * 4, "fz_ln_bwd_workspace_bytes2": 1024}
_ENTRY_POINTS = ("fz_mlp_chain", "fz_mlp_chain_drop", "fz_gemm", "fz_gemm_lnbwd_partials", "fz_mlp_partials",
                 "fz_mlp_wgrad_workspace_bytes", "fz_reduce_rows", "fz_head_bwd_rows", "fz_head_bwd_workspace_bytes", "fz_head_bwd",
                 "fz_chunk_reduce_ld", "fz_ln_bwd", "fz_ln_bwd_workspace_bytes2")


class _FakeLib:
    """N.lib() stand-in: every entry point records (name, arguments) and returns 0, or the row / byte count of _RETURNS.  An
    argument the binding declares as a pointer becomes the role of what it points into; a descriptor becomes {field: value}."""

    def __init__(self, monkeypatch, names):
        self.calls, self.names = [], names
        monkeypatch.setattr(N, "lib", lambda: self)
        monkeypatch.setattr(N, "stream_ptr", lambda t: "stream")
        monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
        monkeypatch.setattr(Fn, "_timed", self.timed)

    def timed(self, name, nbytes, fn, cols=0, flops=0):
        self.calls.append(("timed", name, nbytes, cols, flops))
        return fn()

    def value(self, v, pointer):
        if isinstance(v, ctypes.Array):
            return [self.value(e, pointer) for e in v]
        return self.names.ptr(v)[0] if pointer and v is not None else v

    def desc(self, s):
        return {f: self.value(getattr(s, f), t is ctypes.c_void_p or (isinstance(t, type) and issubclass(t, ctypes.Array)))
                for f, t in s._fields_}

    def __getattr__(self, name):
        if name not in _ENTRY_POINTS:
            raise AttributeError(name)
        argtypes = N._SIGS[name][0]

        def entry(*args):
            assert len(args) == len(argtypes), name
            rec = []
            for a, t in zip(args, argtypes):
                if hasattr(a, "_obj"):     # ctypes.byref(descriptor)
                    rec.append(self.desc(a._obj))
                else:
                    rec.append(self.value(a, t is ctypes.c_void_p and a != "stream"))
            self.calls.append((name, rec))
            return _RETURNS.get(name, 0)
        return entry


def _randn(g, dtype, *shape):
    return torch.randn(*shape, generator=g).to(dtype)


def _mlp_operands(dtype, Hd=HD, bias=True):
    g = torch.Generator().manual_seed(1)
    f = torch.float32
    return dict(x1=_randn(g, dtype, B, C, *SP), a=_randn(g, dtype, B, C, *SP), x=_randn(g, dtype, B, C, *SP), g2=_randn(g, dtype, B, C, *SP),
                z1=_randn(g, dtype, B, Hd, *SP), st=_randn(g, f, B, 2, V), ln_w=_randn(g, f, C), ln_b=_randn(g, f, C),
                w12=_randn(g, f, Hd, C), w22=_randn(g, f, C, Hd), wout2=_randn(g, f, C, C),
                b1=_randn(g, f, Hd) if bias else None, b2=_randn(g, f, C) if bias else None, bout=_randn(g, f, C) if bias else None,
                hw=_randn(g, f, 3, C), hb=_randn(g, f, 3) if bias else None,
                m0=torch.zeros((B, C, 1), dtype=torch.int32), m1=torch.zeros((B, Hd, 1), dtype=torch.int32),
                m2=torch.zeros((B, C, 1), dtype=torch.int32))


def _d_mlp_fwd(o, **kw):
    return PW._mlp_fwd_chain(o["x1"], o["ln_w"], o["ln_b"], 1e-6, o["w12"], o["b1"], o["w22"], o["b2"])


def _d_outproj(o, head=False, drop=None):
    kw = {}
    if head:
        kw["head"] = (o["hw"], o["hb"])
    if drop is not None:
        kw["drop"] = (tuple(o[f"m{s}"] if p else None for s, p in enumerate(drop)), drop)
    return PW._outproj_mlp_fwd_chain(o["a"], o["wout2"], o["bout"], o["x"], o["ln_w"], o["ln_b"], 1e-6, o["w12"], o["b1"], o["w22"],
                                     o["b2"], **kw)


def _d_mlp_bwd(o):
    return PW._mlp_bwd_chain(o["g2"], o["z1"], o["w12"], o["w22"], o["x1"], o["st"], o["ln_w"])


def _d_mlp_bwd_wg(o):
    return PW._mlp_bwd_chain_wgrad(o["g2"], o["z1"], o["w12"], o["w22"], o["x1"], o["st"], o["ln_w"], o["ln_b"])


def _lnbwd_operands(dtype, Cx, Mz, gadd=True):
    g = torch.Generator().manual_seed(2)
    f = torch.float32
    return dict(gz=_randn(g, dtype, B, Mz, *SP), w2=_randn(g, f, Mz, Cx), x=_randn(g, dtype, B, Cx, *SP), stats=_randn(g, f, B, 2, V),
                ln_w=_randn(g, f, Cx), gadd=_randn(g, dtype, B, Cx, *SP) if gadd else None)


def _d_lnbwd(o):
    return PW._dgrad_lnbwd(o["gz"], o["w2"], o["x"], o["stats"], o["ln_w"], o["gadd"])


def _head_operands(dtype, g_dtype=None, bias=True, res=True):
    g = torch.Generator().manual_seed(3)
    return dict(gy=_randn(g, g_dtype or dtype, B, 3, *SP), z=_randn(g, dtype, B, C, *SP), w=_randn(g, torch.float32, 3, C, 1, 1, 1),
                bias=bias, res=res)


def _d_head_act(o):
    ctx = PW._Ctx()
    ctx.save_for_backward(o["z"], o["w"].reshape(3, C))
    ctx.bact, ctx.has_bias, ctx.has_res, ctx.wshape = "none", o["bias"], o["res"], o["w"].shape
    return PW.ActLinearResFn.backward(ctx, o["gy"])


def _d_head_block(o):
    ctx = PW._Ctx()
    ctx.save_for_backward(o["z"], o["w"])
    ctx.has_bias, ctx.wshape = o["bias"], o["w"].shape
    return PW.HeadOfBlockFn.backward(ctx, o["gy"])


f32, bf16 = torch.float32, torch.bfloat16
DESC_CASES = {
    "mlp_fwd-f32": (_mlp_operands, dict(dtype=f32), _d_mlp_fwd, {}),
    "mlp_fwd-bf16-nobias": (_mlp_operands, dict(dtype=bf16, bias=False), _d_mlp_fwd, {}),
    "outproj-f32": (_mlp_operands, dict(dtype=f32), _d_outproj, {}),
    "outproj-bf16-nobias-head": (_mlp_operands, dict(dtype=bf16, bias=False), _d_outproj, dict(head=True)),
    "outproj-f32-drop-p0p": (_mlp_operands, dict(dtype=f32), _d_outproj, dict(drop=(0.1, 0, 0.3))),
    "mlp_bwd-f32": (_mlp_operands, dict(dtype=f32), _d_mlp_bwd, {}),
    "mlp_bwd-bf16": (_mlp_operands, dict(dtype=bf16), _d_mlp_bwd, {}),
    "mlp_bwd_wg-f32-h64": (_mlp_operands, dict(dtype=f32), _d_mlp_bwd_wg, {}),
    "mlp_bwd_wg-bf16-h128": (_mlp_operands, dict(dtype=bf16, Hd=128), _d_mlp_bwd_wg, {}),
    "lnbwd-fused32-f32-nogadd": (_lnbwd_operands, dict(dtype=f32, Cx=32, Mz=64, gadd=False), _d_lnbwd, {}),
    "lnbwd-fused64-bf16": (_lnbwd_operands, dict(dtype=bf16, Cx=64, Mz=64), _d_lnbwd, {}),
    "lnbwd-two-launches-f32": (_lnbwd_operands, dict(dtype=f32, Cx=64, Mz=128), _d_lnbwd, {}),
    "head-act_linear_res-f32": (_head_operands, dict(dtype=f32), _d_head_act, {}),
    "head-of_block-bf16-f32grad-nobias": (_head_operands, dict(dtype=bf16, g_dtype=f32, bias=False), _d_head_block, {}),
}


def _trace_desc(monkeypatch, case):
    make, okw, run, rkw = DESC_CASES[case]
    ops = make(**okw)
    monkeypatch.setattr(PW, "_HEAD_BWD", True)
    monkeypatch.setattr(PW._Defer, "armed", False)
    monkeypatch.delenv("FZ_LNBWD64", raising=False)
    names = _Names(monkeypatch)
    for k, t in ops.items():
        if isinstance(t, torch.Tensor):
            names.add(k, t)
    lib = _FakeLib(monkeypatch, names)
    res = run(ops, **rkw)
    return dict(calls=lib.calls, returns=names.d(res))


@pytest.mark.parametrize("case", list(DESC_CASES))
def test_wrapper_descriptors_are_the_recorded_ones(monkeypatch, case):
    assert _trace_desc(monkeypatch, case) == EXPECTED_DESC[case]


# ==== EXPECTED: the records of the recorders above on pointwise.py before the fold (see the module docstring) ====================
# Ids: ACT none 0, relu 1, gelu 2; FZ_DROP_RES 0, FZ_DROP_GELU 1, FZ_DROP_GELU_BWD 2; FZ_EPI_LNBWD 2 (include/factorizer_hip.h).
# A keyword that is absent was not passed, or was passed with its default value.
EXPECTED_NODE = {
    'plain': {
        'fwd': [('gemm', ['x'], 'win@32x32', 'new1[1x32x2x2x4,f32]',
                 {'B': 1, 'Cin': 32, 'Vin': 16, 'M': 32, 'K': 32, 'Ncol': 16, 'ln': ('n1w', 'n1b', 1e-05), 'stats_out': 'new2[1x2x16,f32]', 'eact': 1,
                  'name': 'ln_linear'}),
                ('core_fwd',
                 {'ctx': 'ctx', 't': 'new1[1x32x2x2x4,f32]', 'u0': 'u0', 'v0': 'v0', 'geo': 'geo', 'T': 5, 'G': 1, 'solver': 1, 'eps': 1e-16,
                  'relu_gate': True}),
                ('gemm', ['core_fwd1.a'], 'wout@32x32', 'new3[1x32x2x2x4,f32]',
                 {'B': 1, 'Cin': 32, 'Vin': 16, 'M': 32, 'K': 32, 'Ncol': 16, 'bias': 'bout', 'res': 'x', 'name': 'act_linear_res'}),
                ('gemm', ['new3[1x32x2x2x4,f32]'], 'w1@64x32', 'new4[1x64x2x2x4,f32]',
                 {'B': 1, 'Cin': 32, 'Vin': 16, 'M': 64, 'K': 32, 'Ncol': 16, 'bias': 'b1', 'ln': ('n2w', 'n2b', 1e-06),
                  'stats_out': 'new5[1x2x16,f32]', 'name': 'ln_linear'}),
                ('gemm', ['new4[1x64x2x2x4,f32]'], 'w2@32x64', 'new6[1x32x2x2x4,f32]',
                 {'B': 1, 'Cin': 64, 'Vin': 16, 'M': 32, 'K': 64, 'Ncol': 16, 'bias': 'b2', 'bact': 2, 'res': 'new3[1x32x2x2x4,f32]',
                  'name': 'act_linear_res'})],
        'out': ('new6[1x32x2x2x4,f32]',),
        'saved': ('x', 'new2[1x2x16,f32]', 'new1[1x32x2x2x4,f32]', 'core_fwd1.a', 'new3[1x32x2x2x4,f32]', 'new5[1x2x16,f32]', 'new4[1x64x2x2x4,f32]',
                  None, 'n1w', 'n1b', 'win@32x32', 'u0', 'v0', 'wout@32x32', 'n2w', 'n2b', 'w1@64x32', 'w2@32x64', None, None, None),
        'marks': [],
        'shapes': ((32, 32, 1, 1, 1), (32, 32, 1, 1, 1), (64, 32, 1, 1, 1), (32, 64, 1, 1, 1)),
        'prm': ('win', 'wout', 'bout', 'w1', 'b1', 'w2', 'b2'),
        'bwd': [('gemm', ['g2'], 'w2@32x64', 'new7[1x64x2x2x4,f32]',
                 {'B': 1, 'Cin': 32, 'Vin': 16, 'M': 64, 'K': 32, 'Ncol': 16, 'w_t': True, 'ldw': 64, 'emul': 'new4[1x64x2x2x4,f32]', 'emul_kind': 2,
                  'name': 'linear_dgrad'}),
                ('dgrad_lnbwd',
                 {'gz': 'new7[1x64x2x2x4,f32]', 'w2': 'w1@64x32', 'x': 'new3[1x32x2x2x4,f32]', 'stats': 'new5[1x2x16,f32]', 'ln_w': 'n2w',
                  'gadd': 'g2'}),
                ('gemm', ['dgrad_lnbwd1.gx'], 'wout@32x32', 'new8[1x32x2x2x4,f32]',
                 {'B': 1, 'Cin': 32, 'Vin': 16, 'M': 32, 'K': 32, 'Ncol': 16, 'w_t': True, 'ldw': 32, 'name': 'linear_dgrad'}),
                ('core_bwd',
                 {'ctx': {'saved_tensors': ('new1[1x32x2x2x4,f32]', 'u0', 'v0'), 'cfg': ('geo', 5, 1, 1, 1e-16, True)}, 'ga': 'new8[1x32x2x2x4,f32]'}),
                ('dgrad_lnbwd',
                 {'gz': 'core_bwd1.gt', 'w2': 'win@32x32', 'x': 'x', 'stats': 'new2[1x2x16,f32]', 'ln_w': 'n1w', 'gadd': 'dgrad_lnbwd1.gx'}),
                ('wgrad_group',
                 [('g2', ['new4[1x64x2x2x4,f32]'], 'new9[32x64,f32]',
                   {'B': 1, 'M': 32, 'Cin': 64, 'K': 64, 'Vq': 16, 'Ncols': 16, 'gbias': 'new10[32,f32]', 'qact': 2}),
                  ('new7[1x64x2x2x4,f32]', ['new3[1x32x2x2x4,f32]'], 'new11[64x32,f32]',
                   {'B': 1, 'M': 64, 'Cin': 32, 'K': 32, 'Vq': 16, 'Ncols': 16, 'gbias': 'new12[64,f32]', 'stats': 'new5[1x2x16,f32]',
                    'ln': ('n2w', 'n2b')}),
                  ('dgrad_lnbwd1.gx', ['core_fwd1.a'], 'new13[32x32,f32]',
                   {'B': 1, 'M': 32, 'Cin': 32, 'K': 32, 'Vq': 16, 'Ncols': 16, 'gbias': 'new14[32,f32]'}),
                  ('core_bwd1.gt', ['x'], 'new15[32x32,f32]',
                   {'B': 1, 'M': 32, 'Cin': 32, 'K': 32, 'Vq': 16, 'Ncols': 16, 'stats': 'new2[1x2x16,f32]', 'ln': ('n1w', 'n1b')})],
                 'wgrad_block_32x64')],
        'grads': ('dgrad_lnbwd2.gx', 'dgrad_lnbwd2.gg', 'dgrad_lnbwd2.gbt', 'new15[32x32,f32]@32x32x1x1x1', None, None,
                  'new13[32x32,f32]@32x32x1x1x1', 'new14[32,f32]', 'dgrad_lnbwd1.gg', 'dgrad_lnbwd1.gbt', 'new11[64x32,f32]@64x32x1x1x1',
                  'new12[64,f32]', 'new9[32x64,f32]@32x64x1x1x1', 'new10[32,f32]', None, None, None, None, None),
    },
    'chain': {
        'fwd': [('gemm', ['x'], 'win@32x32', 'new1[1x32x2x2x4,f32]',
                 {'B': 1, 'Cin': 32, 'Vin': 16, 'M': 32, 'K': 32, 'Ncol': 16, 'ln': ('n1w', 'n1b', 1e-05), 'stats_out': 'new2[1x2x16,f32]', 'eact': 1,
                  'name': 'ln_linear'}),
                ('core_fwd',
                 {'ctx': 'ctx', 't': 'new1[1x32x2x2x4,f32]', 'u0': 'u0', 'v0': 'v0', 'geo': 'geo', 'T': 5, 'G': 1, 'solver': 1, 'eps': 1e-16,
                  'relu_gate': True}),
                ('gemm', ['core_fwd1.a'], 'wout@32x32', 'new3[1x32x2x2x4,f32]',
                 {'B': 1, 'Cin': 32, 'Vin': 16, 'M': 32, 'K': 32, 'Ncol': 16, 'bias': 'bout', 'res': 'x', 'name': 'act_linear_res'}),
                ('mlp_fwd_chain',
                 {'x1': 'new3[1x32x2x2x4,f32]', 'ln_w': 'n2w', 'ln_b': 'n2b', 'eps': 1e-06, 'w12': 'w1@64x32', 'b1': 'b1', 'w22': 'w2@32x64',
                  'b2': 'b2'})],
        'out': ('mlp_fwd_chain1.x2',),
        'saved': ('x', 'new2[1x2x16,f32]', 'new1[1x32x2x2x4,f32]', 'core_fwd1.a', 'new3[1x32x2x2x4,f32]', 'mlp_fwd_chain1.st', 'mlp_fwd_chain1.z1',
                  None, 'n1w', 'n1b', 'win@32x32', 'u0', 'v0', 'wout@32x32', 'n2w', 'n2b', 'w1@64x32', 'w2@32x64', None, None, None),
        'marks': [],
        'shapes': ((32, 32, 1, 1, 1), (32, 32, 1, 1, 1), (64, 32, 1, 1, 1), (32, 64, 1, 1, 1)),
        'prm': ('win', 'wout', 'bout', 'w1', 'b1', 'w2', 'b2'),
        'bwd': [('mlp_bwd_chain',
                 {'g2': 'g2', 'z1': 'mlp_fwd_chain1.z1', 'w12': 'w1@64x32', 'w22': 'w2@32x64', 'x1': 'new3[1x32x2x2x4,f32]',
                  'st': 'mlp_fwd_chain1.st', 'ln_w': 'n2w'}),
                ('wgrad', 'g2', ['mlp_fwd_chain1.z1'], 'new4[32x64,f32]',
                 {'B': 1, 'M': 32, 'Cin': 64, 'K': 64, 'Vq': 16, 'Ncols': 16, 'gbias': 'new5[32,f32]', 'qact': 2, 'name': 'wgrad_linear'}),
                ('wgrad', 'mlp_bwd_chain1.gz1', ['new3[1x32x2x2x4,f32]'], 'new6[64x32,f32]',
                 {'B': 1, 'M': 64, 'Cin': 32, 'K': 32, 'Vq': 16, 'Ncols': 16, 'gbias': 'new7[64,f32]', 'stats': 'mlp_fwd_chain1.st',
                  'ln': ('n2w', 'n2b'), 'name': 'wgrad_ln_linear'}),
                ('gemm_dw', {'g': 'mlp_bwd_chain1.gx1', 'w2': 'wout@32x32', 'q': 'core_fwd1.a', 'want_bias': True}),
                ('core_bwd',
                 {'ctx': {'saved_tensors': ('new1[1x32x2x2x4,f32]', 'u0', 'v0'), 'cfg': ('geo', 5, 1, 1, 1e-16, True)}, 'ga': 'gemm_dw1.y'}),
                ('gemm_dw',
                 {'g': 'core_bwd1.gt', 'w2': 'win@32x32', 'q': 'x', 'ln': ('n1w', 'n1b'), 'stats': 'new2[1x2x16,f32]', 'gadd': 'mlp_bwd_chain1.gx1',
                  'name': 'dgrad_lnbwd_wgrad'})],
        'grads': ('gemm_dw2.y', 'gemm_dw2.gg', 'gemm_dw2.gbt', 'gemm_dw2.gw@32x32x1x1x1', None, None, 'gemm_dw1.gw@32x32x1x1x1', 'gemm_dw1.gb',
                  'mlp_bwd_chain1.gg', 'mlp_bwd_chain1.gbt', 'new6[64x32,f32]@64x32x1x1x1', 'new7[64,f32]', 'new4[32x64,f32]@32x64x1x1x1',
                  'new5[32,f32]', None, None, None, None, None),
    },
    'chain-wgf': {
        'fwd': [('gemm', ['x'], 'win@32x32', 'new1[1x32x2x2x4,f32]',
                 {'B': 1, 'Cin': 32, 'Vin': 16, 'M': 32, 'K': 32, 'Ncol': 16, 'ln': ('n1w', 'n1b', 1e-05), 'stats_out': 'new2[1x2x16,f32]', 'eact': 1,
                  'name': 'ln_linear'}),
                ('core_fwd',
                 {'ctx': 'ctx', 't': 'new1[1x32x2x2x4,f32]', 'u0': 'u0', 'v0': 'v0', 'geo': 'geo', 'T': 5, 'G': 1, 'solver': 1, 'eps': 1e-16,
                  'relu_gate': True}),
                ('gemm', ['core_fwd1.a'], 'wout@32x32', 'new3[1x32x2x2x4,f32]',
                 {'B': 1, 'Cin': 32, 'Vin': 16, 'M': 32, 'K': 32, 'Ncol': 16, 'bias': 'bout', 'res': 'x', 'name': 'act_linear_res'}),
                ('mlp_fwd_chain',
                 {'x1': 'new3[1x32x2x2x4,f32]', 'ln_w': 'n2w', 'ln_b': 'n2b', 'eps': 1e-06, 'w12': 'w1@64x32', 'b1': 'b1', 'w22': 'w2@32x64',
                  'b2': 'b2'})],
        'out': ('mlp_fwd_chain1.x2',),
        'saved': ('x', 'new2[1x2x16,f32]', 'new1[1x32x2x2x4,f32]', 'core_fwd1.a', 'new3[1x32x2x2x4,f32]', 'mlp_fwd_chain1.st', 'mlp_fwd_chain1.z1',
                  None, 'n1w', 'n1b', 'win@32x32', 'u0', 'v0', 'wout@32x32', 'n2w', 'n2b', 'w1@64x32', 'w2@32x64', None, None, None),
        'marks': [],
        'shapes': ((32, 32, 1, 1, 1), (32, 32, 1, 1, 1), (64, 32, 1, 1, 1), (32, 64, 1, 1, 1)),
        'prm': ('win', 'wout', 'bout', 'w1', 'b1', 'w2', 'b2'),
        'bwd': [('mlp_bwd_chain_wgrad',
                 {'g2': 'g2', 'z1': 'mlp_fwd_chain1.z1', 'w12': 'w1@64x32', 'w22': 'w2@32x64', 'x1': 'new3[1x32x2x2x4,f32]',
                  'st': 'mlp_fwd_chain1.st', 'ln_w': 'n2w', 'ln_b': 'n2b'}),
                ('gemm', ['mlp_bwd_chain_wgrad1.gx1'], 'wout@32x32', 'new4[1x32x2x2x4,f32]',
                 {'B': 1, 'Cin': 32, 'Vin': 16, 'M': 32, 'K': 32, 'Ncol': 16, 'w_t': True, 'ldw': 32, 'name': 'linear_dgrad'}),
                ('core_bwd',
                 {'ctx': {'saved_tensors': ('new1[1x32x2x2x4,f32]', 'u0', 'v0'), 'cfg': ('geo', 5, 1, 1, 1e-16, True)}, 'ga': 'new4[1x32x2x2x4,f32]'}),
                ('dgrad_lnbwd',
                 {'gz': 'core_bwd1.gt', 'w2': 'win@32x32', 'x': 'x', 'stats': 'new2[1x2x16,f32]', 'ln_w': 'n1w', 'gadd': 'mlp_bwd_chain_wgrad1.gx1'}),
                ('wgrad_group',
                 [('mlp_bwd_chain_wgrad1.gx1', ['core_fwd1.a'], 'new5[32x32,f32]',
                   {'B': 1, 'M': 32, 'Cin': 32, 'K': 32, 'Vq': 16, 'Ncols': 16, 'gbias': 'new6[32,f32]'}),
                  ('core_bwd1.gt', ['x'], 'new7[32x32,f32]',
                   {'B': 1, 'M': 32, 'Cin': 32, 'K': 32, 'Vq': 16, 'Ncols': 16, 'stats': 'new2[1x2x16,f32]', 'ln': ('n1w', 'n1b')})],
                 'wgrad_block_32x64')],
        'grads': ('dgrad_lnbwd1.gx', 'dgrad_lnbwd1.gg', 'dgrad_lnbwd1.gbt', 'new7[32x32,f32]@32x32x1x1x1', None, None, 'new5[32x32,f32]@32x32x1x1x1',
                  'new6[32,f32]', 'mlp_bwd_chain_wgrad1.gg', 'mlp_bwd_chain_wgrad1.gbt', 'mlp_bwd_chain_wgrad1.gw1@64x32x1x1x1',
                  'mlp_bwd_chain_wgrad1.gb1', 'mlp_bwd_chain_wgrad1.gw2@32x64x1x1x1', 'mlp_bwd_chain_wgrad1.gb2', None, None, None, None, None),
    },
    'outproj': {
        'fwd': [('gemm', ['x'], 'win@32x32', 'new1[1x32x2x2x4,f32]',
                 {'B': 1, 'Cin': 32, 'Vin': 16, 'M': 32, 'K': 32, 'Ncol': 16, 'ln': ('n1w', 'n1b', 1e-05), 'stats_out': 'new2[1x2x16,f32]', 'eact': 1,
                  'name': 'ln_linear'}),
                ('core_fwd',
                 {'ctx': 'ctx', 't': 'new1[1x32x2x2x4,f32]', 'u0': 'u0', 'v0': 'v0', 'geo': 'geo', 'T': 5, 'G': 1, 'solver': 1, 'eps': 1e-16,
                  'relu_gate': True}),
                ('outproj_mlp_fwd_chain',
                 {'a': 'core_fwd1.a', 'wout2': 'wout@32x32', 'bout': 'bout', 'x': 'x', 'ln_w': 'n2w', 'ln_b': 'n2b', 'eps': 1e-06, 'w12': 'w1@64x32',
                  'b1': 'b1', 'w22': 'w2@32x64', 'b2': 'b2'})],
        'out': ('outproj_mlp_fwd_chain1.x2',),
        'saved': ('x', 'new2[1x2x16,f32]', 'new1[1x32x2x2x4,f32]', 'core_fwd1.a', 'outproj_mlp_fwd_chain1.x1', 'outproj_mlp_fwd_chain1.st',
                  'outproj_mlp_fwd_chain1.z1', None, 'n1w', 'n1b', 'win@32x32', 'u0', 'v0', 'wout@32x32', 'n2w', 'n2b', 'w1@64x32', 'w2@32x64', None,
                  None, None),
        'marks': [],
        'shapes': ((32, 32, 1, 1, 1), (32, 32, 1, 1, 1), (64, 32, 1, 1, 1), (32, 64, 1, 1, 1)),
        'prm': ('win', 'wout', 'bout', 'w1', 'b1', 'w2', 'b2'),
        'bwd': [('mlp_bwd_chain',
                 {'g2': 'g2', 'z1': 'outproj_mlp_fwd_chain1.z1', 'w12': 'w1@64x32', 'w22': 'w2@32x64', 'x1': 'outproj_mlp_fwd_chain1.x1',
                  'st': 'outproj_mlp_fwd_chain1.st', 'ln_w': 'n2w'}),
                ('gemm', ['mlp_bwd_chain1.gx1'], 'wout@32x32', 'new3[1x32x2x2x4,f32]',
                 {'B': 1, 'Cin': 32, 'Vin': 16, 'M': 32, 'K': 32, 'Ncol': 16, 'w_t': True, 'ldw': 32, 'name': 'linear_dgrad'}),
                ('core_bwd',
                 {'ctx': {'saved_tensors': ('new1[1x32x2x2x4,f32]', 'u0', 'v0'), 'cfg': ('geo', 5, 1, 1, 1e-16, True)}, 'ga': 'new3[1x32x2x2x4,f32]'}),
                ('dgrad_lnbwd',
                 {'gz': 'core_bwd1.gt', 'w2': 'win@32x32', 'x': 'x', 'stats': 'new2[1x2x16,f32]', 'ln_w': 'n1w', 'gadd': 'mlp_bwd_chain1.gx1'}),
                ('wgrad_group',
                 [('g2', ['outproj_mlp_fwd_chain1.z1'], 'new4[32x64,f32]',
                   {'B': 1, 'M': 32, 'Cin': 64, 'K': 64, 'Vq': 16, 'Ncols': 16, 'gbias': 'new5[32,f32]', 'qact': 2}),
                  ('mlp_bwd_chain1.gz1', ['outproj_mlp_fwd_chain1.x1'], 'new6[64x32,f32]',
                   {'B': 1, 'M': 64, 'Cin': 32, 'K': 32, 'Vq': 16, 'Ncols': 16, 'gbias': 'new7[64,f32]', 'stats': 'outproj_mlp_fwd_chain1.st',
                    'ln': ('n2w', 'n2b')}),
                  ('mlp_bwd_chain1.gx1', ['core_fwd1.a'], 'new8[32x32,f32]',
                   {'B': 1, 'M': 32, 'Cin': 32, 'K': 32, 'Vq': 16, 'Ncols': 16, 'gbias': 'new9[32,f32]'}),
                  ('core_bwd1.gt', ['x'], 'new10[32x32,f32]',
                   {'B': 1, 'M': 32, 'Cin': 32, 'K': 32, 'Vq': 16, 'Ncols': 16, 'stats': 'new2[1x2x16,f32]', 'ln': ('n1w', 'n1b')})],
                 'wgrad_block_32x64')],
        'grads': ('dgrad_lnbwd1.gx', 'dgrad_lnbwd1.gg', 'dgrad_lnbwd1.gbt', 'new10[32x32,f32]@32x32x1x1x1', None, None, 'new8[32x32,f32]@32x32x1x1x1',
                  'new9[32,f32]', 'mlp_bwd_chain1.gg', 'mlp_bwd_chain1.gbt', 'new6[64x32,f32]@64x32x1x1x1', 'new7[64,f32]',
                  'new4[32x64,f32]@32x64x1x1x1', 'new5[32,f32]', None, None, None, None, None),
    },
    'outproj-head': {
        'fwd': [('core_fwd',
                 {'ctx': 'ctx', 't': 't_pre', 'u0': 'u0', 'v0': 'v0', 'geo': 'geo', 'T': 5, 'G': 1, 'solver': 1, 'eps': 1e-16, 'relu_gate': True}),
                ('outproj_mlp_fwd_chain',
                 {'a': 'core_fwd1.a', 'wout2': 'wout@32x32', 'bout': 'bout', 'x': 'x', 'ln_w': 'n2w', 'ln_b': 'n2b', 'eps': 1e-06, 'w12': 'w1@64x32',
                  'b1': 'b1', 'w22': 'w2@32x64', 'b2': 'b2', 'head': ('head_w@3x32', 'head_b')})],
        'out': ('outproj_mlp_fwd_chain1.x2', 'outproj_mlp_fwd_chain1.logits'),
        'saved': ('x', 'st_pre', 't_pre', 'core_fwd1.a', 'outproj_mlp_fwd_chain1.x1', 'outproj_mlp_fwd_chain1.st', 'outproj_mlp_fwd_chain1.z1', None,
                  'n1w', 'n1b', 'win@32x32', 'u0', 'v0', 'wout@32x32', 'n2w', 'n2b', 'w1@64x32', 'w2@32x64', None, None, None),
        'marks': [('mark_non_differentiable', ('outproj_mlp_fwd_chain1.logits',)), ('set_materialize_grads', False)],
        'shapes': ((32, 32, 1, 1, 1), (32, 32, 1, 1, 1), (64, 32, 1, 1, 1), (32, 64, 1, 1, 1)),
        'prm': ('win', 'wout', 'bout', 'w1', 'b1', 'w2', 'b2'),
        'bwd': [('mlp_bwd_chain_wgrad',
                 {'g2': 'g2', 'z1': 'outproj_mlp_fwd_chain1.z1', 'w12': 'w1@64x32', 'w22': 'w2@32x64', 'x1': 'outproj_mlp_fwd_chain1.x1',
                  'st': 'outproj_mlp_fwd_chain1.st', 'ln_w': 'n2w', 'ln_b': 'n2b'}),
                ('gemm_dw', {'g': 'mlp_bwd_chain_wgrad1.gx1', 'w2': 'wout@32x32', 'q': 'core_fwd1.a', 'want_bias': True}),
                ('core_bwd', {'ctx': {'saved_tensors': ('t_pre', 'u0', 'v0'), 'cfg': ('geo', 5, 1, 1, 1e-16, True)}, 'ga': 'gemm_dw1.y'}),
                ('gemm_dw',
                 {'g': 'core_bwd1.gt', 'w2': 'win@32x32', 'q': 'x', 'ln': ('n1w', 'n1b'), 'stats': 'st_pre', 'gadd': 'mlp_bwd_chain_wgrad1.gx1',
                  'name': 'dgrad_lnbwd_wgrad'})],
        'grads': ('gemm_dw2.y', 'gemm_dw2.gg', 'gemm_dw2.gbt', 'gemm_dw2.gw@32x32x1x1x1', None, None, 'gemm_dw1.gw@32x32x1x1x1', 'gemm_dw1.gb',
                  'mlp_bwd_chain_wgrad1.gg', 'mlp_bwd_chain_wgrad1.gbt', 'mlp_bwd_chain_wgrad1.gw1@64x32x1x1x1', 'mlp_bwd_chain_wgrad1.gb1',
                  'mlp_bwd_chain_wgrad1.gw2@32x64x1x1x1', 'mlp_bwd_chain_wgrad1.gb2', None, None, None, None, None),
    },
    'drop-ppp-fused': {
        'fwd': [('dropout_seed', {'device': 'cpu'}),
                ('dropout_keep_bits', {'seed': 'dropout_seed1.seed', 'site': 0, 'B': 1, 'ch': 32, 'V': 16, 'p': 0.1}),
                ('dropout_keep_bits', {'seed': 'dropout_seed1.seed', 'site': 1, 'B': 1, 'ch': 64, 'V': 16, 'p': 0.2}),
                ('dropout_keep_bits', {'seed': 'dropout_seed1.seed', 'site': 2, 'B': 1, 'ch': 32, 'V': 16, 'p': 0.3}),
                ('gemm', ['x'], 'win@32x32', 'new1[1x32x2x2x4,f32]',
                 {'B': 1, 'Cin': 32, 'Vin': 16, 'M': 32, 'K': 32, 'Ncol': 16, 'ln': ('n1w', 'n1b', 1e-05), 'stats_out': 'new2[1x2x16,f32]', 'eact': 1,
                  'name': 'ln_linear'}),
                ('core_fwd',
                 {'ctx': 'ctx', 't': 'new1[1x32x2x2x4,f32]', 'u0': 'u0', 'v0': 'v0', 'geo': 'geo', 'T': 5, 'G': 1, 'solver': 1, 'eps': 1e-16,
                  'relu_gate': True}),
                ('outproj_mlp_fwd_chain',
                 {'a': 'core_fwd1.a', 'wout2': 'wout@32x32', 'bout': 'bout', 'x': 'x', 'ln_w': 'n2w', 'ln_b': 'n2b', 'eps': 1e-06, 'w12': 'w1@64x32',
                  'b1': 'b1', 'w22': 'w2@32x64', 'b2': 'b2',
                  'drop': (('dropout_keep_bits1.bits', 'dropout_keep_bits2.bits', 'dropout_keep_bits3.bits'), (0.1, 0.2, 0.3))})],
        'out': ('outproj_mlp_fwd_chain1.x2',),
        'saved': ('x', 'new2[1x2x16,f32]', 'new1[1x32x2x2x4,f32]', 'core_fwd1.a', 'outproj_mlp_fwd_chain1.x1', 'outproj_mlp_fwd_chain1.st',
                  'outproj_mlp_fwd_chain1.z1', None, 'n1w', 'n1b', 'win@32x32', 'u0', 'v0', 'wout@32x32', 'n2w', 'n2b', 'w1@64x32', 'w2@32x64',
                  'dropout_keep_bits1.bits', 'dropout_keep_bits2.bits', 'dropout_keep_bits3.bits'),
        'marks': [],
        'shapes': ((32, 32, 1, 1, 1), (32, 32, 1, 1, 1), (64, 32, 1, 1, 1), (32, 64, 1, 1, 1)),
        'prm': ('win', 'wout', 'bout', 'w1', 'b1', 'w2', 'b2'),
        'bwd': [('dropout_apply', {'kind': 0, 'bits': 'dropout_keep_bits3.bits', 'p': 0.3, 't': 'g2'}),
                ('gemm', ['dropout_apply1.out'], 'w2@32x64', 'new3[1x64x2x2x4,f32]',
                 {'B': 1, 'Cin': 32, 'Vin': 16, 'M': 64, 'K': 32, 'Ncol': 16, 'w_t': True, 'ldw': 64, 'name': 'linear_dgrad'}),
                ('dropout_apply',
                 {'kind': 2, 'bits': 'dropout_keep_bits2.bits', 'p': 0.2, 't': 'new3[1x64x2x2x4,f32]', 'aux': 'outproj_mlp_fwd_chain1.z1'}),
                ('dropout_apply', {'kind': 1, 'bits': 'dropout_keep_bits2.bits', 'p': 0.2, 't': 'outproj_mlp_fwd_chain1.z1'}),
                ('dgrad_lnbwd',
                 {'gz': 'dropout_apply2.out', 'w2': 'w1@64x32', 'x': 'outproj_mlp_fwd_chain1.x1', 'stats': 'outproj_mlp_fwd_chain1.st', 'ln_w': 'n2w',
                  'gadd': 'g2'}),
                ('gemm_dw',
                 {'g': 'dgrad_lnbwd1.gx', 'w2': 'wout@32x32', 'q': 'core_fwd1.a', 'want_bias': True, 'drop': ('dropout_keep_bits1.bits', 0.1)}),
                ('core_bwd',
                 {'ctx': {'saved_tensors': ('new1[1x32x2x2x4,f32]', 'u0', 'v0'), 'cfg': ('geo', 5, 1, 1, 1e-16, True)}, 'ga': 'gemm_dw1.y'}),
                ('gemm_dw',
                 {'g': 'core_bwd1.gt', 'w2': 'win@32x32', 'q': 'x', 'ln': ('n1w', 'n1b'), 'stats': 'new2[1x2x16,f32]', 'gadd': 'dgrad_lnbwd1.gx',
                  'name': 'dgrad_lnbwd_wgrad'}),
                ('wgrad_group',
                 [('dropout_apply1.out', ['dropout_apply3.out'], 'new4[32x64,f32]',
                   {'B': 1, 'M': 32, 'Cin': 64, 'K': 64, 'Vq': 16, 'Ncols': 16, 'gbias': 'new5[32,f32]'}),
                  ('dropout_apply2.out', ['outproj_mlp_fwd_chain1.x1'], 'new6[64x32,f32]',
                   {'B': 1, 'M': 64, 'Cin': 32, 'K': 32, 'Vq': 16, 'Ncols': 16, 'gbias': 'new7[64,f32]', 'stats': 'outproj_mlp_fwd_chain1.st',
                    'ln': ('n2w', 'n2b')})],
                 'wgrad_block_32x64')],
        'grads': ('gemm_dw2.y', 'gemm_dw2.gg', 'gemm_dw2.gbt', 'gemm_dw2.gw@32x32x1x1x1', None, None, 'gemm_dw1.gw@32x32x1x1x1', 'gemm_dw1.gb',
                  'dgrad_lnbwd1.gg', 'dgrad_lnbwd1.gbt', 'new6[64x32,f32]@64x32x1x1x1', 'new7[64,f32]', 'new4[32x64,f32]@32x64x1x1x1', 'new5[32,f32]',
                  None, None, None, None, None),
    },
    'drop-p00': {
        'fwd': [('dropout_seed', {'device': 'cpu'}),
                ('dropout_keep_bits', {'seed': 'dropout_seed1.seed', 'site': 0, 'B': 1, 'ch': 32, 'V': 16, 'p': 0.25}),
                ('gemm', ['x'], 'win@32x32', 'new1[1x32x2x2x4,f32]',
                 {'B': 1, 'Cin': 32, 'Vin': 16, 'M': 32, 'K': 32, 'Ncol': 16, 'ln': ('n1w', 'n1b', 1e-05), 'stats_out': 'new2[1x2x16,f32]', 'eact': 1,
                  'name': 'ln_linear'}),
                ('core_fwd',
                 {'ctx': 'ctx', 't': 'new1[1x32x2x2x4,f32]', 'u0': 'u0', 'v0': 'v0', 'geo': 'geo', 'T': 5, 'G': 1, 'solver': 1, 'eps': 1e-16,
                  'relu_gate': True}),
                ('gemm', ['core_fwd1.a'], 'wout@32x32', 'new3[1x32x2x2x4,f32]',
                 {'B': 1, 'Cin': 32, 'Vin': 16, 'M': 32, 'K': 32, 'Ncol': 16, 'bias': 'bout', 'name': 'linear'}),
                ('dropout_apply', {'kind': 0, 'bits': 'dropout_keep_bits1.bits', 'p': 0.25, 't': 'new3[1x32x2x2x4,f32]', 'aux': 'x'}),
                ('gemm', ['dropout_apply1.out'], 'w1@64x32', 'new4[1x64x2x2x4,f32]',
                 {'B': 1, 'Cin': 32, 'Vin': 16, 'M': 64, 'K': 32, 'Ncol': 16, 'bias': 'b1', 'ln': ('n2w', 'n2b', 1e-06),
                  'stats_out': 'new5[1x2x16,f32]', 'name': 'ln_linear'}),
                ('gemm', ['new4[1x64x2x2x4,f32]'], 'w2@32x64', 'new6[1x32x2x2x4,f32]',
                 {'B': 1, 'Cin': 64, 'Vin': 16, 'M': 32, 'K': 64, 'Ncol': 16, 'bias': 'b2', 'bact': 2, 'res': 'dropout_apply1.out',
                  'name': 'act_linear_res'})],
        'out': ('new6[1x32x2x2x4,f32]',),
        'saved': ('x', 'new2[1x2x16,f32]', 'new1[1x32x2x2x4,f32]', 'core_fwd1.a', 'dropout_apply1.out', 'new5[1x2x16,f32]', 'new4[1x64x2x2x4,f32]',
                  None, 'n1w', 'n1b', 'win@32x32', 'u0', 'v0', 'wout@32x32', 'n2w', 'n2b', 'w1@64x32', 'w2@32x64', 'dropout_keep_bits1.bits', None,
                  None),
        'marks': [],
        'shapes': ((32, 32, 1, 1, 1), (32, 32, 1, 1, 1), (64, 32, 1, 1, 1), (32, 64, 1, 1, 1)),
        'prm': ('win', 'wout', 'bout', 'w1', 'b1', 'w2', 'b2'),
        'bwd': [('gemm', ['g2'], 'w2@32x64', 'new7[1x64x2x2x4,f32]',
                 {'B': 1, 'Cin': 32, 'Vin': 16, 'M': 64, 'K': 32, 'Ncol': 16, 'w_t': True, 'ldw': 64, 'emul': 'new4[1x64x2x2x4,f32]', 'emul_kind': 2,
                  'name': 'linear_dgrad'}),
                ('dgrad_lnbwd',
                 {'gz': 'new7[1x64x2x2x4,f32]', 'w2': 'w1@64x32', 'x': 'dropout_apply1.out', 'stats': 'new5[1x2x16,f32]', 'ln_w': 'n2w', 'gadd': 'g2'}),
                ('dropout_apply', {'kind': 0, 'bits': 'dropout_keep_bits1.bits', 'p': 0.25, 't': 'dgrad_lnbwd1.gx'}),
                ('gemm', ['dropout_apply2.out'], 'wout@32x32', 'new8[1x32x2x2x4,f32]',
                 {'B': 1, 'Cin': 32, 'Vin': 16, 'M': 32, 'K': 32, 'Ncol': 16, 'w_t': True, 'ldw': 32, 'name': 'linear_dgrad'}),
                ('core_bwd',
                 {'ctx': {'saved_tensors': ('new1[1x32x2x2x4,f32]', 'u0', 'v0'), 'cfg': ('geo', 5, 1, 1, 1e-16, True)}, 'ga': 'new8[1x32x2x2x4,f32]'}),
                ('dgrad_lnbwd',
                 {'gz': 'core_bwd1.gt', 'w2': 'win@32x32', 'x': 'x', 'stats': 'new2[1x2x16,f32]', 'ln_w': 'n1w', 'gadd': 'dgrad_lnbwd1.gx'}),
                ('wgrad_group',
                 [('g2', ['new4[1x64x2x2x4,f32]'], 'new9[32x64,f32]',
                   {'B': 1, 'M': 32, 'Cin': 64, 'K': 64, 'Vq': 16, 'Ncols': 16, 'gbias': 'new10[32,f32]', 'qact': 2}),
                  ('new7[1x64x2x2x4,f32]', ['dropout_apply1.out'], 'new11[64x32,f32]',
                   {'B': 1, 'M': 64, 'Cin': 32, 'K': 32, 'Vq': 16, 'Ncols': 16, 'gbias': 'new12[64,f32]', 'stats': 'new5[1x2x16,f32]',
                    'ln': ('n2w', 'n2b')}),
                  ('dropout_apply2.out', ['core_fwd1.a'], 'new13[32x32,f32]',
                   {'B': 1, 'M': 32, 'Cin': 32, 'K': 32, 'Vq': 16, 'Ncols': 16, 'gbias': 'new14[32,f32]'}),
                  ('core_bwd1.gt', ['x'], 'new15[32x32,f32]',
                   {'B': 1, 'M': 32, 'Cin': 32, 'K': 32, 'Vq': 16, 'Ncols': 16, 'stats': 'new2[1x2x16,f32]', 'ln': ('n1w', 'n1b')})],
                 'wgrad_block_32x64')],
        'grads': ('dgrad_lnbwd2.gx', 'dgrad_lnbwd2.gg', 'dgrad_lnbwd2.gbt', 'new15[32x32,f32]@32x32x1x1x1', None, None,
                  'new13[32x32,f32]@32x32x1x1x1', 'new14[32,f32]', 'dgrad_lnbwd1.gg', 'dgrad_lnbwd1.gbt', 'new11[64x32,f32]@64x32x1x1x1',
                  'new12[64,f32]', 'new9[32x64,f32]@32x64x1x1x1', 'new10[32,f32]', None, None, None, None, None),
    },
    'drop-0p0': {
        'fwd': [('dropout_seed', {'device': 'cpu'}),
                ('dropout_keep_bits', {'seed': 'dropout_seed1.seed', 'site': 1, 'B': 1, 'ch': 64, 'V': 16, 'p': 0.25}),
                ('gemm', ['x'], 'win@32x32', 'new1[1x32x2x2x4,f32]',
                 {'B': 1, 'Cin': 32, 'Vin': 16, 'M': 32, 'K': 32, 'Ncol': 16, 'ln': ('n1w', 'n1b', 1e-05), 'stats_out': 'new2[1x2x16,f32]', 'eact': 1,
                  'name': 'ln_linear'}),
                ('core_fwd',
                 {'ctx': 'ctx', 't': 'new1[1x32x2x2x4,f32]', 'u0': 'u0', 'v0': 'v0', 'geo': 'geo', 'T': 5, 'G': 1, 'solver': 1, 'eps': 1e-16,
                  'relu_gate': True}),
                ('gemm', ['core_fwd1.a'], 'wout@32x32', 'new3[1x32x2x2x4,f32]',
                 {'B': 1, 'Cin': 32, 'Vin': 16, 'M': 32, 'K': 32, 'Ncol': 16, 'bias': 'bout', 'res': 'x', 'name': 'act_linear_res'}),
                ('gemm', ['new3[1x32x2x2x4,f32]'], 'w1@64x32', 'new4[1x64x2x2x4,f32]',
                 {'B': 1, 'Cin': 32, 'Vin': 16, 'M': 64, 'K': 32, 'Ncol': 16, 'bias': 'b1', 'ln': ('n2w', 'n2b', 1e-06),
                  'stats_out': 'new5[1x2x16,f32]', 'name': 'ln_linear'}),
                ('dropout_apply', {'kind': 1, 'bits': 'dropout_keep_bits1.bits', 'p': 0.25, 't': 'new4[1x64x2x2x4,f32]'}),
                ('gemm', ['dropout_apply1.out'], 'w2@32x64', 'new6[1x32x2x2x4,f32]',
                 {'B': 1, 'Cin': 64, 'Vin': 16, 'M': 32, 'K': 64, 'Ncol': 16, 'bias': 'b2', 'res': 'new3[1x32x2x2x4,f32]', 'name': 'act_linear_res'})],
        'out': ('new6[1x32x2x2x4,f32]',),
        'saved': ('x', 'new2[1x2x16,f32]', 'new1[1x32x2x2x4,f32]', 'core_fwd1.a', 'new3[1x32x2x2x4,f32]', 'new5[1x2x16,f32]', 'new4[1x64x2x2x4,f32]',
                  None, 'n1w', 'n1b', 'win@32x32', 'u0', 'v0', 'wout@32x32', 'n2w', 'n2b', 'w1@64x32', 'w2@32x64', None, 'dropout_keep_bits1.bits',
                  None),
        'marks': [],
        'shapes': ((32, 32, 1, 1, 1), (32, 32, 1, 1, 1), (64, 32, 1, 1, 1), (32, 64, 1, 1, 1)),
        'prm': ('win', 'wout', 'bout', 'w1', 'b1', 'w2', 'b2'),
        'bwd': [('gemm', ['g2'], 'w2@32x64', 'new7[1x64x2x2x4,f32]',
                 {'B': 1, 'Cin': 32, 'Vin': 16, 'M': 64, 'K': 32, 'Ncol': 16, 'w_t': True, 'ldw': 64, 'name': 'linear_dgrad'}),
                ('dropout_apply',
                 {'kind': 2, 'bits': 'dropout_keep_bits1.bits', 'p': 0.25, 't': 'new7[1x64x2x2x4,f32]', 'aux': 'new4[1x64x2x2x4,f32]'}),
                ('dropout_apply', {'kind': 1, 'bits': 'dropout_keep_bits1.bits', 'p': 0.25, 't': 'new4[1x64x2x2x4,f32]'}),
                ('dgrad_lnbwd',
                 {'gz': 'dropout_apply2.out', 'w2': 'w1@64x32', 'x': 'new3[1x32x2x2x4,f32]', 'stats': 'new5[1x2x16,f32]', 'ln_w': 'n2w', 'gadd': 'g2'}),
                ('gemm_dw', {'g': 'dgrad_lnbwd1.gx', 'w2': 'wout@32x32', 'q': 'core_fwd1.a', 'want_bias': True}),
                ('core_bwd',
                 {'ctx': {'saved_tensors': ('new1[1x32x2x2x4,f32]', 'u0', 'v0'), 'cfg': ('geo', 5, 1, 1, 1e-16, True)}, 'ga': 'gemm_dw1.y'}),
                ('gemm_dw',
                 {'g': 'core_bwd1.gt', 'w2': 'win@32x32', 'q': 'x', 'ln': ('n1w', 'n1b'), 'stats': 'new2[1x2x16,f32]', 'gadd': 'dgrad_lnbwd1.gx',
                  'name': 'dgrad_lnbwd_wgrad'}),
                ('wgrad_group',
                 [('g2', ['dropout_apply3.out'], 'new8[32x64,f32]',
                   {'B': 1, 'M': 32, 'Cin': 64, 'K': 64, 'Vq': 16, 'Ncols': 16, 'gbias': 'new9[32,f32]'}),
                  ('dropout_apply2.out', ['new3[1x32x2x2x4,f32]'], 'new10[64x32,f32]',
                   {'B': 1, 'M': 64, 'Cin': 32, 'K': 32, 'Vq': 16, 'Ncols': 16, 'gbias': 'new11[64,f32]', 'stats': 'new5[1x2x16,f32]',
                    'ln': ('n2w', 'n2b')})],
                 'wgrad_block_32x64')],
        'grads': ('gemm_dw2.y', 'gemm_dw2.gg', 'gemm_dw2.gbt', 'gemm_dw2.gw@32x32x1x1x1', None, None, 'gemm_dw1.gw@32x32x1x1x1', 'gemm_dw1.gb',
                  'dgrad_lnbwd1.gg', 'dgrad_lnbwd1.gbt', 'new10[64x32,f32]@64x32x1x1x1', 'new11[64,f32]', 'new8[32x64,f32]@32x64x1x1x1',
                  'new9[32,f32]', None, None, None, None, None),
    },
    'drop-00p': {
        'fwd': [('dropout_seed', {'device': 'cpu'}),
                ('dropout_keep_bits', {'seed': 'dropout_seed1.seed', 'site': 2, 'B': 1, 'ch': 32, 'V': 16, 'p': 0.25}),
                ('gemm', ['x'], 'win@32x32', 'new1[1x32x2x2x4,f32]',
                 {'B': 1, 'Cin': 32, 'Vin': 16, 'M': 32, 'K': 32, 'Ncol': 16, 'ln': ('n1w', 'n1b', 1e-05), 'stats_out': 'new2[1x2x16,f32]', 'eact': 1,
                  'name': 'ln_linear'}),
                ('swm_fwd_raw', {'x': 'new1[1x32x2x2x4,f32]', 'geo': 'geo'}),
                ('nmf_fwd_raw', {'x': 'swm_fwd_raw1.m', 'u0': 'u0', 'v0': 'v0', 'T': 5, 'solver': 1, 'eps': 1e-16}),
                ('swm_inv_raw', {'y': 'nmf_fwd_raw1.y', 'geo': 'geo'}),
                ('gemm', ['swm_inv_raw1.out'], 'wout@32x32', 'new3[1x32x2x2x4,f32]',
                 {'B': 1, 'Cin': 32, 'Vin': 16, 'M': 32, 'K': 32, 'Ncol': 16, 'bias': 'bout', 'res': 'x', 'name': 'act_linear_res'}),
                ('gemm', ['new3[1x32x2x2x4,f32]'], 'w1@64x32', 'new4[1x64x2x2x4,f32]',
                 {'B': 1, 'Cin': 32, 'Vin': 16, 'M': 64, 'K': 32, 'Ncol': 16, 'bias': 'b1', 'ln': ('n2w', 'n2b', 1e-06),
                  'stats_out': 'new5[1x2x16,f32]', 'name': 'ln_linear'}),
                ('gemm', ['new4[1x64x2x2x4,f32]'], 'w2@32x64', 'new6[1x32x2x2x4,f32]',
                 {'B': 1, 'Cin': 64, 'Vin': 16, 'M': 32, 'K': 64, 'Ncol': 16, 'bias': 'b2', 'bact': 2, 'name': 'linear'}),
                ('dropout_apply',
                 {'kind': 0, 'bits': 'dropout_keep_bits1.bits', 'p': 0.25, 't': 'new6[1x32x2x2x4,f32]', 'aux': 'new3[1x32x2x2x4,f32]'})],
        'out': ('dropout_apply1.out',),
        'saved': ('x', 'new2[1x2x16,f32]', 'new1[1x32x2x2x4,f32]', 'swm_inv_raw1.out', 'new3[1x32x2x2x4,f32]', 'new5[1x2x16,f32]',
                  'new4[1x64x2x2x4,f32]', 'swm_fwd_raw1.m', 'n1w', 'n1b', 'win@32x32', 'u0', 'v0', 'wout@32x32', 'n2w', 'n2b', 'w1@64x32', 'w2@32x64',
                  None, None, 'dropout_keep_bits1.bits'),
        'marks': [],
        'shapes': ((32, 32, 1, 1, 1), (32, 32, 1, 1, 1), (64, 32, 1, 1, 1), (32, 64, 1, 1, 1)),
        'prm': ('win', 'wout', 'bout', 'w1', 'b1', 'w2', 'b2'),
        'bwd': [('dropout_apply', {'kind': 0, 'bits': 'dropout_keep_bits1.bits', 'p': 0.25, 't': 'g2'}),
                ('gemm', ['dropout_apply2.out'], 'w2@32x64', 'new7[1x64x2x2x4,f32]',
                 {'B': 1, 'Cin': 32, 'Vin': 16, 'M': 64, 'K': 32, 'Ncol': 16, 'w_t': True, 'ldw': 64, 'emul': 'new4[1x64x2x2x4,f32]', 'emul_kind': 2,
                  'name': 'linear_dgrad'}),
                ('wgrad', 'dropout_apply2.out', ['new4[1x64x2x2x4,f32]'], 'new8[32x64,f32]',
                 {'B': 1, 'M': 32, 'Cin': 64, 'K': 64, 'Vq': 16, 'Ncols': 16, 'gbias': 'new9[32,f32]', 'qact': 2, 'name': 'wgrad_linear'}),
                ('dgrad_lnbwd',
                 {'gz': 'new7[1x64x2x2x4,f32]', 'w2': 'w1@64x32', 'x': 'new3[1x32x2x2x4,f32]', 'stats': 'new5[1x2x16,f32]', 'ln_w': 'n2w',
                  'gadd': 'g2'}),
                ('wgrad', 'new7[1x64x2x2x4,f32]', ['new3[1x32x2x2x4,f32]'], 'new10[64x32,f32]',
                 {'B': 1, 'M': 64, 'Cin': 32, 'K': 32, 'Vq': 16, 'Ncols': 16, 'gbias': 'new11[64,f32]', 'stats': 'new5[1x2x16,f32]',
                  'ln': ('n2w', 'n2b'), 'name': 'wgrad_ln_linear'}),
                ('gemm', ['dgrad_lnbwd1.gx'], 'wout@32x32', 'new12[1x32x2x2x4,f32]',
                 {'B': 1, 'Cin': 32, 'Vin': 16, 'M': 32, 'K': 32, 'Ncol': 16, 'w_t': True, 'ldw': 32, 'name': 'linear_dgrad'}),
                ('wgrad', 'dgrad_lnbwd1.gx', ['swm_inv_raw1.out'], 'new13[32x32,f32]',
                 {'B': 1, 'M': 32, 'Cin': 32, 'K': 32, 'Vq': 16, 'Ncols': 16, 'gbias': 'new14[32,f32]', 'name': 'wgrad_linear'}),
                ('swm_fwd_raw', {'x': 'new12[1x32x2x2x4,f32]', 'geo': 'geo', 'div': 2}),
                ('nmf_bwd_raw',
                 {'x': 'swm_fwd_raw1.m', 'u0': 'u0', 'v0': 'v0', 'gy': 'swm_fwd_raw2.m', 'gu': None, 'gv': None, 'T': 5, 'G': 1, 'solver': 1,
                  'eps': 1e-16}),
                ('swm_inv_raw', {'y': 'nmf_bwd_raw1.gx', 'geo': 'geo', 'average': False, 'gate': 'swm_fwd_raw1.m'}),
                ('dgrad_lnbwd',
                 {'gz': 'swm_inv_raw2.out', 'w2': 'win@32x32', 'x': 'x', 'stats': 'new2[1x2x16,f32]', 'ln_w': 'n1w', 'gadd': 'dgrad_lnbwd1.gx'}),
                ('wgrad', 'swm_inv_raw2.out', ['x'], 'new15[32x32,f32]',
                 {'B': 1, 'M': 32, 'Cin': 32, 'K': 32, 'Vq': 16, 'Ncols': 16, 'stats': 'new2[1x2x16,f32]', 'ln': ('n1w', 'n1b'),
                  'name': 'wgrad_ln_linear'})],
        'grads': ('dgrad_lnbwd2.gx', 'dgrad_lnbwd2.gg', 'dgrad_lnbwd2.gbt', 'new15[32x32,f32]@32x32x1x1x1', None, None,
                  'new13[32x32,f32]@32x32x1x1x1', 'new14[32,f32]', 'dgrad_lnbwd1.gg', 'dgrad_lnbwd1.gbt', 'new10[64x32,f32]@64x32x1x1x1',
                  'new11[64,f32]', 'new8[32x64,f32]@32x64x1x1x1', 'new9[32,f32]', None, None, None, None, None),
    },
    'G0-modular-g2none': {
        'fwd': [('gemm', ['x'], 'win@32x32', 'new1[1x32x2x2x4,f32]',
                 {'B': 1, 'Cin': 32, 'Vin': 16, 'M': 32, 'K': 32, 'Ncol': 16, 'ln': ('n1w', 'n1b', 1e-05), 'stats_out': 'new2[1x2x16,f32]', 'eact': 1,
                  'name': 'ln_linear'}),
                ('swm_fwd_raw', {'x': 'new1[1x32x2x2x4,f32]', 'geo': 'geo'}),
                ('nmf_fwd_raw', {'x': 'swm_fwd_raw1.m', 'u0': 'u0', 'v0': 'v0', 'T': 5, 'solver': 1, 'eps': 1e-16}),
                ('swm_inv_raw', {'y': 'nmf_fwd_raw1.y', 'geo': 'geo'}),
                ('gemm', ['swm_inv_raw1.out'], 'wout@32x32', 'new3[1x32x2x2x4,f32]',
                 {'B': 1, 'Cin': 32, 'Vin': 16, 'M': 32, 'K': 32, 'Ncol': 16, 'bias': 'bout', 'res': 'x', 'name': 'act_linear_res'}),
                ('gemm', ['new3[1x32x2x2x4,f32]'], 'w1@64x32', 'new4[1x64x2x2x4,f32]',
                 {'B': 1, 'Cin': 32, 'Vin': 16, 'M': 64, 'K': 32, 'Ncol': 16, 'bias': 'b1', 'ln': ('n2w', 'n2b', 1e-06),
                  'stats_out': 'new5[1x2x16,f32]', 'name': 'ln_linear'}),
                ('gemm', ['new4[1x64x2x2x4,f32]'], 'w2@32x64', 'new6[1x32x2x2x4,f32]',
                 {'B': 1, 'Cin': 64, 'Vin': 16, 'M': 32, 'K': 64, 'Ncol': 16, 'bias': 'b2', 'bact': 2, 'res': 'new3[1x32x2x2x4,f32]',
                  'name': 'act_linear_res'})],
        'out': ('new6[1x32x2x2x4,f32]',),
        'saved': ('x', 'new2[1x2x16,f32]', 'new1[1x32x2x2x4,f32]', 'swm_inv_raw1.out', 'new3[1x32x2x2x4,f32]', 'new5[1x2x16,f32]',
                  'new4[1x64x2x2x4,f32]', 'swm_fwd_raw1.m', 'n1w', 'n1b', 'win@32x32', 'u0', 'v0', 'wout@32x32', 'n2w', 'n2b', 'w1@64x32', 'w2@32x64',
                  None, None, None),
        'marks': [],
        'shapes': ((32, 32, 1, 1, 1), (32, 32, 1, 1, 1), (64, 32, 1, 1, 1), (32, 64, 1, 1, 1)),
        'prm': ('win', 'wout', 'bout', 'w1', 'b1', 'w2', 'b2'),
        'bwd': [('gemm', ['new7[1x32x2x2x4,f32]'], 'w2@32x64', 'new8[1x64x2x2x4,f32]',
                 {'B': 1, 'Cin': 32, 'Vin': 16, 'M': 64, 'K': 32, 'Ncol': 16, 'w_t': True, 'ldw': 64, 'emul': 'new4[1x64x2x2x4,f32]', 'emul_kind': 2,
                  'name': 'linear_dgrad'}),
                ('dgrad_lnbwd',
                 {'gz': 'new8[1x64x2x2x4,f32]', 'w2': 'w1@64x32', 'x': 'new3[1x32x2x2x4,f32]', 'stats': 'new5[1x2x16,f32]', 'ln_w': 'n2w',
                  'gadd': 'new7[1x32x2x2x4,f32]'}),
                ('gemm', ['dgrad_lnbwd1.gx'], 'wout@32x32', 'new9[1x32x2x2x4,f32]',
                 {'B': 1, 'Cin': 32, 'Vin': 16, 'M': 32, 'K': 32, 'Ncol': 16, 'w_t': True, 'ldw': 32, 'name': 'linear_dgrad'}),
                ('dgrad_lnbwd',
                 {'gz': 'new10[1x32x2x2x4,f32]', 'w2': 'win@32x32', 'x': 'x', 'stats': 'new2[1x2x16,f32]', 'ln_w': 'n1w', 'gadd': 'dgrad_lnbwd1.gx'}),
                ('wgrad_group',
                 [('new7[1x32x2x2x4,f32]', ['new4[1x64x2x2x4,f32]'], 'new11[32x64,f32]',
                   {'B': 1, 'M': 32, 'Cin': 64, 'K': 64, 'Vq': 16, 'Ncols': 16, 'gbias': 'new12[32,f32]', 'qact': 2}),
                  ('new8[1x64x2x2x4,f32]', ['new3[1x32x2x2x4,f32]'], 'new13[64x32,f32]',
                   {'B': 1, 'M': 64, 'Cin': 32, 'K': 32, 'Vq': 16, 'Ncols': 16, 'gbias': 'new14[64,f32]', 'stats': 'new5[1x2x16,f32]',
                    'ln': ('n2w', 'n2b')}),
                  ('dgrad_lnbwd1.gx', ['swm_inv_raw1.out'], 'new15[32x32,f32]',
                   {'B': 1, 'M': 32, 'Cin': 32, 'K': 32, 'Vq': 16, 'Ncols': 16, 'gbias': 'new16[32,f32]'}),
                  ('new10[1x32x2x2x4,f32]', ['x'], 'new17[32x32,f32]',
                   {'B': 1, 'M': 32, 'Cin': 32, 'K': 32, 'Vq': 16, 'Ncols': 16, 'stats': 'new2[1x2x16,f32]', 'ln': ('n1w', 'n1b')})],
                 'wgrad_block_32x64')],
        'grads': ('dgrad_lnbwd2.gx', 'dgrad_lnbwd2.gg', 'dgrad_lnbwd2.gbt', 'new17[32x32,f32]@32x32x1x1x1', None, None,
                  'new15[32x32,f32]@32x32x1x1x1', 'new16[32,f32]', 'dgrad_lnbwd1.gg', 'dgrad_lnbwd1.gbt', 'new13[64x32,f32]@64x32x1x1x1',
                  'new14[64,f32]', 'new11[32x64,f32]@32x64x1x1x1', 'new12[32,f32]', None, None, None, None, None),
    },
}

EXPECTED_DESC = {
    'mlp_fwd-f32': {
        'calls': [('timed', 'mlp_chain_fwd_32', 8192, 16, 131072),
                  ('fz_mlp_chain',
                   [{'mode': 0, 'inp': 'x1', 'w1': 'w12', 'w2': 'w22', 'b1': 'b1', 'b2': 'b2', 'ln_g': 'ln_w', 'ln_b': 'ln_b',
                     'ln_eps': 9.999999974752427e-07, 'stats': 'new1[1x2x16,f32]', 'z1': 'new2[1x64x2x2x4,f32]', 'gz1': None, 'x1': None,
                     'out': 'new3[1x32x2x2x4,f32]', 'part': None, 'B': 1, 'C': 32, 'H': 64, 'V': 16, 'act_dtype': 0, 'wpart': None, 'gw1': None,
                     'gb1': None, 'gw2': None, 'gb2': None, 'gln': None, 'glp': None, 'products': 0, 'pre_in': None, 'pre_w': None, 'pre_b': None,
                     'pre_res': None, 'pre_out': None, 'post_w': None, 'post_b': None, 'post_out': None, 'post_m': 0},
                    'stream'])],
        'returns': ('new3[1x32x2x2x4,f32]', 'new2[1x64x2x2x4,f32]', 'new1[1x2x16,f32]'),
    },
    'mlp_fwd-bf16-nobias': {
        'calls': [('timed', 'mlp_chain_fwd_32', 4096, 16, 131072),
                  ('fz_mlp_chain',
                   [{'mode': 0, 'inp': 'x1', 'w1': 'w12', 'w2': 'w22', 'b1': None, 'b2': None, 'ln_g': 'ln_w', 'ln_b': 'ln_b',
                     'ln_eps': 9.999999974752427e-07, 'stats': 'new1[1x2x16,f32]', 'z1': 'new2[1x64x2x2x4,bf16]', 'gz1': None, 'x1': None,
                     'out': 'new3[1x32x2x2x4,bf16]', 'part': None, 'B': 1, 'C': 32, 'H': 64, 'V': 16, 'act_dtype': 1, 'wpart': None, 'gw1': None,
                     'gb1': None, 'gw2': None, 'gb2': None, 'gln': None, 'glp': None, 'products': 0, 'pre_in': None, 'pre_w': None, 'pre_b': None,
                     'pre_res': None, 'pre_out': None, 'post_w': None, 'post_b': None, 'post_out': None, 'post_m': 0},
                    'stream'])],
        'returns': ('new3[1x32x2x2x4,bf16]', 'new2[1x64x2x2x4,bf16]', 'new1[1x2x16,f32]'),
    },
    'outproj-f32': {
        'calls': [('timed', 'outproj_mlp_chain_fwd_32', 12288, 16, 163840),
                  ('fz_mlp_chain',
                   [{'mode': 0, 'inp': None, 'w1': 'w12', 'w2': 'w22', 'b1': 'b1', 'b2': 'b2', 'ln_g': 'ln_w', 'ln_b': 'ln_b',
                     'ln_eps': 9.999999974752427e-07, 'stats': 'new1[1x2x16,f32]', 'z1': 'new2[1x64x2x2x4,f32]', 'gz1': None, 'x1': None,
                     'out': 'new3[1x32x2x2x4,f32]', 'part': None, 'B': 1, 'C': 32, 'H': 64, 'V': 16, 'act_dtype': 0, 'wpart': None, 'gw1': None,
                     'gb1': None, 'gw2': None, 'gb2': None, 'gln': None, 'glp': None, 'products': 0, 'pre_in': 'a', 'pre_w': 'wout2', 'pre_b': 'bout',
                     'pre_res': 'x', 'pre_out': 'new4[1x32x2x2x4,f32]', 'post_w': None, 'post_b': None, 'post_out': None, 'post_m': 0},
                    'stream'])],
        'returns': ('new4[1x32x2x2x4,f32]', 'new3[1x32x2x2x4,f32]', 'new2[1x64x2x2x4,f32]', 'new1[1x2x16,f32]'),
    },
    'outproj-bf16-nobias-head': {
        'calls': [('timed', 'outproj_mlp_chain_fwd_32', 6240, 16, 163840),
                  ('fz_mlp_chain',
                   [{'mode': 0, 'inp': None, 'w1': 'w12', 'w2': 'w22', 'b1': None, 'b2': None, 'ln_g': 'ln_w', 'ln_b': 'ln_b',
                     'ln_eps': 9.999999974752427e-07, 'stats': 'new1[1x2x16,f32]', 'z1': 'new2[1x64x2x2x4,bf16]', 'gz1': None, 'x1': None,
                     'out': 'new3[1x32x2x2x4,bf16]', 'part': None, 'B': 1, 'C': 32, 'H': 64, 'V': 16, 'act_dtype': 1, 'wpart': None, 'gw1': None,
                     'gb1': None, 'gw2': None, 'gb2': None, 'gln': None, 'glp': None, 'products': 0, 'pre_in': 'a', 'pre_w': 'wout2', 'pre_b': None,
                     'pre_res': 'x', 'pre_out': 'new4[1x32x2x2x4,bf16]', 'post_w': 'hw', 'post_b': None, 'post_out': 'new5[1x3x2x2x4,bf16]',
                     'post_m': 3},
                    'stream'])],
        'returns': ('new4[1x32x2x2x4,bf16]', 'new3[1x32x2x2x4,bf16]', 'new2[1x64x2x2x4,bf16]', 'new1[1x2x16,f32]', 'new5[1x3x2x2x4,bf16]'),
    },
    'outproj-f32-drop-p0p': {
        'calls': [('timed', 'outproj_mlp_chain_fwd_32', 12288, 16, 163840),
                  ('fz_mlp_chain_drop',
                   [{'mode': 0, 'inp': None, 'w1': 'w12', 'w2': 'w22', 'b1': 'b1', 'b2': 'b2', 'ln_g': 'ln_w', 'ln_b': 'ln_b',
                     'ln_eps': 9.999999974752427e-07, 'stats': 'new1[1x2x16,f32]', 'z1': 'new2[1x64x2x2x4,f32]', 'gz1': None, 'x1': None,
                     'out': 'new3[1x32x2x2x4,f32]', 'part': None, 'B': 1, 'C': 32, 'H': 64, 'V': 16, 'act_dtype': 0, 'wpart': None, 'gw1': None,
                     'gb1': None, 'gw2': None, 'gb2': None, 'gln': None, 'glp': None, 'products': 0, 'pre_in': 'a', 'pre_w': 'wout2', 'pre_b': 'bout',
                     'pre_res': 'x', 'pre_out': 'new4[1x32x2x2x4,f32]', 'post_w': None, 'post_b': None, 'post_out': None, 'post_m': 0},
                    {'m0': 'm0', 'm1': None, 'm2': 'm2', 's0': 1.1111111640930176, 's1': 0.0, 's2': 1.4285714626312256}, 'stream'])],
        'returns': ('new4[1x32x2x2x4,f32]', 'new3[1x32x2x2x4,f32]', 'new2[1x64x2x2x4,f32]', 'new1[1x2x16,f32]'),
    },
    'mlp_bwd-f32': {
        'calls': [('fz_mlp_partials', [1, 16]), ('timed', 'mlp_chain_bwd_32', 14336, 16, 131072),
                  ('fz_mlp_chain',
                   [{'mode': 1, 'inp': 'g2', 'w1': 'w12', 'w2': 'w22', 'b1': None, 'b2': None, 'ln_g': 'ln_w', 'ln_b': None, 'ln_eps': 0.0,
                     'stats': 'st', 'z1': 'z1', 'gz1': 'new1[1x64x2x2x4,f32]', 'x1': 'x1', 'out': 'new2[1x32x2x2x4,f32]', 'part': 'new3[3x64,f32]',
                     'B': 1, 'C': 32, 'H': 64, 'V': 16, 'act_dtype': 0, 'wpart': None, 'gw1': None, 'gb1': None, 'gw2': None, 'gb2': None,
                     'gln': None, 'glp': None, 'products': 0, 'pre_in': None, 'pre_w': None, 'pre_b': None, 'pre_res': None, 'pre_out': None,
                     'post_w': None, 'post_b': None, 'post_out': None, 'post_m': 0},
                    'stream']),
                  ('fz_reduce_rows', ['new3[3x64,f32]', 3, 64, 'new4[64,f32]', 'new5[64x64,f32]', 'stream'])],
        'returns': ('new1[1x64x2x2x4,f32]', 'new2[1x32x2x2x4,f32]', 'new4[64,f32]@32', 'new4[64,f32]+128@32'),
    },
    'mlp_bwd-bf16': {
        'calls': [('fz_mlp_partials', [1, 16]), ('timed', 'mlp_chain_bwd_32', 7168, 16, 131072),
                  ('fz_mlp_chain',
                   [{'mode': 1, 'inp': 'g2', 'w1': 'w12', 'w2': 'w22', 'b1': None, 'b2': None, 'ln_g': 'ln_w', 'ln_b': None, 'ln_eps': 0.0,
                     'stats': 'st', 'z1': 'z1', 'gz1': 'new1[1x64x2x2x4,bf16]', 'x1': 'x1', 'out': 'new2[1x32x2x2x4,bf16]', 'part': 'new3[3x64,f32]',
                     'B': 1, 'C': 32, 'H': 64, 'V': 16, 'act_dtype': 1, 'wpart': None, 'gw1': None, 'gb1': None, 'gw2': None, 'gb2': None,
                     'gln': None, 'glp': None, 'products': 0, 'pre_in': None, 'pre_w': None, 'pre_b': None, 'pre_res': None, 'pre_out': None,
                     'post_w': None, 'post_b': None, 'post_out': None, 'post_m': 0},
                    'stream']),
                  ('fz_reduce_rows', ['new3[3x64,f32]', 3, 64, 'new4[64,f32]', 'new5[64x64,f32]', 'stream'])],
        'returns': ('new1[1x64x2x2x4,bf16]', 'new2[1x32x2x2x4,bf16]', 'new4[64,f32]@32', 'new4[64,f32]+128@32'),
    },
    'mlp_bwd_wg-f32-h64': {
        'calls': [('fz_mlp_wgrad_workspace_bytes', [1, 16]), ('timed', 'mlp_chain_bwd_wgrad_32', 10240, 16, 262144),
                  ('fz_mlp_chain',
                   [{'mode': 2, 'inp': 'g2', 'w1': 'w12', 'w2': 'w22', 'b1': None, 'b2': None, 'ln_g': 'ln_w', 'ln_b': 'ln_b', 'ln_eps': 0.0,
                     'stats': 'st', 'z1': 'z1', 'gz1': None, 'x1': 'x1', 'out': 'new1[1x32x2x2x4,f32]', 'part': None, 'B': 1, 'C': 32, 'H': 64,
                     'V': 16, 'act_dtype': 0, 'wpart': 'new2[1024,f32]', 'gw1': 'new3[64x32,f32]', 'gb1': 'new4[64,f32]', 'gw2': 'new5[32x64,f32]',
                     'gb2': 'new6[32,f32]', 'gln': 'new7[64,f32]', 'glp': None, 'products': 0, 'pre_in': None, 'pre_w': None, 'pre_b': None,
                     'pre_res': None, 'pre_out': None, 'post_w': None, 'post_b': None, 'post_out': None, 'post_m': 0},
                    'stream'])],
        'returns': ('new1[1x32x2x2x4,f32]', 'new7[64,f32]@32', 'new7[64,f32]+128@32', 'new3[64x32,f32]', 'new4[64,f32]', 'new5[32x64,f32]',
                    'new6[32,f32]'),
    },
    'mlp_bwd_wg-bf16-h128': {
        'calls': [('fz_mlp_wgrad_workspace_bytes', [1, 16]), ('timed', 'mlp_chain_bwd_wgrad_32x128', 13312, 16, 524288),
                  ('fz_mlp_chain',
                   [{'mode': 2, 'inp': 'g2', 'w1': 'w12', 'w2': 'w22', 'b1': None, 'b2': None, 'ln_g': 'ln_w', 'ln_b': 'ln_b', 'ln_eps': 0.0,
                     'stats': 'st', 'z1': 'z1', 'gz1': None, 'x1': 'x1', 'out': 'new1[1x32x2x2x4,bf16]', 'part': None, 'B': 1, 'C': 32, 'H': 128,
                     'V': 16, 'act_dtype': 1, 'wpart': 'new2[1024,f32]', 'gw1': 'new3[128x32,f32]', 'gb1': 'new4[128,f32]', 'gw2': 'new5[32x128,f32]',
                     'gb2': 'new6[32,f32]', 'gln': 'new7[64,f32]', 'glp': 'new8[1x32x2x2x4,f32]', 'products': 0, 'pre_in': None, 'pre_w': None,
                     'pre_b': None, 'pre_res': None, 'pre_out': None, 'post_w': None, 'post_b': None, 'post_out': None, 'post_m': 0},
                    'stream'])],
        'returns': ('new1[1x32x2x2x4,bf16]', 'new7[64,f32]@32', 'new7[64,f32]+128@32', 'new3[128x32,f32]', 'new4[128,f32]', 'new5[32x128,f32]',
                    'new6[32,f32]'),
    },
    'lnbwd-fused32-f32-nogadd': {
        'calls': [('fz_gemm_lnbwd_partials',
                   [{'x': ['gz', None, None, None], 'nsrc': 1, 'src_mode': 0, 'c0': 0, 'Cin': 64, 'Vin': 16, 'Di': 0, 'Hi': 0, 'Wi': 0, 'w': 'w2',
                     'w_t': 1, 'ldw': 32, 'M': 32, 'K': 64, 'bias': None, 'ln': 0, 'ln_g': None, 'ln_b': None, 'ln_eps': 0.0, 'stats_out': None,
                     'bact': 0, 'bmul': None, 'bmul_kind': 0, 'eact': 0, 'res': None, 'emul': None, 'emul_kind': 0, 'y': 'new1[1x32x2x2x4,f32]',
                     'Ncol': 16, 'Ho': 0, 'Wo': 0, 'B': 1, 'loader': 0, 'epilogue': 2, 'lnb_x': 'x', 'lnb_stats': 'stats', 'lnb_g': 'ln_w',
                     'lnb_gadd': None, 'lnb_part': None, 'act_dtype': 0, 'products': 0, 'tune': 0}]),
                  ('timed', 'dgrad_lnbwd_64->32', 8192, 16, 65536),
                  ('fz_gemm',
                   [{'x': ['gz', None, None, None], 'nsrc': 1, 'src_mode': 0, 'c0': 0, 'Cin': 64, 'Vin': 16, 'Di': 0, 'Hi': 0, 'Wi': 0, 'w': 'w2',
                     'w_t': 1, 'ldw': 32, 'M': 32, 'K': 64, 'bias': None, 'ln': 0, 'ln_g': None, 'ln_b': None, 'ln_eps': 0.0, 'stats_out': None,
                     'bact': 0, 'bmul': None, 'bmul_kind': 0, 'eact': 0, 'res': None, 'emul': None, 'emul_kind': 0, 'y': 'new1[1x32x2x2x4,f32]',
                     'Ncol': 16, 'Ho': 0, 'Wo': 0, 'B': 1, 'loader': 0, 'epilogue': 2, 'lnb_x': 'x', 'lnb_stats': 'stats', 'lnb_g': 'ln_w',
                     'lnb_gadd': None, 'lnb_part': 'new2[5x64,f32]', 'act_dtype': 0, 'products': 0, 'tune': 0},
                    'stream']),
                  ('fz_reduce_rows', ['new2[5x64,f32]', 5, 64, 'new3[64,f32]', 'new4[64x64,f32]', 'stream'])],
        'returns': ('new1[1x32x2x2x4,f32]', 'new3[64,f32]@32', 'new3[64,f32]+128@32'),
    },
    'lnbwd-fused64-bf16': {
        'calls': [('fz_gemm_lnbwd_partials',
                   [{'x': ['gz', None, None, None], 'nsrc': 1, 'src_mode': 0, 'c0': 0, 'Cin': 64, 'Vin': 16, 'Di': 0, 'Hi': 0, 'Wi': 0, 'w': 'w2',
                     'w_t': 1, 'ldw': 64, 'M': 64, 'K': 64, 'bias': None, 'ln': 0, 'ln_g': None, 'ln_b': None, 'ln_eps': 0.0, 'stats_out': None,
                     'bact': 0, 'bmul': None, 'bmul_kind': 0, 'eact': 0, 'res': None, 'emul': None, 'emul_kind': 0, 'y': 'new1[1x64x2x2x4,bf16]',
                     'Ncol': 16, 'Ho': 0, 'Wo': 0, 'B': 1, 'loader': 0, 'epilogue': 2, 'lnb_x': 'x', 'lnb_stats': 'stats', 'lnb_g': 'ln_w',
                     'lnb_gadd': 'gadd', 'lnb_part': None, 'act_dtype': 1, 'products': 0, 'tune': 0}]),
                  ('timed', 'dgrad_lnbwd_64->64', 8192, 16, 131072),
                  ('fz_gemm',
                   [{'x': ['gz', None, None, None], 'nsrc': 1, 'src_mode': 0, 'c0': 0, 'Cin': 64, 'Vin': 16, 'Di': 0, 'Hi': 0, 'Wi': 0, 'w': 'w2',
                     'w_t': 1, 'ldw': 64, 'M': 64, 'K': 64, 'bias': None, 'ln': 0, 'ln_g': None, 'ln_b': None, 'ln_eps': 0.0, 'stats_out': None,
                     'bact': 0, 'bmul': None, 'bmul_kind': 0, 'eact': 0, 'res': None, 'emul': None, 'emul_kind': 0, 'y': 'new1[1x64x2x2x4,bf16]',
                     'Ncol': 16, 'Ho': 0, 'Wo': 0, 'B': 1, 'loader': 0, 'epilogue': 2, 'lnb_x': 'x', 'lnb_stats': 'stats', 'lnb_g': 'ln_w',
                     'lnb_gadd': 'gadd', 'lnb_part': 'new2[5x128,f32]', 'act_dtype': 1, 'products': 0, 'tune': 0},
                    'stream']),
                  ('fz_reduce_rows', ['new2[5x128,f32]', 5, 128, 'new3[128,f32]', 'new4[64x128,f32]', 'stream'])],
        'returns': ('new1[1x64x2x2x4,bf16]', 'new3[128,f32]@64', 'new3[128,f32]+256@64'),
    },
    'lnbwd-two-launches-f32': {
        'calls': [('timed', 'linear_dgrad_128->64', 12288, 16, 262144),
                  ('fz_gemm',
                   [{'x': ['gz', None, None, None], 'nsrc': 1, 'src_mode': 0, 'c0': 0, 'Cin': 128, 'Vin': 16, 'Di': 0, 'Hi': 0, 'Wi': 0, 'w': 'w2',
                     'w_t': 1, 'ldw': 64, 'M': 64, 'K': 128, 'bias': None, 'ln': 0, 'ln_g': None, 'ln_b': None, 'ln_eps': 0.0, 'stats_out': None,
                     'bact': 0, 'bmul': None, 'bmul_kind': 0, 'eact': 0, 'res': None, 'emul': None, 'emul_kind': 0, 'y': 'new1[1x64x2x2x4,f32]',
                     'Ncol': 16, 'Ho': 0, 'Wo': 0, 'B': 1, 'loader': 0, 'epilogue': 0, 'lnb_x': None, 'lnb_stats': None, 'lnb_g': None,
                     'lnb_gadd': None, 'lnb_part': None, 'act_dtype': 0, 'products': 0, 'tune': 0},
                    'stream']),
                  ('fz_ln_bwd_workspace_bytes2', [1, 64, 16]), ('timed', 'ln_bwd_64', 12288, 16, 0),
                  ('fz_ln_bwd',
                   ['new1[1x64x2x2x4,f32]', 'x', 'stats', 'ln_w', 'gadd', 'new2[1x64x2x2x4,f32]', 'new3[128,f32]', 'new4[256,f32]', 1, 64, 16, 0,
                    'stream'])],
        'returns': ('new2[1x64x2x2x4,f32]', 'new3[128,f32]@64', 'new3[128,f32]+256@64'),
    },
    'head-act_linear_res-f32': {
        'calls': [('fz_head_bwd_rows', []), ('fz_head_bwd_workspace_bytes', []), ('timed', 'head_bwd_32->3', 4288, 16, 0),
                  ('fz_head_bwd', ['gy', 'z', 'w', 'new1[1x32x2x2x4,f32]', 'new2[924,f32]', 1, 3, 32, 16, 0, 'stream']),
                  ('fz_chunk_reduce_ld', ['new2[924,f32]', 7, 96, 132, 'new3[3x32,f32]', 0, 'stream']),
                  ('fz_chunk_reduce_ld', ['new2[924,f32]+512', 7, 3, 132, 'new4[3,f32]', 0, 'stream'])],
        'returns': ('new1[1x32x2x2x4,f32]', 'new3[3x32,f32]@3x32x1x1x1', 'new4[3,f32]', 'gy', None),
    },
    'head-of_block-bf16-f32grad-nobias': {
        'calls': [('fz_head_bwd_rows', []), ('fz_head_bwd_workspace_bytes', []), ('timed', 'head_bwd_32->3', 2144, 16, 0),
                  ('fz_head_bwd', ['unregistered', 'z', 'w', 'new1[1x32x2x2x4,bf16]', 'new2[924,f32]', 1, 3, 32, 16, 1, 'stream']),
                  ('fz_chunk_reduce_ld', ['new2[924,f32]', 7, 96, 132, 'new3[3x32,f32]', 0, 'stream']),
                  ('fz_chunk_reduce_ld', ['new2[924,f32]+512', 7, 3, 132, 'new4[3,f32]', 0, 'stream'])],
        'returns': ('new1[1x32x2x2x4,bf16]', 'new3[3x32,f32]@3x32x1x1x1', None, None),
    },
}
