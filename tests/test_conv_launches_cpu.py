"""No GPU: the launches of the U-shape's convolution nodes, pinned.  ConvK2S2Fn / SkipConvK2S2Fn / TConvK2S2Fn / ConvK3Fn take
4-D and 5-D activations and read everything that depends on the rank from one table (pointwise._RANK); the kernels see only what
`_gemm` / `_wgrad` put into their descriptors, so equal arguments there are equal device results.  Here those two functions are
replaced by recorders, every node's forward and backward run on CPU tensors against a stand-in ctx, and the recorded calls are
compared with EXPECTED — written down from the same recorder run on the separate 2-D / 3-D classes these nodes replace, and not
to be regenerated from the code under test."""
import pytest
import torch

from factorizer_amd import pointwise as PW

F32 = "torch.float32"


class _Ctx(PW._Ctx):
    def __init__(self, *needs):
        self.needs_input_grad = needs


class _Recorder:
    """`_gemm` / `_wgrad` / `_warn_composed` stand-ins: each call becomes (kind, operand roles..., keyword arguments) with every
    tensor replaced by its role name, by the name of the derived tensor it equals, or by its (shape, dtype)."""

    def __init__(self, monkeypatch, roles, derived=None):
        self.calls = []
        self.roles = {id(t): k for k, t in roles.items() if t is not None}
        self.derived = derived or {}
        monkeypatch.setattr(PW, "_gemm", self.gemm)
        monkeypatch.setattr(PW, "_wgrad", self.wgrad)
        monkeypatch.setattr(PW, "_warn_composed", self.warn)

    def d(self, t):
        if not isinstance(t, torch.Tensor):
            return t
        if id(t) in self.roles:
            return self.roles[id(t)]
        for k, v in self.derived.items():
            if v.shape == t.shape and torch.equal(v, t):
                return k
        return (tuple(t.shape), str(t.dtype))

    def kw(self, kw):
        return {k: self.d(v) for k, v in kw.items()}

    def gemm(self, xs, w, y, **kw):
        self.calls.append(("gemm", [self.d(t) for t in xs], self.d(w), self.d(y), self.kw(kw)))
        return y

    def wgrad(self, p, qs, gw, **kw):
        self.calls.append(("wgrad", self.d(p), [self.d(t) for t in qs], self.d(gw), self.kw(kw)))
        return gw

    def warn(self, op, x, *more):
        self.calls.append(("warn", op, self.d(x)))

    def outs(self, res):
        return [self.d(t) for t in (res if isinstance(res, tuple) else (res,))]


SHAPES = {   # form -> rank -> (x, w); the gradient of the output has the shape the forward returned
    "k2s2": {2: ((1, 4, 8, 8), (6, 4, 2, 2)), 3: ((1, 4, 4, 4, 8), (6, 4, 2, 2, 2))},
    "tconv": {2: ((1, 6, 4, 4), (6, 4, 2, 2)), 3: ((1, 6, 2, 2, 4), (6, 4, 2, 2, 2))},
    # 3-D: 10 input channels, past the stem kernel's C * 27 * 64 * 4 <= 65536, so the generic tap loader is the one taken
    "k3": {2: ((1, 4, 4, 8), (6, 4, 3, 3)), 3: ((1, 10, 2, 4, 8), (6, 10, 3, 3, 3))},
}


def _operands(form, nd, bias=True, odd_o=False):
    torch.manual_seed(nd)
    xs, ws = SHAPES[form][nd]
    if odd_o:
        ws = (5, *ws[1:])
    x, w = torch.randn(xs), torch.randn(ws)
    b = torch.randn(ws[1] if form == "tconv" else ws[0]) if bias else None
    return x, w, b


def _trace(monkeypatch, case):
    form, nd, variant = case
    bias = variant in ("bias", "noinput", "bias_fwd")
    x, w, b = _operands(form, nd, bias=bias and not (form == "tconv" and variant == "noinput"), odd_o=variant == "odd_o")
    roles = {"x": x, "w": w, "b": b}
    derived = {"flip(w).T": torch.flip(w, dims=tuple(range(2, 2 + nd))).transpose(0, 1).contiguous()} if form == "k3" else {}
    rec = _Recorder(monkeypatch, roles, derived)
    need_x = variant != "noinput"
    if form == "k3":
        ctx = _Ctx(need_x, True, True) if nd == 2 else _Ctx(need_x, True, True, False)   # both call forms: (x, w, b) and (x, w, b, pro)
        Fn = PW.ConvK3Fn
        res = Fn.forward(ctx, x, w, b) if nd == 2 else Fn.forward(ctx, x, w, b, None)
    else:
        ctx = _Ctx(need_x, True, True)
        Fn = {"k2s2": PW.SkipConvK2S2Fn if variant == "skip" else PW.ConvK2S2Fn, "tconv": PW.TConvK2S2Fn}[form]
        res = Fn.forward(ctx, x, w, b)
    out = {"fwd": rec.calls, "y": rec.outs(res), "has_bias": ctx.has_bias, "saved": rec.outs(tuple(ctx.saved_tensors))}
    if variant == "bias_fwd":
        return out, None
    rec.calls = []
    y = res[1] if variant == "skip" else res
    gy = torch.randn(y.shape)
    rec.roles[id(gy)] = "gy"
    if variant == "skip":
        g_skip = torch.randn(x.shape)
        rec.roles[id(g_skip)] = "g_skip"
        grads = Fn.backward(ctx, g_skip, gy)
    else:
        grads = Fn.backward(ctx, gy)
    out.update(bwd=rec.calls, grads=rec.outs(grads))
    return out, (x, w, gy, grads)


CASES = [(form, nd, v) for form, vs in (("k2s2", ("bias", "skip", "noinput")), ("tconv", ("nobias", "bias_fwd", "noinput")),
                                        ("k3", ("bias", "odd_o", "noinput"))) for nd in (2, 3) for v in vs]


@pytest.mark.parametrize("case", CASES, ids=["{}-{}d-{}".format(*c) for c in CASES])
def test_launches_are_the_recorded_ones(monkeypatch, case):
    got, more = _trace(monkeypatch, case)
    assert got == EXPECTED[case]
    if case[2] == "odd_o":   # the composed input gradient is the framework's
        x, w, gy, grads = more
        ref = (torch.nn.grad.conv2d_input if case[1] == 2 else torch.nn.grad.conv3d_input)(x.shape, w, gy, padding=1)
        assert torch.equal(grads[0], ref)


@pytest.mark.parametrize("nd", [2, 3])
def test_skip_node_without_a_down_path_gradient_passes_the_skip_gradient_through(monkeypatch, nd):
    x, w, b = _operands("k2s2", nd)
    rec = _Recorder(monkeypatch, {"x": x, "w": w, "b": b})
    ctx = _Ctx(True, True, True)
    Fn = PW.SkipConvK2S2Fn
    skip, y = Fn.forward(ctx, x, w, b)
    assert skip.shape == x.shape and skip.data_ptr() == x.data_ptr()
    rec.calls = []
    g_skip = torch.randn(x.shape)
    grads = Fn.backward(ctx, g_skip, None)
    assert grads[0] is g_skip and grads[1:] == (None, None) and len(grads) == 3
    assert rec.calls == []


@pytest.mark.parametrize("nd", [2, 3])
def test_a_prologue_outside_the_stem_kernel_is_refused(monkeypatch, nd):
    x, w, b = _operands("k3", nd)
    rec = _Recorder(monkeypatch, {"x": x, "w": w, "b": b})
    pro = (torch.ones(6), torch.zeros(6), 1e-5, torch.randn(6, 6))
    with pytest.raises(RuntimeError, match="ConvK3Fn: a block prologue needs the stem kernel"):
        PW.ConvK3Fn.forward(_Ctx(False, True, True, False), x, w, b, pro)
    assert rec.calls == []


# (form, rank, variant) -> the record.  Loader / epilogue ids: FZ_LOAD_S2D 1, FZ_LOAD_K3 2, FZ_LOAD_S2D_2D 3, FZ_LOAD_K3_2D 4,
# FZ_EPI_D2S 1, FZ_EPI_D2S_2D 3 (include/factorizer_hip.h).  A keyword that is absent was not passed.
EXPECTED = {
    ("k2s2", 2, "bias"): dict(
        fwd=[
            ("gemm", ["x"], "w", ((1, 6, 4, 4), F32), dict(B=1, Cin=4, Vin=64, M=6, K=16, Ncol=16, bias="b", loader=3, Di=1, Hi=8, Wi=8,
                Ho=4, Wo=4, name="conv2d_k2s2")),
        ],
        y=[((1, 6, 4, 4), F32)],
        has_bias=True,
        saved=["x", "w"],
        bwd=[
            ("gemm", ["gy"], "w", ((1, 4, 8, 8), F32), dict(B=1, Cin=6, Vin=16, M=16, K=6, Ncol=16, w_t=True, ldw=16, epilogue=3, Ho=4,
                Wo=4, res=None, name="conv2d_k2s2_dgrad")),
            ("wgrad", "gy", ["x"], ((6, 4, 2, 2), F32), dict(B=1, M=6, Cin=4, K=16, Vq=64, Ncols=16, gbias=((6,), F32), loader=3, D=1, H=8,
                W=8, Ho=4, Wo=4, name="wgrad_conv2d_k2s2")),
        ],
        grads=[((1, 4, 8, 8), F32), ((6, 4, 2, 2), F32), ((6,), F32)],
    ),
    ("k2s2", 2, "skip"): dict(
        fwd=[
            ("gemm", ["x"], "w", ((1, 6, 4, 4), F32), dict(B=1, Cin=4, Vin=64, M=6, K=16, Ncol=16, bias=None, loader=3, Di=1, Hi=8, Wi=8,
                Ho=4, Wo=4, name="conv2d_k2s2")),
        ],
        y=[((1, 4, 8, 8), F32), ((1, 6, 4, 4), F32)],
        has_bias=False,
        saved=["x", "w"],
        bwd=[
            ("gemm", ["gy"], "w", ((1, 4, 8, 8), F32), dict(B=1, Cin=6, Vin=16, M=16, K=6, Ncol=16, w_t=True, ldw=16, epilogue=3, Ho=4,
                Wo=4, res="g_skip", name="conv2d_k2s2_dgrad")),
            ("wgrad", "gy", ["x"], ((6, 4, 2, 2), F32), dict(B=1, M=6, Cin=4, K=16, Vq=64, Ncols=16, gbias=((6,), F32), loader=3, D=1, H=8,
                W=8, Ho=4, Wo=4, name="wgrad_conv2d_k2s2")),
        ],
        grads=[((1, 4, 8, 8), F32), ((6, 4, 2, 2), F32), None],
    ),
    ("k2s2", 2, "noinput"): dict(
        fwd=[
            ("gemm", ["x"], "w", ((1, 6, 4, 4), F32), dict(B=1, Cin=4, Vin=64, M=6, K=16, Ncol=16, bias="b", loader=3, Di=1, Hi=8, Wi=8,
                Ho=4, Wo=4, name="conv2d_k2s2")),
        ],
        y=[((1, 6, 4, 4), F32)],
        has_bias=True,
        saved=["x", "w"],
        bwd=[
            ("wgrad", "gy", ["x"], ((6, 4, 2, 2), F32), dict(B=1, M=6, Cin=4, K=16, Vq=64, Ncols=16, gbias=((6,), F32), loader=3, D=1, H=8,
                W=8, Ho=4, Wo=4, name="wgrad_conv2d_k2s2")),
        ],
        grads=[None, ((6, 4, 2, 2), F32), ((6,), F32)],
    ),
    ("k2s2", 3, "bias"): dict(
        fwd=[
            ("gemm", ["x"], "w", ((1, 6, 2, 2, 4), F32), dict(B=1, Cin=4, Vin=128, M=6, K=32, Ncol=16, bias="b", loader=1, Di=4, Hi=4, Wi=8,
                Ho=2, Wo=4, name="conv_k2s2")),
        ],
        y=[((1, 6, 2, 2, 4), F32)],
        has_bias=True,
        saved=["x", "w"],
        bwd=[
            ("gemm", ["gy"], "w", ((1, 4, 4, 4, 8), F32), dict(B=1, Cin=6, Vin=16, M=32, K=6, Ncol=16, w_t=True, ldw=32, epilogue=1, Ho=2,
                Wo=4, res=None, name="conv_k2s2_dgrad")),
            ("wgrad", "gy", ["x"], ((6, 4, 2, 2, 2), F32), dict(B=1, M=6, Cin=4, K=32, Vq=128, Ncols=16, gbias=((6,), F32), loader=1, D=4,
                H=4, W=8, Ho=2, Wo=4, name="wgrad_conv_k2s2")),
        ],
        grads=[((1, 4, 4, 4, 8), F32), ((6, 4, 2, 2, 2), F32), ((6,), F32)],
    ),
    ("k2s2", 3, "skip"): dict(
        fwd=[
            ("gemm", ["x"], "w", ((1, 6, 2, 2, 4), F32), dict(B=1, Cin=4, Vin=128, M=6, K=32, Ncol=16, bias=None, loader=1, Di=4, Hi=4,
                Wi=8, Ho=2, Wo=4, name="conv_k2s2")),
        ],
        y=[((1, 4, 4, 4, 8), F32), ((1, 6, 2, 2, 4), F32)],
        has_bias=False,
        saved=["x", "w"],
        bwd=[
            ("gemm", ["gy"], "w", ((1, 4, 4, 4, 8), F32), dict(B=1, Cin=6, Vin=16, M=32, K=6, Ncol=16, w_t=True, ldw=32, epilogue=1, Ho=2,
                Wo=4, res="g_skip", name="conv_k2s2_dgrad")),
            ("wgrad", "gy", ["x"], ((6, 4, 2, 2, 2), F32), dict(B=1, M=6, Cin=4, K=32, Vq=128, Ncols=16, gbias=((6,), F32), loader=1, D=4,
                H=4, W=8, Ho=2, Wo=4, name="wgrad_conv_k2s2")),
        ],
        grads=[((1, 4, 4, 4, 8), F32), ((6, 4, 2, 2, 2), F32), None],
    ),
    ("k2s2", 3, "noinput"): dict(
        fwd=[
            ("gemm", ["x"], "w", ((1, 6, 2, 2, 4), F32), dict(B=1, Cin=4, Vin=128, M=6, K=32, Ncol=16, bias="b", loader=1, Di=4, Hi=4, Wi=8,
                Ho=2, Wo=4, name="conv_k2s2")),
        ],
        y=[((1, 6, 2, 2, 4), F32)],
        has_bias=True,
        saved=["x", "w"],
        bwd=[
            ("wgrad", "gy", ["x"], ((6, 4, 2, 2, 2), F32), dict(B=1, M=6, Cin=4, K=32, Vq=128, Ncols=16, gbias=((6,), F32), loader=1, D=4,
                H=4, W=8, Ho=2, Wo=4, name="wgrad_conv_k2s2")),
        ],
        grads=[None, ((6, 4, 2, 2, 2), F32), ((6,), F32)],
    ),
    ("tconv", 2, "nobias"): dict(
        fwd=[
            ("gemm", ["x"], "w", ((1, 4, 8, 8), F32), dict(B=1, Cin=6, Vin=16, M=16, K=6, Ncol=16, w_t=True, ldw=16, bias=None, epilogue=3,
                Ho=4, Wo=4, name="tconv2d_k2s2")),
        ],
        y=[((1, 4, 8, 8), F32)],
        has_bias=False,
        saved=["x", "w"],
        bwd=[
            ("gemm", ["gy"], "w", ((1, 6, 4, 4), F32), dict(B=1, Cin=4, Vin=64, M=6, K=16, Ncol=16, loader=3, Di=1, Hi=8, Wi=8, Ho=4, Wo=4,
                name="tconv2d_k2s2_dgrad")),
            ("wgrad", "x", ["gy"], ((6, 4, 2, 2), F32), dict(B=1, M=6, Cin=4, K=16, Vq=64, Ncols=16, loader=3, D=1, H=8, W=8, Ho=4, Wo=4,
                name="wgrad_tconv2d_k2s2")),
        ],
        grads=[((1, 6, 4, 4), F32), ((6, 4, 2, 2), F32), None],
    ),
    ("tconv", 2, "bias_fwd"): dict(
        fwd=[
            ("gemm", ["x"], "w", ((1, 4, 8, 8), F32), dict(B=1, Cin=6, Vin=16, M=16, K=6, Ncol=16, w_t=True, ldw=16, bias="b", epilogue=3,
                Ho=4, Wo=4, name="tconv2d_k2s2")),
        ],
        y=[((1, 4, 8, 8), F32)],
        has_bias=True,
        saved=["x", "w"],
    ),
    ("tconv", 2, "noinput"): dict(
        fwd=[
            ("gemm", ["x"], "w", ((1, 4, 8, 8), F32), dict(B=1, Cin=6, Vin=16, M=16, K=6, Ncol=16, w_t=True, ldw=16, bias=None, epilogue=3,
                Ho=4, Wo=4, name="tconv2d_k2s2")),
        ],
        y=[((1, 4, 8, 8), F32)],
        has_bias=False,
        saved=["x", "w"],
        bwd=[
            ("wgrad", "x", ["gy"], ((6, 4, 2, 2), F32), dict(B=1, M=6, Cin=4, K=16, Vq=64, Ncols=16, loader=3, D=1, H=8, W=8, Ho=4, Wo=4,
                name="wgrad_tconv2d_k2s2")),
        ],
        grads=[None, ((6, 4, 2, 2), F32), None],
    ),
    ("tconv", 3, "nobias"): dict(
        fwd=[
            ("gemm", ["x"], "w", ((1, 4, 4, 4, 8), F32), dict(B=1, Cin=6, Vin=16, M=32, K=6, Ncol=16, w_t=True, ldw=32, bias=None,
                epilogue=1, Ho=2, Wo=4, name="tconv_k2s2")),
        ],
        y=[((1, 4, 4, 4, 8), F32)],
        has_bias=False,
        saved=["x", "w"],
        bwd=[
            ("gemm", ["gy"], "w", ((1, 6, 2, 2, 4), F32), dict(B=1, Cin=4, Vin=128, M=6, K=32, Ncol=16, loader=1, Di=4, Hi=4, Wi=8, Ho=2,
                Wo=4, name="tconv_k2s2_dgrad")),
            ("wgrad", "x", ["gy"], ((6, 4, 2, 2, 2), F32), dict(B=1, M=6, Cin=4, K=32, Vq=128, Ncols=16, loader=1, D=4, H=4, W=8, Ho=2,
                Wo=4, name="wgrad_tconv_k2s2")),
        ],
        grads=[((1, 6, 2, 2, 4), F32), ((6, 4, 2, 2, 2), F32), None],
    ),
    ("tconv", 3, "bias_fwd"): dict(
        fwd=[
            ("gemm", ["x"], "w", ((1, 4, 4, 4, 8), F32), dict(B=1, Cin=6, Vin=16, M=32, K=6, Ncol=16, w_t=True, ldw=32, bias="b",
                epilogue=1, Ho=2, Wo=4, name="tconv_k2s2")),
        ],
        y=[((1, 4, 4, 4, 8), F32)],
        has_bias=True,
        saved=["x", "w"],
    ),
    ("tconv", 3, "noinput"): dict(
        fwd=[
            ("gemm", ["x"], "w", ((1, 4, 4, 4, 8), F32), dict(B=1, Cin=6, Vin=16, M=32, K=6, Ncol=16, w_t=True, ldw=32, bias=None,
                epilogue=1, Ho=2, Wo=4, name="tconv_k2s2")),
        ],
        y=[((1, 4, 4, 4, 8), F32)],
        has_bias=False,
        saved=["x", "w"],
        bwd=[
            ("wgrad", "x", ["gy"], ((6, 4, 2, 2, 2), F32), dict(B=1, M=6, Cin=4, K=32, Vq=128, Ncols=16, loader=1, D=4, H=4, W=8, Ho=2,
                Wo=4, name="wgrad_tconv_k2s2")),
        ],
        grads=[None, ((6, 4, 2, 2, 2), F32), None],
    ),
    ("k3", 2, "bias"): dict(
        fwd=[
            ("gemm", ["x"], "w", ((1, 6, 4, 8), F32), dict(B=1, Cin=4, Vin=32, M=6, K=36, Ncol=32, bias="b", loader=4, Di=1, Hi=4, Wi=8,
                name="conv2d_k3")),
        ],
        y=[((1, 6, 4, 8), F32)],
        has_bias=True,
        saved=["x", "w"],
        bwd=[
            ("gemm", ["gy"], "flip(w).T", ((1, 4, 4, 8), F32), dict(B=1, Cin=6, Vin=32, M=4, K=54, Ncol=32, loader=4, Di=1, Hi=4, Wi=8,
                name="conv2d_k3_dgrad")),
            ("wgrad", "gy", ["x"], ((6, 4, 3, 3), F32), dict(B=1, M=6, Cin=4, K=36, Vq=32, Ncols=32, gbias=((6,), F32), loader=4, D=1, H=4,
                W=8, name="wgrad_conv2d_k3")),
        ],
        grads=[((1, 4, 4, 8), F32), ((6, 4, 3, 3), F32), ((6,), F32)],
    ),
    ("k3", 2, "odd_o"): dict(
        fwd=[
            ("gemm", ["x"], "w", ((1, 5, 4, 8), F32), dict(B=1, Cin=4, Vin=32, M=5, K=36, Ncol=32, bias=None, loader=4, Di=1, Hi=4, Wi=8,
                name="conv2d_k3")),
        ],
        y=[((1, 5, 4, 8), F32)],
        has_bias=False,
        saved=["x", "w"],
        bwd=[
            ("warn", "Conv2d(k=3) input gradient", "x"),
            ("wgrad", "gy", ["x"], ((5, 4, 3, 3), F32), dict(B=1, M=5, Cin=4, K=36, Vq=32, Ncols=32, gbias=((5,), F32), loader=4, D=1, H=4,
                W=8, name="wgrad_conv2d_k3")),
        ],
        grads=[((1, 4, 4, 8), F32), ((5, 4, 3, 3), F32), None],
    ),
    ("k3", 2, "noinput"): dict(
        fwd=[
            ("gemm", ["x"], "w", ((1, 6, 4, 8), F32), dict(B=1, Cin=4, Vin=32, M=6, K=36, Ncol=32, bias="b", loader=4, Di=1, Hi=4, Wi=8,
                name="conv2d_k3")),
        ],
        y=[((1, 6, 4, 8), F32)],
        has_bias=True,
        saved=["x", "w"],
        bwd=[
            ("wgrad", "gy", ["x"], ((6, 4, 3, 3), F32), dict(B=1, M=6, Cin=4, K=36, Vq=32, Ncols=32, gbias=((6,), F32), loader=4, D=1, H=4,
                W=8, name="wgrad_conv2d_k3")),
        ],
        grads=[None, ((6, 4, 3, 3), F32), ((6,), F32)],
    ),
    ("k3", 3, "bias"): dict(
        fwd=[
            ("gemm", ["x"], "w", ((1, 6, 2, 4, 8), F32), dict(B=1, Cin=10, Vin=64, M=6, K=270, Ncol=64, bias="b", loader=2, Di=2, Hi=4,
                Wi=8, name="conv_k3")),
        ],
        y=[((1, 6, 2, 4, 8), F32)],
        has_bias=True,
        saved=["x", "w"],
        bwd=[
            ("gemm", ["gy"], "flip(w).T", ((1, 10, 2, 4, 8), F32), dict(B=1, Cin=6, Vin=64, M=10, K=162, Ncol=64, loader=2, Di=2, Hi=4,
                Wi=8, name="conv_k3_dgrad")),
            ("wgrad", "gy", ["x"], ((6, 10, 3, 3, 3), F32), dict(B=1, M=6, Cin=10, K=270, Vq=64, Ncols=64, gbias=((6,), F32), loader=2, D=2,
                H=4, W=8, name="wgrad_conv_k3")),
        ],
        grads=[((1, 10, 2, 4, 8), F32), ((6, 10, 3, 3, 3), F32), ((6,), F32), None],
    ),
    ("k3", 3, "odd_o"): dict(
        fwd=[
            ("gemm", ["x"], "w", ((1, 5, 2, 4, 8), F32), dict(B=1, Cin=10, Vin=64, M=5, K=270, Ncol=64, bias=None, loader=2, Di=2, Hi=4,
                Wi=8, name="conv_k3")),
        ],
        y=[((1, 5, 2, 4, 8), F32)],
        has_bias=False,
        saved=["x", "w"],
        bwd=[
            ("warn", "Conv3d(k=3) input gradient", "x"),
            ("wgrad", "gy", ["x"], ((5, 10, 3, 3, 3), F32), dict(B=1, M=5, Cin=10, K=270, Vq=64, Ncols=64, gbias=((5,), F32), loader=2, D=2,
                H=4, W=8, name="wgrad_conv_k3")),
        ],
        grads=[((1, 10, 2, 4, 8), F32), ((5, 10, 3, 3, 3), F32), None, None],
    ),
    ("k3", 3, "noinput"): dict(
        fwd=[
            ("gemm", ["x"], "w", ((1, 6, 2, 4, 8), F32), dict(B=1, Cin=10, Vin=64, M=6, K=270, Ncol=64, bias="b", loader=2, Di=2, Hi=4,
                Wi=8, name="conv_k3")),
        ],
        y=[((1, 6, 2, 4, 8), F32)],
        has_bias=True,
        saved=["x", "w"],
        bwd=[
            ("wgrad", "gy", ["x"], ((6, 10, 3, 3, 3), F32), dict(B=1, M=6, Cin=10, K=270, Vq=64, Ncols=64, gbias=((6,), F32), loader=2, D=2,
                H=4, W=8, name="wgrad_conv_k3")),
        ],
        grads=[None, ((6, 10, 3, 3, 3), F32), ((6,), F32), None],
    ),
}
