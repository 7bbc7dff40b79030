"""-m gpu: the native instance norm (csrc/inorm.hip through ft.instance_norm / ft.InstanceNorm*d) against F.instance_norm and
its autograd in float64 on the CPU, on the inputs the kernel sees, at the bounds of tests/inorm_cases.py (one unit in the last
place for y and gx; one rounding plus the float64 summation error for dγ, dβ); the exact properties (a constant plane, repeats,
independence of the batch); the fallbacks; ft.Deconver on the native norm."""
import importlib
import warnings

import pytest
import torch
from torch import nn

import factorizer_amd as ft
import inorm_cases as IC
import parity as P
from factorizer_amd import _native, composed

IN = importlib.import_module("factorizer_amd.instance_norm")   # (ft.instance_norm is the function of that name)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16


@pytest.fixture(scope="module")
def seam_sizes():
    L = _native.lib()
    return IC.seams(L.fz_inorm_one_pass_max(), L.fz_inorm_chunks)


def run(x, w, b, gy):
    """forward and backward on the device through the public function; asserts the launches"""
    xd = IC.to_device(x, DEV).requires_grad_(True)
    wd, bd = (None if p is None else p.to(DEV).requires_grad_(True) for p in (w, b))
    V = x[0, 0].numel()
    n0 = _native.launch_count()
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        y = ft.instance_norm(xd, wd, bd, IC.EPS)
        assert _native.launch_count() - n0 == IN.launches(V)
        grads = torch.autograd.grad(y, [xd] + [p for p in (wd, bd) if p is not None], gy.to(DEV))
    assert _native.launch_count() - n0 == IN.launches(V) + IN.launches(V, backward=True, affine=w is not None)
    assert y.dtype == x.dtype and grads[0].dtype == x.dtype and y.is_contiguous()
    out = {"y": y.detach(), "gx": grads[0]}
    if w is not None:
        assert grads[1].dtype == grads[2].dtype == torch.float32
        out.update(gw=grads[1], gb=grads[2])
    return out, xd


@pytest.mark.parametrize("affine", [False, True], ids=["plain", "affine"])
@pytest.mark.parametrize("dtype", sorted(IC.DTYPES))
@pytest.mark.parametrize("name", IC.CASES)
def test_against_float64(seam_sizes, name, dtype, affine):
    dt = IC.DTYPES[dtype]
    x, w, b, gy = IC.make(name, dt, affine, seam_sizes)
    got, xd = run(x, w, b, gy)
    if name == "storage_offset_odd_v":
        assert xd.is_contiguous() and xd.data_ptr() % 16 != 0        # planes off the 16-byte boundary
    if name == "permuted":
        assert not xd.is_contiguous()
    IC.check(got, IC.reference(x, w, b, gy), dt,
             note=lambda r: P.note(f"instance norm {name} {dtype} {'affine' if affine else 'plain'}: fraction of the bound", **r))


@pytest.mark.parametrize("dtype", sorted(IC.DTYPES))
def test_exact_properties(dtype):
    dt = IC.DTYPES[dtype]
    # a constant plane at 1e6: y == 0 exactly, a finite gx within the bound
    x = torch.full((2, 3, 4099), 1e6).to(dt)
    gy = IC._randn(x.shape, 31).to(dt)
    got, _ = run(x, None, None, gy)
    assert torch.count_nonzero(got["y"]) == 0
    r = IC.ratio_elementwise(got["gx"], IC.reference(x, None, None, gy)["gx"], dt)
    P.note(f"instance norm constant plane {dtype}: gx fraction of the bound", gx=r)
    assert r <= 1.0
    for name in ("tail_odd_planes", "ragged_chunks"):                 # the one-launch and the two-launch path
        x, w, b, gy = IC.make(name, dt, True, None)
        one, _ = run(x, w, b, gy)
        two, _ = run(x, w, b, gy)
        assert all(torch.equal(one[k], two[k]) for k in ("y", "gx", "gw", "gb")), name
        # the planes of x[1:2] alone (a tensor of its own, at another address) equal those planes of the batched run
        part, _ = run(x[1:2].clone(), w, b, gy[1:2].clone())
        assert torch.equal(one["y"][1:2], part["y"]) and torch.equal(one["gx"][1:2], part["gx"]), name


def test_eval_without_running_statistics_equals_training():
    torch.manual_seed(1)
    m = ft.InstanceNorm3d(4, affine=True).to(DEV)
    x = torch.randn(2, 4, 5, 6, 7, device=DEV)
    n0 = _native.launch_count()
    y_train = m(x)
    y_eval = m.eval()(x)
    assert _native.launch_count() - n0 == 2 and torch.equal(y_train, y_eval)
    assert torch.equal(m(x[0]), y_eval[0])                            # an unbatched input: the same planes
    with pytest.raises(ValueError, match="more than 1 spatial element"):
        m(torch.randn(2, 4, 1, 1, 1, device=DEV))


# ------------------------------------------------------------------ fallbacks ---------------------------------------------
@pytest.mark.parametrize("case", ["track_running_stats", "fp16"])
def test_fallbacks_warn_once_and_match_the_framework(case):
    torch.manual_seed(2)
    kw = dict(affine=True, track_running_stats=case == "track_running_stats")
    mine, theirs = ft.InstanceNorm3d(4, **kw).to(DEV), nn.InstanceNorm3d(4, **kw).to(DEV)
    x = torch.randn(2, 4, 5, 6, 7, device=DEV)
    if case == "fp16":
        x, mine, theirs = x.half(), mine.half(), theirs.half()
    composed._warned.clear()
    n0 = _native.launch_count()
    with pytest.warns(RuntimeWarning, match="outside the native kernel set"):
        y = mine(x)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)               # once
        y2 = mine(x)
    assert _native.launch_count() == n0
    ref = theirs(x)
    ref2 = theirs(x)
    assert torch.equal(y, ref) and torch.equal(y2, ref2)
    assert all(torch.equal(a, b) for a, b in zip(mine.state_dict().values(), theirs.state_dict().values()))
    if case == "track_running_stats":                                # eval with running statistics: another reason, its own warning
        with pytest.warns(RuntimeWarning, match="eval mode with running statistics"):
            y3 = mine.eval()(x)
        assert torch.equal(y3, theirs.eval()(x))


# ------------------------------------------------------------------ the network -------------------------------------------
def _net(nd, **kw):
    torch.manual_seed(0)
    return ft.Deconver(in_channels=2, out_channels=3, spatial_dims=nd, encoder_width=(8, 16), encoder_depth=(1, 1),
                       strides=(1, 2), decoder_depth=(1,), act=nn.ReLU, groups=-1, ratio=1, kernel_size=(3,) * nd, num_iters=2,
                       mlp_ratio=2, dropout=0.0, **kw).to(DEV)


def _spy(monkeypatch):
    """counts the calls of the library's two instance norm entry points"""
    L = _native.lib()
    calls = {"fwd": 0, "bwd": 0}
    fwd, bwd = L.fz_inorm_fwd, L.fz_inorm_bwd

    def spy_fwd(*a):
        calls["fwd"] += 1
        return fwd(*a)

    def spy_bwd(*a):
        calls["bwd"] += 1
        return bwd(*a)

    monkeypatch.setattr(L, "fz_inorm_fwd", spy_fwd)
    monkeypatch.setattr(L, "fz_inorm_bwd", spy_bwd)
    return calls


@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "bf16_autocast"])
@pytest.mark.parametrize("nd", [3, 2])
def test_deconver_on_the_native_norm(nd, autocast, monkeypatch):
    """ft.Deconver (widths (8, 16), one down-sampling; 16^3 / 16 x 24) with norm=ft.InstanceNorm*d: forward and backward without a
    RuntimeWarning; the launch counter rises over the same network on the framework norm by exactly the norm's launches; finite
    and bit-identical when repeated.  The distance to the framework norm on the same weights is recorded, not asserted: no bound
    for a whole network can be derived."""
    native_cls, framework_cls = {3: (ft.InstanceNorm3d, nn.InstanceNorm3d), 2: (ft.InstanceNorm2d, nn.InstanceNorm2d)}[nd]
    model, plain = _net(nd, norm=native_cls), _net(nd, norm=framework_cls)
    plain.load_state_dict(model.state_dict())
    norms = [m for m in model.modules() if isinstance(m, native_cls)]
    assert norms and not any(type(m) is native_cls for m in plain.modules())
    torch.manual_seed(8)
    shape = (1, 2, 16, 16, 16) if nd == 3 else (2, 2, 16, 24)
    x = torch.rand(*shape, device=DEV)
    gy = torch.rand(shape[0], 3, *shape[2:], device=DEV)
    seen = []
    hooks = [m.register_forward_hook(lambda m, i, o: seen.append((i[0][0, 0].numel(), m.affine))) for m in norms]

    def go(net):
        composed._warned.clear()
        n0 = _native.launch_count()
        with warnings.catch_warnings(), torch.autocast("cuda", dtype=BF, enabled=autocast):
            warnings.simplefilter("error", RuntimeWarning)
            y = net(x)
            grads = torch.autograd.grad(y, list(net.parameters()), gy.to(y.dtype), allow_unused=True)
        return y, grads, _native.launch_count() - n0

    calls = _spy(monkeypatch)
    y1, g1, n_native = go(model)
    assert calls["fwd"] == calls["bwd"] == len(seen) > 0
    expect = sum(IN.launches(V) + IN.launches(V, backward=True, affine=a) for V, a in seen)
    y2, g2, _ = go(model)
    for h in hooks:
        h.remove()
    before = dict(calls)
    y0, g0, n_plain = go(plain)
    assert calls == before                                            # a framework norm given as norm= stays the framework's
    assert n_native - n_plain == expect
    assert torch.isfinite(y1.float()).all() and torch.equal(y1, y2)
    for (k, _), a, b in zip(model.named_parameters(), g1, g2):
        if a is None:
            continue
        assert a.dtype == torch.float32 and torch.isfinite(a).all(), k
        assert torch.equal(a, b), k
    P.note(f"deconver {nd}-D {'bf16 autocast' if autocast else 'fp32'}: native norm against the framework norm, same weights",
           rel_l2=((y1.float() - y0.float()).norm() / y0.float().norm()).item())


def test_a_framework_norm_launches_no_native_norm_kernel(monkeypatch):
    """norm=nn.InstanceNorm2d keeps running the framework's kernels; converting the model is what opts in"""
    calls = _spy(monkeypatch)
    model = _net(2, norm=nn.InstanceNorm2d)
    x = torch.rand(2, 2, 16, 24, device=DEV)
    model(x).sum().backward()
    assert calls == {"fwd": 0, "bwd": 0}
    conv = ft.convert_instance_norm(model)
    with torch.no_grad():
        y = conv(x)
    assert calls["fwd"] > 0 and calls["bwd"] == 0 and torch.isfinite(y).all()
