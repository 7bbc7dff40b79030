"""Cases, reference and bounds of the instance norm tests (tests/test_instance_norm_cpu.py: the host emulation;
tests/test_gpu_instance_norm.py: the kernels).

Reference: F.instance_norm and its autograd in float64 on the CPU, on the very inputs the kernel sees (bf16 inputs upcast).
Bound for y and gx, element-wise: |got − ref| <= u (|ref| + 1e-3 max|ref|), u = 2^-23 (fp32) / 2^-7 (bf16): one unit in the last
place; the contract — float64 arithmetic, one rounding per stored element — is half of that, the second term covers elements that
cancel to near zero.  Bound for dγ, dβ: |got − ref| <= 2^-23 |ref| + 2^-30 Σ|terms|: one rounding plus the worst-case float64
summation error of up to 8M terms."""
import torch
import torch.nn.functional as F

EPS = 1e-5
U = {torch.float32: 2.0 ** -23, torch.bfloat16: 2.0 ** -7}
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def _randn(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def seams(one_pass_max, chunks):
    """sizes at which the code takes another path, from the library's own answers: the seam between the one-launch and the
    two-launch path, the last V of one chunk, the first of two, and three full chunks + 5"""
    lo, hi = 1, 1 << 24
    assert chunks(lo) == 1 and chunks(hi) > 1
    while hi - lo > 1:                       # the largest V that is one chunk (the chunk count does not fall with V)
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if chunks(mid) == 1 else (lo, mid)
    L = lo
    assert chunks(L) == 1 and chunks(L + 1) == 2 and chunks(3 * L + 5) == 4
    return {"one_pass_max-1": one_pass_max - 1, "one_pass_max": one_pass_max, "one_pass_max+1": one_pass_max + 1,
            "chunk_last_of_1": L, "chunk_first_of_2": L + 1, "chunk_3_plus_5": 3 * L + 5}


FIXED = {
    "tail_odd_planes": lambda: _randn((3, 5, 4099), 1),
    "smallest_v": lambda: _randn((2, 3, 2), 2),
    "below_a_wave": lambda: _randn((2, 3, 7), 3),
    "relu_3d": lambda: torch.relu(_randn((2, 4, 8, 9, 11), 4)),
    "single_plane": lambda: _randn((1, 1, 777), 5),
    "tiny_planes_3d": lambda: _randn((2, 512, 2, 2, 2), 6),
    "tiny_planes_1d": lambda: _randn((2, 512, 8), 7),
    "mean_far_from_zero": lambda: 1000 + _randn((2, 3, 4099), 8),
    "large_scale_offset": lambda: 1e4 * _randn((2, 3, 1023), 9) + 5e5,
    "var_near_eps": lambda: 1e-3 * _randn((2, 3, 1023), 10),
    "ragged_chunks": lambda: 300 * _randn((2, 3, 70001), 11) + 7,
    "storage_offset_odd_v": lambda: _randn((1 + 2 * 3 * 4099,), 12)[1:].view(2, 3, 4099),
    "permuted": lambda: _randn((2, 9, 11, 3), 13).permute(0, 3, 1, 2),
}
SEAMS = ["one_pass_max-1", "one_pass_max", "one_pass_max+1", "chunk_last_of_1", "chunk_first_of_2", "chunk_3_plus_5"]
CASES = sorted(FIXED) + SEAMS


def make(name, dtype, affine, seam_sizes):
    """x (CPU, of `dtype`, possibly a view), weight, bias (fp32 or None), gy (of `dtype`)"""
    if name in FIXED:
        x = FIXED[name]()
    else:
        x = _randn((1, 2, seam_sizes[name]), 20 + SEAMS.index(name))
    if dtype != torch.float32:
        if x.is_contiguous() and x.storage_offset():      # keep the one-element storage offset in the narrower type
            flat = torch.zeros(1 + x.numel(), dtype=dtype)
            flat[1:] = x.reshape(-1).to(dtype)
            x = flat[1:].view(x.shape)
        else:
            x = x.to(dtype)
    C = x.shape[1]
    g = torch.Generator().manual_seed(99)
    w = (1 + 0.5 * torch.randn(C, generator=g)) if affine else None
    b = torch.randn(C, generator=g) if affine else None
    gy = torch.randn(x.shape, generator=g).to(dtype)
    return x, w, b, gy


def to_device(x, dev):
    """x on `dev` with the same storage offset and strides"""
    off = x.storage_offset()
    if x.is_contiguous() and off:
        flat = torch.zeros(off + x.numel(), dtype=x.dtype, device=dev)
        flat[off:] = x.reshape(-1).to(dev)
        return flat[off:].view(x.shape)
    return x.to(dev)   # keeps the strides of a permuted tensor


def reference(x, w, b, gy, eps=EPS):
    """float64: y, gx, gw, gb and the Σ|terms| of gw, gb"""
    x64 = x.double().contiguous().requires_grad_(True)
    ps = [p.double().requires_grad_(True) for p in (w, b) if p is not None]
    y = F.instance_norm(x64, weight=ps[0] if ps else None, bias=ps[1] if ps else None, eps=eps)
    g64 = gy.double()
    grads = torch.autograd.grad(y, [x64] + ps, g64)
    out = {"y": y.detach(), "gx": grads[0]}
    if ps:
        dims = [0] + list(range(2, x.dim()))
        xd = x64.detach()
        xhat = (xd - xd.mean(dims[1:], keepdim=True)) / (xd.var(dims[1:], unbiased=False, keepdim=True) + eps).sqrt()
        out.update(gw=grads[1], gb=grads[2], gw_terms=(g64 * xhat).abs().sum(dims), gb_terms=g64.abs().sum(dims))
    return out


def ratio_elementwise(got, ref, dtype):
    """max over the elements of |got − ref| / (u (|ref| + 1e-3 max|ref|)): the bound is 1"""
    got, ref = got.detach().double().cpu(), ref.double()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    bound = U[dtype] * (ref.abs() + 1e-3 * ref.abs().max())
    err = (got - ref).abs()
    return float((err / bound.clamp_min(1e-300)).max()) if float(err.max()) > 0 else 0.0


def ratio_param(got, ref, terms):
    got = got.detach().double().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    bound = 2.0 ** -23 * ref.abs() + 2.0 ** -30 * terms
    err = (got - ref).abs()
    return float((err / bound.clamp_min(1e-300)).max()) if float(err.max()) > 0 else 0.0


def check(got, ref, dtype, note=None):
    """got: dict y, gx[, gw, gb]; prints each achieved fraction of its bound before asserting"""
    r = {"y": ratio_elementwise(got["y"], ref["y"], dtype), "gx": ratio_elementwise(got["gx"], ref["gx"], dtype)}
    if "gw" in ref:
        r["gw"] = ratio_param(got["gw"], ref["gw"], ref["gw_terms"])
        r["gb"] = ratio_param(got["gb"], ref["gb"], ref["gb_terms"])
    print("fraction of the bound:", r)
    if note:
        note(r)
    for k, v in r.items():
        assert v <= 1.0, f"{k}: {v:.3f} of the bound"
    return r
