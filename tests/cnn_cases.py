"""The modules of tests/golden/g12_cnn.npz (tools/make_goldens.py g12) built from the package, for tests/test_cnn_blocks_cpu.py
and tests/test_gpu_cnn_blocks.py."""
import os

import numpy as np
import torch

import factorizer_amd as ft

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g12_cnn.npz")

BLOCKS = {  # name: (class, in, out, kwargs); the fixture's input is (2, in, 4, 4, 8); seeds as in the recipe
    "double": (ft.DoubleConv, 8, 16, {}), "basic": (ft.BasicBlock, 8, 16, {}), "preact": (ft.PreActivationBlock, 8, 16, {}),
    "sep": (ft.SepConv, 8, 16, {}), "basic_s2": (ft.BasicBlock, 8, 16, {"stride": 2}),
    "preact_s2": (ft.PreActivationBlock, 8, 16, {"stride": 2}),
}
UNETS = {"unet3d": (3, (1, 2, 16, 16, 16)), "unet2d": (2, (1, 2, 32, 32))}


def golden():
    return np.load(GOLDEN)


def make_block(name, cin=None, cout=None):
    cls, i, o, kw = BLOCKS[name]
    torch.manual_seed(1200 + list(BLOCKS).index(name))
    return cls(cin or i, cout or o, **kw)


def make_unet(name, **kw):
    nd, shape = UNETS[name]
    conv = {3: ft.Conv3d, 2: ft.Conv2d}[nd]
    torch.manual_seed(1280 + list(UNETS).index(name))
    return ft.UNet(shape[1], 3, spatial_dims=nd, encoder_depth=(1, 1, 1), encoder_width=(16, 32, 64), strides=(1, 2, 2),
                   decoder_depth=(1, 1), stem=(conv, {"kernel_size": 3, "padding": 1}), **kw)


def digest(t):
    """the fixture's digest of a tensor: sum, sum of absolute values, three projections on fixed random vectors, in float64"""
    t = t.detach().double().reshape(-1)
    r = torch.randn(3, t.numel(), dtype=torch.float64, generator=torch.Generator().manual_seed(t.numel()))
    return np.array([t.sum().item(), t.abs().sum().item(), *(r @ t).tolist()])


# ---- activation gates: record the ones a run had, replay them in another run of the same module --------------------------------
# A LeakyReLU gate is [y > 0] of the activation's OUTPUT (slope > 0: the sign of the pre-activation), so it can be read off the
# fused norm + activation too.  Activations are visited in execution order, which is the same for every copy of a module.
import contextlib  # noqa: E402

import torch.nn.functional as F  # noqa: E402
from torch import nn  # noqa: E402

from factorizer_amd import cnn  # noqa: E402

TIES_PER_ACT, TIES_PER_TEST = 8, 32


@contextlib.contextmanager
def _patched(norm_act, leaky_forward):
    old = cnn.norm_act, nn.LeakyReLU.forward
    cnn.norm_act, nn.LeakyReLU.forward = norm_act, leaky_forward
    try:
        yield
    finally:
        cnn.norm_act, nn.LeakyReLU.forward = old


def record_gates(gates):
    """context: every LeakyReLU (fused behind its norm or called as a module) appends [y > 0] of its output to `gates`"""
    orig_na, orig_fw = cnn.norm_act, nn.LeakyReLU.forward

    def norm_act(norm, act, x):
        y = orig_na(norm, act, x)
        if cnn.fused_act(norm, act) is not None:       # (else the module's forward below has recorded it)
            gates.append((y.detach() > 0).cpu())
        return y

    def forward(self, x):
        y = orig_fw(self, x)
        gates.append((y.detach() > 0).cpu())
        return y

    return _patched(norm_act, forward)


def replay_gates(gates, ties=None, tie_bound=None):
    """context: every LeakyReLU keeps its own VALUE leaky_relu(z) and takes its derivative from the next mask of `gates`.  With
    `ties` (a list): where a mask differs from the sign of z the element must be a tie, |z| <= tie_bound(z) (asserted); the count
    per activation is appended."""
    it = iter(gates)
    orig_na = cnn.norm_act

    def gated(z, slope):
        gate = next(it)
        zd = z.detach()
        if ties is not None:
            diff = (zd > 0) != gate
            if diff.any():
                worst, bound = float(zd[diff].abs().max()), tie_bound(zd)
                print(f"gate ties: {int(diff.sum())}, worst |z| {worst:.3e}, bound {bound:.3e}")
                assert worst <= bound, (worst, bound)
            ties.append(int(diff.sum()))
        factor = torch.where(gate, 1.0, slope).to(z.dtype)
        return F.leaky_relu(zd, slope) + factor * (z - zd)

    def norm_act(norm, act, x):
        if cnn.fused_act(norm, act) is None:
            return orig_na(norm, act, x)
        return gated(norm(x), act.negative_slope)

    def forward(self, x):
        return gated(x, self.negative_slope)

    return _patched(norm_act, forward)


def close_bound(z, rel=1e-4, floor=1e-6):
    """parity.close's default bound for the tensor z"""
    return rel * float(z.abs().max()) + floor


def run(m, x, gy):
    """y and the gradients of x and of every parameter (in named_parameters order)"""
    xr = x.detach().clone().requires_grad_(True)
    y = m(xr)
    grads = torch.autograd.grad(y, [xr] + list(m.parameters()), gy)
    return y.detach(), grads


def gated_float64(m, x, gy, gates, tie_bound=close_bound):
    """the module in float64 and in fp32 on the CPU under `gates`: (y64, grads64, ties per activation, extra) where extra[i] is
    the fp32 CPU module's own distance to float64 for y (i = 0) and each gradient (i = 1 ...)"""
    import copy
    ties = []
    m64, m32 = copy.deepcopy(m).double().cpu(), copy.deepcopy(m).float().cpu()
    with replay_gates(gates, ties, tie_bound):
        y64, g64 = run(m64, x.double().cpu(), gy.double().cpu())
    with replay_gates(gates):
        y32, g32 = run(m32, x.float().cpu(), gy.float().cpu())
    extra = [float((a.double() - b).abs().max()) for a, b in zip((y32, *g32), (y64, *g64))]
    assert len(ties) == len(gates)
    return y64, g64, ties, extra


def check_ties(ties):
    assert all(t <= TIES_PER_ACT for t in ties) and sum(ties) <= TIES_PER_TEST, ties


GPU_CASES = ["double", "basic", "preact", "sep", "unet3d", "unet2d"]


def gpu_case(name):
    """the module (on the CPU), x and dL/dy of tests/test_gpu_cnn_blocks.py: blocks at (16 -> 32, 8x8x8), the fixture's UNets, B = 2"""
    g = torch.Generator().manual_seed(3 + GPU_CASES.index(name))
    if name in BLOCKS:
        return make_block(name, 16, 32), torch.randn(2, 16, 8, 8, 8, generator=g), torch.randn(2, 32, 8, 8, 8, generator=g)
    shape = UNETS[name][1]
    return make_unet(name), torch.randn(2, *shape[1:], generator=g), torch.randn(2, 3, *shape[2:], generator=g)
