"""CPU checks of the CNN blocks (factorizer_amd/cnn.py) and of the default block of ft.UNet / ft.UNetStage against the reference's
own results (tests/golden/g12_cnn.npz): state_dict keys and their order, seed -> bit-identical initial parameters, outputs and
gradients; the fusion gate of a norm and the activation behind it."""
import numpy as np
import pytest
import torch
from torch import nn

import cnn_cases as CC
import factorizer_amd as ft
import parity as P
from factorizer_amd import cnn


@pytest.fixture(scope="module")
def gold():
    return CC.golden()


def _run(m, gold, name):
    x = torch.from_numpy(gold[f"{name}:x"]).requires_grad_(True)
    y = m(x)
    names = [k for k, _ in m.named_parameters()]
    grads = torch.autograd.grad(y, [x] + list(m.parameters()), torch.from_numpy(gold[f"{name}:gy"]))
    return y, grads[0], dict(zip(names, grads[1:]))


@pytest.mark.parametrize("name", list(CC.BLOCKS))
def test_blocks_against_the_reference(gold, name):
    m = CC.make_block(name)
    assert list(m.state_dict()) == list(gold[f"{name}:keys"])
    for k, p in m.named_parameters():
        assert np.array_equal(p.detach().numpy(), gold[f"{name}:p:{k}"]), k       # the seed gives the reference's parameters
    y, gx, gp = _run(m, gold, name)
    P.close(f"{name} y", y, torch.from_numpy(gold[f"{name}:y"]))
    P.close(f"{name} gx", gx, torch.from_numpy(gold[f"{name}:gx"]))
    for k, g in gp.items():
        P.close(f"{name} d{k}", g, torch.from_numpy(gold[f"{name}:g:{k}"]))


@pytest.mark.parametrize("name", list(CC.UNETS))
def test_default_unet_against_the_reference(gold, name):
    m = CC.make_unet(name)
    assert list(m.state_dict()) == list(gold[f"{name}:keys"])
    for k, p in m.named_parameters():
        assert np.array_equal(CC.digest(p), gold[f"{name}:p:{k}"]), k
    y, gx, gp = _run(m, gold, name)
    P.close(f"{name} y", y, torch.from_numpy(gold[f"{name}:y"]))
    P.close(f"{name} gx", gx, torch.from_numpy(gold[f"{name}:gx"]))
    for k, g in gp.items():   # the digest of each parameter gradient: every entry is a sum of numel terms, so the floor is
        # P.close's relative 1e-4 of the sum of absolute values (an element-wise error of 1e-4 max|g| moves an entry by less)
        P.close(f"{name} d{k} digest", torch.from_numpy(CC.digest(g)), torch.from_numpy(gold[f"{name}:g:{k}"]),
                floor=1e-4 * float(gold[f"{name}:g:{k}"][1]) + 1e-6)


def test_defaults_construct_and_name_their_submodules_like_the_reference():
    st = ft.UNetStage(8, 16, depth=2)
    assert all(type(b) is ft.DoubleConv for b in st.blocks)
    assert list(st.state_dict())[:4] == ["blocks.0.block1.0.weight", "blocks.0.block1.0.bias", "blocks.0.block1.2.weight",
                                         "blocks.0.block1.2.bias"]
    net = ft.UNet(4, 3, stem=(ft.Conv3d, {"kernel_size": 3, "padding": 1}))
    dc = net.encoder.blocks[0].block           # (the reference hands DoubleConv over as the stage: unet.py:215-220, 54)
    assert type(dc) is ft.DoubleConv and type(dc.block1[0]) is ft.Conv3d and type(dc.block1[2]) is ft.GroupNorm
    assert (dc.block1[2].num_groups, dc.block1[2].num_channels) == (8, 32) and type(dc.block1[3]) is nn.LeakyReLU
    assert type(dc.block1[1]) is nn.Dropout and dc.block1[1].p == 0.0
    assert dc.block1[0].kernel_size == (3, 3, 3) and dc.block1[0].padding == (1, 1, 1)
    assert type(net.decoder.blocks[-1].block) is ft.DoubleConv
    net2 = ft.UNet(4, 3, spatial_dims=2, stem=(ft.Conv2d, {"kernel_size": 3, "padding": 1}))
    assert type(net2.encoder.blocks[1].block.block2[0]) is ft.Conv2d
    assert type(ft.UNet(32, 3, spatial_dims=1).encoder.blocks[0].block.block1[0]) is nn.Conv1d
    with pytest.raises(RuntimeError):                                   # like the reference: no stem, 4 channels into a 32-channel conv
        ft.UNet(4, 3)(torch.zeros(1, 4, 16, 16, 16))
    b = ft.BasicBlock(8, 8)
    assert type(b.shortcut) is nn.Identity and not hasattr(ft.PreActivationBlock(8, 8), "shortcut")
    assert type(ft.BasicBlock(8, 16).shortcut) is ft.Conv3d and ft.BasicBlock(8, 16).shortcut.bias is None
    s = ft.SepConv(8)
    assert list(s.state_dict()) == ["pwconv1.linear.weight", "dwconv.weight", "dwconv.bias", "pwconv2.linear.weight",
                                    "pwconv2.linear.bias"]
    assert type(s.pwconv1) is ft.Linear and type(s.dwconv) is nn.Conv3d and s.dwconv.groups == 16


def test_the_fusion_gate_leaves_hooked_or_subclassed_modules_alone():
    class MyNorm(ft.GroupNorm):
        pass

    class MyAct(nn.LeakyReLU):
        pass

    n, a = ft.GroupNorm(2, 4), nn.LeakyReLU(0.2)
    assert cnn.fused_act(n, a) == ("leaky_relu", 0.2) and cnn.fused_act(n, nn.ReLU()) == ("relu", 0.0)
    assert cnn.fused_act(MyNorm(2, 4), a) is None and cnn.fused_act(n, MyAct()) is None
    assert cnn.fused_act(nn.GroupNorm(2, 4), a) is None and cnn.fused_act(n, nn.GELU()) is None
    assert cnn.fused_act(ft.InstanceNorm3d(4), a) is None
    seen = []
    h = a.register_forward_hook(lambda m, i, o: seen.append("act"))
    assert cnn.fused_act(n, a) is None
    x = torch.randn(2, 4, 5)
    y = cnn.norm_act(n, a, x)
    assert seen == ["act"] and torch.equal(y, a(n(x)))
    h.remove()
    h = n.register_forward_pre_hook(lambda m, i: seen.append("norm"))
    assert cnn.fused_act(n, a) is None
    h.remove()
    assert cnn.fused_act(n, a) is not None and torch.equal(cnn.norm_act(n, a, x), a(n(x)))
    # a block with a hooked activation still calls it
    blk = ft.DoubleConv(2, 4, norm=(ft.GroupNorm, (2,)))
    blk.block1[3].register_forward_hook(lambda m, i, o: seen.append("block"))
    blk(torch.randn(1, 2, 4, 4, 4))
    assert seen[-1] == "block"


@pytest.mark.parametrize("name", CC.GPU_CASES)
def test_fp32_gates_against_float64_stay_within_the_tie_cap(name):
    """the cases of tests/test_gpu_cnn_blocks.py with the committed seeds: the gates the fp32 CPU module has differ from float64's
    signs only at ties (|z64| within P.close's bound of that tensor), at most 8 per activation and 32 per case; under those
    gates fp32 and float64 agree at P.close's default bound"""
    m, x, gy = CC.gpu_case(name)
    gates = []
    with CC.record_gates(gates):
        y, grads = CC.run(m, x, gy)
    assert len(gates) == {"double": 2, "basic": 2, "preact": 2, "sep": 0, "unet3d": 10, "unet2d": 10}[name]
    y64, g64, ties, _ = CC.gated_float64(m, x, gy, gates)
    print("ties per activation:", ties)
    CC.check_ties(ties)
    P.close(f"{name} y (fp32 CPU, float64 under its gates)", y, y64)
    for k, a, b in zip(["x"] + [k for k, _ in m.named_parameters()], grads, g64):
        P.close(f"{name} d{k} (fp32 CPU, float64 under its gates)", a, b)
