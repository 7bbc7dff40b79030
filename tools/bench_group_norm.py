"""Device time per call of the native group norm with its fused activation (ft.group_norm(act="leaky_relu"), csrc/gnorm.hip)
against nn.GroupNorm + nn.LeakyReLU on the same device (profiles/group_norm.md), G = 8, affine, on the stage shapes of the CNN U-Net:

    3d   B = 2,  (C, 128^3 / 64^3 / 32^3 / 16^3 / 8^3)    for C = 32 / 64 / 128 / 256 / 512
    2d   B = 16, (C, 512^2 / 256^2 / 128^2 / 64^2 / 32^2) for the same widths

Per shape, in fp32 and bf16: the forward alone and forward + backward (input and parameter gradients).  The framework has no
bf16-activation / fp32-parameter group norm of its own: the bf16 baseline is the fp32 modules on the input cast to fp32 and the
result cast back ("framework"), and the same modules under torch.autocast, whose fp32 list holds group_norm and whose output stays
fp32 ("framework_autocast").  Method, windows and the
repeated baseline are those of tools/bench_instance_norm.py, whose helpers this tool uses.  Bytes of the native kernels, from the
shapes: a group of cg V <= fz_gnorm_one_pass_max() elements is read once per direction and tensor, a larger one twice; one write.
One more row: forward + backward of the five-stage ft.UNet(4, 3, stem = k3) at 2 x 128^3 against the same model built on
nn.GroupNorm (framework norm and activation).  A run without a GPU fails.

    python tools/bench_group_norm.py [--rounds 10] [--window-ms 20] [--only 3d] [--no-network] [--out group_norm.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import factorizer_amd as ft  # noqa: E402
from bench_instance_norm import alternate, copy_rate, summary  # noqa: E402
from factorizer_amd import _native  # noqa: E402

WIDTHS = (32, 64, 128, 256, 512)
G = 8
SHAPES = {"3d": [(2, c, (128 >> i,) * 3) for i, c in enumerate(WIDTHS)],
          "2d": [(16, c, (512 >> i,) * 2) for i, c in enumerate(WIDTHS)]}


def native_bytes(numel, esize, span, backward):
    reads = 1 if span <= _native.lib().fz_gnorm_one_pass_max() else 2
    n = reads + 1
    if backward:
        n += 2 * reads + 1
    return n * numel * esize


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--window-ms", type=float, default=20.0)
    ap.add_argument("--only", default=None)
    ap.add_argument("--no-network", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_group_norm.py measures device time: no GPU found")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "window_ms": a.window_ms,
           "copy_bytes_per_s": copy_rate(dev), "one_pass_max": _native.lib().fz_gnorm_one_pass_max(), "rows": []}
    for kind, shapes in SHAPES.items():
        if a.only and kind != a.only:
            continue
        for B, C, S in shapes:
            mine = ft.GroupNorm(G, C).to(dev)
            theirs = nn.Sequential(nn.GroupNorm(G, C), nn.LeakyReLU()).to(dev)
            for dtype in (torch.float32, torch.bfloat16):
                torch.manual_seed(0)
                x = torch.randn(B, C, *S, device=dev).to(dtype)
                g = torch.randn(B, C, *S, device=dev).to(dtype)
                V = x[0, 0].numel()
                native = lambda t: mine.forward_act(t, "leaky_relu", 0.01)  # noqa: E731
                framework = (lambda t: theirs(t)) if dtype == torch.float32 else (lambda t: theirs(t.float()).to(dtype))  # noqa: E731

                def autocast(t):   # what the framework does with a bf16 activation under autocast: group_norm is on its fp32 list
                    with torch.autocast("cuda", dtype=torch.bfloat16):
                        return theirs(t)

                def fwd(f):
                    with torch.no_grad():
                        return f(x)

                def xr_():
                    xr_.last = x.detach().requires_grad_(True)
                    return xr_.last

                def fwd_bwd(f, params):
                    xr = x.detach().requires_grad_(True)
                    return torch.autograd.grad(f(xr), [xr, *params], g)

                for mode in ("fwd", "fwd_bwd"):
                    if mode == "fwd":
                        nat, frm = (lambda: fwd(native)), (lambda: fwd(framework))
                    else:
                        nat = lambda: fwd_bwd(native, list(mine.parameters()))  # noqa: E731
                        frm = lambda: fwd_bwd(framework, list(theirs.parameters()))  # noqa: E731
                    variants = {"native": nat, "framework": frm, "native_again": nat}
                    if dtype == torch.bfloat16:
                        variants["framework_autocast"] = (lambda: fwd(autocast)) if mode == "fwd" else \
                            (lambda: torch.autograd.grad(autocast(xr_()), [xr_.last, *theirs.parameters()], g.float()))
                    n0 = _native.launch_count()
                    nat()
                    launches = _native.launch_count() - n0
                    times, iters = alternate(variants, a.rounds, a.window_ms)
                    nbytes = native_bytes(x.numel(), x.element_size(), C // G * V, mode == "fwd_bwd")
                    ms = summary(times)
                    row = {"kind": kind, "B": B, "C": C, "G": G, "spatial": list(S), "span": C // G * V,
                           "dtype": str(dtype).replace("torch.", ""), "mode": mode, "calls_per_round": iters, "native_launches": launches,
                           "ms_per_call": ms, "native_over_framework": ms["native"]["median"] / ms["framework"]["median"],
                           "native_bytes": nbytes, "native_bytes_per_s": nbytes / (ms["native"]["median"] * 1e-3),
                           "framework_note": "fp32" if dtype == torch.float32 else "bf16 input cast to fp32 and back (fp32 parameters)"}
                    if "framework_autocast" in ms:
                        row["native_over_framework_autocast"] = ms["native"]["median"] / ms["framework_autocast"]["median"]
                    row["native_of_copy_rate"] = row["native_bytes_per_s"] / res["copy_bytes_per_s"]
                    print(json.dumps(row), flush=True)
                    res["rows"].append(row)
                del x, g
                torch.cuda.empty_cache()
    if not a.no_network and (not a.only or a.only == "3d"):
        torch.manual_seed(0)
        stem = (ft.Conv3d, {"kernel_size": 3, "padding": 1})
        fused = ft.UNet(4, 3, stem=stem).to(dev)
        plain = ft.UNet(4, 3, stem=stem, norm=(nn.GroupNorm, (8,))).to(dev)
        plain.load_state_dict(fused.state_dict())
        x = torch.rand(2, 4, 128, 128, 128, device=dev)
        gy = torch.rand(2, 3, 128, 128, 128, device=dev)

        def step(m):
            return torch.autograd.grad(m(x), list(m.parameters()), gy)

        variants = {"native": lambda: step(fused), "framework": lambda: step(plain), "native_again": lambda: step(fused)}
        times, iters = alternate(variants, max(3, a.rounds // 2), a.window_ms)
        ms = summary(times)
        res["network"] = {"model": "ft.UNet(4, 3, stem k3), widths 32..512, DoubleConv stages, 2 x 128^3, fp32, forward + backward",
                          "calls_per_round": iters, "ms_per_step": ms,
                          "native_over_framework": ms["native"]["median"] / ms["framework"]["median"]}
        print(json.dumps(res["network"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
