"""Device time of ft.NMF on the split-N families with bf16 activation storage (profiles/wide_nmf_bf16.md): the four
rank-family stage matrices of the default-constructed model and the 16 x 262 144 R 1 matrix of the reference's own test,
forward and forward + backward, three ways in one process, alternating:

  bf16      bf16 input, native (this tree)
  composed  bf16 input with the split-N gates off: what a bf16 input did before these families took bf16 (x.float(),
            the composed device path, ~60 framework launches per call)
  fp32      fp32 input, native (the fp32 instances of the same kernels)

and one forward + backward of the default-constructed model under torch.autocast(bfloat16), gates off against on.

  python tools/probes/wide_bf16_timing.py OUT.json            all of the above
  python tools/probes/wide_bf16_timing.py --kernels bf16|fp32  a few calls of every shape and nothing else, to be run
                                                               under a kernel tracer (per-kernel times)"""
import json
import statistics
import sys
import warnings

import torch

sys.path.insert(0, ".")
import factorizer_amd as ft                      # noqa: E402
from factorizer_amd import functional as Fn      # noqa: E402

DEV = "cuda:0"
BF = torch.bfloat16
warnings.simplefilter("ignore", RuntimeWarning)
_gates = (Fn.gnmf_supported, Fn.gnmfx_supported)


def composed(on):
    Fn.gnmf_supported, Fn.gnmfx_supported = ((lambda *a: False), (lambda *a: False)) if on else _gates


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return ts


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4), "n": len(ts)}


def abc(make, modes, reps=5, rounds=4):
    """alternate the modes `rounds` times, `reps` calls each, after a warm-up of each"""
    out = {m: [] for m in modes}
    for m in modes:
        for _ in range(2):
            make(m)
        torch.cuda.synchronize()
    for _ in range(rounds):
        for m in modes:
            out[m] += timed(lambda: make(m), reps)
    return {k: stats(v) for k, v in out.items()}


def shapes():
    rows = []
    for side in (64, 128):
        for i, C in enumerate((64, 128, 256, 512), start=1):
            rows.append((C, (side >> i) ** 3, None, "hals", 2, f"default model {side}^3, stage {i}"))
    rows.append((16, 262144, 1, "mu", 1, "global Matricize test of the reference"))
    return rows


def calls(M, N, R, solver, B):
    torch.manual_seed(M)
    nmf = ft.NMF((M, N), rank=R, solver=solver, init="uniform").to(DEV)
    x32 = torch.rand(B, M, N, device=DEV).to(BF).float()
    g32 = torch.rand(B, M, N, device=DEV).to(BF).float()
    xs = {"fp32": x32.requires_grad_(True), "bf16": x32.detach().to(BF).requires_grad_(True)}
    gs = {"fp32": g32, "bf16": g32.to(BF)}

    def fwd(mode):
        composed(mode == "composed")
        with torch.no_grad():
            nmf(xs["fp32" if mode == "fp32" else "bf16"])
        composed(False)

    def fwd_bwd(mode):
        k = "fp32" if mode == "fp32" else "bf16"
        composed(mode == "composed")
        torch.autograd.grad(nmf(xs[k]), xs[k], gs[k])
        composed(False)

    return nmf, fwd, fwd_bwd


def kernels(mode):
    for M, N, R, solver, B, _ in shapes():
        _, fwd, fwd_bwd = calls(M, N, R, solver, B)
        for _ in range(4):
            fwd(mode)
            fwd_bwd(mode)
        torch.cuda.synchronize()


def main():
    if sys.argv[1] == "--kernels":
        return kernels(sys.argv[2])
    res = {"device": torch.cuda.get_device_name(0), "matrices": []}
    modes = ("bf16", "composed", "fp32")
    for M, N, R, solver, B, what in shapes():
        nmf, fwd, fwd_bwd = calls(M, N, R, solver, B)
        row = {"what": what, "M": M, "N": N, "R": nmf.rank, "B": B, "solver": solver, "fwd": abc(fwd, modes),
               "fwd_bwd": abc(fwd_bwd, modes)}
        nmf._native_solver(torch.empty(B, M, N, device=DEV, dtype=BF))
        row["family"] = nmf._wide
        res["matrices"].append(row)
        print(json.dumps(row), flush=True)
    torch.manual_seed(0)
    model = ft.Factorizer(4, 3, (64, 64, 64)).to(DEV)
    x = torch.rand(1, 4, 64, 64, 64, device=DEV)

    def step(mode):
        composed(mode == "composed")
        for p in model.parameters():
            p.grad = None
        with torch.autocast("cuda", dtype=BF):
            y = model(x)
        y.float().square().mean().backward()
        composed(False)

    res["model_64_autocast"] = abc(step, ("composed", "bf16"), reps=3, rounds=3)
    print(json.dumps(res["model_64_autocast"]), flush=True)
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
