"""Device time of ft.NMF on the per-stage matrices of the default-constructed model (rank=None), native split-N
families against the composed path on the same device, alternating; and of one training step (forward + backward) of
the default-constructed model.  `python tools/probes/wide_rank_timing.py OUT.json [side]` (profiles/wide_nmf_rank.md)."""
import json
import statistics
import sys
import warnings

import torch

sys.path.insert(0, ".")
import factorizer_amd as ft                      # noqa: E402
from factorizer_amd import functional as Fn      # noqa: E402

DEV = "cuda:0"
warnings.simplefilter("ignore", RuntimeWarning)
_native_gate = Fn.gnmfx_supported


def composed(on):
    """route what csrc/nmf_global_rank.hip covers to the composed path, as before that family existed"""
    Fn.gnmfx_supported = (lambda *a: False) if on else _native_gate


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


def ab(make, reps=5, rounds=4):
    """alternate composed / native `rounds` times, `reps` calls each, after a warm-up of both"""
    out = {"composed": [], "native": []}
    for mode in ("composed", "native"):
        composed(mode == "composed")
        for _ in range(2):
            make()
        torch.cuda.synchronize()
    for _ in range(rounds):
        for mode in ("composed", "native"):
            composed(mode == "composed")
            out[mode] += timed(make, reps)
    composed(False)
    return {k: stats(v) for k, v in out.items()}


def main():
    path = sys.argv[1]
    side = int(sys.argv[2]) if len(sys.argv) > 2 else 128
    res = {"device": torch.cuda.get_device_name(0), "stages": [], "side": side}
    B = 2
    for i, C in enumerate((32, 64, 128, 256, 512)):
        N = (side >> i) ** 3
        for solver in ("hals", "mu"):
            torch.manual_seed(i)
            nmf = ft.NMF((C, N), rank=None, solver=solver).to(DEV)
            x = torch.rand(B, C, N, device=DEV).relu_().requires_grad_(True)
            gy = torch.rand(B, C, N, device=DEV)

            def fwd():
                with torch.no_grad():
                    nmf(x)

            def fwd_bwd():
                torch.autograd.grad(nmf(x), x, gy)

            row = {"M": C, "N": N, "R": nmf.rank, "B": B, "solver": solver, "fwd": ab(fwd), "fwd_bwd": ab(fwd_bwd)}
            nmf._native_solver(x)
            row["family"] = nmf._wide
            res["stages"].append(row)
            print(json.dumps(row), flush=True)
            del nmf, x, gy
            torch.cuda.empty_cache()
    torch.manual_seed(0)
    model = ft.Factorizer(4, 3, (64, 64, 64)).to(DEV)
    x = torch.rand(1, 4, 64, 64, 64, device=DEV)
    params = list(model.parameters())

    def step():
        y = model(x)
        torch.autograd.grad(y.square().mean(), params)

    res["model_64_step"] = ab(step, reps=3, rounds=3)
    print(json.dumps(res["model_64_step"]), flush=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
