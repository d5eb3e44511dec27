"""Times the native depth-smoothness loss (splatter360_amd.depth_smooth: two kernels forward, one backward) — forward alone and
forward + backward, launch overhead included — against the plain torch statement of the same reference lines
(tests/depth_smooth_reference.torch_statement, float32) on the same GPU, in the four modes (first / second derivative, with /
without the bilateral weight at sigma_image = 2.0), at the training step's shape (1, 6, 256, 256), the evaluation step's
(1, 18, 256, 256) and at (1, 6, 512, 512); records both peaks of allocated memory and, per mode, the distance of the kernels
and of torch's float32 chain from the float64 statement in units of A -> profiles/depth_smooth_timing.json.

    timeout -k 10 900 python scripts/depth_smooth_timing.py [--out profiles/depth_smooth_timing.json] [--calls 200]

Each figure is the median of `calls` timed calls (HIP events around one call) after 10 warm-up calls, all in one process."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import depth_smooth_reference as R  # noqa: E402
from splatter360_amd import _lib, depth_smooth as ds  # noqa: E402

SHAPES = {"train_1x6x256x256": (1, 6, 256, 256), "eval_1x18x256x256": (1, 18, 256, 256), "faces_1x6x512x512": (1, 6, 512, 512)}
DEV = "cuda:0"


def timed(fn, calls, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def legs(native, statement, depth):
    """The four callables of one mode: forward alone (no_grad) and forward + backward, native and torch."""
    def run(fn, backward):
        def call():
            if not backward:
                with torch.no_grad():
                    return fn(depth)
            leaf = depth.detach().requires_grad_(True)
            fn(leaf).backward()
            return leaf.grad
        return call
    return {"native_fwd_ms": run(native, False), "torch_fwd_ms": run(statement, False), "native_fwd_bwd_ms": run(native, True),
            "torch_fwd_bwd_ms": run(statement, True)}


def in_units_of_a(got, want64, a):
    err = np.abs(got.double().cpu().numpy() - want64)
    ok = a > 0
    return {"max": float((err[ok] / a[ok]).max()), "mean": float((err[ok] / a[ok]).mean()), "nonzero_where_A_is_0": int((err[~ok] != 0).sum())}


def measure(shape, calls):
    c = R.make_case(shape, 1, seed=9, device=DEV)
    depth, near, far, image = (torch.from_numpy(c[k]).to(DEV) for k in ("depth", "near", "far", "image"))
    ln, lf = R.torch_log(c["near"], DEV), R.torch_log(c["far"], DEV)
    out = {"shape": list(shape), "depth_bytes": depth.numel() * 4, "image_bytes": image.numel() * 4}
    for name, second, sigma in R.MODES:
        fns = legs(lambda d: ds.depth_smoothness_loss(d, near, far, image, sigma_image=sigma, use_second_derivative=second),
                   lambda d: R.torch_statement(d, near, far, image, sigma, second), depth)
        res = {}
        for key, fn in fns.items():
            res[key] = timed(fn, calls)
            print(name, key, res[key], flush=True)
        res["native_peak_bytes"], res["torch_peak_bytes"] = peak(fns["native_fwd_bwd_ms"]), peak(fns["torch_fwd_bwd_ms"])
        res["speedup_fwd"] = res["torch_fwd_ms"]["median"] / res["native_fwd_ms"]["median"]
        res["speedup_fwd_bwd"] = res["torch_fwd_bwd_ms"]["median"] / res["native_fwd_bwd_ms"]["median"]
        want = R.statement(c["depth"], ln, lf, c["image"], sigma, second)
        w64 = float(want["loss64"])
        res["accuracy"] = {
            "loss_relative": {"kernel": abs(fns["native_fwd_ms"]().item() - w64) / abs(w64), "torch_f32": abs(fns["torch_fwd_ms"]().item() - w64) / abs(w64)},
            "grad_in_units_of_A": {"kernel": in_units_of_a(fns["native_fwd_bwd_ms"](), want["grad64"], want["A"]),
                                   "torch_f32": in_units_of_a(fns["torch_fwd_bwd_ms"](), want["grad64"], want["A"]), "bar": 2.0 ** -23},
        }
        out[name] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "depth_smooth_timing.json"))
    ap.add_argument("--calls", type=int, default=200)
    args = ap.parse_args()
    res = {"calls": args.calls, "device": torch.cuda.get_device_name(0), "source_hash": _lib.source_hash(), "sigma_image": 2.0,
           "shapes": {name: measure(shape, args.calls) for name, shape in SHAPES.items()}}
    print(json.dumps(res))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
