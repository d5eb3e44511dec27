"""Times the native softmax depth head (forward, and forward + backward) against the plain torch statement of the same three
lines (tests/depth_head_reference.py, float32) on the same GPU, at the hm3d shape (v b = 2, D = 128, 128 x 256) and at the
encoder config's default D = 32, and records both peaks of allocated memory and the accuracy figures of
tests/test_gpu_depth_head.py's rule against float64 -> profiles/depth_head_timing.json.

    timeout -k 10 600 python scripts/depth_head_timing.py [--out profiles/depth_head_timing.json] [--calls 20]

Each figure is the median of `calls` timed calls (HIP events around one call) after 3 warm-up calls, all in one process."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import depth_head_reference as R  # noqa: E402
from splatter360_amd import _lib, depth_head as dh  # noqa: E402

SHAPES = {"hm3d": (2, 128, 128, 256), "default_d32": (2, 32, 128, 256)}


def timed(fn, calls, warmup=3):
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
    return ms


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def errors(got, want):
    e = (got.double() - want).abs()
    return {"max": e.max().item(), "mean": e.mean().item()}


def measure(shape, calls, scale=1.0):
    logits, cand, g_depth, g_pmax = R.random_case(shape, scale, "inverse_depth", seed=7, device="cuda:0")

    def native():
        z = logits.detach().requires_grad_(True)
        torch.autograd.backward(dh.softmax_depth_head(z, cand), [g_depth, g_pmax])
        return z.grad

    def native_forward():
        with torch.no_grad():
            return dh.softmax_depth_head(logits, cand)

    def torch_statement():
        z = logits.detach().requires_grad_(True)
        torch.autograd.backward(R.head(z, cand, torch.float32), [g_depth, g_pmax])
        return z.grad

    def torch_forward():
        with torch.no_grad():
            return R.head(logits, cand, torch.float32)

    n, d, h, w = shape
    res = {"shape": {"n": n, "D": d, "h": h, "w": w}, "logits_bytes": logits.numel() * 4}
    for key, fn in (("native_fwd_ms", native_forward), ("torch_fwd_ms", torch_forward), ("native_fwd_bwd_ms", native),
                    ("torch_fwd_bwd_ms", torch_statement)):
        ms = timed(fn, calls)
        res[key] = {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}
        print(shape, key, res[key], flush=True)
    res["native_peak_bytes"] = peak(native)
    res["torch_peak_bytes"] = peak(torch_statement)
    res["speedup_fwd"] = res["torch_fwd_ms"]["median"] / res["native_fwd_ms"]["median"]
    res["speedup_fwd_bwd"] = res["torch_fwd_bwd_ms"]["median"] / res["native_fwd_bwd_ms"]["median"]
    with torch.no_grad():
        want, got, t32 = R.head(logits, cand, torch.float64), native_forward(), torch_forward()
    acc = {"logits_scale": scale}
    for i, name in enumerate(("depth", "pdf_max")):
        acc[name] = {"kernel": errors(got[i], want[i]), "torch_f32": errors(t32[i], want[i]), "floor": 2.0 ** -24 * want[i].abs().max().item()}
    want_g = R.logits_gradient(logits, cand, g_depth, g_pmax, torch.float64)
    acc["g_logits"] = {"kernel": errors(native(), want_g), "torch_f32": errors(torch_statement(), want_g),
                       "floor": 2.0 ** -24 * want_g.abs().max().item()}
    res["accuracy"] = acc
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "depth_head_timing.json"))
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    res = {"calls": args.calls, "device": torch.cuda.get_device_name(0), "source_hash": _lib.source_hash(),
           "shapes": {name: measure(shape, args.calls) for name, shape in SHAPES.items()}}
    res["accuracy"] = res["shapes"]["hm3d"]["accuracy"]
    res["accuracy_one_hot"] = measure(SHAPES["hm3d"], 3, scale=30.0)["accuracy"]
    print(json.dumps(res))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
