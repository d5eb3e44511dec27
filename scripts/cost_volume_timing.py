"""Times the native spherical cost volume (forward + backward) against a plain torch statement of the same closure on the same
GPU, at the hm3d shape (v b = 2, C = 128, D = 128, 128 x 256), and records both peaks of allocated memory and the forward's
accuracy figures against float64 -> profiles/cost_volume_timing.json.

    timeout -k 10 600 python scripts/cost_volume_timing.py [--out profiles/cost_volume_timing.json] [--calls 20]

The torch statement is grid_sample + product + sum + mean in the reference's order (tests/cost_volume_reference.py, float32); the
reference's own function, with its host-side assert on the grid, is not what is timed.  Each figure is the median of `calls`
timed calls (HIP events around one forward + backward) after 3 warm-up calls."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import cost_volume_reference as R  # noqa: E402
from splatter360_amd import _lib, cost_volume as cv  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "cost_volume_timing.json"))
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    dev = "cuda:0"
    b, v, c, d, h, w = 1, 2, 128, 128, 128, 256
    feats, ext, near, far = R.random_inputs(b, v, c, h, w, seed=7, device=dev)
    depths = cv.depth_candidates(near, far, d).float().contiguous()
    poses = cv.relative_poses(ext).contiguous()
    g = torch.randn(v * b, d, h, w, device=dev)

    def native():
        f = feats.detach().requires_grad_(True)
        cv.spherical_cost_volume(f, ext, near, far, d).backward(g)
        return f.grad

    def native_forward():
        with torch.no_grad():
            return cv.spherical_cost_volume(feats, ext, near, far, d)

    def torch_statement():
        f = feats.detach().requires_grad_(True)
        R.cost_volume(f, poses, depths, torch.float32).backward(g)
        return f.grad

    def torch_forward():
        with torch.no_grad():
            return R.cost_volume(feats, poses, depths, torch.float32)

    res = {"shape": {"vb": v * b, "C": c, "D": d, "h": h, "w": w}, "calls": args.calls, "device": torch.cuda.get_device_name(0),
           "source_hash": _lib.source_hash()}
    for key, fn in (("native_fwd_bwd_ms", native), ("torch_fwd_bwd_ms", torch_statement), ("native_fwd_ms", native_forward),
                    ("torch_fwd_ms", torch_forward)):
        ms = timed(fn, args.calls)
        res[key] = {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}
        print(key, res[key], flush=True)
    res["native_peak_bytes"] = peak(native)
    res["torch_peak_bytes"] = peak(torch_statement)
    with torch.no_grad():
        want = R.cost_volume(feats, poses, depths, torch.float64, chunk=8)
        kept = R.well_conditioned(poses, depths, h, w, chunk=8)
        excluded = 1.0 - kept.float().mean().item()
        kept = kept.all(dim=0).view(v * b, d, h, w)
        e_k = (native_forward().double() - want).abs()[kept]
        e_t = (torch_forward().double() - want).abs()[kept]
    res["accuracy"] = {"excluded_share": excluded, "kernel_max": e_k.max().item(), "kernel_mean": e_k.mean().item(),
                       "torch_f32_max": e_t.max().item(), "torch_f32_mean": e_t.mean().item()}
    res["speedup_fwd_bwd"] = res["torch_fwd_bwd_ms"]["median"] / res["native_fwd_bwd_ms"]["median"]
    print(json.dumps(res))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
