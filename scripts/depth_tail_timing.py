"""Times the native fine-depth and opacity tail — fullres_maps (two kernels, two backward) and fine_depth_tail (one kernel, one
backward), forward and forward + backward — against the plain torch statement of the same reference lines
(tests/depth_tail_reference.py, float32) on the same GPU, at the hm3d shape (v b = 2, coarse 128 x 256, s = 4: a 512 x 1024 ERP)
and at coarse 64 x 128 (a 256 x 512 ERP), and records both peaks of allocated memory and the accuracy figures of
tests/test_gpu_depth_tail.py's rule against float64 -> profiles/depth_tail_timing.json.

    timeout -k 10 600 python scripts/depth_tail_timing.py [--out profiles/depth_tail_timing.json] [--calls 200]

Each figure is the median of `calls` timed calls (HIP events around one call) after 10 warm-up calls, all in one process."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import depth_tail_reference as R  # noqa: E402
from splatter360_amd import _lib, depth_tail as dt  # noqa: E402

SHAPES = {"hm3d": (1, 2, 128, 256, 4), "erp_256x512": (1, 2, 64, 128, 4)}       # (b, v, h, w, s)
EXPONENT = 4.0


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


def errors(got, want, t32, keep=None):
    e_k, e_t, ref = (got.double() - want).abs(), (t32.double() - want).abs(), want.abs()
    if keep is not None:
        e_k, e_t, ref = e_k[keep], e_t[keep], ref[keep]
    return {"kernel": {"max": e_k.max().item(), "mean": e_k.mean().item()}, "torch_f32": {"max": e_t.max().item(), "mean": e_t.mean().item()},
            "floor": 2.0 ** -24 * ref.max().item()}


def legs(native, statement, inputs, grads):
    """The four callables of one stretch: forward alone (no_grad) and forward + backward, native and torch."""
    def run(fn, backward):
        def call():
            if not backward:
                with torch.no_grad():
                    return fn(*inputs)
            leaves = [t.detach().requires_grad_(True) for t in inputs]
            torch.autograd.backward(fn(*leaves), grads)
            return [t.grad for t in leaves]
        return call
    return {"native_fwd_ms": run(native, False), "torch_fwd_ms": run(statement, False), "native_fwd_bwd_ms": run(native, True),
            "torch_fwd_bwd_ms": run(statement, True)}


def measure_stretch(res, calls, fns):
    for key, fn in fns.items():
        res[key] = timed(fn, calls)
        print(key, res[key], flush=True)
    res["native_peak_bytes"], res["torch_peak_bytes"] = peak(fns["native_fwd_bwd_ms"]), peak(fns["torch_fwd_bwd_ms"])
    res["speedup_fwd"] = res["torch_fwd_ms"]["median"] / res["native_fwd_ms"]["median"]
    res["speedup_fwd_bwd"] = res["torch_fwd_bwd_ms"]["median"] / res["native_fwd_bwd_ms"]["median"]


def measure(shape, calls):
    b, v, h, w, s = shape
    dev = "cuda:0"
    depth, pmax, g_disps, g_pmax = R.random_maps(b * v, h, w, s, seed=7, device=dev)
    fullres, dd, near, far, *grads = R.random_case(b, v, h * s, w * s, 1, seed=8, device=dev)
    out = {"shape": {"b": b, "v": v, "h": h, "w": w, "s": s, "gpp": 1}, "exponent": EXPONENT}

    maps = {"map_bytes": fullres.numel() * 4}
    fns = legs(lambda d, p: dt.fullres_maps(d, p, s), lambda d, p: R.fullres_maps(d, p, s, torch.float32), (depth, pmax), [g_disps, g_pmax])
    measure_stretch(maps, calls, fns)
    with torch.no_grad():
        want, got, t32 = R.fullres_maps(depth, pmax, s), fns["native_fwd_ms"](), fns["torch_fwd_ms"]()
    acc = {"fullres_disps": errors(got[0], want[0], t32[0]), "pdf_max": errors(got[1], want[1], t32[1])}
    d64 = depth.double().requires_grad_(True)
    want_g = torch.autograd.grad(R.fullres_maps(d64, pmax, s)[0], d64, g_disps.double())[0]
    acc["g_coarse_depths"] = errors(fns["native_fwd_bwd_ms"]()[0], want_g, fns["torch_fwd_bwd_ms"]()[0])
    maps["accuracy"] = acc
    out["fullres_maps"] = maps

    tail = {"map_bytes": fullres.numel() * 4}
    fns = legs(lambda f, d: dt.fine_depth_tail(f, d, near, far, views=v, exponent=EXPONENT, return_densities=True),
               lambda f, d: R.tail(f, d, near, far, 1, EXPONENT, torch.float32), (fullres, dd), grads)
    measure_stretch(tail, calls, fns)
    with torch.no_grad():
        want, got, t32 = R.tail(fullres, dd, near, far, 1, EXPONENT), fns["native_fwd_ms"](), fns["torch_fwd_ms"]()
        keep = (R.clamp_pass(*R.tail_planes(fullres, dd, near, far, 1, EXPONENT, torch.float64)[3:])
                == R.clamp_pass(*R.tail_planes(fullres, dd, near, far, 1, EXPONENT, torch.float32)[3:]))
    acc = {name: errors(got[i], want[i], t32[i]) for i, name in enumerate(("depths", "opacities", "densities"))}
    want_g = R.tail_gradient(fullres, dd, near, far, 1, EXPONENT, grads)
    got_g, t32_g = fns["native_fwd_bwd_ms"](), fns["torch_fwd_bwd_ms"]()
    acc["clamp_decisions_that_differ"] = {"count": (~keep).sum().item(), "of": keep.numel()}
    acc["g_fullres_disps"] = errors(got_g[0], want_g[0], t32_g[0], keep)
    acc["g_delta_disparity"] = errors(got_g[1][:, :1], want_g[1][:, :1], t32_g[1][:, :1], keep)
    acc["g_delta_density"] = errors(got_g[1][:, 1:], want_g[1][:, 1:], t32_g[1][:, 1:])
    tail["accuracy"] = acc
    out["fine_depth_tail"] = tail
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "depth_tail_timing.json"))
    ap.add_argument("--calls", type=int, default=200)
    args = ap.parse_args()
    res = {"calls": args.calls, "device": torch.cuda.get_device_name(0), "source_hash": _lib.source_hash(),
           "shapes": {name: measure(shape, args.calls) for name, shape in SHAPES.items()}}
    print(json.dumps(res))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
