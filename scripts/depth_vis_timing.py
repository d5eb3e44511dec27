"""Times the evaluation step's pictures at the evaluation shapes, per call with launch overhead included, against a plain torch
statement of the same lines that runs on the device -> profiles/depth_vis_timing.json:

  depth_map_faces   depth_map on 18 x 256 x 256 (v = 3 views x 6 rendered depth faces), one call, uint8 [18, 256, 256, 3] out
  depth_map_erp     depth_map on 3 x 512 x 1024 (the stitched depth panoramas), one call, uint8 out
  prep_image        prep_image on 18 x 3 x 256 x 256 -> uint8 [256, 18 * 256, 3]

  native   splatter360_amd.visualize
  torch    a plain torch statement written for this project — NOT the reference's function: per map the boolean selection and two
           torch.quantile, log, normalise, then clip, * 256, floor, clamp and a gather from the turbo table kept on the device, * 255,
           cast, permute (depth_map); clip, * 255, cast, permute (prep_image).  The reference copies every map to the host for
           matplotlib and back, and the frame to the host again; that round trip is removed too and is not what is measured here.

    timeout -k 10 900 python scripts/depth_vis_timing.py [--out profiles/depth_vis_timing.json] [--calls 100]

Each figure is the median of `calls` timed calls (HIP events around one call) after 10 warm-up calls, the legs alternating call by
call in one process.  The figures are reported, not asserted; the native bytes are compared with the torch statement's before
anything is timed (share of pixels that differ: the statement chains float32 operations, the kernels round once)."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import depth_vis_reference as R  # noqa: E402
from splatter360_amd import _lib, visualize  # noqa: E402

SHAPES = {"depth_map_faces": (18, 256, 256), "depth_map_erp": (3, 512, 1024), "prep_image": (18, 3, 256, 256)}


def torch_depth_map(depth, table):
    """uint8 [n, h, w, 3]: the reference's lines per map, on the device."""
    out = []
    for d in depth:
        near = d[d > 0].quantile(0.01).log()
        far = d.view(-1).quantile(0.99).log()
        x = 1 - (d.log() - near) / (far - near)
        idx = (x.clip(min=0, max=1) * 256).floor().clamp(max=255).long()
        idx = torch.where(torch.isnan(x), torch.full_like(idx, 256), idx)
        out.append((table[idx].clip(min=0, max=1) * 255).type(torch.uint8))
    return torch.stack(out)


def torch_prep_image(image):
    b, c, h, w = image.shape
    image = image.permute(1, 2, 0, 3).reshape(c, h, b * w)
    return (image.clip(min=0, max=1) * 255).type(torch.uint8).permute(1, 2, 0).contiguous()


def timed(fns, calls, warmup=10):
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(calls):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "depth_vis_timing.json"))
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--native-only", action="store_true", help="run the native legs alone (for a kernel trace)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(7)
    table = torch.from_numpy(R.tables("turbo")[0]).to(dev)

    def depths(shape):
        d = torch.exp(torch.rand(shape, device=dev, generator=gen) * (np.log(12.0) - np.log(0.3)) + np.log(0.3))
        d[torch.rand(shape, device=dev, generator=gen) < 0.02] = 0.0
        return d

    faces, erp = depths(SHAPES["depth_map_faces"]), depths(SHAPES["depth_map_erp"])
    frames = torch.rand(SHAPES["prep_image"], device=dev, generator=gen) * 1.2 - 0.1
    legs = {"depth_map_faces": (lambda: visualize.depth_map(faces, out="uint8"), lambda: torch_depth_map(faces, table)),
            "depth_map_erp": (lambda: visualize.depth_map(erp, out="uint8"), lambda: torch_depth_map(erp, table)),
            "prep_image": (lambda: visualize.prep_image(frames), lambda: torch_prep_image(frames))}
    if args.native_only:
        for _ in range(args.calls):
            for native, _ in legs.values():
                native()
        torch.cuda.synchronize()
        return
    res = {"calls": args.calls, "device": torch.cuda.get_device_name(0), "source_hash": _lib.source_hash(),
           "shapes": {k: list(v) for k, v in SHAPES.items()},
           "torch_leg": "a plain torch statement of the same lines on the device, written for this project; not the reference's function"}
    for k, (native, plain) in legs.items():
        a, b = native(), plain()
        assert a.shape == b.shape and a.dtype == b.dtype == torch.uint8
        res[f"{k}_share_of_pixels_that_differ_from_torch"] = float((a != b).any(-1).float().mean())
        t = timed({"native": native, "torch": plain}, args.calls)
        res[f"{k}_native_ms"], res[f"{k}_torch_ms"] = t["native"], t["torch"]
        res[f"{k}_speedup_vs_torch"] = t["torch"]["median"] / t["native"]["median"]
    print(json.dumps(res))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
