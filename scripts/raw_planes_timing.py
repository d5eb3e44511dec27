"""Times the fused raw-input training step from the encoder's last convolution output [(v b), C, h, w] — channel planes, C = 2 + 7 + 3 d_sh
with the two offset_xy channels in front — through the reference's own view chain, on the record route (the chain's view transposed into
records by reshape, gradients back through autograd's reshape / slice / permute nodes) and on the plane route
(rasterize_raw(raw_layout="planes"): read and differentiated where it lies), against the floor of ready-made contiguous records, at SH
degrees 0..4 on bench.py's `adapter_plus_render` shape: 2 context panoramas of 512 x 1024 (1 048 576 Gaussians), six 256 x 256 faces,
fused L2 loss -> profiles/raw_planes_timing.json.

    timeout -k 10 600 python scripts/raw_planes_timing.py [--out profiles/raw_planes_timing.json] [--degrees 0 1 2 3 4] [--steps 50]
                                                           [--collections 3] [--legs A B C]

Legs, ALTERNATED in one process per degree (after a warm-up of each, `collections` rounds of every leg in turn; each round timed
wall-clock between device synchronisations, `steps` forwards and then `steps` forward + backward steps):
  A_records_from_planes  NCHW leaf -> "(v b) c h w -> b v (h w) c", "... (srf c) -> ... srf c", [..., 2:] -> raw[0].reshape(-1, 7 + 3 d_sh)
                         -> rasterize_raw (records) -> loss.backward() -> .grad on the leaf: what DecoderSplattingFused did before the
                         plane route existed;
  B_planes               the same leaf -> rasterize_raw(raw_layout="planes", raw_channel_offset=2) -> .grad on the leaf;
  C_records_floor        a persistent contiguous [P, 7 + 3 d_sh] leaf -> rasterize_raw (records) -> .grad as records: the figure
                         scripts/raw_degrees_timing.py quotes, the floor.
Reported per leg: every round's ms per forward and per step, their medians and spreads (max - min), the peak allocated memory of a
round; per degree `planes_not_slower`: B's step median <= A's + the larger of the two spreads — what lazy.RAW_PLANE_SEAM_DEGREES lists.
Kernel against kernel (k_raw_eval / k_raw_bwd, plane against record) is a run of its own under a kernel trace:
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/raw_planes_timing.py --degrees 4 --legs B C --collections 1 --out <scratch>.json"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch
from einops import rearrange

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT)]

from splatter360_amd import _lib, adapter, decoder, lazy, rasterizer  # noqa: E402
from raw_degrees_timing import FACE_W, NVC, PANO_H, PANO_W, cut, inputs  # noqa: E402

OFFSET = 2      # the reference's offset_xy channels


def planes_of(records, h, w):
    """[v, h w, width] records -> [v, OFFSET + width, h, w] channel planes (offset channels: noise, never read)"""
    v, _, width = records.shape
    out = torch.randn(v, OFFSET + width, h, w, device=records.device)
    out[:, OFFSET:] = records.permute(0, 2, 1).reshape(v, width, h, w)
    return out


def measure(degree, dep, op, raw82, cext, cams, steps, collections, legs, warmup=5):
    dev = dep.device
    d_sh = (degree + 1) ** 2
    width = 7 + 3 * d_sh
    ext, K, near, far = cams
    bg = torch.zeros(3, device=dev)
    gt = torch.full((6, 3, FACE_W, FACE_W), 0.5, device=dev)
    rot = adapter.sh_rotation_blocks(cext, d_sh)
    records = cut(raw82, d_sh)
    d_leaf, o_leaf = (t.detach().clone().requires_grad_(True) for t in (dep, op))
    rec_leaf = records.detach().clone().requires_grad_(True)
    conv = planes_of(records, PANO_H, PANO_W).requires_grad_(True)          # the last convolution's output, "(v b)" with b = 1
    kw = dict(image_height=FACE_W, image_width=FACE_W, context_shape=(PANO_H, PANO_W), scale_min=0.5, scale_max=15.0, sh_rotation=rot, mse_target=gt,
              check="lazy")

    def chain():
        x = rearrange(conv, "(v b) c h w -> b v (h w) c", v=NVC, b=1)
        x = rearrange(x, "... (srf c) -> ... srf c", srf=1)
        return rearrange(x[..., OFFSET:], "b v r srf c -> b v r srf () c")
    found = lazy.raw_planes_of(chain())
    assert found is not None and found.base is conv and found.channel_offset == OFFSET

    def render(raw, **layout):
        views = decoder.pack_camera_views(ext, K, near, far, bg)
        return rasterizer.rasterize_raw(d_leaf.reshape(-1), o_leaf.reshape(-1), raw, cext, views=views, **kw, **layout)

    def leg_a():
        return render(chain()[0].reshape(-1, width)), conv

    def leg_b():
        p = lazy.raw_planes_of(chain())
        return render(p.element(0, 1), raw_layout="planes", raw_channel_offset=p.channel_offset), conv

    def leg_c():
        return render(rec_leaf.reshape(-1, width)), rec_leaf

    def run(fn, backward):
        for t in (d_leaf, o_leaf, rec_leaf, conv):
            t.grad = None
        (faces, _, _, fm), leaf = fn()
        if backward:
            fm.loss.backward()
        return faces, leaf

    table = {"A_records_from_planes": leg_a, "B_planes": leg_b, "C_records_floor": leg_c}
    paths = [(n, f) for n, f in table.items() if n[0] in legs]
    finite, grads = {}, {}
    for name, fn in paths:
        for _ in range(warmup):
            faces, leaf = run(fn, True)
        torch.cuda.synchronize(dev)
        finite[name] = bool(torch.isfinite(faces).all()) and bool(torch.isfinite(leaf.grad).all())
        grads[name] = (faces.detach().clone(), leaf.grad.detach().clone())
    same = None
    if "A_records_from_planes" in grads and "B_planes" in grads:        # one computation, two routes: the same bits
        (fa, ga), (fb, gb) = grads["A_records_from_planes"], grads["B_planes"]
        same = bool(torch.equal(fa, fb)) and bool(torch.equal(ga, gb)) and bool((gb[:, :OFFSET] == 0).all())
    grads.clear()
    rounds = {name: {"fwd": [], "step": [], "peak": []} for name, _ in paths}
    for _ in range(collections):
        for name, fn in paths:
            torch.cuda.synchronize(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            for key, backward in (("fwd", False), ("step", True)):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _ in range(steps):
                    run(fn, backward)
                torch.cuda.synchronize(dev)
                rounds[name][key].append((time.perf_counter() - t0) / steps * 1e3)
            rounds[name]["peak"].append(torch.cuda.max_memory_allocated(dev))
    out = {"d_sh": d_sh, "channels": OFFSET + width, "plane_tensor_bytes": 4 * NVC * (OFFSET + width) * PANO_H * PANO_W, "planes_equal_records_bits": same}
    for name, r in rounds.items():
        out[name] = {"forward_ms": r["fwd"], "forward_median": statistics.median(r["fwd"]), "forward_spread": max(r["fwd"]) - min(r["fwd"]),
                     "step_ms": r["step"], "step_median": statistics.median(r["step"]), "step_spread": max(r["step"]) - min(r["step"]),
                     "peak_allocated_bytes": max(r["peak"]), "finite": finite[name]}
    if "A_records_from_planes" in out and "B_planes" in out:
        a, b = out["A_records_from_planes"], out["B_planes"]
        out["A_over_B_step"] = a["step_median"] / b["step_median"]
        out["planes_not_slower"] = b["step_median"] <= a["step_median"] + max(a["step_spread"], b["step_spread"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "raw_planes_timing.json"))
    ap.add_argument("--degrees", type=int, nargs="+", default=[0, 1, 2, 3, 4])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--collections", type=int, default=3)
    ap.add_argument("--legs", nargs="+", default=["A", "B", "C"])
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rasterizer.LAZY_SHRINK = True      # as bench.py: check="lazy" calls sized from the largest instance count seen
    ins = inputs(dev)
    res = {"what": __doc__.split("\n\n")[0], "device": torch.cuda.get_device_name(0), "source_hash": _lib.source_hash(), "steps": args.steps,
           "collections": args.collections, "degrees": {}}
    for degree in args.degrees:
        res["degrees"][str(degree)] = measure(degree, *ins, args.steps, args.collections, args.legs)
        print(degree, json.dumps(res["degrees"][str(degree)]), flush=True)
    res["seam_plane_degrees"] = list(lazy.RAW_PLANE_SEAM_DEGREES)
    print(json.dumps(res))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
