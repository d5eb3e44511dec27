"""Times the fused raw-input training step (rasterizer.rasterize_raw: s360_forward_raw / s360_backward_raw) against the two-step route
(adapter.adapter_tail, then decoder.render_views_fused) at SH degrees 0..4, on bench.py's `adapter_plus_render` shape: 2 context
panoramas of 512 x 1024 (1 048 576 Gaussians), six 256 x 256 faces, fused L2 loss, gradients w.r.t. the raw outputs on persistent
leaves -> profiles/raw_degrees_timing.json.

    timeout -k 10 600 python scripts/raw_degrees_timing.py [--out profiles/raw_degrees_timing.json] [--degrees 0 1 2 3 4]
                                                            [--steps 50] [--collections 3] [--parent parent.json]

Per degree the two paths ALTERNATE in one process: after a warm-up of each, `collections` rounds of (`steps` raw steps, `steps` two-step
steps), each round timed wall-clock between device synchronisations.  Reported per path: every round's ms per step, their median and
their spread (max - min); and whether the raw path is `not_slower`: its median <= the two-step median + the larger of the two spreads
(what lazy.RAW_SEAM_DEGREES lists).  The geometry words, depths and opacities are bench.py's at every degree (the degree-4 records cut
to the first (degree + 1)^2 coefficients per channel), so the tile lists are the same and only the colour work changes.
--degrees 4 runs on a checkout that has the raw path at degree 4 only; --parent merges such a run's degree-4 leg (made with this script
on the parent commit) next to this run's as `parent_commit`."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT)]

from splatter360_amd import _lib, adapter, decoder, rasterizer, synthetic  # noqa: E402

PANO_H, PANO_W, FACE_W, NVC = 512, 1024, 256, 2


def inputs(dev):
    """bench.py's raw cloud (seed 0) and target cameras."""
    gen = torch.Generator().manual_seed(0)
    dep = torch.exp(torch.empty(NVC, PANO_H * PANO_W).uniform_(-0.69, 2.08, generator=gen)).to(dev)
    op = torch.sigmoid(torch.randn(NVC, PANO_H * PANO_W, generator=gen)).to(dev)
    raw = torch.randn(NVC, PANO_H * PANO_W, 82, generator=gen)
    raw[..., 7:] *= 0.6
    cext = torch.eye(4).repeat(NVC, 1, 1)
    cext[0, :3, 3] = torch.tensor([-0.4, 0.0, 0.1])
    cext[1, :3, 3] = torch.tensor([0.4, 0.0, -0.1])
    pose = torch.tensor(synthetic.target_pano_pose((0.0, 0.0, 0.0)), device=dev)
    cams = decoder.cube_cameras(pose, 0.1, 10.0)
    return dep, op, raw.to(dev), cext.to(dev), cams


def cut(raw82, d_sh):
    """[.., 82] degree-4 records -> [.., 7 + 3 d_sh]: the geometry words and the first d_sh coefficients of each channel."""
    sh = raw82[..., 7:].reshape(*raw82.shape[:-1], 3, 25)[..., :d_sh]
    return torch.cat([raw82[..., :7], sh.reshape(*raw82.shape[:-1], 3 * d_sh)], -1).contiguous()


def measure(degree, dep, op, raw82, cext, cams, steps, collections, warmup=5):
    dev = dep.device
    d_sh = (degree + 1) ** 2
    ext, K, near, far = cams
    bg = torch.zeros(3, device=dev)
    gt = torch.full((6, 3, FACE_W, FACE_W), 0.5, device=dev)
    rot = adapter.sh_rotation_blocks(cext, d_sh)
    leaves = [t.detach().clone().requires_grad_(True) for t in (dep, op, cut(raw82, d_sh))]   # persistent leaves, .grad dropped per step

    def step_two():
        for t in leaves:
            t.grad = None
        d, o, r = leaves
        g = adapter.adapter_tail(cext, d, o, r, (PANO_H, PANO_W), 0.5, 15.0, sh_rotation=rot)
        views = decoder.pack_camera_views(ext, K, near, far, bg)
        faces, fm = decoder.render_views_fused(ext, K, near, far, (FACE_W, FACE_W), bg, g.means.reshape(-1, 3), g.covariances.reshape(-1, 3, 3),
                                               g.harmonics.reshape(-1, 3, d_sh), g.opacities.reshape(-1), mse_target=gt, check="lazy",
                                               shared_campos=True, views=views)
        fm.loss.backward()
        return faces

    def step_raw():
        for t in leaves:
            t.grad = None
        d, o, r = leaves
        views = decoder.pack_camera_views(ext, K, near, far, bg)
        faces, _, _, fm = rasterizer.rasterize_raw(d.reshape(-1), o.reshape(-1), r.reshape(-1, 7 + 3 * d_sh), cext, views=views, image_height=FACE_W,
                                                   image_width=FACE_W, context_shape=(PANO_H, PANO_W), scale_min=0.5, scale_max=15.0,
                                                   sh_rotation=rot, mse_target=gt, check="lazy")
        fm.loss.backward()
        return faces

    paths = (("fused_raw", step_raw), ("two_step", step_two))
    finite = {}
    for name, fn in paths:
        for _ in range(warmup):
            f = fn()
        torch.cuda.synchronize(dev)
        finite[name] = bool(torch.isfinite(f).all()) and bool(torch.isfinite(leaves[2].grad).all())
    rounds = {name: [] for name, _ in paths}
    for _ in range(collections):
        for name, fn in paths:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize(dev)
            rounds[name].append((time.perf_counter() - t0) / steps * 1e3)
    out = {"d_sh": d_sh, "raw_record_bytes": 4 * (7 + 3 * d_sh)}
    for name, ms in rounds.items():
        out[name] = {"ms_per_step": ms, "median": statistics.median(ms), "spread": max(ms) - min(ms), "finite": finite[name]}
    spread = max(out["fused_raw"]["spread"], out["two_step"]["spread"])
    out["two_step_over_fused_raw"] = out["two_step"]["median"] / out["fused_raw"]["median"]
    out["not_slower"] = out["fused_raw"]["median"] <= out["two_step"]["median"] + spread
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "raw_degrees_timing.json"))
    ap.add_argument("--degrees", type=int, nargs="+", default=[0, 1, 2, 3, 4])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--collections", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a --degrees 4 result of this script made on the parent commit")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rasterizer.LAZY_SHRINK = True      # as bench.py: check="lazy" calls sized from the largest instance count seen
    ins = inputs(dev)
    res = {"what": __doc__.split("\n\n")[0], "device": torch.cuda.get_device_name(0), "source_hash": _lib.source_hash(), "steps": args.steps,
           "collections": args.collections, "degrees": {}}
    for degree in args.degrees:
        res["degrees"][str(degree)] = measure(degree, *ins, args.steps, args.collections)
        print(degree, json.dumps(res["degrees"][str(degree)]), flush=True)
    if args.parent:
        parent = json.loads(Path(args.parent).read_text())
        res["parent_commit"] = {"source_hash": parent["source_hash"], "degree_4": parent["degrees"]["4"]}
        if "4" in res["degrees"]:
            new, old = res["degrees"]["4"]["fused_raw"], parent["degrees"]["4"]["fused_raw"]
            res["parent_commit"]["degree_4_fused_raw_inside_parent_spread"] = min(old["ms_per_step"]) <= new["median"] <= max(old["ms_per_step"])
            res["parent_commit"]["degree_4_fused_raw_median_ratio_new_over_parent"] = new["median"] / old["median"]
    print(json.dumps(res))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
