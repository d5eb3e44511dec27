"""Times the depth-faces -> ERP distance panorama at the evaluation shape (N = 3 target views, 256 x 256 faces, ERP 512 x 1024),
forward and forward + backward, three ways on the same GPU -> profiles/erp_distance_timing.json:

  fused      Cube2Equirec.stitch_distance_rendered: one kernel (one more for the backward)
  two_step   the native pieces one after the other: depth_to_distance on the reordered faces, then Cube2Equirec.forward (one stitch
             launch per panorama), with the reorder as torch flips and index copies
  torch      a plain float32 torch statement of the three steps written for this project: the reorder, sqrt(X^2 + Y^2 + d^2) with
             u = the row index, and the stitch as eight precomputed index gathers (tests/stitch_reference.py's taps) and a weighted sum

    timeout -k 10 600 python scripts/erp_distance_timing.py [--out profiles/erp_distance_timing.json] [--calls 200]

Each figure is the median of `calls` timed calls (HIP events around one call, launch overhead included) after 10 warm-up calls, the
legs alternating call by call in one process.  The figures are reported, not asserted; the fused call's bits are checked against the
two-step's at this shape before anything is timed."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import stitch_reference as SR  # noqa: E402
from splatter360_amd import _lib, stitch  # noqa: E402

SHAPE = {"n": 3, "face_w": 256, "equ_h": 512, "equ_w": 1024}
CONVENTION = "reference"


def reorder(d):
    """change_order_batch without the in-place write."""
    return torch.stack([d[:, c & 7].flip(-1, -2) if c & 8 else d[:, c & 7] for c in stitch.CHANGE_ORDER_FACE_MAP], 1)


class TorchStatement:
    """The three steps in plain float32 torch.  A tap outside the volume has weight 0 here (finite inputs only)."""

    def __init__(self, fw, eh, ew, dev):
        tex, w, valid = SR.taps(stitch.sample_grid_numpy(fw, eh, ew), fw)
        self.eh, self.ew = eh, ew
        self.tex = [torch.from_numpy(np.where(valid[:, k], tex[:, k], 0)).to(dev) for k in range(8)]
        self.wgt = [torch.from_numpy(np.where(valid[:, k], w[:, k], 0).astype(np.float32)).to(dev) for k in range(8)]
        self.row = torch.arange(fw, device=dev, dtype=torch.float32)[:, None]
        self.col = torch.arange(fw, device=dev, dtype=torch.float32)[None, :]

    def __call__(self, depth, k4):
        n = depth.shape[0]
        d = reorder(depth)
        fx, fy, cx, cy = (k4[..., i, None, None] for i in range(4))
        x = (self.row - cx) * d / fx
        y = (self.col - cy) * d / fy
        flat = torch.sqrt(x ** 2 + y ** 2 + d ** 2).reshape(n, -1)
        return sum(flat[:, t] * wk for t, wk in zip(self.tex, self.wgt)).reshape(n, self.eh, self.ew)


def timed(fns, calls, warmup=10):
    """Medians of the callables of `fns` (a dict), alternating them call by call."""
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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "erp_distance_timing.json"))
    ap.add_argument("--calls", type=int, default=200)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    n, fw, eh, ew = (SHAPE[k] for k in ("n", "face_w", "equ_h", "equ_w"))
    mod = stitch.Cube2Equirec(fw, eh, ew).to(dev)
    statement = TorchStatement(fw, eh, ew, dev)
    gen = torch.Generator(device=dev).manual_seed(3)
    depth = torch.rand(n, 6, fw, fw, device=dev, generator=gen) * 9.5 + 0.5
    intr = torch.tensor([0.5, 0.5, 0.5, 0.5], device=dev) + (torch.rand(n, 6, 4, device=dev, generator=gen) - 0.5) * 0.05
    k4 = (intr * fw).contiguous()
    g = torch.randn(n, eh, ew, device=dev, generator=gen)

    def fused(d):
        return mod.stitch_distance_rendered(d, k4, CONVENTION)

    def two_step(d):
        dist = stitch.depth_to_distance(reorder(d), k4.reshape(n * 6, 4), CONVENTION)
        return mod(dist.permute(0, 2, 1, 3).reshape(n, 1, fw, 6 * fw))[:, 0]

    def torch_f32(d):
        return statement(d, k4)

    legs = {"fused": fused, "two_step": two_step, "torch": torch_f32}

    def fwd(fn):
        def call():
            with torch.no_grad():
                return fn(depth)
        return call

    def fwd_bwd(fn):
        def call():
            leaf = depth.detach().requires_grad_(True)
            return torch.autograd.grad(fn(leaf), leaf, g)[0]
        return call

    # the fused call is the two-step, bit for bit, at the timed shape; the torch statement is the same function to float32 rounding
    out = {k: fwd(fn)() for k, fn in legs.items()}
    grad = {k: fwd_bwd(fn)() for k, fn in legs.items()}
    assert torch.equal(out["fused"], out["two_step"]) and torch.equal(grad["fused"], grad["two_step"])
    res = {"calls": args.calls, "device": torch.cuda.get_device_name(0), "source_hash": _lib.source_hash(), "shape": SHAPE,
           "convention": CONVENTION, "fused_equals_two_step": True,
           "torch_vs_fused_max_abs": {"forward": float((out["torch"] - out["fused"]).abs().max()),
                                      "backward": float((grad["torch"] - grad["fused"]).abs().max())},
           "bytes_moved_fwd": 4 * (n * 6 * fw * fw + n * eh * ew + 3 * eh * ew)}
    t = timed({f"{k}_fwd_ms": fwd(fn) for k, fn in legs.items()}, args.calls)
    t.update(timed({f"{k}_fwd_bwd_ms": fwd_bwd(fn) for k, fn in legs.items()}, args.calls))
    res.update(t)
    for what in ("fwd", "fwd_bwd"):
        res[f"speedup_{what}_vs_two_step"] = t[f"two_step_{what}_ms"]["median"] / t[f"fused_{what}_ms"]["median"]
        res[f"speedup_{what}_vs_torch"] = t[f"torch_{what}_ms"]["median"] / t[f"fused_{what}_ms"]["median"]
    print(json.dumps(res))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
