"""Time of the training step's context-depth loss, forward + backward, on three paths (model_wrapper_erp.py:242-287):

  torch     the reference's closure restated on stock torch: mask, far fill (in place, on a copy made outside the timed region),
            `mask.all()` on the host, erode (pad + max_pool2d), compute_l1_sphere_loss, x 0.1, backward
  two-step  the same closure with erode and compute_l1_sphere_loss rebound to the kernels (what install(depth_loss=True) gives:
            the torch mask / fill / `.all()` stay)
  fused     depth_loss.context_depth_loss: two kernels forward, one backward, no host synchronisation

HIP events around `--iters` back-to-back forward + backward calls on one stream after `--warmup` calls, repeated `--reps` times
(median and range of the per-call time).  Shapes: (14, 2, 512, 1024) (the hm3d experiment: batch 14, 2 context views) and
(1, 2, 512, 1024).  Also checks that the three losses agree (fused == two-step bit for bit; torch within 1e-5 relative).  One JSON
line per (shape, path) on stdout.  Per-kernel times: run under `rocprofv3 --kernel-trace --stats` with --paths fused,two-step.
usage: depth_loss_timing.py [--iters 50] [--warmup 5] [--reps 5] [--paths torch,two-step,fused] [--shapes 14x2x512x1024,...]"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from splatter360_amd import depth_loss  # noqa: E402

SHAPES = ((14, 2, 512, 1024), (1, 2, 512, 1024))


def torch_erode(x, k=5):
    pad = (k - 1) // 2
    return 1 - F.max_pool2d(F.pad(1 - x, pad=[pad, pad, pad, pad], mode="reflect"), kernel_size=k, stride=1, padding=0)


def torch_l1_sphere(y_pred, y_true, mask):
    b, v, h, w = y_pred.shape
    sin_phi = torch.arange(0, h, dtype=y_pred.dtype, device=y_pred.device)
    sin_phi = torch.sin((sin_phi + 0.5) * torch.pi / h)
    sin_phi = sin_phi.view(1, 1, h, 1).expand(b, v, h, w) * mask
    loss = torch.abs(y_true - y_pred) * sin_phi
    den = torch.sum(sin_phi, dim=(0, 1, 2, 3))
    z = torch.tensor(0.0, device=den.device, dtype=den.dtype)
    den = torch.where(torch.ge(den, z), torch.max(den, z + 1e-10), torch.min(den, z - 1e-10))
    return torch.sum(loss, dim=(0, 1, 2, 3)) / den


def closure(pred, depth, far, erode, l1):
    """model_wrapper_erp.py:244-285 with the given erode / compute_l1_sphere_loss; depth is modified in place, as there."""
    mask = depth > 0.1
    depth[depth < 1e-7] = far
    mask = mask.float()
    if not mask.all():
        b, v = mask.shape[:2]
        mask = erode(mask.view(b * v, 1, *mask.shape[2:])).view(mask.shape)
    return 0.1 * l1(pred, depth, mask)


def make_inputs(shape, dev, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    depth = torch.rand(shape, generator=g) * 20.0 + 0.2
    holes = torch.rand(shape, generator=g)
    depth[holes < 0.03] = 0.0                                 # missing depth
    depth[(holes >= 0.03) & (holes < 0.04)] = 0.05            # closer than near
    pred = torch.rand(shape, generator=g) * 20.0
    far = torch.full((1, 2), 100.0)
    return pred.to(dev), depth.to(dev), far.to(dev)


def run_path(path, pred, depth, far):
    """One forward + backward; returns the loss."""
    p = pred.requires_grad_(True)
    if path == "torch":
        loss = closure(p, depth, far[0, 0], torch_erode, torch_l1_sphere)
    elif path == "two-step":
        loss = closure(p, depth, far[0, 0], depth_loss.erode, depth_loss.compute_l1_sphere_loss)
    else:
        loss = depth_loss.context_depth_loss(p, depth, far[0, 0])
    loss.backward()
    return loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--paths", default="torch,two-step,fused")
    ap.add_argument("--shapes", default=",".join("x".join(str(s) for s in sh) for sh in SHAPES))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("depth_loss_timing.py needs a GPU (no CPU fallback)")
    dev = torch.device("cuda:0")
    paths = a.paths.split(",")
    for shape in (tuple(int(s) for s in sh.split("x")) for sh in a.shapes.split(",")):
        pred, depth, far = make_inputs(shape, dev)
        losses = {}
        for path in paths:
            # the reference fills depth in place: every call gets its own copy, made outside the timed region
            p = pred.clone()
            for _ in range(a.warmup):
                p.grad = None
                losses[path] = run_path(path, p, depth.clone(), far).detach()
            torch.cuda.synchronize()
            per_call = []
            for _ in range(a.reps):
                copies = [depth.clone() for _ in range(a.iters)] if path != "fused" else [depth] * a.iters
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(a.iters):
                    p.grad = None
                    run_path(path, p, copies[i], far)
                e1.record()
                e1.synchronize()
                per_call.append(e0.elapsed_time(e1) * 1e3 / a.iters)
            n = int(np.prod(shape))
            rec = dict(shape=list(shape), path=path, what="forward + backward per call, host overhead included",
                       us_per_call_median=round(float(np.median(per_call)), 1),
                       us_per_call_range=[round(min(per_call), 1), round(max(per_call), 1)], iters=a.iters, reps=a.reps,
                       loss=float(losses[path]), pixels=n, device=torch.cuda.get_device_name(dev))
            print(json.dumps(rec), flush=True)
            del copies
        if "fused" in losses and "two-step" in losses:
            assert torch.equal(losses["fused"], losses["two-step"]), (losses["fused"], losses["two-step"])
        if "fused" in losses and "torch" in losses:
            t = float(losses["torch"])
            assert abs(float(losses["fused"]) - t) <= 1e-5 * abs(t), losses


if __name__ == "__main__":
    main()
