"""Time of the evaluation step's depth metrics and PSNR on two paths:

  native   metrics.depth_metrics / metrics.depth_scores / metrics.psnr (csrc/s360_eval_scores.hip)
  torch    a plain torch statement of the same scores WRITTEN FOR THIS PROJECT (masked sums with torch.where, one pass per
           metric).  It is NOT the reference's compute_depth_metrics_batched / compute_psnr — this script runs without the
           reference checkout — and it launches far fewer kernels than those (about 80 and 9 per call); read the ratio as
           "against a reasonable torch implementation", not as "against the reference".

HIP events around `--iters` back-to-back calls on one stream after `--warmup` calls, repeated `--reps` times (median and range of
the per-call time, host launch overhead included).  Shapes: 15 x 65 536 depth rows (five faces of three panoramas at 256 x 256)
and 15 x 262 144 (512 x 512 faces); 18 x 3 x 256 x 256 and 18 x 3 x 512 x 512 for PSNR.  Checks that the two paths agree to 1e-5
relative before timing.  One JSON line per (what, shape, path) on stdout; --out also writes them, with the commit hash, to a file.
usage: eval_scores_timing.py [--iters 200] [--warmup 20] [--reps 5] [--out profiles/eval_scores_timing.json] [--commit HASH]"""
import argparse
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT)]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from splatter360_amd import _lib, metrics  # noqa: E402

THRESHOLDS = (1.05, 1.10, 1.25, 1.10, 1.25, 1.25 ** 2, 1.25 ** 3)
TORCH_NOTE = "torch statement written for this project (masked sums); not the reference's function"


def torch_depth_metrics(gt, pred, valid, mult_a=True):
    """The twelve numbers per row, stacked [12, B], with torch.where-masked sums."""
    zero = torch.zeros((), dtype=gt.dtype, device=gt.device)
    d = gt - pred
    lg = torch.log(gt) - torch.log(pred)
    out = []
    for i, term in enumerate((d.abs(), d.abs() / gt, d * d / gt, d * d, lg * lg)):
        ok = valid & ~torch.isnan(term)
        m = (torch.where(ok, term, zero).sum(dim=1, dtype=torch.float64) / ok.sum(dim=1)).float()
        out.append(m.sqrt() if i >= 3 else m)
    thresh = torch.maximum(gt / pred, pred / gt)
    count = valid.sum(dim=1).float()
    for t in THRESHOLDS:
        a = (valid & (thresh < t)).sum(dim=1).float() / count
        out.append(a * 100 if mult_a else a)
    return torch.stack(out)


def torch_depth_scores(depth_pred, depth_gt):
    """The step's protocol around torch_depth_metrics: drop face 0, rows, valid = gt > 0.1, average over the valid rows -> [12]."""
    b, v = depth_gt.shape[:2]
    gt = depth_gt[:, :, 1:, :, :, 0].reshape(b * v * 5, -1)
    pred = depth_pred.view(b, v, 6, *depth_pred.shape[2:])[:, :, 1:].reshape(b * v * 5, -1)
    valid = gt > 0.1
    rows = torch_depth_metrics(gt, pred, valid)
    has = valid.any(dim=1)
    return torch.where(has, rows, torch.zeros((), device=gt.device)).sum(dim=1) / has.sum()


def torch_psnr(pred, gt):
    mse = ((gt.clip(0, 1) - pred.clip(0, 1)) ** 2).mean(dim=(1, 2, 3))
    return -10 * torch.where(mse == 0, torch.full_like(mse, 1e-10), mse).log10()


def time_calls(fn, iters, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    per_call = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        per_call.append(e0.elapsed_time(e1) * 1e3 / iters)
    return round(float(np.median(per_call)), 1), [round(min(per_call), 1), round(max(per_call), 1)]


def commit_hash():
    r = subprocess.run(["git", "rev-parse", "HEAD"], cwd=str(ROOT), capture_output=True, text=True)
    return r.stdout.strip() if r.returncode == 0 and r.stdout.strip() else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="recorded when the script does not run inside a git checkout")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_scores_timing.py needs a GPU (no CPU fallback)")
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    records = []

    def record(what, shape, path, fn, note):
        med, rng = time_calls(fn, a.iters, a.warmup, a.reps)
        rec = dict(what=what, shape=list(shape), path=path, us_per_call_median=med, us_per_call_range=rng, iters=a.iters,
                   reps=a.reps, note=note)
        records.append(rec)
        print(json.dumps(rec), flush=True)

    def close(x, y):
        x, y = x.double(), y.double()
        fin = torch.isfinite(x) & torch.isfinite(y)
        assert torch.equal(torch.isnan(x), torch.isnan(y)) and ((x - y).abs()[fin] <= 1e-5 * y.abs()[fin]).all(), (x, y)

    for face in (256, 512):
        depth_gt = torch.rand((1, 3, 6, face, face, 1), generator=g) * 9.9 + 0.05
        depth_gt[torch.rand(depth_gt.shape, generator=g) < 0.1] = 0.0
        depth_pred = (depth_gt.view(1, 18, face, face) * (1 + 0.1 * torch.randn((1, 18, face, face), generator=g))).abs() + 1e-3
        depth_gt, depth_pred = depth_gt.to(dev), depth_pred.to(dev)
        gt = depth_gt[0, :, 1:, :, :, 0].reshape(15, -1).contiguous()
        pred = depth_pred.view(3, 6, -1)[:, 1:].reshape(15, -1).contiguous()
        valid = gt > 0.1
        nat = metrics.depth_metrics(gt, pred, valid, True)
        close(torch.stack([nat[k] for k in metrics.DEPTH_METRIC_KEYS]), torch_depth_metrics(gt, pred, valid))
        sc = metrics.depth_scores(depth_pred, depth_gt)
        close(torch.stack([sc[k] for k in metrics.DEPTH_METRIC_KEYS]), torch_depth_scores(depth_pred, depth_gt))
        record("depth_metrics", gt.shape, "native", lambda: metrics.depth_metrics(gt, pred, valid, True),
               "rows, mask given; 2 kernels")
        record("depth_metrics", gt.shape, "torch", lambda: torch_depth_metrics(gt, pred, valid), TORCH_NOTE)
        record("depth_scores", depth_pred.shape, "native", lambda: metrics.depth_scores(depth_pred, depth_gt),
               "from output.depth and depth_cubes in place: face drop, gt > 0.1, average over valid faces; 3 kernels")
        record("depth_scores", depth_pred.shape, "torch", lambda: torch_depth_scores(depth_pred, depth_gt), TORCH_NOTE)
        x = torch.rand((18, 3, face, face), generator=g).to(dev)
        y = (x + 0.05 * torch.randn(x.shape, generator=g).to(dev)).contiguous()
        close(metrics.psnr(x, y), torch_psnr(x, y))
        record("psnr", x.shape, "native", lambda: metrics.psnr(x, y), "2 kernels")
        record("psnr", x.shape, "torch", lambda: torch_psnr(x, y), TORCH_NOTE)
    if a.out:
        doc = dict(commit=commit_hash() or a.commit, source_hash=_lib.source_hash(), device=torch.cuda.get_device_name(dev),
                   method="HIP events around back-to-back calls on one stream after warm-up; per-call time, host launch overhead "
                          "included; median and range over the repetitions",
                   torch_path=TORCH_NOTE, records=records)
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
