"""Records tests/golden/eval_scores.npz from the reference's own compute_depth_metrics_batched (src/scripts/compute_depth_metrics.py,
which needs only torch) and from the expression of its compute_psnr (src/evaluation/metrics.py:16-21, evaluated here without
einops: `reduce(x, "b c h w -> b", "mean")` is `x.mean(dim=(1, 2, 3))`), on CPU.  Run on a machine that has the reference checkout:

    python tests/golden/make_golden_eval_scores.py /path/to/splatter360

Recorded (numbers only; inputs once per case):
  depth_<case>_gt / _pred / _valid       float32 [B,N], float32 [B,N], bool [B,N]
  depth_<case>_out / _out_mult           float32 [12,B] in the order of depth_keys, mult_a False / True
    holes    15 x 2304: gt == 0 on a stride, row 3 without a valid element, pred == 0 on a stride, NaN pred (row 5), negative
             pred (row 6), and in row 7 gt = 1 against pred = float32(t) and one ulp below, for the five thresholds
    clean    4 x 1000: every pred positive (finite rmse_log)
    masked   3 x 777: a validity plane unrelated to gt
  psnr_pred / psnr_gt / psnr_out         float32 [10,3,24,24] twice, float32 [10]: noise 0.2, 0.05, 1e-2, 1e-3, 1e-4, 1e-5 on values
                                          in [-0.1, 1.1], the same with values far outside [0, 1], an identical pair (100 dB), a
                                          NaN pixel, an all-clipped pair
"""
import importlib
import sys
from pathlib import Path

import numpy as np
import torch

KEYS = ("abs_diff", "abs_rel", "sq_rel", "rmse", "rmse_log", "a5", "a10", "a25", "a0", "a1", "a2", "a3")


def main(ref_root: str) -> None:
    sys.path.insert(0, ref_root)
    ref = importlib.import_module("src.scripts.compute_depth_metrics").compute_depth_metrics_batched
    g = torch.Generator().manual_seed(360)
    out = {"depth_keys": np.array(KEYS)}

    def rand(*shape):
        return torch.rand(shape, generator=g, dtype=torch.float32)

    def randn(*shape):
        return torch.randn(shape, generator=g, dtype=torch.float32)

    def depth_case(name, gt, pred, valid):
        out[f"depth_{name}_gt"], out[f"depth_{name}_pred"], out[f"depth_{name}_valid"] = gt.numpy(), pred.numpy(), valid.numpy()
        for suffix, mult in (("out", False), ("out_mult", True)):
            r = ref(gt, pred, valid, mult_a=mult)
            assert tuple(r.keys()) == KEYS
            out[f"depth_{name}_{suffix}"] = torch.stack([r[k] for k in KEYS]).numpy()

    B, N = 15, 48 * 48
    gt = rand(B, N) * 9.9 + 0.05
    gt[:, ::7] = 0.0                                          # holes
    gt[3] = 0.0                                               # a face without any valid depth
    pred = gt * (1 + 0.2 * randn(B, N)) + 0.05 * randn(B, N)
    pred[:, ::11] = 0.0                                       # uncovered pixels
    pred[5, 5:50] = float("nan")
    pred[6, 5:50] = -1.0
    for i, t in enumerate((1.05, 1.10, 1.25, 1.25 ** 2, 1.25 ** 3)):
        t32 = np.float32(t)
        gt[7, 1 + 2 * i] = 1.0
        pred[7, 1 + 2 * i] = float(t32)                       # thresh == float32(t): a miss
        gt[7, 2 + 2 * i] = 1.0
        pred[7, 2 + 2 * i] = float(np.nextafter(t32, np.float32(0)))   # one ulp below: a hit
    depth_case("holes", gt, pred, gt > 0.1)

    gt = rand(4, 1000) * 9.9 + 0.05
    depth_case("clean", gt, (gt * (1 + 0.1 * randn(4, 1000))).abs() + 1e-3, gt > 0.1)

    gt = rand(3, 777) * 5.0 + 0.01
    depth_case("masked", gt, gt + 0.3 * randn(3, 777), rand(3, 777) > 0.3)

    def ref_psnr(ground_truth, predicted):
        ground_truth = ground_truth.clip(min=0, max=1)
        predicted = predicted.clip(min=0, max=1)
        mse = ((ground_truth - predicted) ** 2).mean(dim=(1, 2, 3))
        mse[mse == 0.0] = 1e-10
        return -10 * mse.log10()

    shape = (3, 24, 24)
    gts, preds = [], []
    for noise in (0.2, 0.05, 1e-2, 1e-3, 1e-4, 1e-5):
        x = rand(*shape) * 1.2 - 0.1
        gts.append(x)
        preds.append(x + noise * randn(*shape))
    x = rand(*shape) * 4.0 - 1.5                              # values far outside [0, 1]
    gts.append(x)
    preds.append(x + 0.3 * randn(*shape))
    x = rand(*shape)
    gts.append(x)
    preds.append(x.clone())                                   # identical: 100 dB
    x = rand(*shape)
    y = x + 0.01 * randn(*shape)
    y[1, 2, 3] = float("nan")
    gts.append(x)
    preds.append(y)
    gts.append(rand(*shape) + 1.5)                            # both clipped to 1 everywhere: 100 dB
    preds.append(rand(*shape) + 2.5)
    gt4, pred4 = torch.stack(gts), torch.stack(preds)
    out["psnr_gt"], out["psnr_pred"] = gt4.numpy(), pred4.numpy()
    out["psnr_out"] = ref_psnr(gt4, pred4).numpy()

    dst = Path(__file__).resolve().parent / "eval_scores.npz"
    np.savez_compressed(dst, **out)
    print(dst, dst.stat().st_size, "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else ".")
