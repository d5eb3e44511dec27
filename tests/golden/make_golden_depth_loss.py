"""Records tests/golden/depth_loss.npz from the reference's own erode and compute_l1_sphere_loss (src/model/model_wrapper_helper.py,
which needs only torch), on CPU.  Run on a machine that has the reference checkout:

    python tests/golden/make_golden_depth_loss.py /path/to/splatter360

Recorded (prefix = case name):
  erode_*        input x [N,1,H,W] and erode(x, ksize): binary, non-binary and non-finite inputs, ksize 3 / 5 / 7, odd shapes
  loss_*         pred, target, mask (inputs_* where cases share them), keep_batch, the loss and the autograd gradients of pred
                 and target for an incoming gradient of ones (loss.sum().backward()); one case has an all-zero-mask batch
                 element, one a negative mask
  closure_*      the training step's compute_context_depth_loss (model_wrapper_erp.py:242-287) restated around the reference's
                 two functions — mask = depth > 0.1, far fill of depth < 1e-7 (in place), erode only when the mask has a hole,
                 0.1 x loss — with pred's gradient; one case with holes, one without
  row_weights_H  the reference's sin((h + 0.5) pi / H) for the heights above
"""
import importlib
import sys
from pathlib import Path

import numpy as np
import torch


def main(ref_root: str) -> None:
    sys.path.insert(0, ref_root)
    helper = importlib.import_module("src.model.model_wrapper_helper")
    erode, l1 = helper.erode, helper.compute_l1_sphere_loss
    g = torch.Generator().manual_seed(360)
    out = {}

    def rand(*shape):
        return torch.rand(shape, generator=g, dtype=torch.float32)

    # erode
    binary = (rand(2, 1, 24, 40) > 0.15).float()
    nonbin = rand(2, 1, 24, 40) * 3.0 - 1.0
    special = rand(1, 1, 11, 13)
    flat = special.view(-1)
    flat[[3, 40, 77]] = float("nan")
    flat[[10, 90]] = float("inf")
    flat[[20, 120]] = float("-inf")
    odd = (rand(3, 1, 5, 7) > 0.3).float()
    for name, x, k in (("binary5", binary, 5), ("binary3", binary, 3), ("nonbinary5", nonbin, 5), ("nonbinary7", nonbin, 7),
                       ("special5", special, 5), ("special3", special, 3), ("odd5", odd, 5), ("odd3", odd, 3)):
        out[f"erode_{name}_x"] = x.numpy()
        out[f"erode_{name}_k"] = np.int32(k)
        out[f"erode_{name}_y"] = erode(x, k).numpy()

    # loss
    def loss_case(name, p, t, m, keep_batch, inputs=None, mask_sign=1.0):
        p = p.clone().requires_grad_(True)
        t = t.clone().requires_grad_(True)
        loss = l1(p, t, mask=m, keep_batch=keep_batch)
        loss.sum().backward()
        if inputs is None:
            out[f"loss_{name}_pred"], out[f"loss_{name}_target"], out[f"loss_{name}_mask"] = p.detach().numpy(), t.detach().numpy(), m.numpy()
        else:                                                 # shared inputs: the mask is mask_sign * inputs_<inputs>_mask
            out[f"loss_{name}_inputs"] = np.array(inputs)
            out[f"loss_{name}_mask_sign"] = np.float32(mask_sign)
        out[f"loss_{name}_keep_batch"] = np.int32(keep_batch)
        out[f"loss_{name}_loss"] = loss.detach().numpy()
        out[f"loss_{name}_grad_pred"], out[f"loss_{name}_grad_target"] = p.grad.numpy(), t.grad.numpy()

    shape = (2, 2, 16, 48)
    p, t = rand(*shape) * 10.0, rand(*shape) * 10.0
    m = erode((rand(*shape) > 0.2).float().view(4, 1, *shape[2:])).view(shape)
    m0 = m.clone()
    m0[1] = 0.0                                               # batch element 1: an all-zero mask (den -> 1e-10)
    out["inputs_basic_pred"], out["inputs_basic_target"], out["inputs_basic_mask"] = p.numpy(), t.numpy(), m.numpy()
    out["inputs_zero_pred"], out["inputs_zero_target"], out["inputs_zero_mask"] = p.numpy(), t.numpy(), m0.numpy()
    loss_case("basic", p, t, m, False, "basic")
    loss_case("basic_keep", p, t, m, True, "basic")
    loss_case("zero_element_keep", p, t, m0, True, "zero")
    loss_case("zero_element", p, t, m0, False, "zero")
    loss_case("negative_mask_keep", p, t, -m, True, "basic", -1.0)  # den < 0: clamped to at most -1e-10
    p3, t3 = rand(1, 3, 13, 21) * 5.0, rand(1, 3, 13, 21) * 5.0
    t3.view(-1)[::17] = p3.view(-1)[::17]                     # ties: sign(0) = 0
    loss_case("odd", p3, t3, (rand(1, 3, 13, 21) > 0.3).float(), False)

    # the closure of model_wrapper_erp.py:242-287 around the reference's two functions
    def closure_case(name, pred, depth, far):
        pred = pred.clone().requires_grad_(True)
        depth_in = depth.clone()
        d = depth.clone()
        mask = d > 0.1
        d[d < 1e-7] = far
        mask = mask.float()
        eroded = False
        if not mask.all():
            b, v = mask.shape[:2]
            mask = erode(mask.view(b * v, 1, *mask.shape[2:])).view(mask.shape)
            eroded = True
        loss = 0.1 * l1(pred, d, mask=mask, keep_batch=False)
        loss.backward()
        out[f"closure_{name}_pred"], out[f"closure_{name}_depth"] = pred.detach().numpy(), depth_in.numpy()
        out[f"closure_{name}_far"] = np.float32(far)
        out[f"closure_{name}_mask"] = mask.numpy()
        out[f"closure_{name}_eroded"] = np.int32(eroded)
        out[f"closure_{name}_loss"] = loss.detach().numpy()
        out[f"closure_{name}_grad_pred"] = pred.grad.numpy()

    depth = rand(*shape) * 20.0 + 0.2
    holes = depth.clone()
    holes[rand(*shape) < 0.05] = 0.0                          # missing depth: filled with far, masked out
    holes[rand(*shape) < 0.02] = 0.05                         # closer than near: masked out, kept
    closure_case("holes", rand(*shape) * 20.0, holes, 100.0)
    closure_case("dense", rand(*shape) * 20.0, depth, 100.0)

    for h in (5, 13, 32, 37, 512):
        w = torch.arange(0, h, dtype=torch.float32)
        out[f"row_weights_{h}"] = torch.sin((w + 0.5) * torch.pi / h).numpy()

    dst = Path(__file__).resolve().parent / "depth_loss.npz"
    np.savez_compressed(dst, **out)
    print(dst, dst.stat().st_size, "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else ".")
