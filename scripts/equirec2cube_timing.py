"""Times the native ERP -> cube resampler — Equirec2Cube.faces(order="rendered"): one kernel, one backward kernel — forward and
forward + backward, against a plain torch statement of the same resampling on the same GPU, at the hm3d shape (B = 4 panoramas of
3 x 512 x 1024 -> 256 x 256 faces), and records the accuracy figures of tests/test_gpu_equirec2cube.py's rule against float64
-> profiles/equirec2cube_timing.json.

    timeout -k 10 600 python scripts/equirec2cube_timing.py [--out profiles/equirec2cube_timing.json] [--calls 200]

The torch statement is four precomputed index gathers (the plan's own tap texels), a weighted float32 sum, then the loader's
permute and flip copies (dataset_hm3d.py:204-213).  The reference's own path is numpy + scipy on the host and is not timed here.
Each figure is the median of `calls` timed calls (HIP events around one call, launch overhead included) after 10 warm-up calls, the
two sides alternating in one process."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import equirec2cube_reference as R  # noqa: E402
from splatter360_amd import _lib, equirec2cube as E  # noqa: E402

SHAPE = {"b": 4, "c": 3, "equ_h": 512, "equ_w": 1024, "face_w": 256}


class TorchStatement:
    """faces(order="rendered") in plain torch, float32: out = sum_k erp[..., tex_k] * w_k, split into faces, permuted and flipped."""

    def __init__(self, h, w, fw, dev):
        cy, cx = R.coordinates(h, w, fw)
        tex, wy, wx, _ = R.taps(cy, cx, h, w)
        self.fw = fw
        self.tex = [torch.from_numpy(tex[:, k].copy()).to(dev) for k in range(4)]
        self.wgt = [torch.from_numpy((wy[:, k] * wx[:, k]).astype(np.float32)).to(dev) for k in range(4)]

    def __call__(self, erp):
        b, c, h, w = erp.shape
        flat = erp.reshape(b, c, h * w)
        cube = sum(flat[:, :, t] * wk for t, wk in zip(self.tex, self.wgt)).reshape(b, c, self.fw, 6 * self.fw)
        f = torch.stack(cube.split(self.fw, dim=-1), 1)
        return torch.stack([f[:, k & 7].flip(-1, -2) if k & 8 else f[:, k & 7] for k in E.RENDERED_FACE_MAP], 1).contiguous()


def timed_pair(fns, calls, warmup=10):
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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "equirec2cube_timing.json"))
    ap.add_argument("--calls", type=int, default=200)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    b, c, h, w, fw = (SHAPE[k] for k in ("b", "c", "equ_h", "equ_w", "face_w"))
    native = E.Equirec2Cube(h, w, fw).to(dev)
    statement = TorchStatement(h, w, fw, dev)
    gen = torch.Generator(device=dev).manual_seed(3)
    erp = torch.rand(b, c, h, w, device=dev, generator=gen)
    g = torch.randn(b, 6, c, fw, fw, device=dev, generator=gen)

    def fwd(fn):
        def call():
            with torch.no_grad():
                return fn(erp)
        return call

    def fwd_bwd(fn):
        def call():
            leaf = erp.detach().requires_grad_(True)
            return torch.autograd.grad(fn(leaf), leaf, g)[0]
        return call

    nat = lambda x: native.faces(x, order="rendered")  # noqa: E731
    res = {"calls": args.calls, "device": torch.cuda.get_device_name(0), "source_hash": _lib.source_hash(), "shape": SHAPE,
           "bytes_moved_fwd": 4 * (b * c * h * w + b * c * 6 * fw * fw + 3 * 6 * fw * fw)}
    t = timed_pair({"native_fwd_ms": fwd(nat), "torch_fwd_ms": fwd(statement)}, args.calls)
    t.update(timed_pair({"native_fwd_bwd_ms": fwd_bwd(nat), "torch_fwd_bwd_ms": fwd_bwd(statement)}, args.calls))
    res.update(t)
    res["speedup_fwd"] = t["torch_fwd_ms"]["median"] / t["native_fwd_ms"]["median"]
    res["speedup_fwd_bwd"] = t["torch_fwd_bwd_ms"]["median"] / t["native_fwd_bwd_ms"]["median"]

    # accuracy of both sides against the float64 statement, on the first panorama (the rule of tests/test_gpu_equirec2cube.py)
    cy, cx = R.coordinates(h, w, fw)
    tp = R.taps(cy, cx, h, w)
    want = R.split_faces(R.forward64(erp[:1].cpu().numpy(), cy, cx, tp=tp), "rendered")
    want_g = R.adjoint64(R.join_faces(g[:1].cpu().numpy(), "rendered"), cy, cx, h, w, tp=tp)
    terms = R.adjoint64(R.join_faces(g[:1].cpu().numpy(), "rendered"), cy, cx, h, w, tp=tp, absolute=True)

    def ratios(fn):
        out = fn(erp[:1]).cpu().numpy().astype(np.float64)
        leaf = erp[:1].detach().requires_grad_(True)
        grad = torch.autograd.grad(fn(leaf), leaf, g[:1])[0].cpu().numpy().astype(np.float64)
        nz = want != 0
        bar = 2.0 ** -23 * np.abs(want_g) + 1e-12 * terms
        return {"forward_worst_err_over_2^-23_ref": float((np.abs(out - want)[nz] / (2.0 ** -23 * np.abs(want[nz]))).max()),
                "backward_worst_err_over_bar": float((np.abs(grad - want_g)[bar > 0] / bar[bar > 0]).max())}

    res["accuracy"] = {"native": ratios(nat), "torch_f32": ratios(statement)}
    print(json.dumps(res))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
