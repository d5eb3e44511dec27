"""Records tests/golden/depth_smooth.npz from the reference's own LossDepth (src/loss/loss_depth.py), on CPU.  Run on a machine
that has the reference checkout:

    python tests/golden/make_golden_depth_smooth.py /path/to/splatter360

src/loss/loss.py and src/loss/loss_depth.py are loaded by file path, so src/loss/__init__.py (and its lpips import) is never
touched; jaxtyping, src.dataset.types, src.model.decoder.decoder and src.model.types — annotations only — are stubs.

Recorded (prefix = case name: s2657_vn1, s2657_vn6, s1133_vn1):
  <case>_depth, _near, _far, _image      the inputs of tests/depth_smooth_reference.make_case (a pixel exactly at log(far), one
                                         exactly at log(near), pixels outside both bounds, two equal neighbours in each axis)
  <case>_<mode>_loss, _loss_w025, _grad  the loss for weight 1 and 0.25 and depth.grad (weight 1), for the four modes d1, d2,
                                         d1_bilateral, d2_bilateral (sigma_image = 2.0)
The maker asserts that the reference's float32 chain and the float64 statement take the same sign(t) decision at every term.
"""
import importlib.util
import sys
import types
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import depth_smooth_reference as R  # noqa: E402

CASES = (("s2657_vn1", (2, 6, 5, 7), 1, 11), ("s2657_vn6", (2, 6, 5, 7), 6, 12), ("s1133_vn1", (1, 1, 3, 3), 1, 13))


def load_reference(ref_root: str):
    """The reference's LossDepth and its config classes, loaded by path behind annotation-only stubs."""
    class _Subscriptable:
        def __class_getitem__(cls, item):
            return cls

    def stub(name, **attrs):
        mod = types.ModuleType(name)
        mod.__path__ = []
        mod.__dict__.update(attrs)
        sys.modules[name] = mod

    stub("jaxtyping", Float=_Subscriptable)
    for pkg in ("src", "src.loss", "src.dataset", "src.model", "src.model.decoder"):
        stub(pkg)
    stub("src.dataset.types", BatchedExample=dict)
    stub("src.model.decoder.decoder", DecoderOutput=object)
    stub("src.model.types", Gaussians=object)
    out = None
    for name in ("loss", "loss_depth"):
        spec = importlib.util.spec_from_file_location(f"src.loss.{name}", Path(ref_root) / "src" / "loss" / f"{name}.py")
        out = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = out
        spec.loader.exec_module(out)
    return out


def main(ref_root: str) -> None:
    ref = load_reference(ref_root)
    out = {}
    for case, shape, vn, seed in CASES:
        c = R.make_case(shape, vn, seed)
        for k, x in c.items():
            out[f"{case}_{k}"] = x
        near, far, image = (torch.from_numpy(c[k]) for k in ("near", "far", "image"))
        ln, lf = near.log().numpy(), far.log().numpy()
        batch = {"target": {"near": near, "far": far, "image": image}}
        d = c["depth"]
        assert (d == np.repeat(lf, shape[1] // vn, 1)[:, :, None, None]).any() and (d == np.repeat(ln, shape[1] // vn, 1)[:, :, None, None]).any()
        for mode, second, sigma in R.MODES:
            losses = {}
            for weight in (1.0, 0.25):
                loss_fn = ref.LossDepth(ref.LossDepthCfgWrapper(ref.LossDepthCfg(weight, sigma, second)))
                depth = torch.from_numpy(d).clone().requires_grad_(True)
                loss = loss_fn(types.SimpleNamespace(depth=depth), batch, None, 0)
                loss.backward()
                losses[weight] = (loss.detach().numpy(), depth.grad.numpy())
            out[f"{case}_{mode}_loss"], out[f"{case}_{mode}_grad"] = losses[1.0]
            out[f"{case}_{mode}_loss_w025"] = losses[0.25][0]
            # the reference's float32 chain, restated: the very same loss, and its sign decisions against the statement's
            loss32, tx, ty = R.torch_statement(torch.from_numpy(d), near, far, image, sigma, second, return_terms=True)
            assert torch.equal(loss32, torch.from_numpy(losses[1.0][0])), (case, mode)
            s = R.statement(d, ln, lf, c["image"], sigma, second)
            differing = int((np.sign(tx.numpy()) != np.sign(s["tx"])).sum() + (np.sign(ty.numpy()) != np.sign(s["ty"])).sum())
            assert differing == 0, (case, mode, differing)
            if not second:                                        # the equal neighbours: sign(0) = 0 is exercised
                assert (s["tx"] == 0).any() and (s["ty"] == 0).any()
    dst = HERE / "depth_smooth.npz"
    np.savez_compressed(dst, **out)
    print(dst, dst.stat().st_size, "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else ".")
