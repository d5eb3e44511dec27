"""Regenerates tests/golden/cost_volume.npz from the reference implementation (data only: inputs and recorded results).

    python tests/golden/make_golden_cost_volume.py /path/to/reference

The reference's depth_predictor_multiview_360.py is loaded on its own, with stub modules for its two relative imports
(..backbone.unimatch.geometry, .ldm_unet.unet), together with src/geometry/utils360.py.  On CPU its
`spherical_coords[..., 2] = depth` raises, because einops.repeat returns an expanded view there; the loaded module's `repeat` is
therefore replaced by one that clones (no value changes).  Recorded per case (v = 2: C = 8, D = 16, 16 x 32; v = 3: C = 5, D = 7,
12 x 20; b = 1 and b = 2) and per depth sampling: prepare_feat_proj_data_lists_360's poses and candidates, the volume of
DepthPredictorMultiView360.forward :588-630 and autograd's gradient of the features for a recorded incoming gradient; for the
inverse_depth sampling also slot 0 of the first pairing's warped tensor."""
import importlib.util
import sys
import types
from pathlib import Path

import einops
import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
from cost_volume_reference import random_inputs  # noqa: E402

CASES = {"v2": dict(b=1, v=2, c=8, d=16, h=16, w=32, seed=11), "v3": dict(b=2, v=3, c=5, d=7, h=12, w=20, seed=12)}
SAMPLINGS = ("inverse_depth", "log_depth", "linear_depth")


def load_reference(root: Path):
    pkg = "refsrc.model.encoder.costvolume"
    for name in ("refsrc", "refsrc.model", "refsrc.model.encoder", pkg, "refsrc.model.encoder.backbone", "refsrc.model.encoder.backbone.unimatch",
                 pkg + ".ldm_unet"):
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
    geo = types.ModuleType("refsrc.model.encoder.backbone.unimatch.geometry")
    geo.coords_grid = None
    sys.modules[geo.__name__] = geo
    unet = types.ModuleType(pkg + ".ldm_unet.unet")
    unet.UNetModel = None
    sys.modules[unet.__name__] = unet
    mods = []
    for name, rel in ((pkg + ".depth_predictor_multiview_360", "src/model/encoder/costvolume/depth_predictor_multiview_360.py"),
                      ("refsrc.geometry_utils360", "src/geometry/utils360.py")):
        spec = importlib.util.spec_from_file_location(name, root / rel)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        mods.append(mod)
    mods[0].repeat = lambda *a, **k: einops.repeat(*a, **k).clone()
    return mods


def main(root: Path):
    dp, u360 = load_reference(root)
    out = {}
    for key, cs in CASES.items():
        b, v, c, d, h, w = (cs[k] for k in "bvcdhw")
        feats, ext, near, far = random_inputs(b, v, c, h, w, cs["seed"])
        g = torch.randn(v * b, d, h, w, generator=torch.Generator().manual_seed(cs["seed"] + 100))
        utils = u360.Utils({"dataset_name": "hm3d", "batch_size": b, "height": h, "width": w})
        out.update({f"{key}/features": feats, f"{key}/extrinsics": ext, f"{key}/near": near, f"{key}/far": far, f"{key}/grad_out": g})
        for smp in SAMPLINGS:
            f = feats.clone().requires_grad_(True)
            lists, poses, cand = dp.prepare_feat_proj_data_lists_360(f, ext, near, far, d, smp)
            feat01, vols = lists[0], []
            for k, (feat10, pose) in enumerate(zip(lists[1:], poses)):
                warped = dp.warp_with_pose_depth_candidates(utils, feat10, pose, cand.repeat([1, 1, h, w]), warp_padding_mode="zeros")
                vols.append((feat01.unsqueeze(2) * warped).sum(1) / (c ** 0.5))
                if k == 0 and smp == "inverse_depth":
                    out[f"{key}/warped0"] = warped[0].detach()
            vol = torch.mean(torch.stack(vols, dim=0), dim=0, keepdim=False)
            (vol * g).sum().backward()
            out.update({f"{key}/{smp}/poses": torch.stack(list(poses), dim=0), f"{key}/{smp}/candidates": cand[:, :, 0, 0].detach(),
                        f"{key}/{smp}/volume": vol.detach(), f"{key}/{smp}/grad_features": f.grad})
    np.savez_compressed(HERE / "cost_volume.npz", **{k: t.numpy() for k, t in out.items()})
    print("wrote", HERE / "cost_volume.npz", (HERE / "cost_volume.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main(Path(sys.argv[1]))
