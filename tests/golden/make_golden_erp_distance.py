"""Records tests/golden/erp_distance.npz from the reference's own depth_to_distance_map_batch (src/geometry/z_depth_to_distance.py),
Cube2Equirec (src/geometry/layers.py) and change_order_batch (src/model/model_wrapper_erp.py:147-158), on CPU.  The two geometry
files are imported directly; model_wrapper_erp pulls in Lightning, so change_order_batch is compiled from its source at generation
time, as make_golden.py does for change_order.  Run on a machine that has the reference checkout and einops:

    python tests/golden/make_golden_erp_distance.py /path/to/splatter360

Recorded (arrays only):
  dist_<h>_depth      float32 [N, h, h]   z-depth maps: one exact 0, one negative value, one inf, the rest in [0.5, 10)
  dist_<h>_fxfycxcy   float32 [N, 4]      fx != fy, cx != cy, different per map
  dist_<h>_out        float32 [N, h, h]   depth_to_distance_map_batch(depth, repeat(fxfycxcy))
  dist_<h>_gout       float32 [N, h, h]   the incoming gradient, drawn at random
  dist_<h>_grad       float32 [N, h, h]   torch's autograd of the call for gout: NaN at the zero depth
      for (N, h) = (5, 8) and (6, 24);
  closure_<fw>_<eh>_<ew>_<hm3d|pert>_...: model_wrapper_erp.py:446-463 run around those three functions
    depth             float32 [v, 6, fw, fw]   rendered z-depth faces BEFORE the call (change_order_batch writes to its argument)
    intrinsics        float32 [v, 6, 3, 3]     normalised intrinsics_cubes: hm3d's (0.5, 0.5, 0.5, 0.5), or perturbed per face
    fxfycxcy          float32 [v 6, 4]         :450-454
    dist              float32 [v 6, fw, fw]    the distance faces of :457 (slot order)
    erp               float32 [v, eh, ew]      :462-463
      for (v, fw, eh, ew) = (2, 8, 16, 32) and (3, 24, 48, 96); the perturbed runs hold one 0, one negative depth and one inf.
"""
import ast
import importlib.util
import sys
from pathlib import Path

import numpy as np
import torch
from einops import rearrange, repeat

DIST_SHAPES = ((5, 8), (6, 24))
CLOSURE_SHAPES = ((2, 8, 16, 32), (3, 24, 48, 96))
OUT = Path(__file__).resolve().parent / "erp_distance.npz"


def _load(ref_root, rel, name):
    spec = importlib.util.spec_from_file_location(name, Path(ref_root) / rel)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _change_order_batch(ref_root):
    tree = ast.parse((Path(ref_root) / "src" / "model" / "model_wrapper_erp.py").read_text())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "change_order_batch"][0]
    ns = {"torch": torch}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), "change_order_batch", "exec"), ns)
    return ns["change_order_batch"]


def _special(rng, depth):
    """One exact 0, one negative value and one inf at distinct random places of depth (in place)."""
    flat = depth.reshape(-1)
    idx = rng.choice(flat.size, 3, replace=False)
    flat[idx[0]] = 0.0
    flat[idx[1]] = -flat[idx[1]]
    flat[idx[2]] = np.inf


def main(ref_root: str) -> None:
    z2d = _load(ref_root, "src/geometry/z_depth_to_distance.py", "ref_z_depth_to_distance")
    layers = _load(ref_root, "src/geometry/layers.py", "ref_geometry_layers")
    change_order_batch = _change_order_batch(ref_root)
    rng = np.random.default_rng(457)
    out = {"dist_shapes": np.array(DIST_SHAPES, np.int32), "closure_shapes": np.array(CLOSURE_SHAPES, np.int32)}

    for n, h in DIST_SHAPES:
        depth = rng.uniform(0.5, 10.0, (n, h, h)).astype(np.float32)
        _special(rng, depth)
        k4 = np.stack([rng.uniform(0.4, 0.7, n) * h, rng.uniform(0.8, 1.3, n) * h,
                       rng.uniform(0.3, 0.45, n) * h, rng.uniform(0.55, 0.7, n) * h], 1).astype(np.float32)
        gout = rng.standard_normal((n, h, h)).astype(np.float32)
        d = torch.from_numpy(depth).requires_grad_(True)
        res = z2d.depth_to_distance_map_batch(d, repeat(torch.from_numpy(k4), "vc r -> vc r h w", h=h, w=h))
        grad, = torch.autograd.grad(res, d, torch.from_numpy(gout))
        p = f"dist_{h}_"
        out[p + "depth"], out[p + "fxfycxcy"], out[p + "gout"] = depth, k4, gout
        out[p + "out"], out[p + "grad"] = res.detach().numpy(), grad.numpy()
        zero = depth == 0
        assert zero.sum() == 1 and np.isnan(out[p + "grad"][zero]).all() and (depth < 0).sum() == 1 and np.isinf(depth).sum() == 1
        assert out[p + "out"].dtype == np.float32 and out[p + "grad"].dtype == np.float32

    for v, fw, eh, ew in CLOSURE_SHAPES:
        c2e = layers.Cube2Equirec(fw, eh, ew)
        for kind in ("hm3d", "pert"):
            depth = rng.uniform(0.5, 10.0, (v, 6, fw, fw)).astype(np.float32)
            intr = np.zeros((v, 6, 3, 3), np.float32)
            intr[..., 0, 0] = intr[..., 1, 1] = intr[..., 0, 2] = intr[..., 1, 2] = 0.5
            intr[..., 2, 2] = 1.0
            if kind == "pert":
                _special(rng, depth)
                intr[..., 0, 0] += rng.uniform(-0.1, 0.1, (v, 6)).astype(np.float32)
                intr[..., 1, 1] += rng.uniform(0.15, 0.3, (v, 6)).astype(np.float32)
                intr[..., 0, 2] += rng.uniform(-0.09, -0.02, (v, 6)).astype(np.float32)
                intr[..., 1, 2] += rng.uniform(0.02, 0.09, (v, 6)).astype(np.float32)
            num_cubes = 6
            depths_prob = torch.from_numpy(depth.copy())
            intrinsics_all = torch.from_numpy(intr)
            # model_wrapper_erp.py:446-463 around the reference's three functions
            reordered = change_order_batch(depths_prob)
            intrinsics_cubes = rearrange(intrinsics_all, "v cubes r1 r2 -> (v cubes) r1 r2")
            reordered = rearrange(reordered, "v cubes h w -> (v cubes) h w")
            height, width = reordered.shape[-2:]
            fxfycxcy = torch.stack([intrinsics_cubes[:, 0, 0] * width, intrinsics_cubes[:, 1, 1] * height,
                                    intrinsics_cubes[:, 0, 2] * width, intrinsics_cubes[:, 1, 2] * height], dim=1)
            dist = z2d.depth_to_distance_map_batch(reordered, repeat(fxfycxcy, "vc r -> vc r h w", h=height, w=width))
            cube = rearrange(dist, "(v cubes) h w -> v () h (cubes w)", v=v, cubes=num_cubes)
            erp = c2e(cube).squeeze(1)
            p = f"closure_{fw}_{eh}_{ew}_{kind}_"
            out[p + "depth"], out[p + "intrinsics"], out[p + "fxfycxcy"] = depth, intr, fxfycxcy.numpy()
            out[p + "dist"], out[p + "erp"] = dist.numpy(), erp.numpy()
            assert out[p + "dist"].dtype == np.float32 and out[p + "erp"].shape == (v, eh, ew)

    np.savez_compressed(OUT, **out)
    print(OUT, OUT.stat().st_size, "bytes")
    assert OUT.stat().st_size < 400 * 1024


if __name__ == "__main__":
    main(sys.argv[1])
