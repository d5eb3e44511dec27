"""Records tests/golden/mono_fusion.npz from the reference's own Cube2Equirec (src/geometry/layers.py:41-116) and an nn.Sequential
of rgbd_fusion's four layers (src/model/encoder/encoder_costvolume.py:119-125), on CPU.  Run on a machine that has the reference
checkout:

    python tests/golden/make_golden_mono_fusion.py /path/to/splatter360

layers.py is loaded by file path (besides numpy and torch it imports nothing), so no package __init__ of the reference runs.  The
statements are those of encoder_costvolume.py:297 and :351-354: the stitch under no_grad, torch.cat along the channels, the
channel-last permute, the Sequential, the permute back.  Widths d = 16, Cm = 24, (face_w, equ_h, equ_w) = (4, 8, 16), N = 2.

Recorded:
  erp_feat, mono_cube, g       inputs and output gradient as int16 numerators k of the float32 values k / 64
  p_0.weight, p_1.weight, p_1.bias, p_3.weight
                               the Sequential's parameters by state_dict key, the same way (the norm's weight is 1 + k / 64)
  grid                         the module's sample_grid[0, 0], float32
  out64, g_erp_feat64, g_0.weight64, g_1.weight64, g_1.bias64, g_3.weight64
                               the run with the stitch in float32 (the module as it is) and everything behind it in float64
  out32d, ...                  the all-float32 run, as the int32 distance in float32 steps from float32(the float64 value)
  cfg                          (N, d, Cm, face_w, equ_h, equ_w) int64
Data only.
"""
import importlib.util
import sys
from pathlib import Path

import numpy as np
import torch
from torch import nn

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE.parent.parent))
sys.path.insert(0, str(HERE))

import group_norm_reference as G  # noqa: E402
import mono_fusion_reference as R  # noqa: E402
from make_golden_qkv_attention import steps32  # noqa: E402
from make_golden_transformer_ffn import numerators  # noqa: E402

N, D, CM, GEOMETRY = 2, 16, 24, (4, 8, 16)
KEYS = ("0.weight", "1.weight", "1.bias", "3.weight")


def load_layers(ref_root: str):
    spec = importlib.util.spec_from_file_location("refsrc_layers", Path(ref_root) / "src" / "geometry" / "layers.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(ref_root: str) -> None:
    fw, h, w = GEOMETRY
    c2e = load_layers(ref_root).Cube2Equirec(fw, h, w)
    grid = c2e.sample_grid.detach()[0, 0].clone()
    assert np.array_equal(grid.numpy(), R.grid_of(GEOMETRY).numpy())                    # the project's grid, bit for bit
    fusion = nn.Sequential(nn.Linear(D + CM, D, bias=False), nn.LayerNorm(D), nn.ReLU(), nn.Linear(D, D, bias=False))
    assert tuple(k for k, _ in fusion.named_parameters()) == KEYS
    with torch.no_grad():
        for i, (key, p) in enumerate(fusion.named_parameters()):
            val = G.lattice(tuple(p.shape), 3000 + i, scale=1.0 / 16.0, span=7) if p.dim() == 2 else G.lattice(tuple(p.shape), 3000 + i, span=63)
            p.copy_(torch.from_numpy(val + 1.0 if key == "1.weight" else val))
    erp, cube, g = (torch.from_numpy(G.lattice(s, 3100 + i, span=255)) for i, s in enumerate(((N, D, h, w), (N, CM, fw, 6 * fw), (N, D, h, w))))
    runs = {}
    for dtype in (torch.float32, torch.float64):
        net = fusion.to(dtype)
        net.zero_grad(set_to_none=True)
        x = erp.detach().clone().to(dtype).requires_grad_(True)
        with torch.no_grad():
            features_mono = c2e(cube)                                                    # float32 in both runs
        t = torch.cat([x, features_mono.to(dtype)], dim=1)
        t = net(t.permute(0, 2, 3, 1)).permute(0, 3, 1, 2)
        t.backward(g.to(dtype))
        runs[dtype] = {"out": t.detach().numpy(), "g_erp_feat": x.grad.numpy(), **{"g_" + k: p.grad.numpy().copy() for k, p in net.named_parameters()}}
    fusion.to(torch.float32)
    out = {"erp_feat": numerators(erp.numpy()), "mono_cube": numerators(cube.numpy()), "g": numerators(g.numpy()), "grid": grid.numpy(),
           "cfg": np.array([N, D, CM, fw, h, w], dtype=np.int64)}
    params = {k: p.detach().clone() for k, p in fusion.named_parameters()}
    for k, p in params.items():
        out["p_" + k] = numerators(p.numpy() - (1.0 if k == "1.weight" else 0.0))
    for name, v64 in runs[torch.float64].items():
        out[name + "64"] = v64
        out[name + "32d"] = steps32(runs[torch.float32][name], v64)
    # the maker's own check: the float64 statement is the reference, to rounding
    want = R.statement(erp, cube, grid, params["0.weight"], params["1.weight"], params["1.bias"], params["3.weight"], fusion[1].eps)
    err = (want - torch.from_numpy(runs[torch.float64]["out"])).abs().max().item()
    assert err <= 1e-13 * max(1.0, want.abs().max().item()), err
    dst = HERE / "mono_fusion.npz"
    np.savez_compressed(dst, **out)
    print(dst, dst.stat().st_size, "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else ".")
