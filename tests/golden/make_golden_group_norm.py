"""Records tests/golden/group_norm.npz from the reference's own norm + activation sites, on CPU.  Run on a machine that has the
reference checkout:

    python tests/golden/make_golden_group_norm.py /path/to/splatter360

ldm_unet/util.py, attention.py, unet.py and backbone/unimatch/trident_conv.py, backbone.py are loaded by file path under stub
parent packages, so no package __init__ of the reference runs; besides torch they need einops only.

Recorded per case (prefix = case name, see PAIRS and BLOCKS):
  <case>_x, _g            input and output gradient (the output's shape) as int16 numerators k of the float32 values k / 64
                          (tests/group_norm_reference.lattice values, exact in float32)
  <case>_out64, _gx64     the reference's output and input gradient with the module in .double() on the inputs cast to float64
                          (GroupNorm8 / GroupNorm4 cast their input to float32: for this run their forward is nn.GroupNorm's)
  <case>_out32d, _gx32d   the float32 run, as the int32 distance in float32 steps from float32(_out64) / float32(_gx64)
  <case>_p_<key>          every 1-D parameter of the module (state_dict key); parameters are tests/group_norm_reference.randomise
                          values — nothing keeps its zero initialisation — and the convolution weights, too large to store,
                          are reproduced by the same call
  <case>_groups           the norm's group count (pairs only)
Data only.
"""
import importlib.util
import sys
import types
from pathlib import Path

import numpy as np
import torch
from torch import nn

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import group_norm_reference as R  # noqa: E402

# name: (shape, activation); the norm is built in main()
PAIRS = {"gn8_silu": ((2, 32, 6, 10), "silu"), "gn4_silu": ((1, 36, 5, 7), "silu"), "gn4_gelu": ((2, 32, 4, 6), "gelu"),
         "in_relu": ((3, 16, 5, 9), "relu")}
BLOCKS = {"resblock_same": (1, 32, 4, 6), "resblock_proj": (1, 64, 4, 6), "attention": (2, 32, 4, 6), "residual": (1, 64, 6, 8)}
ACTS = {"silu": nn.SiLU, "gelu": nn.GELU, "relu": nn.ReLU}


def load_reference(ref_root: str):
    """(util, unet, backbone) of the reference, loaded by path behind stub parent packages."""
    enc = Path(ref_root) / "src" / "model" / "encoder"
    for pkg in ("refgn", "refgn.ldm_unet", "refgn.unimatch"):
        mod = types.ModuleType(pkg)
        mod.__path__ = []
        sys.modules[pkg] = mod
    out = {}
    for name, rel in (("refgn.ldm_unet.util", "costvolume/ldm_unet/util.py"), ("refgn.ldm_unet.attention", "costvolume/ldm_unet/attention.py"),
                      ("refgn.ldm_unet.unet", "costvolume/ldm_unet/unet.py"), ("refgn.unimatch.trident_conv", "backbone/unimatch/trident_conv.py"),
                      ("refgn.unimatch.backbone", "backbone/unimatch/backbone.py")):
        spec = importlib.util.spec_from_file_location(name, enc / rel)
        out[name] = importlib.util.module_from_spec(spec)
        sys.modules[name] = out[name]
        spec.loader.exec_module(out[name])
    return out["refgn.ldm_unet.util"], out["refgn.ldm_unet.unet"], out["refgn.unimatch.backbone"]


def steps32(got32, want64):
    """got32 as the distance in float32 steps from float32(want64) (sign-magnitude integers made monotone)."""
    def key(a):
        i = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return (key(got32) - key(want64.astype(np.float32))).astype(np.int32)


def run(fn, module, x, g_seed, dtype):
    """(out, input gradient, g) with g the lattice of g_seed in the output's shape."""
    module = module.to(dtype)
    xin = torch.from_numpy(x).to(dtype).requires_grad_(True)
    out = fn(module, xin)
    g = R.lattice(tuple(out.shape), g_seed, span=255)
    out.backward(torch.from_numpy(g).to(dtype))
    return out.detach().numpy(), xin.grad.numpy(), g


def main(ref_root: str) -> None:
    util, unet, backbone = load_reference(ref_root)
    cast = {cls: cls.forward for cls in (util.GroupNorm8, util.GroupNorm4)}
    modules = {
        "gn8_silu": nn.Sequential(util.normalization(32), nn.SiLU()), "gn4_silu": nn.Sequential(util.normalization(36), nn.SiLU()),
        "gn4_gelu": nn.Sequential(nn.GroupNorm(4, 32), nn.GELU()), "in_relu": nn.Sequential(nn.InstanceNorm2d(16), nn.ReLU()),
        "resblock_same": unet.ResBlock(32, 0, 0.0, out_channels=32, dims=2, postnorm=True),
        "resblock_proj": unet.ResBlock(64, 0, 0.0, out_channels=32, dims=2, postnorm=True),
        "attention": unet.AttentionBlock(32, num_head_channels=32, postnorm=True, num_frames=2, use_cross_view_self_attn=True),
        "residual": backbone.ResidualBlock(64, 96, stride=2),
    }
    assert type(modules["gn8_silu"][0]) is util.GroupNorm8 and modules["gn8_silu"][0].num_groups == 8
    assert type(modules["gn4_silu"][0]) is util.GroupNorm4 and modules["gn4_silu"][0].num_groups == 4
    calls = {"resblock_same": lambda m, t: m._forward(t), "resblock_proj": lambda m, t: m._forward(t), "attention": lambda m, t: m._forward(t)}
    out = {}
    for seed, case in enumerate(modules):
        module = R.randomise(modules[case], seed)
        shape = PAIRS[case][0] if case in PAIRS else BLOCKS[case]
        x = R.lattice(shape, 500 + seed, span=255)
        fn = calls.get(case, lambda m, t: m(t))
        out32, gx32, g = run(fn, module, x, 600 + seed, torch.float32)
        for cls in cast:
            cls.forward = nn.GroupNorm.forward
        try:
            out64, gx64, _ = run(fn, module, x, 600 + seed, torch.float64)
        finally:
            for cls, fwd in cast.items():
                cls.forward = fwd
        out.update({f"{case}_x": np.round(x * 64).astype(np.int16), f"{case}_g": np.round(g * 64).astype(np.int16), f"{case}_out64": out64, f"{case}_gx64": gx64,
                    f"{case}_out32d": steps32(out32, out64), f"{case}_gx32d": steps32(gx32, gx64)})
        for key, p in module.state_dict().items():
            if p.dim() == 1:
                out[f"{case}_p_{key}"] = p.detach().to(torch.float32).numpy()
        if case in PAIRS:
            norm, act = module[0], PAIRS[case][1]
            groups = norm.num_groups if isinstance(norm, nn.GroupNorm) else shape[1]
            out[f"{case}_groups"] = np.array(groups, dtype=np.int64)
            # the maker's own check: the float64 statement is the reference, to rounding; relu's branch is unambiguous
            want = R.statement(x, groups, getattr(norm, "weight", None), getattr(norm, "bias", None), norm.eps, act, None, g)
            for name, ref in (("out", out64), ("g_x", gx64)):
                err = np.abs(want[name] - ref).max() / np.abs(ref).max()
                assert err <= 1e-13, (case, name, err)
            assert act != "relu" or R.relu_is_unambiguous(want), case
    dst = HERE / "group_norm.npz"
    np.savez_compressed(dst, **out)
    print(dst, dst.stat().st_size, "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else ".")
