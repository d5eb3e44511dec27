"""Records tests/golden/qkv_attention.npz from the reference's own QKVAttentionLegacy and QKVAttention, on CPU.  Run on a machine
that has the reference checkout:

    python tests/golden/make_golden_qkv_attention.py /path/to/splatter360

ldm_unet/util.py, attention.py and unet.py are loaded by file path under stub parent packages, so no package __init__ of the
reference runs; besides torch they need einops only.

Recorded per case (prefix = case name, see CASES):
  <case>_qkv, _g          input [N, heads 3 ch, T] and output gradient [N, heads ch, T] as int16 numerators k of the float32 values
                          k / 64 (tests/group_norm_reference.lattice values, exact in float32)
  <case>_out64, _gqkv64   the reference's output and input gradient on the inputs cast to float64 (with the classes' float32
                          cast of the softmax's input switched off for this run: see main)
  <case>_out32d, _gqkv32d the float32 run, as the int32 distance in float32 steps from float32(_out64) / float32(_gqkv64)
  <case>_cfg              (N, heads, n_frames, cross_view, order: 0 legacy / 1 new, ch, T) int64
Data only.
"""
import importlib.util
import sys
import types
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import group_norm_reference as G  # noqa: E402
import qkv_attention_reference as R  # noqa: E402

# name: (N, heads, n_frames, cross_view, order, T); ch = 32
CASES = {
    "indexing": (6, 2, 3, True, "legacy", 2),         # heads = 2, views = 3, B = 2: every index rule changes the result
    "rows": (2, 1, 1, False, "legacy", 5),
    "frames_unused": (4, 1, 2, False, "legacy", 3),   # n_frames = 2 with cross-view off: rows stay separate
    "new_order": (1, 2, 1, False, "new", 4),
}
CH = 32


def load_unet(ref_root: str):
    enc = Path(ref_root) / "src" / "model" / "encoder"
    for pkg in ("refqa", "refqa.ldm_unet"):
        mod = types.ModuleType(pkg)
        mod.__path__ = []
        sys.modules[pkg] = mod
    out = None
    for name, rel in (("refqa.ldm_unet.util", "costvolume/ldm_unet/util.py"), ("refqa.ldm_unet.attention", "costvolume/ldm_unet/attention.py"),
                      ("refqa.ldm_unet.unet", "costvolume/ldm_unet/unet.py")):
        spec = importlib.util.spec_from_file_location(name, enc / rel)
        out = importlib.util.module_from_spec(spec)
        sys.modules[name] = out
        spec.loader.exec_module(out)
    return out


def steps32(got32, want64):
    """got32 as the distance in float32 steps from float32(want64) (sign-magnitude integers made monotone)."""
    def key(a):
        i = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return (key(got32) - key(want64.astype(np.float32))).astype(np.int32)


def main(ref_root: str) -> None:
    unet = load_unet(ref_root)
    out = {}
    for seed, (case, (n, heads, frames, cross, order, t)) in enumerate(CASES.items()):
        module = unet.QKVAttentionLegacy(heads, n_frames=frames, use_cross_view_self_attn=cross) if order == "legacy" \
            else unet.QKVAttention(heads)
        qkv = G.lattice((n, heads * 3 * CH, t), 700 + seed, span=255)
        g = G.lattice((n, heads * CH, t), 800 + seed, span=255)
        runs = {}
        for dtype in (torch.float32, torch.float64):
            # both classes cast the weights to float32 for the softmax (`weight.float()`), whatever comes in: for the float64 run
            # Tensor.float is the identity, so that the whole forward is float64
            cast = torch.Tensor.float
            if dtype is torch.float64:
                torch.Tensor.float = lambda self, *a, **k: self
            try:
                o, gx = R.gradients(module, torch.from_numpy(qkv), torch.from_numpy(g), dtype)
            finally:
                torch.Tensor.float = cast
            runs[dtype] = (o.numpy(), gx.numpy())
        out64, gx64 = runs[torch.float64]
        out.update({f"{case}_qkv": np.round(qkv * 64).astype(np.int16), f"{case}_g": np.round(g * 64).astype(np.int16),
                    f"{case}_out64": out64, f"{case}_gqkv64": gx64,
                    f"{case}_out32d": steps32(runs[torch.float32][0], out64), f"{case}_gqkv32d": steps32(runs[torch.float32][1], gx64),
                    f"{case}_cfg": np.array([n, heads, frames, int(cross), R.ORDERS.index(order), CH, t], dtype=np.int64)})
        # the maker's own check: the float64 statement is the reference, to rounding
        want = R.gradients(lambda x: R.statement(x, heads, frames, cross, order), torch.from_numpy(qkv), torch.from_numpy(g), torch.float64)
        for name, mine, ref in (("out", want[0].numpy(), out64), ("g_qkv", want[1].numpy(), gx64)):
            err = np.abs(mine - ref).max() / np.abs(ref).max()
            assert err <= 1e-13, (case, name, err)
    dst = HERE / "qkv_attention.npz"
    np.savez_compressed(dst, **out)
    print(dst, dst.stat().st_size, "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else ".")
