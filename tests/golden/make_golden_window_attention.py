"""Records tests/golden/window_attention.npz from the reference's own multi-view transformer attention
(src/model/encoder/backbone/multiview_transformer.py), on CPU.  Run on a machine that has the reference checkout:

    python tests/golden/make_golden_window_attention.py /path/to/splatter360

unimatch/position.py, unimatch/utils.py and multiview_transformer.py are loaded by file path under stub parent packages, so no
package __init__ of the reference runs; besides torch they need einops only.

Recorded per case (prefix = case name, see CASES):
  <case>_q, _k, _v, _g              float32 inputs of tests/window_attention_reference.random_case (C = 4) and the output gradient
  <case>_out64, _gq64, _gk64, _gv64   the reference's output and autograd gradients on the inputs cast to float64
  <case>_out32, _gq32, _gk32, _gv32   the same in float32
  <case>_mask                       generate_shift_window_attn_mask(...) of the case's grid (cases with num_splits > 1)
  <case>_meta                       int64 (B, m, h, w, K, shift, full)
"""
import importlib.util
import sys
import types
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import window_attention_reference as R  # noqa: E402

C = 4
# name: (B, m, h, w, K, shift, full)
CASES = {
    "self_s0": (2, 0, 4, 6, 2, 0, 0), "self_s1": (2, 0, 4, 6, 2, 1, 0),
    "m1_s0": (1, 1, 4, 6, 2, 0, 0), "m1_s1": (1, 1, 4, 6, 2, 1, 0),
    "m3_s0": (1, 3, 6, 8, 2, 0, 0), "m3_s1": (1, 3, 6, 8, 2, 1, 0),
    "odd_s1": (1, 0, 6, 10, 2, 1, 0),
    "k1": (2, 0, 3, 5, 1, 0, 0), "full": (2, 0, 3, 5, 1, 0, 1),
}


def load_reference(ref_root: str):
    """The reference's multiview_transformer module, loaded by path behind stub parent packages."""
    base = Path(ref_root) / "src" / "model" / "encoder" / "backbone"
    for pkg in ("refsrc", "refsrc.backbone", "refsrc.backbone.unimatch"):
        mod = types.ModuleType(pkg)
        mod.__path__ = []
        sys.modules[pkg] = mod
    out = None
    for name, rel in (("refsrc.backbone.unimatch.position", "unimatch/position.py"), ("refsrc.backbone.unimatch.utils", "unimatch/utils.py"),
                      ("refsrc.backbone.multiview_transformer", "multiview_transformer.py")):
        spec = importlib.util.spec_from_file_location(name, base / rel)
        out = importlib.util.module_from_spec(spec)
        sys.modules[name] = out
        spec.loader.exec_module(out)
    return out


def main(ref_root: str) -> None:
    ref = load_reference(ref_root)
    out = {}
    for seed, (case, (b, m, h, w, k, shift, full)) in enumerate(CASES.items()):
        q, kk, v, g = R.random_case(b, m, h, w, c=C, scale=1.5, seed=100 + seed)
        mask = None
        if k > 1:
            wh, ww = h // k, w // k
            mask = ref.generate_shift_window_attn_mask((h, w), wh, ww, wh // 2, ww // 2, device=torch.device("cpu"))
            out[f"{case}_mask"] = mask.numpy()
        for tag, dtype in (("64", torch.float64), ("32", torch.float32)):
            def fn(a, bb, cc):
                if full:
                    return ref.single_head_full_attention(a, bb, cc)
                return ref.single_head_split_window_attention(a, bb, cc, num_splits=k, with_shift=bool(shift), h=h, w=w,
                                                              attn_mask=None if mask is None else mask.to(dtype))
            res = R.gradients(fn, q, kk, v, g, dtype)
            for name, t in zip(("out", "gq", "gk", "gv"), res):
                out[f"{case}_{name}{tag}"] = t.numpy()
        for name, t in zip(("q", "k", "v", "g"), (q, kk, v, g)):
            out[f"{case}_{name}"] = t.numpy()
        out[f"{case}_meta"] = np.array([b, m, h, w, k, shift, full], dtype=np.int64)
        # the maker's own check: the float64 statement is the reference, to rounding
        want = R.statement(q, kk, v, k, bool(shift), h, w, "reference")
        err = (want - torch.from_numpy(out[f"{case}_out64"])).abs().max().item()
        assert err <= 1e-13, (case, err)
    dst = HERE / "window_attention.npz"
    np.savez_compressed(dst, **out)
    print(dst, dst.stat().st_size, "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else ".")
