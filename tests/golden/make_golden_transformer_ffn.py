"""Records tests/golden/transformer_ffn.npz from the reference's own TransformerLayer
(src/model/encoder/backbone/multiview_transformer.py:292-414), on CPU.  Run on a machine that has the reference checkout:

    python tests/golden/make_golden_transformer_ffn.py /path/to/splatter360

unimatch/position.py, unimatch/utils.py and multiview_transformer.py are loaded by file path under stub parent packages
(make_golden_window_attention.load_reference), so no package __init__ of the reference runs; besides torch they need einops only.
The layer is built with d_model = 32, nhead = 1, ffn_dim_expansion = 1 and called with attn_type="full" on source, target [B, L, 32].

Recorded per case (prefix = case name, see CASES):
  <case>_source, _target, _g   inputs and output gradient as int16 numerators k of the float32 values k / 64
  <case>_p_<key>               every parameter by its state_dict key, the same way (norm weights are 1 + k / 64); zero_norm is the
                               ffn case's layer with norm2's weight and bias zero and stores those two only
  <case>_out64, _g_source64, _g_target64, _g_<key>64
                               the reference's output and autograd gradients on inputs and parameters cast to float64.  The
                               gradients of q_proj, k_proj and v_proj.weight are NOT stored: with them the file does not stay under
                               128 KB, and g_source / g_target run through all three
  <case>_out32d, ...           the float32 run, as the int32 distance in float32 steps from float32(the float64 value)
  <case>_cfg                   (B, L, C, ffn_dim_expansion, no_ffn) int64
Data only.
"""
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE))

import group_norm_reference as G  # noqa: E402
import transformer_ffn_reference as R  # noqa: E402
from make_golden_qkv_attention import steps32  # noqa: E402
from make_golden_window_attention import load_reference  # noqa: E402

C, EXPANSION = 32, 1
# name: (B, L, no_ffn, norm2 zeroed)
CASES = {"ffn": (2, 5, False, False), "no_ffn": (2, 5, True, False), "zero_norm": (2, 5, False, True)}
NOT_STORED = ("q_proj.weight", "k_proj.weight", "v_proj.weight")


def numerators(x):
    k = np.round(np.asarray(x, dtype=np.float64) * 64)
    assert np.array_equal(k / 64, np.asarray(x, dtype=np.float64)) and np.abs(k).max() < 32768
    return k.astype(np.int16)


def main(ref_root: str) -> None:
    ref = load_reference(ref_root)
    out = {}
    for seed, (case, (b, l, no_ffn, zero_norm)) in enumerate(CASES.items()):
        layer = ref.TransformerLayer(d_model=C, nhead=1, attention_type="swin", no_ffn=no_ffn, ffn_dim_expansion=EXPANSION)
        keys = [k for k, _ in layer.named_parameters()]
        assert tuple(keys) == R.layer_params(no_ffn)
        with torch.no_grad():
            for i, (key, p) in enumerate(layer.named_parameters()):
                pseed = 1000 * (1 if zero_norm else seed + 1) + i                     # zero_norm: the ffn case's layer but for norm2
                val = G.lattice(tuple(p.shape), pseed, scale=1.0 / 16.0, span=7) if p.dim() == 2 else G.lattice(tuple(p.shape), pseed, span=63)
                if key.startswith("norm2") and zero_norm:
                    val = np.zeros_like(val)
                elif key.endswith("norm1.weight") or key.endswith("norm2.weight"):
                    val = val + 1.0
                p.copy_(torch.from_numpy(val))
        source, target, g = (torch.from_numpy(G.lattice((b, l, C), 900 + 10 * seed + i, span=255)) for i in range(3))
        runs = {}
        for dtype in (torch.float32, torch.float64):
            lay = layer.to(dtype)
            lay.zero_grad(set_to_none=True)
            s, t = (x.detach().clone().to(dtype).requires_grad_(True) for x in (source, target))
            o = lay(s, t, attn_type="full")
            o.backward(g.to(dtype))
            runs[dtype] = {"out": o.detach().numpy(), "g_source": s.grad.numpy(), "g_target": t.grad.numpy(),
                           **{"g_" + k: p.grad.numpy().copy() for k, p in lay.named_parameters()}}
        layer.to(torch.float32)
        for name, x in (("source", source), ("target", target), ("g", g)):
            out[f"{case}_{name}"] = numerators(x.numpy())
        params = {k: p.detach().clone() for k, p in layer.named_parameters()}
        for k, p in params.items():
            if zero_norm and not k.startswith("norm2"):
                assert np.array_equal(out[f"ffn_p_{k}"], numerators(p.numpy()))           # stored once, under the ffn case
            else:
                out[f"{case}_p_{k}"] = numerators(p.numpy())
        for name, v64 in runs[torch.float64].items():
            if name[2:] in NOT_STORED:
                continue
            out[f"{case}_{name}64"] = v64
            out[f"{case}_{name}32d"] = steps32(runs[torch.float32][name], v64)
        out[f"{case}_cfg"] = np.array([b, l, C, EXPANSION, int(no_ffn)], dtype=np.int64)
        # the maker's own check: the float64 statement is the reference, to rounding
        want = R.layer_statement(params, source, target, no_ffn)
        err = (want - torch.from_numpy(runs[torch.float64]["out"])).abs().max().item()
        assert err <= 1e-13 * max(1.0, want.abs().max().item()), (case, err)
    dst = HERE / "transformer_ffn.npz"
    np.savez_compressed(dst, **out)
    print(dst, dst.stat().st_size, "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else ".")
