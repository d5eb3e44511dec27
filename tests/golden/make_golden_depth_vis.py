"""Records tests/golden/depth_vis.npz from the reference's own depth_map, get_colormap and convert_single_colormap
(src/model/model_wrapper_erp.py:122-133, :88-92, :109-120), prep_image (src/misc/image_io.py:38-54) and apply_color_map /
apply_color_map_to_image (src/visualization/color_map.py), on CPU.  model_wrapper_erp pulls in Lightning and image_io pulls in
skvideo, so their functions are compiled from the source at generation time with `ast`, as make_golden_erp_distance.py does for
change_order_batch; color_map.py is loaded whole with `jaxtyping`, `colorspacious` and `cv2` stubbed, as make_golden.py stubs them.
matplotlib >= 3.9 has no cm.get_cmap, which the reference calls: it is aliased to matplotlib.colormaps.__getitem__ here.  Run on a
machine that has the reference checkout, einops and matplotlib:

    python tests/golden/make_golden_depth_vis.py /path/to/splatter360

Recorded (arrays only), for every map name in `names` (fixed-seed log-uniform depths in [0.3, 12]):
  map_<name>     float32 [h, w]     the input
  idx_<name>     int16 [h, w]       the reference's colour as a row of the turbo table: nearest entry, 256 = black (NaN)
  rgb_<name>     float32 [3, h, w]  the reference's depth_map output — asserted here to BE the table entry at idx_<name> for every
                                    map, and therefore left out for the 256 x 256 map, where it would be most of the file
  q_<name>       float32 [2]        torch.quantile(pos, 0.01), torch.quantile(all, 0.99) on CPU (absent for the no-positive map)
  prep_<k>_in / prep_<k>_out        prep_image: [3, h, w], [h, w], [1, h, w], [4, 3, 9, 7], [4, h, w] float32 in [-0.2, 1.2]
  cmap_x, cmap_<map>                apply_color_map(x, map) for turbo, viridis, inferno; x in [-0.1, 1.1] with NaN, 0, 1, inf
  err_a, err_b, err_out, err_idx    convert_single_colormap(|a - b|.mean(0, keepdim=True)) float32 [3, h, w], and its viridis row
"""
import ast
import importlib.util
import sys
import types
from pathlib import Path

import matplotlib
import numpy as np
import torch
from einops import rearrange, repeat
from matplotlib import cm

OUT = Path(__file__).resolve().parent / "depth_vis.npz"


def _functions(path: Path, names, ns: dict) -> dict:
    tree = ast.parse(path.read_text())
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert len(body) == len(names), [n.name for n in body]
    for fn in body:                                              # the annotations name jaxtyping types
        fn.returns = None
        for a in fn.args.args:
            a.annotation = None
    exec(compile(ast.Module(body=body, type_ignores=[]), str(path.name), "exec"), ns)
    return ns


def _color_map_module(ref_root):
    jt = types.ModuleType("jaxtyping")

    class _Ann:
        def __getitem__(self, item):
            return object

    jt.Float = _Ann()
    sys.modules.setdefault("jaxtyping", jt)
    cs = types.ModuleType("colorspacious")
    cs.cspace_convert = None
    sys.modules.setdefault("colorspacious", cs)
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))      # convert_single_colormap imports it and does not use it
    if not hasattr(cm, "get_cmap"):
        cm.get_cmap = lambda name: matplotlib.colormaps[name]
    spec = importlib.util.spec_from_file_location("ref_color_map", Path(ref_root) / "src" / "visualization" / "color_map.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _nearest(rgb_hw3: np.ndarray, table: np.ndarray) -> np.ndarray:
    """Row of `table` [257, 3] nearest to every pixel; rows 0 .. 255 first, so black maps to 256 only if no colour is as near."""
    d = ((rgb_hw3[..., None, :].astype(np.float64) - table[None, None].astype(np.float64)) ** 2).sum(-1)
    idx = d.argmin(-1)
    return idx.astype(np.int16)


def depth_inputs(rng) -> dict:
    def draw(h, w):
        return np.exp(rng.uniform(np.log(0.3), np.log(12.0), (h, w))).astype(np.float32)

    maps = {"1x1": draw(1, 1), "1x2": draw(1, 2), "16x16": draw(16, 16), "ties": np.round(draw(16, 16), 1).astype(np.float32),
            "const": np.full((8, 8), draw(1, 1)[0, 0], np.float32)}
    neg = -draw(8, 8)
    neg.reshape(-1)[rng.integers(64)] = 0.0
    maps["nopos"] = neg
    nan = draw(16, 16)
    nan.reshape(-1)[rng.integers(256)] = np.nan
    maps["nan"] = nan
    sp = draw(16, 16)
    at = rng.choice(256, 3, replace=False)
    sp.reshape(-1)[at[0]], sp.reshape(-1)[at[1]], sp.reshape(-1)[at[2]] = np.inf, 0.0, -sp.reshape(-1)[at[2]]
    maps["special"] = sp
    z = draw(37, 53)
    z[rng.uniform(size=z.shape) < 0.3] = 0.0
    maps["37x53"] = z
    big = draw(256, 256)
    big[rng.uniform(size=big.shape) < 0.02] = 0.0
    maps["256x256"] = big
    return maps


def midpoint_distance(maps: dict) -> float:
    """The least relative distance of float64 log(v) from the midpoint of two neighbouring float32 values, over every positive
    finite element and the two quantiles of every map: tests/test_depth_vis_spec.py asserts it stays above 1e-12, so that a
    last-bit difference between two float64 logarithms cannot change float32(log(v))."""
    nearest = np.inf
    for d in maps.values():
        t = torch.from_numpy(d)
        v = d[np.isfinite(d) & (d > 0)].astype(np.float64)
        if v.size:
            q = np.array([t[t > 0].quantile(0.01).item(), t.view(-1).quantile(0.99).item()], np.float64)
            v = np.concatenate([v, q[np.isfinite(q) & (q > 0)]])
        L = np.log(v)
        L = L[L != 0]
        f = L.astype(np.float32)
        other = np.nextafter(f, np.where(L > f.astype(np.float64), np.inf, -np.inf).astype(np.float32))
        mid = (f.astype(np.float64) + other.astype(np.float64)) / 2
        nearest = min(nearest, (np.abs(L - mid) / np.abs(L)).min(initial=np.inf))
    return float(nearest)


def main(ref_root: str) -> None:
    ref = Path(ref_root)
    cmod = _color_map_module(ref)
    ns = {"torch": torch, "np": np, "mpl": matplotlib, "cm": cm, "rearrange": rearrange, "repeat": repeat,
          "apply_color_map_to_image": cmod.apply_color_map_to_image}
    _functions(ref / "src" / "model" / "model_wrapper_erp.py", ("get_colormap", "convert_single_colormap", "depth_map"), ns)
    _functions(ref / "src" / "misc" / "image_io.py", ("prep_image",), ns)
    # the seed: the first from 20250 on whose maps keep every logarithm 1e-12 (relative) away from a float32 rounding midpoint;
    # with 70 000 logarithms about one seed in ten does
    for seed in range(20250, 20350):
        rng = np.random.default_rng(seed)
        maps = depth_inputs(rng)
        if midpoint_distance(maps) > 2e-12:
            break
    else:
        raise AssertionError("no seed keeps the logarithms off the float32 midpoints")
    print("seed", seed, "midpoint distance", midpoint_distance(maps))
    out = {"seed": np.array(seed)}
    turbo = np.concatenate([np.asarray(matplotlib.colormaps["turbo"](np.arange(256)))[:, :3], np.zeros((1, 3))]).astype(np.float32)
    viridis = np.concatenate([np.asarray(matplotlib.colormaps["viridis"](np.arange(256)))[:, :3], np.zeros((1, 3))])

    out["names"] = np.array(list(maps))
    for name, d in maps.items():
        t = torch.from_numpy(d.copy())
        rgb = ns["depth_map"](t).numpy()
        assert rgb.dtype == np.float32 and rgb.shape == (3, *d.shape) and np.array_equal(t.numpy(), d, equal_nan=True)
        idx = _nearest(np.moveaxis(rgb, 0, -1), turbo)
        assert np.array_equal(turbo[idx], np.moveaxis(rgb, 0, -1)), name      # the picture IS table rows
        out[f"map_{name}"], out[f"idx_{name}"] = d, idx
        if d.size < 65536:
            out[f"rgb_{name}"] = rgb
        if (d > 0).any():
            out[f"q_{name}"] = np.array([t[t > 0].quantile(0.01).item(), t.view(-1).quantile(0.99).item()], np.float32)
    assert (out["idx_nan"] == 256).all() and (out["idx_const"] == 256).all() and (out["idx_1x1"] == 256).all()
    digits = np.unique((maps["256x256"].view(np.uint32) >> 0) & 1023).size, np.unique((maps["256x256"].view(np.uint32) >> 10) & 2047).size
    assert digits == (1024, 2048), digits                        # every low and middle radix digit of the key occurs

    preps = {"chw": rng.uniform(-0.2, 1.2, (3, 11, 13)), "hw": rng.uniform(-0.2, 1.2, (11, 13)), "1hw": rng.uniform(-0.2, 1.2, (1, 11, 13)),
             "bchw": rng.uniform(-0.2, 1.2, (4, 3, 9, 7)), "4hw": rng.uniform(-0.2, 1.2, (4, 11, 13))}
    for k, v in preps.items():
        v = v.astype(np.float32)
        v.reshape(-1)[:3] = (0.0, 1.0, 0.5)
        res = ns["prep_image"](torch.from_numpy(v))
        assert res.dtype == np.uint8
        out[f"prep_{k}_in"], out[f"prep_{k}_out"] = v, res
    out["prep_names"] = np.array(list(preps))

    x = rng.uniform(-0.1, 1.1, (19, 23)).astype(np.float32)
    x.reshape(-1)[:6] = (np.nan, 0.0, 1.0, np.inf, -np.inf, 0.5)
    out["cmap_x"] = x
    for name in ("turbo", "viridis", "inferno"):
        res = cmod.apply_color_map(torch.from_numpy(x), name).numpy()
        assert res.dtype == np.float32 and res.shape == (19, 23, 3)
        out[f"cmap_{name}"] = res

    a, b = rng.uniform(0, 1, (3, 21, 17)).astype(np.float32), rng.uniform(0, 1, (3, 21, 17)).astype(np.float32)
    a[:, 0, 0], b[:, 0, 0] = 0.0, 0.0                            # zero error
    a[:, 0, 1], b[:, 0, 1] = 2.5, 0.0                            # beyond the norm's range: the last colour
    res = ns["convert_single_colormap"](torch.abs(torch.from_numpy(a) - torch.from_numpy(b)).mean(0, keepdim=True)).numpy()
    assert res.dtype == np.float32 and res.shape == (3, 21, 17)
    vb = (viridis * 255).astype(np.uint8)
    eidx = _nearest(np.moveaxis(res, 0, -1), (vb.astype(np.float32) / np.float32(255)))
    out["err_a"], out["err_b"], out["err_out"], out["err_idx"] = a, b, res, eidx

    np.savez_compressed(OUT, **out)
    print(OUT, OUT.stat().st_size, "bytes")
    assert OUT.stat().st_size < 400 * 1024


if __name__ == "__main__":
    main(sys.argv[1])
