"""The rasteriser's backward against float64, per (view, Gaussian) pair and per Gaussian.

Every other gradient test of the rasteriser judges a tensor by max |got - want| / max |want|: a Gaussian whose gradient is a
hundredth of the largest may be wrong by 100 % there.  Here each stage of the backward is held to the float64 oracle element by
element, in units of 2^-24 of the sum of the magnitudes of the terms that make the element up (its condition), and the bar is the
float32 oracle's own figure on the same input times 2 — the project's factor for "another operation order plus few-ulp intrinsics".

The seam between the stages is the 48-byte raster-gradient record per pair (s360_backward_pair_records; word order and its
mapping to the oracle: tests/backward_reference.py).

TEST A, the composite (k_order_units, k_render_bwd_em, k_gather_slots or atomics): the records against the float64 oracle's
raster gradients, every visible pair, groups xy / conic / opacity / rgb.  The seed dL/dimage is zero on the pixels whose float64
decision margin is below 1e-4 (there float32 may accept, skip or stop differently: a legitimate O(alpha) difference, which is not
what this test is about); on every other pixel the kernels' last contributor must be the float64 oracle's.  n_contrib is a list
POSITION, and the lean lists drop entries the rectangles keep, so the statement compared is the Gaussian at that position.
Scenes small / dense / wide / split x modes parity (upstream-compatible lists) / default (lean + split) / atomic, and one fused
V = 6 cube call with the depth channel (word 9).

TEST B, the chain (gaussian_bwd inside k_preprocess_bwd<SH, SH_PASS> and k_gaussians_bwd_sh, k_sh_bwd, the packed rows): the
kernels' OWN records go through the float64 oracle's backward_gaussians per view, are folded with scale / scale^2 and get the
depth-value chain in numpy; the condition D of each output element comes from nine unit-record runs.  Every Gaussian counts —
invisible ones, the lower triangle of a [P,3,3] covariance gradient and SH beyond the degree have D = 0 and must be exactly 0.
Output buffers start as NaN, so an element nobody writes fails.

Elsewhere: S360_FLAG_SPHERICAL (geo_sph, the pole clamp, the seam ghost) in tests/test_gpu_spherical_float64.py, the raw-input path
(s360_forward_raw, s360_backward_raw*) in tests/test_gpu_raw_float64.py; both share tests/backward_reference.py with this file.

Measured on an MI355X (kernel / float32 oracle, units of 2^-24; worst, mean):
  composite, per pair [pairgrad64]        group worst kernel/oracle32  mean kernel/oracle32
  cube6_depth/default                    conic 50.5/66.1 2.88/3.10  depth 54.6/68.4 1.61/1.81  opacity 57.1/68.8 1.79/1.84  rgb 57.1/105.7 2.58/2.96  xy 50.8/103.8 2.67/3.03
  dense/atomic                           conic 730.2/767.2 13.13/14.24  opacity 242.0/244.9 8.90/9.90  rgb 308.7/249.8 12.72/14.29  xy 466.3/507.9 13.12/14.45
  dense/default                          conic 730.2/767.2 13.13/14.24  opacity 242.0/244.9 8.90/9.90  rgb 308.7/249.8 12.72/14.29  xy 466.3/507.9 13.11/14.45
  dense/parity                           conic 730.2/767.2 11.80/12.80  opacity 242.0/244.9 8.00/8.90  rgb 308.7/249.8 11.43/12.85  xy 466.3/507.9 11.79/13.00
  small/atomic                           conic 70.8/70.8 12.07/12.20  opacity 56.7/56.0 8.06/8.01  rgb 53.4/54.2 11.64/11.53  xy 48.5/48.0 11.80/11.89
  small/default                          conic 70.8/70.8 12.06/12.20  opacity 56.7/56.0 8.06/8.01  rgb 53.4/54.2 11.64/11.53  xy 48.5/48.0 11.79/11.89
  small/parity                           conic 70.8/70.8 12.06/12.20  opacity 56.7/56.0 8.06/8.01  rgb 53.4/54.2 11.64/11.53  xy 48.5/48.0 11.79/11.89
  split/atomic                           conic 243.6/246.3 10.28/10.07  opacity 22.3/25.5 4.04/3.79  rgb 28.9/30.7 5.73/5.43  xy 78.2/71.8 7.30/7.01
  split/default                          conic 243.0/246.3 10.24/10.07  opacity 30.4/25.5 3.95/3.79  rgb 33.2/30.7 5.51/5.43  xy 75.0/71.8 7.19/7.01
  split/parity                           conic 243.6/246.3 10.29/10.07  opacity 22.3/25.5 4.04/3.79  rgb 28.9/30.7 5.73/5.43  xy 78.2/71.8 7.30/7.01
  wide/atomic                            conic 146.5/148.3 17.52/17.78  opacity 35.2/34.2 7.99/8.05  rgb 83.5/83.2 16.12/16.16  xy 72.0/71.9 15.56/15.53
  wide/default                           conic 146.5/148.3 17.52/17.78  opacity 35.2/34.2 7.99/8.05  rgb 83.5/83.2 16.11/16.16  xy 72.0/71.9 15.57/15.53
  wide/parity                            conic 146.5/148.3 17.52/17.78  opacity 35.2/34.2 7.99/8.05  rgb 83.5/83.2 16.11/16.16  xy 72.0/71.9 15.57/15.53
  chain, per Gaussian [chain64]
  colours/P209                           cov 129.3/129.3 5.24/5.24  means 38.8/38.8 1.79/1.79
  colours/P270                           cov 47.4/47.4 4.66/4.66  means 14.4/14.4 1.85/1.85
  depth0/frozen/P209                     cov 122.3/122.3 5.02/5.02  means 31.9/31.9 1.82/1.77
  depth0/full/P209                       cov 122.3/122.3 5.02/5.02  means 31.9/31.9 1.82/1.77  sh 2938.9/2937.7 38.30/38.39
  depth1/frozen/P209                     cov 214.3/214.3 6.46/6.46  means 31.4/31.4 1.98/1.96
  depth1/full/P209                       cov 214.3/214.3 6.46/6.46  means 31.4/31.4 1.98/1.96  sh 2938.9/2937.7 38.30/38.39
  depth2/frozen/P209                     cov 157.0/157.0 5.50/5.50  means 27.3/27.3 1.95/1.91
  depth2/full/P209                       cov 157.0/157.0 5.50/5.50  means 27.3/27.3 1.95/1.91  sh 2938.9/2937.7 38.30/38.39
  depth3/frozen/P209                     cov 145.8/145.8 6.11/6.11  means 26.2/26.2 1.94/1.89
  depth3/full/P209                       cov 145.8/145.8 6.11/6.11  means 26.2/26.2 1.94/1.89  sh 2938.9/2937.7 38.30/38.39
  frozen/P209                            cov 195.9/195.9 5.71/5.71  means 23.1/23.1 1.95/1.83
  frozen/P270                            cov 81.7/81.7 5.33/5.33  means 16.3/16.3 2.04/1.98
  fused/chm-deg2-M25-cov6/P209           cov 291.9/291.9 5.58/5.58  means 30.1/30.2 1.88/1.83  sh 295.8/297.0 7.17/7.24
  fused/chm-deg2-M25-cov6/P270           cov 135.5/135.5 5.67/5.67  means 30.3/30.3 2.10/2.01  sh 105.0/105.0 4.71/4.64
  fused/chm-deg4-M25-cov9/P209           cov 195.9/195.9 5.71/5.71  means 23.1/23.1 1.95/1.83  sh 2938.9/2937.7 38.30/38.39
  fused/chm-deg4-M25-cov9/P270           cov 81.7/81.7 5.33/5.33  means 16.3/16.3 2.04/1.98  sh 315.2/315.2 19.08/19.07
  fused/pm3-deg3-M16-cov9/P209           cov 183.5/183.5 5.72/5.72  means 31.7/31.6 1.97/1.86  sh 296.8/296.8 9.69/9.71
  fused/pm3-deg3-M16-cov9/P270           cov 96.5/96.5 4.97/4.97  means 28.2/28.2 2.12/2.06  sh 105.3/105.3 9.07/9.11
  fused/pm3-deg4-M25-cov6/P209           cov 195.9/195.9 5.71/5.71  means 23.1/23.1 1.95/1.83  sh 2938.9/2937.7 38.30/38.39
  fused/pm3-deg4-M25-cov6/P270           cov 81.7/81.7 5.33/5.33  means 16.3/16.3 2.04/1.98  sh 315.2/315.2 19.08/19.07
  ranges/P209                            cov 195.9/195.9 5.71/5.71  means 23.1/23.1 1.95/1.83
  ranges/P270                            cov 81.7/81.7 5.33/5.33  means 16.3/16.3 2.04/1.98
  split+sh/P209                          cov 195.9/195.9 5.71/5.71  means 23.1/23.1 1.95/1.83  sh 2938.9/2937.7 38.30/38.39
  split+sh/P270                          cov 81.7/81.7 5.33/5.33  means 16.3/16.3 2.04/1.98  sh 315.2/315.2 19.08/19.07
  two_centres/aligned/P209               cov 417.3/417.3 8.18/8.18  means 57.4/57.4 2.41/2.41  sh 1039.0/1039.0 38.22/38.22
  two_centres/aligned/P270               cov 62.7/62.7 5.66/5.66  means 24.0/24.0 2.39/2.39  sh 618.3/618.3 42.97/42.97
  two_centres/misaligned/P209            cov 417.3/417.3 8.18/8.18  means 57.4/57.4 2.41/2.41  sh 1039.0/1039.0 38.22/38.22
  two_centres/misaligned/P270            cov 62.7/62.7 5.66/5.66  means 24.0/24.0 2.39/2.39  sh 618.3/618.3 42.97/42.97
The chain kernels and the float32 oracle state the same contraction-free formulas: their figures coincide to the digit except where
the fused kernel takes dRGB/dmean from the forward's sh_jac.  The SH worst cases (up to 2900) are the oracle's too: a basis function
near one of its zeros is a difference of monomials, whose rounding does not shrink with it.
"""
import ctypes as C
import json
import os
from pathlib import Path

import numpy as np
import pytest
import torch

import backward_reference as br
from splatter360_amd import _lib, rasterizer

pytestmark = pytest.mark.gpu
FACTOR = 2.0                   # kernel <= FACTOR x float32 oracle, worst and mean; not to be raised
REPORT = {}


WHAT = ("tests/test_gpu_backward_float64.py on an MI355X: each stage of the rasteriser's backward against the float64 oracle, per (view, "
        "Gaussian) pair (pairgrad64: the composite's records) and per Gaussian (chain64: the per-Gaussian chain on the kernels' own records). "
        "Units of 2^-24 of the element's condition (sum of |terms|); kernel_* = the HIP kernels, oracle32_* = the float32 oracle on the same "
        "input (the yardstick; bound: kernel <= 2 x oracle32, worst and mean).")


def _report(key, fig):
    """Keep the case's figures; with S360_ACCURACY_REPORT=<file> in the environment also write all of them there (how
    profiles/backward_float64_accuracy.json is made)."""
    REPORT[key] = fig
    path = os.environ.get("S360_ACCURACY_REPORT")
    if path:
        Path(path).write_text(json.dumps(dict(what=WHAT, cases=REPORT), indent=1, sort_keys=True))


def _t(a, dev):
    return None if a is None else torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _nan(shape, dev):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


def _records(state, bws):
    """[V,P,12] view of the pair records inside the backward workspace, through the accessor."""
    off = C.c_size_t()
    _lib.check(_lib.lib().s360_backward_pair_records(C.byref(state.prm), _ptr(bws), bws.numel(), C.byref(off)), "s360_backward_pair_records")
    p = state.prm
    assert (bws.data_ptr() + off.value) % 256 == 0 and off.value + p.V * p.P * 48 <= bws.numel()
    return bws[off.value:off.value + p.V * p.P * 48].view(torch.float32).view(p.V, p.P, 12)


def _bound(tag, what, kernel, yard):
    """kernel / yard: (worst, mean).  Both figures of the kernel within FACTOR x the yardstick's."""
    assert np.isfinite(kernel[0]), (tag, what, "an element whose condition is 0 is not exactly 0", kernel)
    assert kernel[0] <= FACTOR * yard[0], (tag, what, "worst", kernel, yard)
    assert kernel[1] <= FACTOR * yard[1], (tag, what, "mean", kernel, yard)


# ====================================================================================================== TEST A: the composite, per pair
MODES = {"parity": dict(lean=None, split_lists=None, atomic_grads=False),     # the parity_lists fixture sets both module switches
         "default": dict(lean=True, split_lists=True, atomic_grads=False),    # the product: lean lists, long lists split
         "atomic": dict(lean=True, split_lists=False, atomic_grads=True)}


def _last_contributor_hip(state, v, h, w):
    t = state.tensors()
    gx, gy = (w + 15) // 16, (h + 15) // 16
    ts = t["tile_start"].cpu().numpy().astype(np.int64)[v * gx * gy:(v + 1) * gx * gy + 1]
    lst = t["list"].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    P = state.prm.P
    ranges = np.stack([ts[:-1], ts[1:]], 1)
    last = br.last_contributor(t["n_contrib"][v].cpu().numpy(), ranges, lst, h, w)
    return np.where(last >= 0, last - v * P, -1), np.diff(ranges, axis=1)[:, 0]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(br.SCENES))
def test_composite_records_per_pair(gpu, request, name, mode):
    from test_gpu_split_parity import _Segs
    if mode == "parity":
        request.getfixturevalue("parity_lists")
    sc = br.scene(name)
    h, w, f64 = sc["h"], sc["w"], sc["f64"]
    m = _t(sc["means"], gpu).requires_grad_(True)
    cov, op, sh, col = _t(sc["cov6"], gpu), _t(sc["opac"], gpu), _t(sc["shs"], gpu), _t(sc["colors"], gpu)
    views = sc["views"].to(gpu)
    with _Segs(0):
        _, radii = rasterizer.rasterize_views(m, cov, op, sh, col, views=views, image_height=h, image_width=w, sh_degree=int(sc["S"]["sh_degree"]),
                                              shared_campos=True, **MODES[mode])
    state = rasterizer.last_state()
    prm, lay = state.prm, state.layout
    assert bool(prm.flags & _lib.FLAG_ATOMIC_GRADS) == (mode == "atomic") and bool(prm.flags & _lib.FLAG_SPLIT_LISTS) == (mode == "default")
    assert bool(prm.flags & _lib.FLAG_LEAN_LISTS) == (mode != "parity")
    P = prm.P
    g = _t(sc["seed"][None], gpu)
    bws = torch.empty(lay.backward_bytes, dtype=torch.uint8, device=gpu)
    outs = [_nan((P, 3), gpu), None, _nan((P, 6), gpu), _nan((P,), gpu), None if sh is None else _nan(tuple(sh.shape), gpu),
            None if col is None else _nan((P, 3), gpu)]
    rc = _lib.lib().s360_backward(C.byref(prm), _ptr(views), _ptr(m.detach()), _ptr(cov), _ptr(op), _ptr(sh), _ptr(col), _ptr(state.workspace),
                                  lay.total_bytes, _ptr(g), None, None, 0, *[_ptr(o) for o in outs], _ptr(bws), lay.backward_bytes, _stream(gpu))
    _lib.check(rc, "s360_backward")
    torch.cuda.synchronize()
    rec = _records(state, bws)[0].cpu().numpy()
    hdr = state.header().cpu().numpy()
    assert state.split_errors() == 0 and not state.overflowed()

    # the pairs: radii are upstream's in every list mode; the lean lists bin a pair only where it can reach alpha >= 1/255, and one
    # that reaches it nowhere is visible to nothing behind the forward (vis_mask bit clear: its record is neither written nor
    # read) — the float64 oracle must then hold no term at all for it
    r64, a64 = br.oracle_records(sc["b64"])
    np.testing.assert_array_equal(radii[0].cpu().numpy() > 0, f64["radii"] > 0)
    vis = (state.tensors()["vis_mask"].cpu().numpy() & 1).astype(bool)
    dropped = (f64["radii"] > 0) & ~vis
    assert not (vis & ~(f64["radii"] > 0)).any() and (mode != "parity" or not dropped.any())
    assert (a64[dropped] == 0).all(), (name, mode, int(dropped.sum()))
    # the scene reached its mechanism
    last_hip, lengths = _last_contributor_hip(state, 0, h, w)
    if name == "small":
        assert 0 < lengths.max() <= 64 and lengths.size == 20
    if name == "dense":
        assert lengths.max() > 256 and (f64["final_T"] < 2e-4).any()
    if name == "wide" and mode != "atomic":
        assert int(hdr[4]) >= 8, hdr[:8]                   # pairs with more than 32 slots: the wave-parallel sum of k_gather_slots
    if name == "split":
        assert lengths.max() == 2049
        if mode == "default":
            assert int(hdr[5]) > 0, hdr[:8]                # quadrants that handed their list over

    # decisions: the last contributor of every unflagged pixel is the float64 oracle's
    last64 = br.last_contributor(f64["n_contrib"], f64["ranges"], f64["values"], h, w)
    differ = (last_hip != last64)
    print(f"[pairgrad64] {name}/{mode}: last contributor differs on {int(differ.sum())} pixels, {int((differ & ~sc['flagged']).sum())} unflagged")
    assert not (differ & ~sc["flagged"]).any()

    r32, _ = br.oracle_records(sc["b32"])
    kern = br.group_stats(br.pair_ratios(rec, r64, a64, vis))
    yard = br.group_stats(br.pair_ratios(r32, r64, a64, vis))
    print(f"[pairgrad64] {name}/{mode} ({int(vis.sum())} pairs, {int(dropped.sum())} dropped by the lean lists): " + "  ".join(
        f"{k} {kern[k][0]:.1f}/{yard[k][0]:.1f} {kern[k][1]:.2f}/{yard[k][1]:.2f}" for k in kern))
    _report(f"pairgrad64/{name}/{mode}", {k: dict(kernel_worst=kern[k][0], kernel_mean=kern[k][1], oracle32_worst=yard[k][0], oracle32_mean=yard[k][1])
                                          for k in kern})
    for k in kern:
        _bound(f"{name}/{mode}", k, kern[k], yard[k])


# ============================================================================================ the chain driver (test A's V = 6 case, test B)
DEPTH_NAMES = {0: "depth", 1: "disparity", 2: "relative_disparity", 3: "log"}


def _ranges(p):
    """Three ranges with ragged bounds: none on a multiple of the 256-wide block, the last one short."""
    mid = 257 if p > 257 else 157
    return (0, 100), (100, mid), (mid, p)



def _hip_step(dev, setup, *, path="full", chm=True, cov9=True, depth_mode=None, misalign=False, seed=None, dseed=None):
    """Forward through rasterize_views, then the backward through the C ABI by `path`:
    full: s360_backward with d_shs | frozen: d_shs == NULL | split: s360_backward_split + s360_sh_backward (one group) |
    ranges: s360_backward_composite + s360_backward_gaussians over _ranges(P) into [P,10] + s360_unpack_gradients.
    -> dict of numpy results in canonical layouts (cov [P,6] + the lower triangle apart, sh [P,M,3]).
    Upstream's rectangles (lean=False): the chain kernels are the same in every list mode, and with them the vis_mask bit of a
    pair is the oracle's radii > 0 (the lean lists clear it for a pair that reaches alpha >= 1/255 on no tile)."""
    lib = _lib.lib()
    cloud, views, colors = setup["cloud"], setup["views"].to(dev), setup["colors"]
    V, deg = int(views.shape[0]), setup["deg"]
    P = cloud["means"].shape[0]
    shared = V == 6
    m = _t(cloud["means"], dev).requires_grad_(True)
    cov = _t(cloud["covariances"], dev)
    if not cov9:
        r, c = torch.triu_indices(3, 3)
        cov = cov[:, r, c].contiguous()
    sh = None
    if colors is None:
        sh = _t(cloud["harmonics"], dev)                                    # [P,3,M]
        if not chm:
            sh = sh.transpose(1, 2).contiguous()                            # [P,M,3]
    op = _t(cloud["opacities"], dev)
    col = _t(colors, dev)
    res = rasterizer.rasterize_views(m, cov, op, sh, col, views=views, image_height=br.FACE, image_width=br.FACE, sh_degree=deg,
                                     shared_campos=shared, cov9=cov9, sh_channel_major=chm,
                                     depth_mode=None if depth_mode is None else DEPTH_NAMES[depth_mode], split_lists=False, lean=False)
    state = rasterizer.last_state()
    prm, lay = state.prm, state.layout
    assert bool(prm.flags & _lib.FLAG_SHARED_CAMPOS) == shared and not state.overflowed()
    rng = np.random.default_rng(7)
    g = _t(rng.standard_normal((V, 3, br.FACE, br.FACE)) if seed is None else seed, dev)
    gd = None
    if depth_mode is not None:
        gd = _t(rng.standard_normal((V, br.FACE, br.FACE)) if dseed is None else dseed, dev)
    dm = 0 if depth_mode is None else depth_mode
    bws = torch.empty(lay.backward_bytes, dtype=torch.uint8, device=dev)
    d_m3, d_m2, d_cov, d_op = _nan((P, 3), dev), _nan((V, P, 3), dev), _nan(tuple(cov.shape), dev), _nan((P,), dev)
    d_col = None if col is None else _nan((P, 3), dev)
    d_sh = None if (sh is None or path == "frozen") else _nan(tuple(sh.shape), dev)
    d_rgb = None
    sh_arg = sh
    if misalign:      # both bases one float into a larger tensor: neither is 16-byte aligned (the forward keeps its aligned copy)
        sh_arg = torch.empty(sh.numel() + 1, dtype=torch.float32, device=dev)[1:].view(sh.shape)
        sh_arg.copy_(sh)
        d_sh = torch.full((sh.numel() + 1,), float("nan"), dtype=torch.float32, device=dev)[1:].view(sh.shape)
        assert sh_arg.data_ptr() % 16 == 4 and d_sh.data_ptr() % 16 == 4
    elif sh is not None:
        assert sh.data_ptr() % 16 == 0 and (d_sh is None or d_sh.data_ptr() % 16 == 0)
    st = _stream(dev)
    ws, md = state.workspace, m.detach()
    if path in ("full", "frozen"):
        _lib.check(lib.s360_backward(C.byref(prm), _ptr(views), _ptr(md), _ptr(cov), _ptr(op), _ptr(sh_arg), _ptr(col), _ptr(ws), lay.total_bytes,
                                     _ptr(g), None, _ptr(gd), dm, _ptr(d_m3), _ptr(d_m2), _ptr(d_cov), _ptr(d_op), _ptr(d_sh), _ptr(d_col),
                                     _ptr(bws), lay.backward_bytes, st), "s360_backward")
    elif path == "split":
        d_rgb = _nan((P, 4), dev)
        _lib.check(lib.s360_backward_split(C.byref(prm), _ptr(views), _ptr(md), _ptr(cov), _ptr(op), _ptr(sh), _ptr(ws), lay.total_bytes, _ptr(g),
                                           None, _ptr(gd), dm, _ptr(d_m3), _ptr(d_m2), _ptr(d_cov), _ptr(d_op), _ptr(d_rgb), _ptr(bws),
                                           lay.backward_bytes, st), "s360_backward_split")
        _lib.check(lib.s360_sh_backward(C.byref(prm), 1, _ptr(views), _ptr(md), _ptr(d_rgb), _ptr(d_sh), st), "s360_sh_backward")
    elif path == "ranges":
        d_rgb, packed = _nan((P, 4), dev), _nan((P, 10), dev)
        d_sh = None
        _lib.check(lib.s360_backward_composite(C.byref(prm), _ptr(views), _ptr(ws), lay.total_bytes, _ptr(g), None, _ptr(gd), dm, _ptr(bws),
                                               lay.backward_bytes, st), "s360_backward_composite")
        for lo, hi in _ranges(P):
            _lib.check(lib.s360_backward_gaussians(C.byref(prm), _ptr(views), _ptr(md), _ptr(cov), _ptr(sh), _ptr(ws), lay.total_bytes,
                                                   int(gd is not None), dm, lo, hi - lo, STAMP, _ptr(packed), _ptr(d_m2), _ptr(d_rgb), _ptr(bws),
                                                   lay.backward_bytes, st), "s360_backward_gaussians")
        _lib.check(lib.s360_unpack_gradients(_ptr(packed), P, int(cov9), _ptr(d_m3), _ptr(d_cov), _ptr(d_op), st), "s360_unpack_gradients")
    else:
        raise ValueError(path)
    torch.cuda.synchronize()
    t = state.tensors()
    vbits = t["vis_mask"].cpu().numpy().astype(np.int64)
    vis = np.stack([(vbits >> v) & 1 for v in range(V)]).astype(bool)
    cb = t["clamped"].cpu().numpy().astype(np.int64)
    out = dict(state=state, vis=vis, clamped=np.stack([(cb >> k) & 1 for k in range(3)], -1).astype(bool),
               rec=np.where(vis[:, :, None], _records(state, bws).cpu().numpy(), np.float32(0)),     # culled pairs: never written, never read
               means=d_m3.cpu().numpy(), means2D=d_m2.cpu().numpy(), opac=d_op.cpu().numpy(), radii=res[1].cpu().numpy())
    dc = d_cov.cpu().numpy()
    if cov9:
        r, c = np.triu_indices(3)
        out["cov"], out["cov_lower"] = dc[:, r, c], dc[:, [1, 2, 2], [0, 0, 1]]
    else:
        out["cov"] = dc
    if d_sh is not None:
        out["sh"] = d_sh.cpu().numpy().transpose(0, 2, 1) if chm else d_sh.cpu().numpy()
    if d_col is not None:
        out["colors"] = d_col.cpu().numpy()
    if d_rgb is not None:
        out["rgb_sum"] = d_rgb.cpu().numpy()
    return out


STAMP = 5


def test_composite_records_of_a_fused_cube_call_with_depth(gpu):
    """V = 6, shared camera centre, 32 x 32 faces, the role cloud, the depth channel: all ten words, word 9 against the float64 sum
    of alpha T x dL/ddepth (the oracle's pixel loop carries that one accumulator more)."""
    cs = br.cube_scene()
    s = cs["setup"]
    vo64 = s["vo64"]
    h = _hip_step(gpu, s, path="full", depth_mode=1, seed=cs["seed"], dseed=cs["dseed"])
    np.testing.assert_array_equal(h["vis"], vo64.visible)
    np.testing.assert_array_equal(h["radii"] > 0, vo64.visible)
    fig = {}
    for v in range(6):
        last_hip, _ = _last_contributor_hip(h["state"], v, br.FACE, br.FACE)
        f = vo64.fwd[v]
        last64 = br.last_contributor(f["n_contrib"], f["ranges"], f["values"], br.FACE, br.FACE)
        assert not ((last_hip != last64) & ~cs["flagged"][v]).any(), v
    vis = vo64.visible.reshape(-1)
    flat = lambda a: a.reshape(-1, a.shape[-1])
    qk = br.pair_ratios(flat(h["rec"]), flat(cs["r64"]), flat(cs["a64"]), vis, slice(0, 10))
    qy = br.pair_ratios(flat(cs["r32"]), flat(cs["r64"]), flat(cs["a64"]), vis, slice(0, 10))
    kern, yard = br.group_stats(qk), br.group_stats(qy)
    kern["depth"], yard["depth"] = (float(qk[:, 9].max()), float(qk[:, 9].mean())), (float(qy[:, 9].max()), float(qy[:, 9].mean()))
    assert np.abs(flat(cs["r64"])[vis][:, 9]).max() > 0
    print(f"[pairgrad64] cube6+depth ({int(vis.sum())} pairs): " + "  ".join(
        f"{k} {kern[k][0]:.1f}/{yard[k][0]:.1f} {kern[k][1]:.2f}/{yard[k][1]:.2f}" for k in kern))
    _report("pairgrad64/cube6_depth/default", {k: dict(kernel_worst=kern[k][0], kernel_mean=kern[k][1], oracle32_worst=yard[k][0], oracle32_mean=yard[k][1])
                                               for k in kern})
    for k in kern:
        _bound("cube6+depth", k, kern[k], yard[k])


# ========================================================================================================= TEST B: the chain, per Gaussian
def _check_chain(tag, setup, h, depth_mode=None):
    vo64, vo32 = setup["vo64"], setup["vo32"]
    V, P = vo64.V, vo64.P
    out = br.excluded(vo64, h["vis"], h["clamped"] if vo64.use_sh else np.zeros((V, P, 3), bool))
    assert out.sum() <= 1e-3 * P, (tag, int(out.sum()))
    keep = ~out
    R = h["rec"]
    want, D = vo64.chain(R, depth_mode=depth_mode, want_abs=True)
    yard = vo32.chain(R, depth_mode=depth_mode)
    fig = {}
    quantities = ["means", "cov"] + [k for k in ("sh",) if k in h]
    for k in quantities:
        kern_k, yard_k = br.gaussian_stats(h[k], want[k], D[k], keep), br.gaussian_stats(yard[k], want[k], D[k], keep)
        fig[k] = dict(kernel_worst=kern_k[0], kernel_mean=kern_k[1], oracle32_worst=yard_k[0], oracle32_mean=yard_k[1])
    print(f"[chain64] {tag} (P {P}, V {V}, left out {int(out.sum())}): " + "  ".join(
        f"{k} {f['kernel_worst']:.1f}/{f['oracle32_worst']:.1f} {f['kernel_mean']:.2f}/{f['oracle32_mean']:.2f}" for k, f in fig.items()))
    _report(f"chain64/{tag}", fig)
    # derived bars: no yardstick needed
    vis64 = vo64.visible
    q = br.element_ratios(h["means2D"], want["means2D"], D["means2D"])[:, keep]            # one multiply: 2^-24 |want|; culled pairs and .z: 0
    assert q.max() <= 1.0, (tag, "means2D", q.max())
    assert (np.abs(want["means2D"][..., :2]).max() > 0) and (h["means2D"][..., 2] == 0).all()
    q = br.element_ratios(h["opac"], want["opac"], D["opac"])[keep]                        # a sum of V terms: V - 1 roundings
    assert q.max() <= V - 1, (tag, "opacity", q.max())
    if "colors" in h:
        q = br.element_ratios(h["colors"], want["colors"], D["colors"])[keep]
        assert q.max() <= V - 1, (tag, "colours", q.max())
    if "cov_lower" in h:
        assert (h["cov_lower"].view(np.int32) == 0).all(), (tag, "lower triangle")          # +0 in every word
    if "rgb_sum" in h:
        masked = np.where(vis64[:, :, None] & ~vo64.clamped, R[:, :, 6:9].astype(np.float64), 0.0)
        q = br.element_ratios(h["rgb_sum"][:, :3], masked.sum(0), np.abs(masked).sum(0))[keep]
        assert q.max() <= V - 1, (tag, "rgb_sum", q.max())
        first = np.where(vis64.any(0), vis64.argmax(0), -1)
        stamp = h["rgb_sum"][:, 3].copy().view(np.int32)
        want_w = np.where(first >= 0, STAMP, -1) if h.get("stamped") else first
        np.testing.assert_array_equal(stamp[keep], want_w[keep])
    for k in quantities:
        _bound(tag, k, (fig[k]["kernel_worst"], fig[k]["kernel_mean"]), (fig[k]["oracle32_worst"], fig[k]["oracle32_mean"]))
    return fig


def test_the_role_cloud_reaches_every_role_on_the_gpu(gpu):
    """Each role by the kernels' own visibility and clamp bits; and the seam really is one: the records reproduce the call's
    gradients through the float64 chain (else every Gaussian's ratio would be astronomic), with no Gaussian left out."""
    s = br.chain_setup(br.CHAIN_P[0])
    h = _hip_step(gpu, s, path="full")
    np.testing.assert_array_equal(h["vis"], s["vo64"].visible)
    reached = br.roles_reached(s)
    assert all(n > 0 for n in reached.values()), reached
    n_faces = h["vis"].sum(0)
    assert (n_faces == 0).any() and (n_faces == 1).any() and (n_faces == 2).any() and (n_faces >= 3).any()
    n_cl = (h["clamped"] & h["vis"][:, :, None]).any(0).sum(1)
    assert all((n_cl == n).any() for n in (1, 2, 3))
    assert float(s["vo64"].S[0]["scale"]) == pytest.approx(10.0)


SH_LAYOUTS = [("chm-deg4-M25-cov9", dict(chm=True, cov9=True), 25, 4), ("pm3-deg4-M25-cov6", dict(chm=False, cov9=False), 25, 4),
              ("chm-deg2-M25-cov6", dict(chm=True, cov9=False), 25, 2), ("pm3-deg3-M16-cov9", dict(chm=False, cov9=True), 16, 3)]


@pytest.mark.parametrize("p", br.CHAIN_P)
@pytest.mark.parametrize("tag,kw,m,deg", SH_LAYOUTS)
def test_chain_fused_kernel(gpu, p, tag, kw, m, deg):
    """Path 1: s360_backward, shared centre, dL/dSH wanted -> k_gaussians_bwd_sh; both sh_jac producers (k_sh_eval3_jac at
    channel-major degree 4 / M 25, k_sh_eval otherwise), both SH and both covariance layouts."""
    s = br.chain_setup(p, m, deg)
    fig = _check_chain(f"fused/{tag}/P{p}", s, _hip_step(gpu, s, path="full", **kw))
    assert "sh" in fig


@pytest.mark.parametrize("p", br.CHAIN_P)
def test_chain_frozen_harmonics(gpu, p):
    """Path 2: d_shs == NULL -> k_preprocess_bwd<true, false> alone; dL/dmean still carries the view-direction term (the float64
    reference always computes it)."""
    s = br.chain_setup(p)
    fig = _check_chain(f"frozen/P{p}", s, _hip_step(gpu, s, path="frozen"))
    assert "sh" not in fig


@pytest.mark.parametrize("p", br.CHAIN_P)
def test_chain_split_then_sh_backward(gpu, p):
    """Path 3: s360_backward_split, then s360_sh_backward with one group (k_preprocess_bwd<true, false> + k_sh_bwd)."""
    s = br.chain_setup(p)
    fig = _check_chain(f"split+sh/P{p}", s, _hip_step(gpu, s, path="split"))
    assert "sh" in fig


@pytest.mark.parametrize("p", br.CHAIN_P)
def test_chain_composite_then_gaussian_ranges_packed(gpu, p):
    """Path 4: s360_backward_composite, s360_backward_gaussians over three ragged ranges into [P,10], s360_unpack_gradients."""
    s = br.chain_setup(p)
    h = _hip_step(gpu, s, path="ranges")
    h["stamped"] = True
    _check_chain(f"ranges/P{p}", s, h)


@pytest.mark.parametrize("misalign", [False, True])
@pytest.mark.parametrize("p", br.CHAIN_P)
def test_chain_two_camera_centres(gpu, p, misalign):
    """Path 5: two views with different centres, not shared -> k_preprocess_bwd<true, true>, with shs / d_shs 16-byte aligned (float4
    LDS staging) and both one float off (the scalar staging)."""
    s = br.chain_setup(p, kind="two_centres")
    fig = _check_chain(f"two_centres/{'misaligned' if misalign else 'aligned'}/P{p}", s, _hip_step(gpu, s, path="full", chm=False, cov9=False, misalign=misalign))
    assert "sh" in fig and s["vo64"].visible.any()


@pytest.mark.parametrize("p", br.CHAIN_P)
def test_chain_precomputed_colours(gpu, p):
    """Path 6: colors_precomp -> k_preprocess_bwd<false, false>."""
    s = br.chain_setup(p, colors=True)
    h = _hip_step(gpu, s, path="full", cov9=False)
    assert "colors" in h
    _check_chain(f"colours/P{p}", s, h)


@pytest.mark.parametrize("path", ["full", "frozen"])
@pytest.mark.parametrize("depth_mode", [0, 1, 2, 3])
def test_chain_depth_channel(gpu, depth_mode, path):
    """Path 7: a non-zero dL/ddepth in all four depth modes on paths 1 and 2 (P = 209: the ragged last block of both kernels is
    covered above).  Mode 3 keeps the reference's swapped clamp: its depth column is 0 whenever near < far."""
    s = br.chain_setup(br.CHAIN_P[0])
    h = _hip_step(gpu, s, path=path, depth_mode=depth_mode)
    assert np.abs(h["rec"][..., br.DEPTH_WORD]).max() > 0
    _check_chain(f"depth{depth_mode}/{path}/P{br.CHAIN_P[0]}", s, h, depth_mode=depth_mode)
    if depth_mode != 3:       # the depth column did reach the reference: without it the same records give another dL/dmean
        assert not np.array_equal(s["vo64"].chain(h["rec"])["means"], s["vo64"].chain(h["rec"], depth_mode=depth_mode)["means"])
