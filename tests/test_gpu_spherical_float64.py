"""The native equirectangular splat mode (S360_FLAG_SPHERICAL) against float64, per (view, Gaussian) pair and per Gaussian: what
tests/test_gpu_backward_float64.py does for the cube faces, for geo_sph, its pole clamp, the seam ghost and the two-pairs-per-
Gaussian sum.  tests/test_gpu_spherical.py judges each gradient tensor by max |err| / max |want|, where a pole Gaussian's gradient
is a tiny fraction of the largest: a wrong sign in the clamped branch, a ghost pair added into the wrong Gaussian or a wrong
image_of_view index would pass there.

One panorama is the oracle's NP = 2P pairs (main pairs, then ghosts) = the kernels' views 2i / 2i + 1.  Units: 2^-24 of the
element's condition (sum of |terms|); bar: kernel <= 2 x the float32 oracle on the same input, worst and mean.  The scenes, the
groups and the usability of the yardstick are pinned on the CPU by tests/test_oracle_spherical_parts.py.

TEST A, the composite, per pair: the records of s360_backward_pair_records against the float64 oracle's raster gradients for every
visible pair, main and ghost, in the modes parity / default / atomic; the seed is zero on the pixels whose float64 decision margin
is below 1e-4, and on every other pixel the kernels' last contributor is the float64 oracle's.  Stats per pair group — pole (float64
rho < 0.05 r) | ghost (views 2i + 1) | plain — and record group, so that the pole's loose yardstick (the centre's column is
atan2(t0, t2): roundings amplified by r / rho, which the *_abs sums do not see) never loosens the bar of the others.  Scenes:
32 x 64 and 48 x 96 with planted poles (rho / r in 0.003 .. 0.2, both sides of the clamp, both poles) and seam Gaussians, one call
with TWO panoramas at different poses (V = 4), and 80 x 160 with two pairs over 32 tiles.

TEST A', the forward state per pair, on the same calls: centre, depth, conic (through the pre-scale constants of
test_gpu_parity.check_forward), radii, clamp bits — and, on the upstream-compatible lists, the sorted list and its keys — bit-equal to
the float32 oracle; rgb within 2e-6; final_T within 1e-5 where the last contributor agrees.

TEST B, the chain, per Gaussian: the kernels' OWN records through the float64 spherical chain (SphereOracles.chain: condition D
summed over both pairs separately).  Every Gaussian counts, outputs start as NaN, an element whose D is 0 must be exactly 0
(invisible Gaussians, SH beyond the degree, the lower triangle with cov9).  P = 209 and 270; SH degree 4 with d_shs wanted and with
harmonics frozen; colors_precomp; cov9 and cov6; one panorama and two.  The depth-record word (9) is not produced in this mode: the
fused depth channel is cube-face only.  The pole Gaussians are also reported on their own.

Out of scope: pole pairs with rho / r < 0.003 (the float32 yardstick breaks down: 15 000 .. 28 000 units at 0.001, 1e8 on the axis);
a Gaussian exactly on the axis gets a finiteness check.  d2inv == 0 (an overflowing det^2), as in the cube test.

Measured on an MI355X (kernel / float32 oracle, units of 2^-24; worst, mean; also profiles/spherical_raw_float64_accuracy.json):
  composite, per pair [sph64]: scene/mode/group, then per record group
  p32/atomic/ghost       conic 978.2/1034.2 56.79/56.41  opacity 641.6/720.2 39.89/40.25  rgb 296.5/298.0 46.49/46.44  xy 966.0/1021.6 52.58/52.32
  p32/atomic/plain       conic 136.3/139.5 18.88/18.89  opacity 101.2/102.2 10.00/10.03  rgb 136.2/136.2 13.68/13.68  xy 223.9/223.2 16.27/16.25
  p32/atomic/pole        conic 2725.3/2727.9 265.96/266.08  opacity 2335.9/2336.0 159.75/158.97  rgb 1965.2/1965.8 205.99/206.13  xy 2279.3/2279.1 240.71/240.70
  p32/default/ghost      conic 978.2/1034.2 56.79/56.41  opacity 641.6/720.2 39.90/40.25  rgb 296.5/298.0 46.49/46.44  xy 966.0/1021.6 52.58/52.32
  p32/default/plain      conic 136.3/139.5 18.88/18.89  opacity 100.8/102.2 10.00/10.03  rgb 136.2/136.2 13.68/13.68  xy 223.9/223.2 16.28/16.25
  p32/default/pole       conic 2725.3/2727.9 265.96/266.08  opacity 2335.9/2336.0 159.74/158.97  rgb 1965.2/1965.8 205.99/206.13  xy 2279.3/2279.1 240.71/240.70
  p32/parity/ghost       conic 978.2/1034.2 46.72/46.41  opacity 641.6/720.2 32.82/33.11  rgb 296.5/298.0 38.25/38.20  xy 966.0/1021.6 43.26/43.05
  p32/parity/plain       conic 136.3/139.5 18.88/18.89  opacity 100.8/102.2 10.00/10.03  rgb 136.2/136.2 13.68/13.68  xy 223.9/223.2 16.28/16.25
  p32/parity/pole        conic 2725.3/2727.9 260.05/260.17  opacity 2335.9/2336.0 156.19/155.44  rgb 1965.2/1965.8 201.42/201.55  xy 2279.3/2279.1 235.36/235.35
  p48/atomic/ghost       conic 334.6/343.8 47.68/48.01  opacity 302.3/311.8 35.37/35.01  rgb 316.6/324.0 44.68/45.11  xy 313.2/324.9 43.79/44.33
  p48/atomic/plain       conic 206.1/204.6 24.33/24.33  opacity 179.0/176.9 13.10/13.09  rgb 141.1/142.4 18.64/18.68  xy 244.3/247.4 20.94/20.79
  p48/atomic/pole        conic 4118.8/4119.1 283.86/284.35  opacity 3521.1/3518.9 185.00/184.96  rgb 3271.2/3271.2 225.57/225.57  xy 3119.2/3120.3 234.17/233.41
  p48/default/ghost      conic 334.6/343.8 47.68/48.01  opacity 302.3/311.8 35.37/35.01  rgb 316.6/324.0 44.68/45.11  xy 313.2/324.9 43.80/44.33
  p48/default/plain      conic 206.1/204.6 24.32/24.33  opacity 179.0/176.9 13.10/13.09  rgb 141.1/142.4 18.64/18.68  xy 244.3/247.4 20.94/20.79
  p48/default/pole       conic 4118.8/4119.1 283.88/284.35  opacity 3521.1/3518.9 184.99/184.96  rgb 3271.2/3271.2 225.60/225.57  xy 3119.2/3120.3 234.17/233.41
  p48/parity/ghost       conic 334.6/343.8 40.33/40.60  opacity 302.3/311.8 29.91/29.61  rgb 316.6/324.0 37.79/38.15  xy 313.2/324.9 37.04/37.49
  p48/parity/plain       conic 206.1/204.6 24.32/24.33  opacity 179.0/176.9 13.10/13.09  rgb 141.1/142.4 18.64/18.68  xy 244.3/247.4 20.94/20.79
  p48/parity/pole        conic 4118.8/4119.1 283.88/284.35  opacity 3521.1/3518.9 184.99/184.96  rgb 3271.2/3271.2 225.60/225.57  xy 3119.2/3120.3 234.17/233.41
  two/atomic/ghost       conic 654.3/662.7 50.98/50.99  opacity 249.0/247.8 30.81/31.06  rgb 288.8/288.8 44.62/44.73  xy 354.3/352.7 43.43/43.93
  two/atomic/plain       conic 136.3/139.5 19.18/19.08  opacity 150.2/142.1 10.49/10.49  rgb 146.2/146.2 14.69/14.72  xy 223.9/223.2 16.34/16.25
  two/atomic/pole        conic 4215.0/4211.2 264.79/264.84  opacity 964.7/966.7 99.30/98.74  rgb 1758.8/1756.4 177.87/177.74  xy 4474.0/4468.7 233.97/234.15
  two/default/ghost      conic 654.3/662.7 50.98/50.99  opacity 249.0/247.8 30.80/31.06  rgb 288.8/288.8 44.62/44.73  xy 354.3/352.7 43.43/43.93
  two/default/plain      conic 136.3/139.5 19.17/19.08  opacity 150.5/142.1 10.48/10.49  rgb 146.2/146.2 14.70/14.72  xy 223.9/223.2 16.34/16.25
  two/default/pole       conic 4215.0/4211.2 264.78/264.84  opacity 964.7/966.7 99.30/98.74  rgb 1758.8/1756.4 177.87/177.74  xy 4474.0/4468.7 233.98/234.15
  two/parity/ghost       conic 654.3/662.7 41.61/41.62  opacity 249.0/247.8 25.14/25.35  rgb 288.8/288.8 36.42/36.51  xy 354.3/352.7 35.45/35.85
  two/parity/plain       conic 136.3/139.5 19.17/19.08  opacity 150.5/142.1 10.48/10.49  rgb 146.2/146.2 14.70/14.72  xy 223.9/223.2 16.34/16.25
  two/parity/pole        conic 4215.0/4211.2 264.78/264.84  opacity 964.7/966.7 99.30/98.74  rgb 1758.8/1756.4 177.87/177.74  xy 4474.0/4468.7 233.98/234.15
  wide/atomic/ghost      conic 1499.7/1505.0 60.86/61.50  opacity 177.4/182.4 20.45/21.04  rgb 186.4/184.0 28.54/28.53  xy 299.1/304.3 30.42/30.92
  wide/atomic/plain      conic 473.7/473.1 18.64/18.69  opacity 112.4/111.1 9.63/9.68  rgb 145.3/144.4 13.89/13.98  xy 209.0/208.4 15.13/15.18
  wide/atomic/pole       conic 164.1/164.1 41.69/41.34  opacity 370.3/369.2 46.79/46.78  rgb 248.6/248.6 46.72/46.84  xy 324.7/324.7 55.52/55.71
  wide/default/ghost     conic 1499.7/1505.0 60.88/61.50  opacity 177.4/182.4 20.44/21.04  rgb 186.4/184.0 28.52/28.53  xy 299.1/304.3 30.42/30.92
  wide/default/plain     conic 473.7/473.1 18.65/18.69  opacity 112.4/111.1 9.63/9.68  rgb 145.3/144.4 13.88/13.98  xy 209.0/208.4 15.13/15.18
  wide/default/pole      conic 164.1/164.1 41.62/41.34  opacity 370.3/369.2 46.65/46.78  rgb 248.6/248.6 46.83/46.84  xy 324.7/324.7 55.50/55.71
  wide/parity/ghost      conic 1499.7/1505.0 52.76/53.30  opacity 177.4/182.4 17.72/18.23  rgb 186.4/184.0 24.72/24.73  xy 299.1/304.3 26.37/26.80
  wide/parity/plain      conic 473.7/473.1 18.65/18.69  opacity 112.4/111.1 9.63/9.68  rgb 145.3/144.4 13.88/13.98  xy 209.0/208.4 15.13/15.18
  wide/parity/pole       conic 164.1/164.1 41.62/41.34  opacity 370.3/369.2 46.65/46.78  rgb 248.6/248.6 46.83/46.84  xy 324.7/324.7 55.50/55.71
  chain, per Gaussian [sph64]
  colours/one/P209           cov 891.1/891.1 14.26/14.17  means 238.1/238.1 5.46/5.49  | poles: cov 891.1/891.1  means 238.1/238.1
  colours/one/P270           cov 169.0/169.0 7.44/7.40  means 175.8/175.8 3.54/3.56  | poles: cov 169.0/169.0  means 175.8/175.8
  frozen/one/P209            cov 683.7/683.7 12.42/12.38  means 262.7/262.7 5.90/5.82  | poles: cov 683.7/683.7  means 262.7/262.7
  frozen/one/P270            cov 156.2/156.2 7.30/7.29  means 187.5/187.5 3.69/3.62  | poles: cov 156.2/156.2  means 187.5/187.5
  frozen/two/P209            cov 186.8/186.8 6.91/6.83  means 292.7/292.7 8.04/8.00  | poles: cov 186.8/186.8  means 292.7/292.7
  frozen/two/P270            cov 109.9/109.9 6.68/6.66  means 131.4/131.4 4.22/4.21  | poles: cov 109.9/109.9  means 131.4/131.4
  full/chm-cov9/one/P209     cov 683.7/683.7 12.42/12.38  means 262.7/262.7 5.90/5.82  sh 1080.4/1080.4 33.26/33.26  | poles: cov 683.7/683.7  means 262.7/262.7  sh 201.4/201.4
  full/chm-cov9/one/P270     cov 156.2/156.2 7.30/7.29  means 187.5/187.5 3.69/3.62  sh 7998.6/7998.6 88.74/88.74  | poles: cov 156.2/156.2  means 187.5/187.5  sh 7998.6/7998.6
  full/chm-cov9/two/P209     cov 186.8/186.8 6.91/6.83  means 292.7/292.7 8.04/8.00  sh 1032.0/1032.0 23.48/23.48  | poles: cov 186.8/186.8  means 292.7/292.7  sh 1032.0/1032.0
  full/chm-cov9/two/P270     cov 109.9/109.9 6.68/6.66  means 131.4/131.4 4.22/4.21  sh 557.1/557.7 19.76/19.71  | poles: cov 109.9/109.9  means 131.4/131.4  sh 92.3/92.3
  full/pm3-cov6/one/P209     cov 683.7/683.7 12.42/12.38  means 262.7/262.7 5.90/5.82  sh 1080.4/1080.4 33.26/33.26  | poles: cov 683.7/683.7  means 262.7/262.7  sh 201.4/201.4
  full/pm3-cov6/one/P270     cov 156.2/156.2 7.30/7.29  means 187.5/187.5 3.69/3.62  sh 7998.6/7998.6 88.74/88.74  | poles: cov 156.2/156.2  means 187.5/187.5  sh 7998.6/7998.6
  full/pm3-cov6/two/P209     cov 186.8/186.8 6.91/6.83  means 292.7/292.7 8.04/8.00  sh 1032.0/1032.0 23.48/23.48  | poles: cov 186.8/186.8  means 292.7/292.7  sh 1032.0/1032.0
  full/pm3-cov6/two/P270     cov 109.9/109.9 6.68/6.66  means 131.4/131.4 4.22/4.21  sh 557.1/557.7 19.76/19.71  | poles: cov 109.9/109.9  means 131.4/131.4  sh 92.3/92.3
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
WHAT = ("tests/test_gpu_spherical_float64.py on an MI355X: the spherical mode's backward against the float64 oracle, per (view, Gaussian) "
        "pair (sph64/pair: the composite's records, by pair group plain / ghost / pole and record group) and per Gaussian (sph64/chain: the "
        "per-Gaussian chain on the kernels' own records; *_pole: the pole-clamped Gaussians alone). Units of 2^-24 of the element's condition; "
        "kernel_* = the HIP kernels, oracle32_* = the float32 oracle on the same input (bound: kernel <= 2 x oracle32, worst and mean).")
MODES = {"parity": dict(lean=None, split_lists=None, atomic_grads=False),     # the parity_lists fixture sets both module switches
         "default": dict(lean=True, split_lists=True, atomic_grads=False),    # the product's switches (spherical calls never split)
         "atomic": dict(lean=True, split_lists=False, atomic_grads=True)}


def _report(key, fig):
    """Keep the case's figures; with S360_ACCURACY_REPORT=<file> in the environment merge them into that file (shared with
    tests/test_gpu_raw_float64.py: how profiles/spherical_raw_float64_accuracy.json is made)."""
    REPORT[key] = fig
    path = os.environ.get("S360_ACCURACY_REPORT")
    if path:
        p = Path(path)
        old = json.loads(p.read_text()) if p.exists() else {}
        p.write_text(json.dumps(dict(what={**old.get("what", {}), "sph64": WHAT}, cases={**old.get("cases", {}), **REPORT}), indent=1, sort_keys=True))


def _t(a, dev):
    return None if a is None else torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _nan(shape, dev):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


def _bound(tag, what, kernel, yard):
    assert np.isfinite(kernel[0]), (tag, what, "an element whose condition is 0 is not exactly 0", kernel)
    assert kernel[0] <= FACTOR * yard[0], (tag, what, "worst", kernel, yard)
    assert kernel[1] <= FACTOR * yard[1], (tag, what, "mean", kernel, yard)


def _fig(kern, yard):
    return dict(kernel_worst=kern[0], kernel_mean=kern[1], oracle32_worst=yard[0], oracle32_mean=yard[1])


def _hip_sph(dev, views, cloud, h, w, deg, seed, *, colors=None, chm=True, cov9=True, frozen=False, mode_kw=None):
    """rasterize_views(spherical=True), then s360_backward through the C ABI into NaN-filled outputs.  -> dict of numpy results in
    canonical layouts (cov [P,6] + the lower triangle apart, sh [P,M,3]) + the forward state."""
    views = views.to(dev)
    V = int(views.shape[0])
    P = cloud["means"].shape[0]
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
    op, col = _t(cloud["opacities"], dev), _t(colors, dev)
    kw = dict(split_lists=False, lean=False) if mode_kw is None else mode_kw
    img, radii = rasterizer.rasterize_views(m, cov, op, sh, col, views=views, image_height=h, image_width=w, sh_degree=deg, shared_campos=V == 2,
                                            cov9=cov9, sh_channel_major=chm, spherical=True, **kw)
    state = rasterizer.last_state()
    prm, lay = state.prm, state.layout
    assert prm.flags & _lib.FLAG_SPHERICAL and bool(prm.flags & _lib.FLAG_SHARED_CAMPOS) == (V == 2) and not state.overflowed()
    assert img.shape == (V // 2, 3, h, w) and radii.shape == (V, P)
    g = _t(seed, dev)
    bws = torch.empty(lay.backward_bytes, dtype=torch.uint8, device=dev)
    d_m3, d_m2, d_cov, d_op = _nan((P, 3), dev), _nan((V, P, 3), dev), _nan(tuple(cov.shape), dev), _nan((P,), dev)
    d_col = None if col is None else _nan((P, 3), dev)
    d_sh = None if (sh is None or frozen) else _nan(tuple(sh.shape), dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(_lib.lib().s360_backward(C.byref(prm), _ptr(views), _ptr(m.detach()), _ptr(cov), _ptr(op), _ptr(sh), _ptr(col), _ptr(state.workspace),
                                        lay.total_bytes, _ptr(g), None, None, 0, _ptr(d_m3), _ptr(d_m2), _ptr(d_cov), _ptr(d_op), _ptr(d_sh),
                                        _ptr(d_col), _ptr(bws), lay.backward_bytes, stream), "s360_backward")
    torch.cuda.synchronize()
    off = C.c_size_t()
    _lib.check(_lib.lib().s360_backward_pair_records(C.byref(prm), _ptr(bws), bws.numel(), C.byref(off)), "s360_backward_pair_records")
    assert (bws.data_ptr() + off.value) % 256 == 0 and off.value + V * P * 48 <= bws.numel()
    rec = bws[off.value:off.value + V * P * 48].view(torch.float32).view(V, P, 12).cpu().numpy()
    t = {k: v.cpu().numpy() for k, v in state.tensors().items()}
    vbits = t["vis_mask"].astype(np.int64)
    vis = np.stack([(vbits >> v) & 1 for v in range(V)]).astype(bool)
    cb = t["clamped"].astype(np.int64)
    out = dict(state=state, t=t, vis=vis, clamped=np.stack([(cb >> k) & 1 for k in range(3)], -1).astype(bool), image=img.detach().cpu().numpy(),
               rec=np.where(vis[:, :, None], rec, np.float32(0)),            # culled pairs: never written, never read
               means=d_m3.cpu().numpy(), means2D=d_m2.cpu().numpy(), opac=d_op.cpu().numpy(), radii=radii.cpu().numpy())
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
    return out


def _last_contributor_hip(hs, i, h, w, P):
    """Panorama i: the oracle's pair id (Gaussian g: main g, ghost P + g) of each pixel's last contributor, and its tile ranges.  The
    kernels' list holds view x P + g with the views 2i (main) and 2i + 1 (ghost)."""
    t = hs["t"]
    T = ((w + 15) // 16) * ((h + 15) // 16)
    ts = t["tile_start"].astype(np.int64)[i * T:(i + 1) * T + 1]
    lst = t["list"].astype(np.int64) & 0xFFFFFFFF
    ranges = np.stack([ts[:-1], ts[1:]], 1)
    last = br.last_contributor(t["n_contrib"][i], ranges, lst, h, w)
    assert ((last < 0) | ((last >= 2 * i * P) & (last < (2 * i + 2) * P))).all(), "a list entry of another panorama"
    return np.where(last >= 0, last - 2 * i * P, -1), ranges


# ================================================================================= TESTS A and A': the composite and the forward, per pair
def _check_forward_state(tag, sc, hs, mode):
    """A': per visible pair against the FLOAT32 oracle (the bars of test_gpu_parity.check_forward)."""
    so32, P, h, w = sc["so32"], sc["P"], sc["h"], sc["w"]
    t, vis_hip = hs["t"], hs["vis"]
    kd, ko = np.float32(-0.5 * 1.4426950408889634), np.float32(-1.4426950408889634)
    T = ((w + 15) // 16) * ((h + 15) // 16)
    for i in range(sc["n"]):
        f = so32.fwd[i]
        np.testing.assert_array_equal(br.pair_rows(hs["radii"], i), f["radii"])
        vis = br.pair_rows(vis_hip, i)
        assert not (vis & ~(f["radii"] > 0)).any() and (mode != "parity" or np.array_equal(vis, f["radii"] > 0))
        ra, rb, rc = (br.pair_rows(t[k], i)[vis] for k in ("rec_a", "rec_b", "rec_c"))
        np.testing.assert_array_equal(ra[:, :2], f["xy"][vis])
        np.testing.assert_array_equal(br.pair_rows(t["depths"], i)[vis], f["depth"][vis])
        np.testing.assert_array_equal(rc[:, 1].copy().view(np.int32), f["radii"][vis])
        co = f["conic_opacity"][vis]
        np.testing.assert_array_equal(ra[:, 2], co[:, 0] * kd)
        np.testing.assert_array_equal(ra[:, 3], co[:, 1] * ko)
        np.testing.assert_array_equal(rb[:, 0], co[:, 2] * kd)
        np.testing.assert_array_equal(br.pair_rows(hs["clamped"], i)[vis], f["clamped"].astype(bool)[vis])
        rgb = np.stack([rb[:, 2], rb[:, 3], rc[:, 0]], 1)
        np.testing.assert_allclose(rgb, f["rgb"][vis], rtol=0, atol=2e-6)
        ts = t["tile_start"].astype(np.int64)[i * T:(i + 1) * T + 1]
        if mode == "parity":                                  # upstream's rectangles: the very list and keys of the oracle
            L = int(f["num_rendered"])
            assert ts[-1] - ts[0] == L
            np.testing.assert_array_equal(t["list"][ts[0]:ts[-1]].astype(np.int64) - 2 * i * P, f["values"].astype(np.int64))
            tile_of = np.repeat(np.arange(T, dtype=np.uint64), np.diff(ts))
            keys_up = (tile_of << np.uint64(32)) | (t["keys"][ts[0]:ts[-1]].view(np.uint64) >> np.uint64(32))
            np.testing.assert_array_equal(keys_up, f["keys"])
        last_hip, _ = _last_contributor_hip(hs, i, h, w, P)
        same = last_hip == br.last_contributor(f["n_contrib"], f["ranges"], f["values"], h, w)
        assert same.mean() >= 0.998, (tag, i, same.mean())
        np.testing.assert_allclose(t["final_T"][i][same], f["final_T"][same], rtol=0, atol=1e-5)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(br.SPH_SCENES))
def test_composite_records_and_forward_state_per_pair(gpu, request, name, mode):
    if mode == "parity":
        request.getfixturevalue("parity_lists")
    sc = br.sph_scene(name)
    so64, P, n, h, w = sc["so64"], sc["P"], sc["n"], sc["h"], sc["w"]
    hs = _hip_sph(gpu, sc["views"], sc["cloud"], h, w, 4, sc["seed"], mode_kw=MODES[mode])
    state = hs["state"]
    prm = state.prm
    assert bool(prm.flags & _lib.FLAG_ATOMIC_GRADS) == (mode == "atomic") and bool(prm.flags & _lib.FLAG_LEAN_LISTS) == (mode != "parity")
    assert not (prm.flags & _lib.FLAG_SPLIT_LISTS) and state.split_errors() == 0
    tag = f"{name}/{mode}"
    _check_forward_state(tag, sc, hs, mode)
    if name == "wide" and mode != "atomic":
        assert int(hs["t"]["header"][4]) >= 2, hs["t"]["header"][:8]     # pairs with more than 32 slots: the wave-parallel sum of k_gather_slots

    flat = lambda a: a.reshape(-1, a.shape[-1])
    vis64 = np.stack([br.pair_rows(so64.visible, i) for i in range(n)])                  # [n,2P]
    vis = np.stack([br.pair_rows(hs["vis"], i) for i in range(n)])
    rec = np.stack([br.pair_rows(hs["rec"], i) for i in range(n)])[..., :9]
    dropped = vis64 & ~vis                      # lean lists: a pair that reaches alpha >= 1/255 on no tile is visible to nothing behind the forward
    assert not (vis & ~vis64).any() and (mode != "parity" or not dropped.any())
    assert (sc["a64"][dropped] == 0).all(), (tag, int(dropped.sum()))
    differ_all = 0
    for i in range(n):
        f = so64.fwd[i]
        last_hip, _ = _last_contributor_hip(hs, i, h, w, P)
        differ = last_hip != br.last_contributor(f["n_contrib"], f["ranges"], f["values"], h, w)
        differ_all += int(differ.sum())
        assert not (differ & ~sc["flagged"][i]).any(), (tag, i, int((differ & ~sc["flagged"][i]).sum()))
    v = vis.reshape(-1)
    group = sc["group"].reshape(-1)[v]
    kern = br.sph_group_stats(br.pair_ratios(flat(rec), flat(sc["r64"]), flat(sc["a64"]), v), group)
    yard = br.sph_group_stats(br.pair_ratios(flat(sc["r32"]), flat(sc["r64"]), flat(sc["a64"]), v), group)
    for g in br.SPH_GROUPS:
        print(f"[sph64] pair {tag}/{g} ({int((group == br.SPH_GROUPS.index(g)).sum())} pairs, last contributor differs on {differ_all} flagged pixels): "
              + "  ".join(f"{k} {kern[g, k][0]:.1f}/{yard[g, k][0]:.1f} {kern[g, k][1]:.2f}/{yard[g, k][1]:.2f}" for k, _ in br.GROUPS))
        _report(f"sph64/pair/{tag}/{g}", {k: _fig(kern[g, k], yard[g, k]) for k, _ in br.GROUPS})
    for key in kern:
        _bound(tag, key, kern[key], yard[key])


# ========================================================================================================= TEST B: the chain, per Gaussian
def _check_chain(tag, s, hs):
    so64, so32 = s["so64"], s["so32"]
    V, P = so64.V, so64.P
    out = br.excluded_sph(so64, hs["vis"], hs["clamped"] if so64.use_sh else np.zeros((V, P, 3), bool))
    assert out.sum() <= 1e-3 * P, (tag, int(out.sum()))
    keep = ~out
    R = hs["rec"]
    want, D = so64.chain(R, want_abs=True)
    yard = so32.chain(R)
    pole = ((so64.rho_over_r() < br.POLE_CLAMP) & (so64.visible[0::2] | so64.visible[1::2])).any(0) & keep
    assert pole.sum() >= 8
    fig = {}
    quantities = ["means", "cov"] + [k for k in ("sh",) if k in hs]
    for k in quantities:
        fig[k] = _fig(br.gaussian_stats(hs[k], want[k], D[k], keep), br.gaussian_stats(yard[k], want[k], D[k], keep))
        fig[k + "_pole"] = _fig(br.gaussian_stats(hs[k], want[k], D[k], pole), br.gaussian_stats(yard[k], want[k], D[k], pole))
    print(f"[sph64] chain {tag} (P {P}, V {V}, left out {int(out.sum())}, poles {int(pole.sum())}): " + "  ".join(
        f"{k} {f['kernel_worst']:.1f}/{f['oracle32_worst']:.1f} {f['kernel_mean']:.2f}/{f['oracle32_mean']:.2f}" for k, f in fig.items()))
    _report(f"sph64/chain/{tag}", fig)
    # derived bars: no yardstick needed.  d_means2D is the centre record itself, per VIEW (exact copies; culled pairs and .z: 0)
    np.testing.assert_array_equal(hs["means2D"][..., :2], R[..., :2])
    assert (hs["means2D"][..., 2] == 0).all() and np.abs(R[..., :2]).max() > 0
    q = br.element_ratios(hs["opac"], want["opac"], D["opac"])[keep]                       # a sum of V terms: V - 1 roundings
    assert q.max() <= V - 1, (tag, "opacity", q.max())
    if "colors" in hs:
        q = br.element_ratios(hs["colors"], want["colors"], D["colors"])[keep]
        assert q.max() <= V - 1, (tag, "colours", q.max())
    if "cov_lower" in hs:
        assert (hs["cov_lower"].view(np.int32) == 0).all(), (tag, "lower triangle")         # +0 in every word
    for k in quantities:                                       # the *_pole figures are a report: the poles are inside the bound over all
        _bound(tag, k, (fig[k]["kernel_worst"], fig[k]["kernel_mean"]), (fig[k]["oracle32_worst"], fig[k]["oracle32_mean"]))
    return fig


def _chain_case(gpu, p, kind, *, colors=False, **kw):
    s = br.sph_chain_setup(p, 25, 4, kind, colors)
    so64 = s["so64"]
    seed = np.random.default_rng(7).standard_normal((so64.n, 3, s["h"], s["w"])).astype(np.float32)
    hs = _hip_sph(gpu, s["views"], s["cloud"], s["h"], s["w"], 4, seed, colors=s["colors"], **kw)
    np.testing.assert_array_equal(hs["vis"], so64.visible)          # upstream's rectangles: the vis_mask bit is the oracle's radii > 0
    assert (hs["vis"][0::2] & hs["vis"][1::2]).sum() >= 6
    return s, hs


SH_LAYOUTS = [("chm-cov9", dict(chm=True, cov9=True)), ("pm3-cov6", dict(chm=False, cov9=False))]


@pytest.mark.parametrize("kind", ["one", "two"])
@pytest.mark.parametrize("p", br.CHAIN_P)
@pytest.mark.parametrize("tag,kw", SH_LAYOUTS)
def test_chain_with_harmonics_wanted(gpu, p, tag, kw, kind):
    """SH degree 4, d_shs wanted; one panorama (shared centre: the fused k_gaussians_bwd_sh) and the two-panorama call (per-view SH
    pass), both SH and both covariance layouts.  Invisible Gaussians (one panorama: role 0) must hold exactly 0 everywhere."""
    s, hs = _chain_case(gpu, p, kind, **kw)
    fig = _check_chain(f"full/{tag}/{kind}/P{p}", s, hs)
    assert "sh" in fig
    nowhere = ~s["so64"].visible.any(0)
    assert kind == "two" or nowhere.sum() >= (p - 18) // 8
    for k in ("means", "cov", "opac", "sh"):
        assert (hs[k][nowhere] == 0).all(), k


@pytest.mark.parametrize("kind", ["one", "two"])
@pytest.mark.parametrize("p", br.CHAIN_P)
def test_chain_frozen_harmonics(gpu, p, kind):
    """d_shs == NULL: dL/dmean still carries the view-direction term (the float64 reference always computes it)."""
    s, hs = _chain_case(gpu, p, kind, frozen=True)
    assert "sh" not in _check_chain(f"frozen/{kind}/P{p}", s, hs)


@pytest.mark.parametrize("p", br.CHAIN_P)
def test_chain_precomputed_colours(gpu, p):
    s, hs = _chain_case(gpu, p, "one", colors=True, cov9=False)
    assert "colors" in hs
    _check_chain(f"colours/one/P{p}", s, hs)


def test_a_gaussian_on_the_axis_gives_finite_images_and_gradients(gpu):
    """rho = 0 exactly (identity pose, x = z = 0), at both poles: no accuracy bound — the float32 yardstick does not exist there —
    but nothing may be NaN or inf, in the image or in any gradient."""
    from splatter360_amd import synthetic
    cloud = synthetic.uniform_cloud(64, seed=5, extent=2.0, scale_range=(0.05, 0.3))
    cloud["means"][0], cloud["means"][1] = (0.0, 1.7, 0.0), (0.0, -2.2, 0.0)
    views = br.sph_views([np.eye(4, dtype=np.float32)])
    seed = np.random.default_rng(2).standard_normal((1, 3, 32, 64)).astype(np.float32)
    hs = _hip_sph(gpu, views, cloud, 32, 64, 4, seed)
    assert hs["vis"][0, :2].all()
    for k in ("image", "means", "cov", "opac", "sh", "means2D"):
        assert np.isfinite(hs[k]).all(), k
    assert np.abs(hs["cov"][:2]).max() > 0
