"""The raw-input path (s360_forward_raw: k_raw_eval<.., DEG>; s360_backward_raw / s360_backward_raw_tail: k_raw_bwd<.., DEG>) at SH
degrees 0..3 — d_sh = 1, 4, 9, 16, raw records of 10, 19, 34 and 55 floats — held to what tests/test_gpu_raw_float64.py holds the
degree-4 path to, with that file's measures (tests/test_gpu_adapter_float64.py's _errors), inputs (_inputs) and bound (FACTOR = 2:
the kernels' worst per-Gaussian error <= 2 x the float32 CPU yardstick's worst; no Gaussian left out).  The references are the
degree-general ones of tests/raw_degree_reference.py.

  (a) PER GAUSSIAN  two cases per d_sh — (hm3d, per_ray 1, rotation, differentiable means) and (m3d, per_ray 2, no rotation, detached
      means): means, covariances, d_depths, d_raw scale / quat / SH (per colour and degree block), clamped colours and clamp bits;
      every output of s360_backward_raw NaN-filled between guards.  d_sh = 1: sh_jac exactly 0 and d_raw[..., 7:] = Y_0 dL/dRGB.
      A Gaussian no view sees: SH words exactly 0, geometry words finite.  MECHANISMS, asserted on the pointers the kernels get: the
      records are 40 / 76 / 136 / 220 bytes, so view 1's base sits at 8 / 4 / 8 / 4 bytes mod 16 at Gv = 135 and at 0 / 8 / 0 / 8 at
      Gv = 270.  k_raw_eval stages view 0's full blocks with 16-byte loads and its 7- or 14-record tail (and every block of a
      misaligned view 1) word by word: both branches run in every case.  k_raw_bwd stores 16 bytes at a time wherever the block's
      base is aligned — view 0 always — and word by word at a misaligned view 1: both run in every case but Gv = 270 at d_sh = 1 and
      9, where view 1 is aligned too and the whole store is the 16-byte branch (140 and 476 floats: no remainder either).
  (b) BITS  rgbc (colour + clamp bits), sh_jac and the images equal, as int32 bits and for every Gaussian, those of the two-step path
      (adapter.adapter_tail — the generic k_adapter_fwd at these degrees — then render_views_fused: k_sh_eval<true, true>).
  (c) TAIL  s360_backward_raw_tail with two camera groups at d_sh = 9 and 4, built as in test_raw_tail_with_two_camera_groups.
  (d) AUTOGRAD AND SEAM  rasterize_raw(...).backward() at d_sh = 9 returns the callers' shapes and the direct call's bits; a
      make_adapter_class adapter at sh_degree = 2 + DecoderSplattingFused renders from the raw records (FLAG_RAW_INPUTS), materialises
      nothing and gives the eager adapter's images bit for bit.
  (e) DETERMINISM  two runs at d_sh = 16: identical bits in all outputs.

Measured on an MI355X (worst per-Gaussian error in units of 2^-24, kernels / float32 yardstick; also
profiles/raw_degrees_accuracy.json, written through S360_ACCURACY_REPORT=<file>):
  d_sh=1 hm3d Gv=135 per_ray=1 rot=1 dm=1      means 3.31/3.20  covariances 11.91/11.80  d_depths 2.52/2.37  d_raw_scale 2.22/2.21  d_raw_quat 2.43/2.85  d_raw_sh 1.77/1.77  colour 1.72/1.72
  d_sh=1 m3d Gv=270 per_ray=2 rot=0 dm=0       means 4.93/5.41  covariances 11.48/10.77  d_depths 5.74/4.93  d_raw_scale 1.99/2.00  d_raw_quat 2.70/2.97  d_raw_sh 1.78/1.78  colour 1.81/1.81
  d_sh=4 hm3d Gv=135 per_ray=1 rot=1 dm=1      means 3.31/3.20  covariances 9.75/10.11   d_depths 2.69/2.74  d_raw_scale 1.49/1.49  d_raw_quat 4.15/2.85  d_raw_sh 2.71/3.40  colour 2.31/2.31
  d_sh=4 m3d Gv=270 per_ray=2 rot=0 dm=0       means 4.93/5.41  covariances 13.10/11.40  d_depths 4.28/5.18  d_raw_scale 1.75/1.68  d_raw_quat 3.06/2.42  d_raw_sh 2.99/3.30  colour 2.25/2.25
  d_sh=9 hm3d Gv=135 per_ray=1 rot=1 dm=1      means 3.31/3.20  covariances 11.21/11.19  d_depths 3.06/2.51  d_raw_scale 1.27/1.38  d_raw_quat 2.47/2.60  d_raw_sh 6.34/6.10  colour 1.89/1.89
  d_sh=9 m3d Gv=270 per_ray=2 rot=0 dm=0       means 4.93/5.41  covariances 10.97/10.20  d_depths 4.26/3.67  d_raw_scale 2.50/1.74  d_raw_quat 3.43/3.55  d_raw_sh 5.02/5.60  colour 2.85/2.85
  d_sh=16 hm3d Gv=135 per_ray=1 rot=1 dm=1     means 3.31/3.20  covariances 11.80/10.44  d_depths 2.66/2.38  d_raw_scale 1.12/1.18  d_raw_quat 3.21/2.72  d_raw_sh 7.87/7.15  colour 2.81/2.22
  d_sh=16 m3d Gv=270 per_ray=2 rot=0 dm=0      means 4.93/5.41  covariances 12.76/12.59  d_depths 3.45/3.71  d_raw_scale 1.43/1.10  d_raw_quat 2.79/3.42  d_raw_sh 6.53/6.76  colour 3.11/2.95
  tail d_sh=9 hm3d Gv=135 per_ray=1 rot=1 dm=1 d_depths 3.06/2.51  d_raw_scale 1.27/1.38  d_raw_quat 2.47/2.60  d_raw_sh 6.72/13.58
  tail d_sh=4 m3d Gv=270 per_ray=2 rot=0 dm=1  d_depths 2.96/2.65  d_raw_scale 1.75/1.68  d_raw_quat 3.06/2.42  d_raw_sh 7.19/7.19
  d_sh=1: d_raw SH against Y_0 dL/dRGB 1.77 (rot) and 1.78 (no rot), the yardstick's own figures.  The worst ratio is 1.46 (d_raw_quat, d_sh = 4).
"""
import ctypes as C
import json
import os
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from einops import rearrange

import raw_degree_reference as rr
from test_gpu_adapter_float64 import EPS, GUARD, SMAX, SMIN, U, _assert_owned, _errors, _guarded, _inputs
from test_gpu_raw_float64 import FACTOR, FW, _ptr
from splatter360_amd import _lib, adapter, decoder, lazy, rasterizer

pytestmark = pytest.mark.gpu
REPORT = {}
WHAT = ("tests/test_gpu_raw_degrees.py on an MI355X: the raw-input path at d_sh = 1, 4, 9, 16 per Gaussian against float64 adapter_tail_torch; worst "
        "per-Gaussian error in units of 2^-24 of each measure's denominator (tests/test_gpu_adapter_float64.py), kernel / float32 CPU yardstick "
        "(bound: kernel <= 2 x yardstick).")
D_SH = (1, 4, 9, 16)
CASES = [(d_sh, *rest) for d_sh in D_SH for rest in (("hm3d", 1, True, True), ("m3d", 2, False, False))]
BACKWARD_Q = ("d_depths", "d_raw_scale", "d_raw_quat", "d_raw_sh")
VIEW1_OFFSET = {135: {1: 8, 4: 4, 9: 8, 16: 4}, 270: {1: 0, 4: 8, 9: 0, 16: 8}}     # (Gv x record bytes) mod 16


def _report(key, fig):
    REPORT[key] = fig
    path = os.environ.get("S360_ACCURACY_REPORT")
    if path:
        p = Path(path)
        old = json.loads(p.read_text()) if p.exists() else {}
        p.write_text(json.dumps(dict(what={**old.get("what", {}), "raw_degrees": WHAT}, cases={**old.get("cases", {}), **REPORT}), indent=1, sort_keys=True))


def _setup(gpu, d_sh, name, per_ray, with_rot, diff_means, split_lists=None):
    """test_gpu_raw_float64._setup at d_sh: the forward through rasterize_raw on six 32 x 32 faces centred at context view 0."""
    c = _inputs(300 + per_ray, 2, 9, 15, per_ray, d_sh, with_rot, per_ray == 1)
    assert c.gv == 135 * per_ray and c.gv % 64 in (7, 14) and c.gv > 64
    pose = torch.eye(4)
    pose[:3, 3] = c.ext[0, :3, 3]
    e6, K, near, far = decoder.cube_cameras(pose.to(gpu), 0.1, 10.0)
    views = decoder.pack_camera_views(e6, K, near, far, torch.zeros(3, device=gpu))
    dev = lambda t: None if t is None else t.to(gpu).contiguous()
    ext, rot = dev(c.ext), dev(c.rot)
    d, o, r = (dev(t).reshape(-1, *t.shape[2:]).requires_grad_(True) for t in (c.dep, c.opa, c.raw))
    img, means, cov6 = rasterizer.rasterize_raw(d, o, r, ext, views=views, image_height=FW, image_width=FW, context_shape=(c.h, c.w), scale_min=SMIN,
                                                scale_max=SMAX, sh_rotation=rot, per_ray=per_ray, eps=EPS, erp_convention=adapter.ERP_CONVENTIONS[name],
                                                differentiable_means=diff_means, split_lists=split_lists)
    state = rasterizer.last_state()
    assert not state.overflowed() and state.prm.flags & _lib.FLAG_RAW_INPUTS
    assert state.prm.M == d_sh and state.prm.sh_degree == rr.degree_of(d_sh)
    width = 7 + 3 * d_sh
    s = SimpleNamespace(c=c, views=views, ext=ext, rot=rot, d=d, o=o, r=r, img=img, means=means, cov6=cov6, state=state, name=name, per_ray=per_ray,
                        diff_means=diff_means, P=2 * c.gv, d_sh=d_sh, width=width)
    _assert_mechanisms(s, r.data_ptr(), "raw_gaussians")
    return s


def _assert_mechanisms(s, base, what):
    """On the pointer a kernel gets: view 1 sits at the offset the case expects; a 16-byte-aligned full block exists (view 0's first)
    and so does a block the forward stages word by word (view 0's tail)."""
    gv, bytes_ = s.c.gv, 4 * s.width
    assert bytes_ == {1: 40, 4: 76, 9: 136, 16: 220}[s.d_sh]
    assert [(base + v * gv * bytes_) % 16 for v in range(2)] == [0, VIEW1_OFFSET[gv][s.d_sh]], what
    blocks = [(v, b, min(64, gv - b)) for v in range(2) for b in range(0, gv, 64)]
    aligned = lambda v, b: (base + (v * gv + b) * bytes_) % 16 == 0
    assert any(aligned(v, b) and nb == 64 for v, b, nb in blocks), (what, "no block takes the 16-byte branch")
    assert any(nb < 64 or not aligned(v, b) for v, b, nb in blocks), (what, "no block takes the scalar staging branch")
    misaligned_store = any(not aligned(v, b) for v, b, _ in blocks)                   # k_raw_bwd's word-by-word store
    assert misaligned_store == (VIEW1_OFFSET[gv][s.d_sh] != 0)
    assert misaligned_store or (gv, s.d_sh) in ((270, 1), (270, 9))


def _rin(s):
    c = s.c
    return _lib.S360RawInputs(s.ext.data_ptr(), s.d.data_ptr(), s.r.data_ptr(), None if s.rot is None else s.rot.data_ptr(), 2, c.gv, c.h, c.w, s.per_ray,
                              adapter.ERP_CONVENTIONS[s.name], SMIN, SMAX, EPS)


def _upstream(gpu):
    return torch.tensor(np.random.default_rng(5).standard_normal((6, 3, FW, FW)).astype(np.float32), device=gpu)


def _backward_raw(gpu, s):
    """s360_backward_raw into guarded NaN-filled buffers; -> {name: float32 tensor on the CPU}, ownership asserted."""
    prm, lay, P = s.state.prm, s.state.layout, s.P
    g = _upstream(gpu)
    sizes = dict(d_means3D=3 * P, d_cov6=6 * P, d_opacities=P, d_rgb_sum=4 * P, d_depths=P, d_raw=s.width * P)
    bufs = {k: _guarded(gpu, n) for k, n in sizes.items()}
    body = lambda k: C.c_void_p(bufs[k].data_ptr() + 4 * GUARD)
    _assert_mechanisms(s, body("d_raw").value, "d_raw_gaussians")
    bws = torch.empty(lay.backward_bytes, dtype=torch.uint8, device=gpu)
    rin = _rin(s)
    stream = C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    rc = _lib.lib().s360_backward_raw(C.byref(prm), _ptr(s.views), C.byref(rin), _ptr(s.means), _ptr(s.cov6), _ptr(s.o.detach()), _ptr(s.state.workspace),
                                      lay.total_bytes, _ptr(g), None, None, 0, int(s.diff_means), body("d_means3D"), body("d_cov6"), body("d_opacities"),
                                      body("d_rgb_sum"), body("d_depths"), body("d_raw"), _ptr(bws), lay.backward_bytes, stream)
    _lib.check(rc, "s360_backward_raw")
    torch.cuda.synchronize()
    out = {k: bufs[k][GUARD:GUARD + n].cpu() for k, n in sizes.items()}
    for k, n in sizes.items():
        if k == "d_rgb_sum":        # its .w is an int32 stamp, and -1 (seen by no view) reads as a NaN: ownership by the fill's own bit pattern
            bits, fill = bufs[k].cpu().view(torch.int32), torch.full((1,), float("nan")).view(torch.int32)
            assert not bool((bits[GUARD:GUARD + n] == fill).any()), (k, "an element was not written")
            bufs[k][GUARD + 3:GUARD + n:4] = 0.0
        _assert_owned(bufs[k], n, k)
    return out


def _case_namespace(s, d_cov6, d_means):
    """The `c` of test_gpu_adapter_float64._errors: cotangents in its layouts (wc: the six entries in the upper triangle)."""
    c = s.c
    wc = torch.zeros((c.v, c.gv, 3, 3))
    r_, c_ = torch.triu_indices(3, 3)
    wc[:, :, r_, c_] = d_cov6.reshape(c.v, c.gv, 6)
    wm = torch.zeros((c.v, c.gv, 3)) if d_means is None else d_means.reshape(c.v, c.gv, 3)
    return SimpleNamespace(v=c.v, gv=c.gv, d_sh=s.d_sh, dep=c.dep, ext=c.ext, raw=c.raw, wc=wc, wm=wm, wh=None)


def _judge(tag, s, got_dep, got_raw, ref, y32, cn, quantities, forward=None):
    """test_gpu_raw_float64._judge at d_sh: the kernels' (d_depths, d_raw) — and means / cov6 when forward — against ref under the
    yardstick y32.  A degree block whose reference cotangent g_harm is 0 must be exactly 0 in the kernels and in the yardstick."""
    c, n = s.c, s.d_sh
    wh = ref.g_harm.clone()
    dead = torch.zeros((c.v, c.gv, 3, n), dtype=torch.bool)
    for a, b in rr.sh_block_slices(n):
        z = ref.g_harm[..., a:b].norm(dim=-1) == 0
        dead[..., a:b] = z[..., None]
    wh[dead] = 1.0
    cn.wh = wh
    got = SimpleNamespace(means=ref.means if forward is None else forward[0], cov=ref.cov if forward is None else forward[1], scales=ref.scales,
                          rot=ref.rot, harm=ref.harm, d_dep=got_dep.double().reshape(c.v, c.gv), d_raw=got_raw.double().reshape(c.v, c.gv, s.width))
    for k, t in vars(got).items():
        assert bool(torch.isfinite(t).all()), (tag, k, "not finite")
    sh_k = got.d_raw[..., 7:].reshape(c.v, c.gv, 3, n)
    assert bool((sh_k[dead] == 0).all()) and bool((y32.d_raw[..., 7:].reshape(c.v, c.gv, 3, n)[dead] == 0).all()), (tag, "a dead SH block is not exactly 0")
    ek, ey = _errors(got, ref, cn, True, s.diff_means), _errors(y32, ref, cn, True, s.diff_means)
    ek, ey = ({q: torch.nan_to_num(e[q], nan=0.0, posinf=float("inf")) for q in quantities} for e in (ek, ey))
    fig, bad = {}, []
    for q in quantities:
        k, y = ek[q].max().item(), ey[q].max().item()
        fig[q] = dict(kernel_worst=k / U, float32_worst=y / U)
        if not k <= FACTOR * y:
            bad.append((q, k / U, y / U, int(ek[q].argmax())))
    print(f"[rawdeg] {tag:<46} " + "  ".join(f"{q} {f['kernel_worst']:.2f}/{f['float32_worst']:.2f}" for q, f in fig.items()))
    _report(f"rawdeg/{tag}", fig)
    assert not bad, (tag, "kernel error above 2 x the float32 yardstick: (quantity, kernel, yardstick [2^-24], worst Gaussian)", bad)
    return dead, fig


def _references(s, means32, group_views, d_cov6, d_rgb, d_means):
    c = s.c
    args = (c.ext, c.dep, c.raw, c.rot, means32, group_views, d_cov6.numpy(), d_rgb.numpy(), None if d_means is None else d_means.numpy(), (c.h, c.w), s.per_ray,
            s.name, SMIN, SMAX, EPS)
    return rr.raw_tail_reference(torch.float64, *args), rr.raw_tail_reference(torch.float32, *args), args


def _tag(s):
    return f"d_sh={s.d_sh} {s.name} Gv={s.c.gv} per_ray={s.per_ray} rot={int(s.rot is not None)} dm={int(s.diff_means)}"


# ------------------------------------------------------------------------------------------------ (a) per Gaussian
@pytest.mark.parametrize("d_sh,name,per_ray,with_rot,diff_means", CASES)
def test_raw_path_per_gaussian_at_every_degree(gpu, d_sh, name, per_ray, with_rot, diff_means):
    s = _setup(gpu, d_sh, name, per_ray, with_rot, diff_means)
    c, P, tag = s.c, s.P, _tag(s)
    out = _backward_raw(gpu, s)
    means32, cov6 = s.means.detach().cpu(), s.cov6.detach().cpu()
    d_cov6, d_rgb = out["d_cov6"].reshape(P, 6), out["d_rgb_sum"].reshape(1, P, 4)
    d_means = out["d_means3D"].reshape(P, 3) if diff_means else None
    views = s.views.cpu()
    ref, y32, _ = _references(s, means32, views, d_cov6, d_rgb, d_means)
    cn = _case_namespace(s, d_cov6, d_means)
    fwd = (means32.double().reshape(c.v, c.gv, 3), cov6.double().reshape(c.v, c.gv, 6))
    dead, fig = _judge(tag, s, out["d_depths"], out["d_raw"], ref, y32, cn, ("means", "covariances") + BACKWARD_Q, forward=fwd)

    # the scene reached its mechanisms: Gaussians seen by no face (context view 0's planted depth 1e-2 among them), and seen ones
    w = d_rgb[0, :, 3].contiguous().view(torch.int32)
    vis_any = (s.state.tensors()["vis_mask"].cpu() != 0)
    assert bool(((w >= 0) == vis_any).all()) and int(vis_any.sum()) >= P // 2
    d_raw = out["d_raw"].reshape(P, s.width)
    if per_ray == 1:
        planted = c.planted.reshape(-1)
        assert int(planted.sum()) == 16 and bool((~vis_any)[(0 + 4 * 6) % c.gv]), "the depth-1e-2 Gaussian of view 0 sits at the target's centre"
        assert int((~vis_any).sum()) >= 1
    # a Gaussian no view sees (the per_ray = 2 inputs plant none and may have none)
    assert bool(torch.isfinite(d_raw[~vis_any][:, :7]).all()) and bool((d_raw[~vis_any][:, 7:] == 0).all())
    assert bool(dead.reshape(P, -1)[~vis_any].all())

    # forward colours: the rgbc record (clamped colour, clamp bits) of every Gaussian
    rgbc = s.state._arr(s.state.layout.rgbc, P * 4, torch.float32).view(P, 4).cpu()
    c64, cond = rr.raw_colours(torch.float64, ref.harm, means32, views[0])
    c32, _ = rr.raw_colours(torch.float32, y32.harm.float(), means32, views[0])
    ek = ((rgbc[:, :3].double() - c64.clamp_min(0)).abs() / cond).amax(-1)
    ey = ((c32.clamp_min(0) - c64.clamp_min(0)).abs() / cond).amax(-1)
    k, y = ek.max().item(), ey.max().item()
    print(f"[rawdeg] {tag:<46} colour {k / U:.2f}/{y / U:.2f}")
    _report(f"rawdeg/{tag}/colour", dict(colour=dict(kernel_worst=k / U, float32_worst=y / U)))
    assert k <= FACTOR * y, (tag, "colour", k / U, y / U)
    bits = rgbc[:, 3].contiguous().view(torch.int32)
    got_bits = torch.stack([(bits >> j) & 1 for j in range(3)], -1).bool()
    sure = c64.abs() > FACTOR * y * cond                    # farther from 0 than the bound: the sign is decided
    assert bool((got_bits == (c64 < 0))[sure].all()) and float(sure.float().mean()) > 0.99
    assert bool((rgbc[:, :3][got_bits] == 0).all())
    if d_sh > 1:                                            # higher bands can pull a colour below zero (d_sh = 1: 0.5 + 0.28 x N(0,1) rarely)
        assert bool(got_bits.any())

    if d_sh == 1:
        # degree 0: the colour does not depend on the direction, and dL/d(coefficient) = mask_0 D_0 Y_0 dL/dRGB = Y_0 dL/dRGB
        jac = s.state._arr(s.state.layout.sh_jac, P * 9, torch.float32).cpu()
        assert bool((jac == 0).all()), "sh_jac at degree 0"
        # (times the view's 1 x 1 rotation block as the float32 the kernels read: 1 up to its own rounding)
        d00 = torch.ones(P, 1, dtype=torch.float64) if c.rot is None else c.rot[:, 0, 0].double().repeat_interleave(c.gv)[:, None]
        want = 0.28209479177387814 * d00 * d_rgb[0, :, :3].double() * (w >= 0)[:, None]
        err = (d_raw[:, 7:].double() - want).abs()
        assert bool((err[want == 0] == 0).all())
        rel = (err / want.abs().clamp_min(1e-300))[want != 0].max().item()
        print(f"[rawdeg] {tag:<46} d_raw_sh against Y_0 dL/dRGB {rel / U:.2f}")
        assert rel <= FACTOR * fig["d_raw_sh"]["float32_worst"] * U, (tag, rel / U, fig["d_raw_sh"])


# ------------------------------------------------------------------------------------------------ (b) the two-step path's bits
@pytest.mark.parametrize("d_sh,name,per_ray,with_rot", [(1, "hm3d", 1, True), (4, "m3d", 2, False), (9, "hm3d", 1, True), (16, "m3d", 2, False)])
def test_raw_forward_is_the_two_step_paths_bits_at_every_degree(gpu, d_sh, name, per_ray, with_rot):
    """k_raw_eval<.., DEG> restates the generic two-step kernels' expressions (k_adapter_fwd's rotation, k_sh_eval<true, true>'s colour
    sum, jacobian chains and last rounding): rgbc, sh_jac and the images of every Gaussian, culled ones included, are the same bits."""
    s = _setup(gpu, d_sh, name, per_ray, with_rot, False)
    c, P, st = s.c, s.P, s.state
    grab = lambda state: (state._arr(state.layout.rgbc, P * 4, torch.int32).clone(), state._arr(state.layout.sh_jac, P * 9, torch.int32).clone())
    rgbc_raw, jac_raw = grab(st)
    d, o, r = (t.detach().clone().requires_grad_(True) for t in (s.d, s.o, s.r))
    g = adapter.adapter_tail(s.ext, d.reshape(2, -1), o.reshape(2, -1), r.reshape(2, -1, s.width), (c.h, c.w), SMIN, SMAX, sh_rotation=s.rot, eps=EPS,
                             per_ray=per_ray, dataset_name=name)
    pose = torch.eye(4)
    pose[:3, 3] = c.ext[0, :3, 3]
    e6, K, near, far = decoder.cube_cameras(pose.to(gpu), 0.1, 10.0)
    img2 = decoder.render_views_fused(e6, K, near, far, (FW, FW), torch.zeros(3, device=gpu), g.means.reshape(-1, 3), g.covariances.reshape(-1, 3, 3),
                                      g.harmonics.reshape(-1, 3, d_sh), g.opacities.reshape(-1), shared_campos=True)
    st2 = rasterizer.last_state()
    assert st2 is not st and st2.prm.P == P and st2.prm.M == d_sh and not (st2.prm.flags & _lib.FLAG_RAW_INPUTS) and st.prm.flags & _lib.FLAG_RAW_INPUTS
    rgbc2, jac2 = grab(st2)
    assert torch.equal(rgbc_raw, rgbc2), "rgbc"
    assert torch.equal(jac_raw, jac2), "sh_jac"
    assert torch.equal(img2.detach(), s.img.detach()), "images"
    if d_sh > 1:
        assert int((rgbc2.view(P, 4)[:, 3] != 0).sum()) > 0
    else:
        assert not bool(jac2.any())


# ------------------------------------------------------------------------------------------------ (c) two camera groups
@pytest.mark.parametrize("d_sh,name,per_ray,with_rot,diff_means", [(9, "hm3d", 1, True, True), (4, "m3d", 2, False, True)])
def test_raw_tail_with_two_camera_groups_at_lower_degrees(gpu, d_sh, name, per_ray, with_rot, diff_means):
    """s360_backward_raw_tail, n_groups = 2: group 0 = the call's own clamp-masked dL/dRGB sums (.w rewritten to record 0), group 1 =
    a synthetic rank at another camera centre whose .w is -1 on every other Gaussian.  Outputs guarded."""
    s = _setup(gpu, d_sh, name, per_ray, with_rot, diff_means)
    c, P = s.c, s.P
    out = _backward_raw(gpu, s)
    tag = "tail " + _tag(s)
    rng = np.random.default_rng(8)
    rgb = torch.zeros((2, P, 4))
    rgb[0] = out["d_rgb_sum"].reshape(P, 4)
    w0 = rgb[0, :, 3].contiguous().view(torch.int32)
    rgb[0, :, 3] = torch.where(w0 >= 0, torch.zeros_like(w0), w0).view(torch.float32)
    rgb[1, :, :3] = torch.tensor(rng.standard_normal((P, 3)).astype(np.float32)) * rgb[0, :, :3].abs().max()
    rgb[1, :, 3] = torch.tensor(np.where(np.arange(P) % 2 == 1, 1, -1).astype(np.int32)).view(torch.float32)
    pose2 = torch.eye(4)
    pose2[:3, 3] = c.ext[0, :3, 3] + torch.tensor([0.3, -0.2, 0.1])
    e6, K, near, far = decoder.cube_cameras(pose2.to(gpu), 0.1, 10.0)
    group_views = torch.cat([s.views[:1], decoder.pack_camera_views(e6[:1], K[:1], near[:1], far[:1], torch.zeros(3, device=gpu))]).contiguous()
    assert not torch.equal(group_views[0, 32:35], group_views[1, 32:35])
    d_cov6 = out["d_cov6"].reshape(P, 6)
    d_means = out["d_means3D"].reshape(P, 3) if diff_means else None
    bufs = dict(d_depths=_guarded(gpu, P), d_raw=_guarded(gpu, s.width * P))
    body = lambda k: C.c_void_p(bufs[k].data_ptr() + 4 * GUARD)
    rin = _rin(s)
    dm_dev = None if d_means is None else d_means.to(gpu).contiguous()
    dc_dev, rgb_dev = d_cov6.to(gpu).contiguous(), rgb.to(gpu).contiguous()
    stream = C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)

    def tail(n_groups):
        for k, n in (("d_depths", P), ("d_raw", s.width * P)):
            bufs[k][GUARD:GUARD + n] = float("nan")
        rc = _lib.lib().s360_backward_raw_tail(C.byref(s.state.prm), _ptr(group_views), n_groups, C.byref(rin), _ptr(s.means), _ptr(s.state.workspace),
                                               s.state.layout.total_bytes, _ptr(dm_dev), _ptr(dc_dev), _ptr(rgb_dev), body("d_depths"), body("d_raw"), stream)
        _lib.check(rc, "s360_backward_raw_tail")
        torch.cuda.synchronize()
        _assert_owned(bufs["d_depths"], P, "d_depths")
        _assert_owned(bufs["d_raw"], s.width * P, "d_raw")
        return bufs["d_depths"][GUARD:GUARD + P].cpu(), bufs["d_raw"][GUARD:GUARD + s.width * P].cpu().reshape(P, s.width)

    dep1, raw1 = tail(1)
    dep2, raw2 = tail(2)
    ref, y32, args = _references(s, s.means.detach().cpu(), group_views.cpu(), d_cov6, rgb, d_means)
    dead, _ = _judge(tag, s, dep2, raw2, ref, y32, _case_namespace(s, d_cov6, d_means), BACKWARD_Q)
    nobody = (w0 < 0) & (torch.arange(P) % 2 == 0)                # seen by neither group
    assert (int(nobody.sum()) >= 1 or per_ray != 1) and bool(dead.reshape(P, -1)[nobody].all())
    # the second group reached the result and touched the SH words only: in the kernels ...
    assert torch.equal(raw1[:, :7].view(torch.int32), raw2[:, :7].view(torch.int32)) and torch.equal(dep1.view(torch.int32), dep2.view(torch.int32))
    assert not torch.equal(raw1[:, 7:], raw2[:, 7:])
    assert torch.equal(raw1.view(torch.int32), out["d_raw"].reshape(P, s.width).view(torch.int32)), "one group: s360_backward_raw's own last kernel"
    # ... and in the reference
    one = rr.raw_tail_reference(torch.float64, *args[:7], rgb[:1].numpy(), *args[8:])
    assert not torch.equal(one.d_raw[..., 7:], ref.d_raw[..., 7:]) and torch.equal(one.d_raw[..., :7], ref.d_raw[..., :7])


# ------------------------------------------------------------------------------------------------ (d) autograd and the seam
def test_autograd_returns_the_callers_shapes_and_the_direct_calls_bits(gpu):
    s = _setup(gpu, 9, "hm3d", 1, True, True, split_lists=False)
    c, P = s.c, s.P
    out = _backward_raw(gpu, s)
    d, o, r = s.d.detach().reshape(2, c.gv).clone().requires_grad_(True), s.o.detach().reshape(2, c.gv, 1).clone().requires_grad_(True), \
        s.r.detach().reshape(2, 9, 15, 34).clone().requires_grad_(True)
    img, _, _ = rasterizer.rasterize_raw(d, o, r, s.ext, views=s.views, image_height=FW, image_width=FW, context_shape=(c.h, c.w), scale_min=SMIN, scale_max=SMAX,
                                         sh_rotation=s.rot, per_ray=1, eps=EPS, erp_convention=adapter.ERP_CONVENTIONS["hm3d"], differentiable_means=True,
                                         split_lists=False)
    assert torch.equal(img.detach(), s.img.detach())
    img.backward(_upstream(gpu))
    assert d.grad.shape == (2, c.gv) and o.grad.shape == (2, c.gv, 1) and r.grad.shape == (2, 9, 15, 34)
    bits = lambda t: t.detach().cpu().reshape(-1).view(torch.int32)
    assert torch.equal(bits(d.grad), bits(out["d_depths"])), "d_depths"
    assert torch.equal(bits(o.grad), bits(out["d_opacities"])), "d_opacities"
    assert torch.equal(bits(r.grad), bits(out["d_raw"])), "d_raw"


def test_the_seam_renders_degree_two_from_the_raw_records(gpu):
    """tests/test_gpu_lazy_seam.py's replay at sh_degree = 2 (in lazy.RAW_SEAM_DEGREES): the replaced adapter class hands out lazy
    fields, the encoder's rearranges keep them lazy, the fused decoder renders from the raw tensors."""
    degree = 2
    assert degree in lazy.RAW_SEAM_DEGREES
    d_sh = (degree + 1) ** 2
    c = _inputs(301, 2, 9, 15, 1, d_sh, True, True)
    cfg = SimpleNamespace(gaussian_scale_min=SMIN, gaussian_scale_max=SMAX, sh_degree=degree)
    ext = c.ext.to(gpu)[None]
    dep, op, raw = c.dep.to(gpu).reshape(1, 2, c.gv, 1, 1), c.opa.to(gpu).reshape(1, 2, c.gv, 1, 1), c.raw.to(gpu).reshape(1, 2, c.gv, 1, 1, 7 + 3 * d_sh)
    pose = torch.eye(4, device=gpu)
    pose[:3, 3] = c.ext[0, :3, 3].to(gpu)
    E, K, N, F = (t[None] for t in decoder.cube_cameras(pose, 0.1, 10.0))
    dec = decoder.DecoderSplattingFused(background_color=(0.0, 0.0, 0.0), shared_campos=None).to(gpu)

    def run(lazy_on):
        mod = lazy.make_adapter_class(sh_rotation="native", lazy=lazy_on)(cfg).to(gpu)
        assert mod.d_sh == d_sh and mod.d_in == 7 + 3 * d_sh
        a = mod.forward("hm3d", ext[:, :, None, None, None], dep, op, raw, (c.h, c.w))
        flat = SimpleNamespace(means=rearrange(a.means, "b v r srf spp xyz -> b (v r srf spp) xyz"),
                               covariances=rearrange(a.covariances, "b v r srf spp i j -> b (v r srf spp) i j"),
                               harmonics=rearrange(a.harmonics, "b v r srf spp c d_sh -> b (v r srf spp) c d_sh"),
                               opacities=rearrange(1 * a.opacities, "b v r srf spp -> b (v r srf spp)"))
        bd = lazy.bundle_of(flat)
        assert (bd is not None) == lazy_on
        out = dec(flat, E, K, N, F, (FW, FW))
        st = rasterizer.last_state()
        assert bool(st.prm.flags & _lib.FLAG_RAW_INPUTS) == lazy_on and st.prm.M == d_sh and st.prm.sh_degree == degree
        if lazy_on:
            assert bd._materialised is None, "the fused decoder must render from the raw tensors without materialising the Gaussians"
        return out.color
    lazy_img, eager_img = run(True), run(False)
    assert torch.equal(lazy_img, eager_img) and float(lazy_img.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ (e) determinism
def test_two_runs_at_degree_three_give_the_same_bits(gpu):
    runs = []
    for _ in range(2):
        s = _setup(gpu, 16, "hm3d", 1, True, True, split_lists=False)
        out = _backward_raw(gpu, s)
        P = s.P
        rec = {k: v.view(torch.int32).clone() for k, v in out.items()}
        rec.update(images=s.img.detach().cpu().view(torch.int32), means=s.means.detach().cpu().view(torch.int32), cov6=s.cov6.detach().cpu().view(torch.int32),
                   rgbc=s.state._arr(s.state.layout.rgbc, P * 4, torch.int32).cpu().clone(), sh_jac=s.state._arr(s.state.layout.sh_jac, P * 9, torch.int32).cpu().clone())
        runs.append(rec)
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k
