"""The raw-input path (s360_forward_raw: k_raw_eval; s360_backward_raw / s360_backward_raw_tail: k_raw_bwd) held to float64 PER
GAUSSIAN.  These kernels restate the adapter tail's formulas a second time; tests/test_gpu_adapter_float64.py holds only the
stand-alone k_adapter_* kernels per Gaussian, and tests/test_gpu_lazy_seam.py / test_gpu_raw_entry.py judge the raw kernels by
max |err| / max |want| over a whole tensor — d_raw has 82 words per Gaussian, and one Gaussian of a ragged last block could be
wrong by 100 % without moving that figure.

Three evaluations of the same float32 inputs (tests/test_gpu_adapter_float64.py's _inputs, its planted edge Gaussians included):
the kernels; oracle/adapter_ref.adapter_tail_torch in float64 on the CPU (the reference, backward_reference.raw_tail_reference); the
same in float32 on the CPU (the yardstick).  The per-Gaussian measures and denominators are that file's _errors, imported.

  FORWARD   means_out / cov6_out by the adapter test's `means` / `covariances` measures; the clamped colours (the forward's rgbc
            record) against max(0, 0.5 + sum_k Y_k h_k), h = D (mask . raw), in units of 2^-24 of 0.5 + sum_k |Y_k h_k|; the clamp bits
            equal float64's wherever the float64 colour is farther from 0 than the bound itself.  Bit identity with the two-step
            path (adapter kernel, then k_sh_eval3_jac): rgbc and sh_jac, every Gaussian, invisible ones included.
  BACKWARD  one s360_backward_raw call gives d_means3D, d_cov6, d_rgb_sum (valid results themselves) and d_depths, d_raw_gaussians;
            the first three go through the raw-tail reference in float64 and float32, and d_depths, d_raw scale, d_raw quat and
            d_raw SH (per colour and degree block) are judged per Gaussian.  No Gaussian is left out.
  EXACTNESS a Gaussian invisible in every view has d_raw SH exactly 0 (every block: its g_harm is 0) and finite geometry words.  (At
            d_sh = 25 no degree block is masked out — the mask is 0.1 x 0.25^l — so that case does not exist on this path.)
  TAIL      s360_backward_raw_tail with n_groups = 2: the call's own d_rgb_sum and a synthetic second group at another camera centre
            whose .w is -1 on every other Gaussian, against the same reference.
  OWNERSHIP every output of s360_backward_raw is NaN-filled between sentinel floats: no NaN left, no sentinel touched.

Bound, every quantity and case: the kernels' worst per-Gaussian error <= 2 x the float32 yardstick's worst.

Shapes: Gv = 135 = 9 x 15 per view with 2 context views (two full 64-blocks + a tail of 7; the odd Gv misaligns view 1's records to
8 B: the float4 and the scalar staging branch of k_raw_eval, the aligned and the scalar store of k_raw_bwd) and Gv = 270 with
per_ray = 2; with and without sh_rotation; differentiable_means 0 and 1; two ERP conventions; rendered on six 32 x 32 cube faces
whose centre is context view 0's: its planted depth-1e-2 Gaussian lies inside every near plane (invisible everywhere).

Out of scope: the S360_RAW_MFMA=1 experiment (its switch is read once per process; tests/test_gpu_raw_entry.py shows it gives the
same bits); d2inv == 0 as in tests/test_gpu_backward_float64.py; the seam between composite and chain on this path
(s360_backward_gaussians: tests/test_gpu_backward_float64.py).

Measured on an MI355X (worst per-Gaussian error in units of 2^-24, kernels / float32 yardstick; also
profiles/spherical_raw_float64_accuracy.json):
  hm3d Gv=135 per_ray=1 rot=1 dm=1           covariances 11.47/10.61  d_depths 2.35/2.19  d_raw_quat 2.64/2.52  d_raw_scale 2.86/2.68  d_raw_sh 11.56/18.11  means 3.31/3.20  colour 3.37/3.89
  hm3d Gv=270 per_ray=2 rot=1 dm=0           covariances 11.11/11.95  d_depths 5.86/5.61  d_raw_quat 3.42/3.96  d_raw_scale 2.55/2.32  d_raw_sh 13.39/15.99  means 2.93/3.13  colour 3.92/2.84
  m3d Gv=135 per_ray=1 rot=0 dm=0            covariances 11.47/10.61  d_depths 4.32/4.32  d_raw_quat 2.78/2.65  d_raw_scale 2.42/2.14  d_raw_sh 13.07/16.09  means 3.97/5.11  colour 3.48/2.15
  m3d Gv=270 per_ray=2 rot=0 dm=1            covariances 11.11/11.95  d_depths 4.60/5.34  d_raw_quat 4.42/4.88  d_raw_scale 2.44/2.65  d_raw_sh 13.79/17.37  means 4.93/5.41  colour 3.08/3.02
  tail hm3d Gv=135 per_ray=1 rot=1 dm=1      d_depths 2.35/2.19  d_raw_quat 2.64/2.52  d_raw_scale 2.86/2.68  d_raw_sh 27.23/37.77
  tail m3d Gv=270 per_ray=2 rot=0 dm=1       d_depths 4.60/5.34  d_raw_quat 4.42/4.88  d_raw_scale 2.44/2.65  d_raw_sh 17.70/17.87
"""
import ctypes as C
import json
import os
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import backward_reference as br
from test_gpu_adapter_float64 import EPS, GUARD, SMAX, SMIN, U, _assert_owned, _errors, _guarded, _inputs
from splatter360_amd import _lib, adapter, decoder, rasterizer

pytestmark = pytest.mark.gpu
FACTOR = 2.0                   # kernel <= FACTOR x float32 yardstick, worst per Gaussian; not to be raised
FW = 32
REPORT = {}
WHAT = ("tests/test_gpu_raw_float64.py on an MI355X: the raw-input path per Gaussian against float64 adapter_tail_torch; worst per-Gaussian "
        "error in units of 2^-24 of each measure's denominator (tests/test_gpu_adapter_float64.py), kernel / float32 CPU yardstick "
        "(bound: kernel <= 2 x yardstick).")
CASES = [("hm3d", 1, True, True), ("m3d", 1, False, False), ("hm3d", 2, True, False), ("m3d", 2, False, True)]
BACKWARD_Q = ("d_depths", "d_raw_scale", "d_raw_quat", "d_raw_sh")


def _report(key, fig):
    """Keep the case's figures; with S360_ACCURACY_REPORT=<file> in the environment merge them into that file (shared with
    tests/test_gpu_spherical_float64.py: how profiles/spherical_raw_float64_accuracy.json is made)."""
    REPORT[key] = fig
    path = os.environ.get("S360_ACCURACY_REPORT")
    if path:
        p = Path(path)
        old = json.loads(p.read_text()) if p.exists() else {}
        p.write_text(json.dumps(dict(what={**old.get("what", {}), "raw64": WHAT}, cases={**old.get("cases", {}), **REPORT}), indent=1, sort_keys=True))


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _setup(gpu, name, per_ray, with_rot, diff_means):
    """Inputs, the forward through rasterize_raw on six 32 x 32 faces centred at context view 0, and the call's state."""
    c = _inputs(300 + per_ray, 2, 9, 15, per_ray, 25, with_rot, per_ray == 1)
    assert c.gv == 135 * per_ray and c.gv % 64 in (7, 14)
    pose = torch.eye(4)
    pose[:3, 3] = c.ext[0, :3, 3]
    e6, K, near, far = decoder.cube_cameras(pose.to(gpu), 0.1, 10.0)
    views = decoder.pack_camera_views(e6, K, near, far, torch.zeros(3, device=gpu))
    dev = lambda t: None if t is None else t.to(gpu).contiguous()
    ext, rot = dev(c.ext), dev(c.rot)
    d, o, r = (dev(t).reshape(-1, *t.shape[2:]).requires_grad_(True) for t in (c.dep, c.opa, c.raw))
    img, means, cov6 = rasterizer.rasterize_raw(d, o, r, ext, views=views, image_height=FW, image_width=FW, context_shape=(c.h, c.w), scale_min=SMIN,
                                                scale_max=SMAX, sh_rotation=rot, per_ray=per_ray, eps=EPS, erp_convention=adapter.ERP_CONVENTIONS[name],
                                                differentiable_means=diff_means)
    state = rasterizer.last_state()
    assert not state.overflowed() and state.prm.flags & _lib.FLAG_RAW_INPUTS
    assert [(r.data_ptr() + v * c.gv * 328) % 16 for v in range(2)] == ([0, 8] if per_ray == 1 else [0, 0])
    return SimpleNamespace(c=c, views=views, ext=ext, rot=rot, d=d, o=o, r=r, img=img, means=means, cov6=cov6, state=state, name=name, per_ray=per_ray,
                           diff_means=diff_means, P=2 * c.gv)


def _rin(s):
    c = s.c
    return _lib.S360RawInputs(s.ext.data_ptr(), s.d.data_ptr(), s.r.data_ptr(), None if s.rot is None else s.rot.data_ptr(), 2, c.gv, c.h, c.w, s.per_ray,
                              adapter.ERP_CONVENTIONS[s.name], SMIN, SMAX, EPS)


def _backward_raw(gpu, s):
    """s360_backward_raw into guarded NaN-filled buffers; -> {name: float32 tensor on the CPU}, ownership asserted."""
    prm, lay, P = s.state.prm, s.state.layout, s.P
    g = torch.tensor(np.random.default_rng(5).standard_normal((6, 3, FW, FW)).astype(np.float32), device=gpu)
    sizes = dict(d_means3D=3 * P, d_cov6=6 * P, d_opacities=P, d_rgb_sum=4 * P, d_depths=P, d_raw=82 * P)
    bufs = {k: _guarded(gpu, n) for k, n in sizes.items()}
    body = lambda k: C.c_void_p(bufs[k].data_ptr() + 4 * GUARD)
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
    return {k: out[k] for k in sizes}


def _case_namespace(s, d_cov6, d_means):
    """The `c` of test_gpu_adapter_float64._errors: cotangents in its layouts (wc: the six entries in the upper triangle)."""
    c = s.c
    wc = torch.zeros((c.v, c.gv, 3, 3))
    r_, c_ = torch.triu_indices(3, 3)
    wc[:, :, r_, c_] = d_cov6.reshape(c.v, c.gv, 6)
    wm = torch.zeros((c.v, c.gv, 3)) if d_means is None else d_means.reshape(c.v, c.gv, 3)
    return SimpleNamespace(v=c.v, gv=c.gv, d_sh=25, dep=c.dep, ext=c.ext, raw=c.raw, wc=wc, wm=wm, wh=None)


def _judge(tag, s, got_dep, got_raw, ref, y32, cn, quantities, forward=None):
    """The kernels' (d_depths, d_raw) — and means / cov6 when forward — against ref under the yardstick y32, by _errors' measures.
    A degree block whose reference cotangent g_harm is 0 (a Gaussian invisible to every group) must be exactly 0 in the kernels and
    in the yardstick; _errors then divides by the mask alone (its cotangent norm is replaced by 1)."""
    c = s.c
    wh = ref.g_harm.clone()
    dead = torch.zeros((c.v, c.gv, 3, 25), dtype=torch.bool)
    for a, b in br.sh_block_slices(25):
        z = ref.g_harm[..., a:b].norm(dim=-1) == 0
        dead[..., a:b] = z[..., None]
    wh[dead] = 1.0
    cn.wh = wh
    got = SimpleNamespace(means=ref.means if forward is None else forward[0], cov=ref.cov if forward is None else forward[1], scales=ref.scales,
                          rot=ref.rot, harm=ref.harm, d_dep=got_dep.double().reshape(c.v, c.gv), d_raw=got_raw.double().reshape(c.v, c.gv, 82))
    for k, t in vars(got).items():
        assert bool(torch.isfinite(t).all()), (tag, k, "not finite")
    sh_k = got.d_raw[..., 7:].reshape(c.v, c.gv, 3, 25)
    assert bool((sh_k[dead] == 0).all()) and bool((y32.d_raw[..., 7:].reshape(c.v, c.gv, 3, 25)[dead] == 0).all()), (tag, "a dead SH block is not exactly 0")
    ek, ey = _errors(got, ref, cn, True, s.diff_means), _errors(y32, ref, cn, True, s.diff_means)
    # a measure whose denominator is 0 (no cotangent at all reaches the Gaussian: it is seen by no view) demands exactly 0: 0 / 0 counts
    # as 0, x / 0 stays inf and fails
    ek, ey = ({q: torch.nan_to_num(e[q], nan=0.0, posinf=float("inf")) for q in quantities} for e in (ek, ey))
    fig, bad = {}, []
    for q in quantities:
        k, y = ek[q].max().item(), ey[q].max().item()
        fig[q] = dict(kernel_worst=k / U, float32_worst=y / U)
        if not k <= FACTOR * y:
            bad.append((q, k / U, y / U, int(ek[q].argmax())))
    print(f"[raw64] {tag:<40} " + "  ".join(f"{q} {f['kernel_worst']:.2f}/{f['float32_worst']:.2f}" for q, f in fig.items()))
    _report(f"raw64/{tag}", fig)
    assert not bad, (tag, "kernel error above 2 x the float32 yardstick: (quantity, kernel, yardstick [2^-24], worst Gaussian)", bad)
    return dead


@pytest.mark.parametrize("name,per_ray,with_rot,diff_means", CASES)
def test_raw_path_per_gaussian(gpu, name, per_ray, with_rot, diff_means):
    s = _setup(gpu, name, per_ray, with_rot, diff_means)
    c, P = s.c, s.P
    tag = f"{name} Gv={c.gv} per_ray={per_ray} rot={int(with_rot)} dm={int(diff_means)}"
    out = _backward_raw(gpu, s)
    means32, cov6 = s.means.detach().cpu(), s.cov6.detach().cpu()
    d_cov6, d_rgb = out["d_cov6"].reshape(P, 6), out["d_rgb_sum"].reshape(1, P, 4)
    d_means = out["d_means3D"].reshape(P, 3) if diff_means else None
    views = s.views.cpu()
    args = (c.ext, c.dep, c.raw, c.rot, means32, views, d_cov6.numpy(), d_rgb.numpy(), None if d_means is None else d_means.numpy(), (c.h, c.w), per_ray, name,
            SMIN, SMAX, EPS)
    ref, y32 = br.raw_tail_reference(torch.float64, *args), br.raw_tail_reference(torch.float32, *args)
    cn = _case_namespace(s, d_cov6, d_means)
    fwd = (means32.double().reshape(c.v, c.gv, 3), cov6.double().reshape(c.v, c.gv, 6))
    dead = _judge(tag, s, out["d_depths"], out["d_raw"], ref, y32, cn, ("means", "covariances") + BACKWARD_Q, forward=fwd)

    # the scene reached its mechanisms: Gaussians seen by no face (context view 0's planted depth 1e-2 among them), and seen ones
    w = d_rgb[0, :, 3].contiguous().view(torch.int32)
    t = s.state.tensors()
    vis_any = (t["vis_mask"].cpu() != 0)
    assert bool(((w >= 0) == vis_any).all()) and int(vis_any.sum()) >= P // 2
    if per_ray == 1:
        planted = c.planted.reshape(-1)
        assert int(planted.sum()) == 16 and bool((~vis_any)[(0 + 4 * 6) % c.gv]), "the depth-1e-2 Gaussian of view 0 sits at the target's centre"
        geo = out["d_raw"].reshape(P, 82)[~vis_any][:, :7]
        assert bool(torch.isfinite(geo).all()) and bool((out["d_raw"].reshape(P, 82)[~vis_any][:, 7:] == 0).all())
    assert bool(dead.reshape(P, -1)[~vis_any].all())

    # forward colours: the rgbc record (clamped colour, clamp bits) of every Gaussian
    rgbc = s.state._arr(s.state.layout.rgbc, P * 4, torch.float32).view(P, 4).cpu()
    c64, cond = br.raw_colours(torch.float64, ref.harm, means32, views[0])
    c32, _ = br.raw_colours(torch.float32, y32.harm.float(), means32, views[0])
    ek = ((rgbc[:, :3].double() - c64.clamp_min(0)).abs() / cond).amax(-1)
    ey = ((c32.clamp_min(0) - c64.clamp_min(0)).abs() / cond).amax(-1)
    k, y = ek.max().item(), ey.max().item()
    print(f"[raw64] {tag:<40} colour {k / U:.2f}/{y / U:.2f}")
    _report(f"raw64/{tag}/colour", dict(colour=dict(kernel_worst=k / U, float32_worst=y / U)))
    assert k <= FACTOR * y, (tag, "colour", k / U, y / U)
    bits = rgbc[:, 3].contiguous().view(torch.int32)
    got_bits = torch.stack([(bits >> j) & 1 for j in range(3)], -1).bool()
    sure = c64.abs() > FACTOR * y * cond                    # farther from 0 than the bound: the sign is decided
    assert bool((got_bits == (c64 < 0))[sure].all()) and float(sure.float().mean()) > 0.99 and bool(got_bits.any())
    assert bool((rgbc[:, :3][got_bits] == 0).all())


@pytest.mark.parametrize("name,per_ray,with_rot", [("hm3d", 1, True), ("m3d", 2, False)])
def test_raw_forward_colours_are_the_two_step_paths_bits(gpu, name, per_ray, with_rot):
    """DESIGN: k_raw_eval rotates the coefficients with the adapter kernel's own expression and evaluates colours and jacobian with
    k_sh_eval3_jac's code.  tests/test_gpu_raw_entry.py asserts the IMAGES equal; here the per-Gaussian records themselves — rgbc
    (clamped colour + clamp bits) and sh_jac — of every Gaussian, culled ones included, are the same bits."""
    s = _setup(gpu, name, per_ray, with_rot, False)
    c, P = s.c, s.P
    st = s.state
    grab = lambda state: (state._arr(state.layout.rgbc, P * 4, torch.int32).clone(), state._arr(state.layout.sh_jac, P * 9, torch.int32).clone())
    rgbc_raw, jac_raw = grab(st)
    d, o, r = (t.detach().clone().requires_grad_(True) for t in (s.d, s.o, s.r))
    g = adapter.adapter_tail(s.ext, d.reshape(2, -1), o.reshape(2, -1), r.reshape(2, -1, 82), (c.h, c.w), SMIN, SMAX, sh_rotation=s.rot, eps=EPS,
                             per_ray=per_ray, dataset_name=name)
    pose = torch.eye(4)
    pose[:3, 3] = c.ext[0, :3, 3]
    e6, K, near, far = decoder.cube_cameras(pose.to(gpu), 0.1, 10.0)
    img2 = decoder.render_views_fused(e6, K, near, far, (FW, FW), torch.zeros(3, device=gpu), g.means.reshape(-1, 3), g.covariances.reshape(-1, 3, 3),
                                      g.harmonics.reshape(-1, 3, 25), g.opacities.reshape(-1), shared_campos=True)
    st2 = rasterizer.last_state()
    assert st2 is not st and st2.prm.P == P and not (st2.prm.flags & _lib.FLAG_RAW_INPUTS)
    rgbc2, jac2 = grab(st2)
    assert torch.equal(rgbc_raw, rgbc2) and torch.equal(jac_raw, jac2)
    assert torch.equal(img2.detach(), s.img.detach()) and int((rgbc2.view(P, 4)[:, 3] != 0).sum()) > 0


@pytest.mark.parametrize("name,per_ray,with_rot,diff_means", [CASES[0], CASES[3]])
def test_raw_tail_with_two_camera_groups(gpu, name, per_ray, with_rot, diff_means):
    """s360_backward_raw_tail, n_groups = 2: group 0 = the call's own clamp-masked dL/dRGB sums (.w rewritten to record 0), group 1 =
    a synthetic rank at another camera centre whose .w is -1 on every other Gaussian.  Outputs guarded as above."""
    s = _setup(gpu, name, per_ray, with_rot, diff_means)
    c, P = s.c, s.P
    out = _backward_raw(gpu, s)
    tag = f"tail {name} Gv={c.gv} per_ray={per_ray} rot={int(with_rot)} dm={int(diff_means)}"
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
    bufs = dict(d_depths=_guarded(gpu, P), d_raw=_guarded(gpu, 82 * P))
    body = lambda k: C.c_void_p(bufs[k].data_ptr() + 4 * GUARD)
    rin = _rin(s)
    dm_dev = None if d_means is None else d_means.to(gpu).contiguous()
    dc_dev, rgb_dev = d_cov6.to(gpu).contiguous(), rgb.to(gpu).contiguous()
    stream = C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    rc = _lib.lib().s360_backward_raw_tail(C.byref(s.state.prm), _ptr(group_views), 2, C.byref(rin), _ptr(s.means), _ptr(s.state.workspace),
                                           s.state.layout.total_bytes, _ptr(dm_dev), _ptr(dc_dev), _ptr(rgb_dev), body("d_depths"), body("d_raw"), stream)
    _lib.check(rc, "s360_backward_raw_tail")
    torch.cuda.synchronize()
    _assert_owned(bufs["d_depths"], P, "d_depths")
    _assert_owned(bufs["d_raw"], 82 * P, "d_raw")
    args = (c.ext, c.dep, c.raw, c.rot, s.means.detach().cpu(), group_views.cpu(), d_cov6.numpy(), rgb.numpy(), None if d_means is None else d_means.numpy(),
            (c.h, c.w), per_ray, name, SMIN, SMAX, EPS)
    ref, y32 = br.raw_tail_reference(torch.float64, *args), br.raw_tail_reference(torch.float32, *args)
    dead = _judge(tag, s, bufs["d_depths"][GUARD:GUARD + P].cpu(), bufs["d_raw"][GUARD:GUARD + 82 * P].cpu(), ref, y32, _case_namespace(s, d_cov6, d_means),
                  BACKWARD_Q)
    nobody = (w0 < 0) & (torch.arange(P) % 2 == 0)                # seen by neither group
    assert (int(nobody.sum()) >= 1 or per_ray != 1) and bool(dead.reshape(P, -1)[nobody].all())
    # the second group did reach the result: with one group the same call gives other harmonics words
    one = br.raw_tail_reference(torch.float64, *args[:7], rgb[:1].numpy(), *args[8:])
    assert not torch.equal(one.d_raw[..., 7:], ref.d_raw[..., 7:]) and torch.equal(one.d_raw[..., :7], ref.d_raw[..., :7])
