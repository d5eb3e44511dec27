"""The raw-input path reading the encoder's last convolution output where it lies: channel planes [n_views, C_total, h, w]
(s360_forward_raw_planes: k_raw_eval<.., PLANES = true>; s360_backward_raw_planes / s360_backward_raw_tail_planes: k_raw_bwd<.., true>;
rasterizer.rasterize_raw(raw_layout="planes"); lazy.raw_planes_of + decoder.DecoderSplattingFused) against the record path, as int32
BITS: the plane kernels differ from the record kernels in their staging loads and last stores only, so nothing may differ anywhere.

Six 32 x 32 faces centred at context view 0, two context views, two context shapes:
  9 x 15   Gv = 135 per_ray: planes of 540 B — word 0 of a channel is 16-byte aligned for one channel in four; two full blocks and a
           tail of 7 records per view (per_ray = 1).
  8 x 20   Gv = 160 per_ray: planes of 640 B — every channel base aligned; two full blocks and a tail of 32 records (per_ray = 1).
MECHANISMS (_assert_mechanisms, on the very pointers the kernels get, forward and backward): with per_ray = 1 a full block whose
channel run is 16-byte aligned exists (the 16-byte branch) and so does a run that is loaded / stored word by word (a misaligned
channel at 9 x 15, the tail block at both shapes).  With per_ray = 2 a Gaussian's ray is gi / 2 — a block's words are two interleaved
runs — and the kernels take the word-by-word branch for every block: those cases pin that branch alone.

  (a) every d_sh in 1, 4, 9, 16, 25 x (per_ray 1, rotation, differentiable means, offset 2) and (per_ray 2, no rotation, detached
      means, offset 0), at both shapes: images, means, cov6, rgbc, sh_jac, geo7, d_depths, d_opacities and every record word of the
      gradient equal the record path's bits; the offset channels of the input are NaN and of the autograd gradient exactly 0; the
      direct entries write between guards, leave the offset channels of d_raw_gaussians alone (NaN) and the guards untouched.
  (b) the same with a view stride of 2 C h w: two batch elements interleaved, the other one NaN: nothing of it is read or written.
  (c) s360_backward_raw_tail_planes with two camera groups at d_sh = 9 against s360_backward_raw_tail.
  (d) the seam: a [(v b), C, h, w] leaf through the reference's three-step view chain, make_adapter_class(lazy=True) and
      DecoderSplattingFused, degrees 2 and 4, b = 1 and 2: rendered from the raw inputs without materialising, the eager adapter's
      image bits, the leaf's gradient contiguous, 0 in the offset_xy channels and bit-equal to the record route's
      (lazy.raw_planes_of forced to None); two target centres; a chain the recogniser refuses (.contiguous()) renders the same bits.
  (e) no copy: the plane route's forward peaks at least P (7 + 3 d_sh) 4 bytes - 1 KiB below the record route's — the record copy the
      old route holds, less allocator rounding: derived, not measured.
  (f) two runs at d_sh = 16 on 9 x 15: identical bits in all outputs.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from einops import rearrange

from test_gpu_adapter_float64 import EPS, GUARD, SMAX, SMIN, _assert_owned, _guarded, _inputs
from test_gpu_raw_float64 import FW, _ptr
from splatter360_amd import _lib, adapter, decoder, lazy, rasterizer

pytestmark = pytest.mark.gpu
SHAPES = ((9, 15), (8, 20))
PARAMS = (("hm3d", 1, True, True, 2), ("m3d", 2, False, False, 0))       # dataset, per_ray, rotation, differentiable means, channel offset
NAN_BITS = torch.full((1,), float("nan")).view(torch.int32)


def _bits(t):
    return t.detach().contiguous().cpu().reshape(-1).view(torch.int32)


def _upstream(gpu):
    return torch.tensor(np.random.default_rng(5).standard_normal((6, 3, FW, FW)).astype(np.float32), device=gpu)


def _to_planes(raw, h, w, per_ray, off, fill=float("nan")):
    """records [v, h w per_ray, width] (ray-major, then surface) -> planes [v, per_ray (off + width), h, w]; the offset channels = fill"""
    v, _, width = raw.shape
    out = torch.full((v, per_ray, off + width, h * w), fill, dtype=raw.dtype, device=raw.device)
    out[:, :, off:] = raw.reshape(v, h * w, per_ray, width).permute(0, 2, 3, 1)
    return out.reshape(v, per_ray * (off + width), h, w)


def _from_planes(pl, per_ray, off):
    """-> (records [v h w per_ray, width], offset channels [v, per_ray, off, h w])"""
    v, c, h, w = pl.shape
    x = pl.reshape(v, per_ray, c // per_ray, h * w)
    return x[:, :, off:].permute(0, 3, 1, 2).reshape(v * h * w * per_ray, c // per_ray - off), x[:, :, :off]


def _assert_mechanisms(base, view_stride, hw, width, gv, per_ray, what):
    """On the pointer a plane kernel gets (word 0 of view 0, surface 0, ray 0): which branches its blocks take."""
    if per_ray != 1:
        return          # every block goes word by word (module docstring)
    runs = [((base + 4 * (v * view_stride + c * hw + b0)) % 16 == 0, min(64, gv - b0)) for v in range(2) for b0 in range(0, gv, 64) for c in range(width)]
    assert any(al and nb == 64 for al, nb in runs), (what, "no run takes the 16-byte branch")
    assert any(nb == 64 and not al for al, nb in runs) == (hw % 4 != 0), (what, "misaligned channels of a full block")
    assert any(nb < 64 for al, nb in runs), (what, "no block takes the word-by-word branch")


def _state_bits(state, P):
    arr = lambda off, n: state._arr(off, n, torch.int32).cpu().clone()
    return dict(rgbc=arr(state.layout.rgbc, 4 * P), sh_jac=arr(state.layout.sh_jac, 9 * P), geo7=arr(state.layout.geo7, 7 * P))


def _scene(gpu, d_sh, shape, name, per_ray, with_rot, diff_means, off):
    h, w = shape
    c = _inputs(300 + per_ray, 2, h, w, per_ray, d_sh, with_rot, per_ray == 1)
    pose = torch.eye(4)
    pose[:3, 3] = c.ext[0, :3, 3]
    e6, K, near, far = decoder.cube_cameras(pose.to(gpu), 0.1, 10.0)
    views = decoder.pack_camera_views(e6, K, near, far, torch.zeros(3, device=gpu))
    dev = lambda t: None if t is None else t.to(gpu).contiguous()
    kw = dict(views=views, image_height=FW, image_width=FW, context_shape=(h, w), scale_min=SMIN, scale_max=SMAX, sh_rotation=dev(c.rot), per_ray=per_ray,
              eps=EPS, erp_convention=adapter.ERP_CONVENTIONS[name], differentiable_means=diff_means, split_lists=False)
    return SimpleNamespace(c=c, h=h, w=w, hw=h * w, gv=c.gv, P=2 * c.gv, d_sh=d_sh, width=7 + 3 * d_sh, per_ray=per_ray, off=off, name=name, diff_means=diff_means,
                           views=views, ext=dev(c.ext), rot=dev(c.rot), kw=kw, dep=dev(c.dep).reshape(-1), opa=dev(c.opa).reshape(-1), raw=dev(c.raw),
                           ctot=per_ray * (off + 7 + 3 * d_sh))


def _run(gpu, s, raw, **layout):
    """One forward + backward through rasterize_raw -> every output's bits, the state and the raw gradient."""
    d, o = s.dep.clone().requires_grad_(True), s.opa.clone().requires_grad_(True)
    img, means, cov6 = rasterizer.rasterize_raw(d, o, raw, s.ext, **s.kw, **layout)
    state = rasterizer.last_state()
    assert not state.overflowed() and state.prm.flags & _lib.FLAG_RAW_INPUTS and state.prm.M == s.d_sh
    out = dict(images=_bits(img), means=_bits(means), cov6=_bits(cov6), **_state_bits(state, s.P))
    img.backward(_upstream(gpu))
    out.update(d_depths=_bits(d.grad), d_opacities=_bits(o.grad))
    return SimpleNamespace(out=out, state=state, means=means.detach(), cov6=cov6.detach(), img=img.detach())


def _record_run(gpu, s):
    r = s.raw.reshape(s.P, s.width).clone().requires_grad_(True)
    run = _run(gpu, s, r)
    run.out["d_raw"] = _bits(r.grad)
    return run


def _rin(s, raw_ptr):
    return _lib.S360RawInputs(s.ext.data_ptr(), s.dep.data_ptr(), raw_ptr, None if s.rot is None else s.rot.data_ptr(), 2, s.gv, s.h, s.w, s.per_ray,
                              adapter.ERP_CONVENTIONS[s.name], SMIN, SMAX, EPS)


def _direct(gpu, s, run, planes_in, in_view_stride, out_view_stride, out_floats, out_elem=0):
    """s360_forward_raw_planes and s360_backward_raw_planes themselves, every output between guards: -> bits; d_raw as the whole guarded body."""
    prm, lay, P, hw = run.state.prm, run.state.layout, s.P, s.hw
    stream = C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    word0 = planes_in.data_ptr() + 4 * s.off * hw
    rin = _rin(s, word0)
    surface = (s.off + s.width) * hw
    pin = _lib.S360RawPlanes(in_view_stride, surface, hw)
    _assert_mechanisms(word0, in_view_stride, hw, s.width, s.gv, s.per_ray, "raw_gaussians")
    sizes = dict(means=3 * P, cov6=6 * P, images=6 * 3 * FW * FW, d_means3D=3 * P, d_cov6=6 * P, d_opacities=P, d_rgb_sum=4 * P, d_depths=P, d_raw=out_floats)
    bufs = {k: _guarded(gpu, n) for k, n in sizes.items()}
    body = lambda k: C.c_void_p(bufs[k].data_ptr() + 4 * GUARD)
    ws = torch.empty(lay.total_bytes, dtype=torch.uint8, device=gpu)
    rc = _lib.lib().s360_forward_raw_planes(C.byref(prm), _ptr(s.views), C.byref(rin), C.byref(pin), _ptr(s.opa), body("means"), body("cov6"), body("images"),
                                            None, 0, None, None, 0.0, None, None, None, _ptr(ws), lay.total_bytes, stream)
    _lib.check(rc, "s360_forward_raw_planes")
    g = _upstream(gpu)
    bws = torch.empty(lay.backward_bytes, dtype=torch.uint8, device=gpu)
    out_word0 = body("d_raw").value + 4 * (out_elem + s.off * hw)
    pout = _lib.S360RawPlanes(out_view_stride, surface, hw)
    _assert_mechanisms(out_word0, out_view_stride, hw, s.width, s.gv, s.per_ray, "d_raw_gaussians")
    rc = _lib.lib().s360_backward_raw_planes(C.byref(prm), _ptr(s.views), C.byref(rin), C.byref(pout), body("means"), body("cov6"), _ptr(s.opa), _ptr(ws),
                                             lay.total_bytes, _ptr(g), None, None, 0, int(s.diff_means), body("d_means3D"), body("d_cov6"), body("d_opacities"),
                                             body("d_rgb_sum"), body("d_depths"), C.c_void_p(out_word0), _ptr(bws), lay.backward_bytes, stream)
    _lib.check(rc, "s360_backward_raw_planes")
    torch.cuda.synchronize()
    st2 = rasterizer.RasterState(prm, lay, ws)
    out = {k: _bits(bufs[k][GUARD:GUARD + n]) for k, n in sizes.items() if k != "d_raw"}
    out.update(_state_bits(st2, P))
    for k, n in sizes.items():
        b = bufs[k].cpu()
        if k in ("d_rgb_sum", "d_raw"):      # (.w of d_rgb_sum is an int32 stamp, -1 reads as a NaN; d_raw keeps NaN where the caller owns the words)
            s_ = b[:GUARD].clone()
            assert torch.equal(b[:GUARD], b[GUARD + n:]) and bool((s_ == s_[0]).all()) and not bool(torch.isnan(s_).any()), (k, "a sentinel was overwritten")
            if k == "d_rgb_sum":
                assert not bool((b[GUARD:GUARD + n].view(torch.int32) == NAN_BITS).any()), (k, "an element was not written")
        else:
            _assert_owned(bufs[k], n, k)
    return out, bufs["d_raw"][GUARD:GUARD + out_floats].cpu()


def _compare(a, b, keys=None):
    for k in (keys or a):
        assert torch.equal(a[k], b[k]), k


FORWARD_AND_STATE = ("images", "means", "cov6", "rgbc", "sh_jac", "geo7", "d_depths", "d_opacities")


# ------------------------------------------------------------------------------------------------ (a) bits against the record path
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name,per_ray,with_rot,diff_means,off", PARAMS)
@pytest.mark.parametrize("d_sh", (1, 4, 9, 16, 25))
def test_planes_give_the_record_paths_bits(gpu, d_sh, name, per_ray, with_rot, diff_means, off, shape):
    s = _scene(gpu, d_sh, shape, name, per_ray, with_rot, diff_means, off)
    rec = _record_run(gpu, s)
    assert not bool((rec.out["d_raw"] == NAN_BITS).any()) and bool(rec.out["images"].any())
    planes = _to_planes(s.raw, s.h, s.w, per_ray, off)
    assert planes.shape == (2, s.ctot, s.h, s.w) and (off == 0 or bool(torch.isnan(planes).any()))

    # through autograd: the tensor is read in place, its gradient is contiguous in its shape, the offset channels exactly 0
    leaf = planes.clone().requires_grad_(True)
    pl = _run(gpu, s, leaf, raw_layout="planes", raw_channel_offset=off)
    _compare(rec.out, pl.out, FORWARD_AND_STATE)
    assert leaf.grad.shape == leaf.shape and leaf.grad.is_contiguous()
    g_rec, g_off = _from_planes(leaf.grad, per_ray, off)
    assert torch.equal(_bits(g_rec), rec.out["d_raw"]), "d_raw"
    assert g_off.numel() == 2 * per_ray * off * s.hw and bool((_bits(g_off) == 0).all()), "offset channels of the gradient"

    # the entries themselves, between guards: every record word written, nothing else
    direct, d_raw = _direct(gpu, s, pl, planes, s.ctot * s.hw, s.ctot * s.hw, planes.numel())
    _compare(rec.out, direct, [k for k in direct if k in rec.out])
    g_rec, g_off = _from_planes(d_raw.reshape(planes.shape), per_ray, off)
    assert torch.equal(_bits(g_rec), rec.out["d_raw"]), "d_raw (direct)"
    assert bool(torch.isnan(g_off).all()), "the kernel wrote a channel the records do not cover"


# ------------------------------------------------------------------------------------------------ (b) a view stride of 2 C h w
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("d_sh,name,per_ray,with_rot,diff_means,off", [(25, *PARAMS[0]), (9, *PARAMS[1])])
def test_two_interleaved_batch_elements_share_nothing(gpu, d_sh, name, per_ray, with_rot, diff_means, off, shape):
    s = _scene(gpu, d_sh, shape, name, per_ray, with_rot, diff_means, off)
    rec = _record_run(gpu, s)
    planes = _to_planes(s.raw, s.h, s.w, per_ray, off)
    for mine in (0, 1):
        big = torch.full((2, 2, s.ctot, s.h, s.w), float("nan"), device=gpu)
        big[:, mine] = planes
        big.requires_grad_(True)
        view = big[:, mine]
        assert view.stride(0) == 2 * s.ctot * s.hw and not view.is_contiguous()
        pl = _run(gpu, s, view, raw_layout="planes", raw_channel_offset=off)
        _compare(rec.out, pl.out, FORWARD_AND_STATE)
        g_rec, g_off = _from_planes(big.grad[:, mine], per_ray, off)
        assert torch.equal(_bits(g_rec), rec.out["d_raw"]) and bool((_bits(g_off) == 0).all()) and bool((_bits(big.grad[:, 1 - mine]) == 0).all())
        # the entries, reading and writing at that stride: the other element's words stay NaN
        direct, d_raw = _direct(gpu, s, pl, view, 2 * s.ctot * s.hw, 2 * s.ctot * s.hw, big.numel(), out_elem=mine * s.ctot * s.hw)
        _compare(rec.out, direct, [k for k in direct if k in rec.out])
        whole = d_raw.reshape(2, 2, s.ctot, s.h, s.w)
        g_rec, g_off = _from_planes(whole[:, mine], per_ray, off)
        assert torch.equal(_bits(g_rec), rec.out["d_raw"]) and bool(torch.isnan(g_off).all())
        assert bool(torch.isnan(whole[:, 1 - mine]).all()), "the other batch element was written"


# ------------------------------------------------------------------------------------------------ (c) two camera groups
def test_raw_tail_planes_with_two_camera_groups(gpu):
    """s360_backward_raw_tail_planes, n_groups = 2, built as test_raw_tail_with_two_camera_groups_at_lower_degrees builds its inputs:
    group 0 = the call's own dL/dRGB sums, group 1 = a synthetic rank at another centre, -1 on every other Gaussian."""
    d_sh, (name, per_ray, with_rot, diff_means, off) = 9, PARAMS[0]
    s = _scene(gpu, d_sh, SHAPES[0], name, per_ray, with_rot, diff_means, off)
    r = s.raw.reshape(s.P, s.width).clone().requires_grad_(True)
    d, o = s.dep.clone().requires_grad_(True), s.opa.clone().requires_grad_(True)
    img, means, cov6 = rasterizer.rasterize_raw(d, o, r, s.ext, **s.kw)
    state = rasterizer.last_state()
    P, hw = s.P, s.hw
    rng = np.random.default_rng(8)
    rgb = torch.zeros((2, P, 4))
    rgb[0, :, :3] = torch.tensor(rng.standard_normal((P, 3)).astype(np.float32))
    rgb[0, :, 3] = torch.tensor(np.where(np.arange(P) % 3 == 0, -1, 0).astype(np.int32)).view(torch.float32)
    rgb[1, :, :3] = torch.tensor(rng.standard_normal((P, 3)).astype(np.float32))
    rgb[1, :, 3] = torch.tensor(np.where(np.arange(P) % 2 == 1, 1, -1).astype(np.int32)).view(torch.float32)
    pose2 = torch.eye(4)
    pose2[:3, 3] = s.c.ext[0, :3, 3] + torch.tensor([0.3, -0.2, 0.1])
    e6, K, near, far = decoder.cube_cameras(pose2.to(gpu), 0.1, 10.0)
    group_views = torch.cat([s.views[:1], decoder.pack_camera_views(e6[:1], K[:1], near[:1], far[:1], torch.zeros(3, device=gpu))]).contiguous()
    d_cov6 = torch.tensor(rng.standard_normal((P, 6)).astype(np.float32), device=gpu)
    d_means = torch.tensor(rng.standard_normal((P, 3)).astype(np.float32), device=gpu)
    rgb_dev = rgb.to(gpu).contiguous()
    stream = C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    rin = _rin(s, r.data_ptr())
    n_pl = 2 * s.ctot * hw
    bufs = dict(dep_r=_guarded(gpu, P), raw_r=_guarded(gpu, s.width * P), dep_p=_guarded(gpu, P), raw_p=_guarded(gpu, n_pl))
    body = lambda k: bufs[k].data_ptr() + 4 * GUARD
    args = (_ptr(means), _ptr(state.workspace), state.layout.total_bytes, _ptr(d_means), _ptr(d_cov6), _ptr(rgb_dev))
    _lib.check(_lib.lib().s360_backward_raw_tail(C.byref(state.prm), _ptr(group_views), 2, C.byref(rin), *args, C.c_void_p(body("dep_r")),
                                                 C.c_void_p(body("raw_r")), stream), "s360_backward_raw_tail")
    word0 = body("raw_p") + 4 * off * hw
    pln = _lib.S360RawPlanes(s.ctot * hw, (off + s.width) * hw, hw)
    _assert_mechanisms(word0, s.ctot * hw, hw, s.width, s.gv, per_ray, "d_raw_gaussians")
    _lib.check(_lib.lib().s360_backward_raw_tail_planes(C.byref(state.prm), _ptr(group_views), 2, C.byref(rin), C.byref(pln), *args, C.c_void_p(body("dep_p")),
                                                        C.c_void_p(word0), stream), "s360_backward_raw_tail_planes")
    torch.cuda.synchronize()
    for k, n in (("dep_r", P), ("raw_r", s.width * P), ("dep_p", P)):
        _assert_owned(bufs[k], n, k)
    b = bufs["raw_p"].cpu()
    assert torch.equal(b[:GUARD], b[GUARD + n_pl:]) and bool((b[:GUARD] == b[0]).all()) and not bool(torch.isnan(b[:GUARD]).any())
    g_rec, g_off = _from_planes(b[GUARD:GUARD + n_pl].reshape(2, s.ctot, s.h, s.w), per_ray, off)
    assert torch.equal(_bits(g_rec), _bits(bufs["raw_r"][GUARD:GUARD + s.width * P])) and bool(torch.isnan(g_off).all())
    assert torch.equal(_bits(bufs["dep_p"][GUARD:GUARD + P]), _bits(bufs["dep_r"][GUARD:GUARD + P]))
    one = g_rec.reshape(P, s.width)
    assert bool((one[0::6][:, 7:] == 0).all()) and bool((one[1::2][:, 7:] != 0).any()), "seen by neither group / by the second group"


# ------------------------------------------------------------------------------------------------ (d) the seam
def _chain(leaf, v, b, srf):
    """The reference's three views of its last convolution's output (depth_predictor_multiview_360.py:672-674, encoder_costvolume.py:405-409, :421-424)."""
    x = rearrange(leaf, "(v b) c h w -> b v (h w) c", v=v, b=b)
    x = rearrange(x, "... (srf c) -> ... srf c", srf=srf)
    return rearrange(x[..., 2:], "b v r srf c -> b v r srf () c")


def _seam(gpu, degree, b, centres=1, refuse=False, force_records=False, monkeypatch=None, lazy_on=True, measure=False):
    """One training-like step through the seam -> (images, leaf gradient, bundle)."""
    d_sh = (degree + 1) ** 2
    h, w, v = 9, 15, 2
    ctot = 2 + 7 + 3 * d_sh
    cs = [_inputs(310 + i, v, h, w, 1, d_sh, True, True) for i in range(b)]
    leaf = torch.stack([_to_planes(c.raw, h, w, 1, 2, fill=0.25) for c in cs], 1).reshape(v * b, ctot, h, w).to(gpu).requires_grad_(True)   # "(v b)"
    raw = _chain(leaf, v, b, 1)
    if refuse:
        raw = raw.contiguous()
    if force_records:
        monkeypatch.setattr(lazy, "raw_planes_of", lambda raw: None)
    elif lazy_on:
        assert (lazy.raw_planes_of(raw) is None) == refuse
    cfg = SimpleNamespace(gaussian_scale_min=SMIN, gaussian_scale_max=SMAX, sh_degree=degree)
    ext = torch.stack([c.ext for c in cs]).to(gpu)
    dep = torch.stack([c.dep for c in cs]).to(gpu).reshape(b, v, h * w, 1, 1)
    op = torch.stack([c.opa for c in cs]).to(gpu).reshape(b, v, h * w, 1, 1)
    E, K, N, F = [], [], [], []
    for c in cs:
        per = []
        for j in range(centres):
            pose = torch.eye(4, device=gpu)
            pose[:3, 3] = c.ext[0, :3, 3].to(gpu) + 0.2 * j
            per.append(decoder.cube_cameras(pose, 0.1, 10.0))
        for lst, k in ((E, 0), (K, 1), (N, 2), (F, 3)):
            lst.append(torch.cat([p[k] for p in per]))
    E, K, N, F = (torch.stack(x) for x in (E, K, N, F))
    dec = decoder.DecoderSplattingFused(background_color=(0.0, 0.0, 0.0), shared_campos=None).to(gpu)
    mod = lazy.make_adapter_class(sh_rotation="native", lazy=lazy_on)(cfg).to(gpu)
    a = mod.forward("hm3d", ext[:, :, None, None, None], dep, op, raw, (h, w))
    flat = SimpleNamespace(means=rearrange(a.means, "b v r srf spp xyz -> b (v r srf spp) xyz"),
                           covariances=rearrange(a.covariances, "b v r srf spp i j -> b (v r srf spp) i j"),
                           harmonics=rearrange(a.harmonics, "b v r srf spp c d_sh -> b (v r srf spp) c d_sh"),
                           opacities=rearrange(1 * a.opacities, "b v r srf spp -> b (v r srf spp)"))
    bd = lazy.bundle_of(flat)
    assert (bd is not None) == lazy_on
    calls = []
    if monkeypatch is not None:
        real = rasterizer.rasterize_raw
        monkeypatch.setattr(rasterizer, "rasterize_raw", lambda *a_, **k_: calls.append(k_.get("raw_layout", "records")) or real(*a_, **k_))
    if measure:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
    out = dec(flat, E, K, N, F, (FW, FW))
    if measure:
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before
    st = rasterizer.last_state()
    assert bool(st.prm.flags & _lib.FLAG_RAW_INPUTS) == lazy_on and st.prm.M == d_sh
    if lazy_on:
        assert bd._materialised is None, "the fused decoder must render from the raw tensors without materialising the Gaussians"
    if not lazy_on:
        return out.color.detach(), None, calls
    up = torch.tensor(np.random.default_rng(6).standard_normal(tuple(out.color.shape)).astype(np.float32), device=gpu)
    out.color.backward(up)
    return out.color.detach(), leaf.grad, calls


@pytest.mark.parametrize("b", (1, 2))
@pytest.mark.parametrize("degree", (2, 4))
def test_the_seam_renders_from_the_convolutions_planes(gpu, monkeypatch, degree, b):
    assert degree in lazy.RAW_SEAM_DEGREES
    img, grad, calls = _seam(gpu, degree, b, monkeypatch=monkeypatch)
    want = "planes" if degree in lazy.RAW_PLANE_SEAM_DEGREES else "records"
    assert calls == [want] * b, "one render per batch element, from the planes in place"
    eager, _, _ = _seam(gpu, degree, b, lazy_on=False)
    assert torch.equal(_bits(img), _bits(eager)) and float(img.abs().max()) > 0
    assert grad.is_contiguous() and grad.shape == (2 * b, 2 + 7 + 3 * (degree + 1) ** 2, 9, 15)
    assert bool((_bits(grad[:, :2]) == 0).all()), "offset_xy channels of the leaf's gradient"
    img_r, grad_r, calls_r = _seam(gpu, degree, b, force_records=True, monkeypatch=monkeypatch)
    assert calls_r == ["records"] * b
    assert torch.equal(_bits(img), _bits(img_r)) and torch.equal(_bits(grad), _bits(grad_r))
    assert bool((grad[:, 2:] != 0).any())


def test_the_seam_sums_two_target_centres_and_falls_back_on_a_copy(gpu, monkeypatch):
    img, grad, calls = _seam(gpu, 4, 1, centres=2, monkeypatch=monkeypatch)
    assert calls == ["planes" if 4 in lazy.RAW_PLANE_SEAM_DEGREES else "records"] * 2
    img_r, grad_r, _ = _seam(gpu, 4, 1, centres=2, force_records=True, monkeypatch=monkeypatch)
    assert torch.equal(_bits(img), _bits(img_r)) and torch.equal(_bits(grad), _bits(grad_r)), "a two-term sum is order-free"
    monkeypatch.undo()
    img_c, grad_c, calls_c = _seam(gpu, 4, 1, centres=2, refuse=True, monkeypatch=monkeypatch)
    assert calls_c == ["records"] * 2
    assert torch.equal(_bits(img), _bits(img_c)) and torch.equal(_bits(grad), _bits(grad_c))


# ------------------------------------------------------------------------------------------------ (e) no copy
@pytest.mark.parametrize("degree", (2, 4))
def test_the_plane_route_holds_no_record_copy(gpu, monkeypatch, degree):
    """Peak allocated memory over the seam's forward, after one warm-up of each route: the record route holds bundle.raw[i].reshape(-1, C) —
    P (7 + 3 d_sh) floats — which the plane route never makes.  1 KiB: the caching allocator's 512-byte rounding of two blocks."""
    if degree not in lazy.RAW_PLANE_SEAM_DEGREES:
        monkeypatch.setattr(lazy, "RAW_PLANE_SEAM_DEGREES", tuple(lazy.RAW_PLANE_SEAM_DEGREES) + (degree,))
    _seam(gpu, degree, 1)
    planes = _seam(gpu, degree, 1, measure=True)
    monkeypatch.setattr(lazy, "raw_planes_of", lambda raw: None)
    _seam(gpu, degree, 1, lazy_on=True, force_records=True, monkeypatch=monkeypatch)
    records = _seam(gpu, degree, 1, force_records=True, monkeypatch=monkeypatch, measure=True)
    copy = 2 * 9 * 15 * (7 + 3 * (degree + 1) ** 2) * 4
    print(f"[rawplanes] degree {degree}: forward peak {planes} B (planes) / {records} B (records); record copy {copy} B")
    assert planes <= records - (copy - 1024), (planes, records, copy)


# ------------------------------------------------------------------------------------------------ (f) determinism
def test_two_plane_runs_give_the_same_bits(gpu):
    name, per_ray, with_rot, diff_means, off = PARAMS[0]
    s = _scene(gpu, 16, SHAPES[0], name, per_ray, with_rot, diff_means, off)
    planes = _to_planes(s.raw, s.h, s.w, per_ray, off)
    runs = []
    for _ in range(2):
        leaf = planes.clone().requires_grad_(True)
        run = _run(gpu, s, leaf, raw_layout="planes", raw_channel_offset=off)
        run.out["d_raw"] = _bits(leaf.grad)
        runs.append(run.out)
    assert set(runs[0]) == set(FORWARD_AND_STATE) | {"d_raw"}
    _compare(runs[0], runs[1])
