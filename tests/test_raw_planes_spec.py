"""The plane layout of the raw-input path: what can be held without a GPU.

  * lazy.raw_planes_of on the reference's own three-step view chain over the last convolution's output [(v b), C, h, w]
    (depth_predictor_multiview_360.py:672-674 "(v b) c h w -> b v (h w) c"; encoder_costvolume.py:405-409 "... (srf c) -> ... srf c";
    :421-424 the [..., 2:] slice and the samples-per-pixel axis), built with einops at b = 1, 2 and srf = 1, 2 — and on every chain it
    must refuse;
  * rasterize_raw(raw_layout="planes")'s shape and layout errors, raised on CPU tensors before any device work;
  * the three *_planes entry points' S360_E_BADARG answers to a bad S360RawPlanes, through the binding table, with dummy host
    pointers that are never dereferenced.
"""
import ctypes as C

import pytest
import torch
from einops import rearrange

from splatter360_amd import _lib, lazy, rasterizer

OK, BADARG, WORKSPACE, UNSUPPORTED = 0, -1, -2, -4          # include/s360.h
V, H, W = 2, 9, 15


def _chain(conv, v, b, srf, drop=2):
    x = rearrange(conv, "(v b) c h w -> b v (h w) c", v=v, b=b)
    x = rearrange(x, "... (srf c) -> ... srf c", srf=srf)
    return rearrange(x[..., drop:], "b v r srf c -> b v r srf () c")


# ------------------------------------------------------------------------------------------------ the recogniser
@pytest.mark.parametrize("srf", (1, 2))
@pytest.mark.parametrize("b", (1, 2))
def test_raw_planes_of_recognises_the_reference_chain(b, srf):
    c_total = 84 * srf
    conv = torch.randn(V * b, c_total, H, W)
    raw = _chain(conv, V, b, srf)
    hw = H * W
    assert raw.shape == (b, V, hw, srf, 1, 82) and raw._base is conv and raw.storage_offset() == 2 * hw
    assert raw.stride(2) == 1 and raw.stride(5) == hw and (b == 1 or raw.stride(0) == c_total * hw) and raw.stride(1) == b * c_total * hw
    assert srf == 1 or raw.stride(3) == 84 * hw
    got = lazy.raw_planes_of(raw)
    assert got is not None and got.base is conv
    assert (got.channel_offset, got.surface_channels, got.view_stride) == (2, 84, b * c_total * hw)
    for i in range(b):
        el = got.element(i, b)
        assert el.shape == (V, c_total, H, W) and el.stride() == (b * c_total * hw, hw, W, 1) and el.data_ptr() == conv.data_ptr() + 4 * i * c_total * hw
        # the words the kernels address are the chain's own: word c of (view, ray, surface)
        want = raw[i, :, :, :, 0, :]                                                   # [v, r, srf, 82]
        mine = el.reshape(V, srf, 84, hw)[:, :, 2:].permute(0, 3, 1, 2)               # [v, r, srf, 82]
        assert torch.equal(want, mine)


def test_raw_planes_of_the_issues_own_figures():
    raw = _chain(torch.zeros(2, 84, 9, 15), 2, 1, 1)
    assert raw.shape == (1, 2, 135, 1, 1, 82) and (raw.stride(1), raw.stride(2), raw.stride(5)) == (11340, 1, 135) and raw.storage_offset() == 270
    assert lazy.raw_planes_of(raw).view_stride == 11340
    conv = torch.zeros(4, 84, 9, 15)
    got = lazy.raw_planes_of(_chain(conv, 2, 2, 1))
    assert got.view_stride == 22680 and got.element(1, 2).data_ptr() - conv.data_ptr() == 4 * 11340
    assert _chain(torch.zeros(2, 168, 9, 15), 2, 1, 2).stride(3) == 84 * 135


def test_raw_planes_of_takes_other_degrees_and_offsets():
    for d_sh in (1, 4, 9, 16, 25):
        for drop in (0, 2):
            conv = torch.zeros(V, drop + 7 + 3 * d_sh, H, W)
            got = lazy.raw_planes_of(_chain(conv, V, 1, 1, drop))
            assert got is not None and got.channel_offset == drop and got.surface_channels == drop + 7 + 3 * d_sh


@pytest.mark.parametrize("case", ["contiguous", "channels_last", "float64", "half", "spp_expand", "records", "strided_base", "short_slice", "permuted",
                                  "wrong_rank", "not_a_tensor", "batch_major"])
def test_raw_planes_of_refuses_everything_else(case):
    conv = torch.randn(V * 2, 84, H, W)
    if case == "contiguous":
        raw = _chain(conv, V, 2, 1).contiguous()
    elif case == "channels_last":
        raw = _chain(conv.contiguous(memory_format=torch.channels_last), V, 2, 1)
    elif case == "float64":
        raw = _chain(conv.double(), V, 2, 1)
    elif case == "half":
        raw = _chain(conv.half(), V, 2, 1)
    elif case == "spp_expand":
        raw = _chain(conv, V, 2, 1).expand(-1, -1, -1, -1, 3, -1)
    elif case == "records":
        raw = torch.randn(2, V, H * W, 1, 1, 82)
    elif case == "strided_base":
        raw = _chain(torch.randn(V * 2, 84, H, 2 * W)[..., ::2], V, 2, 1)
    elif case == "short_slice":         # the slice must run to the surface's last channel
        raw = _chain(conv, V, 2, 1)[..., :55]
    elif case == "permuted":
        raw = _chain(conv, V, 2, 1).transpose(0, 1)
    elif case == "wrong_rank":
        raw = _chain(conv, V, 2, 1)[:, :, :, :, 0]
    elif case == "not_a_tensor":
        raw = None
    else:                               # "(b v)" instead of "(v b)": another tensor's layout
        x = rearrange(conv, "(b v) c h w -> b v (h w) c", v=V, b=2)
        raw = rearrange(rearrange(x, "... (srf c) -> ... srf c", srf=1)[..., 2:], "b v r srf c -> b v r srf () c")
    assert lazy.raw_planes_of(raw) is None


def test_raw_planes_of_ignores_strides_of_size_one_dimensions():
    conv = torch.randn(V, 84, H, W)
    raw = _chain(conv, V, 1, 1)
    odd = raw.as_strided(raw.shape, (7, raw.stride(1), 1, 3, 5, raw.stride(5)), raw.storage_offset())      # b, srf and spp have size 1
    assert odd._base is not None and torch.equal(odd, raw)
    got = lazy.raw_planes_of(odd)
    assert got is not None and got.view_stride == 84 * H * W


# ------------------------------------------------------------------------------------------------ rasterize_raw's errors
def _call(raw, per_ray=1, n=V, **kw):
    g = n * H * W * per_ray
    return rasterizer.rasterize_raw(torch.ones(g), torch.ones(g), raw, torch.eye(4).repeat(n, 1, 1), views=torch.zeros(6, 44), image_height=32, image_width=32,
                                    context_shape=(H, W), scale_min=0.5, scale_max=15.0, per_ray=per_ray, **kw)


def test_rasterize_raw_plane_errors_come_before_any_device_work():
    pl = dict(raw_layout="planes")
    with pytest.raises(ValueError, match="raw_layout"):
        _call(torch.zeros(V, 84, H, W), raw_layout="nchw")
    with pytest.raises(ValueError, match="raw_channel_offset"):
        _call(torch.zeros(V * H * W, 82), raw_channel_offset=2)
    with pytest.raises(RuntimeError, match=r"\[2, C, 9, 15\]"):
        _call(torch.zeros(V * H * W, 82), **pl)
    with pytest.raises(RuntimeError, match=r"\[2, C, 9, 15\]"):
        _call(torch.zeros(V, 82, W, H), **pl)
    with pytest.raises(RuntimeError, match=r"\[2, C, 9, 15\]"):
        _call(torch.zeros(3, 82, H, W), **pl)
    with pytest.raises(RuntimeError, match=r"83 channels.*10, 19, 34, 55, 82"):
        _call(torch.zeros(V, 83, H, W), **pl)
    with pytest.raises(RuntimeError, match=r"82 channels.*12, 21, 36, 57, 84"):
        _call(torch.zeros(V, 82, H, W), raw_channel_offset=2, **pl)
    with pytest.raises(RuntimeError, match=r"84 channels.*24, 42, 72, 114, 168"):
        _call(torch.zeros(V, 84, H, W), per_ray=2, raw_channel_offset=2, **pl)
    with pytest.raises(RuntimeError, match="float32"):
        _call(torch.zeros(V, 84, H, W, dtype=torch.float64), raw_channel_offset=2, **pl)
    with pytest.raises(RuntimeError, match="in place"):
        _call(torch.zeros(V, 84, H, W).contiguous(memory_format=torch.channels_last), raw_channel_offset=2, **pl)
    with pytest.raises(RuntimeError, match="in place"):
        _call(torch.zeros(1, 84, H, W).expand(V, -1, -1, -1), raw_channel_offset=2, **pl)
    with pytest.raises(RuntimeError, match="in place"):
        _call(torch.zeros(V, 84, H, 2 * W)[..., ::2], raw_channel_offset=2, **pl)
    with pytest.raises(RuntimeError, match="raw_channel_offset"):
        _call(torch.zeros(V, 84, H, W), raw_channel_offset=-1, **pl)
    with pytest.raises(RuntimeError, match=r"sh_rotation must be \[2, 25, 25\]"):
        _call(torch.zeros(V, 84, H, W), raw_channel_offset=2, sh_rotation=torch.zeros(V, 9, 9), **pl)
    # a well-formed call gets as far as the device check: the rasteriser has no CPU path
    for raw in (torch.zeros(V, 84, H, W), torch.zeros(V, 2, 84, H, W)[:, 1]):
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            _call(raw, raw_channel_offset=2, **pl)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        _call(torch.zeros(V, 168, H, W), per_ray=2, raw_channel_offset=2, **pl)


# ------------------------------------------------------------------------------------------------ the entries' answers
def _answers(planes, per_ray=1, degree=4, h=H, w=W):
    """The three plane entries for a consistent S360Params / S360RawInputs pair (P = 2 h w per_ray) and dummy non-null host pointers:
    nothing is launched or dereferenced before the strides are judged.  The tail entry is given a workspace of 0 bytes, so a strides
    struct that passes gets S360_E_WORKSPACE from it — still before any GPU work."""
    lib = _lib.lib()
    m = (degree + 1) ** 2
    prm = _lib.S360Params()
    prm.P, prm.V, prm.H, prm.W, prm.sh_degree, prm.M = 2 * h * w * per_ray, 1, 32, 32, degree, m
    prm.flags = _lib.FLAG_RAW_INPUTS | _lib.FLAG_SHARED_CAMPOS
    prm.max_instances = 64
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    raw = _lib.S360RawInputs(p.value, p.value, p.value, None, 2, h * w * per_ray, h, w, per_ray, 0, 0.5, 15.0, 1e-8)
    pl = None if planes is None else C.byref(_lib.S360RawPlanes(*planes))
    tail = lib.s360_backward_raw_tail_planes(C.byref(prm), p, 1, C.byref(raw), pl, p, p, 0, None, p, p, p, p, None)
    if tail != BADARG:
        return tail
    fwd = lib.s360_forward_raw_planes(C.byref(prm), p, C.byref(raw), pl, p, p, p, p, None, 0, None, None, 0.0, None, None, None, p, 256, None)
    bwd = lib.s360_backward_raw_planes(C.byref(prm), p, C.byref(raw), pl, p, p, p, p, 256, p, None, None, 0, 0, p, p, p, p, p, p, p, 256, None)
    assert fwd == bwd == tail
    return tail


def test_plane_entries_judge_the_strides_before_any_gpu_work():
    hw = H * W
    assert _answers(None) == BADARG                                            # a null strides struct
    assert _answers((84 * hw, 0, hw)) == WORKSPACE                             # the reference's own: past the stride checks
    assert _answers((82 * hw, 0, hw)) == WORKSPACE                             # no offset channels: the tightest view stride
    assert _answers((82 * hw - 1, 0, hw)) == BADARG                            # view_stride too small for one surface
    assert _answers((84 * hw, 0, hw - 1)) == BADARG                            # channel_stride < H W
    assert _answers((82 * hw + 81, 0, hw + 1)) == WORKSPACE                    # padded planes: 81 strides and the last plane
    assert _answers((82 * hw + 80, 0, hw + 1)) == BADARG
    assert _answers((84 * hw, -5, hw)) == WORKSPACE                            # per_ray = 1: the surface stride is not looked at
    # per_ray = 2
    assert _answers((168 * hw, 84 * hw, hw), per_ray=2) == WORKSPACE
    assert _answers((168 * hw, 82 * hw, hw), per_ray=2) == WORKSPACE
    assert _answers((168 * hw, 82 * hw - 1, hw), per_ray=2) == BADARG          # surface_stride < (7 + 3 M) channel_stride
    assert _answers((84 * hw + 82 * hw - 1, 84 * hw, hw), per_ray=2) == BADARG  # view_stride too small for two surfaces
    assert _answers((84 * hw + 82 * hw, 84 * hw, hw), per_ray=2) == WORKSPACE
    # every degree: the record's own width decides
    for degree in range(5):
        width = 7 + 3 * (degree + 1) ** 2
        assert _answers((width * hw, 0, hw), degree=degree) == WORKSPACE and _answers((width * hw - 1, 0, hw), degree=degree) == BADARG


def test_plane_entries_keep_the_record_entries_degree_rule_and_the_abi():
    lib = _lib.lib()
    prm = _lib.S360Params()
    prm.P, prm.V, prm.H, prm.W, prm.sh_degree, prm.M = 4, 1, 32, 32, 2, 10
    prm.flags = _lib.FLAG_RAW_INPUTS | _lib.FLAG_SHARED_CAMPOS
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    raw, pl = _lib.S360RawInputs(), _lib.S360RawPlanes(1, 1, 1)
    assert lib.s360_backward_raw_tail_planes(C.byref(prm), p, 1, C.byref(raw), C.byref(pl), p, p, 0, None, p, p, p, p, None) == UNSUPPORTED
    assert lib.s360_forward_raw_planes(C.byref(prm), p, C.byref(raw), C.byref(pl), p, p, p, p, None, 0, None, None, 0.0, None, None, None, p, 256, None) == UNSUPPORTED
    assert _lib.ABI_VERSION == 25 and lib.s360_abi_version() == 25
    assert C.sizeof(_lib.S360RawPlanes) == 24 and C.sizeof(_lib.S360RawInputs) == 72
