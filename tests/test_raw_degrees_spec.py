"""The raw-input path at SH degrees 0..4: what can be held without a GPU.  The three entry points (s360_forward_raw, s360_backward_raw,
s360_backward_raw_tail) check their arguments before any launch, so their answers to a degree / coefficient-count pair are read on
the CPU with dummy host pointers that are never dereferenced; rasterize_raw's shape errors and lazy.bundle_of are pure Python.

The degree rule (csrc/s360_device.h: s360_raw_degree_check, at the place of the former `M != 25 || sh_degree != 4`):
  sh_degree outside 0..4            -> S360_E_UNSUPPORTED
  M >  (sh_degree + 1)^2            -> S360_E_UNSUPPORTED   (an active degree below the stored one: the general path's feature)
  M <  (sh_degree + 1)^2            -> S360_E_BADARG        (s360_forward's own rule: the degree needs coefficients that are not there)
  M == (sh_degree + 1)^2            -> the call goes on to its next check
"""
import ctypes as C
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch
from einops import rearrange

from splatter360_amd import _lib, lazy, rasterizer

BADARG, UNSUPPORTED = -1, -4          # include/s360.h
HEADER = (Path(__file__).resolve().parent.parent / "include" / "s360.h").read_text()


def _answers(m, degree):
    """The three entry points' return codes for P = 4 with valid flags, a zeroed S360RawInputs (extrinsics == NULL, n_views * per_view
    = 0 != P) and non-null dummy pointers everywhere else: nothing is launched, nothing is dereferenced."""
    lib = _lib.lib()
    prm = _lib.S360Params()
    prm.P, prm.V, prm.H, prm.W, prm.sh_degree, prm.M = 4, 1, 32, 32, degree, m
    prm.flags = _lib.FLAG_RAW_INPUTS | _lib.FLAG_SHARED_CAMPOS
    prm.max_instances = 64
    raw = _lib.S360RawInputs()
    assert not raw.extrinsics and raw.n_views == 0 and raw.per_view == 0
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    fwd = lib.s360_forward_raw(C.byref(prm), p, C.byref(raw), p, p, p, p, None, 0, None, None, 0.0, None, None, None, p, 256, None)
    bwd = lib.s360_backward_raw(C.byref(prm), p, C.byref(raw), p, p, p, p, 256, p, None, None, 0, 0, p, p, p, p, p, p, p, 256, None)
    tail = lib.s360_backward_raw_tail(C.byref(prm), p, 1, C.byref(raw), p, p, 256, None, p, p, p, p, None)
    return fwd, bwd, tail


def test_a_lower_degree_with_its_own_coefficient_count_passes_the_degree_check():
    """M = 9 at degree 2 used to be S360_E_UNSUPPORTED; now the call reaches the next check (extrinsics == NULL / n_views * per_view
    != P: S360_E_BADARG).  Every degree 0..4 with M = (degree + 1)^2 does."""
    assert _answers(9, 2) == (BADARG, BADARG, BADARG)
    for degree in range(5):
        assert _answers((degree + 1) ** 2, degree) == (BADARG, BADARG, BADARG), degree


@pytest.mark.parametrize("m,degree,want", [(9, 4, BADARG), (10, 2, UNSUPPORTED), (25, 3, UNSUPPORTED), (25, 5, UNSUPPORTED), (36, 5, UNSUPPORTED),
                                            (1, -1, UNSUPPORTED), (0, 0, BADARG)])
def test_degree_and_coefficient_count_that_do_not_match(m, degree, want):
    assert _answers(m, degree) == (want, want, want)


def test_abi_version_is_unchanged_and_the_header_states_the_general_shapes():
    assert _lib.ABI_VERSION == 25 and _lib.lib().s360_abi_version() == 25 and "#define S360_ABI_VERSION 25" in HEADER
    for text in ("raw_gaussians [P, 7 + 3*M]", "sh_rotation [n_views, M, M]", "d_raw_gaussians [P, 7 + 3*M]"):
        assert text in HEADER, text
    assert "[n_views*per_view, 82]" not in HEADER and "[n_views,25,25]" not in HEADER and "d_raw_gaussians[P,82]" not in HEADER


def _raw_call(width, rot_shape=None, n=2, h=2, w=3):
    g = n * h * w
    views = torch.zeros(6, 44)
    rot = None if rot_shape is None else torch.zeros(rot_shape)
    return rasterizer.rasterize_raw(torch.ones(g), torch.ones(g), torch.zeros(g, width), torch.eye(4).repeat(n, 1, 1), views=views, image_height=32,
                                    image_width=32, context_shape=(h, w), scale_min=0.5, scale_max=15.0, sh_rotation=rot)


def test_rasterize_raw_names_the_allowed_record_widths():
    with pytest.raises(RuntimeError, match=r"33 floats.*10, 19, 34, 55, 82"):
        _raw_call(33)
    for width in (7, 9, 35, 81, 83, 109):
        with pytest.raises(RuntimeError, match="allowed widths"):
            _raw_call(width)


def test_rasterize_raw_rejects_a_rotation_of_another_degree():
    with pytest.raises(RuntimeError, match=r"sh_rotation must be \[2, 9, 9\]"):
        _raw_call(34, (2, 25, 25))
    with pytest.raises(RuntimeError, match=r"sh_rotation must be \[2, 25, 25\]"):
        _raw_call(82, (3, 25, 25))
    # a matching pair passes the shape checks and reaches the device check (these are CPU tensors: the product has no CPU path)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        _raw_call(34, (2, 9, 9))


class _StubModule:
    """tests/test_lazy_fields.py's stand-in for the adapter instance."""

    def rotation_blocks(self, ext):
        return None


@pytest.mark.parametrize("degree", [0, 1, 2, 3, 4])
def test_bundle_of_reads_d_sh_from_the_bundle(degree):
    d_sh = (degree + 1) ** 2
    b, v, r = 2, 2, 6
    depths, op = torch.rand(b, v, r, 1, 1), torch.rand(b, v, r, 1, 1)
    bd = lazy.RawBundle(_StubModule(), "hm3d", torch.eye(4).expand(b, v, 4, 4).contiguous(), depths, op, torch.randn(b, v, r, 1, 1, 7 + 3 * d_sh), (2, 3), 1e-8)
    assert bd.d_sh == d_sh
    sh5 = (b, v, r, 1, 1)
    f = lambda name, tail: lazy.LazyField(bd, name, sh5 + tail)
    flat = SimpleNamespace(means=rearrange(f("means", (3,)), "b v r srf spp xyz -> b (v r srf spp) xyz"),
                           covariances=rearrange(f("covariances", (3, 3)), "b v r srf spp i j -> b (v r srf spp) i j"),
                           harmonics=rearrange(f("harmonics", (3, d_sh)), "b v r srf spp c d_sh -> b (v r srf spp) c d_sh"),
                           opacities=rearrange(1 * op, "b v r srf spp -> b (v r srf spp)"))
    assert lazy.bundle_of(flat) is bd and lazy.bundle_of(flat, d_sh) is bd
    assert lazy.bundle_of(flat, 25 if d_sh != 25 else 16) is None
    wrong = SimpleNamespace(**{**vars(flat), "harmonics": rearrange(f("harmonics", (3, d_sh + 1)), "b v r srf spp c d_sh -> b (v r srf spp) c d_sh")})
    assert lazy.bundle_of(wrong) is None


def test_the_seam_table_is_one_named_constant_of_known_degrees():
    assert isinstance(lazy.RAW_SEAM_DEGREES, tuple) and set(lazy.RAW_SEAM_DEGREES) <= {0, 1, 2, 3, 4} and 4 in lazy.RAW_SEAM_DEGREES
    assert rasterizer.RAW_D_SH == (1, 4, 9, 16, 25)
