"""The S360Params a rasteriser call is launched with (rasterizer._params: no GPU) — the flag word of both autograd nodes for every
combination of options that changes it, M, the binning capacity, the pinned mirror's address and the segment storage.  The expected
flag words are written out from the values of S360_FLAG_* in include/s360.h (SHARED_CAMPOS 1, COV9 2, SH_CHANNEL_MAJOR 4, FORWARD_ONLY 8,
SH_DEG4_IGNORED 16, SPHERICAL 32, LEAN_LISTS 64, DEFER_LOSS 128, ATOMIC_GRADS 256, SPLIT_LISTS 512, RAW_INPUTS 1024, COOP_WALK 2048)."""
import itertools

import pytest
import torch

from splatter360_amd import rasterizer as R

P = 1000
_fresh = itertools.count(1)


@pytest.fixture(autouse=True)
def _switches(monkeypatch):
    monkeypatch.setattr(R, "DETERMINISTIC", False)
    monkeypatch.setattr(R, "SH_DEG4_IGNORED", False)
    monkeypatch.setattr(R, "COOP_WALK", "auto")


def _build(v=6, p=P, needs_bwd=True, target=False, fixed=0, sh=(P, 3, 25), **options):
    """_params on a hint key no other case uses (the height carries the case number's tile rows), with a plain tensor as its mirror."""
    options = dict(dict(h=16 * next(_fresh), w=64, lean=True, split_lists=False), **options)
    key = R._hint_key("cpu", p, v, options["h"], options["w"], options["lean"])
    for d in (R._CAPACITY_HINT, R._CHUNK_HINT, R._SPLIT_AGE, R._OVERFLOW_WARNED):
        d.pop(key, None)
    mirror = R._MIRRORS[key] = torch.tensor([-1, 0, -1], dtype=torch.int64)
    for k, val in options.pop("hints", {}).items():
        getattr(R, k)[key] = val
    prm = R._params("cpu", p, v, R._Options(**options), needs_bwd, target, fixed, sh)
    return prm, key, mirror


VIEWS = dict(sh_degree=4, shared_campos=True, cov9=True, sh_channel_major=True)
RAW = dict(fixed=1 | 1024, sh=25, sh_degree=4)


@pytest.mark.parametrize("flags,case", [
    (71, dict()),                                                           # training
    (79, dict(needs_bwd=False)),                                            # inference
    (71, dict(needs_bwd=False, keep_slots=True)),
    (199, dict(target=True, mse_defer=True)),
    (79, dict(target=True, mse_defer=True, needs_bwd=False)),               # nothing to defer the reduction to
    (583, dict(split_lists=True)),
    (327, dict(split_lists=True, atomic_grads=True)),                       # the atomic backward has no split instances
    (591, dict(split_lists=True, atomic_grads=True, needs_bwd=False)),
])
def test_views_node_flag_words(flags, case):
    assert _build(**VIEWS, **case)[0].flags == flags


def test_views_node_module_switches(monkeypatch):
    monkeypatch.setattr(R, "SH_DEG4_IGNORED", True)
    assert _build(**VIEWS)[0].flags == 87
    monkeypatch.setattr(R, "SH_DEG4_IGNORED", False)
    monkeypatch.setattr(R, "COOP_WALK", True)
    assert _build(**VIEWS)[0].flags == 2119


def test_atomic_grads_withholds_the_split_flag_but_not_the_segment_storage():
    prm, _, _ = _build(**VIEWS, split_lists=True, atomic_grads=True, hints={"_CHUNK_HINT": 7})
    assert prm.flags == 327 and prm.max_segments == 624


def test_spherical_mode_never_splits_and_one_view_shares_its_camera_centre():
    prm, _, _ = _build(v=2, sh_degree=4, cov9=True, sh_channel_major=True, spherical=True, split_lists=True)
    assert prm.flags == 102 and prm.max_segments == 0
    assert _build(v=1, lean=False, sh=(P, 1, 3))[0].flags == 1


@pytest.mark.parametrize("flags,case", [
    (1089, dict()),
    (1097, dict(needs_bwd=False)),
    (1601, dict(split_lists=True)),
    (1217, dict(target=True, mse_defer=True)),
])
def test_raw_node_flag_words(flags, case):
    prm = _build(**RAW, **case)[0]
    assert prm.flags == flags and (prm.sh_degree, prm.M) == (4, 25)


def test_coefficient_count_follows_the_layout_of_the_harmonics():
    assert _build(**VIEWS)[0].M == 25
    assert _build(sh=(P, 25, 3), sh_degree=4)[0].M == 25                    # point-major
    assert _build(p=0, sh=(0, 3, 0), sh_degree=4, sh_channel_major=True)[0].M == 25     # an empty cloud still states its degree's count
    assert _build(sh=None)[0].M == 0                                        # precomputed colours


@pytest.mark.parametrize("check", ["sync", "lazy"])
def test_capacity_and_mirror(check):
    prm, _, mirror = _build(**VIEWS, check=check)
    assert prm.max_instances == (3 * P * 6) // 2 + (1 << 18)                # a first call: the guess
    assert prm.header_mirror == mirror.data_ptr()
    assert _build(**VIEWS, check=check, max_instances=12345)[0].max_instances == 12345


def test_the_policies_run_once_per_call():
    options = dict(VIEWS, h=16 * next(_fresh), w=64, lean=True, split_lists="auto")
    key = R._hint_key("cpu", P, 6, options["h"], 64, True)
    R._MIRRORS[key] = torch.tensor([-1, 1, -1], dtype=torch.int64)          # a forward reported a quadrant worth splitting
    assert R._params("cpu", P, 6, R._Options(**options), True, False, 0, (P, 3, 25)).flags == 583 and R._SPLIT_AGE[key] == 0
    for _ in range(2):
        assert R._params("cpu", P, 6, R._Options(**options), True, False, 0, (P, 3, 25)).flags == 583
    assert R._SPLIT_AGE[key] == 2 and int(R._MIRRORS[key][1]) == 0
