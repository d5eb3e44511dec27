"""Loader / builder of the C-ABI shared library libs360.so (include/s360.h).

The product path has NO fallback: if the HIP library is missing or cannot be loaded, every
operator raises.  `build()` cross-compiles for gfx950 with hipcc (works without a GPU).
"""
from __future__ import annotations

import ctypes as C
import os
import shutil
import subprocess
from pathlib import Path

_PKG = Path(__file__).resolve().parent
_CSRC = _PKG / "csrc"
LIB_PATH = _PKG / "libs360.so"
SOURCES = ("s360_forward.hip", "s360_backward.hip", "s360_backward_em.hip", "s360_stitch.hip", "s360_views.hip", "s360_adapter.hip", "s360_metrics.hip",
           "s360_depth_loss.hip", "s360_eval_scores.hip", "s360_cost_volume.hip", "s360_depth_head.hip", "s360_depth_tail.hip", "s360_equirec2cube.hip", "s360_visualize.hip",
           "s360_depth_smooth.hip", "s360_window_attention.hip", "s360_group_norm.hip", "s360_qkv_attention.hip",
           "s360_transformer_ffn.hip", "s360_mono_fusion.hip")
# per-source extra flags (s360_backward_em.hip: see the launcher comment in csrc/s360_bwd_em.h)
SOURCE_FLAGS = {"s360_backward_em.hip": ("-fno-slp-vectorize",)}
HIPCC_FLAGS = ("--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wno-unused-result")

S360_MAX_VIEWS = 8
FLAG_SHARED_CAMPOS = 1
FLAG_COV9 = 2
FLAG_SH_CHANNEL_MAJOR = 4
FLAG_FORWARD_ONLY = 8
FLAG_SH_DEG4_IGNORED = 16
FLAG_SPHERICAL = 32
FLAG_LEAN_LISTS = 64
FLAG_DEFER_LOSS = 128
FLAG_ATOMIC_GRADS = 256
FLAG_SPLIT_LISTS = 512
FLAG_RAW_INPUTS = 1024
FLAG_COOP_WALK = 2048
DS_SECOND = 1        # s360_depth_smooth_*: flags
DS_BILATERAL = 2
GN_ACT_NONE, GN_ACT_RELU, GN_ACT_SILU, GN_ACT_GELU = 0, 1, 2, 3   # s360_group_norm_*: activation
QKV_LEGACY, QKV_NEW = 0, 1                                        # s360_qkv_attention_*: order
ABI_VERSION = 25


class S360Params(C.Structure):
    _fields_ = [("P", C.c_int32), ("V", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("sh_degree", C.c_int32), ("M", C.c_int32), ("flags", C.c_uint32),
                ("max_instances", C.c_uint32), ("max_segments", C.c_uint32), ("_reserved", C.c_uint32),
                ("header_mirror", C.c_void_p)]


class S360Layout(C.Structure):
    _fields_ = [(n, C.c_size_t) for n in (
        "total_bytes", "header", "tiles_touched", "vis_mask", "slot_base", "rec_a", "rec_b", "rec_c",
        "clamped", "depths", "tile_count", "slot_ticket", "merge_done", "seg_flag", "seg_arrive", "seg_arrive2", "tile_start", "tile_cursor", "chunk_start", "tile_order", "keys", "keys_alt", "list", "final_T", "n_contrib",
        "tile_max_contrib", "strip_last", "slot_pair", "long_pairs", "rgbc", "sh_jac", "surv", "surv_count", "part_c", "part_t", "part_e", "part_l", "part_n", "seg_c", "seg_t", "seg_cnt", "seg_info", "geo7", "backward_bytes")]


class S360RawInputs(C.Structure):
    """include/s360.h S360RawInputs: the encoder's raw per-pixel outputs (device pointers)."""
    _fields_ = [("extrinsics", C.c_void_p), ("depths", C.c_void_p), ("raw_gaussians", C.c_void_p), ("sh_rotation", C.c_void_p),
                ("n_views", C.c_int32), ("per_view", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("per_ray", C.c_int32),
                ("erp_convention", C.c_int32), ("scale_min", C.c_float), ("scale_max", C.c_float), ("eps", C.c_float)]


class S360RawPlanes(C.Structure):
    """include/s360.h S360RawPlanes: where the raw words lie as channel planes (strides in floats)."""
    _fields_ = [("view_stride", C.c_int64), ("surface_stride", C.c_int64), ("channel_stride", C.c_int64)]


_int, _i32, _i64, _sz, _f32, _vp = C.c_int, C.c_int32, C.c_int64, C.c_size_t, C.c_float, C.c_void_p
_prm, _raw, _pln = C.POINTER(S360Params), C.POINTER(S360RawInputs), C.POINTER(S360RawPlanes)
_p32, _p64, _psz, _pf64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_size_t), C.POINTER(C.c_double)

# Every function include/s360.h declares: name -> (restype, argtypes).  lib() applies it; tests/test_abi.py holds it to the header.
SIGNATURES = {
    "s360_abi_version": (_int, []),
    "s360_error_string": (C.c_char_p, [_int]),
    "s360_layout": (_int, [_prm, C.POINTER(S360Layout)]),
    "s360_forward": (_int, [_prm] + [_vp] * 9 + [_sz, _vp]),
    "s360_forward_depth": (_int, [_prm] + [_vp] * 8 + [_i32, _vp, _vp, _sz, _vp]),
    "s360_forward_mse": (_int, [_prm] + [_vp] * 8 + [_i32, _vp, _vp, _f32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "s360_backward": (_int, [_prm] + [_vp] * 7 + [_sz] + [_vp] * 3 + [_i32] + [_vp] * 7 + [_sz, _vp]),
    "s360_backward_split": (_int, [_prm] + [_vp] * 6 + [_sz] + [_vp] * 3 + [_i32] + [_vp] * 6 + [_sz, _vp]),
    "s360_backward_composite": (_int, [_prm, _vp, _vp, _sz, _vp, _vp, _vp, _i32, _vp, _sz, _vp]),
    "s360_backward_gaussians": (_int, [_prm, _vp, _vp, _vp, _vp, _vp, _sz, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "s360_backward_pair_records": (_int, [_prm, _vp, _sz, _psz]),
    "s360_reduce_unpack_gradients": (_int, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "s360_unpack_gradients": (_int, [_vp, _i32, _i32, _vp, _vp, _vp, _vp]),
    "s360_sh_backward": (_int, [_prm, _i32] + [_vp] * 5),
    "s360_forward_raw": (_int, [_prm, _vp, _raw] + [_vp] * 5 + [_i32, _vp, _vp, _f32] + [_vp] * 4 + [_sz, _vp]),
    "s360_backward_raw_tail": (_int, [_prm, _vp, _i32, _raw, _vp, _vp, _sz] + [_vp] * 6),
    "s360_backward_raw": (_int, [_prm, _vp, _raw] + [_vp] * 4 + [_sz] + [_vp] * 3 + [_i32, _i32] + [_vp] * 7 + [_sz, _vp]),
    "s360_forward_raw_planes": (_int, [_prm, _vp, _raw, _pln] + [_vp] * 5 + [_i32, _vp, _vp, _f32] + [_vp] * 4 + [_sz, _vp]),
    "s360_backward_raw_planes": (_int, [_prm, _vp, _raw, _pln] + [_vp] * 4 + [_sz] + [_vp] * 3 + [_i32, _i32] + [_vp] * 7 + [_sz, _vp]),
    "s360_backward_raw_tail_planes": (_int, [_prm, _vp, _i32, _raw, _pln, _vp, _vp, _sz] + [_vp] * 6),
    "s360_pack_views": (_int, [_vp] * 5 + [_i32, _i32, _i32, _vp, _vp]),
    "s360_adapter_forward": (_int, [_vp] * 4 + [_i32] * 6 + [_f32] * 3 + [_vp, _vp, _i32, _vp, _vp, _vp, _i32, _vp]),
    "s360_adapter_backward": (_int, [_vp] * 4 + [_i32] * 6 + [_f32] * 3 + [_vp, _vp, _i32, _vp, _vp, _vp, _i32, _vp]),
    "s360_sh_rotation_blocks": (_int, [_vp, _i32, _i32, _i32, _vp, _vp]),
    "s360_cube2erp_forward": (_int, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _p32, _p64, _vp]),
    "s360_cube2erp_backward": (_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _p32, _p64, _vp]),
    "s360_ssim": (_int, [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _psz, _vp]),
    "s360_erode": (_int, [_vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "s360_l1_sphere_forward": (_int, [_vp] * 4 + [_i32] * 5 + [_vp, _f32, _f32, _i32, _vp, _vp, _vp, _psz, _vp]),
    "s360_l1_sphere_backward": (_int, [_vp] * 4 + [_i32] * 5 + [_vp, _f32, _f32, _i32] + [_vp] * 5),
    "s360_depth_metrics": (_int, [_vp] * 3 + [_i32, _i32] + [_sz] * 3 + [_i32, _sz, _sz, _f32] + [_i32] * 5 + [_vp] * 4 + [_psz, _vp]),
    "s360_psnr": (_int, [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _psz, _vp]),
    "s360_cost_volume_forward": (_int, [_vp] * 5 + [_i32] * 8 + [_f32, _vp, _vp, _psz, _vp]),
    "s360_cost_volume_backward": (_int, [_vp] * 5 + [_i32] * 8 + [_f32, _vp, _vp, _vp, _vp, _psz, _vp]),
    "s360_cost_volume_warp": (_int, [_vp] * 4 + [_i32] * 7 + [_vp, _vp]),
    "s360_depth_head_forward": (_int, [_vp, _vp] + [_i32] * 4 + [_vp] * 5),
    "s360_depth_head_backward": (_int, [_vp] * 7 + [_i32] * 4 + [_vp, _vp]),
    "s360_upsample_forward": (_int, [_vp, _vp] + [_i32] * 6 + [_vp]),
    "s360_upsample_backward": (_int, [_vp] * 3 + [_i32] * 6 + [_vp]),
    "s360_depth_tail_forward": (_int, [_vp] * 4 + [_f32, _i32, _i32] + [_vp] * 3 + [_i32] * 3 + [_vp]),
    "s360_depth_tail_backward": (_int, [_vp] * 7 + [_f32, _i32, _i32, _vp, _vp] + [_i32] * 3 + [_vp]),
    "s360_opacity_map_forward": (_int, [_vp, _vp, _sz, _f32, _vp]),
    "s360_opacity_map_backward": (_int, [_vp, _vp, _vp, _sz, _f32, _vp]),
    "s360_erp2cube_forward": (_int, [_vp] * 4 + [_i32] * 8 + [_p32, _p64, _vp]),
    "s360_erp2cube_backward": (_int, [_vp] * 6 + [_i32] * 7 + [_p32, _p64, _vp]),
    "s360_depth_to_distance_forward": (_int, [_vp] * 3 + [_i32] * 4 + [_vp]),
    "s360_depth_to_distance_backward": (_int, [_vp] * 4 + [_i32] * 4 + [_vp]),
    "s360_cube2erp_distance_forward": (_int, [_vp] * 4 + [_i32] * 5 + [_p32, _p64, _vp]),
    "s360_cube2erp_distance_backward": (_int, [_vp] * 7 + [_i32] * 5 + [_p32, _p64, _vp]),
    "s360_depth_colormap": (_int, [_vp, _i32, _i32, _i32, _sz, _vp, _vp, _vp, _vp, _psz, _vp]),
    "s360_colorize": (_int, [_vp, _sz, _sz, _i32, _i32, _vp, _vp, _vp]),
    "s360_prep_image": (_int, [_vp] + [_i32] * 4 + [_vp, _vp]),
    "s360_error_map": (_int, [_vp, _vp, _i32, _i32, _vp, _vp]),
    "s360_depth_smooth_forward": (_int, [_vp] * 4 + [_i32] * 6 + [_f32, _i32, _vp, _vp, _psz, _vp]),
    "s360_depth_smooth_backward": (_int, [_vp] * 4 + [_i32] * 6 + [_f32, _i32, _vp, _vp, _vp]),
    "s360_window_attention_forward": (_int, [_vp] * 3 + [_i32] * 8 + [_vp] * 3),
    "s360_window_attention_backward": (_int, [_vp] * 5 + [_i32] * 8 + [_vp] * 5),
    "s360_window_attention_high_scratch_bytes": (_sz, [_i32] * 7),
    "s360_window_attention_high_forward": (_int, [_vp] * 3 + [_i32] * 8 + [_vp] * 3 + [_sz, _vp]),
    "s360_window_attention_high_backward": (_int, [_vp] * 5 + [_i32] * 8 + [_vp] * 5 + [_sz, _vp]),
    "s360_group_norm_scratch_doubles": (_sz, [_i32, _i32, _i64]),
    "s360_group_norm_forward": (_int, [_vp] * 4 + [_i32, _i32, _sz, _i32, _pf64, _i32] + [_vp] * 4),
    "s360_group_norm_backward": (_int, [_vp] * 5 + [_i32, _i32, _sz, _i32, _pf64, _i32] + [_vp] * 5),
    "s360_qkv_attention_forward": (_int, [_vp] + [_i32] * 6 + [_vp] * 3),
    "s360_qkv_attention_backward": (_int, [_vp] * 3 + [_i32] * 6 + [_vp] * 3),
    "s360_qkv_attention_high_scratch_bytes": (_sz, [_i32] * 6),
    "s360_qkv_attention_high_forward": (_int, [_vp] + [_i32] * 6 + [_vp] * 3 + [_sz, _vp]),
    "s360_qkv_attention_high_backward": (_int, [_vp] * 3 + [_i32] * 6 + [_vp] * 3 + [_sz, _vp]),
    "s360_ffn_tail_scratch_bytes": (_sz, [_i32]),
    "s360_ffn_tail_weight_chunks": (_int, [_i32]),
    "s360_ffn_tail_forward": (_int, [_vp] * 8 + [_i32] * 3 + [_pf64] + [_vp] * 4),
    "s360_ffn_tail_backward": (_int, [_vp] * 11 + [_i32] * 3 + [_pf64, _vp, _sz] + [_vp] * 9),
    "s360_ffn_tail_high_scratch_bytes": (_sz, [_i32, _i32]),
    "s360_ffn_tail_high_forward": (_int, [_vp] * 8 + [_i32] * 3 + [_pf64] + [_vp] * 4 + [_sz, _vp]),
    "s360_ffn_tail_high_backward": (_int, [_vp] * 11 + [_i32] * 3 + [_pf64, _vp, _sz] + [_vp] * 9),
    "s360_layer_norm_residual_forward": (_int, [_vp] * 4 + [_i32, _i32, _pf64] + [_vp] * 3),
    "s360_layer_norm_residual_backward": (_int, [_vp] * 4 + [_i32, _i32, _vp, _sz] + [_vp] * 5),
    "s360_mono_fusion_scratch_bytes": (_sz, [_i32, _i32]),
    "s360_mono_fusion_weight_chunks": (_int, [_i32]),
    "s360_mono_fusion_forward": (_int, [_vp] * 7 + [_i32] * 6 + [_pf64] + [_vp] * 4),
    "s360_mono_fusion_backward": (_int, [_vp] * 10 + [_i32] * 6 + [_pf64, _vp, _sz] + [_vp] * 6),
    "s360_mono_fusion_high_scratch_bytes": (_sz, [_i32, _i32, _i32]),
    "s360_mono_fusion_high_forward": (_int, [_vp] * 7 + [_i32] * 6 + [_pf64] + [_vp] * 4 + [_sz, _vp]),
    "s360_mono_fusion_high_backward": (_int, [_vp] * 10 + [_i32] * 6 + [_pf64, _vp, _sz] + [_vp] * 6),
    "s360_count_backward_slots": (_int, [_prm, _vp, _sz, _vp, _vp]),
    "s360_count_contributions": (_int, [_prm, _vp, _sz, _vp, _vp]),
    "s360_profile_slots": (_int, []),
    "s360_profile_slot_name": (C.c_char_p, [_int]),
    "s360_profile_enable": (_int, [_int]),
    "s360_profile_collect": (_int, [C.POINTER(_f32), _p32]),
}
EXPORTS = tuple(SIGNATURES)


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and Path(cand).exists():
            return cand
    raise RuntimeError("hipcc not found; cannot build libs360.so")


def needs_build() -> bool:
    if not LIB_PATH.exists():
        return True
    t = LIB_PATH.stat().st_mtime
    return any(d.stat().st_mtime > t for d in _dep_files())


def _dep_files():
    """Every file the library is compiled from: csrc/*.hip, csrc/*.h, include/*.h."""
    return sorted(list(_CSRC.glob("*.hip")) + list(_CSRC.glob("*.h")) + list((_PKG.parent / "include").glob("*.h")))


def source_hash() -> str:
    """sha256 (first 16 hex digits) over the kernel sources: stamps profiles/pmc_latest.json so that bench.py only
    quotes counter traffic collected from THIS code."""
    import hashlib
    h = hashlib.sha256()
    for f in _dep_files():
        h.update(f.name.encode())
        h.update(f.read_bytes())
    return h.hexdigest()[:16]


def build(force: bool = False, verbose: bool = False, out: Path = None, extra=()) -> Path:
    """hipcc --offload-arch=gfx950 ... -> splatter360_amd/libs360.so (in-tree), or -> `out` (objects beside it) with the further
    compiler flags `extra` — a schedule variant of the same sources (tests/test_gpu_split_parity.py builds one into a temporary
    directory)."""
    target = LIB_PATH if out is None else Path(out)
    if out is None and not force and not needs_build():
        return LIB_PATH
    extra = [*os.environ.get("S360_HIPCC_EXTRA", "").split(), *extra]
    from concurrent.futures import ThreadPoolExecutor
    objdir = _PKG / "build" if out is None else target.parent / "build"
    objdir.mkdir(parents=True, exist_ok=True)

    def compile_one(src: str):
        obj = objdir / (src + ".o")
        cmd = [_hipcc(), *HIPCC_FLAGS, *SOURCE_FLAGS.get(src, ()), *extra, "-c", str(_CSRC / src), "-o", str(obj)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        return obj, cmd, r

    with ThreadPoolExecutor(max_workers=len(SOURCES)) as pool:
        results = list(pool.map(compile_one, SOURCES))
    for obj, cmd, r in results:
        if verbose or r.returncode:
            print(" ".join(cmd))
            print(r.stdout, r.stderr)
        if r.returncode:
            raise RuntimeError("hipcc failed building libs360.so:\n" + r.stderr[-4000:])
    cmd = [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", *[str(o) for o, _, _ in results], "-o", str(target)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if verbose or r.returncode:
        print(" ".join(cmd))
        print(r.stdout, r.stderr)
    if r.returncode:
        raise RuntimeError("hipcc failed linking libs360.so:\n" + r.stderr[-4000:])
    return target


_lib = None


def lib() -> C.CDLL:
    """The loaded library.  Raises (never falls back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    # torch FIRST: its wheel bundles its own libamdhip64; if this library were loaded before torch, the system HIP runtime
    # it links against would come up as a second runtime in the process and every launch on torch's streams / memory would
    # fail (seen as "HIP launch / runtime error" when build() and smoke() ran in one process)
    import torch  # noqa: F401
    if not LIB_PATH.exists():
        raise RuntimeError(
            f"{LIB_PATH} is missing: the HIP rasteriser was not built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc). There is no CPU fallback.")
    l = C.CDLL(str(LIB_PATH))
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(l, name)
        fn.restype, fn.argtypes = restype, argtypes
    if l.s360_abi_version() != ABI_VERSION:
        raise RuntimeError("libs360.so ABI version mismatch")
    _lib = l
    return l


def check(code: int, what: str) -> None:
    if code != 0:
        raise RuntimeError(f"{what} failed: {lib().s360_error_string(code).decode()} ({code})")


def layout(prm: S360Params) -> S360Layout:
    out = S360Layout()
    check(lib().s360_layout(C.byref(prm), C.byref(out)), "s360_layout")
    return out


def profile_enable(on: bool) -> None:
    check(lib().s360_profile_enable(int(bool(on))), "s360_profile_enable")


def profile_collect() -> dict:
    """{slot_name: (total_ms, launches)} since the previous collect (host-synchronising)."""
    n = lib().s360_profile_slots()
    ms = (C.c_float * n)()
    calls = (C.c_int32 * n)()
    check(lib().s360_profile_collect(ms, calls), "s360_profile_collect")
    return {lib().s360_profile_slot_name(i).decode(): (float(ms[i]), int(calls[i])) for i in range(n)}
