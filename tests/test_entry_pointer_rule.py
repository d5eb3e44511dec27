"""The host-side argument rule of include/s360.h at the ten launch entries of the FFN tail and the mono-feature fusion, as one
table, without a GPU: a null pointer, a pointer that is not 16-byte aligned, an output that is an input and an output that is
another output (the caller's scratch counts as an output) are S360_E_BADARG, and the classes of refusal come in the order
pointers and eps (BADARG), sizes (BADARG / UNSUPPORTED), scratch size (WORKSPACE).  Every address is fake and never
dereferenced, the stream is None and every row is a refusal, so nothing launches.
A row marked `new` is one that three forward entries accepted before they went through the one rule of csrc/s360_launch.h (a
misaligned stats, and stats equal to out or z): the header forbade them all along."""
import ctypes as C

import pytest

from splatter360_amd import _lib

BADARG, WORKSPACE, UNSUPPORTED = -1, -2, -4

FF_IN = ("source", "m", "norm1_weight", "norm1_bias", "w1", "w2", "norm2_weight", "norm2_bias")
FF_DIMS = ("tokens", "channels", "hidden")
FF_GRADS = ("g_source", "g_m", "g_w1", "g_w2", "g_norm1_weight", "g_norm1_bias", "g_norm2_weight", "g_norm2_bias")
MF_IN = ("erp_feat", "mono_cube", "grid", "w1", "ln_weight", "ln_bias", "w2")
MF_DIMS = ("n", "channels", "mono_channels", "face_w", "equ_h", "equ_w")
MF_GRADS = ("g_erp_feat", "g_w1", "g_ln_weight", "g_ln_bias", "g_w2")
SCRATCH = ("scratch", "scratch_bytes")

FF_SIZES = dict(tokens=40, channels=128, hidden=1024)
LN_SIZES = dict(tokens=40, channels=128)
MF_SIZES = dict(n=1, channels=128, mono_channels=64, face_w=4, equ_h=8, equ_w=16)


def _ff_need(high, backward):
    def need(lib, d):
        return lib.s360_ffn_tail_high_scratch_bytes(d["tokens"], backward) if high else lib.s360_ffn_tail_scratch_bytes(d["tokens"])
    return need


def _mf_need(high, backward):
    def need(lib, d):
        t = d["n"] * d["equ_h"] * d["equ_w"]
        if high:
            return lib.s360_mono_fusion_high_scratch_bytes(t, d["mono_channels"], backward)
        return lib.s360_mono_fusion_scratch_bytes(t, d["mono_channels"])
    return need


# entry -> (arguments in the order of include/s360.h, inputs, outputs, valid sizes, an unsupported width, scratch bytes needed,
#           what a short scratch together with the unsupported width gives, rows that are new refusals)
# In `args` a name of `sizes` is an int32, "eps" the host pointer, "scratch_bytes" the size, "stream" None, every other a pointer slot.
NEW_FWD = {"misaligned-stats", "alias-out-stats", "alias-z-stats"}
ENTRIES = {
    "s360_ffn_tail_forward": (
        FF_IN + FF_DIMS + ("eps", "out", "z", "stats", "stream"),
        FF_IN, ("out", "z", "stats"), FF_SIZES, dict(hidden=512), None, None, NEW_FWD),
    "s360_ffn_tail_backward": (
        FF_IN + ("z", "stats", "g_out") + FF_DIMS + ("eps",) + SCRATCH + FF_GRADS + ("stream",),
        FF_IN + ("z", "stats", "g_out"), FF_GRADS + ("scratch",), FF_SIZES, dict(hidden=512), _ff_need(False, 1), UNSUPPORTED, ()),
    "s360_ffn_tail_high_forward": (
        FF_IN + FF_DIMS + ("eps", "out", "z", "stats") + SCRATCH + ("stream",),
        FF_IN, ("out", "z", "stats", "scratch"), FF_SIZES, dict(channels=64), _ff_need(True, 0), UNSUPPORTED, NEW_FWD),
    "s360_ffn_tail_high_backward": (
        FF_IN + ("z", "stats", "g_out") + FF_DIMS + ("eps",) + SCRATCH + FF_GRADS + ("stream",),
        FF_IN + ("z", "stats", "g_out"), FF_GRADS + ("scratch",), FF_SIZES, dict(channels=64), _ff_need(True, 1), UNSUPPORTED, ()),
    "s360_layer_norm_residual_forward": (
        ("x", "weight", "bias", "residual", "tokens", "channels", "eps", "out", "stats", "stream"),
        ("x", "weight", "bias", "residual"), ("out", "stats"), LN_SIZES, dict(channels=96), None, None, NEW_FWD),
    "s360_layer_norm_residual_backward": (
        ("x", "weight", "stats", "g_out", "tokens", "channels") + SCRATCH + ("g_x", "g_residual", "g_weight", "g_bias", "stream"),
        ("x", "weight", "stats", "g_out"), ("g_x", "g_residual", "g_weight", "g_bias", "scratch"), LN_SIZES, dict(channels=96),
        _ff_need(False, 1), UNSUPPORTED, ()),
    "s360_mono_fusion_forward": (
        MF_IN + MF_DIMS + ("eps", "out", "y", "stats", "stream"),
        MF_IN, ("out", "y", "stats"), MF_SIZES, dict(mono_channels=96), None, None, ()),
    "s360_mono_fusion_backward": (
        MF_IN + ("y", "stats", "g_out") + MF_DIMS + ("eps",) + SCRATCH + MF_GRADS + ("stream",),
        MF_IN + ("y", "stats", "g_out"), MF_GRADS + ("scratch",), MF_SIZES, dict(channels=64), _mf_need(False, 1), UNSUPPORTED, ()),
    "s360_mono_fusion_high_forward": (
        MF_IN + MF_DIMS + ("eps", "out", "y", "stats") + SCRATCH + ("stream",),
        MF_IN, ("out", "y", "stats", "scratch"), MF_SIZES, dict(channels=256), _mf_need(True, 0), UNSUPPORTED, ()),
    "s360_mono_fusion_high_backward": (
        MF_IN + ("y", "stats", "g_out") + MF_DIMS + ("eps",) + SCRATCH + MF_GRADS + ("stream",),
        MF_IN + ("y", "stats", "g_out"), MF_GRADS + ("scratch",), MF_SIZES, dict(mono_channels=1088), _mf_need(True, 1), UNSUPPORTED, ()),
}


def _call(entry, ptr=(), sizes=(), eps=1e-5, short=None):
    """The entry's status for valid arguments changed by `ptr` (slot -> address or None), `sizes`, `eps` (None: a null pointer)
    and `short` (bytes taken off the scratch the valid sizes need)."""
    args, ins, outs, good, _, need, _, _ = ENTRIES[entry]
    lib = _lib.lib()
    value = {name: 0x10000 * (i + 1) for i, name in enumerate(ins + outs)}
    value.update(good)
    value.update(stream=None)
    if "eps" in args:
        value.update(eps=None if eps is None else C.byref(C.c_double(eps)))
    if need is not None:
        value["scratch_bytes"] = need(lib, good) - (short or 0)
        assert need(lib, good) > 0
    value.update(sizes)
    value.update(ptr)
    assert sorted(args) == sorted(value), entry
    return getattr(lib, entry)(*(value[name] for name in args))


def _rows():
    rows = []
    for entry, (args, ins, outs, good, bad_width, need, short_and_width, new) in ENTRIES.items():
        def row(label, want, **change):
            rows.append(pytest.param(entry, change, want, id=f"{entry[5:]}-{label}" + ("-new" if label in new else "")))
        at = {name: 0x10000 * (i + 1) for i, name in enumerate(ins + outs)}
        for slot in ins + outs:
            row(f"null-{slot}", BADARG, ptr={slot: None})
            row(f"misaligned-{slot}", BADARG, ptr={slot: at[slot] + 8})
        for i, out in enumerate(outs):
            for other in ins + outs[i + 1:]:
                row(f"alias-{out}-{other}", BADARG, ptr={out: at[other]})
        # the order of the classes
        row("bad-pointer-and-width", BADARG, ptr={ins[0]: None}, sizes=bad_width)
        row("misaligned-output-and-width", BADARG, ptr={outs[0]: at[outs[0]] + 8}, sizes=bad_width)
        row("width", UNSUPPORTED, sizes=bad_width)
        if "eps" in args:
            row("null-eps-and-width", BADARG, eps=None, sizes=bad_width)
            row("zero-eps-and-width", BADARG, eps=0.0, sizes=bad_width)
            row("nan-eps", BADARG, eps=float("nan"))
        if need is not None:
            row("short-scratch", WORKSPACE, short=1)
            row("no-scratch-bytes", WORKSPACE, sizes=dict(scratch_bytes=0))
            row("null-scratch-and-short", BADARG, ptr=dict(scratch=None), short=1)
            row("null-scratch-and-width", BADARG, ptr=dict(scratch=None), sizes=bad_width)
            row("short-scratch-and-width", short_and_width, sizes=dict(bad_width, scratch_bytes=0))
    return rows


def test_table_names_the_ten_entries_with_their_bound_signatures():
    assert len(ENTRIES) == 10
    for entry, (args, ins, outs, good, bad_width, *_rest) in ENTRIES.items():
        assert len(args) == len(_lib.SIGNATURES[entry][1]), entry
        assert set(ins + outs) | set(good) | {"stream"} | ({"scratch_bytes"} if "scratch" in outs else set()) == set(args) - {"eps"}, entry
        assert set(bad_width) <= set(good), entry
        assert _call(entry, sizes=bad_width) == UNSUPPORTED, entry


@pytest.mark.parametrize("entry, change, want", _rows())
def test_entry_refuses(entry, change, want):
    assert _call(entry, **change) == want
