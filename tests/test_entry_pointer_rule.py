"""The host-side argument rule of include/s360.h at the eighteen launch entries of the FFN tail, the mono-feature fusion, the
window attention and the QKV attention, as one table, without a GPU: a null pointer, a pointer that is not aligned (16 bytes; the
QKV attention's tensors their element's alone, its scratch 16), an output that is an input and an output that is another output
(the caller's scratch counts as an output) are S360_E_BADARG, and the classes of refusal come in the order pointers and eps
(BADARG), sizes (BADARG / UNSUPPORTED), scratch size (WORKSPACE).  An optional output (the window backward's g_q, g_k, g_v) is an
output whenever it is given, so it has misaligned and alias rows and no null row.  Every address is fake and never dereferenced,
the stream is None and every row is a refusal, so nothing launches; all optional outputs null is S360_OK with nothing launched.
A row marked `new` is one that an entry accepted, or refused with another status, before it went through the one rule of
csrc/s360_launch.h.  FFN tail: a misaligned stats, and stats equal to out or z, which the header forbade all along.  The
attentions: every output that is an input or another output (only g_qkv == qkv was refused), a misaligned lse or delta of the
window attention, a QKV tensor that is not a multiple of its element's size (an address no float32 or float64 tensor has), and
a call that is wrong twice and now meets the pointer class before the width."""
import ctypes as C
from typing import NamedTuple

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
WA_IN = ("q", "k", "v")
WA_DIMS = ("batch", "partners", "height", "width", "channels", "num_splits", "with_shift", "mask_rule")
WA_GRADS = ("g_q", "g_k", "g_v")
QA_DIMS = ("rows", "views", "heads", "ch", "tokens", "order")

FF_SIZES = dict(tokens=40, channels=128, hidden=1024)
LN_SIZES = dict(tokens=40, channels=128)
MF_SIZES = dict(n=1, channels=128, mono_channels=64, face_w=4, equ_h=8, equ_w=16)
WA_SIZES = dict(batch=1, partners=0, height=4, width=8, channels=32, num_splits=2, with_shift=1, mask_rule=0)
QA_SIZES = dict(rows=2, views=1, heads=1, ch=32, tokens=8, order=0)


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


def _wa_need(backward):
    def need(lib, d):
        return lib.s360_window_attention_high_scratch_bytes(*(d[n] for n in WA_DIMS[:6]), backward)
    return need


def _qa_need(backward):
    def need(lib, d):
        return lib.s360_qkv_attention_high_scratch_bytes(*(d[n] for n in QA_DIMS[:5]), backward)
    return need


class Entry(NamedTuple):
    """One launch entry.  In `args` a name of `good` is an int32, "eps" the host pointer, "scratch_bytes" the size, "stream" None,
    every other a pointer slot."""
    args: tuple                 # the arguments in the order of include/s360.h
    ins: tuple                  # what the call reads
    outs: tuple                 # what it writes, the scratch among them
    good: dict                  # valid sizes
    bad_width: dict             # an unsupported width
    need: object                # (lib, sizes) -> the scratch bytes needed, or None
    short_and_width: object     # what a short scratch together with the unsupported width gives
    new: tuple                  # label prefixes of the rows that are new refusals
    opt: tuple = ()             # outputs that may be null
    off: int = 8                # the bytes that misalign a pointer: 2 where the element's alignment is all that is asked


NEW_FWD = ("misaligned-stats", "alias-out-stats", "alias-z-stats")
NEW_WA = ("alias-", "misaligned-lse", "misaligned-delta", "misaligned-output-and-width", "null-scratch-and-width")
NEW_QA = ("alias-out-", "alias-lse-", "alias-delta-", "alias-scratch-", "alias-g_qkv-lse", "alias-g_qkv-g_out", "alias-g_qkv-scratch",
          "misaligned-qkv", "misaligned-out", "misaligned-lse", "misaligned-g_out", "misaligned-delta", "misaligned-g_qkv",
          "misaligned-output-and-width", "null-scratch-and-width")
ENTRIES = {
    "s360_ffn_tail_forward": Entry(
        FF_IN + FF_DIMS + ("eps", "out", "z", "stats", "stream"),
        FF_IN, ("out", "z", "stats"), FF_SIZES, dict(hidden=512), None, None, NEW_FWD),
    "s360_ffn_tail_backward": Entry(
        FF_IN + ("z", "stats", "g_out") + FF_DIMS + ("eps",) + SCRATCH + FF_GRADS + ("stream",),
        FF_IN + ("z", "stats", "g_out"), FF_GRADS + ("scratch",), FF_SIZES, dict(hidden=512), _ff_need(False, 1), UNSUPPORTED, ()),
    "s360_ffn_tail_high_forward": Entry(
        FF_IN + FF_DIMS + ("eps", "out", "z", "stats") + SCRATCH + ("stream",),
        FF_IN, ("out", "z", "stats", "scratch"), FF_SIZES, dict(channels=64), _ff_need(True, 0), UNSUPPORTED, NEW_FWD),
    "s360_ffn_tail_high_backward": Entry(
        FF_IN + ("z", "stats", "g_out") + FF_DIMS + ("eps",) + SCRATCH + FF_GRADS + ("stream",),
        FF_IN + ("z", "stats", "g_out"), FF_GRADS + ("scratch",), FF_SIZES, dict(channels=64), _ff_need(True, 1), UNSUPPORTED, ()),
    "s360_layer_norm_residual_forward": Entry(
        ("x", "weight", "bias", "residual", "tokens", "channels", "eps", "out", "stats", "stream"),
        ("x", "weight", "bias", "residual"), ("out", "stats"), LN_SIZES, dict(channels=96), None, None, NEW_FWD),
    "s360_layer_norm_residual_backward": Entry(
        ("x", "weight", "stats", "g_out", "tokens", "channels") + SCRATCH + ("g_x", "g_residual", "g_weight", "g_bias", "stream"),
        ("x", "weight", "stats", "g_out"), ("g_x", "g_residual", "g_weight", "g_bias", "scratch"), LN_SIZES, dict(channels=96),
        _ff_need(False, 1), UNSUPPORTED, ()),
    "s360_mono_fusion_forward": Entry(
        MF_IN + MF_DIMS + ("eps", "out", "y", "stats", "stream"),
        MF_IN, ("out", "y", "stats"), MF_SIZES, dict(mono_channels=96), None, None, ()),
    "s360_mono_fusion_backward": Entry(
        MF_IN + ("y", "stats", "g_out") + MF_DIMS + ("eps",) + SCRATCH + MF_GRADS + ("stream",),
        MF_IN + ("y", "stats", "g_out"), MF_GRADS + ("scratch",), MF_SIZES, dict(channels=64), _mf_need(False, 1), UNSUPPORTED, ()),
    "s360_mono_fusion_high_forward": Entry(
        MF_IN + MF_DIMS + ("eps", "out", "y", "stats") + SCRATCH + ("stream",),
        MF_IN, ("out", "y", "stats", "scratch"), MF_SIZES, dict(channels=256), _mf_need(True, 0), UNSUPPORTED, ()),
    "s360_mono_fusion_high_backward": Entry(
        MF_IN + ("y", "stats", "g_out") + MF_DIMS + ("eps",) + SCRATCH + MF_GRADS + ("stream",),
        MF_IN + ("y", "stats", "g_out"), MF_GRADS + ("scratch",), MF_SIZES, dict(mono_channels=1088), _mf_need(True, 1), UNSUPPORTED, ()),
    "s360_window_attention_forward": Entry(
        WA_IN + WA_DIMS + ("out", "lse", "stream"),
        WA_IN, ("out", "lse"), WA_SIZES, dict(channels=48), None, None, NEW_WA),
    "s360_window_attention_backward": Entry(
        WA_IN + ("lse", "g_out") + WA_DIMS + ("delta",) + WA_GRADS + ("stream",),
        WA_IN + ("lse", "g_out"), ("delta",), WA_SIZES, dict(channels=48), None, None, NEW_WA, opt=WA_GRADS),
    "s360_window_attention_high_forward": Entry(
        WA_IN + WA_DIMS + ("out", "lse") + SCRATCH + ("stream",),
        WA_IN, ("out", "lse", "scratch"), WA_SIZES, dict(channels=48), _wa_need(0), UNSUPPORTED, NEW_WA),
    "s360_window_attention_high_backward": Entry(
        WA_IN + ("lse", "g_out") + WA_DIMS + ("delta",) + WA_GRADS + SCRATCH + ("stream",),
        WA_IN + ("lse", "g_out"), ("delta", "scratch"), WA_SIZES, dict(channels=48), _wa_need(1), UNSUPPORTED, NEW_WA, opt=WA_GRADS),
    "s360_qkv_attention_forward": Entry(
        ("qkv",) + QA_DIMS + ("out", "lse", "stream"),
        ("qkv",), ("out", "lse"), QA_SIZES, dict(ch=16), None, None, NEW_QA, off=2),
    "s360_qkv_attention_backward": Entry(
        ("qkv", "lse", "g_out") + QA_DIMS + ("delta", "g_qkv", "stream"),
        ("qkv", "lse", "g_out"), ("delta", "g_qkv"), QA_SIZES, dict(ch=16), None, None, NEW_QA, off=2),
    "s360_qkv_attention_high_forward": Entry(
        ("qkv",) + QA_DIMS + ("out", "lse") + SCRATCH + ("stream",),
        ("qkv",), ("out", "lse", "scratch"), QA_SIZES, dict(ch=16), _qa_need(0), UNSUPPORTED, NEW_QA, off=2),
    "s360_qkv_attention_high_backward": Entry(
        ("qkv", "lse", "g_out") + QA_DIMS + ("delta", "g_qkv") + SCRATCH + ("stream",),
        ("qkv", "lse", "g_out"), ("delta", "g_qkv", "scratch"), QA_SIZES, dict(ch=16), _qa_need(1), UNSUPPORTED, NEW_QA, off=2),
}

def _call(entry, ptr=(), sizes=(), eps=1e-5, short=None):
    """The entry's status for valid arguments changed by `ptr` (slot -> address or None), `sizes`, `eps` (None: a null pointer)
    and `short` (bytes taken off the scratch the valid sizes need)."""
    e = ENTRIES[entry]
    args, good, need = e.args, e.good, e.need
    lib = _lib.lib()
    value = {name: 0x10000 * (i + 1) for i, name in enumerate(e.ins + e.outs + e.opt)}
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
    for entry, (args, ins, outs, good, bad_width, need, short_and_width, new, opt, off) in ENTRIES.items():
        def row(label, want, **change):
            rows.append(pytest.param(entry, change, want, id=f"{entry[5:]}-{label}" + ("-new" if label.startswith(new) else "")))
        at = {name: 0x10000 * (i + 1) for i, name in enumerate(ins + outs + opt)}
        for slot in ins + outs + opt:
            if slot not in opt:                               # a null optional output is a valid call, which would launch
                row(f"null-{slot}", BADARG, ptr={slot: None})
            row(f"misaligned-{slot}", BADARG, ptr={slot: at[slot] + off})
        for i, out in enumerate(outs + opt):
            for other in ins + (outs + opt)[i + 1:]:
                row(f"alias-{out}-{other}", BADARG, ptr={out: at[other]})
        # the order of the classes
        row("bad-pointer-and-width", BADARG, ptr={ins[0]: None}, sizes=bad_width)
        row("misaligned-output-and-width", BADARG, ptr={outs[0]: at[outs[0]] + off}, sizes=bad_width)
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


def test_table_names_the_eighteen_entries_with_their_bound_signatures():
    assert len(ENTRIES) == 18
    for entry, e in ENTRIES.items():
        assert len(e.args) == len(_lib.SIGNATURES[entry][1]), entry
        slots = set(e.ins + e.outs + e.opt) | set(e.good) | {"stream"} | ({"scratch_bytes"} if "scratch" in e.outs else set())
        assert slots == set(e.args) - {"eps"}, entry
        assert set(e.bad_width) <= set(e.good), entry
        assert _call(entry, sizes=e.bad_width) == UNSUPPORTED, entry


@pytest.mark.parametrize("entry, change, want", _rows())
def test_entry_refuses(entry, change, want):
    assert _call(entry, **change) == want


@pytest.mark.parametrize("entry", ["s360_window_attention_backward", "s360_window_attention_high_backward"])
def test_no_optional_output_asked_for_is_ok_and_launches_nothing(entry):
    assert _call(entry, ptr=dict(g_q=None, g_k=None, g_v=None)) == 0
    assert _call(entry, ptr=dict(g_q=None, g_k=None, g_v=None, delta=None)) == BADARG      # after the checks, not in their place
