"""tests/qkv_attention_reference.py against the reference's recorded outputs (tests/golden/qkv_attention.npz, made by
tests/golden/make_golden_qkv_attention.py from the reference's QKVAttentionLegacy and QKVAttention on the CPU): the float64
statement is the reference's function, the float32 lines are its float32 run, and the index rules the kernels implement — head
and order, rows (v b) <-> joint sequence — are the ones a wrong rule would miss.  No GPU."""
import functools
from pathlib import Path

import numpy as np
import pytest
import torch

import qkv_attention_reference as R

GOLDEN = Path(__file__).resolve().parent / "golden" / "qkv_attention.npz"
CASES = ("indexing", "rows", "frames_unused", "new_order")
E24 = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def recorded(case):
    """The case's arrays: qkv and g as float32, out64 / gqkv64, the float32 run rebuilt from its step distances, cfg as a tuple."""
    with np.load(GOLDEN) as z:
        g = {k[len(case) + 1:]: z[k] for k in z.files if k.startswith(case + "_")}

    def from_steps(want64, steps):
        i = np.ascontiguousarray(want64.astype(np.float32)).view(np.int32).astype(np.int64)
        key = np.where(i < 0, -(i & 0x7fffffff), i) + steps
        return np.where(key < 0, (-key) | 0x80000000, key).astype(np.uint32).view(np.float32).reshape(want64.shape)

    n, heads, frames, cross, order, ch, t = (int(x) for x in g["cfg"])
    return {"qkv": (g["qkv"].astype(np.float32) / 64.0), "g": (g["g"].astype(np.float32) / 64.0), "out64": g["out64"], "gqkv64": g["gqkv64"],
            "out32": from_steps(g["out64"], g["out32d"]), "gqkv32": from_steps(g["gqkv64"], g["gqkv32d"]),
            "cfg": (heads, frames, bool(cross), R.ORDERS[order]), "shape": (n, heads, ch, t)}


def test_the_golden_file_is_small_and_holds_the_cases():
    assert GOLDEN.stat().st_size < 128 * 1024
    for case in CASES:
        g = recorded(case)
        n, heads, ch, t = g["shape"]
        assert ch == 32 and g["qkv"].shape == (n, heads * 3 * ch, t) and g["out64"].shape == (n, heads * ch, t) == g["g"].shape
        assert g["out64"].dtype == np.float64 and g["gqkv64"].shape == g["qkv"].shape
    assert recorded("indexing")["cfg"] == (2, 3, True, "legacy") and recorded("indexing")["shape"][0] == 6    # heads 2, views 3, B 2
    assert recorded("frames_unused")["cfg"][1:3] == (2, False) and recorded("new_order")["cfg"][3] == "new"


@pytest.mark.parametrize("case", CASES)
def test_statement_and_float32_lines_reproduce_the_recorded_runs(case):
    """float64: the statement is the reference's function to float64 rounding (1e-12 of the largest element), which is far inside the
    float32 run's own distance from it.  float32: the lines and the recorded run round the same operations; their sums (32
    channels, at most 6 keys here) may be taken in another order on another machine, which moves a sum of n float32 terms by at
    most n 2^-24 of the sum of the terms' magnitudes — bounded here by 32 x 2^-24 x the largest element."""
    g = recorded(case)
    qkv, gout = torch.from_numpy(g["qkv"]), torch.from_numpy(g["g"])
    want = R.gradients(lambda x: R.statement(x, *g["cfg"]), qkv, gout, torch.float64)
    lines = R.gradients(lambda x: R.reference_lines(x, *g["cfg"]), qkv, gout)
    for name, w64, l32, rec64, rec32 in (("out", want[0], lines[0], g["out64"], g["out32"]), ("g_qkv", want[1], lines[1], g["gqkv64"], g["gqkv32"])):
        assert w64.dtype == torch.float64 and l32.dtype == torch.float32
        top = np.abs(rec64).max()
        d64 = np.abs(w64.numpy() - rec64).max()
        own = np.abs(rec32.astype(np.float64) - rec64).max()                       # the float32 run's own distance
        d32 = np.abs(l32.numpy().astype(np.float64) - rec32.astype(np.float64)).max()
        print(f"{case} {name}: statement {d64:.3e}, float32 run's own distance {own:.3e}, lines vs float32 run {d32:.3e}, largest {top:.3e}")
        assert own > 0 and d64 <= 1e-12 * top and d64 <= own
        assert d32 <= 32 * E24 * top


def explicit(qkv, heads, views, cross, order):
    """The function by the index rules alone, one (batch element, head) at a time in float64 numpy: joint token s is token s mod T
    of view s // T in row (s // T) B + bi; head hd's q, k, v rows by `order`."""
    n, width, t = qkv.shape
    nv = views if cross else 1
    b, ch = n // nv, width // (3 * heads)
    x = qkv.astype(np.float64)
    out = np.zeros((n, heads * ch, t))
    for bi in range(b):
        for hd in range(heads):
            if order == "legacy":
                qo, ko, vo = hd * 3 * ch, hd * 3 * ch + ch, hd * 3 * ch + 2 * ch
            else:
                qo, ko, vo = hd * ch, heads * ch + hd * ch, 2 * heads * ch + hd * ch
            rows = [u * b + bi for u in range(nv)]
            q, k, v = (np.concatenate([x[r, o:o + ch] for r in rows], axis=1) for o in (qo, ko, vo))      # [ch, L]
            s = (q * ch ** -0.25).T @ (k * ch ** -0.25)
            w = np.exp(s - s.max(axis=1, keepdims=True))
            w /= w.sum(axis=1, keepdims=True)
            a = v @ w.T                                                             # [ch, L]
            for u, r in enumerate(rows):
                out[r, hd * ch:(hd + 1) * ch] = a[:, u * t:(u + 1) * t]
    return out


@pytest.mark.parametrize("case", CASES)
def test_the_index_rules_are_the_reference_s(case):
    g = recorded(case)
    got = explicit(g["qkv"], *g["cfg"])
    assert np.abs(got - g["out64"]).max() <= 1e-12 * np.abs(g["out64"]).max()


def test_a_wrong_rule_changes_the_result():
    """heads = 2, views = 3, B = 2: the other order, rows read as (b v), cross-view dropped and heads swapped each move the output
    by far more than rounding."""
    g = recorded("indexing")
    heads, views, cross, order = g["cfg"]
    n, t = g["shape"][0], g["shape"][3]
    b, top = n // views, np.abs(g["out64"]).max()
    x = g["qkv"]
    assert b == 2
    bv = np.arange(n).reshape(b, views).T.reshape(-1)                              # position u B + bi holds row bi views + u
    inv = np.argsort(bv)
    swapped = x.reshape(n, heads, -1, t)[:, ::-1].reshape(x.shape)
    wrong = {"order": explicit(x, heads, views, cross, "new"),
             "rows as (b v)": explicit(x[bv], heads, views, cross, order)[inv],
             "no cross-view": explicit(x, heads, views, False, order),
             "heads swapped": explicit(swapped, heads, views, cross, order)}
    for name, out in wrong.items():
        assert np.abs(out - g["out64"]).max() > 1e-2 * top, name
    st = R.statement(torch.from_numpy(x), heads, views, cross, order).numpy()
    assert np.abs(st - g["out64"]).max() <= 1e-12 * top
    for name, alt in (("order", R.statement(torch.from_numpy(x), heads, views, cross, "new")),
                      ("no cross-view", R.statement(torch.from_numpy(x), heads, views, False, order))):
        assert np.abs(alt.numpy() - wrong[name]).max() <= 1e-12 * top, name          # the statement follows the same rules


def test_parts_splits_a_gradient_into_its_q_k_v_rows():
    for order in R.ORDERS:
        x = torch.arange(2 * 2 * 3 * 32 * 3, dtype=torch.float32).reshape(2, 192, 3)
        q, k, v = R.split_heads(x, 2, 1, False, order)
        pq, pk, pv = R.parts(x, 2, order)
        assert torch.equal(pq, q) and torch.equal(pk, k) and torch.equal(pv, v)
