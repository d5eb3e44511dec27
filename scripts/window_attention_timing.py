"""Times the fused window attention (forward, and forward + backward) against the reference's lines restated in torch
(tests/window_attention_reference.reference_lines, float32) on the same GPU, at the two hm3d backbone shapes, records both
peaks of allocated memory and the accuracy figures of tests/test_gpu_window_attention.py's rule against float64
-> profiles/window_attention_timing.json.

    python scripts/window_attention_timing.py [--out profiles/window_attention_timing.json] [--calls 50] [--cases erp_self ...]

Cases (B, m, h, w, K), C = 128, each with shift off and on:
  erp_self (2, 0, 128, 256, 2), erp_cross (2, 1, 128, 256, 2)      the ERP backbone: Lw = Lk = 8192
  cube_self (12, 0, 64, 64, 2), cube_cross (12, 11, 64, 64, 2)     the cube backbone: Lw = 1024, Lk = 1024 / 11264

The driver starts no GPU work itself: every step (one case, one shift, one of native / torch / accuracy) is a child process
under its own `timeout`, the steps run one after the other, and the first one that fails, is killed or times out ends the run
(what was measured until then is written, with the failed step's name).  Each time is the median of `calls` calls (HIP events
around one call, launch overhead included) after 3 warm-up calls.

    python scripts/window_attention_timing.py --precision [--out profiles/window_attention_high_timing.json]

is the leg of the "high" (bf16x3) mode, at erp_self, cube_self and cube_cross, shift off and on: a `precision` child times "high",
"highest" and the float32 torch lines in ONE process, alternated, forward and forward + backward, the whole collection three
times over (the spread between the three medians is what a difference has to exceed), and records peak memory and the scratch
bytes; a `precision_accuracy` child records the distance from the float64 statement of "high", "highest", the float32 lines
and the terms=3 statement of tests/window_attention_high_reference.py.  `--step CASE SHIFT precision_trace` is the short run
(one collection) meant for a profiler's kernel trace."""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

CASES = {"erp_self": (2, 0, 128, 256, 2), "erp_cross": (2, 1, 128, 256, 2), "cube_self": (12, 0, 64, 64, 2),
         "cube_cross": (12, 11, 64, 64, 2)}
CHANNELS = 128
STEP_LIMIT = {"native": 240, "torch": 240, "accuracy": 400, "precision": 300, "precision_accuracy": 400}     # seconds, per child
PRECISION_CASES = ("erp_self", "cube_self", "cube_cross")
COLLECTIONS = 3


def timed(fn, calls, warmup=3):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}


def peak(fn):
    import torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def step(case, shift, side, calls):
    """One child's work: returns the figures of (case, shift, side)."""
    import torch

    import window_attention_reference as R
    from splatter360_amd import window_attention as wa

    b, m, h, w, k = CASES[case]
    q, kk, v, g = R.random_case(b, m, h, w, c=CHANNELS, seed=11, device="cuda:0")
    mask = R.dense_mask(h, w, k, "cuda:0") if shift and side != "native" else None

    def native(a, bb, cc):
        return wa.window_attention(a, bb, cc, height=h, width=w, num_splits=k, with_shift=shift)

    def lines(a, bb, cc):
        return R.reference_lines(a, bb, cc, k, shift, h, w, mask)

    if side.startswith("precision"):
        return precision_step(side, q, kk, v, g, lines, CASES[case], shift, calls)

    if side == "accuracy":
        want = R.gradients(lambda a, bb, cc: R.statement(a, bb, cc, k, shift, h, w), q, kk, v, g, torch.float64)
        res = {}
        for tag, fn in (("kernel", native), ("torch_f32", lines)):
            got = R.gradients(fn, q, kk, v, g)
            for name, x, w64 in zip(("out", "g_q", "g_k", "g_v"), got, want):
                e = (x.double() - w64).abs()
                res.setdefault(name, {"floor": 2.0 ** -24 * w64.abs().max().item()})[tag] = {"max": e.max().item(), "mean": e.mean().item()}
            del got
        return res
    fn = native if side == "native" else lines

    def forward():
        with torch.no_grad():
            return fn(q, kk, v)

    def forward_backward():
        return R.gradients(fn, q, kk, v, g)

    res = {"fwd_ms": timed(forward, calls), "fwd_bwd_ms": timed(forward_backward, calls)}
    res["fwd_peak_bytes"], res["fwd_bwd_peak_bytes"] = peak(forward), peak(forward_backward)
    res["q_bytes"] = q.numel() * 4
    res["mask_bytes"] = 0 if mask is None else mask.numel() * 4
    return res


def precision_step(side, q, kk, v, g, lines, shape, shift, calls):
    """The children of the --precision leg (see the module's docstring)."""
    import torch

    import window_attention_high_reference as H
    import window_attention_reference as R
    from splatter360_amd import window_attention as wa

    b, m, h, w, k = shape
    fns = {p: (lambda a, bb, cc, p=p: wa.window_attention(a, bb, cc, height=h, width=w, num_splits=k, with_shift=shift, precision=p))
           for p in ("high", "highest")}
    fns["torch_f32"] = lines
    if side == "precision_accuracy":
        want = R.gradients(lambda a, bb, cc: R.statement(a, bb, cc, k, shift, h, w), q, kk, v, g, torch.float64)
        res = {}
        runs = [(tag, fn, None) for tag, fn in fns.items()] + [("terms3", lambda a, bb, cc: H.split_statement(a, bb, cc, k, shift, h, w), torch.float64)]
        for tag, fn, dtype in runs:
            got = R.gradients(fn, q, kk, v, g, dtype)
            for name, x, w64 in zip(("out", "g_q", "g_k", "g_v"), got, want):
                res.setdefault(name, {"floor": 2.0 ** -24 * w64.abs().max().item()})[tag] = dict(zip(("max", "mean"), H.errors(x, w64)))
            del got
        return res
    legs = {"fwd_ms": lambda fn: (lambda: _no_grad(fn, q, kk, v)), "fwd_bwd_ms": lambda fn: (lambda: R.gradients(fn, q, kk, v, g))}
    res = {tag: {leg: [] for leg in legs} for tag in fns}
    for _ in range(1 if side == "precision_trace" else COLLECTIONS):
        for leg, make in legs.items():
            for tag, fn in fns.items():                          # alternated: one mode after the other inside every collection
                res[tag][leg].append(timed(make(fn), calls))
    for tag, fn in fns.items():
        res[tag]["fwd_peak_bytes"], res[tag]["fwd_bwd_peak_bytes"] = peak(legs["fwd_ms"](fn)), peak(legs["fwd_bwd_ms"](fn))
    res["q_bytes"] = q.numel() * 4
    res["scratch_bytes"] = {"forward": wa.scratch_bytes(b, m, h, w, CHANNELS, k, False), "backward": wa.scratch_bytes(b, m, h, w, CHANNELS, k, True)}
    return res


def _no_grad(fn, q, kk, v):
    import torch
    with torch.no_grad():
        return fn(q, kk, v)


def precision_summary(entry):
    """Per leg: the three medians of every mode, their spread (max - min), and whether "high" is ahead of "highest" by more than
    the larger of the two spreads."""
    out = {}
    for leg in ("fwd_ms", "fwd_bwd_ms"):
        med = {tag: [c["median"] for c in entry["precision"][tag][leg]] for tag in ("high", "highest", "torch_f32")}
        mid = {tag: statistics.median(v) for tag, v in med.items()}
        spread = {tag: max(v) - min(v) for tag, v in med.items()}
        out[leg] = {"medians": med, "median": mid, "spread": spread,
                    "high_ahead_of_highest": mid["highest"] - mid["high"] > max(spread["high"], spread["highest"]),
                    "highest_over_high": mid["highest"] / mid["high"], "torch_over_high": mid["torch_f32"] / mid["high"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--precision", action="store_true", help="the leg of the \"high\" mode -> profiles/window_attention_high_timing.json")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--cases", nargs="*", default=None)
    ap.add_argument("--sides", nargs="*", default=None)
    ap.add_argument("--step", nargs=3, metavar=("CASE", "SHIFT", "SIDE"), help="run one step in this process and print its JSON")
    args = ap.parse_args()
    if args.step:
        case, shift, side = args.step
        print("STEP_RESULT " + json.dumps(step(case, bool(int(shift)), side, args.calls)))
        return 0
    args.cases = args.cases or (list(PRECISION_CASES) if args.precision else list(CASES))
    args.sides = args.sides or (["precision", "precision_accuracy"] if args.precision else ["native", "torch", "accuracy"])
    out_path = Path(args.out or ROOT / "profiles" / ("window_attention_high_timing.json" if args.precision else "window_attention_timing.json"))
    res = json.loads(out_path.read_text()) if out_path.exists() else {}
    res.update({"calls": args.calls, "channels": CHANNELS, "failed_step": None})
    res.setdefault("cases", {})
    rc = 0
    for case in args.cases:
        for shift in (0, 1):
            entry = res["cases"].setdefault(f"{case}_shift{shift}", {"shape": dict(zip(("B", "m", "h", "w", "K"), CASES[case])), "with_shift": bool(shift)})
            for side in args.sides:
                cmd = ["timeout", "-k", "10", str(STEP_LIMIT[side]), sys.executable, __file__, "--calls", str(args.calls), "--step", case,
                       str(shift), side]
                r = subprocess.run(cmd, capture_output=True, text=True)
                lines = [ln for ln in r.stdout.splitlines() if ln.startswith("STEP_RESULT ")]
                if r.returncode != 0 or not lines:
                    res["failed_step"] = {"case": case, "shift": shift, "side": side, "returncode": r.returncode, "stderr": r.stderr[-1500:]}
                    print("FAILED", res["failed_step"], flush=True)
                    rc = 1
                    break                                       # nothing is started on the GPU after a failed step
                entry[side] = json.loads(lines[0][len("STEP_RESULT "):])
                print(case, shift, side, json.dumps(entry[side]), flush=True)
            if rc:
                break
            if "precision" in entry:
                entry["precision_summary"] = precision_summary(entry)
                print(case, shift, "summary", json.dumps(entry["precision_summary"]), flush=True)
            if "native" in entry and "torch" in entry:
                for key in ("fwd_ms", "fwd_bwd_ms"):
                    entry[f"speedup_{key[:-3]}"] = entry["torch"][key]["median"] / entry["native"][key]["median"]
        if rc:
            break
    if rc == 0:
        import torch

        from splatter360_amd import _lib
        res["device"], res["source_hash"] = torch.cuda.get_device_name(0), _lib.source_hash()
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(res, indent=1) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
