"""Times the fused transformer FFN tail and the no_ffn tail (forward, and forward + backward) at the two backbone shapes of the
reference on two paths and records each one's peak of allocated memory -> profiles/transformer_ffn_timing.json.

    python scripts/transformer_ffn_timing.py [--out profiles/transformer_ffn_timing.json] [--calls 50] [--cases erp ...]

Cases (T tokens per layer), C = 128, hidden width 1024:
  erp    65 536     the ERP backbone: 2 views x 128 x 256 tokens
  cube   49 152     the cube backbone: 12 faces x 64 x 64 tokens
each for `ffn` (splatter360_amd.transformer_ffn.ffn_tail) and `norm` (layer_norm_residual, the layer with no_ffn).

Paths:
  native   the fused kernels
  torch    the reference's lines in float32 torch (tests/transformer_ffn_reference.reference_lines / norm_lines): forms the
           [T, 2C] concatenation and both [T, 8C] activations, autograd keeps them

The driver starts no GPU work itself: every step (one case, one tail, one path) is a child process under its own `timeout`, the
steps run one after the other, and the first one that fails, is killed or times out ends the run (what was measured until then
is written, with the failed step's name).  Each time is the median of `calls` calls (HIP events around one call, launch overhead
included) after 3 warm-up calls; forward + backward takes the gradients of all eight (four) tensors.  forward_tflops is
2 T (2C 8C + 8C C) floating-point operations (the two products) over the forward's median time; peak_fraction is that over the
157 TFLOP/s float32 MFMA peak.

    python scripts/transformer_ffn_timing.py --precision [--out profiles/transformer_ffn_high_timing.json]

is the leg of the "high" (bf16x3) mode of ffn_tail, at erp and cube: one `precision` child per case times the native "high" and
"highest" kernels, the float32 torch lines at torch's 'highest' and the same lines under
torch.set_float32_matmul_precision('high') (held over the whole measurement, the backward's products included, and restored
afterwards) in ONE process, alternated, forward and forward + backward, the whole collection three times over (the spread between the three medians is what a difference has to exceed), and records peak
memory, the scratch bytes and the forward's TFLOP/s.  `--calls 6 --step erp ffn precision_trace` is the native modes alone, the
step whose kernel trace (`rocprofv3 --kernel-trace --stats --`, a run of its own) is profiles/transformer_ffn_high_kernel_trace.txt."""
import argparse
import contextlib
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

CASES = {"erp": 65536, "cube": 49152}
TAILS = ("ffn", "norm")
PATHS = ("native", "torch")
MODES = ("high", "highest", "torch_f32", "torch_high")         # the `precision` child's paths
COLLECTIONS = 3
C, HIDDEN = 128, 1024
PEAK_TFLOPS = 157.0
STEP_LIMIT = 240                                               # seconds, per child


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


def step(case, tail, path, calls):
    """One child's work: returns the figures of (case, tail, path)."""
    import torch

    import transformer_ffn_reference as R
    from splatter360_amd import transformer_ffn as tf

    tokens = CASES[case]
    tensors, g = R.random_case(tokens, seed=11, device="cuda:0")
    if tail == "norm":
        tensors, g = R.norm_case((tensors, g))
        fn = tf.layer_norm_residual if path == "native" else R.norm_lines
    else:
        fn = tf.ffn_tail if path == "native" else R.reference_lines

    def forward():
        with torch.no_grad():
            return fn(*tensors)

    def forward_backward():
        return R.gradients(fn, tensors, g)

    res = {"fwd_ms": timed(forward, calls), "fwd_bwd_ms": timed(forward_backward, calls)}
    res["fwd_peak_bytes"], res["fwd_bwd_peak_bytes"] = peak(forward), peak(forward_backward)
    if tail == "ffn":
        res["forward_tflops"] = 2.0 * tokens * (2 * C * HIDDEN + HIDDEN * C) / (res["fwd_ms"]["median"] * 1e-3) / 1e12
        res["peak_fraction"] = res["forward_tflops"] / PEAK_TFLOPS
    res["one_hidden_tensor_bytes"] = tokens * HIDDEN * 4
    return res


def precision_step(case, calls):
    """The `precision` child's work: the four modes of one case, alternated inside each of COLLECTIONS collections."""
    import torch

    import transformer_ffn_reference as R
    from splatter360_amd import transformer_ffn as tf

    tokens = CASES[case]
    tensors, g = R.random_case(tokens, seed=11, device="cuda:0")
    before = torch.get_float32_matmul_precision()

    @contextlib.contextmanager
    def under(setting):
        """torch's float32 matmul precision over a whole measurement: warm-up, every forward AND every backward in it (the
        setting is process-wide, so the autograd engine's thread sees it; backward() returns after its last launch)."""
        torch.set_float32_matmul_precision(setting)
        try:
            yield
        finally:
            torch.set_float32_matmul_precision(before)

    fns = {"high": lambda *t: tf.ffn_tail(*t, precision="high"), "highest": lambda *t: tf.ffn_tail(*t, precision="highest"),
           "torch_f32": R.reference_lines, "torch_high": R.reference_lines}
    settings = {"high": before, "highest": before, "torch_f32": "highest", "torch_high": "high"}   # the native paths do not read it

    def forward(fn):
        def run():
            with torch.no_grad():
                return fn(*tensors)
        return run

    def forward_backward(fn):
        return lambda: R.gradients(fn, tensors, g)

    res = {tag: {"fwd_ms": [], "fwd_bwd_ms": []} for tag in MODES}
    for _ in range(COLLECTIONS):
        for leg, whole in (("fwd_ms", forward), ("fwd_bwd_ms", forward_backward)):
            for tag in MODES:                                   # alternated: one mode after the other inside every collection
                with under(settings[tag]):
                    res[tag][leg].append(timed(whole(fns[tag]), calls))
    for tag in MODES:
        with under(settings[tag]):
            res[tag]["fwd_peak_bytes"], res[tag]["fwd_bwd_peak_bytes"] = peak(forward(fns[tag])), peak(forward_backward(fns[tag]))
        res[tag]["matmul_precision"] = settings[tag]
        mid = statistics.median(c["median"] for c in res[tag]["fwd_ms"])
        res[tag]["forward_tflops"] = 2.0 * tokens * (2 * C * HIDDEN + HIDDEN * C) / (mid * 1e-3) / 1e12
    assert torch.get_float32_matmul_precision() == before
    res["one_hidden_tensor_bytes"] = tokens * HIDDEN * 4
    res["scratch_bytes"] = {p: {"forward": tf.scratch_bytes(tokens, False, p), "backward": tf.scratch_bytes(tokens, True, p)}
                            for p in tf.PRECISIONS}
    return res


def precision_trace_step(case, calls):
    """The step that profiles/transformer_ffn_high_kernel_trace.txt is a kernel trace of: the two native modes only, alternated,
    per mode 3 + `calls` forward calls and 3 + `calls` forward + backward calls; returns the medians of the timed calls."""
    import torch

    import transformer_ffn_reference as R
    from splatter360_amd import transformer_ffn as tf

    tensors, g = R.random_case(CASES[case], seed=11, device="cuda:0")
    res = {}
    for tag in tf.PRECISIONS[::-1]:
        def fn(*t, tag=tag):
            return tf.ffn_tail(*t, precision=tag)

        def forward():
            with torch.no_grad():
                return fn(*tensors)

        res[tag] = {"fwd_ms": timed(forward, calls)["median"], "fwd_bwd_ms": timed(lambda: R.gradients(fn, tensors, g), calls)["median"]}
    return res


def precision_summary(entry):
    """Per leg: the three medians of every mode, their spread (max - min), whether "high" is ahead of "highest" by more than the
    larger of the two spreads, and where it stands against the torch lines."""
    out = {}
    for leg in ("fwd_ms", "fwd_bwd_ms"):
        med = {tag: [c["median"] for c in entry["precision"][tag][leg]] for tag in MODES}
        mid = {tag: statistics.median(v) for tag, v in med.items()}
        spread = {tag: max(v) - min(v) for tag, v in med.items()}
        out[leg] = {"medians": med, "median": mid, "spread": spread,
                    "high_ahead_of_highest": mid["highest"] - mid["high"] > max(spread["high"], spread["highest"]),
                    "highest_over_high": mid["highest"] / mid["high"], "torch_high_over_high": mid["torch_high"] / mid["high"],
                    "torch_f32_over_high": mid["torch_f32"] / mid["high"],
                    "high_behind_torch_high": mid["high"] - mid["torch_high"] > max(spread["high"], spread["torch_high"])}
    return out


def precision_main(args):
    """The driver of --precision: one child per case, each under its own time limit, nothing after the first failure."""
    out_path = Path(args.out or ROOT / "profiles" / "transformer_ffn_high_timing.json")
    res = {"calls": args.calls, "collections": COLLECTIONS, "channels": C, "hidden": HIDDEN, "float32_mfma_peak_tflops": PEAK_TFLOPS,
           "failed_step": None, "cases": {}}
    rc = 0
    for case in args.cases:
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT), sys.executable, __file__, "--calls", str(args.calls), "--step", case, "ffn", "precision"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("STEP_RESULT ")]
        if r.returncode != 0 or not lines:
            res["failed_step"] = {"case": case, "tail": "ffn", "path": "precision", "returncode": r.returncode, "stderr": r.stderr[-1500:]}
            print("FAILED", res["failed_step"], flush=True)
            rc = 1
            break                                               # nothing is started on the GPU after a failed step
        entry = res["cases"][case] = {"tokens": CASES[case], "precision": json.loads(lines[0][len("STEP_RESULT "):])}
        entry["precision_summary"] = precision_summary(entry)
        print(case, json.dumps(entry["precision_summary"]), flush=True)
    if rc == 0:
        import torch

        from splatter360_amd import _lib
        res["device"], res["source_hash"] = torch.cuda.get_device_name(0), _lib.source_hash()
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(res, indent=1) + "\n")
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/transformer_ffn_timing.json (--precision: transformer_ffn_high_timing.json)")
    ap.add_argument("--precision", action="store_true", help="the leg of the \"high\" mode -> profiles/transformer_ffn_high_timing.json")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--cases", nargs="*", default=list(CASES))
    ap.add_argument("--tails", nargs="*", default=list(TAILS))
    ap.add_argument("--paths", nargs="*", default=list(PATHS))
    ap.add_argument("--step", nargs=3, metavar=("CASE", "TAIL", "PATH"), help="run one step in this process and print its JSON")
    args = ap.parse_args()
    if args.step:
        case, tail, path = args.step
        special = {"precision": precision_step, "precision_trace": precision_trace_step}
        print("STEP_RESULT " + json.dumps(special[path](case, args.calls) if path in special else step(case, tail, path, args.calls)))
        return 0
    if args.precision:
        return precision_main(args)
    out_path = Path(args.out or ROOT / "profiles" / "transformer_ffn_timing.json")
    res = json.loads(out_path.read_text()) if out_path.exists() else {}
    res.update({"calls": args.calls, "channels": C, "hidden": HIDDEN, "float32_mfma_peak_tflops": PEAK_TFLOPS, "failed_step": None})
    res.setdefault("cases", {})
    rc = 0
    for case in args.cases:
        for tail in args.tails:
            entry = res["cases"].setdefault(f"{case}_{tail}", {"tokens": CASES[case], "tail": tail})
            for path in args.paths:
                cmd = ["timeout", "-k", "10", str(STEP_LIMIT), sys.executable, __file__, "--calls", str(args.calls), "--step", case, tail, path]
                r = subprocess.run(cmd, capture_output=True, text=True)
                lines = [ln for ln in r.stdout.splitlines() if ln.startswith("STEP_RESULT ")]
                if r.returncode != 0 or not lines:
                    res["failed_step"] = {"case": case, "tail": tail, "path": path, "returncode": r.returncode, "stderr": r.stderr[-1500:]}
                    print("FAILED", res["failed_step"], flush=True)
                    rc = 1
                    break                                       # nothing is started on the GPU after a failed step
                entry[path] = json.loads(lines[0][len("STEP_RESULT "):])
                print(case, tail, path, json.dumps(entry[path]), flush=True)
            if rc:
                break
            if "native" in entry and "torch" in entry:
                for key in ("fwd_ms", "fwd_bwd_ms"):
                    entry[f"native_speedup_over_torch_{key[:-3]}"] = entry["torch"][key]["median"] / entry["native"][key]["median"]
                entry["fwd_bwd_peak_ratio_torch_over_native"] = entry["torch"]["fwd_bwd_peak_bytes"] / max(1, entry["native"]["fwd_bwd_peak_bytes"])
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
