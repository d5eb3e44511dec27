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
157 TFLOP/s float32 MFMA peak."""
import argparse
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "transformer_ffn_timing.json"))
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--cases", nargs="*", default=list(CASES))
    ap.add_argument("--tails", nargs="*", default=list(TAILS))
    ap.add_argument("--paths", nargs="*", default=list(PATHS))
    ap.add_argument("--step", nargs=3, metavar=("CASE", "TAIL", "PATH"), help="run one step in this process and print its JSON")
    args = ap.parse_args()
    if args.step:
        print("STEP_RESULT " + json.dumps(step(*args.step, args.calls)))
        return 0
    out_path = Path(args.out)
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
