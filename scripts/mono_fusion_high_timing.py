"""Times the "high" (bf16x3) precision mode of the fused mono-feature fusion (forward, and forward + backward) at the hm3d shape of
the reference against its two yardsticks — the "highest" kernels at this commit and the reference's lines in float32 torch under
torch.set_float32_matmul_precision('high') — and records each path's peak of allocated memory
-> profiles/mono_fusion_high_timing.json.

    python scripts/mono_fusion_high_timing.py [--out profiles/mono_fusion_high_timing.json] [--calls 50] [--cases vits vitb]

Cases: N = 2 context views, (face_w, equ_h, equ_w) = (64, 128, 256): 65 536 tokens, C = 128 and
  vits   Cm = 384     the configuration (config/model/encoder/costvolume.yaml: vit_type vits)
  vitb   Cm = 768     vit_type vitb

Paths:
  high         splatter360_amd.mono_fusion.mono_fusion(precision="high"): bf16x3 products on the bf16 MFMA, forward and backward
  highest      the same with precision="highest": exact float32 products
  torch        tests/mono_fusion_reference.reference_lines in float32 under torch's 'highest'
  torch_high   the same lines under torch.set_float32_matmul_precision('high'), held over torch's forward and backward

The driver starts no GPU work itself: every step (one case) is a child process under its own `timeout`, the steps run one after
the other, and the first one that fails, is killed or times out ends the run (what was measured until then is written, with the
failed step's name).  Inside a child the four paths are ALTERNATED in one process, forward and forward + backward, the whole
collection three times over (the spread between the three medians is what a difference has to exceed).  Each time is the median
of `calls` calls (HIP events around one call, launch overhead included) after 3 warm-up calls; forward + backward takes the
gradients of erp_feat and the four parameters.  `--calls 6 --step vits trace` is the "high" path alone, the step whose kernel
trace (`rocprofv3 --kernel-trace --stats --`, a run of its own) is profiles/mono_fusion_high_kernel_trace.txt."""
import argparse
import contextlib
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests"), str(ROOT / "scripts")]

from mono_fusion_timing import C, CASES, COLLECTIONS, GEOMETRY, N, peak, timed  # noqa: E402  (the "highest" script's shapes and clocks)

PATHS = ("high", "highest", "torch", "torch_high")
YARDSTICKS = ("highest", "torch_high")
STEP_LIMIT = 420                                               # seconds, per child


@contextlib.contextmanager
def matmul_precision(setting):
    import torch
    before = torch.get_float32_matmul_precision()
    torch.set_float32_matmul_precision(setting)
    try:
        yield
    finally:
        torch.set_float32_matmul_precision(before)


def _paths(case):
    import torch

    import mono_fusion_reference as R
    from splatter360_amd import mono_fusion as mf

    tensors, g = R.random_case(N, GEOMETRY, CASES[case], seed=11, device="cuda:0")
    fns = {"high": lambda *t: mf.mono_fusion(*t, precision="high"), "highest": lambda *t: mf.mono_fusion(*t, precision="highest"),
           "torch": R.reference_lines, "torch_high": R.reference_lines}
    setting = {"high": "highest", "highest": "highest", "torch": "highest", "torch_high": "high"}

    def forward(tag):
        def run():
            with matmul_precision(setting[tag]), torch.no_grad():
                return fns[tag](*tensors)
        return run

    def forward_backward(tag):
        def run():
            with matmul_precision(setting[tag]):                # held over torch's forward and its backward
                return R.gradients(fns[tag], tensors, g)
        return run

    return forward, forward_backward


def step(case, calls):
    """One child's work: the four paths of one case, alternated inside each of COLLECTIONS collections."""
    from splatter360_amd import mono_fusion as mf

    forward, forward_backward = _paths(case)
    tokens, cm = N * GEOMETRY[1] * GEOMETRY[2], CASES[case]
    res = {tag: {"fwd_ms": [], "fwd_bwd_ms": []} for tag in PATHS}
    for _ in range(COLLECTIONS):
        for leg, whole in (("fwd_ms", forward), ("fwd_bwd_ms", forward_backward)):
            for tag in PATHS:                                   # alternated: one path after the other inside every collection
                res[tag][leg].append(timed(whole(tag), calls))
    for tag in PATHS:
        res[tag]["fwd_peak_bytes"], res[tag]["fwd_bwd_peak_bytes"] = peak(forward(tag)), peak(forward_backward(tag))
    res["tokens"], res["mono_channels"] = tokens, cm
    res["scratch_bytes"] = {p: {"forward": mf.scratch_bytes(tokens, cm, False, p), "backward": mf.scratch_bytes(tokens, cm, True, p)}
                            for p in ("highest", "high")}
    return res


def trace_step(case, calls):
    """The step that profiles/mono_fusion_high_kernel_trace.txt is a kernel trace of: the "high" path alone, 3 + `calls` forward
    calls and 3 + `calls` forward + backward calls; returns the medians of the timed calls."""
    forward, forward_backward = _paths(case)
    return {"fwd_ms": timed(forward("high"), calls)["median"], "fwd_bwd_ms": timed(forward_backward("high"), calls)["median"]}


def summary(entry):
    """Per leg: the three medians of every path, their spread (max - min), each yardstick over "high", and whether "high" is ahead
    of (behind) the yardstick by more than the larger of the two spreads."""
    out = {}
    for leg in ("fwd_ms", "fwd_bwd_ms"):
        med = {tag: [c["median"] for c in entry[tag][leg]] for tag in PATHS}
        mid = {tag: statistics.median(v) for tag, v in med.items()}
        spread = {tag: max(v) - min(v) for tag, v in med.items()}
        out[leg] = {"medians": med, "median": mid, "spread": spread}
        for other in (*YARDSTICKS, "torch"):
            margin = max(spread["high"], spread[other])
            out[leg][other + "_over_high"] = mid[other] / mid["high"]
            out[leg]["high_ahead_of_" + other] = mid[other] - mid["high"] > margin
            out[leg]["high_behind_" + other] = mid["high"] - mid[other] > margin
    out["fwd_bwd_peak_ratio_torch_high_over_high"] = entry["torch_high"]["fwd_bwd_peak_bytes"] / max(1, entry["high"]["fwd_bwd_peak_bytes"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/mono_fusion_high_timing.json")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--cases", nargs="*", default=list(CASES))
    ap.add_argument("--step", nargs=2, metavar=("CASE", "KIND"), help="run one step (KIND: timing or trace) in this process and print its JSON")
    args = ap.parse_args()
    if args.step:
        case, kind = args.step
        print("STEP_RESULT " + json.dumps(trace_step(case, args.calls) if kind == "trace" else step(case, args.calls)))
        return 0
    out_path = Path(args.out or ROOT / "profiles" / "mono_fusion_high_timing.json")
    res = {"calls": args.calls, "collections": COLLECTIONS, "views": N, "geometry": list(GEOMETRY), "channels": C, "paths": list(PATHS),
           "yardsticks": list(YARDSTICKS), "failed_step": None, "cases": {}}
    rc = 0
    for case in args.cases:
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT), sys.executable, __file__, "--calls", str(args.calls), "--step", case, "timing"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("STEP_RESULT ")]
        if r.returncode != 0 or not lines:
            res["failed_step"] = {"case": case, "returncode": r.returncode, "stderr": r.stderr[-1500:]}
            print("FAILED", res["failed_step"], flush=True)
            rc = 1
            break                                               # nothing is started on the GPU after a failed step
        entry = res["cases"][case] = json.loads(lines[0][len("STEP_RESULT "):])
        entry["summary"] = summary(entry)
        print(case, json.dumps(entry["summary"]), flush=True)
    if rc == 0:
        import torch

        from splatter360_amd import _lib
        res["device"], res["source_hash"] = torch.cuda.get_device_name(0), _lib.source_hash()
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(res, indent=1) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
