"""Times the fused mono-feature fusion (forward, and forward + backward) at the hm3d shape of the reference against the
reference's lines in float32 torch and records each path's peak of allocated memory -> profiles/mono_fusion_timing.json.

    python scripts/mono_fusion_timing.py [--out profiles/mono_fusion_timing.json] [--calls 50] [--cases vits vitb]

Cases: N = 2 context views, (face_w, equ_h, equ_w) = (64, 128, 256): 65 536 tokens, C = 128 and
  vits   Cm = 384     the configuration (config/model/encoder/costvolume.yaml: vit_type vits)
  vitb   Cm = 768     vit_type vitb

Paths:
  native   splatter360_amd.mono_fusion.mono_fusion: the stitch inside the kernels, no stitched map, no concatenation
  torch    tests/mono_fusion_reference.reference_lines: F.grid_sample as Cube2Equirec.forward calls it (under no_grad), torch.cat,
           the channel-last permute, F.linear, F.layer_norm, F.relu, F.linear, the permute back; autograd keeps the concatenation

The driver starts no GPU work itself: every step (one case) is a child process under its own `timeout`, the steps run one after
the other, and the first one that fails, is killed or times out ends the run (what was measured until then is written, with the
failed step's name).  Inside a child the two paths are ALTERNATED in one process, forward and forward + backward, the whole
collection three times over (the spread between the three medians is what a difference has to exceed).  Each time is the median
of `calls` calls (HIP events around one call, launch overhead included) after 3 warm-up calls; forward + backward takes the
gradients of erp_feat and the four parameters.  forward_tflops is 2 T ((C + Cm) C + C C) floating-point operations (the two
products; the stitch's are not counted) over the median of the forward's three medians; peak_fraction is that over the 157 TFLOP/s
float32 MFMA peak.  `--calls 6 --step vits trace` is the native path alone, the step whose kernel trace (`rocprofv3 --kernel-trace
--stats --`, a run of its own) is profiles/mono_fusion_kernel_trace.txt."""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

N, GEOMETRY, C = 2, (64, 128, 256), 128
CASES = {"vits": 384, "vitb": 768}
PATHS = ("native", "torch")
COLLECTIONS = 3
PEAK_TFLOPS = 157.0
STEP_LIMIT = 300                                               # seconds, per child


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


def _paths(case):
    import torch

    import mono_fusion_reference as R
    from splatter360_amd import mono_fusion as mf

    tensors, g = R.random_case(N, GEOMETRY, CASES[case], seed=11, device="cuda:0")
    fns = {"native": mf.mono_fusion, "torch": R.reference_lines}

    def forward(fn):
        def run():
            with torch.no_grad():
                return fn(*tensors)
        return run

    def forward_backward(fn):
        return lambda: R.gradients(fn, tensors, g)

    return fns, forward, forward_backward


def step(case, calls):
    """One child's work: both paths of one case, alternated inside each of COLLECTIONS collections."""
    from splatter360_amd import mono_fusion as mf

    fns, forward, forward_backward = _paths(case)
    tokens, cm = N * GEOMETRY[1] * GEOMETRY[2], CASES[case]
    res = {tag: {"fwd_ms": [], "fwd_bwd_ms": []} for tag in PATHS}
    for _ in range(COLLECTIONS):
        for leg, whole in (("fwd_ms", forward), ("fwd_bwd_ms", forward_backward)):
            for tag in PATHS:                                   # alternated: one path after the other inside every collection
                res[tag][leg].append(timed(whole(fns[tag]), calls))
    flops = 2.0 * tokens * ((C + cm) * C + C * C)
    for tag in PATHS:
        res[tag]["fwd_peak_bytes"], res[tag]["fwd_bwd_peak_bytes"] = peak(forward(fns[tag])), peak(forward_backward(fns[tag]))
        mid = statistics.median(c["median"] for c in res[tag]["fwd_ms"])
        res[tag]["forward_tflops"] = flops / (mid * 1e-3) / 1e12
        res[tag]["peak_fraction"] = res[tag]["forward_tflops"] / PEAK_TFLOPS
    res["tokens"], res["mono_channels"] = tokens, cm
    res["stitched_map_bytes"], res["concatenation_bytes"] = tokens * cm * 4, tokens * (C + cm) * 4
    res["scratch_bytes"] = mf.scratch_bytes(tokens, cm)
    return res


def trace_step(case, calls):
    """The step that profiles/mono_fusion_kernel_trace.txt is a kernel trace of: the native path alone, 3 + `calls` forward calls
    and 3 + `calls` forward + backward calls; returns the medians of the timed calls."""
    fns, forward, forward_backward = _paths(case)
    return {"fwd_ms": timed(forward(fns["native"]), calls)["median"], "fwd_bwd_ms": timed(forward_backward(fns["native"]), calls)["median"]}


def summary(entry):
    """Per leg: the three medians of both paths, their spread (max - min), torch over native, and whether native is behind torch
    by more than the larger of the two spreads."""
    out = {}
    for leg in ("fwd_ms", "fwd_bwd_ms"):
        med = {tag: [c["median"] for c in entry[tag][leg]] for tag in PATHS}
        mid = {tag: statistics.median(v) for tag, v in med.items()}
        spread = {tag: max(v) - min(v) for tag, v in med.items()}
        out[leg] = {"medians": med, "median": mid, "spread": spread, "torch_over_native": mid["torch"] / mid["native"],
                    "native_behind_torch": mid["native"] - mid["torch"] > max(spread.values()),
                    "native_ahead_of_torch": mid["torch"] - mid["native"] > max(spread.values())}
    out["fwd_bwd_peak_ratio_torch_over_native"] = entry["torch"]["fwd_bwd_peak_bytes"] / max(1, entry["native"]["fwd_bwd_peak_bytes"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/mono_fusion_timing.json")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--cases", nargs="*", default=list(CASES))
    ap.add_argument("--step", nargs=2, metavar=("CASE", "KIND"), help="run one step (KIND: timing or trace) in this process and print its JSON")
    args = ap.parse_args()
    if args.step:
        case, kind = args.step
        print("STEP_RESULT " + json.dumps(trace_step(case, args.calls) if kind == "trace" else step(case, args.calls)))
        return 0
    out_path = Path(args.out or ROOT / "profiles" / "mono_fusion_timing.json")
    res = {"calls": args.calls, "collections": COLLECTIONS, "views": N, "geometry": list(GEOMETRY), "channels": C,
           "float32_mfma_peak_tflops": PEAK_TFLOPS, "failed_step": None, "cases": {}}
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
