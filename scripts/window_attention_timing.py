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
around one call, launch overhead included) after 3 warm-up calls."""
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
STEP_LIMIT = {"native": 240, "torch": 240, "accuracy": 400}     # seconds, per child


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "window_attention_timing.json"))
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--cases", nargs="*", default=list(CASES))
    ap.add_argument("--sides", nargs="*", default=["native", "torch", "accuracy"])
    ap.add_argument("--step", nargs=3, metavar=("CASE", "SHIFT", "SIDE"), help="run one step in this process and print its JSON")
    args = ap.parse_args()
    if args.step:
        case, shift, side = args.step
        print("STEP_RESULT " + json.dumps(step(case, bool(int(shift)), side, args.calls)))
        return 0
    out_path = Path(args.out)
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
