"""Times the fused multi-head QKV attention (forward, and forward + backward) at the two U-Net shapes of the hm3d configuration
(the replica configuration has the same: 512 x 1024 panoramas, attention at the 32 x 64 level, 2 views, 32 channels per head)
on three paths and records each one's peak of allocated memory -> profiles/qkv_attention_timing.json.

    python scripts/qkv_attention_timing.py [--out profiles/qkv_attention_timing.json] [--calls 50] [--cases costvolume ...]

Cases (N, views, heads, T), ch = 32, cross-view on, order legacy:
  costvolume (2, 2, 4, 2048)     the cost-volume U-Net: 128 channels, L = 4096
  depth      (2, 2, 1, 2048)     the depth U-Net: 32 channels, L = 4096

Paths:
  native   splatter360_amd.qkv_attention.qkv_attention on the qkv tensor as it lies
  torch    the reference's lines restated in float32 torch (tests/qkv_attention_reference.reference_lines): forms the
           [B heads, L, L] weights and their softmax, autograd keeps them
  window   splatter360_amd.window_attention.full_attention fed through permuted copies of q, k, v ([B heads, L, ch], token-major)
           and a permuted copy of its output back: the route that needs no new kernel

The driver starts no GPU work itself: every step (one case, one path) is a child process under its own `timeout`, the steps run
one after the other, and the first one that fails, is killed or times out ends the run (what was measured until then is
written, with the failed step's name).  Each time is the median of `calls` calls (HIP events around one call, launch overhead
included) after 3 warm-up calls.  forward_tflops is 4 B heads L^2 ch floating-point operations (the two products) over the
forward's median time.

    python scripts/qkv_attention_timing.py --high [--out profiles/qkv_attention_high_timing.json] [--collections 3]

times the "high" precision mode (bf16x3 products) against the default one -> profiles/qkv_attention_high_timing.json.  Paths:
  highest     qkv_attention(..., precision="highest"), the `native` path above
  high        qkv_attention(..., precision="high")
  torch       the float32 torch lines under torch.set_float32_matmul_precision('highest')
  torch_high  the same lines under 'high', the setting held over the backward too
One child process per case runs the four paths ALTERNATED: `collections` rounds, in each round every path in turn, `calls` calls
of the forward and `calls` of forward + backward.  A figure is the median of the rounds' medians, and `spread` the distance between
the largest and the smallest round median — what a difference between two paths has to exceed to mean anything.  Peaks are
bytes REQUESTED from the allocator (requested_bytes of torch.cuda.memory_stats)."""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

CASES = {"costvolume": (2, 2, 4, 2048), "depth": (2, 2, 1, 2048)}
CH = 32
PATHS = ("native", "torch", "window")
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


def path_function(path, n, views, heads):
    import qkv_attention_reference as R
    from splatter360_amd import qkv_attention as qa, window_attention as wa

    if path == "native":
        return lambda x: qa.qkv_attention(x, heads, n_frames=views, cross_view=True)
    if path == "torch":
        return lambda x: R.reference_lines(x, heads, views, True, "legacy")

    def window(x):
        q, k, v = (t.reshape(-1, t.shape[2], t.shape[3]).transpose(1, 2).contiguous() for t in R.split_heads(x, heads, views, True, "legacy"))
        a = wa.full_attention(q, k, v)                          # [B heads, L, ch]
        return R.merge_heads(a.transpose(1, 2).reshape(n // views, heads, CH, -1), views, True)
    return window


HIGH_PATHS = ("highest", "high", "torch", "torch_high")


def peak_requested(fn):
    import torch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_stats()["requested_bytes.all.current"]
    fn()
    torch.cuda.synchronize()
    return torch.cuda.memory_stats()["requested_bytes.all.peak"] - base


def high_step(case, calls, collections):
    """One child's work in the --high mode: the four paths of one case, alternated."""
    import torch

    import qkv_attention_reference as R
    from splatter360_amd import qkv_attention as qa

    n, views, heads, t = CASES[case]
    qkv, g = R.random_case(n, heads, t, ch=CH, seed=11, device="cuda:0")

    def under(setting, fn):
        def run(*a):
            before = torch.get_float32_matmul_precision()
            torch.set_float32_matmul_precision(setting)
            try:
                return fn(*a)
            finally:
                torch.set_float32_matmul_precision(before)
        return run

    lines = lambda x: R.reference_lines(x, heads, views, True, "legacy")
    fns = {"highest": lambda x: qa.qkv_attention(x, heads, n_frames=views, cross_view=True, precision="highest"),
           "high": lambda x: qa.qkv_attention(x, heads, n_frames=views, cross_view=True, precision="high"),
           "torch": lines, "torch_high": lines}
    setting = {"highest": "highest", "high": "highest", "torch": "highest", "torch_high": "high"}

    def legs(path):
        def forward():
            with torch.no_grad():
                return fns[path](qkv)
        return under(setting[path], forward), under(setting[path], lambda: R.gradients(fns[path], qkv, g))

    rounds = {path: {"fwd_ms": [], "fwd_bwd_ms": []} for path in HIGH_PATHS}
    for _ in range(collections):
        for path in HIGH_PATHS:
            forward, forward_backward = legs(path)
            rounds[path]["fwd_ms"].append(timed(forward, calls)["median"])
            rounds[path]["fwd_bwd_ms"].append(timed(forward_backward, calls)["median"])
    res = {}
    for path in HIGH_PATHS:
        forward, forward_backward = legs(path)
        res[path] = {key: {"median": statistics.median(ms), "spread": max(ms) - min(ms), "rounds": ms} for key, ms in rounds[path].items()}
        res[path]["fwd_peak_requested_bytes"], res[path]["fwd_bwd_peak_requested_bytes"] = peak_requested(forward), peak_requested(forward_backward)
    length = views * t
    for path in ("highest", "high"):
        res[path]["forward_tflops"] = 4.0 * (n // views) * heads * length * length * CH / (res[path]["fwd_ms"]["median"] * 1e-3) / 1e12
    for key in ("fwd_ms", "fwd_bwd_ms"):
        for other in ("highest", "torch", "torch_high"):
            res[f"high_speedup_over_{other}_{key[:-3]}"] = res[other][key]["median"] / res["high"][key]["median"]
    res["qkv_bytes"] = qkv.numel() * 4
    res["high_scratch_bytes"] = {"forward": qa.scratch_bytes(n, views, heads, t, False), "backward": qa.scratch_bytes(n, views, heads, t, True)}
    return res


def high_main(args):
    out_path = Path(args.out if args.out else ROOT / "profiles" / "qkv_attention_high_timing.json")
    res = {"calls": args.calls, "collections": args.collections, "head_channels": CH, "failed_step": None, "cases": {}}
    rc = 0
    for case in args.cases:
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT), sys.executable, __file__, "--calls", str(args.calls), "--collections",
               str(args.collections), "--high-step", case]
        r = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("STEP_RESULT ")]
        if r.returncode != 0 or not lines:
            res["failed_step"] = {"case": case, "returncode": r.returncode, "stderr": r.stderr[-1500:]}
            print("FAILED", res["failed_step"], flush=True)
            rc = 1
            break                                               # nothing is started on the GPU after a failed step
        res["cases"][case] = {"shape": dict(zip(("N", "views", "heads", "T"), CASES[case])), **json.loads(lines[0][len("STEP_RESULT "):])}
        print(case, json.dumps(res["cases"][case]), flush=True)
    if rc == 0:
        import torch

        from splatter360_amd import _lib
        res["device"], res["source_hash"] = torch.cuda.get_device_name(0), _lib.source_hash()
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(res, indent=1) + "\n")
    return rc


def step(case, path, calls):
    """One child's work: returns the figures of (case, path)."""
    import torch

    import qkv_attention_reference as R

    n, views, heads, t = CASES[case]
    qkv, g = R.random_case(n, heads, t, ch=CH, seed=11, device="cuda:0")
    fn = path_function(path, n, views, heads)

    def forward():
        with torch.no_grad():
            return fn(qkv)

    def forward_backward():
        return R.gradients(fn, qkv, g)

    res = {"fwd_ms": timed(forward, calls), "fwd_bwd_ms": timed(forward_backward, calls)}
    res["fwd_peak_bytes"], res["fwd_bwd_peak_bytes"] = peak(forward), peak(forward_backward)
    length = views * t
    res["forward_tflops"] = 4.0 * (n // views) * heads * length * length * CH / (res["fwd_ms"]["median"] * 1e-3) / 1e12
    res["qkv_bytes"] = qkv.numel() * 4
    res["one_score_tensor_bytes"] = (n // views) * heads * length * length * 4
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/qkv_attention_timing.json (--high: profiles/qkv_attention_high_timing.json)")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--cases", nargs="*", default=list(CASES))
    ap.add_argument("--paths", nargs="*", default=list(PATHS))
    ap.add_argument("--step", nargs=2, metavar=("CASE", "PATH"), help="run one step in this process and print its JSON")
    ap.add_argument("--high", action="store_true", help='time the "high" precision mode (the docstring)')
    ap.add_argument("--collections", type=int, default=3)
    ap.add_argument("--high-step", metavar="CASE", help="run one case of the --high mode in this process and print its JSON")
    args = ap.parse_args()
    if args.high_step:
        print("STEP_RESULT " + json.dumps(high_step(args.high_step, args.calls, args.collections)))
        return 0
    if args.high:
        return high_main(args)
    if args.out is None:
        args.out = str(ROOT / "profiles" / "qkv_attention_timing.json")
    if args.step:
        print("STEP_RESULT " + json.dumps(step(args.step[0], args.step[1], args.calls)))
        return 0
    out_path = Path(args.out)
    res = json.loads(out_path.read_text()) if out_path.exists() else {}
    res.update({"calls": args.calls, "head_channels": CH, "failed_step": None})
    res.setdefault("cases", {})
    rc = 0
    for case in args.cases:
        entry = res["cases"].setdefault(case, {"shape": dict(zip(("N", "views", "heads", "T"), CASES[case]))})
        for path in args.paths:
            cmd = ["timeout", "-k", "10", str(STEP_LIMIT), sys.executable, __file__, "--calls", str(args.calls), "--step", case, path]
            r = subprocess.run(cmd, capture_output=True, text=True)
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith("STEP_RESULT ")]
            if r.returncode != 0 or not lines:
                res["failed_step"] = {"case": case, "path": path, "returncode": r.returncode, "stderr": r.stderr[-1500:]}
                print("FAILED", res["failed_step"], flush=True)
                rc = 1
                break                                           # nothing is started on the GPU after a failed step
            entry[path] = json.loads(lines[0][len("STEP_RESULT "):])
            print(case, path, json.dumps(entry[path]), flush=True)
        if rc:
            break
        for other in ("torch", "window"):
            if "native" in entry and other in entry:
                for key in ("fwd_ms", "fwd_bwd_ms"):
                    entry[f"native_speedup_over_{other}_{key[:-3]}"] = entry[other][key]["median"] / entry["native"][key]["median"]
    if rc == 0:
        import torch

        from splatter360_amd import _lib
        res["device"], res["source_hash"] = torch.cuda.get_device_name(0), _lib.source_hash()
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(res, indent=1) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
