"""Times the fused group norm + activation (+ residual) (splatter360_amd.group_norm.group_norm_act) against torch's lines
(F.group_norm / F.instance_norm, the activation, the add; float32 on the device) at the encoder's hm3d shapes
-> profiles/group_norm_timing.json.

    python scripts/group_norm_timing.py [--out profiles/group_norm_timing.json] [--calls 100] [--cases unet32_silu ...]

Cases (N, C, H, W), groups, activation, residual:
  unet32_silu, unet32_silu_res   (2, 32, 512, 1024) G = 8 silu     the depth U-Net's top level, without / with the skip add
  head32_gelu                    (2, 32, 512, 1024) G = 4 gelu     the head in front of it
  unet128_silu, head128_gelu     (2, 128, 128, 256) G = 8          the cost-volume U-Net's top level and its head
  erp_in_relu                    (2, 64, 256, 512) instance relu   the ERP backbone's ResidualBlock
  cube_in_relu                   (12, 64, 128, 128) instance relu  the cube backbone's

The driver starts no GPU work itself: every step (one case, one of native / torch / kernels) is a child process under its own
`timeout`, the steps run one after the other, and the first one that fails, is killed or times out ends the run (what was
measured until then is written, with the failed step's name).  native / torch: medians of `calls` calls (HIP events around one
call, launch overhead included) after 5 warm-up calls, forward (no_grad) and forward + backward (x, weight, bias and residual
require grad), and the peak of allocated bytes above the inputs.  kernels: the native step again, 20 calls, under
`rocprofv3 --kernel-trace --stats` in a run of its own; the k_gn_* kernels' average durations, and from them the achieved bytes
per second of the bytes the algorithm has to move (forward: 2 reads + 1 write of x, + 1 read with a residual; backward: 4 reads
+ 1 write) against the 6.3 TB/s streaming ceiling."""
import argparse
import csv
import json
import statistics
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

# name: (shape, groups (0 = instance), activation, residual)
CASES = {"unet32_silu": ((2, 32, 512, 1024), 8, "silu", False), "unet32_silu_res": ((2, 32, 512, 1024), 8, "silu", True),
         "head32_gelu": ((2, 32, 512, 1024), 4, "gelu", False), "unet128_silu": ((2, 128, 128, 256), 8, "silu", False),
         "head128_gelu": ((2, 128, 128, 256), 8, "gelu", False), "erp_in_relu": ((2, 64, 256, 512), 0, "relu", False),
         "cube_in_relu": ((12, 64, 128, 128), 0, "relu", False)}
STEP_LIMIT = {"native": 180, "torch": 180, "kernels": 240}      # seconds, per child
CEILING = 6.3e12                                                # bytes / s, streaming
KERNEL_CALLS = 20


def timed(fn, calls, warmup=5):
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
    out = fn()
    torch.cuda.synchronize()
    kept = torch.cuda.memory_allocated() - base
    del out
    return torch.cuda.max_memory_allocated() - base, kept


def step(case, side, calls):
    """One child's work: returns the figures of (case, side)."""
    import torch
    import torch.nn.functional as F

    from splatter360_amd import group_norm as gn

    shape, groups, act, with_res = CASES[case]
    gen = torch.Generator(device="cuda:0").manual_seed(5)
    affine = groups > 0
    x = torch.randn(shape, device="cuda:0", generator=gen).requires_grad_(True)
    w = (1 + 0.5 * torch.randn(shape[1], device="cuda:0", generator=gen)).requires_grad_(True) if affine else None
    b = (0.3 * torch.randn(shape[1], device="cuda:0", generator=gen)).requires_grad_(True) if affine else None
    res = torch.randn(shape, device="cuda:0", generator=gen).requires_grad_(True) if with_res else None
    g = torch.randn(shape, device="cuda:0", generator=gen)
    torch_act = {"silu": F.silu, "gelu": F.gelu, "relu": F.relu}[act]

    def native():
        return gn.group_norm_act(x, groups if affine else shape[1], w, b, 1e-5, act, res)

    def lines():
        y = torch_act(F.group_norm(x, groups, w, b, 1e-5) if affine else F.instance_norm(x, eps=1e-5))
        return y if res is None else res + y

    fn = lines if side == "torch" else native

    def forward():
        with torch.no_grad():
            return fn()

    def forward_backward():
        for t in (x, w, b, res):
            if t is not None:
                t.grad = None
        out = fn()
        out.backward(g)
        return out

    if side == "kernels":
        timed(forward_backward, KERNEL_CALLS, warmup=2)
        return {}
    out = {"fwd_ms": timed(forward, calls), "fwd_bwd_ms": timed(forward_backward, calls), "x_bytes": x.numel() * 4}
    out["fwd_peak_bytes"], _ = peak(forward)
    out["fwd_bwd_peak_bytes"], _ = peak(forward_backward)
    _, out["kept_after_fwd_bytes"] = peak(fn)                    # with autograd on and the output alive: out + what the node saved
    if side == "native":
        with torch.no_grad():
            out["max_abs_diff_from_torch_f32"] = (native() - lines()).abs().max().item()
    return out


def kernel_figures(case, stats_csv):
    """Average duration of each k_gn_* kernel from rocprofv3's kernel stats, and the achieved share of the streaming ceiling."""
    shape, _, _, with_res = CASES[case]
    xb = 4
    for s in shape:
        xb *= s
    kernels = {}
    with open(stats_csv, newline="") as f:
        for row in csv.DictReader(f):
            if "k_gn_" in row["Name"]:
                name = row["Name"][row["Name"].index("k_gn_"):].split("(")[0]
                kernels[name] = {"calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3}
    def total(prefixes):
        return sum(v["average_us"] for k, v in kernels.items() if k.startswith(prefixes)) * 1e-6
    fwd_s, bwd_s = total(("k_gn_stats", "k_gn_apply")), total(("k_gn_bwd_sums", "k_gn_bwd_apply", "k_gn_bwd_params"))
    fwd_bytes, bwd_bytes = (4 if with_res else 3) * xb, 5 * xb
    out = {"kernels": kernels, "fwd_kernels_us": fwd_s * 1e6, "bwd_kernels_us": bwd_s * 1e6, "fwd_bytes": fwd_bytes, "bwd_bytes": bwd_bytes}
    if fwd_s > 0 and bwd_s > 0:
        out["fwd_bytes_per_s"], out["bwd_bytes_per_s"] = fwd_bytes / fwd_s, bwd_bytes / bwd_s
        out["fwd_share_of_ceiling"], out["bwd_share_of_ceiling"] = fwd_bytes / fwd_s / CEILING, bwd_bytes / bwd_s / CEILING
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "group_norm_timing.json"))
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--cases", nargs="*", default=list(CASES))
    ap.add_argument("--sides", nargs="*", default=["native", "torch", "kernels"])
    ap.add_argument("--step", nargs=2, metavar=("CASE", "SIDE"), help="run one step in this process and print its JSON")
    args = ap.parse_args()
    if args.step:
        print("STEP_RESULT " + json.dumps(step(args.step[0], args.step[1], args.calls)))
        return 0
    out_path = Path(args.out)
    res = json.loads(out_path.read_text()) if out_path.exists() else {}
    res.update({"calls": args.calls, "kernel_calls": KERNEL_CALLS, "ceiling_bytes_per_s": CEILING, "failed_step": None})
    res.setdefault("cases", {})
    rc = 0
    for case in args.cases:
        shape, groups, act, with_res = CASES[case]
        entry = res["cases"].setdefault(case, {"shape": list(shape), "groups": groups or shape[1], "activation": act, "residual": with_res})
        for side in args.sides:
            child = [sys.executable, __file__, "--calls", str(args.calls), "--step", case, side]
            with tempfile.TemporaryDirectory() as tmp:
                if side == "kernels":
                    child = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "gn", "--", *child]
                r = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT[side]), *child], capture_output=True, text=True)
                lines = [ln for ln in r.stdout.splitlines() if ln.startswith("STEP_RESULT ")]
                stats = sorted(Path(tmp).rglob("*kernel_stats.csv"))
                if r.returncode != 0 or not lines:
                    res["failed_step"] = {"case": case, "side": side, "returncode": r.returncode, "stderr": r.stderr[-1500:]}
                    print("FAILED", res["failed_step"], flush=True)
                    rc = 1
                    break                                       # nothing is started on the GPU after a failed step
                if side != "kernels":
                    entry[side] = json.loads(lines[0][len("STEP_RESULT "):])
                else:
                    entry[side] = kernel_figures(case, stats[0]) if stats else {"error": "the profiler wrote no kernel stats file"}
            print(case, side, json.dumps(entry[side]), flush=True)
        if rc:
            break
        if "native" in entry and "torch" in entry:
            for key in ("fwd_ms", "fwd_bwd_ms"):
                entry[f"speedup_{key[:-3]}"] = entry["torch"][key]["median"] / entry["native"][key]["median"]
    if rc == 0:
        import torch

        from splatter360_amd import _lib
        res["device"], res["source_hash"] = torch.cuda.get_device_name(0), _lib.source_hash()
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(res, indent=1) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
