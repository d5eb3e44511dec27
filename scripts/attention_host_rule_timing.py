"""Per-call time of the window attention and the QKV attention on two builds of this repository, a parent checkout (built, with
its own tests/) and this tree, the two alternating on one box -> profiles/attention_host_rule_timing.json.

    python scripts/attention_host_rule_timing.py --parent DIR [--out profiles/attention_host_rule_timing.json] [--rounds 10]

Legs: the cases of scripts/window_attention_timing.py (shift off and on) and scripts/qkv_attention_timing.py and the tiny shapes
of tests/test_gpu_attention_argument_rule.py, where host time dominates; precision "highest" and "high"; forward and forward +
backward through the autograd node.  A figure is the median of 8 (erp, cube_cross), 30 (cube_self), 50 (qkv) or 1000 (tiny) calls
(HIP events around one call, launch overhead included) after 3 warm-up calls.  Per leg: every round's figure for both builds, the
parent's min, max and median over its rounds, the new build's median and whether it lies inside the parent's min-max (and how
many legs lie above the parent's max, where a wrapper's per-call work grew, and below its min, where it shrank).  Under
`bench`: `python bench.py --gpus 1 --steps 20 --warmup 5` in each tree, parent, new, parent, new.

The driver starts no GPU work itself: every (round, build) and every bench run is a child process under its own `timeout` with
that build's tree as working directory and PYTHONPATH, one after the other, and the first one that fails ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
WINDOW = {"erp_self": (2, 0, 128, 256, 2), "erp_cross": (2, 1, 128, 256, 2), "cube_self": (12, 0, 64, 64, 2), "cube_cross": (12, 11, 64, 64, 2)}
QKV = {"costvolume": (2, 2, 4, 2048), "depth": (2, 2, 1, 2048)}
TINY_CALLS = 1000


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
    return statistics.median(ms)


def child():
    """One build's legs, in the process whose working directory is that build's tree."""
    import torch
    sys.path.insert(0, str(Path.cwd() / "tests"))
    import qkv_attention_reference as QR
    import window_attention_reference as WR
    from splatter360_amd import qkv_attention as qa, window_attention as wa

    res = {}

    def legs(tag, fn, inputs, g, grads, calls):
        def forward():
            with torch.no_grad():
                return fn(*inputs)
        res[f"{tag}/fwd_ms"] = timed(forward, calls)
        res[f"{tag}/fwd_bwd_ms"] = timed(lambda: grads(fn, *inputs, g), calls)

    for precision in ("highest", "high"):
        for case, (b, m, h, w, k) in WINDOW.items():
            for shift in (0, 1):
                q, kk, v, g = WR.random_case(b, m, h, w, c=128, seed=11, device="cuda:0")
                fn = lambda a, bb, cc: wa.window_attention(a, bb, cc, height=h, width=w, num_splits=k, with_shift=bool(shift), precision=precision)
                legs(f"window_attention/{case}_shift{shift}/{precision}", fn, (q, kk, v), g, WR.gradients, 30 if case == "cube_self" else 8)
                del q, kk, v, g
        q, kk, v, g = WR.random_case(1, 0, 4, 8, c=32, seed=11, device="cuda:0")
        fn = lambda a, bb, cc: wa.window_attention(a, bb, cc, height=4, width=8, num_splits=2, with_shift=True, precision=precision)
        legs(f"window_attention/tiny_shift1/{precision}", fn, (q, kk, v), g, WR.gradients, TINY_CALLS)
        for case, (n, views, heads, t) in QKV.items():
            qkv, g = QR.random_case(n, heads, t, ch=32, seed=11, device="cuda:0")
            fn = lambda x: qa.qkv_attention(x, heads, n_frames=views, cross_view=True, precision=precision)
            legs(f"qkv_attention/{case}/{precision}", fn, (qkv,), g, QR.gradients, 50)
        qkv, g = QR.random_case(2, 1, 35, ch=32, seed=11, device="cuda:0")
        fn = lambda x: qa.qkv_attention(x, 1, precision=precision)
        legs(f"qkv_attention/tiny_ragged/{precision}", fn, (qkv,), g, QR.gradients, TINY_CALLS)
    print("CHILD_RESULT " + json.dumps(res))


def run(root, cmd, limit):
    """cmd as a child in the tree `root` under `timeout`; its stdout lines, or None when it failed."""
    p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, *cmd], cwd=root, env=dict(os.environ, PYTHONPATH=str(root)),
                       capture_output=True, text=True)
    if p.returncode != 0:
        print("FAILED", root, cmd, p.returncode, p.stderr[-2000:], flush=True)
        return None
    return p.stdout.splitlines()


def summary(runs, bench):
    legs = {}
    for leg in sorted(runs["parent"][0]):
        p, n = [x[leg] for x in runs["parent"]], [x[leg] for x in runs["new"]]
        legs[leg] = {"parent_ms": p, "new_ms": n, "parent_min": min(p), "parent_max": max(p), "parent_median": statistics.median(p),
                     "new_median": statistics.median(n), "new_median_inside_parent_min_max": min(p) <= statistics.median(n) <= max(p)}
    return {"what": __doc__.split("\n\n")[2].replace("\n", " "), "rounds": len(runs["new"]), "legs": legs,
            "legs_inside": sum(v["new_median_inside_parent_min_max"] for v in legs.values()),
            "legs_above_parent_max": sum(v["new_median"] > v["parent_max"] for v in legs.values()),
            "legs_below_parent_min": sum(v["new_median"] < v["parent_min"] for v in legs.values()), "legs_total": len(legs), "bench": bench}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="the parent commit's tree, built")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "attention_host_rule_timing.json"))
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--child", action="store_true", help="run one build's legs in this process and print their JSON")
    args = ap.parse_args()
    if args.child:
        child()
        return 0
    builds = {"parent": Path(args.parent).resolve(), "new": ROOT}
    runs, bench = {b: [] for b in builds}, {b: [] for b in builds}
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    for r in range(args.rounds):
        for name, root in builds.items():
            lines = run(root, [str(Path(__file__).resolve()), "--child"], 180)
            if lines is None:
                return 1                                        # nothing is started on the GPU after a failed step
            runs[name].append(json.loads([ln for ln in lines if ln.startswith("CHILD_RESULT ")][0][len("CHILD_RESULT "):]))
            print("round", r, name, flush=True)
        out.write_text(json.dumps(summary(runs, bench), indent=1) + "\n")
    for _ in range(2):
        for name, root in builds.items():
            lines = run(root, ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], 300)
            if lines is None:
                return 1
            line = json.loads([ln for ln in lines if ln.startswith("{")][-1])
            bench[name].append({k: line[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step")})
            print("bench", name, bench[name][-1]["value"], flush=True)
    out.write_text(json.dumps(summary(runs, bench), indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
