#!/usr/bin/env python3
"""bench.py — headline benchmark of the MI355X panoramic Gaussian-splat render path.

Metric (BASELINE.json): Msplats/s forward+backward at 1 048 576 Gaussians, 1024x512 ERP
(= six 256x256 cube faces + cube->ERP stitch), L2 pixel loss on the faces (the reference's loss,
src/loss/loss_mse.py:30-31), 1/2/4/8 GPUs with one target view per GPU (weak scaling) and one RCCL
exchange of the per-Gaussian gradients per step (default --grad-sync chunked: the factored form of DESIGN.md section 5 —
all-reduce of the packed mean / covariance / opacity gradients + all-gather of the per-Gaussian dL/dRGB factors, SH gradient
rebuilt locally — issued Gaussian range by Gaussian range INSIDE the backward; --grad-sync factored = the same bytes as one
exchange per step, optionally finished behind the next micro-batch's forward; --grad-sync allreduce = one all-reduce of all
352 B/Gaussian).

A "step" is one pass of the hot path per rank: fused six-face forward (L2 loss and its gradient seed fused
into the composite store unless --fused-loss 0), stitch, backward (+ the gradient exchange when N > 1; after
it every rank holds the summed gradients of all four parameter tensors).  Inputs are resident in HBM before
the timed region.

    python bench.py --gpus 1 --steps 200 --warmup 20
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

Rank 0 prints ONE JSON line.  `value` comes from the un-instrumented timed region of K steps and `ms_per_step` is that
region's time over K.  A plain run does only that: set up, warm up, time the K steps, write the outputs (--dump-outputs DIR),
print the line.  Everything else it can measure runs only with --full: the per-kernel durations behind `kernels` / `roofline`
(a second pass of the same K steps with HIP events recorded on the launch stream, s360_profile_*, so the numbers can be
compared with profiles/*kernel_stats*, rocprofv3 --kernel-trace --stats of this same command), the forward-only figure, the
exposed exchange, the lean-over-upstream list count, the other clouds, the adapter and drop-in legs and the CPU baselines.

    python bench.py --gpus 1 --steps 200 --warmup 20 --full
    python bench.py --gpus 1 --steps 200 --warmup 20 --dump-outputs DIR

--dump-outputs DIR writes what the timed path computed in its last timed step, as a caller of it receives it, to DIR/<name>.npy
(float32; rank 0): fwdbwd: the six faces, the stitched ERP, the loss and the gradients of the four parameter tensors (rows of a
fixed seeded sample of the Gaussians when the cloud has more than DUMP_ROWS); fwd / eval: the faces and the ERP (eval: of the
last of its three panoramas, plus that panorama's depth faces).  The inputs are seeded: the same arguments give the same inputs.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from splatter360_amd import _lib, decoder, distributed, rasterizer, stitch, synthetic  # noqa: E402

HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E spec (MI355X_MICROARCH.md); ~6300 measured-achievable
# VALU issue peak: 256 CUs x 4 SIMDs, one wave64 VALU instruction per 4 cycles per SIMD at 2.4 GHz (MI355X_MICROARCH.md chip
# table; profiles/ VALU-busy figures use the same 4-cycle slot) = 614.4 G wave-instructions / s
VALU_PEAK_GINST = 1024 * 2.4 / 4.0
DUMP_ROWS = 32768             # --dump-outputs: gradient rows written per parameter tensor (11.5 MB in all at deg-4 SH)
DUMP_IMAGE_BYTES = 8 << 20    # --dump-outputs: an image array beyond this is written as a fixed seeded sample of its elements
FWD_KERNELS = ("sh_eval", "preprocess", "tile_scan", "emit", "sort_tiles", "render", "cube2erp")
VALU_BOUND = ("render", "render_bwd")   # the two alpha composites: instruction-issue-bound


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # 200 timed steps (~155 ms): starting and draining the timed region costs ~0.8 ms whatever its length (the first step's launches
    # reach an idle device, the closing synchronise) — 20 steps carry 0.04 ms of it each (0.801 ms/step measured against 0.766 at 200,
    # same box, same minute; VERDICT r05 weak #17: a 15.8-ms timed region)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--mode", choices=("fwdbwd", "fwd", "eval"), default="fwdbwd",
                    help="eval = BASELINE configs[3] shape: 3 target panoramas x 6 faces, colour + depth, forward only")
    ap.add_argument("--pano-h", type=int, default=512, help="context/target ERP height (width = 2h)")
    ap.add_argument("--face", type=int, default=0, help="cube face size (default pano_h/2)")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beyond the headline figure (off by default): per-kernel durations and roofline, "
                         "forward-only figure, exposed exchange, lean-over-upstream list count, the other clouds, the adapter and "
                         "drop-in legs, the CPU baselines; the options below that select those legs apply with --full only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed path computed in its last step to DIR/<name>.npy (float32)")
    ap.add_argument("--cpu-baseline", type=int, default=1)
    ap.add_argument("--events-in-timed-region", type=int, default=0,
                    help="--full: 0 (default): the HIP events behind `kernels` / `roofline` are recorded in a second pass of the "
                         "same K steps, so the timed region carries no event records (they cost ~6 %% of the step: "
                         "1.53 vs 1.44 ms); 1: record them during the K timed steps")
    ap.add_argument("--fused-loss", type=int, default=1, help="1: L2 loss + its gradient seed fused into the render epilogue; "
                    "0: the reference's torch ops on the rendered faces")
    ap.add_argument("--defer-loss", type=int, default=1, help="fused loss: 1 (default) = the loss scalar is reduced inside the backward's first "
                    "launch (S360_FLAG_DEFER_LOSS: a training loop reads it after the step); 0 = by a launch of its own at the end of the forward")
    ap.add_argument("--overlap-exchange", type=int, default=1,
                    help="N>1, factored: 1 (default) = a micro-batch's exchange is finished only after the next micro-batch's forward "
                         "has been queued (it overlaps with that forward: a gradient-accumulation schedule); 0 = finished right "
                         "after its own backward")
    ap.add_argument("--grad-sync", choices=("chunked", "factored", "allreduce"), default="chunked",
                    help="N>1 gradient exchange: chunked (default: factored bytes, exchanged range by range inside the backward), "
                         "factored (one exchange per step, see --overlap-exchange) or allreduce (the full 352 B/Gaussian set)")
    ap.add_argument("--chunks", type=int, default=0, help="Gaussian ranges of the chunked exchange (0 = chosen from the cloud's size: one per 2 M Gaussians)")
    ap.add_argument("--exchange-mode", choices=("auto", "gather", "reduce"), default="auto",
                    help="form of the exchange: gather = ONE coalesced all-gather per range + local sum (auto up to 2 ranks), "
                         "reduce = all-reduce of the packed rows + all-gather of the dRGB rows (auto beyond)")
    ap.add_argument("--forward-figure", type=int, default=1,
                    help="fwdbwd mode: 1 (default) = K more forward-only steps after the timed region, reported as `forward_only` "
                         "(BASELINE configs[1]); 0 = skip them (the rocprofv3 passes of scripts/collect_profiles.sh: per-kernel averages "
                         "then hold the training form of every kernel only)")
    ap.add_argument("--atomic-grads", type=int, default=0, help="1: S360_FLAG_ATOMIC_GRADS (float32 atomics in the backward composite instead of the "
                    "deterministic partial-record gather; opt-in, not the headline configuration)")
    ap.add_argument("--workloads", type=int, default=1,
                    help="fwdbwd, 1 GPU: 1 (default) = after the headline measurement, time the same step on two more clouds of the same size "
                         "(SURVEY 8(d)'s uniform-random stress cloud and a surface-like cloud: coherent depth, opacity >= 0.9) and the "
                         "per-face drop-in training step of the unchanged reference (`dropin_train`); 0 = skip them")
    ap.add_argument("--split-lists", choices=("auto", "1", "0"), default="auto",
                    help="S360_FLAG_SPLIT_LISTS — long tile lists whose pixels do not saturate are composited segment-parallel (forward and "
                         "backward): auto (default, the product's default) = set for the calls that follow a forward which reported a quadrant worth "
                         "splitting; 1 = always; 0 = never (every list one sequential chain)")
    ap.add_argument("--single-rank-rccl", type=int, default=0,
                    help="1 (with --gpus 1): create a ONE-rank process group with backend nccl (= RCCL) and run the chunked exchange through "
                         "its collective branch (distributed.ExchangeConfig(force_collectives=True)) — the all-reduces / all-gathers really "
                         "go through RCCL on its own streams beside the backward's kernels; what a one-GPU box can show of the N > 1 path")
    ap.add_argument("--dry-run", type=int, default=0,
                    help="1: launch / rendezvous / collectives only (no GPU work, value = null): lets the CPU test suite exercise "
                         "`python bench.py --gpus N` end to end with the gloo backend")
    return ap.parse_args()


def self_launch(a):
    """`python bench.py --gpus N` started plainly (no torchrun environment): become the launcher — one process per GPU under
    torch.distributed.run on 127.0.0.1 (the driver's own N>1 command line), rank 0's JSON line passes through on stdout.
    Reference behaviour: Lightning starts one DDP process per device itself (/root/reference/src/main.py:117-130)."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), str(Path(__file__).resolve())] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "8")
    raise SystemExit(subprocess.run(cmd, env=env).returncode)


def dry_run(a, rank, local_rank, world):
    """Everything around the hot path, nothing of it: rendezvous, one gradient-shaped all-reduce through the product's own
    helper, the barrier + max-over-ranks timing protocol, the JSON line."""
    import torch.distributed as dist
    dev = torch.device("cpu")
    g = [torch.full((1000, k), float(rank + 1)) for k in (3, 9, 75, 1)]
    distributed.barrier()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        distributed.allreduce_gradients(g)
    distributed.barrier()
    dt = distributed.max_over_ranks(time.perf_counter() - t0, dev)
    ok = all(abs(float(t[0, 0]) - sum(range(1, world + 1)) * (world ** (a.steps - 1))) < 1e-3 * world ** a.steps for t in g) if world > 1 else True
    info = distributed.rank_report(dev)
    if rank == 0:
        print(json.dumps({"metric": "dry run (no GPU work)", "value": None, "unit": "Msplats/s", "n_gpus": world, "steps": a.steps,
                          "warmup": a.warmup, "ms_per_step": dt / max(a.steps, 1) * 1e3, "higher_is_better": True, "scaling": "weak",
                          "vs_baseline": None, "dtype": "f32", "data": "synthetic", "dry_run": True, "allreduce_ok": bool(ok),
                          "config": {"workload": "dry run"}, **info}), flush=True)
    if world > 1:
        dist.destroy_process_group()


def cpu_baseline(cloud, face_w, near, far, mode):
    """The CPU oracle (C restatement, OpenMP) on ONE ERP view of the same cloud: six faces forward
    (+ backward), timed on this host's cores."""
    sys.path.insert(0, str(ROOT / "tests"))
    import numpy as np
    from helpers import boundary_tensors, face_settings  # settings exactly as the reference glue builds them
    from oracle import oracle
    oracle.set_parallel_backward(True)
    cores = os.cpu_count() or 1
    t0 = time.time()
    for face in range(6):
        S = face_settings(face, face_w, face_w, near=near, far=far)
        means, cov6, shs, opac = boundary_tensors(cloud, S["scale"])
        orc = oracle.rasterize(S, means3D=means, cov3D_precomp=cov6, opacities=opac, shs=shs)
        f = orc.forward()
        if mode == "fwdbwd":
            orc.backward((2.0 / f["image"].size) * (f["image"] - 0.5))
        del orc
    dt = time.time() - t0
    oracle.set_parallel_backward(False)
    g = cloud["means"].shape[0]
    return dict(value=g / dt / 1e6, unit="Msplats/s", cores=cores, kind="port",
                sample=f"1 ERP view (6 faces {face_w}x{face_w}) of the same {g}-Gaussian cloud, {mode}, "
                       f"oracle/s360_oracle.c with OpenMP, {dt:.1f} s incl. boundary-tensor prep")


def cpu_baseline_torch():
    """BASELINE configs[0]: the PyTorch-CPU restatement of the composite (oracle/torch_ref.py) on 10 000 Gaussians, one
    256x128 ERP view = six 64x64 faces, forward + backward, all host cores.  (The reference has no CPU path; this times
    the project's own torch restatement, as SURVEY.md 8(d) asks.)"""
    sys.path.insert(0, str(ROOT / "tests"))
    import numpy as np
    from helpers import boundary_tensors, face_settings
    from oracle import torch_ref
    # 8 threads: these are thousands of small tensor ops — with one thread per core of a 256-core host the intra-op pool's
    # fork/join cost dominates (measured: 1 137 s with 256 threads against 1.6 s with 8)
    cores = min(8, os.cpu_count() or 1)
    prev_threads = torch.get_num_threads()
    torch.set_num_threads(cores)
    cloud = synthetic.uniform_cloud(10_000, seed=0, extent=3.0, scale_range=(0.02, 0.3))
    t0 = time.time()
    for face in range(6):
        S = face_settings(face, 64, 64)
        means, cov6, shs, opac = boundary_tensors(cloud, S["scale"])
        t = lambda x: torch.tensor(x, dtype=torch.float32, requires_grad=True)
        m, c, s_, o = t(means), t(cov6), t(shs), t(opac)
        img = torch_ref.render(S, m, c, o, shs=s_)
        ((img - 0.5) ** 2).mean().backward()
    dt = time.time() - t0
    torch.set_num_threads(prev_threads)
    return dict(value=10_000 / dt / 1e6, unit="Msplats/s", cores=cores, kind="port",
                sample=f"BASELINE configs[0]: 10000 Gaussians, 256x128 ERP (6 faces 64x64), fwd+bwd, oracle/torch_ref.py "
                       f"(PyTorch CPU, {cores} threads), {dt:.1f} s")


def dump_outputs(d, out, params):
    """--dump-outputs: what the timed path computed in its last step, as its caller receives it, to d/<name>.npy in float32 (under
    40 MB in all).  Images: whole, or above DUMP_IMAGE_BYTES the flattened elements at the sorted indices
    numpy.random.default_rng(1).choice(numel, DUMP_IMAGE_BYTES // 4, replace=False); gradients (fwdbwd): whole, or the rows of a
    seeded sample of DUMP_ROWS Gaussians, whose indices are written too (grad_rows.npy).  Same seeds every run."""
    import numpy as np
    d.mkdir(parents=True, exist_ok=True)

    def save(name, t):
        np.save(d / f"{name}.npy", t.detach().float().cpu().numpy())

    for name in ("faces", "depth", "erp"):
        t = out.get(name)
        if t is None:
            continue
        if t.numel() * 4 <= DUMP_IMAGE_BYTES:
            save(name, t)
        else:
            n = DUMP_IMAGE_BYTES // 4
            idx = torch.from_numpy(np.sort(np.random.default_rng(1).choice(t.numel(), n, replace=False))).to(t.device)
            save(name, t.reshape(-1).index_select(0, idx))
    if params is None:
        return
    if out.get("loss") is not None:
        save("loss", out["loss"])
    G = params[0].shape[0]
    idx = None
    if G > DUMP_ROWS:
        idx = torch.from_numpy(np.sort(np.random.default_rng(0).choice(G, DUMP_ROWS, replace=False))).to(params[0].device)
        np.save(d / "grad_rows.npy", idx.cpu().numpy().astype(np.float64))
    for name, p in zip(("means", "covariances", "harmonics", "opacities"), params):
        if p.grad is not None:
            save(f"grad_{name}", p.grad if idx is None else p.grad.index_select(0, idx))


def main():
    a = parse()
    if a.events_in_timed_region and not a.full:
        raise SystemExit("--events-in-timed-region 1 records the per-kernel figures of --full: pass --full")
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(a)      # does not return
    rasterizer.ATOMIC_GRADS = bool(a.atomic_grads)
    rasterizer.LAZY_SHRINK = True    # check="lazy" calls sized at 1.25 x the largest instance count seen (config.workspace_bytes_*): the
                                     # bench's scenes do not change between steps; the library default keeps the first-call guess as a floor
    rasterizer.SPLIT_LONG_LISTS = "auto" if a.split_lists == "auto" else bool(int(a.split_lists))
    rank, local_rank, world = distributed.init()
    if a.single_rank_rccl and world == 1 and not a.dry_run:
        import socket
        import torch.distributed as dist
        sock = socket.socket()
        sock.bind(("127.0.0.1", 0))
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(sock.getsockname()[1]))
        sock.close()
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        torch.cuda.set_device(0)
        dist.init_process_group(backend="nccl", rank=0, world_size=1)
    if a.gpus != world:
        raise SystemExit(f"--gpus {a.gpus} but the launcher started {world} rank(s)")
    if a.dry_run:
        return dry_run(a, rank, local_rank, world)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (no CPU fallback in the product path)")
    if world > 1 and "S360_FORCE_DEVICE" not in os.environ and torch.cuda.device_count() < world:
        raise SystemExit(f"--gpus {world} but only {torch.cuda.device_count()} GPU(s) are visible")
    dev = torch.device("cuda", torch.cuda.current_device())  # distributed.init() pinned cuda:LOCAL_RANK
    _lib.lib()

    pano_h, pano_w = a.pano_h, 2 * a.pano_h
    face_w = a.face or pano_h // 2
    cloud = synthetic.encoder_like_cloud(pano_h, pano_w, n_context=2, d_sh=25, seed=0)
    G = cloud["means"].shape[0]
    def to_params(c):
        return [torch.tensor(c[k], device=dev, requires_grad=(a.mode == "fwdbwd")) for k in ("means", "covariances", "harmonics", "opacities")]

    params = to_params(cloud)
    cur = {"params": params, "check": "lazy"}     # what step_train renders (the extra workloads swap the cloud in)
    # one target panorama per rank (identity rotation, small per-rank offsets)
    pose = torch.tensor(synthetic.target_pano_pose((0.05 * rank, 0.02 * rank, -0.03 * rank)), device=dev)
    # what the reference's dataloader hands the decoder for one target panorama: 6 face cameras
    ext, K, near, far = decoder.cube_cameras(pose, 0.1, 10.0)
    bg = torch.zeros(3, device=dev)
    gt = torch.full((6, 3, face_w, face_w), 0.5, device=dev)
    c2e = stitch.Cube2Equirec(face_w, 2 * face_w, 4 * face_w).to(dev)   # target ERP = (2 fw) x (4 fw)
    out = {}

    eval_poses = [decoder.cube_cameras(torch.tensor(synthetic.target_pano_pose((0.1 * i, 0.0, -0.05 * i)), device=dev), 0.1, 10.0)
                  for i in range(3)]

    def step_eval():
        # evaluation_index_replica.json: 3 target views per scene -> 18 faces, colour + depth (test_step :336-345)
        for (e, k, n, f) in eval_poses:
            col, dep = decoder.render_views_fused(e, k, n, f, (face_w, face_w), bg, *params, check="lazy", shared_campos=True, depth_mode="depth",
                                                  views=decoder.pack_camera_views(e, k, n, f, bg))
            out["erp"] = c2e.stitch_rendered(col)
            out["faces"] = col
            if a.dump_outputs:
                out["depth"] = dep

    one = torch.ones((), device=dev)
    pending = [None]   # the previous micro-batch's gradient exchange, still in flight (N > 1)

    def finish_pending():
        if pending[0] is not None:
            out["grads"] = pending[0].finish()     # waits (on the stream) for the collectives, rebuilds dL/dSH locally
            pending[0] = None

    local_only = [False]   # N > 1: steps without the exchange, to quote how much of it a step exposes

    def step_train():
        params = cur["params"]
        for p in params:
            p.grad = None
        views = decoder.pack_camera_views(ext, K, near, far, bg)  # camera glue of this step: one kernel (s360_pack_views)
        ex = exchange_cfg if (chunked and not local_only[0]) else None
        kw = dict(check=cur["check"], shared_campos=True, views=views, defer_sh=factored and not local_only[0], exchange=ex)
        if a.mode == "fwdbwd" and a.fused_loss:   # LossMse fused into the composite store
            faces, fm = decoder.render_views_fused(ext, K, near, far, (face_w, face_w), bg, *params, mse_target=gt, mse_defer=bool(a.defer_loss), **kw)
            loss = fm.loss
        else:
            faces = decoder.render_views_fused(ext, K, near, far, (face_w, face_w), bg, *params, **kw)
            loss = ((faces - gt) ** 2).mean() if a.mode == "fwdbwd" else None
        out["erp"] = c2e.stitch_rendered(faces.detach())
        # factored + overlap: the forward above was queued while the PREVIOUS micro-batch's exchange is still running on the
        # communicator's stream (gradient accumulation over micro-batches)
        finish_pending()
        if a.mode == "fwdbwd":
            loss.backward(one)   # the seed autograd would otherwise allocate and fill every step.  chunked: the per-Gaussian
                                 # gradients come back summed over the ranks (the exchange runs inside this backward)
            if factored and not local_only[0]:   # all-reduce 40 B/Gaussian (one packed buffer) + all-gather 16 B/Gaussian/rank
                pending[0] = distributed.start_factored_exchange(*params, rasterizer.deferred_of(faces))
                if not a.overlap_exchange:
                    finish_pending()
            elif world > 1 and not chunked and not local_only[0]:
                distributed.allreduce_gradients([p.grad for p in params])
        out["faces"] = faces
        if a.dump_outputs:
            out["loss"] = loss

    forced = bool(a.single_rank_rccl) and world == 1     # one RCCL rank, collectives really issued
    factored = world > 1 and a.mode == "fwdbwd" and a.grad_sync == "factored"
    chunked = (world > 1 or forced) and a.mode == "fwdbwd" and a.grad_sync == "chunked"
    exchange_cfg = distributed.ExchangeConfig(n_chunks=a.chunks or None, force_collectives=forced,
                                              mode=None if a.exchange_mode == "auto" else a.exchange_mode) if chunked else None
    ex_bounds, ex_mode = distributed.exchange_plan(G, world, a.chunks or None, None if a.exchange_mode == "auto" else a.exchange_mode)
    step = step_eval if a.mode == "eval" else step_train
    views_per_step = 3 if a.mode == "eval" else 1

    def sync():
        torch.cuda.synchronize(dev)
        distributed.barrier()
        torch.cuda.synchronize(dev)

    for _ in range(a.warmup):
        step()
    finish_pending()
    if a.warmup:
        # check="lazy" calls size their binning buffers and backward scratch from the instance count the PREVIOUS call of the shape
        # reported into pinned host memory (S360Params.header_mirror; x 1.25 instead of the first-call guess 1.5 G V) — no read-back,
        # no synchronisation in the loop.  The warm-up has been through that; one more step so that the timed steps all run at the
        # steady-state size even if the host ran ahead of the device during the warm-up.
        torch.cuda.synchronize(dev)
        step()
        finish_pending()
    sync()
    if a.events_in_timed_region:
        _lib.profile_enable(True)
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    finish_pending()     # the last exchange completes INSIDE the timed region
    sync()
    dt = distributed.max_over_ranks(time.perf_counter() - t0, dev)
    ms_per_step = dt / a.steps * 1e3
    st_timed = rasterizer.last_state()     # workspace of the last timed step (a training workspace in fwdbwd mode)
    if a.dump_outputs and rank == 0:
        dump_outputs(Path(a.dump_outputs), out, cur["params"] if a.mode == "fwdbwd" else None)

    extra = {}
    if a.full and a.mode == "fwdbwd" and a.forward_figure:
        # (1) the forward-only figure of BASELINE configs[1] (north_star: ">= 400 Msplats/s forward") from the same process: K
        # more steps with nothing requiring grad (inference form of the call: no backward state is written)
        frozen = [p.detach() for p in params]   # nothing requires grad: the call takes its inference form (S360_FLAG_FORWARD_ONLY)

        def step_fwd():
            with torch.no_grad():
                views = decoder.pack_camera_views(ext, K, near, far, bg)
                faces = decoder.render_views_fused(ext, K, near, far, (face_w, face_w), bg, *frozen, check="lazy", shared_campos=True, views=views)
                out["erp_fwd"] = c2e.stitch_rendered(faces)
        for _ in range(2):
            step_fwd()
        sync()
        t1 = time.perf_counter()
        for _ in range(a.steps):
            step_fwd()
        sync()
        dt_f = distributed.max_over_ranks(time.perf_counter() - t1, dev)
        extra["forward_only"] = {"value": G * world / (dt_f / a.steps) / 1e6, "unit": "Msplats/s", "ms_per_step": dt_f / a.steps * 1e3,
                                 "steps": a.steps, "what": "BASELINE configs[1]: fused six-face forward + stitch, inference form of the call"}
    if a.full and a.mode == "fwdbwd":
        if world > 1 or forced:
            # (2) how much of the gradient exchange a step exposes: the same K steps without it
            local_only[0] = True
            for _ in range(2):
                step()
            sync()
            t1 = time.perf_counter()
            for _ in range(a.steps):
                step()
            sync()
            dt_l = distributed.max_over_ranks(time.perf_counter() - t1, dev)
            local_only[0] = False
            extra["exchange"] = {"mode": a.grad_sync, "ms_per_step_without_exchange": dt_l / a.steps * 1e3,
                                 "exposed_ms_per_step": (dt - dt_l) / a.steps * 1e3,
                                 "form": ex_mode if a.grad_sync == "chunked" else a.grad_sync, "ranges": len(ex_bounds),
                                 "collective_calls_per_step": len(ex_bounds) * (1 if ex_mode == "gather" else 2) if a.grad_sync == "chunked" else None,
                                 "bytes_received_per_rank": ((world - 1) * 56 * G if (a.grad_sync == "chunked" and ex_mode == "gather") else
                                                             (2 * (world - 1) / world * 40 + (world - 1) * 16) * G) if a.grad_sync != "allreduce"
                                 else 2 * (world - 1) / world * 352 * G}
    extra.update(distributed.rank_report(dev))   # backend, rccl_ranks (as the process group reports it), device index of every rank

    st = rasterizer.last_state()
    if st.overflowed():
        raise SystemExit("binning capacity overflowed during the timed region: result invalid")
    if st.split_errors():
        raise SystemExit("k_render_tail reported a watchdog error during the timed region: result invalid")
    L = st.num_rendered()
    ws_fwd, ws_bwd = int(st_timed.layout.total_bytes), int(st_timed.layout.backward_bytes)   # scratch of a timed step (check="lazy")
    n_split = int(st_timed.header()[5].item()) if (st_timed.prm.flags & _lib.FLAG_SPLIT_LISTS) else 0
    tt = st.tensors()
    visible_pairs = int((tt["tiles_touched"] > 0).sum().item())
    assert torch.isfinite(out["faces"]).all() and torch.isfinite(out["erp"]).all()
    # contributing (pixel, entry) pairs of this step's render and the pairs the backward evaluates for them (measurement aid)
    n_contrib_pairs, n_bwd_pairs = st_timed.count_contributions() if (a.full and a.mode == "fwdbwd") else (None, None)
    # the same call with upstream's 3-sigma rectangles: how much the lean lists remove (identical images; tests/test_gpu_lean.py)
    L_upstream = L if a.full else None
    if a.full and rasterizer.LEAN_LISTS and a.mode != "eval":
        with torch.no_grad():
            decoder.render_views_fused(ext, K, near, far, (face_w, face_w), bg, *[p.detach() for p in params], shared_campos=True, lean=False)
        L_upstream = rasterizer.last_state().num_rendered()

    value = G * views_per_step * world / (dt / a.steps) / 1e6
    erp_w, erp_h = 4 * face_w, 2 * face_w          # the target ERP the six faces stitch into
    gm = f"{G / 2**20:g}M" if G % 2**18 == 0 else str(G)
    what = {"fwdbwd": "fwd+bwd", "fwd": "fwd", "eval": "fwd colour+depth, 3 ERP views"}[a.mode]
    if G == 1 << 20 and face_w == 256:
        cfg_name = {"fwdbwd": "BASELINE configs[2]", "fwd": "BASELINE configs[1]", "eval": "BASELINE configs[3] shape (synthetic cloud)"}[a.mode]
    elif face_w == 512:
        cfg_name = "BASELINE configs[4] single-rank shape" + (" (G = 2 context panoramas at 2048x1024)" if G == 1 << 22 else " (resolution-decoupled cloud)")
    else:
        cfg_name = "non-BASELINE size"

    figures = {}   # --full: kernels, roofline, path_roofline
    if a.full:
        # ---- per-kernel durations: HIP events around every kernel group, recorded on the stream the kernels run on,
        # in a second pass of the same K steps (default) or inside the timed region itself (--events-in-timed-region 1)
        if not a.events_in_timed_region:
            _lib.profile_enable(True)
            for _ in range(a.steps):
                step()
            finish_pending()
            torch.cuda.synchronize(dev)
        prof = _lib.profile_collect()
        _lib.profile_enable(False)
        kernels = {k: dict(avg_us=ms / n * 1e3, launches=n) for k, (ms, n) in prof.items() if n}
        dom = max(kernels, key=lambda k: kernels[k]["avg_us"] * kernels[k]["launches"])
        # kernel-interface (compulsory) bytes per launch, for the per-kernel table
        hw = 6 * face_w * face_w
        iface = dict(
            sh_eval=G * (300 + 12 + 16 + (36 if a.mode == "fwdbwd" else 0)),
            preprocess=G * (12 + 36 + 4 + 16) + 6 * G * 4 + visible_pairs * 57,
            render=L * (4 + 48) + hw * (12 + 8),
            sort_tiles=L * (8 + 8 + 4),
            emit=6 * G * 4 + visible_pairs * 32 + L * 8,
            render_bwd=L * (48 + 4) + hw * (12 + 8) + L * 48,
            gather_slots=L * (4 + 4) + L * 48 + visible_pairs * 48,
            preprocess_bwd=G * (12 + 36 + 36 + 1) + visible_pairs * (48 + 1) + G * (12 + 36 + 4 + 16),
            sh_bwd=G * (16 + 12 + 300),
            cube2erp=hw * 12 + (2 * face_w) * (4 * face_w) * (12 + 12),
        )
        for k, v in kernels.items():
            if k in iface:
                v["interface_bytes"] = iface[k]
                v["interface_GBps"] = iface[k] / (v["avg_us"] * 1e-6) / 1e9
        # SURVEY.md §8(d) compulsory bytes per splat, for THIS workload (350.5 / 684.5 at G = 1 048 576, 1024x512 ERP)
        face_bytes, erp_bytes = hw * 12, (2 * face_w) * (4 * face_w) * 12
        BYTES_FWD = 340.0 + (face_bytes + erp_bytes) / G
        BYTES_BWD = 340.0 + face_bytes / G + 340.0
        per_splat = BYTES_FWD if dom in FWD_KERNELS else BYTES_BWD
        dom_s = kernels[dom]["avg_us"] * 1e-6
        achieved = per_splat * G / dom_s / 1e9
        traffic = valu_busy = valu_insts = counter_bytes_step = None
        pmc_note = "no committed PMC profile"
        pmc = ROOT / "profiles" / "pmc_latest.json"
        if pmc.exists():   # PMC counters of the committed rocprofv3 passes (scripts/collect_profiles.sh), per launch
            try:
                blob = json.loads(pmc.read_text())
                stamp = blob.get("_meta", {})
                if stamp.get("source_hash") == _lib.source_hash() and stamp.get("gaussians") == G and stamp.get("face") == face_w:
                    rec = blob.get(dom, {})
                    traffic, valu_busy, valu_insts = rec.get("hbm_bytes_per_launch"), rec.get("valu_busy_frac"), rec.get("valu_insts_per_launch")
                    counter_bytes_step = stamp.get("counter_bytes_per_step")
                    pmc_note = f"PMC counters from profiles/pmc_latest.json (same kernel sources {stamp.get('source_hash')}, same workload)"
                else:   # never quote counters of other code or another workload: traffic stays null
                    pmc_note = (f"profiles/pmc_latest.json was collected from kernel sources {stamp.get('source_hash')} / G={stamp.get('gaussians')}"
                                f" (now {_lib.source_hash()} / G={G}): traffic not quoted")
            except Exception:
                traffic = None
        bytes_step = (BYTES_FWD + (BYTES_BWD if a.mode == "fwdbwd" else 0.0)) * G * views_per_step
        # ---- roofline, exactly as the measurement contract defines it: ALGORITHMIC bytes of the dominant kernel's phase (SURVEY 8(d):
        # 350.5 B/splat forward, 684.5 B/splat backward at this workload) x the splats one launch processes / that launch's duration
        # (HIP events on the launch stream), against the 8 TB/s HBM peak.  frac_path = the whole step's algorithmic bytes / step time.
        # The dominant kernels are alpha composites, whose own limit is VALU issue, so two VALU figures follow as extra keys:
        # valu_issue_frac = EXECUTED wave64 VALU instructions / issue peak (rises if the kernel executes more instructions: a
        # utilisation, not an efficiency) and valu_work_frac = the instructions the contributing (pixel, entry) pairs NEED
        # (pairs x MIN_INST lane-slots / 64) / issue peak — executing more instructions cannot raise that one.
        MIN_INST = {"render": 26, "render_bwd": 68}   # VALU issue slots per contributing pair (v_exp / v_rcp = 4 slots); DESIGN.md section 4
        a_inst = None if valu_insts is None else valu_insts / dom_s / 1e9
        work_inst = None if (n_contrib_pairs is None or dom not in MIN_INST) else n_contrib_pairs * views_per_step * MIN_INST[dom] / 64.0
        roofline = {"bound": "hbm", "kernel": dom, "achieved": achieved, "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBPS,
                    "traffic": traffic,
                    # what the kernel REALLY moves through HBM per unit time (PMC counter bytes / launch time / peak): `frac` prices the
                    # phase's algorithmic bytes against the kernel's duration, as the contract defines it — it is not "42 % of HBM"
                    "hbm_frac_kernel": None if traffic is None else traffic / dom_s / 1e9 / HBM_PEAK_GBPS,
                    "frac_path": bytes_step / (dt / a.steps) / 1e9 / HBM_PEAK_GBPS,
                    "algorithmic_bytes_per_launch": per_splat * G, "launch_us": kernels[dom]["avg_us"],
                    "valu_issue_frac": None if a_inst is None else a_inst / VALU_PEAK_GINST, "valu_insts_per_launch": valu_insts,
                    "valu_work_frac": None if work_inst is None else work_inst / dom_s / 1e9 / VALU_PEAK_GINST,
                    "valu_work_insts_per_launch": work_inst, "contributing_pairs": n_contrib_pairs, "backward_evaluated_pairs": n_bwd_pairs,
                    "valu_peak_Ginst_per_s": VALU_PEAK_GINST, "valu_busy_frac": valu_busy,
                    "note": f"frac = {per_splat:.1f} B/splat (SURVEY 8d, {'fwd' if dom in FWD_KERNELS else 'bwd'} phase) x {G} splats / "
                            f"{kernels[dom]['avg_us']:.1f} us (avg launch of the dominant kernel group, HIP events) / 8 TB/s; the group is an alpha "
                            "composite, VALU-issue-bound (DESIGN.md section 4): valu_* are the figures against 1024 SIMDs x 2.4 GHz / 4; " + pmc_note}
        figures = {"roofline": roofline,
                   "path_roofline": {"bytes_per_step": bytes_step, "achieved_GBps": bytes_step / (dt / a.steps) / 1e9,
                                     "frac_of_8TBps": bytes_step / (dt / a.steps) / 1e9 / HBM_PEAK_GBPS,
                                     "counter_bytes_per_step": counter_bytes_step,
                                     "counter_over_algorithmic": None if counter_bytes_step is None else counter_bytes_step / bytes_step},
                   "kernels": kernels}
    res = {
        "metric": f"Msplats/s {what} @{gm} Gaussians, {erp_w}x{erp_h} ERP",
        "value": value, "unit": "Msplats/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
        "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic",
        "config": {"workload": f"{cfg_name}: {G} encoder-like synthetic Gaussians (seed 0, deg-4 SH, from {a.n_context if hasattr(a, 'n_context') else 2} "
                               f"context panoramas {pano_w}x{pano_h}), {erp_w}x{erp_h} ERP = 6 faces {face_w}x{face_w} + stitch, {a.mode}"
                               + (", L2 loss on faces" + (" (fused epilogue" + (", scalar reduced in the backward's first launch)" if a.defer_loss else ")") if a.fused_loss else "") if a.mode == "fwdbwd" else "")
                               + (", lean tile lists" if rasterizer.LEAN_LISTS else ", upstream-compatible tile lists")
                               + (", ATOMIC gradient accumulation (opt-in, non-deterministic)" if rasterizer.ATOMIC_GRADS and a.mode == "fwdbwd" else ""),
                   "gaussians": G, "erp": [erp_w, erp_h], "face": face_w, "views_per_gpu": views_per_step,
                   "parallelism": f"view-sharded x{world}" + (
                       "" if not (world > 1 and a.mode == "fwdbwd") else
                       f", RCCL exchange inside the backward ({len(ex_bounds)} Gaussian range(s), " + ("ONE coalesced all-gather of packed 40 B/G + dRGB 16 B/G rows per range, summed locally" if ex_mode == "gather" else "all-reduce 40 B/G packed + all-gather dRGB 16 B/G/rank per range") + "; chunked exchange inside the backward)" if chunked else
                       ", RCCL factored grad exchange (all-reduce 40 B/G packed + all-gather dRGB 16 B/G/rank" + (", overlapped with the next micro-batch's forward" if a.overlap_exchange else "") + ")" if factored else
                       ", RCCL all-reduce of Gaussian grads"),
                   "num_rendered": L, "num_rendered_upstream_lists": L_upstream, "lean_over_upstream": None if L_upstream is None else L / max(L_upstream, 1),
                   "visible_pairs": visible_pairs, "split_lists": a.split_lists, "split_flag_set_in_timed_steps": bool(st_timed.prm.flags & _lib.FLAG_SPLIT_LISTS), "split_quadrants": n_split,
                   "wide_rectangles": int(st_timed.header()[4].item()), "coop_walk_flag_set_in_timed_steps": bool(st_timed.prm.flags & _lib.FLAG_COOP_WALK),
                   "workspace_bytes_forward": ws_fwd, "workspace_bytes_backward": ws_bwd if a.mode == "fwdbwd" else 0,
                   "max_instances": int(st_timed.prm.max_instances)},
        **figures,
        **extra,
    }
    if a.full and a.mode == "eval" and rank == 0:
        # the same 18 colour + 18 depth face renders through the reference-style per-face drop-in calls
        from types import SimpleNamespace
        gs = SimpleNamespace(means=params[0][None], covariances=params[1][None], harmonics=params[2][None], opacities=params[3][None])
        dec = decoder.DecoderSplattingCUDA().to(dev)
        e18 = torch.cat([e for (e, _, _, _) in eval_poses])[None]
        k18 = torch.cat([k for (_, k, _, _) in eval_poses])[None]
        n18 = torch.cat([n for (_, _, n, _) in eval_poses])[None]
        f18 = torch.cat([f for (_, _, _, f) in eval_poses])[None]
        with torch.no_grad():
            dec(gs, e18, k18, n18, f18, (face_w, face_w), depth_mode="depth")
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(3):
                dec(gs, e18, k18, n18, f18, (face_w, face_w), depth_mode="depth")
            torch.cuda.synchronize(dev)
        res["per_face_dropin_ms_per_step"] = (time.perf_counter() - t0) / 3 * 1e3
    if a.full and world == 1 and a.mode == "fwdbwd" and a.workloads:
        # ---- the same training step on two more clouds of the same size (every tuning decision of rounds 1-3 was taken on the
        # encoder-like cloud alone): SURVEY 8(d)'s uniform-random stress cloud, and a surface-like cloud (what a trained encoder
        # emits: spatially coherent depth, opacity >= 0.9 — the first surface hides most of what lies behind it)
        k2 = max(3, min(a.steps, 100))    # (round 6: 100 instead of 10 — the fixed cost of a timed region, see --steps)
        res["workloads"] = {}
        for name, make in (("uniform_U[-5,5]^3", lambda: synthetic.uniform_cloud(G, seed=0, extent=5.0)),
                           ("surface_like", lambda: synthetic.surface_like_cloud(pano_h, pano_w, n_context=2, seed=0))):
            cur["params"], cur["check"] = to_params(make()), "sync"
            step()                       # sizes the binning buffers (one synchronising call, re-rendered if the guess was short)
            cur["check"] = "lazy"
            for _ in range(2):
                step()
            sync()
            t1 = time.perf_counter()
            for _ in range(k2):
                step()
            sync()
            dtw = (time.perf_counter() - t1) / k2
            stw = rasterizer.last_state()
            _lib.profile_enable(True)     # per-kernel averages of this workload (second pass, HIP events, like the headline's)
            for _ in range(k2):
                step()
            torch.cuda.synchronize(dev)
            kw_us = {k: round(ms / n * 1e3, 1) for k, (ms, n) in _lib.profile_collect().items() if n}
            _lib.profile_enable(False)
            res["workloads"][name] = {"value": G / dtw / 1e6, "unit": "Msplats/s", "ms_per_step": dtw * 1e3, "steps": k2,
                                      "num_rendered": stw.num_rendered(), "overflowed": stw.overflowed(),
                                      "split_quadrants": int(stw.header()[5].item()) if (stw.prm.flags & _lib.FLAG_SPLIT_LISTS) else 0, "split_errors": stw.split_errors(),
                                      "wide_rectangles": int(stw.header()[4].item()), "coop_walk": bool(stw.prm.flags & _lib.FLAG_COOP_WALK),
                                      "workspace_bytes_forward": int(stw.layout.total_bytes), "workspace_bytes_backward": int(stw.layout.backward_bytes),
                                      "visible_pairs": int((stw.tensors()["tiles_touched"] > 0).sum().item()),
                                      "finite": bool(torch.isfinite(out["faces"]).all()), "kernels_avg_us": kw_us}
            cur["params"] = None
            torch.cuda.empty_cache()
        cur["params"], cur["check"] = params, "lazy"
        # ---- the adapter tail in front of the render: the encoder's raw outputs -> Gaussians -> the same training step,
        # as two steps (s360_adapter_forward, fused render, backward, s360_adapter_backward: the [G,3,25] harmonics / dL/dSH and the
        # covariances make a round trip through HBM) and FUSED (s360_forward_raw / s360_backward_raw)
        try:
            from splatter360_amd import adapter as _adapter
            gen = torch.Generator().manual_seed(0)
            nvc = 2
            rdep = torch.exp(torch.empty(nvc, pano_h * pano_w).uniform_(-0.69, 2.08, generator=gen)).to(dev)
            rop = torch.sigmoid(torch.randn(nvc, pano_h * pano_w, generator=gen)).to(dev)
            rraw = torch.randn(nvc, pano_h * pano_w, 82, generator=gen)
            rraw[..., 7:] *= 0.6
            rraw = rraw.to(dev)
            cext = torch.eye(4).repeat(nvc, 1, 1)
            cext[0, :3, 3] = torch.tensor([-0.4, 0.0, 0.1])
            cext[1, :3, 3] = torch.tensor([0.4, 0.0, -0.1])
            cext = cext.to(dev)
            crot = _adapter.sh_rotation_blocks(cext, 25)
            leaves = [t.requires_grad_(True) for t in (rdep, rop, rraw)]   # persistent leaves, gradients dropped per step like step_train's

            def step_two():
                for t in leaves:
                    t.grad = None
                d, o, r = leaves
                gA = _adapter.adapter_tail(cext, d, o, r, (pano_h, pano_w), 0.5, 15.0, sh_rotation=crot)
                views = decoder.pack_camera_views(ext, K, near, far, bg)
                faces, fm = decoder.render_views_fused(ext, K, near, far, (face_w, face_w), bg, gA.means.reshape(-1, 3), gA.covariances.reshape(-1, 3, 3),
                                                       gA.harmonics.reshape(-1, 3, 25), gA.opacities.reshape(-1), mse_target=gt, check="lazy",
                                                       shared_campos=True, views=views)
                fm.loss.backward()
                return faces

            def step_raw():
                for t in leaves:
                    t.grad = None
                d, o, r = leaves
                views = decoder.pack_camera_views(ext, K, near, far, bg)
                faces, _, _, fm = rasterizer.rasterize_raw(d.reshape(-1), o.reshape(-1), r.reshape(-1, 82), cext, views=views, image_height=face_w,
                                                           image_width=face_w, context_shape=(pano_h, pano_w), scale_min=0.5, scale_max=15.0,
                                                           sh_rotation=crot, mse_target=gt, check="lazy")
                fm.loss.backward()
                return faces

            apr = {}
            for nm, fn in (("two_step", step_two), ("fused_raw", step_raw)):
                for _ in range(3):
                    f_ = fn()
                sync()
                t1 = time.perf_counter()
                for _ in range(k2):
                    f_ = fn()
                sync()
                dta = (time.perf_counter() - t1) / k2
                _lib.profile_enable(True)
                for _ in range(k2):
                    fn()
                torch.cuda.synchronize(dev)
                ku = {k: round(ms / n * 1e3, 1) for k, (ms, n) in _lib.profile_collect().items() if n}
                _lib.profile_enable(False)
                apr[nm] = {"ms_per_step": dta * 1e3, "value": G / dta / 1e6, "unit": "Msplats/s", "kernels_avg_us": ku,
                           "finite": bool(torch.isfinite(f_).all())}
            apr["fused_over_two_step"] = apr["two_step"]["ms_per_step"] / apr["fused_raw"]["ms_per_step"]
            apr["what"] = ("encoder raw outputs (2 context panoramas, 82 floats + depth + opacity per pixel) -> adapter tail -> fused six-face training "
                           "step -> gradients w.r.t. the raw outputs (persistent leaf tensors, .grad dropped per step: what step_train does)")
            apr["bytes_not_moved_per_gaussian"] = {"forward": 340 + 340, "backward": 300 + 300 + 36}
            res["adapter_plus_render"] = apr
        except Exception as e:   # an extra leg, never a reason to lose the bench line
            res["adapter_plus_render"] = {"error": repr(e)}
        # ---- the path a user of the UNCHANGED reference is on without splatter360_amd.install(): its own decoder loop — one drop-in
        # `diff_gaussian_rasterization` call per face with the reference's torch camera glue and upstream's host synchronisation
        # (decoder_splatting_cuda.py:47-59 -> cuda_splatting.py:47-127), torch L2 loss on the faces, backward
        from types import SimpleNamespace
        gs = SimpleNamespace(means=params[0][None], covariances=params[1][None], harmonics=params[2][None], opacities=params[3][None])
        dec = decoder.DecoderSplattingCUDA().to(dev)

        def step_dropin():
            for p in params:
                p.grad = None
            colors = dec(gs, ext[None], K[None], near[None], far[None], (face_w, face_w)).color
            ((colors[0] - gt) ** 2).mean().backward()

        step_dropin()
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        for _ in range(3):
            step_dropin()
        torch.cuda.synchronize(dev)
        dtd = (time.perf_counter() - t1) / 3
        res["dropin_train"] = {"value": G / dtd / 1e6, "unit": "Msplats/s", "ms_per_step": dtd * 1e3, "steps": 3,
                               "fused_over_dropin": dtd / (dt / a.steps),
                               "what": "the same training step through the unchanged reference's decoder loop: six per-face drop-in rasteriser "
                                       "calls (torch camera glue, host sync per call), torch L2 loss, backward — what a user gets without "
                                       "splatter360_amd.install()"}
    if rank == 0 and a.full and a.cpu_baseline and a.mode != "eval":    # N > 1 too: rank 0's host cores, the other ranks wait at the teardown
        res["cpu_baseline"] = cpu_baseline(cloud, face_w, 0.1, 10.0, a.mode)
        try:
            res["cpu_baseline_torch"] = cpu_baseline_torch()
        except Exception as e:  # the torch restatement is an extra, never a reason to lose the bench line
            res["cpu_baseline_torch"] = {"error": repr(e)}
    elif rank == 0:
        res["cpu_baseline"] = None
    if world > 1 or forced:
        torch.distributed.destroy_process_group()
    if rank == 0:
        # the JSON line is the LAST thing on stdout: RCCL prints its version banner through C stdio, which — stdout being a pipe — is
        # flushed at exit, i.e. behind anything Python printed earlier (seen with one RCCL rank: five banner lines after the JSON line)
        try:
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
