"""Duration of the tile sort's launch (k_sort_stage1, profile slot `sort_tiles`: HIP events around the launch) for one build of the
library — how the S360_SORT_BMAX crossover table and the chunk-role comparison of DESIGN.md section 4 were measured.

usage: sort_bucket_timing.py tiles    [--lib PATH] [--steps K]   256 tiles of 2 048 keys whose occupied buckets hold EXACTLY m keys each,
                                                                 m = 1 .. 127 (depth words laid out on the bucket grid of the kernel)
       sort_bucket_timing.py headline [--lib PATH] [--steps K]   the bench's clouds (1 M Gaussians, six 256^2 faces), forward of a training step

--lib: a variant built with  _lib.build(out=PATH, extra=["-DS360_SORT_BMAX=127"])  (bucket path whatever the occupancy; =0: always the
merge-sort branch, i.e. what a list pays that is sent there; "-DS360_SORT_BUCKET_CHUNKS=1": 4 096-key chunks through the bucket sort).
Prints one JSON line per configuration."""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch

from splatter360_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("what", choices=("tiles", "headline"))
ap.add_argument("--lib", default=None)
ap.add_argument("--steps", type=int, default=50)
a = ap.parse_args()
if a.lib:
    _lib.LIB_PATH = Path(a.lib).resolve()
from splatter360_amd import cameras, decoder, rasterizer, synthetic  # noqa: E402

dev = torch.device("cuda:0")
label = Path(a.lib).parent.name if a.lib else "in-tree"


def timed(step):
    for _ in range(5):
        step()
    torch.cuda.synchronize()
    _lib.profile_enable(True)
    _lib.profile_collect()
    for _ in range(a.steps):
        step()
    torch.cuda.synchronize()
    ms, calls = _lib.profile_collect()["sort_tiles"]
    _lib.profile_enable(False)
    return round(ms / calls * 1e3, 2)


def tile_depth_words(m, rng, nb=2048, n=2048):
    """n depth words in [4.0, 8.0): 2^23 bit patterns = nb buckets of 4 096 patterns (min and max pinned, so the kernel's scale is
    exactly nb / 2^23); every m-th bucket holds m keys, the others none."""
    lo = int(np.float32(4.0).view(np.uint32))
    words = []
    for j in range(0, nb, m):
        off = rng.choice(4094, min(m, n - len(words)), replace=False) + 1
        words += [lo + j * 4096 + int(o) for o in off]
    words = np.asarray(words[:n], np.int64)
    words[0], words[-1] = lo, lo + (1 << 23) - 1
    b = (words - lo) >> 12
    assert np.unique(words).size == n and np.bincount(b).max() == m
    return words.astype(np.uint32)


if a.what == "tiles":
    hw, gx, n = 256, 16, 2048
    proj = cameras.get_projection_matrix(torch.tensor([1.0]), torch.tensor([100.0]), torch.tensor([np.pi / 2]), torch.tensor([np.pi / 2]))[0]
    views = rasterizer.pack_views(torch.eye(4)[None].to(dev), proj.T.contiguous()[None].float().to(dev), torch.zeros(3, device=dev), 1.0, 1.0,
                                  torch.zeros(3, device=dev))
    for m in (1, 2, 4, 8, 16, 32, 64, 127):
        rng = np.random.default_rng(m)
        tile = np.repeat(np.arange(gx * gx), n)
        z = np.concatenate([rng.permutation(tile_depth_words(m, rng)) for _ in range(gx * gx)]).view(np.float32).astype(np.float64)
        px = (tile % gx) * 16 + 8 + rng.uniform(-2.0, 2.0, tile.size)
        py = (tile // gx) * 16 + 8 + rng.uniform(-2.0, 2.0, tile.size)
        means = np.stack([((2 * px + 1) / hw - 1) * z, ((2 * py + 1) / hw - 1) * z, z], 1)
        s = 0.25 / hw
        cov6 = np.tile(np.array([[s * s, 0, 0, s * s, 0, s * s]]), (tile.size, 1)) * (z[:, None] ** 2)
        perm = rng.permutation(tile.size)
        t = lambda x: torch.tensor(np.asarray(x, np.float32), device=dev)
        args = (t(means[perm]), t(cov6[perm]), t(np.full((tile.size, 1), 0.01)), None, t(rng.uniform(0, 1, (tile.size, 3))))

        def step():
            rasterizer.rasterize_views(*args, views=views, image_height=hw, image_width=hw, sh_degree=0, shared_campos=True)

        us = timed(step)
        st = rasterizer.last_state()
        ts = st.tensors()
        assert (ts["tile_start"].cpu().numpy()[1:gx * gx + 1] - ts["tile_start"].cpu().numpy()[:gx * gx] == n).all() and st.sort_errors() == 0
        k = ts["keys"][:gx * gx * n].view(gx * gx, n)
        assert bool((k[:, 1:] > k[:, :-1]).all())
        print(json.dumps({"lib": label, "what": "256 tiles x 2048 keys", "keys_per_occupied_bucket": m, "sort_tiles_us": us}), flush=True)
else:
    clouds = {"encoder_like": lambda: synthetic.encoder_like_cloud(512, 1024), "surface_like": lambda: synthetic.surface_like_cloud(512, 1024),
              "uniform": lambda: synthetic.uniform_cloud(1 << 20, seed=0, extent=5.0)}
    ext, K, near, far = decoder.cube_cameras(torch.eye(4, device=dev), 0.1, 10.0)
    for name, make in clouds.items():
        cloud = make()
        g = [torch.tensor(cloud[k], device=dev).requires_grad_(True) for k in ("means", "covariances", "harmonics", "opacities")]

        def step():
            decoder.render_views_fused(ext, K, near, far, (256, 256), torch.zeros(3, device=dev), *g, shared_campos=True)

        us = timed(step)
        st = rasterizer.last_state()
        n = np.diff(st.tensors()["tile_start"].cpu().numpy().astype(np.int64))
        assert st.sort_errors() == 0
        print(json.dumps({"lib": label, "what": name, "sort_tiles_us": us, "keys": int(n.sum()), "lists_over_2048": int((n > 2048).sum()),
                          "lists_over_4096": int((n > 4096).sum())}), flush=True)
