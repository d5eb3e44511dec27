#!/usr/bin/env python3
"""The multi-chunk tile lists of the three bench clouds at 1 M Gaussians, six 256^2 faces, counted from tile_start after a forward
call: tiles beyond 2 048 keys, their 4 096-key chunks, the chunk count of every multi-chunk list, the (pass, chunk) merge units
and the tickets k_sort_stage1 hands out for them, and the sort's error word.  Usage: count_long_lists.py [--out FILE]
(profiles/r07_long_list_counts.json = count_long_lists.py --out profiles/r07_long_list_counts.json)."""
import json
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch
from splatter360_amd import decoder, rasterizer, synthetic

SORT_SHORT, SORT_CHUNK = 2048, 4096
dev = torch.device("cuda:0")
ext, K, near, far = decoder.cube_cameras(torch.tensor(synthetic.target_pano_pose((0.0, 0.0, 0.0)), device=dev), 0.1, 10.0)
bg = torch.zeros(3, device=dev)
res = {}
for name, make in (("encoder_like", lambda: synthetic.encoder_like_cloud(512, 1024, n_context=2, d_sh=25, seed=0)),
                   ("uniform", lambda: synthetic.uniform_cloud(1 << 20, seed=0, extent=5.0)),
                   ("surface_like", lambda: synthetic.surface_like_cloud(512, 1024, n_context=2, seed=0))):
    c = make()
    ps = [torch.tensor(c[k], device=dev) for k in ("means", "covariances", "harmonics", "opacities")]
    for _ in range(2):   # the second call has the first one's capacity hint: no overflow
        with torch.no_grad():
            decoder.render_views_fused(ext, K, near, far, (256, 256), bg, *ps, shared_campos=True,
                                       views=decoder.pack_camera_views(ext, K, near, far, bg))
    st = rasterizer.last_state()
    assert not st.overflowed()
    n = np.diff(st.tensors()["tile_start"].cpu().numpy().astype(np.int64))
    nch = np.where(n > SORT_SHORT, (n + SORT_CHUNK - 1) // SORT_CHUNK, 0)
    passes = np.array([0 if x <= 1 else int(x - 1).bit_length() for x in nch])
    res[name] = dict(gaussians=int(c["means"].shape[0]), tiles=int(n.size), longest=int(n.max()), chunked_tiles=int((nch > 0).sum()),
                     chunks=int(nch.sum()), multi_chunk_tiles=int((nch > 1).sum()),
                     chunk_counts_of_multi_chunk_tiles=sorted((int(x) for x in nch[nch > 1]), reverse=True),
                     merge_units=int((nch * passes).sum()), tickets=int(passes.max() * nch.sum()),
                     sort_errors=st.sort_errors(), split_errors=st.split_errors())
    del ps
text = json.dumps(res, indent=1)
print(text)
if "--out" in sys.argv:
    Path(sys.argv[sys.argv.index("--out") + 1]).write_text(text + "\n")
