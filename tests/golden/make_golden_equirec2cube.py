"""Records tests/golden/equirec2cube.npz from the reference's own Equirec2Cube (src/geometry/util.py, numpy + scipy), on CPU.
util.py imports cv2 at module level but run() uses it only to resize; a stub module stands in for it here, at generation time
only.  Run on a machine that has the reference checkout and scipy:

    python tests/golden/make_golden_equirec2cube.py /path/to/splatter360

Recorded (arrays only), for each (equ_h, equ_w, face_w) of SHAPES under the prefix e2c_<equ_h>_<equ_w>_<face_w>_:
  coor_y, coor_x   float32 [fw, 6 fw]     Equirec2Cube.coor_y / coor_x
  cosmaps          float32 [fw, 6 fw]     Equirec2Cube.cosmaps
  img              float32 [H, W, 3]      multiples of 1 / 4096 in [-2, 2)
  img_out          float32 [fw, 6 fw, 3]  run(img): what the reference returns for a float32 image
  img_out64        float64 [fw, 6 fw, 3]  run(img.astype(float64)): the same before the rounding
  u8, u8_out       uint8 [H, W, 3], [fw, 6 fw, 3]    run(u8)
  dist, dep_out    float32 [H, W, 1], [fw, 6 fw, 1]  run(img, dist)[1]: nearest sampling times cosmaps
The odd face widths (5, 7) are the smallest shapes at which scipy's wrap and the pole rows are reached at all.
"""
import importlib.util
import sys
import types
from pathlib import Path

import numpy as np

SHAPES = ((8, 16, 4), (12, 24, 5), (10, 28, 7), (16, 32, 8), (32, 64, 16))
OUT = Path(__file__).resolve().parent / "equirec2cube.npz"


def main(ref_root: str) -> None:
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    spec = importlib.util.spec_from_file_location("ref_geometry_util", Path(ref_root) / "src" / "geometry" / "util.py")
    util = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(util)
    rng = np.random.default_rng(360)
    out = {"shapes": np.array(SHAPES, np.int32)}
    for h, w, fw in SHAPES:
        e2c = util.Equirec2Cube(h, w, fw)
        img = (rng.integers(-8192, 8192, (h, w, 3)) / 4096).astype(np.float32)
        u8 = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        dist = (rng.integers(256, 40960, (h, w, 1)) / 4096).astype(np.float32)
        p = f"e2c_{h}_{w}_{fw}_"
        out[p + "coor_y"], out[p + "coor_x"], out[p + "cosmaps"] = e2c.coor_y[..., 0], e2c.coor_x[..., 0], e2c.cosmaps[..., 0]
        out[p + "img"], out[p + "u8"], out[p + "dist"] = img, u8, dist
        out[p + "img_out"], out[p + "dep_out"] = e2c.run(img, dist)
        out[p + "img_out64"] = e2c.run(img.astype(np.float64))
        out[p + "u8_out"] = e2c.run(u8)
        assert out[p + "coor_y"].dtype == np.float32 and out[p + "cosmaps"].dtype == np.float32 and out[p + "img_out"].dtype == np.float32
        assert out[p + "img_out64"].dtype == np.float64 and out[p + "u8_out"].dtype == np.uint8 and out[p + "dep_out"].dtype == np.float32
    np.savez_compressed(OUT, **out)
    print(OUT, OUT.stat().st_size, "bytes")
    assert OUT.stat().st_size < 200 * 1024


if __name__ == "__main__":
    main(sys.argv[1])
