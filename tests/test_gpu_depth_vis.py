"""splatter360_amd.visualize on the GPU against the numpy statement of tests/depth_vis_reference.py, on the maps of
tests/golden/depth_vis.npz (recorded from the reference by tests/golden/make_golden_depth_vis.py; tests/test_depth_vis_spec.py
holds the statement to that recording on CPU).

Equality is exact: the quantiles are an exact selection and every later step is one float64 expression rounded once, evaluated
the same way by the statement; the only library function is the float64 log, and the spec test asserts that no fixture
logarithm lies close enough to a float32 rounding midpoint for a last-bit difference to show.  No tolerance, no excluded pixel."""
from pathlib import Path

import numpy as np
import pytest
import torch

import depth_vis_reference as R

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden" / "depth_vis.npz"


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def statement(golden):
    """Per fixture map: (range [4], index map, float picture [3, h, w], byte picture [h, w, 3]) of the statement, computed once."""
    f32, prep, _ = R.tables("turbo")
    out = {}
    for n in (str(n) for n in golden["names"]):
        idx = R.depth_index(golden[f"map_{n}"])
        out[n] = (R.depth_range(golden[f"map_{n}"]), idx, np.moveaxis(f32[idx], -1, 0), prep[idx])
    return out


def _same_floats(a: np.ndarray, b: np.ndarray) -> bool:
    """Bit-equal, any NaN counting as equal to any NaN."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and a[~np.isnan(a)].tobytes() == b[~np.isnan(b)].tobytes()


def test_depth_range_and_pictures_equal_the_statement_on_every_map(gpu, golden, statement):
    from splatter360_amd import visualize
    for n, (rng, idx, rgb, u8) in statement.items():
        d = torch.from_numpy(golden[f"map_{n}"]).to(gpu)
        got = visualize.depth_range(d).cpu().numpy()
        assert got.shape == (4,) and _same_floats(got, rng), (n, got, rng)
        pf, pb = visualize.depth_map(d), visualize.depth_map(d, out="uint8")
        assert pf.dtype == torch.float32 and pf.shape == (3, *d.shape) and pb.dtype == torch.uint8 and pb.shape == (*d.shape, 3)
        assert np.array_equal(pb.cpu().numpy(), u8), (n, int((pb.cpu().numpy() != u8).any(-1).sum()))
        assert pf.cpu().numpy().tobytes() == rgb.tobytes(), n
        assert torch.equal(visualize.depth_map(d), pf) and torch.equal(visualize.depth_map(d, out="uint8"), pb)      # call to call
        assert d.cpu().numpy().tobytes() == golden[f"map_{n}"].tobytes()                                           # input untouched


def test_a_map_shared_by_workgroups_with_ties_across_digit_boundaries(gpu):
    """40 000 elements (three workgroups share the map, the last one partly filled) drawn from 300 values whose keys differ in
    the top, the middle and the low digit alike, so the ranks sit among duplicates that straddle digit boundaries."""
    from splatter360_amd import visualize
    rng = np.random.default_rng(5)
    base = np.float32(1.5).view(np.uint32)
    values = (base + np.concatenate([np.arange(-50, 50), (np.arange(100) - 50) * 1024 + 1023, (np.arange(100) - 50) * (1 << 21)])
              ).astype(np.uint32).view(np.float32)
    d = values[rng.integers(0, values.size, (160, 250))]
    d[rng.uniform(size=d.shape) < 0.1] = 0.0
    got = visualize.depth_range(torch.from_numpy(d).to(gpu)).cpu().numpy()
    assert _same_floats(got, R.depth_range(d)), (got, R.depth_range(d))
    t = torch.from_numpy(d)
    assert got[0] == t[t > 0].quantile(0.01).item() and got[1] == t.view(-1).quantile(0.99).item()
    assert np.array_equal(visualize.depth_map(torch.from_numpy(d).to(gpu), out="uint8").cpu().numpy(), R.depth_map(d, out="uint8"))


def _mixed_batch(golden):
    names = ("16x16", "ties", "nan", "special", "16x16", "ties", "special")
    maps = np.stack([golden[f"map_{n}"] for n in names])
    maps[4] = maps[4][::-1].copy()
    maps[5] = -maps[5]                                           # no positive element: the min / max branch
    maps[6] = maps[6].T.copy()
    return maps


def test_batch_of_seven_equals_seven_single_calls(gpu, golden):
    from splatter360_amd import visualize
    maps = torch.from_numpy(_mixed_batch(golden)).to(gpu)
    bf, bb, br = visualize.depth_map(maps), visualize.depth_map(maps, out="uint8"), visualize.depth_range(maps)
    assert bf.shape == (7, 3, 16, 16) and bb.shape == (7, 16, 16, 3) and br.shape == (7, 4)
    for i in range(7):
        assert torch.equal(bf[i], visualize.depth_map(maps[i])), i
        assert torch.equal(bb[i], visualize.depth_map(maps[i], out="uint8")), i
        assert _same_floats(br[i].cpu().numpy(), visualize.depth_range(maps[i]).cpu().numpy()), i
        assert np.array_equal(bb[i].cpu().numpy(), R.depth_map(maps[i].cpu().numpy(), out="uint8")), i
    two = maps.view(7, 1, 16, 16).expand(7, 2, 16, 16)           # two leading dims, not collapsible: copied, same pictures
    assert torch.equal(visualize.depth_map(two, out="uint8")[:, 1], bb)


def test_strided_view_is_read_in_place(gpu, golden):
    from splatter360_amd import visualize
    maps = torch.from_numpy(_mixed_batch(golden)).to(gpu)
    faces = torch.rand(7, 6, 16, 16, device=gpu, generator=torch.Generator(device=gpu).manual_seed(1)) + 0.5
    faces[:, 2] = maps
    keep = faces.clone()
    view = faces[:, 2]
    assert not view.is_contiguous()
    assert torch.equal(visualize.depth_map(view, out="uint8"), visualize.depth_map(maps, out="uint8"))
    assert torch.equal(visualize.depth_map(view), visualize.depth_map(maps))
    assert faces.cpu().numpy().tobytes() == keep.cpu().numpy().tobytes()


def _torch_prep(image):
    """The reference's prep_image lines in torch on the device (image_io.py:38-54), without the final copy to the host."""
    if image.ndim == 4:
        b, c, h, w = image.shape
        image = image.permute(1, 2, 0, 3).reshape(c, h, b * w)
    if image.ndim == 2:
        image = image[None]
    if image.shape[0] == 1:
        image = image.expand(3, -1, -1)
    return (image.detach().clip(min=0, max=1) * 255).type(torch.uint8).permute(1, 2, 0).contiguous()


@pytest.mark.parametrize("shape", [(3, 11, 13), (11, 13), (1, 11, 13), (4, 3, 9, 7), (4, 11, 13), (2, 4, 5, 3), (3, 1, 8, 6), (3, 64, 96)])
def test_prep_image_equals_the_torch_lines(gpu, golden, shape):
    from splatter360_amd import visualize
    x = torch.rand(shape, device=gpu, generator=torch.Generator(device=gpu).manual_seed(sum(shape))) * 1.4 - 0.2
    x.view(-1)[:3] = torch.tensor([0.0, 1.0, 0.5], device=gpu)
    got = visualize.prep_image(x)
    want = _torch_prep(x)
    assert got.dtype == torch.uint8 and got.shape == want.shape and torch.equal(got, want)
    assert np.array_equal(got.cpu().numpy(), R.prep_image(x.cpu().numpy()))
    nan = x.clone()
    nan.view(-1)[5] = float("nan")
    assert np.array_equal(visualize.prep_image(nan).cpu().numpy(), R.prep_image(nan.cpu().numpy()))       # NaN -> 0
    key = {(3, 11, 13): "chw", (11, 13): "hw", (1, 11, 13): "1hw", (4, 3, 9, 7): "bchw", (4, 11, 13): "4hw"}.get(shape)
    if key:                                                      # the reference's own recording
        rec = visualize.prep_image(torch.from_numpy(golden[f"prep_{key}_in"]).to(gpu)).cpu().numpy()
        assert np.array_equal(rec, golden[f"prep_{key}_out"])


@pytest.mark.parametrize("color_map", R.MAPS)
def test_colorize_gives_both_layouts(gpu, golden, color_map):
    from splatter360_amd import visualize
    x = golden["cmap_x"]
    xd = torch.from_numpy(x).to(gpu)
    last = visualize.colorize(xd, color_map)
    assert last.shape == (19, 23, 3) and np.array_equal(last.cpu().numpy(), golden[f"cmap_{color_map}"])       # the reference's
    first = visualize.colorize(xd, color_map, channels="first")
    assert first.shape == (3, 19, 23) and torch.equal(first, last.permute(2, 0, 1))
    for channels in ("last", "first"):
        got = visualize.colorize(xd, color_map, channels=channels, out="uint8")
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), R.colorize(x, color_map, channels, "uint8"))
    batch = torch.stack([xd, xd.flip(0), xd * 0.5])
    assert torch.equal(visualize.colorize(batch, color_map, channels="first")[1], visualize.colorize(xd.flip(0), color_map, channels="first"))
    flat = visualize.colorize(xd.reshape(-1)[:5], color_map, out="uint8")                 # a tail shorter than one store
    assert flat.shape == (5, 3) and torch.equal(flat, visualize.colorize(xd, color_map, out="uint8").view(-1, 3)[:5])


def test_error_map_equals_the_statement(gpu, golden):
    from splatter360_amd import visualize
    a, b = golden["err_a"], golden["err_b"]
    got = visualize.error_map(torch.from_numpy(a).to(gpu), torch.from_numpy(b).to(gpu))
    assert got.dtype == torch.uint8 and got.shape == (21, 17, 3)
    assert np.array_equal(got.cpu().numpy(), R.error_map(a, b))
    assert torch.equal(got, visualize.error_map(torch.from_numpy(b).to(gpu), torch.from_numpy(a).to(gpu)))
    nan = a.copy()
    nan[1, 3, 4] = np.nan
    assert np.array_equal(visualize.error_map(torch.from_numpy(nan).to(gpu), torch.from_numpy(b).to(gpu)).cpu().numpy(), R.error_map(nan, b))


def test_errors(gpu):
    from splatter360_amd import visualize
    x = torch.rand(4, 5)
    for call in (lambda: visualize.depth_map(x), lambda: visualize.depth_range(x), lambda: visualize.colorize(x),
                 lambda: visualize.prep_image(x), lambda: visualize.error_map(torch.rand(3, 4, 5), torch.rand(3, 4, 5))):
        with pytest.raises(RuntimeError):
            call()
    g = x.to(gpu)
    for call in (lambda: visualize.depth_map(g, out="bytes"), lambda: visualize.depth_map(g[0]), lambda: visualize.depth_map(g.double()),
                 lambda: visualize.colorize(g, "magma"), lambda: visualize.colorize(g, channels="middle"),
                 lambda: visualize.prep_image(torch.rand(2, 4, 5, device=gpu)), lambda: visualize.prep_image(g[0]),
                 lambda: visualize.error_map(g, g), lambda: visualize.error_map(torch.rand(3, 4, 5, device=gpu), torch.rand(3, 4, 6, device=gpu))):
        with pytest.raises(ValueError):
            call()
    import splatter360_amd
    assert splatter360_amd.visualize is visualize


def test_seam_wrappers_run_the_kernels_on_a_standin_module(gpu, golden):
    """The three wrappers of install(visualization=True) around stand-in functions that must not run for GPU float32 tensors."""
    from splatter360_amd import plugin, visualize

    def never(*a, **k):
        raise AssertionError("the replaced function ran")

    import types
    mod = types.ModuleType("standin_reference_module")          # not in sys.modules: the seams patch the object they are given
    mod.depth_map = mod.prep_image = mod.apply_color_map = never
    patched = {}
    for seam in plugin.VIS_SEAMS:
        patched.update(seam.patch(mod))
    assert all(getattr(mod, k) is f and f.replaced is never for k, f in patched.items()) and len(patched) == 3

    d = torch.from_numpy(np.stack([golden["map_16x16"], golden["map_ties"], golden["map_special"]])).to(gpu)
    depth_map = mod.depth_map
    got = depth_map(d)                                           # the reference normalises over the WHOLE argument
    whole = np.moveaxis(R.tables("turbo")[0][R.depth_index(d.cpu().numpy())], -1, -3)
    assert got.shape == (3, 3, 16, 16) and got.cpu().numpy().tobytes() == np.ascontiguousarray(whole).tobytes()
    assert depth_map(d[0]).cpu().numpy().tobytes() == R.depth_map(golden["map_16x16"]).tobytes()
    assert plugin._native_depth_map(lambda r: "replaced")(d.double()) == "replaced"

    prep = mod.prep_image
    frame = prep(got[0])
    assert isinstance(frame, np.ndarray) and frame.dtype == np.uint8 and np.array_equal(frame, R.prep_image(got[0].cpu().numpy()))
    assert np.array_equal(prep(got), R.prep_image(got.cpu().numpy())) and prep(got).shape == (16, 48, 3)
    assert plugin._native_prep_image(lambda i: "replaced")(torch.rand(2, 4, 4, device=gpu)) == "replaced"        # two channels

    acm = mod.apply_color_map
    x = torch.from_numpy(golden["cmap_x"]).to(gpu)
    assert np.array_equal(acm(x).cpu().numpy(), golden["cmap_inferno"]) and np.array_equal(acm(x, "turbo").cpu().numpy(), golden["cmap_turbo"])
    assert plugin._native_apply_color_map(lambda x, m: "replaced " + m)(x, "magma") == "replaced magma"
    assert visualize.depth_map_whole(d).shape == (3, 3, 16, 16)


def test_stitched_distance_panorama_to_bytes(gpu):
    """The composition the evaluation step runs per scene: stitch_distance_rendered -> depth_map(out="uint8"), against the
    statement applied to the stitched tensor."""
    from splatter360_amd import stitch, visualize
    v, fw, eh, ew = 2, 8, 16, 32
    g = torch.Generator(device=gpu).manual_seed(3)
    depth = torch.rand(v, 6, fw, fw, device=gpu, generator=g) * 9.5 + 0.5
    k4 = torch.tensor([fw * 0.5] * 4, device=gpu).expand(v, 6, 4).contiguous()
    erp = stitch.Cube2Equirec(fw, eh, ew).to(gpu).stitch_distance_rendered(depth, k4)
    assert erp.shape == (v, eh, ew)
    got = visualize.depth_map(erp, out="uint8")
    host = erp.cpu().numpy()
    assert got.shape == (v, eh, ew, 3)
    for i in range(v):
        assert np.array_equal(got[i].cpu().numpy(), R.depth_map(host[i], out="uint8")), i
