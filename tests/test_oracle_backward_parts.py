"""The oracle's backward in its two parts, its term magnitudes and its decision margins (oracle/s360_oracle.c, both precisions),
and the conditions tests/test_gpu_backward_float64.py rests on — all on the CPU:

  * backward_gaussians (orc_backward's second loop alone) on the oracle's own raster gradients is backward() bit for bit, and is
    linear in them;
  * every raster_* is bounded by its raster_*_abs (sum |term|), which does not see the sign of the seed;
  * decision_margin and raster_depth_value against a numpy restatement of the pixel loop;
  * THE MASK: on every scene of the GPU test, the float32 oracle takes the float64 oracle's decisions (n_contrib) on every pixel
    whose float64 margin is at least backward_reference.MARGIN, and at most 10 % of the pixels are flagged;
  * THE YARDSTICK: with the seed zeroed on the flagged pixels the float32 oracle's per-pair ratio stays finite and below 2^10;
  * THE EXCLUSIONS of the chain test: the Gaussians whose visibility or clamp flags differ between float32 and float64, or whose
    tangent lies within 1e-5 of the 1.3 tan(fov) limit, are at most 1e-3 of each case's cloud (the float32 oracle stands in for
    the kernels: the parity tests show its radii and clamp flags are theirs bit for bit), and every role of the cloud occurs."""
import numpy as np
import pytest

import backward_reference as br
from oracle import oracle

SCENE_NAMES = tuple(br.SCENES)
OUT_KEYS = ("means3D", "means2D", "cov3D", "opacities", "shs", "colors_precomp")
RASTER = ("raster_xy_pix", "raster_conic", "raster_opacity", "raster_rgb")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", ["small", "split"])        # SH colours (the view-direction term) | colors_precomp
def test_backward_gaussians_is_the_second_loop_bit_for_bit_and_linear(name, dtype):
    sc = br.scene(name)
    o = sc["orc32" if dtype == np.float32 else "orc64"]
    b = sc["b32" if dtype == np.float32 else "b64"]
    raster = [b[k] for k in RASTER]
    g = o.backward_gaussians(*raster)
    g2 = o.backward_gaussians(*[2 * r for r in raster])
    nonzero = 0
    for k in OUT_KEYS:
        if b[k] is None:
            assert g[k] is None
            continue
        np.testing.assert_array_equal(_bits(g[k]), _bits(b[k]), err_msg=k)
        np.testing.assert_array_equal(_bits(g2[k]), _bits(2 * g[k]), err_msg=k)       # a power of two commutes with every rounding
        nonzero += int(np.count_nonzero(g[k]))
    assert nonzero > 0
    # backward() itself still works after the records were replaced, and a depth seed changes nothing but its own record
    b_again = o.backward(sc["seed"], dL_ddepth=np.ones((sc["h"], sc["w"])))
    for k in OUT_KEYS + RASTER:
        if b[k] is not None:
            np.testing.assert_array_equal(_bits(b_again[k]), _bits(b[k]), err_msg=k)
    assert np.abs(b_again["raster_depth_value"]).max() > 0 and np.abs(b["raster_depth_value"]).max() == 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_term_magnitudes_bound_the_sums_and_ignore_the_seed_sign(dtype):
    sc = br.scene("small")
    o = sc["orc32" if dtype == np.float32 else "orc64"]
    seed = sc["seed_raw"]
    gz = np.random.default_rng(5).standard_normal((sc["h"], sc["w"])).astype(np.float32)
    b = o.backward(seed, dL_ddepth=gz)
    flip = np.where(np.random.default_rng(6).random((sc["h"], sc["w"])) < 0.5, -1.0, 1.0).astype(np.float32)
    bf = o.backward(seed * flip[None], dL_ddepth=gz * flip)
    changed = 0
    for k in RASTER + ("raster_depth_value",):
        assert (np.abs(b[k]) <= b[k + "_abs"]).all(), k
        assert (b[k + "_abs"] >= 0).all() and b[k + "_abs"].max() > 0
        np.testing.assert_array_equal(_bits(b[k + "_abs"]), _bits(bf[k + "_abs"]), err_msg=k)
        changed += int((b[k] != bf[k]).sum())
    assert changed > 0                                     # the flip did change the sums themselves


def _restated_pixel_loop(f, h, w, gz):
    """render_forward's decisions in float64 numpy from the oracle's own 2D records and lists: (margin[H,W], depth record[P])."""
    xy, co = f["xy"].astype(np.float64), f["conic_opacity"].astype(np.float64)
    gx = (w + 15) // 16
    margin = np.full((h, w), np.inf)
    g_z = np.zeros(xy.shape[0])
    for py in range(h):
        for px in range(w):
            s, e = f["ranges"][(py // 16) * gx + px // 16]
            T = 1.0
            for j in range(int(s), int(e)):
                i = int(f["values"][j])
                dx, dy = xy[i, 0] - px, xy[i, 1] - py
                power = -0.5 * (co[i, 0] * dx * dx + co[i, 2] * dy * dy) - co[i, 1] * dx * dy
                margin[py, px] = min(margin[py, px], abs(power))
                if power > 0:
                    continue
                alpha = min(0.99, co[i, 3] * np.exp(power))
                margin[py, px] = min(margin[py, px], abs(255 * alpha - 1))
                if alpha < 1.0 / 255.0:
                    continue
                test_T = T * (1 - alpha)
                margin[py, px] = min(margin[py, px], abs(test_T / 1e-4 - 1) / 100)
                if test_T < 1e-4:
                    break
                g_z[i] += alpha * T * gz[py, px]
                T = test_T
    return margin, g_z


def test_decision_margin_and_depth_record_against_a_numpy_restatement():
    """A 32 x 64 scene (the loop above is plain Python) crowded into its two middle tile columns: pixels that stop, and outer tiles
    whose pixels evaluate nothing."""
    from helpers import small_front_scene
    h, w = 32, 64
    S, means, cov6, shs, opac = small_front_scene(n=80, seed=2, h=h, w=w, spread=0.12, srange=(0.05, 0.2))
    opac = np.minimum(1.0, opac * 1.3)
    o = oracle.rasterize(S, means3D=means, cov3D_precomp=cov6, opacities=opac, shs=shs, dtype=np.float64)
    f = o.forward()
    gz = np.random.default_rng(0).standard_normal((h, w))
    b = o.backward(np.zeros((3, h, w)), dL_ddepth=gz)
    margin, g_z = _restated_pixel_loop(f, h, w, gz)
    assert np.isinf(margin).any() and np.isfinite(margin).any()                       # pixels that evaluate nothing, and the others
    lengths = np.diff(f["ranges"].astype(np.int64), axis=1).reshape(h // 16, w // 16)
    stopped = f["n_contrib"] < lengths[np.arange(h)[:, None] // 16, np.arange(w)[None] // 16]
    assert (f["final_T"][stopped] < 2e-4).any()                                       # the stop test did fire somewhere
    np.testing.assert_array_equal(np.isinf(margin), np.isinf(f["decision_margin"]))
    fin = np.isfinite(margin)
    np.testing.assert_allclose(f["decision_margin"][fin], margin[fin], rtol=1e-9, atol=1e-13)
    np.testing.assert_allclose(b["raster_depth_value"], g_z, rtol=0, atol=1e-12 * max(1.0, b["raster_depth_value_abs"].max()))
    assert (f["decision_margin"] >= 0).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_depth_channel_is_a_fourth_colour_channel(dtype):
    """A depth seed with per-pair values must move dL/dalpha exactly as a colour channel with those values and that seed does (zero
    background): same centre / conic / opacity records bit for bit, and the depth record is that channel's colour record."""
    sc = br.scene("split")                                  # colors_precomp
    o = sc["orc32" if dtype == np.float32 else "orc64"]
    h, w = sc["h"], sc["w"]
    rng = np.random.default_rng(9)
    zval = rng.uniform(0.1, 2.0, sc["means"].shape[0]).astype(np.float32)
    dz = rng.standard_normal((h, w)).astype(np.float32)
    col = sc["colors"].copy()
    col[:, 0] = zval
    S0 = dict(sc["So"], bg=np.zeros(3, np.float32))
    as_colour = oracle.rasterize(S0, means3D=sc["means"], cov3D_precomp=sc["cov6"], opacities=sc["opac"], colors_precomp=col, dtype=dtype)
    as_depth = oracle.rasterize(S0, means3D=sc["means"], cov3D_precomp=sc["cov6"], opacities=sc["opac"], colors_precomp=sc["colors"], dtype=dtype)
    as_colour.forward(), as_depth.forward()
    seed = np.zeros((3, h, w), np.float32)
    seed[0] = dz
    bc = as_colour.backward(seed)
    bd = as_depth.backward(np.zeros((3, h, w), np.float32), dL_ddepth=dz, depth_values=zval)
    for k in ("raster_xy_pix", "raster_conic", "raster_opacity"):
        assert np.abs(bc[k]).max() > 0
        np.testing.assert_array_equal(bd[k], bc[k], err_msg=k)
        np.testing.assert_array_equal(bd[k + "_abs"], bc[k + "_abs"], err_msg=k)
    np.testing.assert_array_equal(bd["raster_depth_value"], bc["raster_rgb"][:, 0])
    only_record = as_depth.backward(np.zeros((3, h, w), np.float32), dL_ddepth=dz)       # without values: the record alone
    np.testing.assert_array_equal(only_record["raster_depth_value"], bd["raster_depth_value"])
    assert np.abs(only_record["raster_xy_pix"]).max() == 0


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_the_mask_keeps_float32_on_the_float64_decisions(name):
    sc = br.scene(name)
    flagged = sc["flagged"]
    share = float(flagged.mean())
    differ = sc["f32"]["n_contrib"] != sc["f64"]["n_contrib"]
    print(f"[mask] {name}: flagged {share:.4f} of {flagged.size} pixels; n_contrib differs on {int(differ.sum())} pixels, "
          f"{int((differ & ~flagged).sum())} of them unflagged")
    assert not (differ & ~flagged).any()
    assert share <= 0.10
    assert np.array_equal(sc["f32"]["radii"] > 0, sc["f64"]["radii"] > 0)             # the pairs the measure runs over are the same
    assert (sc["seed"][:, flagged] == 0).all() and (sc["seed"][:, ~flagged] != 0).any()


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_the_float32_oracle_is_a_usable_yardstick(name):
    sc = br.scene(name)
    r32, _ = br.oracle_records(sc["b32"])
    r64, a64 = br.oracle_records(sc["b64"])
    vis = sc["f64"]["radii"] > 0
    stats = br.group_stats(br.pair_ratios(r32, r64, a64, vis))
    print(f"[pairgrad64-yardstick] {name}: " + "  ".join(f"{g} worst {w:.1f} mean {m:.2f}" for g, (w, m) in stats.items()) + "  (units of 2^-24)")
    assert vis.sum() > 0
    for g, (worst, mean) in stats.items():
        assert np.isfinite(worst) and worst < 2.0 ** 10, (name, g, worst)
        assert mean > 0, (name, g)                                                    # ... and it is not trivially exact


def test_the_scenes_reach_their_mechanisms_on_the_oracle():
    """What can be said without a GPU: the wide scene's planted pairs own more than 32 tiles, the dense one has long lists and
    pixels that stop, the split one a list longer than SORT_SHORT."""
    from helpers import SORT_SHORT
    wide = br.scene("wide")
    assert wide["f64"]["tiles_touched"][wide["info"]["planted"]].min() > 32 and len(wide["info"]["planted"]) >= 8
    assert (wide["h"], wide["w"]) == (96, 128)
    dense = br.scene("dense")
    lengths = np.diff(dense["f64"]["ranges"].astype(np.int64), axis=1)[:, 0]
    assert lengths.max() > 256 and (dense["f64"]["final_T"] < 2e-4).any()
    small = br.scene("small")
    assert (small["h"], small["w"]) == (64, 80)                                       # 5 x 4 tiles
    split = br.scene("split")
    assert np.diff(split["f64"]["ranges"].astype(np.int64), axis=1).max() == SORT_SHORT + 1


CHAIN_SETUPS = [(p, 25, 4, "cube6", False) for p in br.CHAIN_P] + [(br.CHAIN_P[0], 25, 2, "cube6", False), (br.CHAIN_P[0], 16, 3, "cube6", False),
                                                                    (br.CHAIN_P[0], 25, 4, "two_centres", False), (br.CHAIN_P[1], 25, 4, "two_centres", False),
                                                                    (br.CHAIN_P[0], 25, 4, "cube6", True), (br.CHAIN_P[1], 25, 4, "cube6", True)]


@pytest.mark.parametrize("p,m,deg,kind,colors", CHAIN_SETUPS)
def test_the_chain_cases_leave_out_at_most_a_thousandth_and_reach_every_role(p, m, deg, kind, colors):
    s = br.chain_setup(p, m, deg, kind, colors)
    out = br.excluded(s["vo64"], s["vo32"].visible, s["vo32"].clamped)
    print(f"[chain64-excluded] P {p} M {m} degree {deg} {kind} colours {colors}: {int(out.sum())} of {p}")
    assert out.sum() <= 1e-3 * p
    if kind == "cube6":
        reached = br.roles_reached(s)
        print("   roles:", reached)
        for k, n in reached.items():
            assert n > 0 or (colors and k.startswith("clamped")), k
    else:
        assert s["vo64"].visible.all(0).any() or s["vo64"].visible.any()
        assert not np.array_equal(s["vo64"].S[0]["campos"], s["vo64"].S[1]["campos"])


def test_the_chain_reference_is_linear_and_its_condition_bounds_it():
    """ViewOracles.chain: the float64 reference of test B is the sum the kernels form (scale and scale^2 folds, depth column), its
    condition D bounds it element by element, and an element with D == 0 is exactly 0 (invisible Gaussians, SH beyond the degree)."""
    s = br.chain_setup(br.CHAIN_P[0], 25, 2, "cube6", False)
    vo = s["vo64"]
    R = np.random.default_rng(3).standard_normal((6, vo.P, 12)).astype(np.float32)
    want, D = vo.chain(R, depth_mode=1, want_abs=True)
    twice = vo.chain(2 * R, depth_mode=1)
    plain = vo.chain(R)
    for k in want:
        assert (np.abs(want[k]) <= D[k] * (1 + 1e-12)).all(), k
        assert (want[k][D[k] == 0] == 0).all(), k
        np.testing.assert_array_equal(twice[k], 2 * want[k])
    assert (D["sh"][:, 9:] == 0).all() and (D["sh"][:, :9].max(0) > 0).all()          # degree 2 of M = 25
    assert (D["means"][~vo.visible.any(0)] == 0).all() and (~vo.visible.any(0)).any()
    assert not np.array_equal(plain["means"], want["means"])                          # the depth column is there
    assert vo.S[0]["scale"] == pytest.approx(10.0)                                    # near = 0.1: the folds are not 1


# ------------------------------------------------------------------------------------- the raw-tail reference (tests/test_gpu_raw_float64.py)
def _tiny_raw_case(seed=0, v=2, h=2, w=3, n_groups=2):
    import torch
    from oracle import adapter_ref
    from splatter360_amd import synthetic
    rng = np.random.default_rng(seed)
    gv = h * w
    ext = np.tile(np.eye(4, dtype=np.float32), (v, 1, 1))
    ext[:, :3, :3] = synthetic._random_rotations(rng, v)
    ext[:, :3, 3] = rng.uniform(-1, 1, (v, 3))
    dep = np.exp(rng.uniform(np.log(0.5), np.log(8.0), (v, gv))).astype(np.float32)
    raw = rng.standard_normal((v, gv, 82)).astype(np.float32)
    rot = adapter_ref.wigner_blocks(ext[:, :3, :3], 25).astype(np.float32)
    views = br.cube_views(n_groups)
    rgb = rng.standard_normal((n_groups, v * gv, 4)).astype(np.float32)
    w_ = (np.arange(v * gv)[None, :] + np.arange(n_groups)[:, None]) % (n_groups + 1) - 1          # -1, 0, 1, ... : some groups see nothing
    rgb[..., 3] = w_.astype(np.int32).view(np.float32)
    t = torch.tensor
    return dict(ext=t(ext), dep=t(dep), raw=t(raw), rot=t(rot), views=views, d_cov6=rng.standard_normal((v * gv, 6)).astype(np.float32),
                d_rgb=rgb, d_means=rng.standard_normal((v * gv, 3)).astype(np.float32), hw=(h, w), v=v, gv=gv)


def test_the_raw_tail_reference_agrees_with_central_differences():
    """Float64 autograd of backward_reference.raw_tail_reference against central differences of the scalar it differentiates,
    <cov6, d_cov6> + <harmonics, g_harm> + <means, d_means>, at a tiny shape, with the SH rotation and differentiable means."""
    import torch
    from oracle import adapter_ref
    c = _tiny_raw_case()
    tt = torch.float64
    means32 = adapter_ref.adapter_tail_torch(c["ext"], c["dep"], c["dep"], c["raw"], c["hw"], 0.5, 15.0, sh_rotation=c["rot"]).means.reshape(-1, 3)
    ref = br.raw_tail_reference(tt, c["ext"], c["dep"], c["raw"], c["rot"], means32, c["views"], c["d_cov6"], c["d_rgb"], c["d_means"], c["hw"])
    g_harm = ref.g_harm
    r_, c_ = torch.triu_indices(3, 3)

    def scalar(dep, raw):
        o = adapter_ref.adapter_tail_torch(c["ext"].to(tt), dep, torch.zeros_like(dep), raw, c["hw"], 0.5, 15.0, sh_rotation=c["rot"].to(tt),
                                           differentiable_means=True)
        return float((o.covariances[:, :, r_, c_] * torch.tensor(c["d_cov6"]).to(tt).reshape(c["v"], c["gv"], 6)).sum() + (o.harmonics * g_harm).sum()
                     + (o.means * torch.tensor(c["d_means"]).to(tt).reshape(c["v"], c["gv"], 3)).sum())

    rng = np.random.default_rng(1)
    dep0, raw0 = c["dep"].to(tt), c["raw"].to(tt)
    eps = 1e-6
    noise = 8 * 2.0 ** -53 * abs(scalar(dep0, raw0)) / eps                  # the rounding of the two scalars in the difference quotient
    for which, grad, base in (("dep", ref.d_dep, dep0), ("raw", ref.d_raw, raw0)):
        idx = rng.choice(base.numel(), size=6 if which == "dep" else 40, replace=False)
        for i in idx:
            hi, lo = base.clone(), base.clone()
            hi.view(-1)[i] += eps
            lo.view(-1)[i] -= eps
            num = (scalar(hi, raw0) - scalar(lo, raw0)) / (2 * eps) if which == "dep" else (scalar(dep0, hi) - scalar(dep0, lo)) / (2 * eps)
            ana = float(grad.reshape(-1)[i])
            assert abs(num - ana) <= 1e-6 * max(abs(num), abs(ana)) + noise, (which, int(i), num, ana, noise)
    assert float(ref.d_raw[..., 7:].abs().max()) > 0 and float(ref.d_raw[..., :7].abs().max()) > 0
    # a group whose .w is -1 contributes nothing: zeroing its dRGB changes nothing
    rgb2 = c["d_rgb"].copy()
    rgb2[..., :3][rgb2[..., 3].view(np.int32) < 0] = 0
    assert torch.equal(br.raw_rank1_harmonics(tt, means32, c["views"], rgb2), g_harm.reshape(-1, 3, 25)) and (c["d_rgb"][..., 3].view(np.int32) < 0).any()


def test_the_rank_one_harmonics_gradient_is_the_oracles_dL_dSH():
    """One view, float64: g_harm[c][k] = Y_k(dir) x (the clamp-masked dL/dRGB) equals the oracle's dL/dSH to 1e-12 of its largest entry."""
    import torch
    sc = br.scene("small")
    b, f = sc["b64"], sc["f64"]
    P = sc["means"].shape[0]
    vis = f["radii"] > 0
    rgb = np.zeros((1, P, 4), np.float32)
    masked = np.where(f["clamped"].astype(bool), 0.0, b["raster_rgb"])
    # the cotangent must be float32 (the kernels' d_rgb_sum): feed the oracle's second loop the very same rounded numbers
    rgb[0, :, :3] = masked
    rgb[0, :, 3] = np.where(vis, 0, -1).astype(np.int32).view(np.float32)
    want = sc["orc64"].backward_gaussians(b["raster_xy_pix"], b["raster_conic"], b["raster_opacity"], rgb[0, :, :3].astype(np.float64))["shs"]
    got = br.raw_rank1_harmonics(torch.float64, sc["means"], sc["views"], rgb).numpy().transpose(0, 2, 1)            # [P,25,3]
    assert float(sc["views"][0, 40]) == 1.0 and vis.sum() > 30
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max() and np.abs(want).max() > 0
    assert (got[~vis] == 0).all()
