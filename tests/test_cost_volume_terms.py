"""The per-element float64 statement of the spherical cost volume (tests/cost_volume_reference.py: taps, correlation_terms,
own_gradient_terms, partner_gradient_terms, warp_terms, near_singular) checked on the CPU, before tests/test_gpu_cost_volume_terms.py
holds the kernels to it: the explicit gather agrees with the grid_sample statement and with autograd; no input of the GPU tests has
a sample at which the float64 position itself jumps; the forward bar has teeth (the float32 statement, which is what a kernel with a
float32 warp would compute, breaks it); and the pose set's long merged runs are what they claim to be.  No GPU."""
import pytest
import torch

import cost_volume_reference as R
from splatter360_amd import cost_volume as cv

U = 2.0 ** -24
SHAPES = ("small_v2", "odd_v3", "wide_c")


def inputs(name, device="cpu"):
    """The inputs of tests/test_gpu_cost_volume.py's case `name` (and of d33, made the same way) on `device`: features, poses,
    depths, grad_out."""
    b, v, c, d, h, w, smp = R.terms_cases()[name]
    feats, ext, near, far = R.random_inputs(b, v, c, h, w, seed=sum(map(ord, name)), device=device)
    depths = cv.depth_candidates(near, far, d, smp).float().contiguous()
    poses = cv.relative_poses(ext).contiguous()
    g = torch.randn(v * b, d, h, w, generator=torch.Generator().manual_seed(5)).to(device)
    return feats, poses, depths, g


def forward_k(c, pairs):
    """The forward's rounding count (derived in tests/test_gpu_cost_volume_terms.py): 18 + ceil(CP / 128) + pairs."""
    cp = (c + 3) // 4 * 4
    return 18 + (cp + 127) // 128 + pairs


@pytest.fixture(scope="module")
def statements():
    out = {}
    for name in SHAPES:
        feats, poses, depths, g = inputs(name)
        b, v, c, h, w = feats.shape
        f = feats.transpose(0, 1).reshape(v * b, c, h, w)
        # the exact 1 / ((v - 1) sqrt C) of R.cost_volume, not the float32 value the C entry point receives (R.volume_terms)
        out[name] = (feats, poses, depths, g, *R.correlation_terms(f, f, R.rolled_slots(b, v), poses, depths, 1.0 / ((v - 1) * c ** 0.5)))
    return out


@pytest.mark.parametrize("name", SHAPES)
def test_gather_statement_equals_the_grid_sample_statement(statements, name):
    feats, poses, depths, _, val, mag = statements[name]
    want = R.cost_volume(feats, poses, depths, torch.float64)
    ratio = ((val - want).abs() / (1e-13 * mag)).max().item()
    print(f"{name}: gather against grid_sample, worst |difference| / (1e-13 A) = {ratio:.3g}")
    assert val.shape == want.shape and (mag > 0).all() and ratio <= 1.0


@pytest.mark.parametrize("name", SHAPES)
def test_own_plus_partner_gradient_equals_autograd(statements, name):
    feats, poses, depths, g, _, _ = statements[name]
    b, v, c, h, w = feats.shape
    f = feats.transpose(0, 1).reshape(v * b, c, h, w)
    slots, scale = R.rolled_slots(b, v), R.volume_scale(v, c)
    own, own_mag = R.own_gradient_terms(g, f, slots, poses, depths, scale)
    partner, partner_mag, count = R.partner_gradient_terms(g, f, v * b, slots, poses, depths, scale)
    got = (own + partner).view(v, b, c, h, w).transpose(0, 1)            # the (v b) slots back to [b, v]
    mag = (own_mag + partner_mag).view(v, b, c, h, w).transpose(0, 1)
    # autograd differentiates the statement with the exact 1 / ((v - 1) sqrt C); the entry point's scale is that rounded to float32
    want = R.feature_gradient(feats, poses, depths, g, torch.float64) * (scale * (v - 1) * c ** 0.5)
    ratio = ((got - want).abs() / (1e-12 * mag)).max().item()
    print(f"{name}: own + partner against autograd, worst |difference| / (1e-12 magnitude) = {ratio:.3g}; terms per texel up to {int(count.max())}")
    assert ratio <= 1.0
    assert count.sum().item() > 0 and ((count == 0) == (partner_mag.sum(1) == 0)).all()


def test_no_input_of_the_gpu_tests_is_near_singular():
    for name in R.terms_cases():
        _, poses, depths, _ = inputs(name)
        h, w = R.terms_cases()[name][4:6]
        for k in range(poses.shape[0]):
            assert not R.near_singular(poses[k], depths, h, w).any(), (name, k)
    _, _, depths, _, poses = R.pose_set_inputs()
    nan = depths.clone()
    nan[0, 3] = float("nan")
    for name, pose in poses.items():
        assert not R.near_singular(pose, depths, 12, 20).any(), name
    assert not R.near_singular(poses["centre"], nan, 12, 20).any()


def test_no_sample_of_the_gpu_tests_sits_on_a_cell_edge():
    """The value is continuous across a cell edge, but the partner gradient's term count N and the set of texels that receive
    nothing are not: with every ix, iy at least 1e-9 from an integer, any correct float64 evaluation of the warp finds the same
    cells as this one."""
    def edge_distance(pose, depths, h, w):
        grid, _ = R.warp(pose, depths, h, w)
        grid = grid[torch.isfinite(grid).all(-1)]
        ix, iy = (grid[..., 0] + 1.0) / 2.0 * (w - 1), (grid[..., 1] + 1.0) / 2.0 * (h - 1)
        return min((ix - ix.round()).abs().min().item(), (iy - iy.round()).abs().min().item())

    for name in R.terms_cases():
        _, poses, depths, _ = inputs(name)
        h, w = R.terms_cases()[name][4:6]
        assert min(edge_distance(poses[k], depths, h, w) for k in range(poses.shape[0])) >= 1e-9, name
    _, _, depths, _, poses = R.pose_set_inputs()
    for name, pose in poses.items():
        assert edge_distance(pose, depths, 12, 20) >= 1e-9, name


def test_near_singular_flags_seam_pole_and_centre():
    """Pins the predicate itself at 12 x 20: a half turn about y puts the ray of column 9.5 on the seam, which no pixel has, so
    the seam is reached by translating one pixel's point onto the -z axis; likewise a pole and the centre."""
    h, w = 12, 20
    depths = torch.tensor([[2.0]], dtype=torch.float64)
    ray = R.unit_ray(4, 13, h, w)
    hit = 4 * w + 13

    def flags(target):
        pose = torch.eye(4, dtype=torch.float64).unsqueeze(0)
        pose[0, :3, 3] = torch.tensor(target, dtype=torch.float64) - 2.0 * ray
        return R.near_singular(pose, depths, h, w)[0, 0]

    for target in ([0.0, 0.3, -1.0], [0.0, 1.0, 0.0], [0.0, 0.0, 0.0]):          # seam, pole, centre
        assert flags(target)[hit], target
        assert not flags([target[0] + 1e-6, target[1], target[2]])[hit], target   # 1e-6 off it: an ordinary sample
    assert not flags([0.0, 0.3, 1.0])[hit]                                         # q_x = 0 in front is no seam


@pytest.mark.parametrize("name", ("small_v2", "odd_v3"))
def test_forward_bar_has_teeth_against_a_float32_warp(statements, name):
    """torch's float32 statement evaluates the warp in float32: a kernel that fell back to that would be as far from float64."""
    feats, poses, depths, _, val, mag = statements[name]
    v, c = feats.shape[1:3]
    t32 = R.cost_volume(feats, poses, depths, torch.float32).double()
    ratio = ((t32 - val).abs() / (forward_k(c, v - 1) * U * mag)).max().item()
    print(f"{name}: float32 statement, worst |error| / bar = {ratio:.3g}")
    assert ratio > 2.0


@pytest.mark.parametrize("name", ("identity", "tiny_t"))
def test_every_depth_of_a_pixel_shares_one_cell(name):
    """The partner kernel's longest merged run: all D depths of a pixel in one 2 x 2 cell, every sample valid.  Identity: every
    pixel.  tiny_t: every pixel but two.  Column 9 samples at ix = 9.5 * 19 / 20 = 9.025, the closest any column comes to a cell
    edge; in the two pole rows (cos phi = 0.13) the translation's 1.4e-3 across the ray, seen from depth 0.5, moves the sample by
    up to 0.07 columns, so there the nearest candidate alone falls into column 8: a run of 1 and one of D - 1.  From the second
    candidate (0.92) on, and in every other row, the shift stays below 0.025."""
    _, _, depths, _, poses = R.pose_set_inputs()
    h, w = 12, 20
    t = R.taps(poses[name], depths, h, w)
    assert t.valid.all()
    moved = ((t.x0 != t.x0[:, -1:]) | (t.y0 != t.y0[:, -1:]))[0]         # [D, h w]: not in the farthest candidate's cell
    if name == "identity":
        assert not moved.any()
    else:
        assert moved.nonzero().tolist() == [[0, 0 * w + 9], [0, (h - 1) * w + 9]]


def test_pose_set_reaches_what_it_is_for():
    """The half turn's samples straddle the seam columns, the quarter turn's reach both pole rows, and the centre pose's sample
    of pixel (4, 13) at depths[3] lies 1e-4 depths from the partner's centre."""
    _, _, depths, _, poses = R.pose_set_inputs()
    h, w = 12, 20
    x0 = R.taps(poses["half_turn_y"], depths, h, w).x0
    assert (x0 == 0).any() and (x0 == w - 2).any()
    y0 = R.taps(poses["quarter_turn_x"], depths, h, w).y0
    assert (y0 == 0).any() and (y0 == h - 2).any()
    _, q = R.warp(poses["centre"], depths, h, w)
    r = torch.linalg.norm(q[0, 3, 4 * w + 13]).item() / depths[0, 3].item()
    assert 0.9e-4 <= r <= 1.1e-4
