"""k_gaussians_bwd_sh — the per-Gaussian geometry backward and the dL/dSH product in one pass, what s360_backward runs for a local
step whose views share one camera centre — against the project's own two-kernel path, which stays reachable without any switch:
the same call with defer_sh=True runs s360_backward_split (k_preprocess_bwd<true, false>) and rasterizer.finish_deferred_sh runs
k_sh_bwd with one group.  Same inputs, same grad seeds: every gradient must be the SAME BITS (int32 views are compared, so a
-0 / +0 change is caught).  k_sh_bwd itself (first contributing group stored as 0 + product, no zero-fill pass) is checked for
1, 2 and 3 groups against a float32 torch restatement evaluated in the kernel's operation order, bit for bit.

Every Gaussian has a role by its index (mod 8), so each wave mixes them: visible in no view (inside the near plane) | on a cube
edge | on a cube corner (visible in two / three faces) | SH sum clamped at 0 in one / two / three channels | two plain ones."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FACE = 32


def _cloud(p, m=25, seed=0, shift=0):
    from splatter360_amd import synthetic
    c = synthetic.uniform_cloud(p, d_sh=m, seed=seed, extent=2.0, scale_range=(0.05, 0.4))
    rng = np.random.default_rng(seed + 1000)
    role = (np.arange(p) + shift) % 8
    means, sh = c["means"], c["harmonics"]
    d = rng.standard_normal((p, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    means[role == 0] = 0.01 * d[role == 0]                                  # inside every face's near plane
    sgn = np.where(rng.random((p, 3)) < 0.5, -1.0, 1.0).astype(np.float32)
    r = rng.uniform(0.8, 1.5, (p, 1)).astype(np.float32)
    edge = sgn * r * np.array([1.0, 1.0, 0.05], np.float32)
    edge = np.stack([np.roll(edge[i], i % 3) for i in range(p)])           # the small coordinate names the edge's direction
    means[role == 1] = edge[role == 1]
    means[role == 2] = (sgn * r)[role == 2]
    for n_ch, ro in ((1, 3), (2, 4), (3, 5)):
        sh[role == ro, :n_ch, 0] = -4.0                                     # 0.282 * -4 + 0.5 < 0 whatever the higher bands add: clamped
        sh[role == ro, :n_ch, 1:] *= 0.1
    return c, role


def _views(dev, n_views):
    from splatter360_amd import decoder, synthetic
    pano = torch.from_numpy(synthetic.target_pano_pose((0.0, 0.0, 0.0))).to(dev)
    ext, k, near, far = decoder.cube_cameras(pano, 0.1, 10.0)
    return decoder.pack_camera_views(ext[:n_views], k[:n_views], near[:n_views], far[:n_views], torch.zeros(3, device=dev))


def _step(dev, cloud, *, defer, deg=4, n_views=6, chm=True, cov9=True, depth=False, means2d=False, sh_grad=True):
    """One forward + backward; -> (dict of gradients, RasterState).  defer=True: the two-kernel reference path."""
    from splatter360_amd import rasterizer
    m = torch.tensor(cloud["means"], device=dev).requires_grad_(True)
    cov = torch.tensor(cloud["covariances"], device=dev)
    if not cov9:
        r, c = torch.triu_indices(3, 3)
        cov = cov[:, r, c].contiguous()
    cov.requires_grad_(True)
    sh = torch.tensor(cloud["harmonics"], device=dev)                      # [P,3,M]
    if not chm:
        sh = sh.transpose(1, 2).contiguous()                                # [P,M,3]
    sh.requires_grad_(sh_grad)
    op = torch.tensor(cloud["opacities"], device=dev).requires_grad_(True)
    m2 = torch.zeros((m.shape[0], 3), device=dev, requires_grad=True) if means2d else None
    views = _views(dev, n_views)
    out = rasterizer.rasterize_views(m, cov, op, sh, views=views, image_height=FACE, image_width=FACE, sh_degree=deg,
                                     shared_campos=True, cov9=cov9, sh_channel_major=chm, means2D=m2,
                                     depth_mode="disparity" if depth else None, defer_sh=defer, split_lists=False)
    state = rasterizer.last_state()
    gen = torch.Generator(device="cpu").manual_seed(7)
    loss = (out[0] * torch.randn(out[0].shape, generator=gen).to(dev)).sum()
    if depth:
        loss = loss + (out[2] * torch.randn(out[2].shape, generator=gen).to(dev)).sum()
    loss.backward()
    g = dict(means=m.grad, cov=cov.grad, opac=op.grad)
    if means2d:
        g["means2D"] = m2.grad
    if defer:
        assert sh.grad is None
        d = rasterizer.deferred_of(out[0])
        g["sh"] = rasterizer.finish_deferred_sh(d.prm, d.views, d.means3D, d.shs, d.d_rgb_sum[None])
        g["first_view"] = d.d_rgb_sum[:, 3].contiguous().view(torch.int32)
    elif sh_grad:
        g["sh"] = sh.grad
    torch.cuda.synchronize()
    return g, state


def _same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype == torch.float32, what
    diff = a.contiguous().view(torch.int32) != b.contiguous().view(torch.int32)
    assert not bool(diff.any()), (what, int(diff.sum()), "of", diff.numel(), "words differ")


def _check(dev, p, *, m=25, shift=0, **kw):
    cloud, _ = _cloud(p, m, seed=p, shift=shift)
    want, _ = _step(dev, cloud, defer=True, **kw)
    got, state = _step(dev, cloud, defer=False, **kw)
    for k in ("means", "cov", "sh", "opac") + (("means2D",) if kw.get("means2d") else ()):
        _same_bits(got[k], want[k], (k, p, kw))
    assert bool(torch.isfinite(got["sh"]).all())
    return got, want, state


@pytest.mark.parametrize("p,shift", [(1, 0), (1, 1), (63, 0), (64, 0), (65, 0), (64 * 3 + 17, 0), (64 * 40 + 17, 0)])
def test_fused_equals_two_kernels_at_every_wave_edge(gpu, p, shift):
    """Partial last workgroup, lanes beyond P in the staging loop, the scalar tail of the store loop (P * 75 floats is no
    multiple of 4 for odd P)."""
    _check(gpu, p, shift=shift)


def test_the_cloud_exercises_what_it_is_built_for(gpu):
    """Invisible next to visible Gaussians, Gaussians seen by two and by three faces, one / two / three clamped channels — and
    the gradients of the invisible ones are +0 in every word."""
    p = 64 * 3 + 17
    got, want, state = _check(gpu, p)
    t = state.tensors()
    vis = t["vis_mask"].to(torch.int32)
    n_faces = sum((vis >> v) & 1 for v in range(6))
    assert bool((n_faces == 0).any()) and bool((n_faces == 1).any()) and bool((n_faces == 2).any()) and bool((n_faces >= 3).any())
    lowest_bit = torch.tensor([-1] + [(x & -x).bit_length() - 1 for x in range(1, 64)], dtype=torch.int32, device=gpu)
    first = lowest_bit[vis.long() & 63]                 # first visible view, -1 if none
    assert torch.equal(first, want["first_view"])
    assert bool((first > 0).any())                       # the direction comes from another view than view 0 somewhere
    bits = (vis[None, :] >> torch.arange(6, device=gpu, dtype=torch.int32)[:, None]) & 1
    cl = t["clamped"].to(torch.int32) * bits
    n_cl = (cl & 1) + ((cl >> 1) & 1) + ((cl >> 2) & 1)
    for n in (1, 2, 3):
        assert bool((n_cl == n).any()), n
    inv = n_faces == 0
    assert bool((got["sh"][inv].view(torch.int32) == 0).all()) and bool((got["means"][inv].view(torch.int32) == 0).all())
    assert bool((got["sh"][~inv].abs().amax(dim=(1, 2)) > 0).any())


@pytest.mark.parametrize("chm", [True, False])
@pytest.mark.parametrize("cov9", [True, False])
def test_fused_equals_two_kernels_in_both_sh_and_both_covariance_layouts(gpu, chm, cov9):
    _check(gpu, 64 * 3 + 17, chm=chm, cov9=cov9)


@pytest.mark.parametrize("deg", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("chm", [True, False])
def test_fused_zero_pads_the_coefficients_beyond_the_degree(gpu, deg, chm):
    """M = 25 at every degree: (deg + 1)^2 < M below degree 4, and the padding is +0."""
    got, _, _ = _check(gpu, 64 * 3 + 17, deg=deg, chm=chm)
    n_sh = (deg + 1) ** 2
    pad = got["sh"][:, :, n_sh:] if chm else got["sh"][:, n_sh:, :]
    assert bool((pad.contiguous().view(torch.int32) == 0).all())


@pytest.mark.parametrize("chm", [True, False])
def test_fused_with_sixteen_coefficients_at_degree_three(gpu, chm):
    _check(gpu, 64 * 3 + 17, m=16, deg=3, chm=chm)


@pytest.mark.parametrize("p", [65, 64 * 3 + 17])
def test_fused_with_one_view(gpu, p):
    """V = 1: whatever lies behind or beside the one face is visible nowhere."""
    _, want, _ = _check(gpu, p, n_views=1, shift=1)
    assert bool((want["first_view"] < 0).any()) and bool((want["first_view"] == 0).any())


@pytest.mark.parametrize("cov9", [True, False])
def test_fused_with_the_depth_channel_and_means2d(gpu, cov9):
    """depth_mode given and a non-zero grad_depth; d_means2D requested."""
    got, _, _ = _check(gpu, 64 * 3 + 17, depth=True, means2d=True, cov9=cov9)
    assert float(got["means2D"].abs().max()) > 0
    plain, _ = _step(gpu, _cloud(64 * 3 + 17, seed=64 * 3 + 17)[0], defer=False, cov9=cov9)
    assert not torch.equal(plain["means"], got["means"])        # the depth gradient did reach dL/dmean


def test_frozen_harmonics_take_the_old_kernel_and_keep_the_view_direction_term(gpu):
    """requires_grad=False harmonics (d_shs == NULL): k_preprocess_bwd<true, false> alone — no launch under the SH profile slot,
    one under the geometry slot — with the same dL/dmean (sh_jac term included), dL/dcov and dL/dopacity as with harmonics
    that require grad (the fused kernel: one launch under the geometry slot, none under the SH slot either)."""
    from splatter360_amd import _lib
    cloud, _ = _cloud(64 * 3 + 17, seed=5)
    _lib.profile_enable(True)
    try:
        _lib.profile_collect()
        frozen, _ = _step(gpu, cloud, defer=False, sh_grad=False)
        prof_frozen = _lib.profile_collect()
        full, _ = _step(gpu, cloud, defer=False)
        prof_full = _lib.profile_collect()
        _step(gpu, cloud, defer=True)
        prof_split = _lib.profile_collect()
    finally:
        _lib.profile_enable(False)
    assert "sh" not in frozen
    for k in ("means", "cov", "opac"):
        _same_bits(frozen[k], full[k], k)
    launches = lambda prof, key: sum(n for name, (_, n) in prof.items() if key in name.lower())
    assert launches(prof_split, "preprocess_bwd") == 1 and launches(prof_split, "sh_bwd") == 1      # the reference path: two kernels
    assert launches(prof_full, "preprocess_bwd") == 1 and launches(prof_full, "sh_bwd") == 0        # fused: one
    assert launches(prof_frozen, "preprocess_bwd") == 1 and launches(prof_frozen, "sh_bwd") == 0


# ------------------------------------------------------------------------------------------------------------- k_sh_bwd, N groups
_C0 = 0.28209479177387814
_C1 = 0.4886025119029199
_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
_C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
       -0.5900435899266435)
_C4 = (2.5033429417967046, -1.7701307697799304, 0.9461746957575601, -0.6690465435572892, 0.10578554691520431, -0.6690465435572892,
       0.47308734787878004, -1.7701307697799304, 0.6258357354491761)


def _sh_basis_f32(deg, x, y, z):
    """csrc/s360_device.h sh_basis, operation for operation, on float32 CPU tensors (every torch op is one correctly rounded IEEE
    operation, as every operation of the kernel is under -ffp-contract=off) -> [P, (deg+1)^2]."""
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    ys = [f(_C0).expand_as(x)]
    if deg > 0:
        ys += [f(-_C1) * y, f(_C1) * z, f(-_C1) * x]
    if deg > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        ys += [f(_C2[0]) * xy, f(_C2[1]) * yz, f(_C2[2]) * (2.0 * zz - xx - yy), f(_C2[3]) * xz, f(_C2[4]) * (xx - yy)]
    if deg > 2:
        ys += [f(_C3[0]) * y * (3.0 * xx - yy), f(_C3[1]) * xy * z, f(_C3[2]) * y * (4.0 * zz - xx - yy),
               f(_C3[3]) * z * (2.0 * zz - 3.0 * xx - 3.0 * yy), f(_C3[4]) * x * (4.0 * zz - xx - yy), f(_C3[5]) * z * (xx - yy),
               f(_C3[6]) * x * (xx - 3.0 * yy)]
    if deg > 3:
        ys += [f(_C4[0]) * xy * (xx - yy), f(_C4[1]) * yz * (3.0 * xx - yy), f(_C4[2]) * xy * (7.0 * zz - 1.0),
               f(_C4[3]) * yz * (7.0 * zz - 3.0), f(_C4[4]) * (zz * (35.0 * zz - 30.0) + 3.0), f(_C4[5]) * xz * (7.0 * zz - 3.0),
               f(_C4[6]) * (xx - yy) * (7.0 * zz - 1.0), f(_C4[7]) * xz * (xx - 3.0 * yy),
               f(_C4[8]) * (xx * (xx - 3.0 * yy) - yy * (3.0 * xx - yy))]
    return torch.stack(ys, dim=1)


def _sh_sum_restated(deg, m, views, means, rgbs):
    """sum_j 0 + Y(dir_j) (x) dRGB_j in group order, float32 on the CPU -> [P, 3, M] (channel-major)."""
    p = means.shape[0]
    out = torch.zeros((p, 3, m), dtype=torch.float32)
    n_sh = (deg + 1) ** 2
    for j in range(rgbs.shape[0]):
        w = rgbs[j, :, 3].contiguous().view(torch.int32)
        vw = views[w.clamp(min=0).long()]                                   # [P,44]: the record the group's .w names
        dd = [means[:, a] * vw[:, 40] - vw[:, 32 + a] for a in range(3)]
        # torch's float32 sqrt on the CPU is not correctly rounded (1 ulp off for about 1 value in 150); through float64 it is,
        # as the kernel's sqrtf and division are
        inv = 1.0 / torch.sqrt((dd[0] * dd[0] + dd[1] * dd[1] + dd[2] * dd[2]).double()).float()
        y = _sh_basis_f32(deg, dd[0] * inv, dd[1] * inv, dd[2] * inv)       # [P, n_sh]
        prod = y[:, None, :] * rgbs[j, :, :3, None]                         # [P, 3, n_sh]
        out[:, :, :n_sh] = torch.where((w >= 0)[:, None, None], out[:, :, :n_sh] + prod, out[:, :, :n_sh])
    return out


@pytest.mark.parametrize("n_groups", [1, 2, 3])
@pytest.mark.parametrize("chm,deg,m", [(True, 4, 25), (False, 4, 25), (True, 2, 25), (False, 3, 16)])
def test_sh_backward_n_groups_is_the_ordered_sum_bit_for_bit(gpu, n_groups, chm, deg, m):
    """s360_sh_backward with 1, 2 and 3 groups: Gaussians whose first group is invisible, whose every group is, zero dL/dRGB
    next to a negative Y (a -0 product: stored as +0) — every case bit for bit, since the restatement runs the kernel's own
    operation order (no case needs the 1-ulp-per-group allowance)."""
    from splatter360_amd import _lib, rasterizer
    p = 64 * 3 + 17
    gen = torch.Generator().manual_seed(100 * n_groups + deg)
    means = torch.rand((p, 3), generator=gen) * 4.0 - 2.0
    views = torch.zeros((n_groups, 44), dtype=torch.float32)
    views[:, 32:35] = torch.rand((n_groups, 3), generator=gen) - 0.5
    views[:, 40] = torch.tensor([10.0, 1.0, 2.5][:n_groups])
    views[:, 32:35] *= views[:, 40:41]
    rgbs = torch.randn((n_groups, p, 4), generator=gen)
    rgbs[:, 5::11, :3] = 0.0                                               # zero dL/dRGB: -0 products where Y < 0
    rgbs[:, 7::13, 1] = -0.0
    for j in range(n_groups):
        seen = torch.rand(p, generator=gen) < 0.6
        seen[3::8] = j == n_groups - 1                                      # only the last group sees these: the first ones do not
        seen[4::8] = False                                                  # nobody sees these
        rgbs[j, :, 3] = torch.where(seen, torch.tensor(j, dtype=torch.int32), torch.tensor(-1, dtype=torch.int32)).view(torch.float32)
    want = _sh_sum_restated(deg, m, views, means, rgbs)
    if not chm:
        want = want.transpose(1, 2).contiguous()
    prm = _lib.S360Params()
    prm.P, prm.V, prm.H, prm.W, prm.sh_degree, prm.M = p, n_groups, FACE, FACE, deg, m
    prm.flags = _lib.FLAG_SHARED_CAMPOS | (_lib.FLAG_SH_CHANNEL_MAJOR if chm else 0)
    template = torch.full(want.shape, float("nan"), device=gpu)
    got = rasterizer.finish_deferred_sh(prm, views.to(gpu), means.to(gpu), template, rgbs.to(gpu))
    torch.cuda.synchronize()
    gi, wi = got.cpu().view(torch.int32), want.view(torch.int32)
    bad = (gi != wi).view(p, -1)
    print("k_sh_bwd", n_groups, chm, deg, m, "words that differ:", int(bad.sum()), "in", int(bad.any(1).sum()), "Gaussians; per slab word:",
          bad.sum(0).tolist(), "max |diff|:", float((got.cpu() - want).abs().max()))
    assert bool((wi == -2147483648).sum() == 0)                             # the restated sum holds no -0 either
    assert torch.equal(gi, wi)
