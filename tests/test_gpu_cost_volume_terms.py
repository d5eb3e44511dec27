"""The spherical cost-volume kernels (csrc/s360_cost_volume.hip) held per output element to the float64 statement of
tests/cost_volume_reference.py (taps -> correlation_terms, own_gradient_terms, partner_gradient_terms, warp_terms; pinned on the
CPU by tests/test_cost_volume_terms.py), at every sample: poles, seam and the partner's centre included.

Rule.  With u = 2^-24 (the largest relative error of one float32 rounding) every element obeys

    |got - ref64| <= K u magnitude,

magnitude = the sum of the absolute values of the element's terms with the bilinear weights replaced by 1, and K = the number of
float32 roundings the kernel's source performs on the way to that element, plus 1 for second-order terms, the float64 warp's own
error and the reference's rounding.  An element of magnitude 0 must be exactly 0.  K is counted, never fitted; the worst ratio
|got - ref64| / (K u magnitude) of every case is printed (pytest -s) and, with S360_ACCURACY_REPORT=<file>, written to that file
(profiles/cost_volume_terms_accuracy.json).  No sample is excluded; instead every input must have no sample at which the float64
position itself jumps (cost_volume_reference.near_singular, tol 1e-9), which is asserted, not measured.

The counts (statements of s360_cost_volume.hip, with their line numbers at the commit that added this file; the library is built
with -ffp-contract=off, so a product and a sum are fused only where the source says fmaf):

  weights, 3.  cv_sample: `wx = (float)(ix - fx)`, `wy = (float)(iy - fy)` (85-86) round the float64 fractions: 1/2 u each,
      absolute, since wx, wy < 1.  cv_bilinear4: `(1.f - wx)`, `(1.f - wy)` and their product (105) round once each, 1/2 u
      absolute each as every value is <= 1.  A weight is therefore off by at most 5/2 u, counted as 3 u, whatever its size: this
      is why the magnitude carries unit weights (sum_t |tap_t|) and not sum_t w_t |tap_t|.
  bilinear, 4.  cv_bilinear4: `fmaf(w11, t11, fmaf(w10, t10, fmaf(w01, t01, w00 * t00)))` (107-110): one product and three
      fused multiply-adds, each rounding a partial sum that sum_t |tap_t| bounds.
  forward, K = 18 + ceil(CP / 128) + pairs.  weights 3 + bilinear 4; k_cv_forward: `fmaf(o.w, s.w, fmaf(o.z, s.z, fmaf(o.y, s.y,
      o.x * s.x)))` (197) 4; `acc[dd] +=` (197) once per pass of the `jb` loop (184), i.e. ceil(CP / 128) times per lane;
      cv_fold<16> ... cv_fold<1> (202-206; `keep + __shfl_xor(send, O, 32)`, 152) 5 levels; `tot += acc[0]` (207) once per
      pairing; `tot * a.scale` (210) 1; slack 1.  The first `acc[dd] +=` and the first `tot +=` add to an exact zero and do
      not round, so the count is two above what the source can do: margin that was there before any measurement.
  own gradient, K = 9 + pairs D.  weights 3 + bilinear 4; k_cv_backward_own: `acc.x = fmaf(sg, s.x, acc.x)` (257-260) once
      per depth of every pairing, in sequence, each rounding a partial sum of |g_d| sum_t |tap_t|; `acc.x * a.scale` (267) 1;
      slack 1.
  partner gradient, K = N + 8, N = the number of terms the texel receives (the scatter of ones over its in-range taps).
      k_cv_backward_partner: `own_cl[...] * a.scale` (307) 1; `(1.f - swx) * (1.f - swy) * sg` (335) counted as 5: the weight's
      3 as above, the product with g 1, and 1 more than the source can do (by the forward's counting the statement is worth
      4; the figure was set before any measurement and is kept); then a term enters its run's register sum at `A[t][k] =
      fmaf(wt[t], own[k], A[t][k])` (339) and its texel at `unsafeAtomicAdd` (cv_flush, 284).  A rounding of a partial sum is at most u times the sum of |term| over the terms in
      it, so the total is at most u sum_term |term| (the roundings that term passes through), which is at most (the length of
      its run) + (the number of atomic adds to the texel) <= N + 1, in any arrival order, since the runs' lengths add up to N.
      Slack 1.
  _warp output, K = 8.  k_cv_warp: the weights as `(float)` of cv_sample and the products of line 366, 3; the chain of line 373,
      4; slack 1.

Measured worst ratios on an MI355X: profiles/cost_volume_terms_accuracy.json and DESIGN.md (cost volume, *Tests*)."""
import ctypes as C
import json
import os
from pathlib import Path

import pytest
import torch

import cost_volume_reference as R
from splatter360_amd import _lib, cost_volume as cv

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
REPORT = {}
WHAT = ("tests/test_gpu_cost_volume_terms.py on an MI355X: per case and output the worst |kernel - float64 statement| / (K 2^-24 magnitude) "
        "over all elements (bound: <= 1), K counted from the roundings of csrc/s360_cost_volume.hip (forward 18 + ceil(CP / 128) + pairs, "
        "own gradient 9 + pairs D, partner gradient N + 8 with N the texel's term count, _warp 8), magnitude = the sum of |terms| with unit "
        "bilinear weights; no sample excluded.")


def _report(key, fig):
    """Keep the case's figures; with S360_ACCURACY_REPORT=<file> in the environment also write all of them there (how
    profiles/cost_volume_terms_accuracy.json is made)."""
    REPORT[key] = fig
    path = os.environ.get("S360_ACCURACY_REPORT")
    if path:
        Path(path).write_text(json.dumps(dict(what=WHAT, cases=REPORT), indent=1, sort_keys=True))


def _worst(got, ref, mag, k):
    """The worst |got - ref| / (k u mag) over the elements with mag > 0; the others must be exactly 0.  k: a number or a tensor
    that broadcasts against ref."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    zero = mag == 0
    assert (got[zero] == 0).all()
    ratio = (got - ref).abs() / (U * mag * k).clamp_min(torch.finfo(torch.float64).tiny)
    return ratio[~zero].max().item()


def forward_k(c, pairs):
    cp = (c + 3) // 4 * 4
    return 18 + (cp + 127) // 128 + pairs


def own_k(pairs, d):
    return 9 + pairs * d


def partner_k(count):
    return (count + 8).unsqueeze(1)                                      # [m, 1, h, w] against [m, C, h, w]


def _no_singular_sample(poses, depths, h, w):
    return all(not R.near_singular(poses[k], depths, h, w).any() for k in range(poses.shape[0]))


def _inputs(name):
    """tests/test_gpu_cost_volume.py's inputs of that name (d33: made the same way)."""
    b, v, c, d, h, w, smp = R.terms_cases()[name]
    feats, ext, near, far = R.random_inputs(b, v, c, h, w, seed=sum(map(ord, name)), device=DEV)
    depths = cv.depth_candidates(near, far, d, smp).float().contiguous()
    poses = cv.relative_poses(ext).contiguous()
    return feats, ext, near, far, depths, poses, d, smp


@pytest.mark.parametrize("name", list(R.terms_cases()))
def test_forward_per_element(name):
    feats, ext, near, far, depths, poses, d, smp = _inputs(name)
    b, v, c, h, w = feats.shape
    assert _no_singular_sample(poses, depths, h, w)
    got = cv.spherical_cost_volume(feats, ext, near, far, d, smp, "hm3d")
    ref, mag = R.volume_terms(feats, poses, depths)
    worst = _worst(got, ref, mag, forward_k(c, v - 1))
    print(f"{name}: forward K = {forward_k(c, v - 1)}, worst ratio {worst:.3f}")
    _report(f"{name}/forward", worst)
    assert worst <= 1.0


@pytest.mark.parametrize("name", list(R.terms_cases()))
def test_own_and_partner_gradient_per_element(name):
    feats, ext, near, far, depths, poses, d, smp = _inputs(name)
    b, v, c, h, w = feats.shape
    assert _no_singular_sample(poses, depths, h, w)
    f = feats.transpose(0, 1).reshape(v * b, c, h, w).contiguous()
    g = torch.randn(v * b, d, h, w, device=DEV, generator=torch.Generator(DEV).manual_seed(5))
    slots, scale = cv.partner_slots(b, v, DEV), R.volume_scale(v, c)
    assert torch.equal(slots.cpu().long(), R.rolled_slots(b, v))
    g_own, g_partner = cv.correlation_backward(g, f, f, slots, poses, depths, scale, 0)
    own, own_mag = R.own_gradient_terms(g, f, slots.cpu(), poses, depths, scale)
    partner, partner_mag, count = R.partner_gradient_terms(g, f, v * b, slots.cpu(), poses, depths, scale)
    worst_own = _worst(g_own, own, own_mag, own_k(v - 1, d))
    worst_partner = _worst(g_partner, partner, partner_mag, partner_k(count))
    print(f"{name}: own gradient K = {own_k(v - 1, d)}, worst ratio {worst_own:.3f}; partner gradient N up to {int(count.max())}, "
          f"worst ratio {worst_partner:.3f}")
    _report(f"{name}/own_gradient", worst_own)
    _report(f"{name}/partner_gradient", worst_partner)
    assert worst_own <= 1.0 and worst_partner <= 1.0


@pytest.fixture(scope="module")
def pose_inputs():
    return R.pose_set_inputs(DEV)


def _pair_forward_backward(f_own, f_partner, pose, depths, g):
    fo, fp = f_own.clone().requires_grad_(True), f_partner.clone().requires_grad_(True)
    out = cv.pair_correlation(fo, fp, pose, depths)
    out.backward(g)
    return out.detach(), fo.grad, fp.grad


def _pair_worst(out, g_own, g_partner, f_own, f_partner, pose, depths, g):
    """The three worst ratios of one pairing (pairs = 1, scale = 1, slot i) against the statement at `depths`, `g`."""
    c, d = f_own.shape[1], depths.shape[1]
    p = pose.unsqueeze(0)
    ref, mag = R.correlation_terms(f_own, f_partner, None, p, depths, 1.0)
    own, own_mag = R.own_gradient_terms(g, f_partner, None, p, depths, 1.0)
    partner, partner_mag, count = R.partner_gradient_terms(g, f_own, f_partner.shape[0], None, p, depths, 1.0)
    return (_worst(out, ref, mag, forward_k(c, 1)), _worst(g_own, own, own_mag, own_k(1, d)),
            _worst(g_partner, partner, partner_mag, partner_k(count)), int(count.max()))


@pytest.mark.parametrize("name", ["identity", "half_turn_y", "quarter_turn_x", "tiny_t", "centre"])
def test_pose_set_per_element(pose_inputs, name):
    """Identity and tiny_t: the partner kernel's longest merged runs; the half turn: the seam in the middle of the image; the
    quarter turn: the poles on the equator; centre: a sample 1e-4 depths from the partner's centre.  Every sample is kept."""
    f_own, f_partner, depths, g, poses = pose_inputs
    pose = poses[name]
    assert not R.near_singular(pose, depths, 12, 20).any()
    out, g_own, g_partner = _pair_forward_backward(f_own, f_partner, pose, depths, g)
    fwd, own, partner, n_max = _pair_worst(out, g_own, g_partner, f_own, f_partner, pose, depths, g)
    print(f"pose {name}: worst ratio forward {fwd:.3f}, own gradient {own:.3f}, partner gradient {partner:.3f} (N up to {n_max})")
    _report(f"pose_{name}/forward", fwd)
    _report(f"pose_{name}/own_gradient", own)
    _report(f"pose_{name}/partner_gradient", partner)
    assert fwd <= 1.0 and own <= 1.0 and partner <= 1.0


def test_nan_candidate_in_the_middle_of_the_row(pose_inputs):
    """Candidate 3 of 7 is NaN under the general pose: that depth's volume is exactly 0, the other depths are the bits of the call
    on the six remaining candidates, both gradients are those of the six (the NaN depth's g is finite and must go nowhere), and
    nothing is non-finite."""
    f_own, f_partner, depths, g, poses = pose_inputs
    pose = poses["centre"]
    keep = [0, 1, 2, 4, 5, 6]
    with_nan = depths.clone()
    with_nan[0, 3] = float("nan")
    assert not R.near_singular(pose, with_nan, 12, 20).any()
    out, g_own, g_partner = _pair_forward_backward(f_own, f_partner, pose, with_nan, g)
    six = cv.pair_correlation(f_own, f_partner, pose, depths[:, keep].contiguous())
    assert all(torch.isfinite(t).all() for t in (out, g_own, g_partner))
    assert (out[:, 3] == 0).all()
    assert torch.equal(out[:, keep], six)
    fwd, own, partner, n_max = _pair_worst(out[:, keep], g_own, g_partner, f_own, f_partner, pose, depths[:, keep], g[:, keep])
    print(f"NaN candidate: worst ratio forward {fwd:.3f}, own gradient {own:.3f}, partner gradient {partner:.3f} (N up to {n_max})")
    _report("nan_candidate/forward", fwd)
    _report("nan_candidate/own_gradient", own)
    _report("nan_candidate/partner_gradient", partner)
    assert fwd <= 1.0 and own <= 1.0 and partner <= 1.0


def test_partner_slot_outside_the_table_contributes_nothing():
    """include/s360.h: a partner_slot entry outside [0, m) contributes nothing.  odd_v3's first pairing with a second row of -1
    (its poses are real) and the same scale: forward and own gradient are the bits of the pairs = 1 call, the partner gradient
    is within its bar of the one pairing's statement."""
    feats, ext, near, far, depths, poses, d, smp = _inputs("odd_v3")
    b, v, c, h, w = feats.shape
    f = feats.transpose(0, 1).reshape(v * b, c, h, w).contiguous()
    g = torch.randn(v * b, d, h, w, device=DEV, generator=torch.Generator(DEV).manual_seed(6))
    slots = cv.partner_slots(b, v, DEV)
    slots[1] = -1
    scale = R.volume_scale(v, c)
    one = (slots[:1].contiguous(), poses[:1].contiguous())
    out2 = cv.correlation_forward(f, f, slots, poses, depths, scale, 0)
    out1 = cv.correlation_forward(f, f, *one, depths, scale, 0)
    own2, partner2 = cv.correlation_backward(g, f, f, slots, poses, depths, scale, 0)
    own1, _ = cv.correlation_backward(g, f, f, *one, depths, scale, 0)
    assert torch.equal(out2, out1) and torch.equal(own2, own1)
    partner, partner_mag, count = R.partner_gradient_terms(g, f, v * b, slots.cpu(), poses, depths, scale)
    again = R.partner_gradient_terms(g, f, v * b, one[0].cpu(), one[1], depths, scale)
    assert all(torch.equal(x, y) for x, y in zip((partner, partner_mag, count), again))     # the statement skips the row too
    worst = _worst(partner2, partner, partner_mag, partner_k(count))
    print(f"slot -1: partner gradient N up to {int(count.max())}, worst ratio {worst:.3f}")
    _report("slot_outside/partner_gradient", worst)
    assert worst <= 1.0


def test_warp_entry_point_per_element():
    """s360_cost_volume_warp at odd_v3's shape with its first pairing's poses and slot row: every element within K = 8."""
    feats, ext, near, far, depths, poses, d, smp = _inputs("odd_v3")
    b, v, c, h, w = feats.shape
    n = v * b
    assert _no_singular_sample(poses[:1], depths, h, w)
    f = feats.transpose(0, 1).reshape(n, c, h, w).contiguous()
    slots = cv.partner_slots(b, v, DEV)[0].contiguous()
    pose = poses[0].contiguous()
    out = torch.full((n, c, d, h, w), 7.0, device=DEV)
    rc = _lib.lib().s360_cost_volume_warp(C.c_void_p(f.data_ptr()), C.c_void_p(slots.data_ptr()), C.c_void_p(pose.data_ptr()),
                                          C.c_void_p(depths.data_ptr()), n, n, c, h, w, d, 0, C.c_void_p(out.data_ptr()),
                                          C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    ref, mag = R.warp_terms(f[slots.long()], pose, depths)
    worst = _worst(out, ref, mag, 8)
    print(f"_warp: worst ratio {worst:.3f}")
    _report("odd_v3/warp", worst)
    assert worst <= 1.0
