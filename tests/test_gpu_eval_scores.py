"""s360_depth_metrics and s360_psnr (csrc/s360_eval_scores.hip) through splatter360_amd.metrics, against the numpy statement
tests/depth_metrics_reference.py on the same inputs (its fidelity to the reference's functions is pinned on CPU in
tests/test_eval_scores_spec.py, where the reference's own float32 arithmetic meets every bar below).

Bars, none of them fitted to the kernels:
  a-metrics, valid_count, NaN / inf patterns   exact: the counts are integers below 2^24, the division and the x 100 single
                                               float32 operations
  abs_diff, abs_rel, sq_rel, rmse              relative 2^-22 against the float32-terms / float64-sums statement: the terms are
                                               bit-identical (IEEE sub / mul / div), the float64 sums of <= 2^24 terms agree to
                                               ~1e-9, one rounding to float32 (2^-24) and a square root
  rmse_log                                     the device's logf and the host's differ in the last place: against the all-float64
                                               statement within depth_metrics_reference.rmse_log_bound (u = 2^-22, computed from
                                               the data)
  PSNR                                         4.35 * 2^-22 + 4 ulp32(|psnr|) dB against the float64-sum statement
  depth_scores                                 relative 2^-22 against the statement's average of its own rows (float64 sum of
                                               float32 rows, one division, one rounding); rmse_log: the mean of the rows' bounds
                                               plus 2^-23 of the value
"""
import sys
import types
from pathlib import Path

import numpy as np
import pytest
import torch

import depth_metrics_reference as R

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "eval_scores.npz"
REL = 2.0 ** -22


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _same_specials(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.where(np.isinf(a), a, 0), np.where(np.isinf(b), b, 0))


def _check_rows(got: dict, count, gt, pred, valid, mult_a, what=""):
    """got: {key: float32 [B] on the GPU}, count: int32 [B] or None; gt, pred, valid: numpy, the rows the kernel saw."""
    want, want_count = R.depth_metrics(gt, pred, valid, mult_a)
    f64 = R.depth_metrics_f64(gt, pred, valid)
    bound = R.rmse_log_bound(gt, pred, valid)
    assert tuple(got.keys()) == R.KEYS
    if count is not None:
        assert count.dtype == torch.int32 and np.array_equal(count.cpu().numpy(), want_count)
    for k in R.KEYS:
        g = got[k]
        assert g.dtype == torch.float32 and g.shape == (gt.shape[0],) and g.is_cuda, k
        g = g.cpu().numpy()
        ref = f64[k] if k == "rmse_log" else want[k]
        assert _same_specials(g, ref), (what, k, g, ref)
        fin = np.isfinite(ref)
        if k in R.A_KEYS:
            assert np.array_equal(g, want[k], equal_nan=True), (what, k, g, want[k])
        elif k == "rmse_log":
            err = np.abs(g.astype(np.float64)[fin] - ref[fin])
            print(f"{what} rmse_log: at most {np.max(err / np.maximum(bound[fin], 1e-300), initial=0):.3f} of the bound")
            assert (err <= bound[fin]).all(), (what, k, err, bound[fin])
        else:
            err = np.abs(g.astype(np.float64)[fin] - ref[fin].astype(np.float64)) / np.maximum(np.abs(ref[fin]), 1e-300)
            print(f"{what} {k}: relative error {np.max(err, initial=0):.2e} (bar {REL:.2e})")
            assert (err <= REL).all(), (what, k, err)


def _check_depth(gt: torch.Tensor, pred: torch.Tensor, valid: torch.Tensor, mult_a=False, what=""):
    from splatter360_amd import metrics
    got, count = metrics.depth_metrics(gt, pred, valid, mult_a, return_valid_count=True)
    _check_rows(got, count, gt.cpu().numpy(), pred.cpu().numpy(), valid.cpu().numpy(), mult_a, what)
    return got


def _check_scores(got: dict, depth_pred, depth_gt, what="", **kw):
    gt, pred, valid = R.depth_score_rows(depth_pred.cpu().numpy(), depth_gt.cpu().numpy(), **kw)
    rows, count = R.depth_metrics(gt, pred, valid, mult_a=True)
    want = R.average_valid_rows(rows, count)
    has = count > 0
    f64 = R.depth_metrics_f64(gt, pred, valid)["rmse_log"]
    with np.errstate(all="ignore"):
        want_log = np.where(has, f64, 0.0).sum() / has.sum()
    log_bound = np.where(has, R.rmse_log_bound(gt, pred, valid), 0.0).sum() / max(has.sum(), 1) + 2.0 ** -23 * abs(want_log)
    assert tuple(got.keys()) == R.KEYS
    for k in R.KEYS:
        g = got[k]
        assert g.dtype == torch.float32 and g.dim() == 0 and g.is_cuda, k
        g = float(g)
        ref = float(want_log) if k == "rmse_log" else float(want[k])
        assert _same_specials([g], [ref]), (what, k, g, ref)
        if np.isfinite(ref):
            bar = log_bound if k == "rmse_log" else REL * abs(ref)
            print(f"{what} score {k}: {g} error {abs(g - ref):.2e} (bar {bar:.2e})")
            assert abs(g - ref) <= bar, (what, k, g, ref)
    return count


def _random_depth(shape, seed, dev, holes=True):
    g = _gen(seed)
    gt = torch.rand(shape, generator=g) * 9.9 + 0.05
    if holes:
        gt[torch.rand(shape, generator=g) < 0.15] = 0.0
    pred = (gt * (1 + 0.2 * torch.randn(shape, generator=g)) + 0.05 * torch.randn(shape, generator=g)).abs() + 1e-3
    return gt.to(dev), pred.to(dev)


def _rendered_depth(dev, w=256):
    """The evaluation shape: depth of the six w x w cube faces of three target panoramas, from the fused pass -> [18,w,w]."""
    from splatter360_amd import decoder, synthetic
    cloud = synthetic.encoder_like_cloud(128, 256, seed=5)
    ps = [torch.tensor(cloud[k], device=dev) for k in ("means", "covariances", "harmonics", "opacities")]
    faces = []
    with torch.no_grad():
        for pos in ((0.0, 0.0, 0.0), (0.3, -0.1, 0.2), (-0.2, 0.15, -0.3)):
            pano = torch.from_numpy(synthetic.target_pano_pose(pos)).to(dev)
            ext, K, near, far = decoder.cube_cameras(pano, 0.1, 10.0)
            _, depth = decoder.render_views_fused(ext, K, near, far, (w, w), torch.zeros(3, device=dev), *ps, shared_campos=True,
                                                  depth_mode="depth")
            faces.append(depth)
    return torch.cat(faces).contiguous()


def _perturbed_gt(depth, seed):
    """A perturbed copy of rendered depth with holes, as ground truth."""
    g = _gen(seed)
    gt = depth.cpu() * (1 + 0.1 * torch.randn(depth.shape, generator=g)) + 0.02 * torch.randn(depth.shape, generator=g)
    gt[torch.rand(depth.shape, generator=g) < 0.1] = 0.0
    return gt.to(depth.device).contiguous()


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("case", ("holes", "clean", "masked"))
@pytest.mark.parametrize("mult_a", (False, True))
def test_golden_depth_cases(gpu, golden, case, mult_a):
    gt, pred, valid = (torch.from_numpy(golden[f"depth_{case}_{k}"]).to(gpu) for k in ("gt", "pred", "valid"))
    got = _check_depth(gt, pred, valid, mult_a, what=case)
    want = golden[f"depth_{case}_out_mult" if mult_a else f"depth_{case}_out"]
    for i, k in enumerate(R.KEYS):                           # and against the reference's recorded numbers
        g = got[k].cpu().numpy()
        assert _same_specials(g, want[i]), k
        if k in R.A_KEYS:
            assert np.array_equal(g, want[i], equal_nan=True), k


def test_golden_psnr_cases(gpu, golden):
    from splatter360_amd import metrics
    pred, gt = torch.from_numpy(golden["psnr_pred"]).to(gpu), torch.from_numpy(golden["psnr_gt"]).to(gpu)
    got = _check_psnr(pred, gt)
    assert np.isnan(got[8]) and got[7] == 100.0 and got[9] == 100.0
    ref = golden["psnr_out"].astype(np.float64)
    fin = np.isfinite(ref)
    assert _same_specials(got, ref) and (np.abs(got[fin] - ref[fin]) <= 2 * R.psnr_bar(ref)[fin]).all()   # both within one bar of the statement
    assert np.array_equal(got, metrics.psnr(gt, pred).cpu().numpy().astype(np.float64), equal_nan=True)   # symmetric


def _check_psnr(pred, gt, got=None):
    from splatter360_amd import metrics
    if got is None:
        got = metrics.psnr(pred, gt)
    assert got.dtype == torch.float32 and got.shape == (pred.shape[0],) and got.device == pred.device
    want = R.psnr(pred.cpu().numpy(), gt.cpu().numpy())
    g = got.cpu().numpy().astype(np.float64)
    assert _same_specials(g, want), (g, want)
    fin = np.isfinite(want)
    err, bar = np.abs(g[fin] - want[fin]), R.psnr_bar(want)[fin]
    print(f"psnr {tuple(pred.shape)}: worst error {np.max(err, initial=0):.2e} dB, smallest bar {np.min(bar, initial=1):.2e}")
    assert (err <= bar).all(), (err, bar)
    return g


def test_evaluation_shape_rendered_depth(gpu):
    from splatter360_amd import metrics
    depth = _rendered_depth(gpu)
    assert depth.shape == (18, 256, 256) and torch.isfinite(depth).all()
    gt = _perturbed_gt(depth, 1)
    # all 18 faces as rows; uncovered pixels (pred == 0) give rmse_log = inf, exactly as in the statement
    _check_depth(gt.flatten(1), depth.flatten(1), gt.flatten(1) > 0.1, mult_a=True, what="rendered")
    covered = depth.clamp_min(1e-3)
    _check_depth(gt.flatten(1), covered.flatten(1), gt.flatten(1) > 0.1, mult_a=True, what="rendered, covered")
    # the step's protocol on the tensors it holds: face 0 of every view dropped, 15 rows
    depth_gt = gt.view(1, 3, 6, 256, 256, 1)
    for pred, what in ((depth, "rendered"), (covered, "covered")):
        depth_pred = pred.view(1, 18, 256, 256)
        count = _check_scores(metrics.depth_scores(depth_pred, depth_gt), depth_pred, depth_gt, what=what)
        assert count.shape == (15,)
    # a face without any valid depth is left out of the average
    depth_gt2 = depth_gt.clone()
    depth_gt2[0, 1, 3] = 0.0
    count = _check_scores(metrics.depth_scores(covered.view(1, 18, 256, 256), depth_gt2), covered.view(1, 18, 256, 256), depth_gt2,
                          what="one empty face")
    assert (count == 0).sum() == 1
    # the same rows through depth_metrics
    rows_gt = depth_gt[0, :, 1:, :, :, 0].reshape(15, -1)
    rows_pred = covered.view(3, 6, -1)[:, 1:].reshape(15, -1)
    _check_depth(rows_gt, rows_pred, rows_gt > 0.1, mult_a=True, what="15 rows")
    # [b, v, 6, H, W] without the trailing 1, b = 3 / v = 1, and keeping face 0
    _check_scores(metrics.depth_scores(covered.view(3, 6, 256, 256), depth_gt.view(3, 1, 6, 256, 256)), covered.view(3, 6, 256, 256),
                  depth_gt.view(3, 1, 6, 256, 256), what="b=3")
    _check_scores(metrics.depth_scores(covered.view(1, 18, 256, 256), depth_gt, drop_first_face=False, min_depth=0.5),
                  covered.view(1, 18, 256, 256), depth_gt, what="18 rows", drop_first_face=False, min_depth=0.5)


@pytest.mark.parametrize("hw,HW", [((256, 256), (512, 512)), ((256, 256), (320, 320)), ((128, 128), (64, 64)), ((100, 37), (37, 100))])
def test_depth_scores_nearest_lookup(gpu, hw, HW):
    """Ground truth at another resolution than the rendered depth: pred is looked up by F.interpolate(mode="nearest")'s rule."""
    from splatter360_amd import metrics
    if hw == (256, 256):
        pred = _rendered_depth(gpu).clamp_min(1e-3).view(1, 18, 256, 256)
    else:
        pred = (torch.rand((1, 18, *hw), generator=_gen(3)) * 8 + 0.2).to(gpu)
    up = torch.nn.functional.interpolate(pred, size=HW, mode="bilinear", align_corners=False)
    gt = _perturbed_gt(up, 2).view(1, 3, 6, *HW, 1)
    got = metrics.depth_scores(pred, gt)
    _check_scores(got, pred, gt, what=f"{hw}->{HW}")
    # and it is what F.interpolate + depth_metrics give on the rearranged tensors
    near = torch.nn.functional.interpolate(pred, size=HW, mode="nearest").view(3, 6, -1)[:, 1:].reshape(15, -1)
    rows_gt = gt[0, :, 1:, :, :, 0].reshape(15, -1)
    rows = metrics.depth_metrics(rows_gt, near, rows_gt > 0.1, mult_a=True)
    for k in R.KEYS:
        want = R.average_valid_rows({k: rows[k].cpu().numpy()}, np.ones(15))[k]
        assert float(got[k]) == float(want), (k, float(got[k]), float(want))


@pytest.mark.parametrize("shape", [(15, 64 * 64), (15, 512 * 512), (1, 256 * 256), (1, 1), (2, 3), (3, 4095), (3, 4096), (3, 4097),
                                   (5, 1000), (2, 3 * 4096 + 5)])
def test_shapes(gpu, shape):
    """64 x 64 and 512 x 512 faces, B = 1, N below, at and above the workgroup's stride of 4096 elements and no multiple of 4."""
    gt, pred = _random_depth(shape, 7, gpu)
    _check_depth(gt, pred, gt > 0.1, mult_a=True, what=str(shape))
    valid = (torch.rand(shape, generator=_gen(8)) > 0.4).to(gpu)
    _check_depth(gt + 0.01, pred, valid, mult_a=False, what=f"{shape} mask")


@pytest.mark.parametrize("shape", [(18, 3, 256, 256), (6, 3, 512, 512), (55, 3, 64, 64), (1, 1, 1, 1), (2, 3, 5, 7), (3, 1, 37, 301)])
@pytest.mark.parametrize("noise", (0.2, 1e-3, 1e-5))
def test_psnr_shapes(gpu, shape, noise):
    gt = torch.rand(shape, generator=_gen(9)) * 1.2 - 0.1
    pred = gt + noise * torch.randn(shape, generator=_gen(10))
    _check_psnr(pred.to(gpu), gt.to(gpu))


def test_determinism_and_batch_independence(gpu):
    from splatter360_amd import metrics
    gt, pred = _random_depth((15, 256 * 256), 11, gpu)
    valid = gt > 0.1
    a = metrics.depth_metrics(gt, pred, valid, True)
    b = metrics.depth_metrics(gt, pred, valid, True)
    for k in R.KEYS:
        assert torch.equal(a[k], b[k]), k
    for i in range(gt.shape[0]):
        one = metrics.depth_metrics(gt[i:i + 1], pred[i:i + 1], valid[i:i + 1], True)
        for k in R.KEYS:
            assert torch.equal(one[k][0], a[k][i]), (k, i)
    x = torch.rand((18, 3, 256, 256), generator=_gen(12)).to(gpu)
    y = (x + 0.05 * torch.randn(x.shape, generator=_gen(13)).to(gpu)).contiguous()
    p = metrics.psnr(x, y)
    assert torch.equal(p, metrics.psnr(x, y))
    for i in range(x.shape[0]):
        assert torch.equal(metrics.psnr(x[i:i + 1], y[i:i + 1])[0], p[i]), i
    d = _rendered_depth(gpu, 64).clamp_min(1e-3).view(1, 18, 64, 64)
    g = _perturbed_gt(d, 14).view(1, 3, 6, 64, 64, 1)
    s1, s2 = metrics.depth_scores(d, g), metrics.depth_scores(d, g)
    assert all(torch.equal(s1[k], s2[k]) for k in R.KEYS)


def test_non_default_stream(gpu):
    from splatter360_amd import metrics
    gt, pred = _random_depth((15, 256 * 256), 15, gpu)
    want = metrics.depth_metrics(gt, pred, gt > 0.1, True)
    x = torch.rand((18, 3, 256, 256), generator=_gen(16)).to(gpu)
    y = torch.rand((18, 3, 256, 256), generator=_gen(17)).to(gpu)
    want_p = metrics.psnr(x, y)
    want_s = metrics.depth_scores(pred.view(1, 15, 256, 256), gt.view(1, 3, 5, 256, 256), faces_per_view=5)
    s = torch.cuda.Stream(device=gpu)
    s.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(s):
        gs, ps = gt * 1.0, pred * 1.0                     # produced on s: the calls must run after them, on s
        got = metrics.depth_metrics(gs, ps, gs > 0.1, True)
        got_p = metrics.psnr(x * 1.0, y * 1.0)
        got_s = metrics.depth_scores(ps.view(1, 15, 256, 256), gs.view(1, 3, 5, 256, 256), faces_per_view=5)
    torch.cuda.current_stream(gpu).wait_stream(s)
    for k in R.KEYS:
        assert torch.equal(got[k], want[k]) and torch.equal(got_s[k], want_s[k]), k
    assert torch.equal(got_p, want_p)
    _check_rows(got, None, gt.cpu().numpy(), pred.cpu().numpy(), (gt > 0.1).cpu().numpy(), True, "side stream")


def test_strided_inputs_equal_their_contiguous_copies(gpu):
    from splatter360_amd import metrics
    n = 5000
    big_gt, big_pred = _random_depth((6, n + 40), 18, gpu)
    big_valid = big_gt > 0.1
    for ofs in (0, 4, 3, 1):                                  # rows that start 16-byte aligned, and rows that do not
        gt, pred, valid = big_gt[:, ofs:ofs + n], big_pred[:, ofs:ofs + n], big_valid[:, ofs:ofs + n]
        assert not gt.is_contiguous() and gt.stride(1) == 1
        a = metrics.depth_metrics(gt, pred, valid, True)
        b = metrics.depth_metrics(gt.contiguous(), pred.contiguous(), valid.contiguous(), True)
        for k in R.KEYS:
            assert torch.equal(a[k], b[k]), (k, ofs)
        c = metrics.depth_metrics(gt, pred.contiguous(), valid, True)          # mixed layouts
        assert all(torch.equal(a[k], c[k]) for k in R.KEYS)
    _check_depth(big_gt[:, 3:3 + n], big_pred[:, 3:3 + n], big_valid[:, 3:3 + n], True, "strided rows")
    # every other row, and a transposed layout (elements of a row not adjacent: converted)
    a = metrics.depth_metrics(big_gt[::2], big_pred[::2], big_valid[::2])
    b = metrics.depth_metrics(big_gt[::2].contiguous(), big_pred[::2].contiguous(), big_valid[::2].contiguous())
    assert all(torch.equal(a[k], b[k]) for k in R.KEYS)
    tg, tp = big_gt.t().contiguous().t(), big_pred.t().contiguous().t()
    assert tg.stride(1) != 1
    a = metrics.depth_metrics(tg, tp, (tg > 0.1).t().contiguous().t())
    b = metrics.depth_metrics(big_gt, big_pred, big_valid)
    assert all(torch.equal(a[k], b[k]) for k in R.KEYS)
    # an expanded mask (row stride 0) and a non-bool mask
    row_mask = (torch.rand(n + 40, generator=_gen(19)) > 0.5).to(gpu)
    a = metrics.depth_metrics(big_gt + 0.01, big_pred, row_mask.expand(6, -1))
    b = metrics.depth_metrics(big_gt + 0.01, big_pred, row_mask.expand(6, -1).contiguous().float())
    assert all(torch.equal(a[k], b[k]) for k in R.KEYS)
    # other float types are converted
    h = metrics.depth_metrics(big_gt.half(), big_pred.double(), big_valid)
    f = metrics.depth_metrics(big_gt.half().float(), big_pred.double().float(), big_valid)
    assert all(h[k].dtype == torch.float32 and torch.equal(h[k], f[k]) for k in R.KEYS)
    # psnr: sliced images (not contiguous; the copy may start unaligned) and an unaligned contiguous view
    x = torch.rand((5, 3, 33, 35), generator=_gen(20)).to(gpu)
    y = torch.rand((5, 3, 33, 35), generator=_gen(21)).to(gpu)
    xs, ys = x[:, :, 1:, 2:], y[:, :, 1:, 2:]
    assert torch.equal(metrics.psnr(xs, ys), metrics.psnr(xs.contiguous(), ys.contiguous()))
    assert torch.equal(metrics.psnr(x[1:], y[1:]), metrics.psnr(x, y)[1:])     # 3 * 33 * 35 floats per image: images 1.. start unaligned
    _check_psnr(x[1:], y[1:])
    assert torch.equal(metrics.psnr(x.half(), y.double()), metrics.psnr(x.half().float(), y.double().float()))
    # depth_scores: non-contiguous tensors are converted
    d, g = _random_depth((1, 12, 40, 56), 22, gpu)
    g6 = g.view(1, 2, 6, 40, 56, 1)
    want = metrics.depth_scores(d, g6)
    got = metrics.depth_scores(d.transpose(2, 3).contiguous().transpose(2, 3), g6.transpose(3, 4).contiguous().transpose(3, 4))
    assert all(torch.equal(want[k], got[k]) for k in R.KEYS)


def test_errors_and_empty_batches(gpu):
    from splatter360_amd import metrics
    gt, pred = _random_depth((4, 100), 23, gpu)
    valid = gt > 0.1
    with pytest.raises(ValueError):
        metrics.depth_metrics(gt, pred[:3], valid)
    with pytest.raises(ValueError):
        metrics.depth_metrics(gt, pred, valid[:, :50])
    with pytest.raises(ValueError):
        metrics.depth_metrics(gt[0], pred[0], valid[0])
    with pytest.raises(RuntimeError):
        metrics.depth_metrics(gt.cpu(), pred.cpu(), valid.cpu())
    with pytest.raises(RuntimeError):
        metrics.depth_metrics(gt, pred, valid.cpu())
    empty, count = metrics.depth_metrics(gt[:0], pred[:0], valid[:0], return_valid_count=True)
    assert tuple(empty.keys()) == R.KEYS and all(v.shape == (0,) and v.dtype == torch.float32 and v.is_cuda for v in empty.values())
    assert count.shape == (0,)
    none = metrics.depth_metrics(gt[:, :0], pred[:, :0], valid[:, :0])
    assert all(v.shape == (4,) and torch.isnan(v).all() for v in none.values())
    # no valid element at all: NaN twelve times per row, and from depth_scores
    nothing = metrics.depth_metrics(gt, pred, torch.zeros_like(valid))
    assert all(torch.isnan(v).all() for v in nothing.values())
    s = metrics.depth_scores(pred.view(1, 4, 10, 10), torch.zeros((1, 1, 4, 10, 10, 1), device=gpu), faces_per_view=4)
    assert all(torch.isnan(v) for v in s.values())
    x = torch.rand((3, 3, 8, 8), device=gpu)
    with pytest.raises(ValueError):
        metrics.psnr(x, x[:2])
    with pytest.raises(ValueError):
        metrics.psnr(x[0], x[0])
    with pytest.raises(RuntimeError):
        metrics.psnr(x.cpu(), x.cpu())
    e = metrics.psnr(x[:0], x[:0])
    assert e.shape == (0,) and e.dtype == torch.float32 and e.is_cuda
    with pytest.raises(ValueError):
        metrics.depth_scores(pred.view(1, 4, 10, 10), gt.view(1, 1, 4, 10, 10, 1))                  # faces_per_view = 6 does not fit
    with pytest.raises(ValueError):
        metrics.depth_scores(pred.view(2, 2, 10, 10), gt.view(1, 2, 2, 10, 10, 1), faces_per_view=2)   # batch sizes differ
    with pytest.raises(RuntimeError):
        metrics.depth_scores(pred.view(1, 4, 10, 10).cpu(), gt.view(1, 1, 4, 10, 10, 1).cpu(), faces_per_view=4)


def test_reference_contracts(gpu):
    """compute_depth_metrics_batched(gt_bN, pred_bN, valid_masks_bN, mult_a) -> the twelve keys, float32 [B] on the device,
    inputs untouched; compute_psnr(ground_truth, predicted) -> [b] (compute_depth_metrics.py:47-116, metrics.py:11-21)."""
    from splatter360_amd import metrics
    gt, pred = _random_depth((15, 4096), 24, gpu)
    valid = gt > 0.1
    gt0, pred0 = gt.clone(), pred.clone()
    got = metrics.compute_depth_metrics_batched(gt, pred, valid, mult_a=True)
    assert torch.equal(gt, gt0) and torch.equal(pred, pred0)
    _check_rows(got, None, gt.cpu().numpy(), pred.cpu().numpy(), valid.cpu().numpy(), True, "contract")
    plain = metrics.compute_depth_metrics_batched(gt, pred, valid)
    assert torch.equal(plain["a25"] * 100, got["a25"]) and torch.equal(plain["rmse"], got["rmse"])
    x = torch.rand((4, 3, 32, 32), generator=_gen(25)).to(gpu)
    y = torch.rand((4, 3, 32, 32), generator=_gen(26)).to(gpu)
    p = metrics.compute_psnr(x, y)
    assert p.shape == (4,) and p.dtype == torch.float32 and p.device == y.device and torch.equal(p, metrics.psnr(y, x))
    assert metrics.compute_psnr(x.half(), y.half()).dtype == torch.float16
    _check_psnr(y, x, p)


def test_patched_functions_through_the_seam(gpu, monkeypatch):
    """install(depth_metrics=True, psnr=True)'s replacements: the kernels for GPU tensors, the replaced functions for CPU
    tensors and for the inputs the native path does not take."""
    from splatter360_amd import metrics, plugin
    calls = []

    def replaced_depth(gt_bN, pred_bN, valid_masks_bN, mult_a=False):
        calls.append(("depth", gt_bN.device.type, gt_bN.dtype, mult_a))
        return {"abs_diff": torch.full((gt_bN.shape[0],), -3.0)}

    def replaced_psnr(ground_truth, predicted):
        calls.append(("psnr", ground_truth.device.type))
        return torch.full((ground_truth.shape[0],), -2.0)

    dmod = types.ModuleType(plugin.DEPTH_METRICS_MODULE)
    dmod.compute_depth_metrics_batched = replaced_depth
    user = types.ModuleType(plugin.DEPTH_METRICS_USERS[0])
    user.compute_depth_metrics_batched, user.compute_psnr = replaced_depth, replaced_psnr
    mmod = types.ModuleType(plugin.METRICS_MODULE)
    mmod.compute_psnr = replaced_psnr
    for m in (dmod, user, mmod):
        monkeypatch.setitem(sys.modules, m.__name__, m)
    fd, fp = plugin.install_depth_metrics(), plugin.install_psnr()
    try:
        assert dmod.compute_depth_metrics_batched is fd and user.compute_depth_metrics_batched is fd and fd.replaced is replaced_depth
        assert mmod.compute_psnr is fp and user.compute_psnr is fp and fp.replaced is replaced_psnr
        gt, pred = _random_depth((15, 64 * 64), 27, gpu)
        valid = gt > 0.1
        got = user.compute_depth_metrics_batched(gt, pred, valid, mult_a=True)
        assert not calls
        want = metrics.compute_depth_metrics_batched(gt, pred, valid, True)
        assert all(torch.equal(got[k], want[k]) for k in R.KEYS)
        _check_rows(got, None, gt.cpu().numpy(), pred.cpu().numpy(), valid.cpu().numpy(), True, "seam")
        assert user.compute_depth_metrics_batched(gt.cpu(), pred.cpu(), valid.cpu(), mult_a=True)["abs_diff"].tolist() == [-3.0] * 15
        assert calls == [("depth", "cpu", torch.float32, True)]
        user.compute_depth_metrics_batched(gt.double(), pred.double(), valid)        # not float32: the replaced function
        user.compute_depth_metrics_batched(gt, pred, valid.float())                  # not a bool mask
        assert [c[:3] for c in calls[1:]] == [("depth", "cuda", torch.float64), ("depth", "cuda", torch.float32)]
        del calls[:]
        x = torch.rand((6, 3, 64, 64), generator=_gen(28)).to(gpu)
        y = torch.rand((6, 3, 64, 64), generator=_gen(29)).to(gpu)
        p = user.compute_psnr(x, y)
        assert not calls and torch.equal(p, metrics.compute_psnr(x, y))
        _check_psnr(y, x, p)
        assert user.compute_psnr(x.cpu(), y.cpu()).tolist() == [-2.0] * 6 and calls == [("psnr", "cpu")]
        user.compute_psnr(x[0], y[0])                                                # not 4-D: the replaced function
        assert calls[1:] == [("psnr", "cuda")]
    finally:
        plugin.DEPTH_METRICS_SEAM.restore()
        plugin.PSNR_SEAM.restore()
    assert dmod.compute_depth_metrics_batched is replaced_depth and user.compute_psnr is replaced_psnr
