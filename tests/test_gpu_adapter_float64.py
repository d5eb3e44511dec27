"""The adapter-tail kernels (s360_adapter.hip: k_adapter_fwd / k_adapter_bwd for d_sh in {1, 4, 9, 16}, k_adapter_fwd25 /
k_adapter_bwd25 for d_sh = 25) held to a float64 reference PER GAUSSIAN, at every path the kernels have.

Three evaluations of the same float32 inputs (built on the CPU from a seeded generator):
  * the kernels, through adapter.adapter_tail (values, and gradients from one backward of sum(out * cotangent));
  * oracle/adapter_ref.adapter_tail_torch in float64 on the CPU — the reference ("64");
  * adapter_tail_torch in float32 on the CPU — the yardstick: what a plain float32 evaluation of the same formulas loses.

Per-Gaussian error measures (G = the covariance cotangent, nine entries or the six of the cov6 layout; g_mean = the means'
cotangent, 0 where the means are detached).  Each denominator is the magnitude of the terms the result is summed from, so a
float32 evaluation lands at a small multiple of 2^-24 whatever cancels:
  covariances  |dSigma|_F / |Sigma64|_F            means      |d| / (depth + |t|)
  scales       max_k |ds_k| / s_k                  rotations  |dq^|
  harmonics    per colour and degree block, |d| / |block64|   (a block whose reference norm is 0 must be exactly 0)
  d_depths     |d| / (2 |G| |Sigma64| / depth + |g_mean|)
  d_raw scale  |d| / (2 |G| |Sigma64|)             d_raw quat |d| / (4 |G| |Sigma64| / (|q_raw| + eps))
  d_raw SH     per colour and degree block, |d| / (mask_l |g_harm block|)

The bound, for every quantity and every case: the kernels' worst per-Gaussian error <= 2 x the float32 yardstick's worst
error on the same inputs (the factor of tests/test_gpu_lazy_seam.py: a different operation order and the few-ulp expf / sinf /
cosf), no Gaussian left out, at least 1000 Gaussians per case.  Where the yardstick is exact the kernels must be too, bit for
bit: harmonics without SH rotation are float32(raw * mask), their gradient float32(g_harm * mask).

Cases (the smallest shapes that reach each path):
  1. d_sh = 25 with Gv = 135 (9 x 15): two full 64-Gaussian blocks and a tail of 7 per view; the odd Gv misaligns the raw /
     d_raw base (328 B per Gaussian) of odd views and the harmonics base (300 B) of every view but each fourth — the scalar
     staging and store branches and the float4 loops' remainders (525 = 4 * 131 + 1 harmonics floats, 574 = 4 * 143 + 2 d_raw
     floats in an aligned tail).  The congruences are asserted on data_ptr() of the buffers the kernels read and write.
  2. the generic kernels, d_sh in {1, 4, 9, 16}, Gv = 270 (one full 256-thread block + 14), per_ray = 2, one ERP convention each.
  3. per_ray in {2, 3} at d_sh = 25 (Gv = 105, odd, at per_ray = 3), and GaussianAdapterERP.forward with spp = 2.
  4. planted edge Gaussians (zero / 1e-6 / 1e3 / (0,0,0,1) quaternions, scale logits +-20, depths 1e-2 / 1e2) at every pixel of a
     4 x 8 panorama — pole rows included — in all four conventions: everything finite, same measures, same bound.
  5. structure: cov9 exactly symmetric, cov6 = its upper triangle bit for bit, detached means leave d_depths untouched.
  6. ownership through the C ABI: NaN-filled outputs between sentinel floats — no NaN left, no sentinel touched.

Measured on an MI355X (gfx950), worst per-Gaussian error over each case in units of 2^-24, kernels / float32 yardstick.  Every test
prints these "[adapter64]" lines itself (run with -s).  No margin has been raised: 2 x for every quantity; the worst ratio of a
case is 1.25 (d_raw quat, case 1), and harmonics / d_raw SH without SH rotation are bit-exact.  "planted" rows are the maxima over
the planted Gaussians of case 4 alone, for the record: the bound is the case's.
  case                                             cov       means      scales         rot        harm    d_depths     d_scale      d_quat        d_sh
  deg4 Gv=135 hm3d cov6=0 rot=1            12.15/12.79  3.18/3.18   4.12/3.90   1.99/1.99   2.70/2.70   5.73/5.59   2.92/3.13   5.70/4.55   2.91/3.11
  deg4 Gv=135 m3d cov6=1 rot=0             12.09/10.98  5.47/5.47   4.12/3.90   1.99/1.99   0.94/0.94   6.37/5.92   2.45/2.63   5.30/4.83   0.94/0.94
  generic d_sh=1 hm3d cov6=0 rot=1         12.34/13.63  3.61/3.13   4.11/4.03   2.16/2.16   0.00/0.00   5.67/6.03   3.66/3.66   4.74/4.78   0.00/0.00
  generic d_sh=4 m3d cov6=1 rot=0          13.16/13.00  5.62/5.62   4.16/4.16   2.35/2.35   0.94/0.94   7.68/8.69   3.35/3.02   4.55/4.56   0.93/0.93
  generic d_sh=9 residential cov6=0 rot=1  14.34/14.56  3.19/3.19   3.88/3.88   2.15/2.15   2.94/2.96   6.98/6.98   2.87/2.87   6.34/6.18   2.61/2.61
  generic d_sh=16 CoffeeArea cov6=1 rot=1  13.67/12.00  4.65/4.59   3.75/3.75   1.85/1.85   2.59/2.59   8.35/8.35   3.11/3.05   5.22/4.40   3.05/3.05
  deg4 per_ray=2 replica cov6=1            12.86/10.72  3.46/3.45   3.63/3.63   2.06/2.06   2.91/2.69   6.25/5.83   4.63/4.10   4.93/5.60   3.30/3.27
  deg4 per_ray=3 outdoor_colmap cov6=0     14.33/12.43  4.52/4.52   4.16/4.16   2.01/2.01   2.79/2.63   7.72/6.41   2.89/3.52   3.99/4.32   3.24/2.85
  module spp=2                             11.89/10.93  3.77/3.38   4.03/4.03   1.79/1.79   2.51/2.62   5.50/5.26   2.24/2.24   5.66/4.58   2.97/3.04
  edges hm3d cov6=0 rot=1                   9.24/9.18   3.34/3.42   3.00/3.00   2.01/2.01   2.97/2.86   4.30/4.30   2.90/2.90   3.82/4.03   3.09/2.99
  edges hm3d cov6=0 rot=1 planted           7.54/8.80   3.34/3.34   2.79/2.70   1.39/1.39   2.97/2.86   4.30/4.30   1.63/1.02   2.90/3.10   2.84/2.49
  edges m3d cov6=1 rot=1                    8.69/8.91   4.77/4.84   3.00/3.00   2.01/2.01   2.97/2.86   5.13/4.52   2.54/2.13   4.11/3.93   3.09/2.99
  edges m3d cov6=1 rot=1 planted            7.32/8.05   4.73/4.73   2.79/2.70   1.39/1.39   2.97/2.86   3.32/3.18   2.01/2.01   2.68/2.82   2.84/2.49
  edges residential cov6=0 rot=0            9.24/9.18   2.98/3.66   3.00/3.00   2.01/2.01   0.93/0.93   4.80/3.90   2.90/2.90   3.82/4.03   0.94/0.94
  edges residential cov6=0 rot=0 planted    7.54/8.80   2.89/3.22   2.79/2.70   1.39/1.39   0.91/0.91   4.80/3.89   1.63/1.02   2.90/3.10   0.92/0.92
  edges CoffeeArea cov6=1 rot=1             8.69/8.91   4.92/4.92   3.00/3.00   2.01/2.01   2.97/2.86   5.33/4.86   2.54/2.13   4.11/3.93   3.09/2.99
  edges CoffeeArea cov6=1 rot=1 planted     7.32/8.05   4.92/4.92   2.79/2.70   1.39/1.39   2.97/2.86   4.44/4.44   2.01/2.01   2.68/2.82   2.84/2.49
"""
import ctypes as C
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import adapter_ref
from splatter360_amd import _lib, adapter, synthetic

pytestmark = pytest.mark.gpu

SMIN, SMAX, EPS = 0.5, 15.0, 1e-8
U = 2.0 ** -24
MARGIN = 2.0
QUANTITIES = ("covariances", "means", "scales", "rotations", "harmonics", "d_depths", "d_raw_scale", "d_raw_quat", "d_raw_sh")
_TRIU = tuple(torch.triu_indices(3, 3))


@functools.lru_cache(maxsize=None)
def _inputs(seed, v, h, w, per_ray, d_sh, with_rot, edges=False):
    """CPU float32 inputs and cotangents.  Cached and shared: nobody writes into them."""
    rng = np.random.default_rng(seed)
    gv = h * w * per_ray
    ext = np.tile(np.eye(4, dtype=np.float32), (v, 1, 1))
    ext[:, :3, :3] = synthetic._random_rotations(rng, v)
    ext[:, :3, 3] = rng.uniform(-1, 1, (v, 3))
    dep = np.exp(rng.uniform(np.log(0.5), np.log(8.0), (v, gv))).astype(np.float32)
    raw = rng.standard_normal((v, gv, 7 + 3 * d_sh)).astype(np.float32)
    raw[..., :3] *= 3
    planted = None
    if edges:      # kind k of view i sits at Gaussian (i + 4 k) % gv: with v = gv every kind visits every pixel
        assert gv >= 32 and per_ray == 1
        planted = np.zeros((v, gv), dtype=bool)
        for i in range(v):
            planted[i, [(i + 4 * k) % gv for k in range(8)]] = True
            at = lambda k: (i + 4 * k) % gv
            unit = lambda k: raw[i, at(k), 3:7] / np.linalg.norm(raw[i, at(k), 3:7])
            raw[i, at(0), 3:7] = 0
            raw[i, at(1), 3:7] = unit(1) * np.float32(1e-6)
            raw[i, at(2), 3:7] = unit(2) * np.float32(1e3)
            raw[i, at(3), 3:7] = (0, 0, 0, 1)
            raw[i, at(4), :3] = 20
            raw[i, at(5), :3] = -20
            dep[i, at(6)] = 1e-2
            dep[i, at(7)] = 1e2
    rot = adapter_ref.wigner_blocks(ext[:, :3, :3], d_sh).astype(np.float32) if with_rot else None
    t = lambda a: None if a is None else torch.tensor(a)
    return SimpleNamespace(v=v, h=h, w=w, per_ray=per_ray, d_sh=d_sh, gv=gv, ext=t(ext), dep=t(dep), raw=t(raw), rot=t(rot), planted=t(planted),
                           opa=t(rng.uniform(0.05, 0.95, (v, gv)).astype(np.float32)),
                           wm=t(rng.standard_normal((v, gv, 3)).astype(np.float32)),
                           wc=t(rng.standard_normal((v, gv, 3, 3)).astype(np.float32)),
                           wh=t(rng.standard_normal((v, gv, 3, d_sh)).astype(np.float32)))


def _leaf(t, device=None, dtype=None):
    """A fresh leaf that requires grad; the shared input stays as it is."""
    return t.detach().to(device=device, dtype=dtype, copy=True).requires_grad_(True)


def _collect(out, d, rw, c, cov6, diff_means, cov_is_6):
    """One backward of sum(out * cotangent); everything as float64 CPU tensors (exact for float32 results)."""
    dev, dt = d.device, d.dtype
    wm, wc, wh = (x.to(dev, dt) for x in (c.wm, c.wc, c.wh))
    r_, c_ = _TRIU
    cov = out.covariances
    if cov6:    # the 6-entry layout reads the upper triangle only
        loss = ((cov if cov_is_6 else cov[:, :, r_, c_]) * wc[:, :, r_, c_]).sum()
    else:
        loss = (cov * wc).sum()
    loss = loss + (out.harmonics * wh).sum()
    assert out.means.requires_grad == diff_means
    if diff_means:
        loss = loss + (out.means * wm).sum()
    loss.backward()
    f = lambda x: x.detach().double().cpu()
    return SimpleNamespace(means=f(out.means), cov=f(cov), scales=f(out.scales), rot=f(out.rotations), harm=f(out.harmonics),
                           d_dep=f(d.grad), d_raw=f(rw.grad))


def _torch_eval(c, dtype, cov6, diff_means, name):
    d, rw = _leaf(c.dep, dtype=dtype), _leaf(c.raw, dtype=dtype)
    out = adapter_ref.adapter_tail_torch(c.ext.to(dtype), d, c.opa.to(dtype), rw, (c.h, c.w), SMIN, SMAX,
                                         sh_rotation=None if c.rot is None else c.rot.to(dtype), eps=EPS, per_ray=c.per_ray,
                                         differentiable_means=diff_means, dataset_name=name)
    return _collect(out, d, rw, c, cov6, diff_means, False)


@functools.lru_cache(maxsize=None)
def _torch_run(key, dtype, cov6, diff_means, name):
    """The CPU evaluation of a cached case, computed once and shared."""
    return _torch_eval(_inputs(*key), dtype, cov6, diff_means, name)


def _kernel_run(gpu, c, cov6, diff_means, name):
    d, rw = _leaf(c.dep, gpu), _leaf(c.raw, gpu)
    out = adapter.adapter_tail(c.ext.to(gpu), d, c.opa.to(gpu), rw, (c.h, c.w), SMIN, SMAX,
                               sh_rotation=None if c.rot is None else c.rot.to(gpu), eps=EPS, per_ray=c.per_ray, cov6=cov6,
                               differentiable_means=diff_means, dataset_name=name)
    res = _collect(out, d, rw, c, cov6, diff_means, cov6)
    res.ptr = SimpleNamespace(raw=rw.data_ptr(), harm=out.harmonics.data_ptr())   # the buffers the kernels themselves read / wrote
    return res


def _blocks(d_sh):
    return [(l * l, (l + 1) ** 2) for l in range(math.isqrt(d_sh))]


def _errors(got, ref, c, cov6, diff_means):
    """{quantity: [V, Gv] per-Gaussian error of `got` against the float64 `ref`} by the measures of the module docstring."""
    r_, c_ = _TRIU
    fro = lambda t: t.flatten(2).norm(dim=-1)
    dep = c.dep.double()
    sig = fro(ref.cov)
    gn = fro(c.wc.double()[:, :, r_, c_] if cov6 else c.wc.double())
    gm = c.wm.double().norm(dim=-1) if diff_means else torch.zeros_like(dep)
    mask = adapter_ref.sh_mask(c.d_sh).double()
    e = {}
    six = lambda t: t[:, :, r_, c_] if cov6 and t.dim() == 4 else t          # cov6: the six entries the layout holds
    e["covariances"] = fro(six(got.cov) - six(ref.cov)) / sig
    e["means"] = (got.means - ref.means).norm(dim=-1) / (dep + c.ext[:, :3, 3].double().norm(dim=-1)[:, None])
    e["scales"] = ((got.scales - ref.scales).abs() / ref.scales).amax(-1)
    e["rotations"] = (got.rot - ref.rot).norm(dim=-1)
    hs, gs = [], []
    for a, b in _blocks(c.d_sh):
        den = ref.harm[..., a:b].norm(dim=-1)                                     # [V, Gv, 3]
        num = (got.harm[..., a:b] - ref.harm[..., a:b]).norm(dim=-1)
        assert bool((num[den == 0] == 0).all()), "a harmonics block that is exactly 0 in the reference is not 0"
        hs.append(torch.where(den > 0, num / den.clamp_min(1e-300), torch.zeros_like(num)))
        den = mask[a] * c.wh.double()[..., a:b].norm(dim=-1)
        num = (got.d_raw[..., 7:] - ref.d_raw[..., 7:]).reshape(c.v, c.gv, 3, c.d_sh)[..., a:b].norm(dim=-1)
        assert bool((den > 0).all())
        gs.append(num / den)
    e["harmonics"] = torch.stack(hs, -1).flatten(2).amax(-1)
    e["d_raw_sh"] = torch.stack(gs, -1).flatten(2).amax(-1)
    e["d_depths"] = (got.d_dep - ref.d_dep).abs() / (2 * gn * sig / dep + gm)
    e["d_raw_scale"] = (got.d_raw[..., :3] - ref.d_raw[..., :3]).norm(dim=-1) / (2 * gn * sig)
    e["d_raw_quat"] = (got.d_raw[..., 3:7] - ref.d_raw[..., 3:7]).norm(dim=-1) / (4 * gn * sig / (c.raw[..., 3:7].double().norm(dim=-1) + EPS))
    return e


def _compare(got, ref, y32, c, cov6, diff_means, label):
    """`got` (the kernels) against float64 under the float32 yardstick: every quantity, every Gaussian."""
    assert c.v * c.gv >= 1000
    for k, t in vars(got).items():
        if k != "ptr":
            assert bool(torch.isfinite(t).all()), (label, k, "not finite")
    ek, ey = _errors(got, ref, c, cov6, diff_means), _errors(y32, ref, c, cov6, diff_means)
    bad = []
    for q in QUANTITIES:
        assert ek[q].shape == (c.v, c.gv) and bool(torch.isfinite(ek[q]).all()) and bool(torch.isfinite(ey[q]).all()), (label, q)
        k, y = ek[q].max().item(), ey[q].max().item()
        print(f"[adapter64] {label:<34} {q:<12} kernel {k / U:8.3f}  float32 {y / U:8.3f}  (x 2^-24)")
        if c.planted is not None:    # for the record: the planted Gaussians alone (the bound is the case's, above)
            print(f"[adapter64] {label + ' planted':<34} {q:<12} kernel {ek[q][c.planted].max().item() / U:8.3f}  "
                  f"float32 {ey[q][c.planted].max().item() / U:8.3f}  (x 2^-24)")
        if not k <= MARGIN * y:
            bad.append((q, k / U, y / U, int(ek[q].argmax())))
    assert not bad, (label, "kernel error above 2 x the float32 yardstick: (quantity, kernel, yardstick [2^-24], worst Gaussian)", bad)
    if c.rot is None:    # one float32 multiply each: exact
        m = adapter_ref.sh_mask(c.d_sh)
        assert torch.equal(got.harm.float(), c.raw[..., 7:].reshape(c.v, c.gv, 3, c.d_sh) * m)
        assert torch.equal(got.d_raw[..., 7:].float(), (c.wh * m).reshape(c.v, c.gv, -1))


def _check(gpu, key, cov6, diff_means, name, label):
    """One case through adapter.adapter_tail and _compare.  Returns the kernels' results."""
    c = _inputs(*key)
    got = _kernel_run(gpu, c, cov6, diff_means, name)
    _compare(got, _torch_run(key, torch.float64, cov6, diff_means, name), _torch_run(key, torch.float32, cov6, diff_means, name),
             c, cov6, diff_means, label)
    return got


# ------------------------------------------------------------------------------------------------ 1. misaligned d_sh = 25
@pytest.mark.parametrize("cov6,with_rot,diff_means,name", [(False, True, True, "hm3d"), (True, False, False, "m3d")])
def test_degree4_kernels_at_misaligned_views_and_remainders(gpu, cov6, with_rot, diff_means, name):
    """Gv = 135: views 0..3 (repeated as 4..7 to pass 1000 Gaussians) have raw / d_raw bases at 0, 8, 0, 8 and harmonics bases at
    0, 4, 8, 12 modulo 16; the 7-Gaussian tails leave float4 remainders of 1 (harmonics) and 2 (d_raw).  The congruences are asserted
    on the buffers the kernels themselves read and wrote (raw, harmonics).  d_raw reaches this test only as a .grad, which autograd
    may have copied: its base is asserted where the test owns the buffer, in test_kernels_write_all_of_their_outputs_and_nothing_else."""
    key = (101, 8, 9, 15, 1, 25, with_rot)
    got = _check(gpu, key, cov6, diff_means, name, f"deg4 Gv=135 {name} cov6={int(cov6)} rot={int(with_rot)}")
    gv = 135
    assert gv % 64 == 7 and (7 * 75) % 4 == 1 and (7 * 82) % 4 == 2
    assert [(got.ptr.raw + v * gv * 328) % 16 for v in range(4)] == [0, 8, 0, 8]
    assert [(got.ptr.harm + v * gv * 300) % 16 for v in range(4)] == [0, 4, 8, 12]


# ------------------------------------------------------------------------------------------------ 2. generic kernels
@pytest.mark.parametrize("d_sh,cov6,with_rot,diff_means,name", [(1, False, True, True, "hm3d"), (4, True, False, False, "m3d"),
                                                                 (9, False, True, False, "residential"), (16, True, True, True, "CoffeeArea")])
def test_generic_kernels_every_degree_below_four(gpu, d_sh, cov6, with_rot, diff_means, name):
    """k_adapter_fwd / k_adapter_bwd: Gv = 270 = one full 256-thread block + 14, per_ray = 2, V = 4."""
    _check(gpu, (102 + d_sh, 4, 9, 15, 2, d_sh, with_rot), cov6, diff_means, name, f"generic d_sh={d_sh} {name} cov6={int(cov6)} rot={int(with_rot)}")


# ------------------------------------------------------------------------------------------------ 3. per_ray at d_sh = 25
@pytest.mark.parametrize("per_ray,v,h,w,cov6,with_rot,diff_means,name", [(2, 4, 9, 15, True, True, True, "replica"),
                                                                          (3, 10, 5, 7, False, True, True, "outdoor_colmap")])
def test_degree4_kernels_with_several_gaussians_per_ray(gpu, per_ray, v, h, w, cov6, with_rot, diff_means, name):
    """The pixel of Gaussian g is g / per_ray (means and the means' part of d_depths); Gv = 105 is odd at per_ray = 3."""
    _check(gpu, (120 + per_ray, v, h, w, per_ray, 25, with_rot), cov6, diff_means, name, f"deg4 per_ray={per_ray} {name} cov6={int(cov6)}")


def test_module_forward_with_two_samples_per_pixel(gpu):
    """GaussianAdapterERP.forward passes per_ray = srf * spp: depths[b, v, r, 1, 2] against adapter_tail_torch(per_ray = 2), same
    measures and bound — and the documented broadcast layout raw_gaussians[b, v, r, srf, 1, c] gives the same bits."""
    v, h, w, spp = 4, 9, 15, 2
    key = (131, v, h, w, spp, 25, True)
    c0 = _inputs(*key)
    raw = c0.raw.reshape(v, h * w, spp, -1)[:, :, :1].expand(-1, -1, spp, -1).reshape(v, h * w * spp, -1).contiguous()  # one record per ray
    c = SimpleNamespace(**{**vars(c0), "raw": raw})
    ref, y32 = (_torch_eval(c, dt, False, True, "hm3d") for dt in (torch.float64, torch.float32))
    mod = adapter.GaussianAdapterERP(SMIN, SMAX, 4, sh_rotation=lambda r: c.rot.to(gpu), differentiable_means=True).to(gpu)
    sh5 = (1, v, h * w, 1, spp)

    def run(raw_in):
        d, rw = _leaf(c.dep.reshape(sh5), gpu), _leaf(raw_in, gpu)
        out = mod("hm3d", c.ext.to(gpu)[None, :, None, None, None], d, c.opa.to(gpu).reshape(sh5), rw, (h, w))
        assert out.means.shape == (*sh5, 3) and out.covariances.shape == (*sh5, 3, 3) and out.harmonics.shape == (*sh5, 3, 25)
        flat = SimpleNamespace(means=out.means.reshape(v, -1, 3), covariances=out.covariances.reshape(v, -1, 3, 3), scales=out.scales.reshape(v, -1, 3),
                               rotations=out.rotations.reshape(v, -1, 4), harmonics=out.harmonics.reshape(v, -1, 3, 25))
        res = _collect(flat, d, rw, c, False, True, False)
        res.d_dep = res.d_dep.reshape(v, -1)
        return res
    got = run(c.raw.reshape(*sh5, -1))
    got.d_raw = got.d_raw.reshape(v, h * w * spp, -1)
    _compare(got, ref, y32, c, False, True, "module spp=2")
    shared = run(c.raw.reshape(1, v, h * w, spp, -1)[:, :, :, None, :1])          # [b, v, r, srf, 1, c]
    for f in ("means", "cov", "scales", "rot", "harm", "d_dep"):
        assert torch.equal(getattr(shared, f), getattr(got, f)), f
    assert torch.equal(shared.d_raw.float().reshape(v, h * w, -1), got.d_raw.float().reshape(v, h * w, spp, -1).sum(2))


# ------------------------------------------------------------------------------------------------ 4. planted edge Gaussians
@pytest.mark.parametrize("name,cov6,with_rot,diff_means", [("hm3d", False, True, True), ("m3d", True, True, True),
                                                           ("residential", False, False, True), ("CoffeeArea", True, True, False)])
def test_edge_gaussians_stay_finite_and_within_the_bound(gpu, name, cov6, with_rot, diff_means):
    """32 views of a 4 x 8 panorama, eight planted Gaussians per view (see _inputs), each kind at every pixel once — the pole rows
    y = 0 and y = h - 1 of conventions 1-3 included.  The zero quaternion's gradient is exactly 0."""
    key = (140, 32, 4, 8, 1, 25, with_rot, True)
    got = _check(gpu, key, cov6, diff_means, name, f"edges {name} cov6={int(cov6)} rot={int(with_rot)}")
    c = _inputs(*key)
    zero_q = (c.raw[..., 3:7] == 0).all(-1)
    assert int(zero_q.sum()) == 32 and bool((got.d_raw[..., 3:7][zero_q] == 0).all())


# ------------------------------------------------------------------------------------------------ 5. structure
@pytest.mark.parametrize("d_sh,per_ray", [(25, 1), (9, 2)])
def test_covariance_layouts_and_detached_means(gpu, d_sh, per_ray):
    c = _inputs(150 + d_sh, 4, 9, 15, per_ray, d_sh, True)
    a9 = _kernel_run(gpu, c, False, False, "hm3d")
    a6 = _kernel_run(gpu, c, True, False, "hm3d")
    assert torch.equal(a9.cov, a9.cov.transpose(-1, -2))
    r_, c_ = _TRIU
    assert torch.equal(a6.cov, a9.cov[:, :, r_, c_])
    for f in ("means", "scales", "rot", "harm"):
        assert torch.equal(getattr(a6, f), getattr(a9, f)), f
    # detached means: d_depths is what a run gives whose means cotangent is ignored — the opt-in run with a zero cotangent
    d, rw = _leaf(c.dep, gpu), _leaf(c.raw, gpu)
    out = adapter.adapter_tail(c.ext.to(gpu), d, c.opa.to(gpu), rw, (c.h, c.w), SMIN, SMAX, sh_rotation=c.rot.to(gpu), eps=EPS,
                               per_ray=per_ray, differentiable_means=True)
    ((out.covariances * c.wc.to(gpu)).sum() + (out.harmonics * c.wh.to(gpu)).sum() + (out.means * 0.0).sum()).backward()
    assert torch.equal(d.grad.double().cpu(), a9.d_dep) and torch.equal(rw.grad.double().cpu(), a9.d_raw)
    # ... and differs from the run that does use it
    b9 = _kernel_run(gpu, c, False, True, "hm3d")
    assert not torch.equal(b9.d_dep, a9.d_dep) and torch.equal(b9.d_raw, a9.d_raw)


# ------------------------------------------------------------------------------------------------ 6. ownership
GUARD = 64
_SENTINEL = 12345.678


def _guarded(gpu, n):
    """n NaN floats between two runs of GUARD sentinel floats (256 B in front: the body keeps the allocation's alignment)."""
    buf = torch.full((n + 2 * GUARD,), _SENTINEL, dtype=torch.float32, device=gpu)
    buf[GUARD:GUARD + n] = float("nan")
    return buf


def _assert_owned(buf, n, what):
    b = buf.cpu()
    assert not bool(torch.isnan(b[GUARD:GUARD + n]).any()), (what, "an element was not written", int(torch.isnan(b[GUARD:GUARD + n]).sum()))
    s = torch.full((GUARD,), _SENTINEL, dtype=torch.float32)
    assert torch.equal(b[:GUARD], s) and torch.equal(b[GUARD + n:], s), (what, "a sentinel was overwritten")


@pytest.mark.parametrize("v,per_ray,d_sh,with_rot,cov6", [(8, 1, 25, True, False), (8, 1, 25, False, True), (4, 2, 9, True, False), (4, 2, 9, False, True)])
def test_kernels_write_all_of_their_outputs_and_nothing_else(gpu, v, per_ray, d_sh, with_rot, cov6):
    c = _inputs(160 + d_sh, v, 9, 15, per_ray, d_sh, with_rot)
    n = c.v * c.gv
    ci = 7 + 3 * d_sh
    ins = [x.to(gpu).contiguous() for x in (c.ext, c.dep, c.raw)]
    rot = None if c.rot is None else c.rot.to(gpu).contiguous()
    cots = [x.to(gpu).contiguous() for x in (c.wm, c.wc[:, :, _TRIU[0], _TRIU[1]] if cov6 else c.wc, c.wh)]
    sizes = {"means": 3 * n, "covariances": (6 if cov6 else 9) * n, "harmonics": 3 * d_sh * n, "scales": 3 * n, "rotations": 4 * n,
             "d_depths": n, "d_raw": ci * n}
    bufs = {k: _guarded(gpu, s) for k, s in sizes.items()}
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    body = lambda k: C.c_void_p(bufs[k].data_ptr() + 4 * GUARD)
    if d_sh == 25:     # case 1's alignment, on the very pointers the kernels get: the views' bases differ as there
        base = lambda ptr, stride: [(ptr + v_ * c.gv * stride) % 16 for v_ in range(4)]
        assert base(ins[2].data_ptr(), 328) == [0, 8, 0, 8] and base(body("d_raw").value, 328) == [0, 8, 0, 8]
        assert base(cots[2].data_ptr(), 300) == [0, 4, 8, 12] and base(body("harmonics").value, 300) == [0, 4, 8, 12]
    stream = C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    lib = _lib.lib()
    rc = lib.s360_adapter_forward(p(ins[0]), p(ins[1]), p(ins[2]), p(rot), c.v, c.gv, c.h, c.w, per_ray, d_sh, SMIN, SMAX, EPS,
                                  body("means"), body("covariances"), int(not cov6), body("harmonics"), body("scales"), body("rotations"), 0, stream)
    _lib.check(rc, "s360_adapter_forward")
    rc = lib.s360_adapter_backward(p(ins[0]), p(ins[1]), p(ins[2]), p(rot), c.v, c.gv, c.h, c.w, per_ray, d_sh, SMIN, SMAX, EPS,
                                   p(cots[0]), p(cots[1]), int(not cov6), p(cots[2]), body("d_depths"), body("d_raw"), 0, stream)
    _lib.check(rc, "s360_adapter_backward")
    torch.cuda.synchronize()
    for k, s in sizes.items():
        _assert_owned(bufs[k], s, k)
    # the same values as through the wrapper
    got = _kernel_run(gpu, c, cov6, True, "hm3d")
    for k, f in (("means", "means"), ("covariances", "cov"), ("harmonics", "harm"), ("scales", "scales"), ("rotations", "rot"),
                 ("d_depths", "d_dep"), ("d_raw", "d_raw")):
        assert torch.equal(bufs[k][GUARD:GUARD + sizes[k]].double().cpu(), getattr(got, f).reshape(-1)), k
