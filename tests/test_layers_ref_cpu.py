"""The references of tests/_layers_ref.py, checked without a GPU: the max-pool routing transcription equals torch's CPU
autograd, the nearest-index rule equals torch's, and fp32 emulations of the GroupNorm and unfold kernels' arithmetic sit
inside the bounds tests/test_gpu_layers.py asserts (so the references alone do not use those bounds up)."""
import numpy as np
import pytest
import torch

import _layers_ref as R


@pytest.mark.parametrize("shape", R.POOL_BWD_SHAPES + [(2, 12, 11, 4)], ids=str)
def test_maxpool_routing_rule_equals_torch_cpu_autograd(shape):
    B, H, W, C = shape
    s, dpool = R.pool_bwd_inputs(shape, seed=11)
    ref = R.maxpool_bwd_relu_ref(s, dpool)
    got = R.maxpool_bwd_relu_rule(s.permute(0, 2, 3, 1).numpy(), dpool.permute(0, 2, 3, 1).numpy())
    assert torch.equal(torch.from_numpy(got).double().permute(0, 3, 1, 2), ref)
    # the inputs do what they are built for: ties inside windows, zero plateaus, and sums that are exact in fp32
    assert float((s == 0).float().mean()) > 0.2 and len(torch.unique(s)) <= 9
    assert torch.equal(ref.float().double(), ref)


def test_maxpool_forward_reference_shapes():
    for B, H, W, C in R.POOL_SHAPES:
        x = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(0))
        assert tuple(R.maxpool_ref(x).shape) == (B, C, R.pool_out(H), R.pool_out(W))


@pytest.mark.parametrize("pair", R.NEAREST_PAIRS, ids=str)
def test_nearest_index_rule_equals_torch(pair):
    out_size, in_size = pair
    assert np.array_equal(R.nearest_index_rule(out_size, in_size), R.nearest_index_torch(out_size, in_size))


def test_nearest_pairs_cover_every_upsample_geometry():
    assert len(R.NEAREST_PAIRS) >= 13
    for (ho, wo), (hi, wi), _ in R.UPSAMPLE_GEOMS:
        assert (ho, hi) in R.NEAREST_PAIRS and (wo, wi) in R.NEAREST_PAIRS


def test_upsample_backward_reference_is_the_scatter_of_the_index_rule():
    g = torch.Generator().manual_seed(3)
    for (ho, wo), (hi, wi), _ in R.UPSAMPLE_GEOMS[2:]:
        dd = torch.randint(-64, 65, (2, 4, ho, wo), generator=g).double() / 64
        want = torch.zeros(2, 4, hi, wi, dtype=torch.float64)
        iy, ix = R.nearest_index_rule(ho, hi), R.nearest_index_rule(wo, wi)
        for oy in range(ho):
            for ox in range(wo):
                want[:, :, iy[oy], ix[ox]] += dd[:, :, oy, ox]
        assert torch.equal(R.upsample_bwd_ref(dd, (hi, wi)), want)


def test_stem_wgrad_reference_against_autograd():
    g = torch.Generator().manual_seed(4)
    img = torch.randn(1, 3, 9, 13, generator=g)
    ds = torch.randn(35, 64, generator=g) * (torch.rand(35, 64, generator=g) > 0.5)
    w = torch.zeros(64, 3, 7, 7, dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.conv2d(img.double(), w, stride=2, padding=3)
    gw, = torch.autograd.grad(y, w, R.unrows(ds.double(), 1, 5, 7))
    ref, db = R.stem_wgrad_ref(img, ds)
    assert R.rel_err(ref, gw.permute(0, 2, 3, 1).reshape(64, 49, 3)) < 1e-14
    assert torch.equal(db, ds.double().sum(0))


@pytest.mark.parametrize("name", sorted(R.FOLD_ENTRIES))
def test_unfold_formulas_in_fp32_sit_inside_the_bounds(name):
    """torch fp32 of the kernel's formulas against the fp64 autograd reference: dw <= 1.6e-7, dgamma <= 7.5e-8 of the summed
    magnitude, db <= 6.4e-8 were measured on these entries -- 6-13x inside the asserted 1e-6."""
    e = R.fold_entry(name)
    figs = R.check_unfold(R.unfold_formulas_fp32(e), R.unfold_ref(e), name)
    assert max(figs.values()) < 5e-7, figs


@pytest.mark.parametrize("name", sorted(R.FOLD_ENTRIES))
def test_fold_formulas_in_fp32_sit_inside_the_bounds(name):
    """fp32 fold (sqrt, divide, two multiplies, each within an ulp) within 2^-21 of the fp64 reference element by element; its
    bf16 rounding within 2^-8"""
    e = R.fold_entry(name)
    wf, wft, bias_f = R.fold_ref(e)
    wf32, bias32, _ = R.fold_formulas(e, dtype=torch.float32)
    assert bool(((wf32.double() - wf).abs() <= 2.0 ** -21 * wf.abs()).all())
    assert bool(((wf32.bfloat16().double() - wf).abs() <= 2.0 ** -8 * wf.abs()).all())
    assert torch.equal(wft, wf.permute(2, 1, 0))
    assert R.rel_err(bias32, bias_f) < 1e-6 if e["scaling"] else not bool(bias_f.any())


# ---------------------------------------------------------------------- GroupNorm: fp32 emulation of the kernels
def _gn_emulate(z, gamma, beta, dy, hw, B, relu=True, bf16=False):
    """The GroupNorm kernels' arithmetic in fp32: one-pass moments (fp32 partial sums per 64-pixel chunk, combined in fp64),
    fp32 apply, one rounding to the storage type; backward alike.  Returns (y, stats, dz, dgamma, dbeta)."""
    f = torch.float32
    z, dy = z.to(f), dy.to(f)
    y, dz, stats = torch.empty_like(z), torch.empty_like(z), []
    dgamma, dbeta = torch.zeros(256, dtype=f), torch.zeros(256, dtype=f)
    r = 0
    for h, w in hw:
        for n in range(B):
            zi, di = z[r:r + h * w].view(h * w, 32, 8), dy[r:r + h * w].view(h * w, 32, 8)
            chunks = [slice(p, min(p + 64, h * w)) for p in range(0, h * w, 64)]
            s = sum(zi[c].sum((0, 2)).double() for c in chunks)
            ss = sum((zi[c] * zi[c]).sum((0, 2)).double() for c in chunks)
            cnt = float(h * w * 8)
            mean = s / cnt
            rstd = (1.0 / torch.sqrt((ss / cnt - mean * mean).clamp_min(0) + R.GN_EPS)).to(f)
            mean = mean.to(f)
            stats.append(torch.stack([mean, rstd], 1))
            xh = (zi - mean[None, :, None]) * rstd[None, :, None]
            pre = xh * gamma.view(1, 32, 8) + beta.view(1, 32, 8)
            y[r:r + h * w] = (pre.clamp_min(0) if relu else pre).reshape(h * w, 256)
            d = torch.where(pre <= 0, torch.zeros((), dtype=f), di) if relu else di
            a = d * gamma.view(1, 32, 8)
            m1 = (sum(a[c].sum((0, 2)).double() for c in chunks) / cnt).to(f)
            m2 = (sum((a[c] * xh[c]).sum((0, 2)).double() for c in chunks) / cnt).to(f)
            dz[r:r + h * w] = (rstd[None, :, None] * (a - m1[None, :, None] - xh * m2[None, :, None])).reshape(h * w, 256)
            dgamma += (d * xh).sum(0).reshape(256)
            dbeta += d.sum(0).reshape(256)
            r += h * w
    if bf16:
        y, dz = y.bfloat16(), dz.bfloat16()
    return y, torch.stack(stats), dz, dgamma, dbeta


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("levels", [R.GN_SET1, R.GN_SET2], ids=["set1", "set2"])
def test_groupnorm_emulation_sits_inside_the_bounds(levels, bf16):
    """What test_gpu_layers asserts of the kernels, asserted of an fp32 emulation of them: the references and the bounds fit
    together.  Measured: the bf16 outputs exceed the 2^-8 |ref| rounding part by 5.4e-9 (y) and 1.3e-10 (dz) of the
    maximum, against the 1e-5 allowed; no ReLU decision differs from fp64's on either level set."""
    hw, B = levels
    z, gamma, beta, dy = R.gn_inputs(hw, B, seed=21 + len(hw), bf16=bf16)
    y, stats, dz, dgamma, dbeta = _gn_emulate(z, gamma, beta, dy, hw, B, bf16=bf16)
    pre, stats_ref = R.gn_fwd_ref(z, gamma, beta, hw, B)
    ref = pre.clamp_min(0)
    assert R.rel_err(stats[..., 0], stats_ref[..., 0]) < 1e-5 and R.rel_err(stats[..., 1], stats_ref[..., 1]) < 1e-5
    assert R.check_gn_knife_edges(pre, y) == 0
    dz_ref, dg_ref, db_ref = R.gn_bwd_ref(z, gamma, beta, dy, (y > 0), hw, B)
    if bf16:
        assert R.bf16_excess(y, ref) <= 1e-7 and R.bf16_excess(dz, dz_ref) <= 1e-7
    else:
        r = 0
        for h, w in hw:
            sl = slice(r, r + B * h * w)
            assert R.rel_err(y[sl], ref[sl]) < 1e-5 and R.rel_err(dz[sl], dz_ref[sl]) < 2e-5
            r += B * h * w
    assert R.rel_err(dgamma, dg_ref) < 2e-5 and R.rel_err(dbeta, db_ref) < 2e-5


def test_groupnorm_level_sets_reach_the_multi_chunk_paths():
    hw, B = R.GN_SET2
    per_image = [-(-h * w // 64) for h, w in hw]
    assert per_image == [34, 9, 1] and (19 * 27) % 64 == 1          # more than 8 chunks per image; the 9th holds one pixel
    assert B * sum(per_image) == 132                                # more than 128 chunks: the parameter reduction's second round
    hw1, B1 = R.GN_SET1
    assert max(h * w for h, w in hw1) > 64 and R.gn_rows(hw1, B1) == 2 * (117 + 35 + 9 + 2 + 1)
