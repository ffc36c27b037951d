"""Direct parity tests of the memory-bound layer kernels (radet_amd/csrc/layers.hip), each called through its wrapper in
radet_amd/kernels.py and compared with a CPU reference (tests/_layers_ref.py, checked on its own by
tests/test_layers_ref_cpu.py) computed in fp64 from exactly the values the kernel reads (bf16 cases: inputs rounded first).

kernel                               reference                                      bound
maxpool fp32 / bf16                  F.max_pool2d(x, 3, 2, 1)                       bit equal (a max has no rounding)
maxpool, y's amax slot               |y| of the same                                slot == max |y| exactly; never lowered
maxpool yq= (plane pairs)            the fp32 output y                              |err| <= 2^-22 |ref| + 2^-36 bound; yq.amax = x's slot
maxpool_bwd_relu                     [s > 0] * torch CPU fp64 autograd of the pool  bit equal (sums of <= 4 exact terms)
stem_wgrad                           nn.grad.conv2d_weight fp64, column sums of ds  rel_err < 1e-5; two runs bit identical
fold_weights w16 = 0                 s w, beta - mean s in fp64                     |err| <= 2^-21 |ref| per element
fold_weights w16 = 1 (bf16)          same                                           |err| <= 2^-8 |ref| per element
unfold_grads                         fp64 autograd of <wf, G> + <bias_f, db>        dw, db rel_err < 1e-6; dgamma 1e-6 of the summed magnitude
relu_bwd fp32 / bf16                 (dy + addend) * (act > 0) in fp32 (rounded)    bit equal (zeros +0.0); slot == max |dx| exactly
upsample_add fp32 / bf16             dst + F.interpolate(nearest), torch CPU        equal (bf16: one rounding of the fp32 sum)
upsample_add_bwd fp32 / bf16         base + fp64 autograd of the same               rel_err < 1e-6 / equal to the bf16 rounding (exact sums)
upsample_add(_bwd), amax slot        |output|                                       slot == max exactly; never lowered
gn_relu_fwd fp32 / bf16              F.group_norm fp64 + ReLU                       rel_err < 1e-5 per level / 2^-8 |ref| + 1e-5 max |ref|; stats 1e-5
gn_relu_bwd fp32 / bf16              fp64 autograd, ReLU mask of the kernel's y     rel_err < 2e-5 per level / 2^-8 |ref| + 1e-5 max |ref|; dgamma, dbeta 2e-5
nchw_to_nhwc / nhwc_to_nchw          torch permute                                  bit equal (bf16: one rounding); slot == max |x|
absmax (behind nchw_to_nhwc)         max |x|                                        slot == max exactly for any element count; never lowered
stem, y's amax slot                  |y| of its own output                          slot == max |y| exactly
gn_relu_fwd / _bwd output forms      two single launches / the fp32-only call       bit equal; planes vs fp32: equal (triples), pair rule
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import _layers_ref as R
from test_gpu_kernels import from_rows, rel_err, to_rows

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def K():
    from radet_amd import kernels
    return kernels


def _bits(v):
    return int(torch.tensor(float(v), dtype=torch.float32).view(torch.int32))


class _Slot:
    """an amax slot registered on tensor t for the length of a `with` block; `preset` fills every word with that float first"""

    def __init__(self, K, t, preset=None):
        self.K, self.t = K, t
        self.slot = K.new_amax(t.device)
        if preset is not None:
            self.slot.fill_(_bits(preset))

    def __enter__(self):
        self.key = self.K.register_amax(self.t, self.slot)
        return self

    def __exit__(self, *exc):
        self.K.unregister_amax([self.key])

    @property
    def value(self):
        return self.K.amax_value(self.slot)


def _pairs_close(K, planes, ref):
    """the close() rule of test_plane_pair_outputs_of_groupnorm_and_fold"""
    got = planes.to_float()
    bound = K.amax_value(planes.amax)
    assert bound >= float(ref.abs().max()), (bound, float(ref.abs().max()))
    tol = ref.abs() * 2.0 ** -22 + bound * 2.0 ** -36
    assert bool(((got - ref).abs() <= tol).all()), float(((got - ref).abs() / tol).max())


# ---------------------------------------------------------------------- 1. max-pool forward
def _pool_input(shape, seed, negative_corner=False):
    B, H, W, Cc = shape
    x = torch.randn(B, Cc, H, W, generator=torch.Generator().manual_seed(seed))
    if negative_corner:
        # the window of the last output pixel of the last image holds only large negative values: the largest |y| is a
        # negative element, in the last pixel of the last image
        y0, x0 = max(2 * (R.pool_out(H) - 1) - 1, 0), max(2 * (R.pool_out(W) - 1) - 1, 0)
        x[B - 1, :, y0:, x0:] = -50.0 - x[B - 1, :, y0:, x0:].abs()
    return x


@pytest.mark.parametrize("shape", R.POOL_SHAPES, ids=str)
def test_maxpool_fp32_and_bf16_bit_equal(K, shape):
    B, H, W, Cc = shape
    Ho, Wo = R.pool_out(H), R.pool_out(W)
    x = _pool_input(shape, 31)
    y = torch.empty(B * Ho * Wo, Cc, device=DEV)
    K.maxpool(to_rows(x).to(DEV), y, B, H, W, Cc)
    assert torch.equal(from_rows(y.cpu(), B, Ho, Wo), R.maxpool_ref(x))
    xh = x.bfloat16()
    yh = torch.empty(B * Ho * Wo, Cc, device=DEV, dtype=torch.bfloat16)
    K.maxpool(to_rows(xh).to(DEV), yh, B, H, W, Cc)
    assert torch.equal(from_rows(yh.cpu(), B, Ho, Wo), R.maxpool_ref(xh.float()).bfloat16())


@pytest.mark.parametrize("shape", R.POOL_SHAPES, ids=str)
def test_maxpool_amax_slot(K, shape):
    B, H, W, Cc = shape
    Ho, Wo = R.pool_out(H), R.pool_out(W)
    x = _pool_input(shape, 32, negative_corner=True)
    ref = R.maxpool_ref(x)
    big = float(ref.abs().max())
    assert big >= 50.0 and float(ref[B - 1, :, Ho - 1, Wo - 1].min()) == -big      # negative, last pixel of the last image
    xr = to_rows(x).to(DEV)
    y = torch.empty(B * Ho * Wo, Cc, device=DEV)
    with _Slot(K, y) as s:
        K.maxpool(xr, y, B, H, W, Cc)
        assert torch.equal(from_rows(y.cpu(), B, Ho, Wo), ref)
        assert s.value == big
    with _Slot(K, y, preset=1000.0) as s:            # "The slot is NOT reset here"
        K.maxpool(xr, y, B, H, W, Cc)
        assert s.value == 1000.0


@pytest.mark.parametrize("shape", [s for s in R.POOL_SHAPES if s[3] % 32 == 0], ids=str)
def test_maxpool_plane_pair_copy(K, shape):
    B, H, W, Cc = shape
    Ho, Wo = R.pool_out(H), R.pool_out(W)
    x = _pool_input(shape, 33, negative_corner=True)
    xr = to_rows(x).to(DEV)
    y = torch.empty(B * Ho * Wo, Cc, device=DEV)
    yq = K.Planes(B * Ho * Wo, Cc, device=DEV, kind="h2")
    with _Slot(K, xr) as sx, _Slot(K, y) as sy:
        K.absmax(xr, sx.slot)
        K.maxpool(xr, y, B, H, W, Cc, yq=yq)
        assert torch.equal(from_rows(y.cpu(), B, Ho, Wo), R.maxpool_ref(x))
        assert sy.value == float(y.abs().max())
        assert sx.value == float(x.abs().max())
        assert int(yq.amax.max()) == int(sx.slot.max())                 # the bits of x's slot
    _pairs_close(K, yq, y)


# ---------------------------------------------------------------------- 2. max-pool backward fused with the stem ReLU
@pytest.mark.parametrize("shape", R.POOL_BWD_SHAPES + [R.POOL_BWD_LARGE], ids=str)
def test_maxpool_bwd_relu_bit_equal_to_torch_cpu_autograd(K, shape):
    B, H, W, Cc = shape
    s, dpool = R.pool_bwd_inputs(shape, seed=41)
    ref = R.maxpool_bwd_relu_ref(s, dpool)
    ds = torch.full((B * H * W, Cc), float("nan"), device=DEV)
    K.maxpool_bwd_relu(to_rows(s).to(DEV), to_rows(dpool).to(DEV), ds, B, H, W, Cc)
    assert torch.equal(from_rows(ds.cpu(), B, H, W).double(), ref)


# ---------------------------------------------------------------------- 3. stem weight gradient, fold / unfold
def _stem_wgrad_run(K, B, H, W, S, seed):
    g = torch.Generator().manual_seed(seed)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    img = torch.randn(B, 3, H, W, generator=g)
    ds = torch.randn(B * Ho * Wo, 64, generator=g) * (torch.rand(B * Ho * Wo, 64, generator=g) > 0.5)
    out = []
    for _ in range(2):
        slabs = torch.full((S, 64, 49, 3), float("nan"), device=DEV)
        bp = torch.full((S, 64), float("nan"), device=DEV)
        K.stem_wgrad(img.to(DEV), ds.to(DEV), slabs, bp, B, H, W, S)
        out.append((slabs.cpu(), bp.cpu()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])       # deterministic
    return img, ds, out[0][0], out[0][1]


@pytest.fixture(scope="module")
def stem_case(K):
    """the (2, 70, 90) stem weight-gradient launch: 3150 pixels = 197 chunks of 16, S = 7 splits of 29 chunks, ragged last split"""
    B, H, W = 2, 70, 90
    S = K.stem_wgrad_splits(B, H, W)
    assert S == 7
    return _stem_wgrad_run(K, B, H, W, S, seed=51)


def _check_stem_wgrad(img, ds, slabs, bp):
    gw, db = R.stem_wgrad_ref(img, ds)
    assert bool(torch.isfinite(slabs).all()) and bool(torch.isfinite(bp).all())
    assert rel_err(slabs.double().sum(0), gw) < 1e-5
    assert rel_err(bp.double().sum(0), db) < 1e-5


def test_stem_wgrad_ragged_splits(stem_case):
    _check_stem_wgrad(*stem_case)


@pytest.mark.parametrize("S", [1, 4])
def test_stem_wgrad_small_image_and_empty_split(K, S):
    """(1, 9, 13): 35 pixels = 3 chunks.  S = 4: the fourth split owns no pixel and writes zeros over the NaN prefill."""
    img, ds, slabs, bp = _stem_wgrad_run(K, 1, 9, 13, S, seed=52)
    _check_stem_wgrad(img, ds, slabs, bp)
    if S == 4:
        assert not bool(slabs[3].any()) and not bool(bp[3].any())


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _build_table(entries, w16):
    """one RadetConvDesc table over `entries` (dicts of R.fold_entry plus options wft_ld / wft_off / no_dw); every device
    buffer is kept in the entry under "dev".  Output buffers are pre-filled with NaN."""
    from radet_amd import _lib
    arr = (_lib.RadetConvDesc * len(entries))()
    wdt = torch.bfloat16 if w16 else torch.float32
    nan = float("nan")
    for d, e in zip(arr, entries):
        cout, cin, kt = e["cout"], e["cin"], e["k"] ** 2
        ld = e.get("wft_ld", 0) or cout
        b = e["dev"] = {n: e[n].to(DEV).contiguous() for n in ("w", "slabs", "partials", "gamma", "beta", "mean", "var", "bias") if n in e}
        b.update(wf=torch.full((cout, kt, cin), nan, device=DEV, dtype=wdt), wft=torch.full((cin * kt, ld), nan, device=DEV, dtype=wdt),
                 bias_f=torch.full((cout,), nan, device=DEV), dw=torch.full((cout, cin, e["k"], e["k"]), nan, device=DEV),
                 dgamma=torch.full((cout,), nan, device=DEV), dbeta=torch.full((cout,), nan, device=DEV),
                 dbias=torch.full((cout,), nan, device=DEV))
        d.w, d.bias = _ptr(b["w"]), _ptr(b.get("bias"))
        d.bn_gamma, d.bn_beta, d.bn_mean, d.bn_var = (_ptr(b.get(n)) for n in ("gamma", "beta", "mean", "var"))
        d.wf, d.wft, d.bias_f = _ptr(b["wf"]), _ptr(b["wft"]), _ptr(b["bias_f"])
        d.dwf_slabs, d.dbias_partials = _ptr(b["slabs"]), _ptr(b["partials"])
        d.dw = None if e.get("no_dw") else _ptr(b["dw"])
        d.dgamma, d.dbeta = _ptr(b["dgamma"]), _ptr(b["dbeta"])
        d.dbias = _ptr(b["dbias"]) if e["scaling"] == "bias" else None
        d.cout, d.cin, d.kh, d.kw, d.nsplit, d.eps = cout, cin, e["k"], e["k"], e["nsplit"], R.FOLD_EPS
        d.wft_ld, d.wft_off, d.w16 = e.get("wft_ld", 0), e.get("wft_off", 0), w16
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)


def _fold_entries(stem_case):
    """the five table entries; the stem entry is fed with the stem weight-gradient launch's slabs and bias partials, the 1 x 1
    bias entry writes its transposed copy into rows of 64 at column 16.  (The chaining is wanted: unfold reduces what the stem
    launch wrote.  A failure of stem_wgrad therefore also shows as errors of the fold / unfold tests, through `stem_case`.)"""
    entries = [R.fold_entry(n) for n in sorted(R.FOLD_ENTRIES)]
    _, _, slabs, bp = stem_case
    assert entries[0]["name"] == "a" and tuple(slabs.shape) == (entries[0]["nsplit"], 64, 49, 3)
    entries[0].update(slabs=slabs, partials=bp)
    entries[2].update(wft_ld=64, wft_off=16)
    return entries


@pytest.mark.parametrize("w16", [0, 1], ids=["fp32", "bf16"])
def test_fold_weights_against_fp64(K, stem_case, w16):
    entries = _fold_entries(stem_case)
    table = _build_table(entries, w16)
    K.fold_weights(table, len(entries))
    tol = 2.0 ** -8 if w16 else 2.0 ** -21
    for e in entries:
        wf, wft, bias_f = R.fold_ref(e)
        b = {n: t.cpu() for n, t in e["dev"].items()}
        got = b["wf"].double()
        assert bool(((got - wf).abs() <= tol * wf.abs()).all()), (e["name"], float(((got - wf).abs() / wf.abs()).max()))
        off, cout = e.get("wft_off", 0), e["cout"]
        got_t = b["wft"].double().view(e["cin"], e["k"] ** 2, -1)
        assert bool(((got_t[..., off:off + cout] - wft).abs() <= tol * wft.abs()).all()), e["name"]
        assert torch.equal(got_t[..., off:off + cout], got.permute(2, 1, 0))              # "the same value"
        pad = torch.ones(got_t.shape[-1], dtype=torch.bool)
        pad[off:off + cout] = False
        assert bool(torch.isnan(got_t[..., pad]).all()), e["name"]                        # the padding columns are not written
        if e["scaling"] == "bn":
            assert rel_err(b["bias_f"], bias_f) < 1e-6, e["name"]
        else:
            assert torch.equal(b["bias_f"].double(), bias_f), e["name"]                   # the conv bias, or 0


def test_unfold_grads_against_fp64_autograd(K, stem_case):
    entries = _fold_entries(stem_case)
    skipped = dict(R.fold_entry("e", seed=1), no_dw=True)                                  # dw = NULL: the entry is skipped
    entries.append(skipped)
    table = _build_table(entries, 0)
    K.unfold_grads(table, len(entries), max(e["cout"] for e in entries))
    for e in entries[:-1]:
        b = {n: t.cpu() for n, t in e["dev"].items()}
        ref = R.unfold_ref(e)
        got = dict(dw=b["dw"])
        if e["scaling"] == "bn":
            got.update(dgamma=b["dgamma"], dbeta=b["dbeta"])
        else:
            assert bool(torch.isnan(b["dgamma"]).all()) and bool(torch.isnan(b["dbeta"]).all()), e["name"]   # untouched without BN
            if e["scaling"] == "bias":
                got.update(dbias=b["dbias"])
        assert all(bool(torch.isfinite(t).all()) for t in got.values()), e["name"]
        R.check_unfold(got, ref, e["name"])
    for n in ("dw", "dgamma", "dbeta"):
        assert bool(torch.isnan(skipped["dev"][n]).all()), n


# ---------------------------------------------------------------------- 4. ReLU backward
RELU_SIZES = [4, 4100, 4 * (4096 * 256 + 257)]         # the last: more float4 items than 4096 blocks x 256 threads, and a tail


def _relu_inputs(n, seed):
    g = torch.Generator().manual_seed(seed)
    dy, addend, act = (torch.randn(n, generator=g) for _ in range(3))
    act[0::7] = 0.0
    act[1::11] = -0.0
    act[2::13] = -act[2::13].abs()
    act[n - 2] = 1.5
    act[n - 1] = -0.0
    act[1] = 0.0
    dy[1], addend[1] = -500.0, -250.0                  # the largest |dy + addend|, where act <= 0: must not count
    dy[n - 2], addend[n - 2] = 40.0, 37.0              # the true maximum, in the stride loop's tail
    return dy, addend, act


@pytest.mark.parametrize("with_addend", [False, True], ids=["plain", "addend"])
@pytest.mark.parametrize("n", RELU_SIZES)
def test_relu_bwd_fp32_and_amax(K, n, with_addend):
    dy, addend, act = _relu_inputs(n, 61)
    ref = ((dy + addend) if with_addend else dy) * (act > 0) + 0.0     # (+ 0.0: the product's -0.0 where act <= 0 is the kernel's +0.0)
    dx = torch.full((n,), float("nan"), device=DEV)
    with _Slot(K, dx) as s:
        K.relu_bwd(dy.to(DEV), addend.to(DEV) if with_addend else None, act.to(DEV), dx)
        assert torch.equal(dx.cpu().view(torch.int32), ref.view(torch.int32))            # bit for bit
        assert s.value == float(ref.abs().max()) == (77.0 if with_addend else 40.0)
    with _Slot(K, dx, preset=1000.0) as s:
        K.relu_bwd(dy.to(DEV), addend.to(DEV) if with_addend else None, act.to(DEV), dx)
        assert s.value == 1000.0


@pytest.mark.parametrize("with_addend", [False, True], ids=["plain", "addend"])
@pytest.mark.parametrize("n", RELU_SIZES)
def test_relu_bwd_bf16(K, n, with_addend):
    dy, addend, act = (t.bfloat16() for t in _relu_inputs(n, 62))
    ref = (((dy.float() + addend.float()) if with_addend else dy.float()) * (act > 0) + 0.0).bfloat16()
    dx = torch.full((n,), float("nan"), device=DEV, dtype=torch.bfloat16)
    K.relu_bwd(dy.to(DEV), addend.to(DEV) if with_addend else None, act.to(DEV), dx)
    assert torch.equal(dx.cpu().view(torch.int16), ref.view(torch.int16))                # bit for bit


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_relu_bwd_rejects_a_length_that_is_no_multiple_of_four(K, dtype):
    from radet_amd import _lib
    t = torch.zeros(6, device=DEV, dtype=dtype)
    with pytest.raises(_lib.RadetHipError):
        K.relu_bwd(t, None, t, torch.empty_like(t))


# ---------------------------------------------------------------------- 5. upsample-add
def _upsample_case(geom, seed, exact=False):
    (ho, wo), (hi, wi), B = geom
    g = torch.Generator().manual_seed(seed)

    def draw(*shape):
        if exact:                                      # multiples of 1/64: bf16 values whose fp32 sums are exact
            return torch.randint(-64, 65, shape, generator=g).float() / 64
        return torch.randn(*shape, generator=g)
    return dict(B=B, ho=ho, wo=wo, hi=hi, wi=wi, dst=draw(B, 256, ho, wo), src=draw(B, 256, hi, wi), ddst=draw(B, 256, ho, wo),
                base=draw(B, 256, hi, wi))


@pytest.mark.parametrize("geom", R.UPSAMPLE_GEOMS, ids=str)
def test_upsample_add_fp32_and_amax(K, geom):
    c = _upsample_case(geom, 71)
    B, ho, wo, hi, wi = (c[n] for n in ("B", "ho", "wo", "hi", "wi"))
    ref = c["dst"] + R.upsample_ref(c["src"], (ho, wo))
    src = to_rows(c["src"]).to(DEV)
    d = to_rows(c["dst"]).to(DEV)
    with _Slot(K, d) as s:
        K.upsample_add(d, src, B, ho, wo, hi, wi, 256)
        assert torch.equal(from_rows(d.cpu(), B, ho, wo), ref)
        assert s.value == float(ref.abs().max())
    with _Slot(K, d, preset=1000.0) as s:
        K.upsample_add(d, src, B, ho, wo, hi, wi, 256)
        assert s.value == 1000.0
    ref_b = c["base"].double() + R.upsample_bwd_ref(c["ddst"], (hi, wi))
    ds = to_rows(c["base"]).to(DEV)
    with _Slot(K, ds) as s:
        K.upsample_add_bwd(ds, to_rows(c["ddst"]).to(DEV), B, ho, wo, hi, wi, 256)
        assert rel_err(from_rows(ds, B, hi, wi), ref_b) < 1e-6
        assert s.value == float(ds.abs().max())
    with _Slot(K, ds, preset=1000.0) as s:
        K.upsample_add_bwd(ds, to_rows(c["ddst"]).to(DEV), B, ho, wo, hi, wi, 256)
        assert s.value == 1000.0


@pytest.mark.parametrize("geom", R.UPSAMPLE_GEOMS, ids=str)
def test_upsample_add_bf16(K, geom):
    c = _upsample_case(geom, 72)
    B, ho, wo, hi, wi = (c[n] for n in ("B", "ho", "wo", "hi", "wi"))
    dst, src = c["dst"].bfloat16(), c["src"].bfloat16()
    ref = (dst.float() + R.upsample_ref(src.float(), (ho, wo))).bfloat16()
    d = to_rows(dst).to(DEV)
    K.upsample_add(d, to_rows(src).to(DEV), B, ho, wo, hi, wi, 256)
    assert torch.equal(from_rows(d.cpu(), B, ho, wo), ref)
    c = _upsample_case(geom, 73, exact=True)
    ddst, base = c["ddst"].bfloat16(), c["base"].bfloat16()
    assert torch.equal(ddst.float(), c["ddst"]) and torch.equal(base.float(), c["base"])
    ref_b = (base.double() + R.upsample_bwd_ref(ddst.float(), (hi, wi))).bfloat16()
    ds = to_rows(base).to(DEV)
    K.upsample_add_bwd(ds, to_rows(ddst).to(DEV), B, ho, wo, hi, wi, 256)
    assert torch.equal(from_rows(ds.cpu(), B, hi, wi), ref_b)


# ---------------------------------------------------------------------- 6. GroupNorm + ReLU
def _gn_run(K, levels, bf16, relu, seed):
    hw, B = levels
    lv = K.Levels(hw, B)
    z, gamma, beta, dy = R.gn_inputs(hw, B, seed, bf16=bf16)
    assert lv.rows == z.shape[0]
    zd, dyd, gm, bt = z.to(DEV), dy.to(DEV), gamma.to(DEV), beta.to(DEV)
    y = torch.empty_like(zd)
    stats = torch.full((len(hw) * B * 64,), float("nan"), device=DEV)
    ws = torch.empty(K.gn_ws_floats(lv), device=DEV)
    K.gn_relu_fwd(lv, K.GnFwd(zd, gm, bt, stats, ws, y=y), relu=relu)
    dz = torch.empty_like(zd)
    dg, db = torch.full((256,), float("nan"), device=DEV), torch.full((256,), float("nan"), device=DEV)
    K.gn_relu_bwd(lv, dyd, zd, stats, gm, bt, dg, db, ws, dz=dz, relu=relu)
    assert y.dtype == dz.dtype == (torch.bfloat16 if bf16 else torch.float32)
    return z, gamma, beta, dy, y.cpu(), stats.cpu().view(-1, 32, 2), dz.cpu(), dg.cpu(), db.cpu()


def _gn_check(K, levels, bf16, relu, seed):
    hw, B = levels
    z, gamma, beta, dy, y, stats, dz, dg, db = _gn_run(K, levels, bf16, relu, seed)
    pre, stats_ref = R.gn_fwd_ref(z, gamma, beta, hw, B)
    ref = pre.clamp_min(0) if relu else pre
    assert rel_err(stats[..., 0], stats_ref[..., 0]) < 1e-5 and rel_err(stats[..., 1], stats_ref[..., 1]) < 1e-5
    mask = None
    if relu:
        # the discrete part is taken out: the reference uses the kernel's own ReLU decisions, which may differ from fp64's
        # only on knife edges
        R.check_gn_knife_edges(pre, y)
        mask = y > 0
    dz_ref, dg_ref, db_ref = R.gn_bwd_ref(z, gamma, beta, dy, mask, hw, B)
    if bf16:
        assert R.bf16_excess(y, ref) <= 1e-5, R.bf16_excess(y, ref)
        assert R.bf16_excess(dz, dz_ref) <= 1e-5, R.bf16_excess(dz, dz_ref)
    else:
        r = 0
        for h, w in hw:
            sl = slice(r, r + B * h * w)
            assert rel_err(y[sl], ref[sl]) < 1e-5, (h, w)
            assert rel_err(dz[sl], dz_ref[sl]) < 2e-5, (h, w)
            r += B * h * w
    assert rel_err(dg, dg_ref) < 2e-5 and rel_err(db, db_ref) < 2e-5


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("levels", [R.GN_SET1, R.GN_SET2], ids=["set1", "set2"])
def test_groupnorm_relu_fwd_bwd_against_fp64(K, levels, bf16):
    _gn_check(K, levels, bf16, True, seed=21 + len(levels[0]))


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_groupnorm_without_relu_against_fp64(K, bf16):
    _gn_check(K, R.GN_SET1, bf16, False, seed=81)


# ---------------------------------------------------------------------- 7. layout helpers, stem amax
LAYOUT_SHAPES = [(2, 3, 9, 13), (1, 21, 5, 7), (2, 256, 4, 5), (1, 3, 800, 900)]      # the last: more elements than 8192 blocks x 256


@pytest.mark.parametrize("shape", LAYOUT_SHAPES, ids=str)
def test_layout_helpers_are_exact_permutes(K, shape):
    B, Cc, H, W = shape
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(91))
    xd = x.to(DEV)
    y = torch.full((B * H * W, Cc), float("nan"), device=DEV)
    K.nchw_to_nhwc(xd, y, B, Cc, H, W)
    assert torch.equal(y.cpu(), to_rows(x))
    back = torch.full(shape, float("nan"), device=DEV)
    K.nhwc_to_nchw(y, back, B, Cc, H, W)
    assert torch.equal(back.cpu(), x)
    yh = torch.empty(B * H * W, Cc, device=DEV, dtype=torch.bfloat16)                # through the fp32 staging + convert_rows
    K.nchw_to_nhwc(xd, yh, B, Cc, H, W)
    assert torch.equal(yh.cpu(), to_rows(x).bfloat16())
    back.fill_(float("nan"))
    K.nhwc_to_nchw(yh, back, B, Cc, H, W)                                              # bf16 source: exact
    assert torch.equal(back.cpu(), x.bfloat16().float())


@pytest.mark.parametrize("shape", LAYOUT_SHAPES, ids=str)
def test_nchw_to_nhwc_raises_the_destination_slot(K, shape):
    """The largest magnitude is the LAST element of the destination: at 702 and 735 elements it sits in the n % 4 floats behind
    the float4 part of the stand-alone absmax pass (the wrapper used to skip the pass for such sizes and left the slot stale)."""
    B, Cc, H, W = shape
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(92))
    x[B - 1, Cc - 1, H - 1, W - 1] = -9.5
    y = torch.empty(B * H * W, Cc, device=DEV)
    with _Slot(K, y) as s:
        K.nchw_to_nhwc(x.to(DEV), y, B, Cc, H, W)
        assert s.value == float(x.abs().max()) == 9.5


@pytest.mark.parametrize("n", [1, 2, 3, 5, 4098, 4 * 2048 * 256 + 7])
def test_absmax_any_element_count(K, n):
    """radet_absmax over n floats with n % 4 != 0, n < 4 and more float4 items than its 2048 x 256 threads: the slot is raised to
    the exact maximum wherever it sits (first element, last float4, each tail position) and is never lowered"""
    x = torch.randn(n, generator=torch.Generator().manual_seed(94)).to(DEV)
    for pos in sorted({0, max(n - n % 4 - 1, 0)} | set(range(n - n % 4, n))):
        xx = x.clone()
        xx[pos] = -9.5
        slot = K.new_amax(DEV)
        K.absmax(xx, slot)
        assert K.amax_value(slot) == 9.5, pos
    slot = K.new_amax(DEV).fill_(_bits(1000.0))
    K.absmax(x, slot)
    assert K.amax_value(slot) == 1000.0


@pytest.mark.parametrize("size", [(2, 70, 90), (3, 9, 13)], ids=str)
def test_stem_amax_slot(K, size):
    B, H, W = size
    g = torch.Generator().manual_seed(93)
    img = torch.randn(B, 3, H, W, generator=g)
    w = torch.randn(64, 3, 7, 7, generator=g) * 0.1
    bias = torch.randn(64, generator=g)
    ref = F.relu(F.conv2d(img.double(), w.double(), bias.double(), stride=2, padding=3))
    Ho, Wo = ref.shape[2:]
    y = torch.empty(B * Ho * Wo, 64, device=DEV)
    with _Slot(K, y) as s:
        K.stem(img.to(DEV), w.permute(0, 2, 3, 1).contiguous().to(DEV), bias.to(DEV), y, B, H, W)
        assert rel_err(from_rows(y, B, Ho, Wo), ref) < 1e-5
        assert s.value == float(y.abs().max())


# ---------------------------------------------------------------------- 8. GroupNorm: every output form through the one entry point
GN_FORMS = dict(y=(True, None), b3=(False, "b3"), y_b3=(True, "b3"), h2=(False, "h2"), y_h2=(True, "h2"), bf16=(True, None))
NAN = float("nan")


def _same_bits(a, b):
    """bit for bit (NaN equals NaN, -0.0 differs from 0.0): tensors, or Planes by their plane tensors and bound slots"""
    if a is None or b is None:
        return a is None and b is None
    if hasattr(a, "kind"):
        return _same_bits(a.t, b.t) and _same_bits(a.amax, b.amax)
    w = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return a.dtype == b.dtype and torch.equal(a.view(w), b.view(w))


class _GnFwdOut:
    """fresh, NaN-filled outputs of one tensor of a forward launch in the given form, and the slots the launch may raise"""

    def __init__(self, K, lv, src, form):
        with_y, kind = GN_FORMS[form]
        self.z, self.gamma, self.beta = src
        fp32 = form != "bf16"
        if not fp32:
            self.z = self.z.bfloat16()
        self.stats = torch.full((len(lv) * lv.B * 64,), NAN, device=DEV)
        self.ws = torch.empty(K.gn_ws_floats(lv), device=DEV)
        self.y = torch.full_like(self.z, NAN) if with_y else None
        self.planes = K.Planes(lv.rows, 256, device=DEV, kind=kind) if kind else None
        if kind:
            self.planes.t.fill_(NAN)
        self.y_slot = K.new_amax(DEV) if with_y and fp32 else None
        self.zhat = K.new_amax(DEV) if fp32 else None

    def arg(self, K):
        return K.GnFwd(self.z, self.gamma, self.beta, self.stats, self.ws, y=self.y, planes=self.planes, zhat_amax=self.zhat)

    def same(self, o):
        return all(_same_bits(getattr(self, n), getattr(o, n)) for n in ("stats", "y", "planes", "y_slot", "zhat"))


def _gn_fwd_launch(K, lv, *outs):
    keys = [K.register_amax(o.y, o.y_slot) for o in outs if o.y_slot is not None]
    try:
        K.gn_relu_fwd(lv, *[o.arg(K) for o in outs])
    finally:
        K.unregister_amax(keys)


@pytest.fixture(scope="module")
def gn_forms_case(K):
    """R.GN_SET1 (crosses the chunk and the level boundaries), two tensors with different z / gamma / beta, and each one's fp32
    output from a single launch: the reference of every other form"""
    hw, B = R.GN_SET1
    lv = K.Levels(hw, B)
    z, gamma, beta, dy = (t.to(DEV) for t in R.gn_inputs(hw, B, 101))
    srcs = [(z, gamma, beta), (z * 0.7 - 0.2, gamma * 1.3, beta - 0.1)]
    refs = [_GnFwdOut(K, lv, s, "y") for s in srcs]
    for o in refs:
        _gn_fwd_launch(K, lv, o)
        assert bool(torch.isfinite(o.y).all()) and bool(torch.isfinite(o.stats).all())
    return lv, srcs, refs, dy


@pytest.mark.parametrize("form", list(GN_FORMS))
def test_groupnorm_fwd_output_forms_single_and_paired_launch(K, gn_forms_case, form):
    """Two single launches and one paired launch write the same bits: y, the planes, the statistics and every amax slot (the
    raised slot of y, the bound of the pairs, the zhat slot).  The planes against the fp32 y: equal for bf16 triples (the split is
    exact), the rule of test_plane_pair_outputs_of_groupnorm_and_fold for fp16 pairs."""
    lv, srcs, refs, _ = gn_forms_case
    single = [_GnFwdOut(K, lv, s, form) for s in srcs]
    for o in single:
        _gn_fwd_launch(K, lv, o)
    paired = [_GnFwdOut(K, lv, s, form) for s in srcs]
    _gn_fwd_launch(K, lv, *paired)
    for s, q, ref in zip(single, paired, refs):
        assert q.same(s)
        assert bool(torch.isfinite(q.stats).all()) and (q.y is None or bool(torch.isfinite(q.y.float()).all()))
        if form == "bf16":
            continue
        assert _same_bits(q.stats, ref.stats) and _same_bits(q.zhat, ref.zhat)
        if q.y is not None:
            assert _same_bits(q.y, ref.y) and K.amax_value(q.y_slot) == float(ref.y.abs().max())
        if q.planes is not None and q.planes.kind == "b3":
            assert torch.equal(q.planes.to_float(), ref.y)
        elif q.planes is not None:
            _pairs_close(K, q.planes, ref.y)


def test_groupnorm_bwd_output_forms(K, gn_forms_case):
    """dz as fp32, as bf16 triples and as fp16 pairs: dz, dgamma and dbeta of the fp32 + planes call are those of the fp32-only
    call bit for bit, the planes-only call writes the same planes, and the planes hold dz (triples: exactly; pairs: the pair rule)"""
    lv, srcs, refs, dy = gn_forms_case
    (z, gamma, beta), fwd = srcs[0], refs[0]

    def run(with_dz, kind):
        dz = torch.full_like(z, NAN) if with_dz else None
        planes = K.Planes(lv.rows, 256, device=DEV, kind=kind) if kind else None
        if kind:
            planes.t.fill_(NAN)
        dg, db = torch.full((256,), NAN, device=DEV), torch.full((256,), NAN, device=DEV)
        K.gn_relu_bwd(lv, dy, z, fwd.stats, gamma, beta, dg, db, fwd.ws, dz=dz, planes=planes, zhat_amax=fwd.zhat)
        return dz, planes, dg, db

    dz, _, dg, db = run(True, None)
    assert all(bool(torch.isfinite(t).all()) for t in (dz, dg, db))
    for kind in ("b3", "h2"):
        dz2, both, dg2, db2 = run(True, kind)
        assert _same_bits(dz2, dz) and _same_bits(dg2, dg) and _same_bits(db2, db)
        _, only, dg3, db3 = run(False, kind)
        assert _same_bits(only, both) and _same_bits(dg3, dg) and _same_bits(db3, db)
        if kind == "b3":
            assert torch.equal(both.to_float(), dz)
        else:
            _pairs_close(K, both, dz)
