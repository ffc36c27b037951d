"""Plain torch / numpy references for the layer kernels of radet_amd/csrc/layers.hip (tests/test_gpu_layers.py compares
the kernels with them, tests/test_layers_ref_cpu.py checks them without a GPU).  Nothing here imports the GPU side:
every function takes and returns CPU tensors / arrays, and the arithmetic is fp64 unless a function says otherwise."""
import numpy as np
import torch
import torch.nn.functional as F

# ---------------------------------------------------------------------- layouts


def rows(x):
    """NCHW -> [B*H*W, C] (the kernels' NHWC row layout)"""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def unrows(r, B, H, W):
    """[B*H*W, C] -> NCHW"""
    return r.reshape(B, H, W, -1).permute(0, 3, 1, 2)


# ---------------------------------------------------------------------- max-pool 3x3 / 2, pad 1
POOL_SHAPES = [(2, 35, 45, 64), (1, 8, 6, 64), (3, 1, 5, 8), (1, 2, 1, 4)]                          # (B, H, W, C)
POOL_BWD_SHAPES = [(2, 7, 9, 64), (1, 8, 6, 4), (3, 1, 5, 4), (1, 2, 1, 4), (1, 1, 1, 4)]
POOL_BWD_LARGE = (2, 257, 256, 64)          # 2 105 344 float4 items: more than 8192 blocks x 256 threads


def pool_out(n):
    return (n - 1) // 2 + 1


def maxpool_ref(x_nchw):
    return F.max_pool2d(x_nchw, 3, 2, 1)


def pool_bwd_inputs(shape, seed):
    """s = relu(randint(-4, 9) / 4) (ties inside windows and zero plateaus everywhere), dpool = randint(-64, 65) / 64 (every
    fp32 sum of at most four of them is exact), both NCHW fp32"""
    B, H, W, C = shape
    g = torch.Generator().manual_seed(seed)
    s = torch.relu(torch.randint(-4, 9, (B, C, H, W), generator=g).float() * 0.25)
    dpool = torch.randint(-64, 65, (B, C, pool_out(H), pool_out(W)), generator=g).float() / 64
    return s, dpool


def maxpool_bwd_relu_ref(s_nchw, dpool_nchw):
    """[s > 0] * (torch CPU autograd of max_pool2d(s, 3, 2, 1)), fp64 -> NCHW fp64"""
    assert s_nchw.device.type == "cpu"           # the CPU backend's tie rule is the contract
    s = s_nchw.double().requires_grad_(True)
    g, = torch.autograd.grad(F.max_pool2d(s, 3, 2, 1), s, dpool_nchw.double())
    return g * (s_nchw > 0)


def maxpool_bwd_relu_rule(s_nhwc, dpool_nhwc):
    """The routing rule of maxpool_bwd_relu_kernel, transcribed line for line (fp32 numpy, [B, H, W, C] arrays): an element
    receives dpool of every window that contains it and whose FIRST maximum in row-major scan order over the window's
    in-range taps it is -- earlier taps must be strictly smaller, later ones smaller or equal."""
    s, dpool = np.asarray(s_nhwc, np.float32), np.asarray(dpool_nhwc, np.float32)
    B, H, W, C = s.shape
    Ho, Wo = pool_out(H), pool_out(W)
    ds = np.zeros_like(s)
    for y in range(H):
        for x in range(W):
            v = s[:, y, x, :]
            g = np.zeros_like(v)
            for oy in range(y >> 1, min((y + 1) >> 1, Ho - 1) + 1):
                for ox in range(x >> 1, min((x + 1) >> 1, Wo - 1) + 1):
                    seen, first = False, np.ones(v.shape, bool)
                    for r in range(3):
                        iy = oy * 2 - 1 + r
                        if iy < 0 or iy >= H:
                            continue
                        for q in range(3):
                            ix = ox * 2 - 1 + q
                            if ix < 0 or ix >= W:
                                continue
                            if iy == y and ix == x:
                                seen = True
                                continue
                            u = s[:, iy, ix, :]
                            first &= (u <= v) if seen else (u < v)
                    g = np.where(first, g + dpool[:, oy, ox, :], g)
            ds[:, y, x, :] = np.where(v > 0, g, np.float32(0))
    return ds


# ---------------------------------------------------------------------- nearest upsample-add
UPSAMPLE_GEOMS = [((60, 80), (30, 40), 4), ((100, 100), (50, 50), 2), ((15, 20), (8, 10), 2), ((7, 9), (3, 4), 2),
                  ((33, 33), (17, 17), 2), ((5, 5), (5, 5), 2), ((1, 1), (1, 1), 2)]       # (Ho, Wo), (Hi, Wi), B
NEAREST_PAIRS = sorted({(o, i) for (ho, wo), (hi, wi), _ in UPSAMPLE_GEOMS for o, i in ((ho, hi), (wo, wi))}
                       | {(13, 7), (25, 13), (4, 3), (200, 67), (11, 11)})                 # (out, in)


def nearest_index_rule(out_size, in_size):
    """the kernel's source index per destination index: floorf(dst * ((float)in / (float)out)), clamped to in - 1"""
    scale = np.float32(in_size) / np.float32(out_size)
    idx = np.floor(np.arange(out_size, dtype=np.float32) * scale).astype(np.int64)
    return np.minimum(idx, in_size - 1)


def nearest_index_torch(out_size, in_size):
    src = torch.arange(in_size, dtype=torch.float64).view(1, 1, in_size, 1)
    return F.interpolate(src, size=(out_size, 1), mode="nearest").view(-1).long().numpy()


def upsample_ref(src_nchw, size):
    return F.interpolate(src_nchw, size=size, mode="nearest")


def upsample_bwd_ref(ddst_nchw, in_size):
    """fp64 autograd of the nearest upsampling: the sum of ddst over the destination pixels that read each source pixel"""
    B, Cc = ddst_nchw.shape[:2]
    src = torch.zeros(B, Cc, *in_size, dtype=torch.float64, requires_grad=True)
    g, = torch.autograd.grad(F.interpolate(src, size=tuple(ddst_nchw.shape[2:]), mode="nearest"), src, ddst_nchw.double())
    return g


# ---------------------------------------------------------------------- stem weight gradient
def stem_wgrad_ref(img, ds_rows):
    """fp64 weight gradient of the 7x7 / 2 / pad 3 stem conv laid out [64][49][3], and the column sums of ds"""
    B, _, H, W = img.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    ds = unrows(ds_rows.double(), B, Ho, Wo).contiguous()
    gw = torch.nn.grad.conv2d_weight(img.double(), (64, 3, 7, 7), ds, stride=2, padding=3)
    return gw.permute(0, 2, 3, 1).reshape(64, 49, 3).contiguous(), ds_rows.double().sum(0)


# ---------------------------------------------------------------------- fold / unfold
# name -> (cout, cin, k, nsplit, scaling).  scaling: "bn", "bias" (plain conv bias) or None.  The stem entry's nsplit is the
# split count of its weight-gradient launch (7 at (2, 70, 90)).
FOLD_ENTRIES = {"a": (64, 3, 7, 7, "bn"), "b": (8, 512, 3, 5, "bn"), "c": (40, 256, 1, 1, "bias"), "d": (21, 64, 3, 8, None),
                "e": (8, 2048, 1, 3, "bn")}
FOLD_EPS = 1e-5


def fold_entry(name, seed=0):
    """fp32 parameters, weight-gradient slabs [S][cout][k*k][cin] and bias partials [S][cout] of one table entry"""
    cout, cin, k, S, scaling = FOLD_ENTRIES[name]
    g = torch.Generator().manual_seed(1000 + 17 * seed + ord(name))
    e = dict(name=name, cout=cout, cin=cin, k=k, nsplit=S, scaling=scaling,
             w=torch.randn(cout, cin, k, k, generator=g) * 0.1,
             slabs=torch.randn(S, cout, k * k, cin, generator=g), partials=torch.randn(S, cout, generator=g))
    if scaling == "bn":
        e.update(gamma=torch.rand(cout, generator=g) + 0.5, beta=torch.randn(cout, generator=g) * 0.3,
                 mean=torch.randn(cout, generator=g), var=torch.rand(cout, generator=g) + 0.5)
    elif scaling == "bias":
        e.update(bias=torch.randn(cout, generator=g))
    return e


def fold_formulas(e, dtype=torch.float64, grad=False):
    """(wf [o][t][c], bias_f [o], leaves) in `dtype` from the entry's fp32 parameters:
    s = gamma / sqrt(var + eps); wf = s * w; bias_f = beta - mean * s | conv bias | 0"""
    w = e["w"].to(dtype).requires_grad_(grad)
    leaves = dict(w=w)
    if e["scaling"] == "bn":
        gamma, beta = e["gamma"].to(dtype).requires_grad_(grad), e["beta"].to(dtype).requires_grad_(grad)
        s = gamma / torch.sqrt(e["var"].to(dtype) + FOLD_EPS)
        bias_f = beta - e["mean"].to(dtype) * s
        leaves.update(gamma=gamma, beta=beta)
    else:
        s = torch.ones(e["cout"], dtype=dtype)
        if e["scaling"] == "bias":
            bias_f = e["bias"].to(dtype).requires_grad_(grad)
            leaves.update(bias=bias_f)
        else:
            bias_f = torch.zeros(e["cout"], dtype=dtype)
    wf = (w * s[:, None, None, None]).permute(0, 2, 3, 1).reshape(e["cout"], e["k"] ** 2, e["cin"])
    return wf, bias_f, leaves


def fold_ref(e):
    """fp64 (wf [o][t][c], wft [c][t][o], bias_f [o])"""
    wf, bias_f, _ = fold_formulas(e)
    return wf, wf.permute(2, 1, 0).contiguous(), bias_f


def unfold_ref(e, slabs=None, partials=None):
    """fp64 autograd of L = <wf(w, gamma), G> + <bias_f(gamma, beta), db>, G / db = the fp64 sums of the slabs / partials:
    dict(dw [OIHW], dgamma, dbeta | dbias) plus `gmag`, the per-channel magnitude rstd * (sum |G w| + |db mean|) of what
    dgamma sums (the value itself cancels)"""
    G = (e["slabs"] if slabs is None else slabs).double().sum(0)
    db = (e["partials"] if partials is None else partials).double().sum(0)
    wf, bias_f, leaves = fold_formulas(e, grad=True)
    L = (wf * G).sum()
    if bias_f.requires_grad:
        L = L + (bias_f * db).sum()
    names = list(leaves)
    out = dict(zip(("d" + n for n in names), torch.autograd.grad(L, [leaves[n] for n in names])))
    if e["scaling"] == "bn":
        rstd = 1.0 / torch.sqrt(e["var"].double() + FOLD_EPS)
        w_ohwi = e["w"].double().permute(0, 2, 3, 1).reshape(e["cout"], e["k"] ** 2, e["cin"])
        out["gmag"] = rstd * ((G * w_ohwi).abs().sum((1, 2)) + (db * e["mean"].double()).abs())
    return out


def unfold_formulas_fp32(e):
    """the kernel's formulas in torch fp32 (another summation order than the kernel's): what a correct fp32 implementation
    reaches against unfold_ref"""
    G, db = e["slabs"].sum(0), e["partials"].sum(0)
    w_ohwi = e["w"].permute(0, 2, 3, 1).reshape(e["cout"], e["k"] ** 2, e["cin"])
    out = {}
    if e["scaling"] == "bn":
        rstd = 1.0 / torch.sqrt(e["var"] + np.float32(FOLD_EPS))
        s = e["gamma"] * rstd
        out["dgamma"] = rstd * ((G * w_ohwi).sum((1, 2)) - db * e["mean"])
        out["dbeta"] = db
    else:
        s = torch.ones(e["cout"])
        if e["scaling"] == "bias":
            out["dbias"] = db
    out["dw"] = (G * s[:, None, None]).reshape(e["cout"], e["k"], e["k"], e["cin"]).permute(0, 3, 1, 2).contiguous()
    return out


def check_unfold(got, ref, tag=""):
    """the unfold bounds: dw and dbeta / dbias rel_err < 1e-6, dgamma per channel within 1e-6 of the summed magnitude.
    Returns the three figures (each as a fraction of its bound's scale)."""
    def rel(a, b):
        return float((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-12))
    figs = dict(dw=rel(got["dw"], ref["dw"]))
    assert figs["dw"] < 1e-6, (tag, figs)
    for n in ("dbeta", "dbias"):
        if n in ref:
            figs["db"] = rel(got[n], ref[n])
            assert figs["db"] < 1e-6, (tag, figs)
    if "dgamma" in ref:
        figs["dgamma"] = float(((got["dgamma"].double() - ref["dgamma"]).abs() / ref["gmag"]).max())
        assert figs["dgamma"] <= 1e-6, (tag, figs)
    return figs


# ---------------------------------------------------------------------- GroupNorm(32) + ReLU over row-concatenated levels
GN_SET1 = ([(9, 13), (5, 7), (3, 3), (2, 1), (1, 1)], 2)
GN_SET2 = ([(45, 47), (19, 27), (1, 1)], 3)      # 34 + 9 chunks per image (the 9th of (19, 27) holds 1 pixel), 132 chunks in all
GN_EPS = 1e-5


def gn_rows(hw, B):
    return sum(B * h * w for h, w in hw)


def gn_inputs(hw, B, seed, bf16=False):
    """z = randn * 2 + 0.5, gamma in [0.5, 1.5], beta = 0.3 randn, dy = randn; z / dy as rows [sum B h w, 256], rounded to bf16
    when the kernel stores bf16 (the reference then reads exactly those values)"""
    g = torch.Generator().manual_seed(seed)
    R = gn_rows(hw, B)
    z = torch.randn(R, 256, generator=g) * 2 + 0.5
    gamma, beta = torch.rand(256, generator=g) + 0.5, torch.randn(256, generator=g) * 0.3
    dy = torch.randn(R, 256, generator=g)
    if bf16:
        z, dy = z.bfloat16(), dy.bfloat16()
    return z, gamma, beta, dy


def gn_levels(t_rows, hw, B):
    """rows [sum B h w, 256] -> list of NCHW tensors, one per level"""
    out, r = [], 0
    for h, w in hw:
        out.append(unrows(t_rows[r:r + B * h * w], B, h, w))
        r += B * h * w
    return out


def gn_unlevels(ts):
    return torch.cat([rows(t) for t in ts])


def gn_fwd_ref(z_rows, gamma, beta, hw, B):
    """fp64 F.group_norm of every level (before the ReLU) as rows, and the statistics [(level, image)][32][2] = (mean, rstd)"""
    pre, stats = [], []
    for z in gn_levels(z_rows.double(), hw, B):
        pre.append(F.group_norm(z, 32, gamma.double(), beta.double(), GN_EPS))
        zg = z.reshape(B, 32, -1)
        stats.append(torch.stack([zg.mean(2), 1.0 / torch.sqrt(zg.var(2, unbiased=False) + GN_EPS)], 2))
    return gn_unlevels(pre), torch.cat(stats).reshape(-1, 32, 2)


def gn_bwd_ref(z_rows, gamma, beta, dy_rows, mask_rows, hw, B):
    """fp64 autograd of mask * group_norm(z) (mask: the ReLU's discrete part, taken from the kernel's forward output; None
    without ReLU) -> (dz rows, dgamma, dbeta)"""
    zs = [z.contiguous().requires_grad_(True) for z in gn_levels(z_rows.double(), hw, B)]
    gm, bt = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    ys = [F.group_norm(z, 32, gm, bt, GN_EPS) for z in zs]
    if mask_rows is not None:
        ys = [y * m for y, m in zip(ys, gn_levels(mask_rows.double(), hw, B))]
    grads = torch.autograd.grad(ys, zs + [gm, bt], [d.contiguous() for d in gn_levels(dy_rows.double(), hw, B)])
    return gn_unlevels(grads[:-2]), grads[-2], grads[-1]


def gn_knife_edges(pre_ref, y_kernel):
    """elements whose ReLU decision differs between the fp64 reference and the kernel's forward output: their count and
    the largest |pre-activation| among them as a fraction of max |pre-activation| (0 when there are none)"""
    flip = (pre_ref > 0) != (y_kernel.double() > 0)
    n = int(flip.sum())
    return n, (float(pre_ref[flip].abs().max() / pre_ref.abs().max()) if n else 0.0)


def check_gn_knife_edges(pre_ref, y_kernel):
    n, worst = gn_knife_edges(pre_ref, y_kernel)
    assert n <= 8 and worst <= 2e-6, (n, worst)
    return n


def bf16_excess(got, ref):
    """largest excess of |got - ref| over the rounding part 2^-8 |ref| of the bf16 bound, as a fraction of max |ref|; the
    bound |got - ref| <= 2^-8 |ref| + 1e-5 max |ref| holds when this is <= 1e-5"""
    got, ref = got.double(), ref.double()
    return float(((got - ref).abs() - ref.abs() * 2.0 ** -8).max() / ref.abs().max().clamp_min(1e-300))


def rel_err(a, b):
    """the rel_err of test_gpu_kernels (largest error over largest reference magnitude), repeated here only so that the CPU test
    file need not import a GPU test module"""
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))
