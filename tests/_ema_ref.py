"""Shared by tests/test_ema_cpu.py and tests/test_gpu_ema.py: the yardstick of the EMA arithmetic (torch's CPU
`ema.mul_(1 - m).add_(param, alpha=m)`), its NumPy restatement, the momenta and the inputs both files use."""
import numpy as np
import torch

# mmcv's default, its third power (interval = 3), two warm-up values ((1 + it) / (warm_up + it) at (100, 0) and (100, 37)), 1/2
MOMENTA = (0.0002, 0.0002 ** 3, 1 / 100, 38 / 137, 0.5)


def inputs(n, seed):
    """(ema, param): finite normal fp32 values over a few binades, with +0 and -0 sprinkled into both (every sign pairing)"""
    g = torch.Generator().manual_seed(seed)
    ema = torch.randn(n, generator=g) * torch.exp2(torch.randint(-6, 7, (n,), generator=g).float())
    p = torch.randn(n, generator=g) * torch.exp2(torch.randint(-6, 7, (n,), generator=g).float())
    pairs = [(0.0, None), (-0.0, None), (None, 0.0), (None, -0.0), (0.0, 0.0), (0.0, -0.0), (-0.0, 0.0), (-0.0, -0.0)]
    for j, (e, q) in enumerate(pairs):              # at n < 8 the later pairs overwrite the earlier ones
        i = (j * 5) % n
        if e is not None:
            ema[i] = e
        if q is not None:
            p[i] = q
    assert bool(torch.isfinite(ema).all() and torch.isfinite(p).all())
    tiny = torch.finfo(torch.float32).tiny
    assert bool((((ema.abs() >= tiny) | (ema == 0)) & ((p.abs() >= tiny) | (p == 0))).all())
    return ema, p


def torch_ema(ema, p, m):
    """the yardstick: mmcv EMAHook's line on CPU tensors; m is a Python float.  Returns a new tensor."""
    assert ema.device.type == "cpu" and p.device.type == "cpu"
    return ema.clone().mul_(1 - m).add_(p, alpha=m)


def numpy_ema(ema, p, m):
    """t = fl32(ema * fl32(1 - m)); ema' = fma(fl32(m), p, t) with ONE rounding.  The fma is done in fp64: the product of two
    fp32 values is exact there (48 significant bits), the sum with t is rounded to odd (a TwoSum gives the rounding error of
    the fp64 addition; a non-zero error sets the sticky last bit), and 53 >= 2 * 24 + 2 bits make the final rounding of that
    to fp32 the rounding of the exact value."""
    ema, p = np.asarray(ema, np.float32), np.asarray(p, np.float32)
    m32, om32 = np.float32(m), np.float32(1 - m)
    t = (ema * om32).astype(np.float32)
    a = m32.astype(np.float64) * p.astype(np.float64)          # exact
    b = t.astype(np.float64)
    s = a + b
    bb = s - a
    err = (a - (s - bb)) + (b - bb)                            # TwoSum: a + b = s + err exactly
    even = (s.view(np.int64) & 1) == 0
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where((err != 0) & even, np.nextafter(s, toward), s)
    return s.astype(np.float32)


def bits(x):
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return np.ascontiguousarray(x, np.float32).view(np.uint32)
