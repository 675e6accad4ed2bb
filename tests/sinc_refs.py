"""float64 yardstick of the windowed-sinc resampler (SPEC.md 4f), written with torch on the CPU: the FULL L-tap kernel of every
phase in float64 and conv1d with stride o, as torchaudio.functional.resample's _get_sinc_resample_kernel /
_apply_sinc_resample_kernel do it (restated from the definition; torchaudio is not a dependency).  Nothing here reads the code under
test: tests/test_resample_sinc_host.py and tests/test_gpu_resample_sinc.py compare against it.

The error bound of one output sample m (phase p, frame i), in float64:
    (S + 1) 2^-24 sum_j |K32[p][j] xpad[i o + j]|  +  L 2^-50 max|x|
The first term is the standard bound of a float32 sum of S products (it also covers fused multiply-adds); the second covers the
clamped taps the compact table drops.  S = 2 width + 2 bounds the run of every phase."""
import math
from functools import lru_cache

import numpy as np
import torch

BETA = 14.769656459379492

# (src, dst, lowpass_filter_width, rolloff) -> (o, n, width)
CASES = [
    ((44100, 48000, 64, 0.945), (147, 160, 68)),
    ((48000, 44100, 64, 0.945), (160, 147, 74)),
    ((48000, 32000, 64, 0.945), (3, 2, 102)),
    ((44100, 32000, 64, 0.945), (441, 320, 94)),
    ((44100, 16000, 6, 0.99), (441, 160, 17)),
    ((16000, 48000, 6, 0.99), (1, 3, 7)),
    ((8000, 8001, 6, 0.99), (8000, 8001, 7)),
]
TILE = 256


def geometry(src, dst, lpw, rolloff):
    g = math.gcd(src, dst)
    o, n = src // g, dst // g
    base = min(o, n) * rolloff
    width = int(math.ceil(lpw * o / base))
    return o, n, base, width


def kernel_f64(src, dst, lpw=6, rolloff=0.99, method="sinc_interp_hann", beta=None):
    """-> (K float64 [n][L], t_unclamped float64 [n][L], (o, n, width))."""
    o, n, base, width = geometry(src, dst, lpw, rolloff)
    beta = BETA if beta is None else float(beta)
    j = torch.arange(-width, width + o, dtype=torch.float64)
    p = torch.arange(n, dtype=torch.float64)
    tu = (-p[:, None] / n + j[None, :] / o) * base
    t = tu.clamp(-float(lpw), float(lpw))
    if method == "sinc_interp_hann":
        win = torch.cos(math.pi * t / (2.0 * lpw)) ** 2
    elif method == "sinc_interp_kaiser":
        win = torch.i0(beta * torch.sqrt(1.0 - (t / lpw) ** 2)) / torch.i0(torch.tensor(beta, dtype=torch.float64))
    else:
        raise ValueError(method)
    a = math.pi * t
    snc = torch.where(a == 0.0, torch.ones_like(a), torch.sin(a) / torch.where(a == 0.0, torch.ones_like(a), a))
    return snc * win * (base / o), tu, (o, n, width)


@lru_cache(maxsize=2)
def _kernel_cached(src, dst, lpw, rolloff, method, beta):
    """(K, |float32(K)| in float64, (o, n, width)): computed once per filter and shared by every call that uses it."""
    K, _, geo = kernel_f64(src, dst, lpw, rolloff, method, beta)
    return K, K.to(torch.float32).to(torch.float64).abs(), geo


def lengths(o, n):
    """Input lengths of the model and parity tests: 1, 2, o - 1, o, o + 1 and the lengths whose output ends one sample before, on and
    after a 256-output tile (the second tile's edge when that stays below 20 000 samples)."""
    out = {1, 2, o - 1, o, o + 1}
    tiles = 2 if 2 * TILE * o // n + 2 <= 20000 else 1
    for want in (tiles * TILE - 1, tiles * TILE, tiles * TILE + 1):
        out.add(max(1, want * o // n))                 # ceil(N n / o) lands on or next to `want`; the neighbours cover the edge
        out.add(max(1, -(-want * o // n)))
    return sorted(v for v in out if 1 <= v <= 20000)


def resample_f64(x, src, dst, lpw=6, rolloff=0.99, method="sinc_interp_hann", beta=None):
    """x float32/float64 [C][N] (numpy) -> (y float64 [C][ceil(N n / o)], bound float64 of the same shape) for float32 data x."""
    K, K32, (o, n, width) = _kernel_cached(int(src), int(dst), int(lpw), float(rolloff), method, None if beta is None else float(beta))
    L = K.shape[1]
    x64 = torch.from_numpy(np.asarray(x, dtype=np.float32).astype(np.float64))
    C, N = x64.shape
    n_out = -(-N * n // o)
    frames = -(-n_out // n)
    need = (frames - 1) * o + L
    xpad = torch.zeros((C, 1, max(need, width + N)), dtype=torch.float64)
    xpad[:, 0, width:width + N] = x64
    with torch.no_grad():
        y = torch.nn.functional.conv1d(xpad, K[:, None, :], stride=o)[:, :, :frames]           # [C][n][frames]
        s = torch.nn.functional.conv1d(xpad.abs(), K32[:, None, :], stride=o)[:, :, :frames]
    y = y.permute(0, 2, 1).reshape(C, -1)[:, :n_out]
    s = s.permute(0, 2, 1).reshape(C, -1)[:, :n_out]
    S = 2 * width + 2
    bound = (S + 1) * 2.0 ** -24 * s + L * 2.0 ** -50 * float(x64.abs().max())
    return y.numpy(), bound.numpy()


def signal(C, N, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return (0.5 * rng.standard_normal((C, N))).astype(np.float32)
