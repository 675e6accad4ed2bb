"""numpy / CPU-torch references for tests/test_gpu_nn_ops_laps.py: every operator of csrc/egr_nn_ops.hip restated on the host.
Each operator has a float64 function (the yardstick) and, where the kernel promises an order of operations, a float32 restatement
in that order (bit-exact cases, and the "four times the restatement's own error" cases).  Nothing here touches the device.

Layouts are the kernels': activations channels-last ([B][HW][C], [B][L][C], [B][H][W][C]), rows contiguous."""
import math

import numpy as np
import torch

F32, F64 = np.float32, np.float64
U24 = 2.0 ** -24
EW_ADD, EW_AXPBY, EW_SILU, EW_SCALE, EW_COPY, EW_ADD_SCALE = range(6)


def erf64(x):
    from scipy.special import erf
    return erf(np.asarray(x, F64))


def silu64(v):
    return v / (1.0 + np.exp(-v))


# ---------------------------------------------------------------- GroupNorm over [B][HW][C]
def gn_coeff64(x, gamma, beta, G, eps):
    """-> (scale, shift) [B][C] float64 with y = x scale + shift; biased variance over the HW * C/G elements of a group."""
    x = np.asarray(x, F64)
    B, HW, C = x.shape
    xg = x.reshape(B, HW, G, C // G)
    mean = xg.mean(axis=(1, 3))
    var = ((xg - mean[:, None, :, None]) ** 2).mean(axis=(1, 3))
    rstd = 1.0 / np.sqrt(var + eps)
    sc = np.repeat(rstd, C // G, axis=1) * np.asarray(gamma, F64)[None]
    sh = np.asarray(beta, F64)[None] - np.repeat(mean, C // G, axis=1) * sc
    return sc, sh


def groupnorm64(x, gamma, beta, G, eps, silu=False):
    sc, sh = gn_coeff64(x, gamma, beta, G, eps)
    y = np.asarray(x, F64) * sc[:, None, :] + sh[:, None, :]
    return silu64(y) if silu else y


def gn_coeff32(x, gamma, beta, G, eps):
    """The statistics pass as the header of k_gn_stats states it: float32 squares, the sum and the sum of squares in double,
    var = E[x^2] - mean^2 in double (clamped at 0), scale and shift rounded to float32."""
    x = np.asarray(x, F32)
    B, HW, C = x.shape
    xg = x.reshape(B, HW, G, C // G)
    n = HW * (C // G)
    mean = xg.sum(axis=(1, 3), dtype=F64) / n
    var = np.maximum((xg * xg).sum(axis=(1, 3), dtype=F64) / n - mean * mean, 0.0)
    rstd = 1.0 / np.sqrt(var + F64(F32(eps)))
    sc = np.repeat(rstd, C // G, axis=1) * np.asarray(gamma, F32).astype(F64)[None]
    sh = np.asarray(beta, F32).astype(F64)[None] - np.repeat(mean, C // G, axis=1) * sc
    return sc.astype(F32), sh.astype(F32)


def groupnorm32(x, gamma, beta, G, eps):
    """gn_coeff32, then y = x * scale + shift in float32, product and sum each rounded (k_affine_c without SiLU)."""
    sc, sh = gn_coeff32(x, gamma, beta, G, eps)
    return (np.asarray(x, F32) * sc[:, None, :] + sh[:, None, :]).astype(F32)


# ---------------------------------------------------------------- LayerNorm, softmax
def layernorm64(x, gamma, beta, eps):
    x = np.asarray(x, F64)
    mean = x.mean(axis=-1, keepdims=True)
    var = ((x - mean) ** 2).mean(axis=-1, keepdims=True)
    return (x - mean) / np.sqrt(var + eps) * np.asarray(gamma, F64) + np.asarray(beta, F64)


def softmax64(x):
    """Row softmax; a row's -inf entries give exactly 0."""
    x = np.asarray(x, F64)
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


# ---------------------------------------------------------------- element-wise
def eltwise64(a, b, op, s0=0.0, s1=0.0):
    a = np.asarray(a, F64)
    b = None if b is None else np.asarray(b, F64)
    s0, s1 = F64(F32(s0)), F64(F32(s1))                   # the scalars arrive as floats
    if op == EW_ADD:
        return a + b
    if op == EW_AXPBY:
        return s0 * a + s1 * b
    if op == EW_SILU:
        return silu64(a)
    if op == EW_SCALE:
        return s0 * a
    if op == EW_ADD_SCALE:
        return s0 * (a + b)
    return a.copy()


def eltwise32(a, b, op, s0=0.0, s1=0.0):
    """The float32 order of k_eltwise; EW_ADD_SCALE rounds the sum first (add followed by scale), EW_AXPBY rounds both products."""
    a = np.asarray(a, F32)
    b = None if b is None else np.asarray(b, F32)
    s0, s1 = F32(s0), F32(s1)
    if op == EW_ADD:
        return a + b
    if op == EW_AXPBY:
        return s0 * a + s1 * b
    if op == EW_SILU:
        return (a / (F32(1) + np.exp(-a))).astype(F32)
    if op == EW_SCALE:
        return s0 * a
    if op == EW_ADD_SCALE:
        return s0 * (a + b)
    return a.copy()


def geglu64(u, D):
    """u [rows][2 D] -> u[:, :D] * gelu(u[:, D:]) with the exact erf."""
    u = np.asarray(u, F64)
    g = u[..., D:]
    return u[..., :D] * (0.5 * g * (1.0 + erf64(g * math.sqrt(0.5))))


def concat(a, b):
    return np.concatenate([a, b], axis=-1)


def transpose(x):
    """[batch][R][C] -> [batch][C][R]."""
    return np.ascontiguousarray(np.swapaxes(x, 1, 2))


# ---------------------------------------------------------------- anti-aliased snake over [B][L][C], any even K
def snake64(x, alpha, beta, filt):
    """oracle/flashsr_torch._act_aa in float64 on the float32 inputs; channels-last in and out."""
    from oracle import flashsr_torch as R
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, F64)))
    y = R._act_aa(t(x).permute(0, 2, 1).contiguous(), t(alpha), t(beta), t(filt))
    return y.permute(0, 2, 1).contiguous().numpy()


def snake_direct64(x, alpha, beta, filt):
    """The formula above k_snake_aa by explicit loops (slow; checks snake64's index conventions on short inputs):
    u[i] = 2 sum_n xp[n] f[i + pl - 2n], s = u + sin^2(a u) / (b + 1e-9), y[l] = sum_k f[k] s[clamp(2l + k - (K/2 - 1))]."""
    x = np.asarray(x, F64)
    f = np.asarray(filt, F64)
    B, L, C = x.shape
    K = len(f)
    pad = K // 2 - 1
    pl = 2 * pad + (K - 2) // 2
    a, ib = np.exp(np.asarray(alpha, F64)), 1.0 / (np.exp(np.asarray(beta, F64)) + 1e-9)
    xp = x[:, np.clip(np.arange(-pad, L + pad), 0, L - 1)]
    s = np.zeros((B, 2 * L, C))
    for i in range(2 * L):
        u = np.zeros((B, C))
        for n in range(L + 2 * pad):
            j = i + pl - 2 * n
            if 0 <= j < K:
                u += xp[:, n] * f[j]
        u *= 2.0
        s[:, i] = u + ib * np.sin(u * a) ** 2
    y = np.zeros((B, L, C))
    for l in range(L):
        for k in range(K):
            y[:, l] += f[k] * s[:, min(max(2 * l + k - pad, 0), 2 * L - 1)]
    return y


# ---------------------------------------------------------------- ConvTranspose1d overlap-add
def col2im(Y, bias, add, Lout, r, pad, dtype=F64):
    """Y [B][Lin][K][Co] -> out [B][Lout][Co] = bias[co] + add[b][o][co] + sum over k == (o + pad) mod r (ascending k) of
    Y[b][(o + pad - k) / r][k][co] where that row exists: the order written in k_col2im1d, in `dtype`."""
    Y = np.asarray(Y, dtype)
    B, Lin, K, Co = Y.shape
    out = np.zeros((B, Lout, Co), dtype)
    if bias is not None:
        out += np.asarray(bias, dtype)[None, None]
    if add is not None:
        out = out + np.asarray(add, dtype)
    q = np.arange(Lout) + pad
    k, i = q % r, q // r
    while (k < K).any():
        ok = (k < K) & (i >= 0) & (i < Lin)
        o = np.flatnonzero(ok)
        out[:, o] = out[:, o] + Y[:, i[o], k[o]]
        k, i = k + r, i - 1
    return out


# ---------------------------------------------------------------- thin ends: tap gather, one-input-channel convolution
def tap_gather(P, bias, KH, KW, Cout, pad_t, pad_l, dtype=F64):
    """P [B][H][W][KH KW Cout] -> y [B][H][W][Cout] = bias + taps in ky, kx order, each read at the tap's source pixel (outside the
    image: nothing), in `dtype`."""
    P = np.asarray(P, dtype)
    B, H, W, _ = P.shape
    y = np.zeros((B, H, W, Cout), dtype)
    if bias is not None:
        y += np.asarray(bias, dtype)
    for ky in range(KH):
        for kx in range(KW):
            dy, dx = ky - pad_t, kx - pad_l                     # source pixel = output pixel + (dy, dx)
            o0, o1, p0, p1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
            if o0 >= o1 or p0 >= p1:
                continue
            t = ky * KW + kx
            y[:, o0:o1, p0:p1] = y[:, o0:o1, p0:p1] + P[:, o0 + dy:o1 + dy, p0 + dx:p1 + dx, t * Cout:(t + 1) * Cout]
    return y


def pack_cin1(w):
    """[Cout][KH][KW] -> the [Cout][16] layout egr_conv_cin1 reads (k = ky KW + kx contiguous, the rest zero)."""
    w = np.asarray(w, F32)
    out = np.zeros((w.shape[0], 16), F32)
    out[:, :w.shape[1] * w.shape[2]] = w.reshape(w.shape[0], -1)
    return out


def conv_cin1(x, w_packed, bias, KH, KW, pad_t, pad_l, fused32=False):
    """x [B][H][W] (one channel), packed weight -> y [B][H][W][Cout], zero padding.  float64, or with fused32 the kernel's float32
    chain acc = fma(v, w[k], acc) over k = 0 .. KH KW - 1 from acc = bias (the fused multiply-add formed in double: the product of
    two floats is exact there, the sum rounds to double and then to float)."""
    x = np.asarray(x, F64)
    B, H, W = x.shape
    wp = np.asarray(w_packed, F64)
    Cout = wp.shape[0]
    acc = np.zeros((B, H, W, Cout), F32 if fused32 else F64)
    if bias is not None:
        acc += np.asarray(bias, acc.dtype)
    xp = np.zeros((B, H + KH, W + KW))
    xp[:, pad_t:pad_t + H, pad_l:pad_l + W] = x
    for k in range(KH * KW):
        ky, kx = divmod(k, KW)
        v = xp[:, ky:ky + H, kx:kx + W, None]
        acc = (v * wp[:, k] + acc.astype(F64)).astype(acc.dtype)
    return acc


# ---------------------------------------------------------------- Winograd F(2x2, 3x3)
def wino_tiles(H, W):
    return (H + 1) // 2, (W + 1) // 2


def wino_in(x, scale=None, shift=None, silu=False, dtype=F64):
    """x [B][H][W][C] -> V [16][B TH TW][C] = B^T d B per 2x2 output tile (4x4 patch from row 2 ty - 1, column 2 tx - 1, zero padded),
    the row combination first and then the columns, each in the order written in k_wino_in; `dtype` arithmetic.  scale / shift
    [B][C] (+ SiLU) act on the samples, never on the padding."""
    x = np.asarray(x, dtype)
    B, H, W, C = x.shape
    TH, TW = wino_tiles(H, W)
    v = x
    if scale is not None:
        v = x * np.asarray(scale, dtype)[:, None, None] + np.asarray(shift, dtype)[:, None, None]
        if silu:
            v = silu64(v).astype(dtype)
    xp = np.zeros((B, 2 * TH + 2, 2 * TW + 2, C), dtype)
    xp[:, 1:H + 1, 1:W + 1] = v
    d = [[xp[:, r:r + 2 * TH:2, q:q + 2 * TW:2] for q in range(4)] for r in range(4)]
    V = np.empty((16, B * TH * TW, C), dtype)
    rows = (lambda q: d[0][q] - d[2][q], lambda q: d[1][q] + d[2][q], lambda q: d[2][q] - d[1][q], lambda q: d[1][q] - d[3][q])
    for r in range(4):
        row = [rows[r](q) for q in range(4)]
        for j, o in enumerate((row[0] - row[2], row[1] + row[2], row[2] - row[1], row[1] - row[3])):
            V[4 * r + j] = o.reshape(-1, C)
    return V


def wino_out(M, H, W, bias=None, res=None, act=0, dtype=F64):
    """M [16][B TH TW][N] -> y [B][H][W][N] = act((A^T M A) + bias + res), cropped to H x W, in the order written in k_wino_out
    (the bias is added even when absent, as a zero)."""
    M = np.asarray(M, dtype)
    TH, TW = wino_tiles(H, W)
    N = M.shape[2]
    B = M.shape[1] // (TH * TW)
    m = M.reshape(4, 4, B, TH, TW, N)
    s0 = [(m[0][q] + m[1][q]) + m[2][q] for q in range(4)]
    s1 = [(m[1][q] - m[2][q]) - m[3][q] for q in range(4)]
    o = [[(s0[0] + s0[1]) + s0[2], (s0[1] - s0[2]) - s0[3]], [(s1[0] + s1[1]) + s1[2], (s1[1] - s1[2]) - s1[3]]]
    y = np.empty((B, 2 * TH, 2 * TW, N), dtype)
    bv = np.zeros(N, dtype) if bias is None else np.asarray(bias, dtype)
    for a in range(2):
        for c in range(2):
            y[:, a::2, c::2] = o[a][c] + bv
    y = np.ascontiguousarray(y[:, :H, :W])
    if res is not None:
        y = y + np.asarray(res, dtype)
    if act == 1:
        y = silu64(y).astype(dtype)
    return y


def wino_weight(w):
    """G g G^T of a [N][C][3][3] weight in float64 -> U [16][C][N]: the weight transform that pairs with wino_in / wino_out."""
    G = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], F64)
    U = np.einsum("ir,ncrq,jq->ijcn", G, np.asarray(w, F64), G)
    return U.reshape(16, U.shape[2], U.shape[3])


# ---------------------------------------------------------------- input low-pass: cutoff bin and Chebyshev gain
def cutoff_bin(mag, nb, pct):
    """mag [B][T][ldm] -> cut [B]: the scan of oracle/flashsr_torch.lowpass_ref on e[k] = sum_t mag[t][k] (float32, t ascending)."""
    mag = np.asarray(mag, F32)
    cuts = []
    for m in mag:
        e = np.zeros(nb, F32)
        for t in range(m.shape[0]):
            e = e + m[t, :nb]
        c = np.cumsum(e.astype(F64))
        lim = c[-1] * F64(F32(pct))
        cut = 0
        for i in range(1, nb):
            if c[nb - i] < lim:
                cut = nb - i
                break
        cuts.append(cut)
    return np.array(cuts, np.int32)


def cheby_gain64(cut, nb_stft, sr, order, ripple_db, nbins):
    """gain [B][nbins] = 1 / (1 + eps^2 T_n^2(tan(pi f / sr) / tan(pi fc / sr))), 0 from 0.4999 sr, as lowpass_ref defines it."""
    eps2 = 10.0 ** (ripple_db / 10.0) - 1.0
    f = 0.5 * sr * np.arange(nbins, dtype=F64) / (nbins - 1)
    out = []
    for c in np.asarray(cut).tolist():
        fc = max(1.0, min(c / (nb_stft - 1), 0.999) * 0.5 * sr)
        xw = np.tan(math.pi * np.minimum(f, 0.4999 * sr) / sr) / math.tan(math.pi * fc / sr)
        tn = np.where(xw <= 1, np.cos(order * np.arccos(np.minimum(xw, 1.0))), np.cosh(order * np.arccosh(np.maximum(xw, 1.0))))
        out.append(np.where(f < 0.4999 * sr, 1.0 / (1.0 + eps2 * tn * tn), 0.0))
    return np.stack(out)


def cheby_gain32(cut, nb_stft, sr, order, ripple_db, nbins):
    """The same in float32, operation by operation as k_cheby_gain and its launcher write it (eps^2 = powf(10, ripple / 10) - 1)."""
    sr = F32(sr)
    eps2 = np.power(F32(10.0), F32(ripple_db) / F32(10.0)) - F32(1.0)
    pi = F32(3.14159265358979)
    k = np.arange(nbins).astype(F32)
    f = F32(0.5) * sr * k / F32(nbins - 1)
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for c in np.asarray(cut).tolist():
            fc = np.maximum(F32(1.0), np.minimum(F32(c) / F32(nb_stft - 1), F32(0.999)) * F32(0.5) * sr)
            wc = np.tan(pi * fc / sr)
            xw = np.tan(pi * f / sr) / wc
            tn = np.where(xw <= 1, np.cos(F32(order) * np.arccos(np.minimum(xw, F32(1)))),
                          np.cosh(F32(order) * np.arccosh(np.maximum(xw, F32(1)))))
            g = F32(1.0) / (F32(1.0) + eps2 * tn * tn)
            out.append(np.where(f < F32(0.4999) * sr, g, F32(0)).astype(F32))
    return np.stack(out)


# ---------------------------------------------------------------- STFT magnitude frames
def stft_index(L, n_fft, hop, rpad, T):
    """[T][n_fft] sample index of every frame element: reflect padding without edge repeat, then clamped (k_stft_frames)."""
    i = (np.arange(T) * hop - rpad)[:, None] + np.arange(n_fft)[None]
    i = np.where(i < 0, -i, i)
    i = np.where(i > L - 1, 2 * (L - 1) - i, i)
    return np.clip(i, 0, L - 1)


def stft_mag(x, n_fft, hop, rpad, T, t_valid, ldm, window, single=False):
    """x [B][L] -> mag [B][T][ldm]: |rfft(x[index] * window)| in bins 0 .. n_fft / 2, zero in the tail up to ldm and in frames
    t >= t_valid.  float64, or with single the float32 product and scipy's single-precision transform."""
    from scipy import fft as sfft
    dt = F32 if single else F64
    x = np.asarray(x, dt)
    fr = x[:, stft_index(x.shape[1], n_fft, hop, rpad, T)] * np.asarray(window, dt)
    X = sfft.rfft(fr, axis=-1)
    assert X.dtype == (np.complex64 if single else np.complex128)
    mag = np.zeros((x.shape[0], T, ldm), dt)
    mag[:, :, :n_fft // 2 + 1] = np.abs(X)
    mag[:, t_valid:] = 0
    return mag


# ---------------------------------------------------------------- Philox4x32-10 + Box-Muller
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays (or ints), key: two -> four uint32 arrays: ten rounds, the key raised by (W0, W1) between rounds."""
    c = [np.atleast_1d(np.asarray(v, np.uint64)) & MASK for v in ctr]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def randn(per_row, rows, seed, ids, single=False):
    """[rows][per_row] standard normals of k_randn: quad q of the row with id `ids[r]` from the counter (q, q >> 32, id, id >> 32) and
    the key (seed, seed >> 32); u = (float32(c) + 0.5f) 2^-32 and the angle float32(6.2831855f u) in float32; then log / sqrt / cos /
    sin in float64, or with single in float32 throughout."""
    quads = (per_row + 3) // 4
    q = np.arange(quads, dtype=np.uint64)
    out = np.empty((rows, quads * 4), F32 if single else F64)
    dt = F32 if single else F64
    for r in range(rows):
        rid = int(ids[r]) & 0xFFFFFFFFFFFFFFFF
        c = philox4x32_10([q & MASK, q >> np.uint64(32), rid & 0xFFFFFFFF, rid >> 32], [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF])
        c[2], c[3] = np.broadcast_to(c[2], c[0].shape), np.broadcast_to(c[3], c[0].shape)
        u = [(v.astype(F32) + F32(0.5)) * F32(2.3283064365386963e-10) for v in c]
        z = out[r].reshape(quads, 4)
        for j, (ua, ub) in enumerate(((u[0], u[1]), (u[2], u[3]))):
            rad = np.sqrt(dt(-2.0) * np.log(ua.astype(dt)))
            ang = (F32(6.283185307179586) * ub).astype(dt)
            z[:, 2 * j] = rad * np.cos(ang)
            z[:, 2 * j + 1] = rad * np.sin(ang)
    return out[:, :per_row]
