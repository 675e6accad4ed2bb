"""The host references of tests/nn_refs.py checked against themselves: every float64 function against torch.nn.functional in float64
where torch has the operator, the Winograd pair against a direct 3x3 convolution, the integer Philox against known-answer vectors,
each float32 restatement within its own rounding bound of float64.  No device."""
import math
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nn_refs as N
from nn_refs import F32, F64, U24


def rng_for(seed):
    return np.random.Generator(np.random.PCG64(seed))


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, F64)))


def close64(got, want, tol=1e-12):
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    assert got.shape == want.shape, (got.shape, want.shape)
    err, ref = float(np.abs(got - want).max()), float(np.abs(want).max())
    assert err <= tol * max(ref, 1.0), (err, ref)


# ---------------------------------------------------------------- float64 functions against torch float64
@pytest.mark.parametrize("B,HW,C,G", [(2, 17, 6, 3), (1, 64, 64, 32), (3, 5, 24, 2), (2, 1, 4, 1)])
@pytest.mark.parametrize("silu", [False, True])
def test_groupnorm_vs_torch(B, HW, C, G, silu):
    r = rng_for(B + HW + C)
    x, ga, be = 3 * r.standard_normal((B, HW, C)) + 1.5, r.standard_normal(C), r.standard_normal(C)
    want = F.group_norm(t64(x).permute(0, 2, 1), G, t64(ga), t64(be), 1e-6)
    want = F.silu(want) if silu else want
    close64(N.groupnorm64(x, ga, be, G, 1e-6, silu), want.permute(0, 2, 1).numpy(), 1e-11)
    sc, sh = N.gn_coeff64(x, ga, be, G, 1e-6)
    close64(x * sc[:, None] + sh[:, None], N.groupnorm64(x, ga, be, G, 1e-6), 1e-13)


def test_layernorm_softmax_geglu_vs_torch():
    r = rng_for(2)
    for C in (1, 3, 64, 65, 1000):
        x, ga, be = 2 * r.standard_normal((7, C)) + 0.3, r.standard_normal(C), r.standard_normal(C)
        close64(N.layernorm64(x, ga, be, 1e-5), F.layer_norm(t64(x), (C,), t64(ga), t64(be), 1e-5).numpy(), 1e-11)
    s = 6 * r.standard_normal((5, 300))
    s[1, ::3] = -np.inf
    s[2] = 0.25
    close64(N.softmax64(s), torch.softmax(t64(s), -1).numpy())
    assert (N.softmax64(s)[1, ::3] == 0).all()
    u = 2 * r.standard_normal((20, 64))
    a, g = t64(u).chunk(2, -1)
    close64(N.geglu64(u, 32), (a * F.gelu(g)).numpy())


def test_eltwise_concat_transpose():
    r = rng_for(3)
    a, b = r.standard_normal(1000).astype(F32), r.standard_normal(1000).astype(F32)
    s0, s1 = 0.7, -1.3
    a64, b64 = a.astype(F64), b.astype(F64)
    f0, f1 = float(F32(s0)), float(F32(s1))
    want = {N.EW_ADD: a64 + b64, N.EW_AXPBY: f0 * a64 + f1 * b64, N.EW_SILU: F.silu(t64(a)).numpy(), N.EW_SCALE: f0 * a64,
            N.EW_COPY: a64, N.EW_ADD_SCALE: f0 * (a64 + b64)}
    terms = {N.EW_ADD: 1, N.EW_AXPBY: 3, N.EW_SILU: 4, N.EW_SCALE: 1, N.EW_COPY: 0, N.EW_ADD_SCALE: 2}      # roundings per element
    for op, w in want.items():
        close64(N.eltwise64(a, b, op, s0, s1), w, 1e-15)
        got32 = N.eltwise32(a, b, op, s0, s1)
        assert got32.dtype == F32
        mag = np.abs(f0 * a64) + np.abs(f1 * b64) if op == N.EW_AXPBY else np.maximum(np.abs(w), np.abs(a64) + np.abs(b64) if op == N.EW_ADD_SCALE else 0)
        assert (np.abs(got32 - w) <= terms[op] * U24 * (mag + 1e-30) + 0).all(), op
    assert np.array_equal(N.eltwise32(a, b, N.EW_ADD_SCALE, s0), F32(s0) * (a + b))          # the sum rounded first
    x, y = r.standard_normal((2, 5, 3)), r.standard_normal((2, 5, 4))
    assert np.array_equal(N.concat(x, y), torch.cat([t64(x), t64(y)], -1).numpy())
    assert np.array_equal(N.transpose(x), t64(x).transpose(1, 2).contiguous().numpy())


@pytest.mark.parametrize("K", [8, 12, 32])
@pytest.mark.parametrize("L", [1, 3, 4, 5, 37])
def test_snake_index_conventions(K, L):
    """oracle/flashsr_torch._act_aa in float64 is the formula above k_snake_aa, for every even K."""
    from packload import load_pack
    load_pack()
    from egregora_amd import flashsr_arch as A
    r = rng_for(K + L)
    x, al, be = 2 * r.standard_normal((2, L, 5)), 0.5 + 0.1 * r.standard_normal(5), -0.3 + 0.1 * r.standard_normal(5)
    filt = A.kaiser_sinc_filter(K)
    close64(N.snake64(x, al, be, filt), N.snake_direct64(x, al, be, filt), 1e-13)


@pytest.mark.parametrize("r_,add,bias", [(2, True, True), (3, False, False), (5, True, True), (6, False, True)])
def test_col2im_vs_conv_transpose1d(r_, add, bias):
    rg = rng_for(r_)
    K = 2 * r_ + r_ % 2
    B, Lin, Ci, Co = 2, 23, 7, 5
    x, w = rg.standard_normal((B, Ci, Lin)), rg.standard_normal((Ci, Co, K))
    b = rg.standard_normal(Co) if bias else None
    ad = rg.standard_normal((B, Lin * r_, Co)) if add else None
    want = F.conv_transpose1d(t64(x), t64(w), None if b is None else t64(b), stride=r_, padding=(K - r_) // 2).permute(0, 2, 1).numpy()
    want = want + ad if add else want
    Y = np.einsum("bil,iok->blko", x, w)                                       # [B][Lin][K][Co]
    got = N.col2im(Y, b, ad, Lin * r_, r_, (K - r_) // 2)
    close64(got, want)
    Y32 = Y.astype(F32)
    b32, ad32 = (None if b is None else b.astype(F32)), (None if ad is None else ad.astype(F32))
    got32 = N.col2im(Y32, b32, ad32, Lin * r_, r_, (K - r_) // 2, F32)
    ref = N.col2im(Y32, b32, ad32, Lin * r_, r_, (K - r_) // 2)
    mag = N.col2im(np.abs(Y32), None if b is None else np.abs(b32), None if ad is None else np.abs(ad32), Lin * r_, r_, (K - r_) // 2)
    assert got32.dtype == F32 and (np.abs(got32 - ref) <= (K // r_ + 3) * U24 * mag).all()


@pytest.mark.parametrize("Co", [1, 3])
def test_tap_gather_vs_conv2d(Co):
    rg = rng_for(Co)
    B, H, W, Ci = 2, 6, 7, 5
    x, w, b = rg.standard_normal((B, Ci, H, W)), rg.standard_normal((Co, Ci, 3, 3)), rg.standard_normal(Co)
    want = F.conv2d(t64(x), t64(w), t64(b), padding=1).permute(0, 2, 3, 1).numpy()
    P = np.einsum("bchw,ocyx->bhwyxo", x, w).reshape(B, H, W, 9 * Co)           # per-tap products [ky][kx][co]
    close64(N.tap_gather(P, b, 3, 3, Co, 1, 1), want)
    P32, b32 = P.astype(F32), b.astype(F32)
    got32 = N.tap_gather(P32, b32, 3, 3, Co, 1, 1, F32)
    mag = N.tap_gather(np.abs(P32), np.abs(b32), 3, 3, Co, 1, 1)
    assert got32.dtype == F32 and (np.abs(got32 - N.tap_gather(P32, b32, 3, 3, Co, 1, 1)) <= 9 * U24 * mag).all()


@pytest.mark.parametrize("k", [3, 1])
def test_conv_cin1_vs_conv2d(k):
    rg = rng_for(k)
    B, H, W, Co = 2, 7, 5, 8
    x = rg.standard_normal((B, H, W)).astype(F32)
    w, b = (rg.standard_normal((Co, k, k)) / k).astype(F32), rg.standard_normal(Co).astype(F32)
    wp = N.pack_cin1(w)
    assert wp.shape == (Co, 16) and not wp[:, k * k:].any()
    want = F.conv2d(t64(x)[:, None], t64(w)[:, None], t64(b), padding=k // 2).permute(0, 2, 3, 1).numpy()
    got = N.conv_cin1(x, wp, b, k, k, k // 2, k // 2)
    close64(got, want)
    got32 = N.conv_cin1(x, wp, b, k, k, k // 2, k // 2, fused32=True)
    mag = N.conv_cin1(np.abs(x), np.abs(wp), np.abs(b), k, k, k // 2, k // 2)
    assert got32.dtype == F32 and (np.abs(got32 - got) <= k * k * U24 * mag).all()
    assert np.abs(got32 - got).max() > 0


@pytest.mark.parametrize("H,W", [(6, 8), (7, 5), (1, 1)])
def test_winograd_pair_is_a_3x3_convolution(H, W):
    rg = rng_for(H * W)
    B, C, Nn = 2, 4, 8
    x, w = rg.standard_normal((B, H, W, C)), rg.standard_normal((Nn, C, 3, 3))
    b, res = rg.standard_normal(Nn), rg.standard_normal((B, H, W, Nn))
    V = N.wino_in(x)
    M = np.einsum("xtc,xcn->xtn", V, N.wino_weight(w))
    want = F.conv2d(t64(x).permute(0, 3, 1, 2), t64(w), t64(b), padding=1).permute(0, 2, 3, 1).numpy() + res
    close64(N.wino_out(M, H, W, b, res), want)
    close64(N.wino_out(M, H, W, b, res, act=1), F.silu(t64(want)).numpy())
    sc, sh = 1 + 0.1 * rg.standard_normal((B, C)), 0.1 * rg.standard_normal((B, C))
    xa = F.silu(t64(x * sc[:, None, None] + sh[:, None, None])).numpy()
    close64(N.wino_in(x, sc, sh, True), N.wino_in(xa))                           # the affine + SiLU act on samples, padding stays 0
    x32, M32 = x.astype(F32), M.astype(F32)
    V32 = N.wino_in(x32, dtype=F32)
    assert V32.dtype == F32 and np.abs(V32 - N.wino_in(x32)).max() <= 3 * U24 * 4 * np.abs(x32).max()
    y32 = N.wino_out(M32, H, W, dtype=F32)
    assert y32.dtype == F32 and np.abs(y32 - N.wino_out(M32, H, W)).max() <= 6 * U24 * 9 * np.abs(M32).max()


def test_cutoff_and_chebyshev_gain_vs_lowpass_ref():
    from oracle import flashsr_torch as R
    cfg = types.SimpleNamespace(n_fft=128, hop=30, sr=48000)
    L = 3840
    t = np.arange(L) / cfg.sr
    g = rng_for(11)
    x = np.stack([sum(np.sin(2 * math.pi * f0 * t + i) / (i + 1) for i, f0 in enumerate((300.0, 1200.0, 2500.0, 5800.0))),
                  sum(np.sin(2 * math.pi * f0 * t + i) / (i + 1) for i, f0 in enumerate((200.0, 900.0, 2900.0))), np.zeros(L)])
    x = (0.3 * x / np.abs(x).max() + 1e-4 * g.standard_normal(x.shape) * (np.arange(3) < 2)[:, None]).astype(F32)
    want, cuts = R.lowpass_ref(torch.from_numpy(x), cfg)
    rpad = (cfg.n_fft - cfg.hop) // 2
    T = (L + 2 * rpad - cfg.n_fft) // cfg.hop + 1
    win = torch.hann_window(cfg.n_fft, periodic=True, dtype=torch.float64).numpy()
    mag = N.stft_mag(x, cfg.n_fft, cfg.hop, rpad, T, T, 80, win)
    nb = cfg.n_fft // 2 + 1
    got_cuts = N.cutoff_bin(mag, nb, 0.985)
    assert got_cuts.tolist() == cuts and cuts[2] == 0 and 0 < cuts[1] < cuts[0] < nb - 1          # the silent row cuts at bin 0
    nbins = L // 2 + 1
    gain = N.cheby_gain64(got_cuts, nb, cfg.sr, 8, 0.05, nbins)
    y = np.fft.irfft(np.fft.rfft(x.astype(F64), axis=1) * gain, n=L, axis=1)
    assert np.abs(y - want.numpy()).max() <= 2 * U24 * np.abs(x).max()                # lowpass_ref rounds its output to float32
    g32 = N.cheby_gain32(got_cuts, nb, cfg.sr, 8, 0.05, nbins)
    assert g32.dtype == F32 and np.isfinite(g32).all() and np.abs(g32 - gain).max() <= 1e-4
    assert gain[0, 0] == pytest.approx(1.0 / (1.0 + (10.0 ** 0.005 - 1.0)), abs=1e-12) and gain[:, -1].tolist() == [0, 0, 0]          # T_8(0) = 1


@pytest.mark.parametrize("n_fft,hop,L,ldm", [(4, 1, 9, 19), (128, 30, 500, 80), (2048, 480, 3000, 1025), (16, 4, 7, 9)])
def test_stft_mag_vs_torch(n_fft, hop, L, ldm):
    rg = rng_for(n_fft)
    rpad = min((n_fft - hop) // 2, L - 1)
    T = max(1, (L + 2 * rpad - n_fft) // hop + 1) + 2
    x, win = rg.standard_normal((2, L)).astype(F32), rg.uniform(0.1, 1, n_fft).astype(F32)
    got = N.stft_mag(x, n_fft, hop, rpad, T, T - 2, ldm, win)
    assert not got[:, T - 2:].any() and not got[:, :, n_fft // 2 + 1:].any()
    if rpad <= L - 1 and (T - 3) * hop - rpad + n_fft <= L + rpad:                  # every valid frame inside one reflection: F.pad's own
        xp = F.pad(t64(x)[:, None], (rpad, rpad), mode="reflect")[:, 0]
        fr = xp.unfold(1, n_fft, hop)[:, :T - 2] * t64(win)
        close64(got[:, :T - 2, :n_fft // 2 + 1], torch.fft.rfft(fr, dim=-1).abs().numpy())
    got32 = N.stft_mag(x, n_fft, hop, rpad, T, T - 2, ldm, win, single=True)
    assert got32.dtype == F32
    assert np.abs(got32 - got).max() <= (math.log2(n_fft) + 2) * 2 * U24 * np.abs(got).max() * math.sqrt(n_fft)


# ---------------------------------------------------------------- Philox and Box-Muller
def test_philox4x32_10_known_answers():
    """The known-answer vectors of Philox4x32-10 as Random123's kat_vectors lists them (recalled, see profiles/nn_ops_laps.md)."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = tuple(int(v[0]) for v in N.philox4x32_10(ctr, key))
        assert got == want, ([hex(v) for v in got], [hex(v) for v in want])
    ctrs = np.array([k[0] for k in kat], np.uint32).T                               # vectorised over the counter
    got = N.philox4x32_10(list(ctrs), kat[0][1])
    assert tuple(int(v[0]) for v in got) == kat[0][2] and got[0].shape == (3,)


def test_randn_restatement_and_moments():
    ids = [5, 2 ** 33 + 1, 7]
    z = N.randn(40001, 3, 0x123456789ABCDEF, ids)
    assert z.shape == (3, 40001) and np.isfinite(z).all()
    assert abs(z.mean()) < 0.02 and abs(z.std() - 1) < 0.02 and abs((z ** 3).mean()) < 0.05
    assert np.array_equal(N.randn(40001, 1, 0x123456789ABCDEF, [2 ** 33 + 1])[0], z[1])          # a row is a function of (seed, id)
    assert not np.array_equal(N.randn(40001, 1, 0x123456789ABCDEF, [1])[0], z[1])                # the id's high word counts
    assert np.array_equal(N.randn(7, 1, 9, [3])[0], N.randn(40001, 1, 9, [3])[0, :7])            # ragged last quad
    z32 = N.randn(40001, 3, 0x123456789ABCDEF, ids, single=True)
    # log, sqrt, -2 x, cos / sin and the product: a few float32 roundings of a value below 7
    assert z32.dtype == F32 and 0 < np.abs(z32 - z).max() <= 8 * U24 * 7


def test_groupnorm32_within_rounding_of_float64():
    r = rng_for(40)
    x = (r.standard_normal((2, 300, 8)) + 10.0).astype(F32)                         # mean 10 x the standard deviation
    ga, be = r.standard_normal(8).astype(F32), r.standard_normal(8).astype(F32)
    got, want = N.groupnorm32(x, ga, be, 2, 1e-6), N.groupnorm64(x, ga, be, 2, 1e-6)
    sc, _ = N.gn_coeff64(x, ga, be, 2, 1e-6)
    # scale, shift, the product and the sum round once each, at the size of x scale (the sum cancels to the size of y)
    assert got.dtype == F32 and 0 < np.abs(got - want).max() <= 4 * U24 * float(np.abs(x).max() * np.abs(sc).max())
