"""The many-pair null test on the device against the single path on each pair alone.

One ragged wave of 37 pairs at 8 kHz with max_shift_ms = 20 (160 samples; n = 512 is the smallest legal transform): common lengths on
both sides of the power-of-two rule (2 n_common exactly 2^k, and one sample more), 1 / 2 / 3 channels, sides of unequal length in both
directions, reference lengths 255 / 256 / 257, clips shorter than one 400 ms block, an all-zero pair, a transform group with one pair
and one with more than twenty, known integer and fractional delays of both signs, gains within +-6 dB, noise 30 dB down.

Delays: out4 BIT-EQUAL to egr_gcc_phat (nothing in the plan split or the row hook depends on the row count: the rows run on a
one-channel plan's tables); a known integer delay d comes back as d - 1 (quirk Q8) to 5e-3 samples (the integer delays sit on clips
of 256 samples and more: on 255 samples with noise 30 dB down the float64 oracle's own parabola is already 5.8e-3 off).  Shift + FIR: BIT-EQUAL to
egr_shift_fir.  Levels: LUFS equal as floats (the block values are bit-equal), RMS within 1e-9 dB (a reordered double sum
moves by n 2^-53 relative).  Mix: matched and null BIT-EQUAL to device_ops.scale + null_mix, the counts equal, null_rms_dbfs within
1e-9 dB, null_lufs equal, corr_coef and lsd_mean_db within one float32 ulp, lsd_p95_db equal; with least squares scale_k within 1e-12
relative (the single path's sums use atomics) and the samples within one float32 step of k times the clip's peak.  A pair's results are
the same bits alone, among the 37, reversed and on a second run; launches and blocking reads do not depend on the number of pairs.
"""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
SR, SHIFT_MS = 8000, 20
N_FFT, HOP = 512, 64


def _delayed(x, d):
    """x [C, n] delayed by d samples (d > 0: later), zeros shifted in; a fractional part through the spectrum of the zero-padded clip."""
    C, n = x.shape
    di = int(np.floor(d))
    fr = d - di
    y = x.astype(np.float64)
    if fr:
        m = 2 * n
        f = np.fft.rfftfreq(m)
        y = np.fft.irfft(np.fft.rfft(np.pad(y, ((0, 0), (0, n))), axis=1) * np.exp(-2j * np.pi * f * fr), m, axis=1)[:, :n]
    out = np.zeros_like(y)
    if di >= 0:
        out[:, di:] = y[:, :n - di] if di < n else 0
    else:
        out[:, :n + di] = y[:, -di:]
    return out


def _pair(rng, cr, cp, tr, tp, d, gain_db, zero=False):
    n = max(tr, tp) + 200
    ref = 0.1 * rng.standard_normal((cr, n))
    if zero:
        ref[:] = 0.0
    mono = ref.mean(axis=0, keepdims=True)
    proc = np.repeat(_delayed(mono, d), cp, axis=0) * 10 ** (gain_db / 20.0)
    proc += rng.standard_normal((cp, n)) * (np.sqrt(np.mean(mono ** 2)) * 10 ** (-30 / 20.0))
    return dict(ref=torch.from_numpy(ref[:, :tr].astype(np.float32).copy()), proc=torch.from_numpy(proc[:, :tp].astype(np.float32).copy()),
                d=d, gain_db=gain_db, zero=zero)


def _wave37():
    rng = np.random.Generator(np.random.PCG64(2037))
    #        cr cp  tr    tp    delay  gain
    spec = [(1, 1, 256, 256, 3, 1.0), (2, 2, 255, 300, -4.5, -2.0), (1, 1, 400, 256, 0, 0.0),                      # n = 512 (2 * 256 IS 512)
            (1, 1, 257, 257, 5, 3.0), (2, 2, 512, 700, -2.5, -3.0), (3, 3, 300, 600, 7.25, 2.0),                 # n = 1024
            (1, 1, 513, 513, -6, 1.5), (2, 2, 1000, 900, 10.5, -6.0),                                            # n = 2048
            (1, 1, 4096, 4096, 12, 6.0), (3, 3, 3200, 3199, -9.75, -1.0), (2, 2, 2049, 4000, 20, 0.5),           # n = 8192 (3199 < one block)
            (1, 1, 9000, 9000, -31, 2.5),                                                                        # n = 32768: a group of one
            (2, 2, 4097, 4097, 1, -4.0), (1, 1, 8192, 8192, -1, 4.0), (2, 2, 5000, 6000, 0, 0.0)]                # n = 16384 ...
    while len(spec) < 36:                                                                                        # ... 25 pairs in all
        c = 1 + int(rng.integers(3))
        d = float(rng.integers(-60, 61)) + (0.0 if rng.integers(2) else float(rng.integers(1, 8)) / 8.0)
        spec.append((c, c, 4097 + int(rng.integers(4000)), 4097 + int(rng.integers(4000)), d, float(rng.uniform(-6, 6))))
    pairs = [_pair(rng, *s) for s in spec]
    pairs.insert(20, _pair(rng, 2, 2, 4500, 4500, 0, 0.0, zero=True))                                            # an all-zero pair
    assert len(pairs) == 37
    return pairs


def _tensors(pairs):
    return [(p["ref"], p["proc"]) for p in pairs]


def _gcc_phat_single(xr, xp, ms):
    """egr_gcc_phat on one pair as device_ops.xcorr_delay calls it -> the four floats (host)."""
    import ctypes as C
    from egregora_amd import device_ops, fatllama_engine as fe, native
    n_c = min(xr.shape[1], xp.shape[1])
    a, b = device_ops.mono_mean(xr, n_c), device_ops.mono_mean(xp, n_c)
    n = device_ops.xcorr_transform_length(n_c, n_c)
    plan = fe._plan(2 * n, 1, 1, 0)
    work = torch.empty(4 * n, dtype=torch.float32, device="cuda")
    out4 = torch.empty(4, dtype=torch.float32, device="cuda")
    native.check(native.lib().egr_gcc_phat(C.c_void_p(plan), native.ptr(a), n_c, native.ptr(b), n_c, ms, native.ptr(work), native.ptr(out4),
                                           native.stream_ptr()), "egr_gcc_phat")
    return out4.cpu(), n


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _ulp32(a, b):
    return abs(a - b) <= float(np.spacing(np.float32(max(abs(a), abs(b)))))


@pytest.fixture(scope="module")
def wave(pack):
    return _wave37()


@pytest.fixture(scope="module")
def single(pack, wave):
    """The single path on every pair alone, computed once: out4, the three stages' outputs (device tensors moved to the host)."""
    from egregora_amd import egregora_null_test_suite as ns
    ms = int(SR * (SHIFT_MS / 1000.0))
    out = []
    for p in wave:
        xr, xp = p["ref"].cuda(), p["proc"].cuda()
        o4, n = _gcc_phat_single(xr, xp, ms)
        aligned, lag = ns.align_stage(xr, xp, SR, SHIFT_MS, True, 64)
        matched, gain_db, ref_level, in_level = ns.gain_stage(xr, aligned, SR, "LUFS-I")
        null, metrics = ns.null_stage(xr, matched, SR, True, False, True, True, True, True, False, N_FFT, HOP)
        out.append(dict(out4=o4, n=n, lag=lag, aligned=aligned.cpu(), matched=matched.cpu(), gain_db=gain_db, ref_level=ref_level,
                        in_level=in_level, null=null.cpu(), metrics=metrics))
    return out


@pytest.fixture(scope="module")
def many(pack, wave):
    from egregora_amd import null_many
    stats = {}
    res = null_many.full_many(_tensors(wave), SR, SHIFT_MS, "gcc-phat", True, 64, "LUFS-I", False, n_fft=N_FFT, hop=HOP, stats=stats)
    return res, stats


def test_wave_covers_the_cases(pack, wave):
    from egregora_amd import null_many
    nc = [min(p["ref"].shape[1], p["proc"].shape[1]) for p in wave]
    groups = null_many.transform_groups(nc)
    assert sorted(groups) == [512, 1024, 2048, 8192, 16384, 32768] and len(groups[32768]) == 1 and len(groups[16384]) >= 20
    assert 256 in nc and 257 in nc and 4096 in nc and 4097 in nc and 8192 in nc
    assert {p["ref"].shape[0] for p in wave} == {1, 2, 3} and {p["ref"].shape[1] for p in wave} >= {255, 256, 257}
    assert any(p["ref"].shape[1] > p["proc"].shape[1] for p in wave) and any(p["ref"].shape[1] < p["proc"].shape[1] for p in wave)
    assert any(p["ref"].shape[1] < 3200 for p in wave) and sum(p["zero"] for p in wave) == 1
    assert any(p["d"] > 0 and p["d"] % 1 for p in wave) and any(p["d"] < 0 and p["d"] % 1 for p in wave)
    assert any(p["d"] > 0 and not p["d"] % 1 for p in wave) and any(p["d"] < 0 and not p["d"] % 1 for p in wave)
    assert all(abs(p["gain_db"]) <= 6.0 for p in wave)


def test_delays_are_the_single_calls_bits(pack, wave, single):
    from egregora_amd import null_many
    raw, stats = [], {}
    lags = null_many.delays_many(_tensors(wave), SR, SHIFT_MS, stats=stats, raw=raw)
    assert stats["transform_groups"] == 6 and stats["host_reads"] == 1 and stats["library_calls"] == 6 and stats["waves"] == 1
    worst = 0.0
    for i, (p, s) in enumerate(zip(wave, single)):
        assert _same_bits(raw[i], s["out4"]), (i, raw[i], s["out4"])
        assert lags[i] == s["lag"], (i, lags[i], s["lag"])
        if not p["zero"] and not p["d"] % 1:
            worst = max(worst, abs(lags[i] - (p["d"] - 1)))
            assert abs(lags[i] - (p["d"] - 1)) <= 5e-3, (i, p["d"], lags[i])                   # quirk Q8: the true lag minus one
    frac = [abs(lags[i] - (p["d"] - 1)) for i, p in enumerate(wave) if p["d"] % 1]
    print(f"integer delays recovered to {worst:.2e} samples; fractional ones to {max(frac):.3f} (reported, the estimator's own limit)")


@pytest.mark.parametrize("fir_len", [16, 64, 255])
def test_shift_fir_is_the_single_kernels_bits(pack, fir_len):
    from egregora_amd import egregora_null_test_suite as ns, null_many
    rng = np.random.Generator(np.random.PCG64(fir_len))
    #        C  n_in  n_out  delay
    cases = [(1, 300, 255, 0.0), (2, 300, 256, 5e-7), (3, 300, 257, 4.0), (1, 1000, 1000, -7.0000004), (2, 700, 900, 2.25), (1, 900, 700, -3.625),
             (2, 257, 513, 0.5), (1, 256, 256, -0.125), (1, 1, 300, 0.0), (1, 1, 5, 0.4), (2, 1, 1, -0.4), (1, 50, 80, 50.0), (1, 50, 30, -73.5),
             (3, 9000, 8999, 159.875), (1, 600, 1, 1.5), (1, 255, 600, -254.75)]
    xs = [torch.from_numpy(rng.standard_normal((c, n)).astype(np.float32)) for c, n, _, _ in cases]
    want = [ns.apply_delay(x.cuda(), d, fir_len, n_out).cpu() for x, (_, _, n_out, d) in zip(xs, cases)]
    stats = {}
    got = null_many.shift_fir_many(xs, [c[3] for c in cases], fir_len, [c[2] for c in cases], stats=stats)
    assert stats["launches"] == 1 and stats["library_calls"] == 1 and stats["host_reads"] == 0
    for i, (g, w) in enumerate(zip(got, want)):
        assert _same_bits(g, w), (i, cases[i], float((g.cpu() - w).abs().max()))
    assert float(want[11].abs().max()) == 0.0 and float(want[12].abs().max()) == 0.0          # |int_d| >= n_in: all zeros
    on_device = null_many.shift_fir_many([x.cuda() for x in xs], [c[3] for c in cases], fir_len, [c[2] for c in cases])
    assert all(_same_bits(g, w) for g, w in zip(on_device, want))


def test_levels(pack, wave):
    from egregora_amd import device_ops, loudness, null_many
    clips = [p["ref"].cuda() for p in wave] + [p["proc"].cuda() for p in wave]
    stats = {}
    lufs = null_many._lufs(clips, [SR] * len(clips), stats)
    assert stats["level_groups"] == 3 and stats["host_reads"] == 3 and stats["library_calls"] == 3
    rms = null_many._rms_db(clips)
    blk, hop = max(1, int(round(0.400 * SR))), max(1, int(round(0.100 * SR)))
    worst = 0.0
    for i, x in enumerate(clips):
        ms = loudness.engine_many([x], SR, False, 0)[0][0]
        assert np.array_equal(ms, device_ops.block_mean_squares(device_ops.k_weight(x, SR), blk, hop)), i        # the 400 ms blocks, bit for bit
        assert lufs[i] == device_ops.integrated_lufs(x, SR), i
        worst = max(worst, abs(rms[i] - device_ops.rms_db(x)))
        assert abs(rms[i] - device_ops.rms_db(x)) <= 1e-9, (i, rms[i], device_ops.rms_db(x))
    print(f"RMS levels within {worst:.2e} dB of rms_db")
    got = null_many.gain_match_many(_tensors(wave)[:12], SR, "RMS", 12.0)
    from egregora_amd import egregora_null_test_suite as ns
    for i, (g, p) in enumerate(zip(got, wave)):
        _, gain_db, ref_level, in_level = ns.gain_stage(p["ref"].cuda(), p["proc"].cuda(), SR, "RMS", 12.0)
        assert abs(g[1] - gain_db) <= 2e-9 and abs(g[2] - ref_level) <= 1e-9 and abs(g[3] - in_level) <= 1e-9, i


def _check_metrics(got, want, i):
    assert list(got) == list(want), i
    for k in ("overshoot_count", "clipped_pct", "null_lufs", "lsd_p95_db"):
        assert got[k] == want[k], (i, k, got[k], want[k])
    if "hf_residual_db" in want:          # the same single call on the same null: its double sums use atomics (n 2^-53 relative, as RMS)
        assert abs(got["hf_residual_db"] - want["hf_residual_db"]) <= 1e-9, (i, got["hf_residual_db"], want["hf_residual_db"])
    assert abs(got["null_rms_dbfs"] - want["null_rms_dbfs"]) <= 1e-9, (i, got["null_rms_dbfs"], want["null_rms_dbfs"])
    assert _ulp32(got["corr_coef"], want["corr_coef"]), (i, got["corr_coef"], want["corr_coef"])
    assert _ulp32(got["lsd_mean_db"], want["lsd_mean_db"]), (i, got["lsd_mean_db"], want["lsd_mean_db"])


def test_full_many_is_the_three_stages(pack, wave, single, many):
    res, stats = many
    assert stats["waves"] == 1 and stats["transform_groups"] == 6 and stats["per_pair_calls"] == 0
    for i, ((matched, null, delay_ms, gain_db, metrics), s) in enumerate(zip(res, single)):
        assert delay_ms == float(1000.0 * s["lag"] / SR) and gain_db == s["gain_db"], (i, delay_ms, gain_db, s["lag"], s["gain_db"])
        assert _same_bits(matched, s["matched"]) and _same_bits(null, s["null"]), i
        assert metrics["scale_k"] == 1.0
        _check_metrics(metrics, s["metrics"], i)


def test_stage_calls_are_the_single_stages(pack, wave, single):
    """align_many, gain_match_many and null_test_many each against its stage, fed the single path's own intermediate signals."""
    from egregora_amd import null_many
    idx = list(range(0, 37, 3))
    al = null_many.align_many([_tensors(wave)[i] for i in idx], SR, SHIFT_MS, True, 64)
    gm = null_many.gain_match_many([(wave[i]["ref"], single[i]["aligned"]) for i in idx], SR, "LUFS-I", 12.0)
    nt = null_many.null_test_many([(wave[i]["ref"], single[i]["matched"]) for i in idx], SR, n_fft=N_FFT, hop=HOP)
    for j, i in enumerate(idx):
        s = single[i]
        assert _same_bits(al[j][0], s["aligned"]) and al[j][1] == s["lag"], i
        assert _same_bits(gm[j][0], s["matched"]) and gm[j][1:] == (s["gain_db"], s["ref_level"], s["in_level"]), i
        assert _same_bits(nt[j][0], s["null"]), i
        _check_metrics(nt[j][1], s["metrics"], i)
    # integer-only compensation and the sign without inversion
    from egregora_amd import egregora_null_test_suite as ns
    al = null_many.align_many([_tensors(wave)[i] for i in idx[:4]], SR, SHIFT_MS, False, 64)
    nt = null_many.null_test_many([(wave[i]["ref"], single[i]["matched"]) for i in idx[:4]], SR, invert_b=False, compute_lsd=False,
                                  compute_null_lufs=False)
    for j, i in enumerate(idx[:4]):
        want, _ = ns.align_stage(wave[i]["ref"].cuda(), wave[i]["proc"].cuda(), SR, SHIFT_MS, False, 64)
        assert _same_bits(al[j][0], want), i
        null, m = ns.null_stage(wave[i]["ref"].cuda(), single[i]["matched"].cuda(), SR, False, False, True, True, False, False)
        assert _same_bits(nt[j][0], null) and list(nt[j][1]) == list(m) and _ulp32(nt[j][1]["corr_coef"], m["corr_coef"]), i
    with pytest.raises(ValueError, match="pair 1: operands could not be broadcast together"):
        null_many.null_test_many([(wave[0]["ref"], wave[0]["ref"]), (torch.zeros(2, 300), torch.zeros(1, 300))], SR)


def test_least_squares_scale(pack, wave, single):
    from egregora_amd import egregora_null_test_suite as ns, null_many
    idx = [i for i in range(0, 37, 2) if not wave[i]["zero"]]
    stats = {}
    got = null_many.full_many([_tensors(wave)[i] for i in idx], SR, SHIFT_MS, least_squares_scale=True, n_fft=N_FFT, hop=HOP, stats=stats)
    worst_k = worst = 0.0
    for j, i in enumerate(idx):
        s = single[i]
        null, m = ns.null_stage(wave[i]["ref"].cuda(), s["matched"].cuda(), SR, True, True, True, True, True, True, False, N_FFT, HOP)
        matched, gnull, _, _, gm = got[j]
        assert _same_bits(matched, s["matched"]), i
        k = m["scale_k"]
        worst_k = max(worst_k, abs(gm["scale_k"] - k) / abs(k))
        assert abs(gm["scale_k"] - k) <= 1e-12 * abs(k), (i, gm["scale_k"], k)
        step = float(np.spacing(np.float32(abs(k) * float(s["matched"].abs().max()))))
        diff = float((gnull.cpu() - null.cpu()).abs().max())
        worst = max(worst, diff / step)
        assert diff <= step, (i, diff, step)
        assert list(gm) == list(m) and gm["overshoot_count"] == m["overshoot_count"]
        # a float32 k one step apart (6e-8 relative) moves a null 30 dB below the signal by 2e-6 relative: far inside these
        assert abs(gm["null_rms_dbfs"] - m["null_rms_dbfs"]) <= 1e-4 and abs(gm["lsd_mean_db"] - m["lsd_mean_db"]) <= 1e-3, i
    print(f"scale_k within {worst_k:.2e} relative; null samples within {worst:.2f} float32 steps of k x peak")
    plain = {}
    null_many.full_many([_tensors(wave)[i] for i in idx], SR, SHIFT_MS, n_fft=N_FFT, hop=HOP, stats=plain)
    assert stats["host_reads"] == plain["host_reads"] + 1 and stats["launches"] == plain["launches"] + 2           # once more for k


def _equal_results(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        assert _same_bits(x[0], y[0]) and _same_bits(x[1], y[1]) and x[2:4] == y[2:4], i
        assert list(x[4]) == list(y[4]) and all(np.float64(x[4][k]).tobytes() == np.float64(y[4][k]).tobytes() for k in x[4]), (i, x[4], y[4])


def test_a_pair_does_not_depend_on_the_others(pack, wave, many):
    from egregora_amd import null_many
    res, _ = many
    kw = dict(align_max_shift_ms=SHIFT_MS, n_fft=N_FFT, hop=HOP)
    again = null_many.full_many(_tensors(wave), SR, **kw)
    _equal_results(res, again)
    rev = null_many.full_many(_tensors(wave)[::-1], SR, **kw)
    _equal_results(res, rev[::-1])
    for i in (0, 4, 9, 11, 20, 25, 36):
        alone = null_many.full_many([_tensors(wave)[i]], SR, **kw)
        _equal_results([res[i]], alone)


def test_shape_of_the_work(pack, wave, many):
    from egregora_amd import null_many
    res, stats = many
    kw = dict(align_max_shift_ms=SHIFT_MS, n_fft=N_FFT, hop=HOP)
    three, split = {}, {}
    res3 = null_many.full_many(_tensors(wave) * 3, SR, stats=three, **kw)
    assert stats["waves"] == three["waves"] == 1
    for k in ("launches", "host_reads", "library_calls", "transform_groups", "level_groups"):
        assert stats[k] == three[k], (k, stats[k], three[k])
    # lags, levels (three channel counts), sums, the nulls' loudness (three again), LSD
    assert stats["host_reads"] == 1 + 3 + 1 + 3 + 1 and stats["level_groups"] == 6 and stats["transform_groups"] == 6
    _equal_results(res + res + res, res3)
    budget = 6 * max(null_many.pair_bytes(p["ref"].shape[0], p["ref"].shape[1], p["proc"].shape[0], p["proc"].shape[1], N_FFT, HOP) for p in wave)
    res_split = null_many.full_many(_tensors(wave), SR, stats=split, max_bytes=budget, **kw)
    assert split["waves"] > 1
    _equal_results(res, res_split)
    print(f"37 pairs: {stats['launches']} launches, {stats['host_reads']} blocking reads, {stats['library_calls']} library calls in one wave")


def test_other_rate_hf_residual_and_device_inputs(pack, wave, single):
    from egregora_amd import device_ops, egregora_null_test_suite as ns, null_many
    rng = np.random.Generator(np.random.PCG64(5))
    other = _pair(rng, 2, 2, 3000, 6200, 3, 1.0)                              # the processed side at 16 kHz
    pairs = [_tensors(wave)[1], (other["ref"], other["proc"]), _tensors(wave)[9]]
    stats = {}
    got = null_many.full_many([(a.cuda(), b.cuda()) for a, b in pairs], [SR, (SR, 2 * SR), SR], SHIFT_MS, compute_hf_residual=True,
                              n_fft=N_FFT, hop=HOP, stats=stats)
    assert stats["per_pair_calls"] == 1 + 3                                   # one resample, three band energies
    for j, (a, b) in enumerate(pairs):
        xr, xp = a.cuda(), b.cuda()
        if j == 1:
            xp = ns._at_rate(xp, 2 * SR, SR)
        aligned, lag = ns.align_stage(xr, xp, SR, SHIFT_MS, True, 64)
        matched, gain_db, _, _ = ns.gain_stage(xr, aligned, SR, "LUFS-I")
        null, m = ns.null_stage(xr, matched, SR, True, False, True, True, True, True, True, N_FFT, HOP)
        assert got[j][2] == float(1000.0 * lag / SR) and got[j][3] == gain_db, j
        assert _same_bits(got[j][0], matched) and _same_bits(got[j][1], null), j
        assert "hf_residual_db" in m
        _check_metrics(got[j][4], m, j)
    # the band edge inside the spectrum (the Full node has no widget for it: at 8 kHz its 8000 Hz leaves no band)
    i = 9
    got = null_many.null_test_many([(wave[i]["ref"], single[i]["matched"])], SR, compute_hf_residual=True, n_fft=N_FFT, hop=HOP, hf_band_hz=2000)
    null, m = ns.null_stage(wave[i]["ref"].cuda(), single[i]["matched"].cuda(), SR, True, False, True, True, True, True, True, N_FFT, HOP, 2000)
    assert _same_bits(got[0][0], null) and -60.0 < m["hf_residual_db"] < 0.0
    _check_metrics(got[0][1], m, i)


_NODES = """
import json, sys
sys.path.insert(0, %r)
import numpy as np, torch
from packload import load_pack
p = load_pack()
rng = np.random.Generator(np.random.PCG64(11))
def clip(c, n, sr):
    return {"waveform": torch.from_numpy((0.1 * rng.standard_normal((1, c, n))).astype(np.float32)), "sample_rate": sr}
refs = [clip(2, 3000, 8000), clip(1, 700, 8000), clip(2, 2500, 8000)]
procs = []
for r in refs:
    w = torch.roll(r["waveform"], 5, dims=2) * 0.8 + 0.003 * torch.from_numpy(rng.standard_normal(tuple(r["waveform"].shape)).astype(np.float32))
    procs.append({"waveform": w, "sample_rate": 8000, "meta": {"tag": int(w.shape[2])}})
stack = {"waveform": torch.cat([refs[0]["waveform"], refs[2]["waveform"][:, :, :2500].repeat(1, 1, 2)[:, :, :3000]]), "sample_rate": 8000}
M = p.NODE_CLASS_MAPPINGS
out = {"same": True, "why": []}
def same(tag, a, b):
    ok = a == b if not hasattr(a, "shape") else (a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32)))
    if not ok:
        out["same"] = False
        out["why"].append(tag)
full = M["Null Test (Full) (batch)"]().execute(refs, procs, [20], ["gcc-phat"], [True], [64], ["LUFS-I"], [False], [True], [True], [True], [True], [False], [512], [64])
assert len(full) == 5 and all(len(v) == 3 for v in full)
for i in range(3):
    one = M["Null Test (Full)"]().execute(refs[i], procs[i], 20, "gcc-phat", True, 64, "LUFS-I", False, True, True, True, True, False, False, False, False, 512, 64)
    same(f"full matched {i}", full[0][i]["samples"], one[0]["samples"]); same(f"full null {i}", full[1][i]["samples"], one[1]["samples"])
    same(f"full meta {i}", full[0][i]["meta"], one[0]["meta"]); same(f"full rate {i}", full[0][i]["sample_rate"], one[0]["sample_rate"])
    same(f"full delay {i}", full[2][i], one[2]); same(f"full gain {i}", full[3][i], one[3])
    same(f"full keys {i}", list(full[4][i]), list(one[4]))
    for k in ("overshoot_count", "clipped_pct", "scale_k", "null_lufs", "lsd_p95_db"):
        same(f"full {k} {i}", full[4][i][k], one[4][k])
    same(f"full waveform shape {i}", tuple(full[1][i]["waveform"].shape), tuple(one[1]["waveform"].shape))
nt = M["Audio Null Test (batch)"]().execute(refs, [full[0][i] for i in range(3)], [True], [False], [True], [True], [True], [True], [False], [512], [64], [8000])
assert len(nt) == 2 and len(nt[0]) == len(nt[1]) == 3
for i in range(3):
    one = M["Audio Null Test"]().execute(refs[i], full[0][i], True, False, True, True, True, True, False, 512, 64, 8000)
    same(f"null audio {i}", nt[0][i]["samples"], one[0]["samples"]); same(f"null keys {i}", list(nt[1][i]), list(one[1]))
    for k in ("overshoot_count", "clipped_pct", "scale_k", "null_lufs", "lsd_p95_db"):
        same(f"null {k} {i}", nt[1][i][k], one[1][k])
b = M["Audio Null Test (batch)"]().execute([stack], [stack], [True], [False], [True], [True], [False], [False], [False], [512], [64], [8000])
out["stack"] = [len(b[0]), [list(a["samples"].shape) for a in b[0]], [m["overshoot_count"] for m in b[1]]]
print("DUMP" + json.dumps(out))
"""


def test_batch_nodes_give_the_single_nodes_results():
    env = dict(os.environ, EGREGORA_NULLTEST_BATCH_NODES="1")
    args = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", _NODES % str(ROOT)]
    r = subprocess.run(args, env=env, cwd=str(ROOT), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("DUMP")][-1][4:])
    assert d["same"], d["why"]
    assert d["stack"] == [2, [[2, 3000], [2, 3000]], [0, 0]]
