"""The loudness engine (egr_loudness_frames, egr_true_peak) and the meter / gain-match nodes on the device.

Bit identity: the fused kernels must give exactly what the kernels of the null-test suite give when they are composed
(k_weight -> mono mean -> block mean squares; mono mean -> polyphase resampler -> max |.|), at every channel path (1-4 in registers,
5 and 9 through the general path), at n = 1, n shorter than any block, and around a multiple of the per-thread chunk x 64.

Nodes against fixture G15: each level within max(2e-5 dB, 2 x |reference - float64 restatement|), both taken from the fixture
(2e-5 dB is the bar tests/test_nulltest_nodes.py holds node levels to; the factor 2 lets the device sit on the other side of the
float64 value from the reference); the true peak on the linear value at 2e-6 relative (fixture G4's resampler bar); gain-match
floats at 2e-5 dB (exactly where the gain is clipped), audio at 2.5e-6 x max|golden| (2e-5 dB of gain is 2.3e-6, plus an ulp).
"""
import math

import numpy as np
import pytest
import torch

from conftest import gjson, gnpz
from loudness_cases import METER_KEYS, aud, case_signal, gain_inputs

pytestmark = pytest.mark.gpu

LEVEL_BAR_DB = 2e-5


def chunk_len(sr):
    """The per-thread chunk of egr_kweight / egr_loudness_frames for this rate (csrc/egr_glue.hip)."""
    k = float(np.float32(math.exp(-2 * math.pi * (60.0 / (sr * 0.5)))))
    w = max(64, int(math.ceil(26.0 / -math.log(k))))
    return (w + 2) // 3


def raw_engine(xt, sr):
    """egr_loudness_frames called directly -> (mono [n] tensor, ms_a, ms_b)."""
    from egregora_amd import loudness, native
    C, n = xt.shape
    k = math.exp(-2 * math.pi * (60.0 / (sr * 0.5)))
    wa, ha, fa = loudness.block_shape(sr, 0.400, 0.100, n)
    wb, hb, fb = loudness.block_shape(sr, 3.0, 1.0, n)
    mono = torch.full((n + 8,), float("nan"), device="cuda")          # guard floats behind the n the call may write
    out = torch.empty(fa + fb, dtype=torch.float64, device="cuda")
    native.check(native.lib().egr_loudness_frames(native.ptr(xt), C, n, float(np.float32(1 - k)), float(np.float32(k)), wa, ha, fa, wb, hb,
                                                  fb, native.ptr(mono), out.data_ptr(), out.data_ptr() + 8 * fa, native.stream_ptr()),
                 "egr_loudness_frames")
    o = out.cpu().numpy()
    assert bool(torch.isnan(mono[n:]).all())
    return mono[:n], o[:fa], o[fa:]


def composed(xt, sr):
    from egregora_amd import device_ops, loudness
    n = xt.shape[1]
    y = device_ops.k_weight(xt, sr)
    wa, ha, _ = loudness.block_shape(sr, 0.400, 0.100, n)
    wb, hb, _ = loudness.block_shape(sr, 3.0, 1.0, n)
    return device_ops.mono_mean(y), device_ops.block_mean_squares(y, wa, ha), device_ops.block_mean_squares(y, wb, hb)


def _shapes():
    g = gjson("g15_loudness")["cases"]
    out = [(f"g15{name}", e["sr"], e["channels"], e["n"]) for name, e in sorted(g.items())]
    out += [("c5", 48000, 5, 30011), ("c9", 16000, 9, 20001), ("c4", 22050, 4, 25000), ("c7n1", 48000, 7, 1)]
    m = 2 * chunk_len(48000) * 64
    out += [(f"chunk{d:+d}", 48000, 2, m + d) for d in (-1, 0, 1)]
    out += [(f"chunk{d:+d}c6", 48000, 6, m // 2 + d) for d in (-1, 0, 1)]
    return out


@pytest.mark.parametrize("name,sr,C,n", _shapes(), ids=[s[0] for s in _shapes()])
def test_loudness_frames_bit_identical_to_composed_kernels(pack, name, sr, C, n):
    from egregora_amd import loudness
    rng = np.random.Generator(np.random.PCG64(1000 + C * 7 + n % 97))
    x = (0.3 * rng.standard_normal((C, n)) + 0.05).astype(np.float32)
    xt = torch.from_numpy(x).cuda()
    mono, ms_a, ms_b = raw_engine(xt, sr)
    want_mono, want_a, want_b = composed(xt, sr)
    assert torch.equal(mono, want_mono), (name, int((mono != want_mono).sum()))
    assert np.array_equal(ms_a, want_a) and np.array_equal(ms_b, want_b), name
    e_a, e_b, peak = loudness.engine(xt, sr)                     # the wrapper: same call, one buffer
    assert np.array_equal(e_a, want_a) and np.array_equal(e_b, want_b) and peak is None
    only_a, none_b, _ = loudness.engine(xt, sr, short_term=False)
    assert np.array_equal(only_a, want_a) and len(none_b) == 0


@pytest.mark.parametrize("C,n", [(1, 1), (2, 7), (2, 60000), (3, 70001), (5, 4099), (1, 185220)])
def test_true_peak_bit_identical_to_resample_then_absmax(pack, C, n):
    from egregora_amd import device_ops, loudness, native, resample
    rng = np.random.Generator(np.random.PCG64(2000 + C + n))
    x = (0.4 * rng.standard_normal((C, n))).astype(np.float32)
    x[-1, n // 2] = -3.0 * C                                       # a peak the filter overshoots, away from the ends
    xt = torch.from_numpy(x).cuda()
    mono = device_ops.mono_mean(xt)
    for up in (1, 2, 4, 8):
        y = resample.resample_hq(mono[None], 1, up).contiguous()
        assert y.shape[1] == n * up
        slot = torch.zeros(1, device="cuda")
        native.check(native.lib().egr_absmax(native.ptr(y), y.numel(), native.ptr(slot), native.stream_ptr()), "egr_absmax")
        want = float(slot.cpu()[0])
        assert want == float(y.abs().max().cpu())
        got_db = loudness.true_peak_dbfs(xt, up)
        assert got_db == 20.0 * math.log10(want + 1e-20), (C, n, up, got_db, want)
        assert loudness.engine(xt, 48000, False, up)[2] == want


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e", "f1000", "f1"])
def test_meter_node_vs_fixture(pack, name):
    from egregora_amd import egregora_audio_eval_loudness as el
    e = gjson("g15_loudness")["cases"][name]
    x = case_signal(e)
    node = el.Loudness_Meter_1770()
    for os_, want in sorted(e["ref"].items()):
        (got,) = node.execute(aud(x, e["sr"]), True, int(os_))
        f64 = e["f64"][os_]
        assert list(got) == METER_KEYS
        for k in METER_KEYS[:4]:
            bar = max(LEVEL_BAR_DB, 2.0 * abs(want[k] - f64[k]))
            print(f"{name} os={os_} {k}: got {got[k]!r} ref {want[k]!r} |d| {abs(got[k] - want[k]):.2e} bar {bar:.1e}")
            assert abs(got[k] - want[k]) <= bar, (name, os_, k, got[k], want[k], bar)
        lin_got, lin_want = 10 ** (got["true_peak_dbfs"] / 20.0), 10 ** (want["true_peak_dbfs"] / 20.0)
        print(f"{name} os={os_} true peak: got {lin_got!r} ref {lin_want!r} rel {abs(lin_got - lin_want) / lin_want:.2e}")
        assert abs(lin_got - lin_want) <= 2e-6 * lin_want, (name, os_, lin_got, lin_want)
    (got,) = node.execute(aud(x, e["sr"]), False)
    assert list(got) == e["keys_without_true_peak"] == METER_KEYS[:4]
    assert all(isinstance(v, float) for v in got.values())


@pytest.mark.parametrize("name", ["lufs", "rms", "clipped", "rate"])
def test_gain_match_node_vs_fixture(pack, name):
    from egregora_amd import egregora_audio_eval_loudness as el
    c = gjson("g15_loudness")["gain"][name]
    golden = gnpz("g15_loudness")[f"gain_{name}"]
    ref, ins = gain_inputs()
    x, sr = ins[c["input"]]
    out, gdb, rl, il = el.Audio_Gain_Match_1770().execute(aud(ref, 48000), aud(x, sr, {"tag": name}), **c["kwargs"])
    print(f"{name}: gain {gdb!r} ({c['gain_db']!r}) ref {rl!r} ({c['ref_level']!r}) in {il!r} ({c['in_level']!r})")
    assert all(isinstance(v, float) for v in (gdb, rl, il))
    assert max(abs(rl - c["ref_level"]), abs(il - c["in_level"])) <= LEVEL_BAR_DB
    if name == "clipped":
        assert gdb == c["gain_db"] == 1.0
    else:
        assert abs(gdb - c["gain_db"]) <= LEVEL_BAR_DB
    assert list(out["waveform"].shape) == c["shape"] and out["sample_rate"] == c["sr"] and sorted(out.keys()) == c["keys"]
    assert out["meta"] == c["meta"] and out["samples"].dtype == np.float32 and out["waveform"].dtype == torch.float32
    err = float(np.abs(out["samples"][:, ::29] - golden).max())
    print(f"{name}: audio max error {err:.2e}, bar {2.5e-6 * float(np.abs(golden).max()):.2e}")
    assert err <= 2.5e-6 * float(np.abs(golden).max())


def test_measure_issues_one_engine_call(pack, monkeypatch):
    """One measure(): one egr_loudness_frames, at most one egr_true_peak, no other per-sample entry point of the library."""
    from egregora_amd import loudness, native
    real = native.lib()
    calls = []

    class Counting:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if not callable(fn):
                return fn

            def wrapped(*a):
                calls.append(name)
                return fn(*a)
            return wrapped

    xt = torch.from_numpy(case_signal(gjson("g15_loudness")["cases"]["a"])).cuda()
    loudness.measure(xt, 48000, True, 4)                          # filter taps cached before counting
    monkeypatch.setattr(native, "lib", lambda: Counting())
    with_peak = loudness.measure(xt, 48000, True, 4)
    assert sorted(c for c in calls if c != "egr_last_error") == ["egr_loudness_frames", "egr_true_peak"], calls
    calls.clear()
    without = loudness.measure(xt, 48000, False)
    assert [c for c in calls if c != "egr_last_error"] == ["egr_loudness_frames"], calls
    assert list(without) == METER_KEYS[:4] and all(with_peak[k] == without[k] for k in without)
