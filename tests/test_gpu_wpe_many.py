"""Many clips in one WPE call (egr_wpemany_dereverb, wpe_engine.dereverb_many, wpe_many, the batch node and CLI).

A (clip, bin) workgroup of the many-clip kernels runs the single call's text on the single call's layout behind a base pointer, and a
clip's spectra, weights and filter never touch another clip's: every clip must come back with the BITS wpe_engine.dereverb gives it
alone (torch.equal; no tolerance).  The one test with a bar holds the packed X of case B to the float64 restatement under the bar of
test_gpu_wpe.py::test_forward_error_well_conditioned, max(2e-7, the complex64 restatement's own error), on the spectra the packed
call itself formed.

The short-transform wave runs at n_fft = 64, hop = 16, taps = 3, delay = 1, where no clip can have fewer frames than delay + taps - 1
= 3 (one sample already frames into n_fft / hop = 4): its second clip has the fewest frames there are.  A clip with fewer frames than
the history is reached in test_clips_shorter_than_the_history, at hop = 32 and delay = 2 (2 and 3 frames against a history of 4).
"""
import ctypes
import random

import numpy as np
import pytest
import torch

import wpe_cases
import wpe_numpy as wn

pytestmark = pytest.mark.gpu

SHORT = dict(n_fft=64, hop=16, taps=3, delay=1, iterations=2)


def n_for_frames(F, n_fft=64, hop=16, short_by=0):
    """The largest n (less short_by < hop) that frames into exactly F frames."""
    return hop * (F - 1) - (n_fft - 2 * hop) - short_by


def noise(c, n, seed):
    """[c, n] float32 on the device: white noise with a decaying echo, so that the filter has something to remove."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(c, n, generator=g)
    if n > 40:
        x[:, 40:] += 0.5 * x[:, :-40].clone()
    return (0.1 * x).cuda()


def case_clip(name, n=None, seed=None):
    c = wpe_cases.CASES[name]
    if n is None:
        return torch.from_numpy(wpe_cases.case_signal(name)).cuda()
    return torch.from_numpy(wpe_cases.signal(c["channels"], n, seed)).cuda()


def cfg_of(name):
    c = wpe_cases.CASES[name]
    return dict(n_fft=c["n_fft"], hop=c["hop"], taps=c["taps"], delay=c["delay"], iterations=c["iterations"])


def singles(xs, cfg):
    from egregora_amd import wpe_engine
    return [wpe_engine.dereverb(x, **cfg).clone() for x in xs]


def assert_wave_equals_singles(xs, cfg, want=None, equal_nan=False):
    from egregora_amd import wpe_engine
    want = singles(xs, cfg) if want is None else want              # (first: the workspace then keeps the many-clip call's state)
    got = [y.clone() for y in wpe_engine.dereverb_many(xs, **cfg)]
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape == (xs[i].shape[0], wpe_engine.out_length(xs[i].shape[1], cfg["n_fft"], cfg["hop"])), i
        same = torch.equal(g, w) or (equal_nan and torch.allclose(g, w, rtol=0, atol=0, equal_nan=True))
        assert same, f"clip {i} of {len(xs)} (n = {xs[i].shape[1]}): {int((g != w).sum())} samples differ"
    return got


def packed_state(lengths, channels, cfg):
    """Y, X (complex64 numpy [bins][C][frames]) and flags of every clip, read from the workspace the last many-clip call used."""
    from egregora_amd import wpe_engine
    ws = wpe_engine.workspace(torch.device("cuda", torch.cuda.current_device()), 0).cpu().numpy()
    bins, out = cfg["n_fft"] // 2 + 1, []
    for lay in wpe_engine.many_layout(lengths, channels, cfg["n_fft"], cfg["hop"]):
        nb = bins * channels * lay["frames"] * 8
        spec = lambda o: ws[o:o + nb].view(np.complex64).reshape(bins, channels, lay["frames"]).copy()
        out.append((spec(lay["Y"]), spec(lay["X"]), ws[lay["flags"]:lay["flags"] + 4 * bins].view(np.int32).copy()))
    return out


# ---------------------------------------------------------------------------------------------------------------- one wave, short transform
_SHORT = {}


def short_wave():
    if not _SHORT:
        lengths = [1, 2, n_for_frames(63), n_for_frames(64, short_by=3), n_for_frames(65), n_for_frames(24, short_by=7), n_for_frames(25),
                   16000]
        xs = [noise(1, n, 500 + i) for i, n in enumerate(lengths)]
        _SHORT.update(xs=xs, want=singles(xs, SHORT))
    return _SHORT["xs"], _SHORT["want"]


@pytest.mark.parametrize("order", ["given", "reversed", "shuffled"])
def test_one_wave_on_the_short_transform(pack, order):
    from egregora_amd import wpe_engine
    xs, want = short_wave()
    fr = [wpe_engine.frames(x.shape[1], 64, 16) for x in xs]
    assert fr == [4, 4, 63, 64, 65, 24, 25, 1003]
    idx = list(range(len(xs)))
    if order == "reversed":
        idx.reverse()
    elif order == "shuffled":
        random.Random(7).shuffle(idx)
        assert idx != sorted(idx) and idx != sorted(idx, reverse=True)
    assert_wave_equals_singles([xs[i] for i in idx], SHORT, [want[i] for i in idx])


def test_clips_shorter_than_the_history(pack):
    cfg = dict(n_fft=64, hop=32, taps=3, delay=2, iterations=2)
    from egregora_amd import wpe_engine
    xs = [noise(2, n, 540 + i) for i, n in enumerate((1, 33, 3000, 64, 700))]
    assert [wpe_engine.frames(x.shape[1], 64, 32) for x in xs][:2] == [2, 3] and cfg["delay"] + cfg["taps"] - 1 == 4
    assert_wave_equals_singles(xs, cfg)


# ---------------------------------------------------------------------------------------------------------------- wpe_cases
def test_case_b_packed_bits_and_forward_error(pack):
    c, cfg = wpe_cases.CASES["B"], cfg_of("B")
    xs = [case_clip("B", 5000, 601), case_clip("B"), case_clip("B", 12345, 602)]
    from egregora_amd import wpe_engine
    assert_wave_equals_singles(xs, cfg)
    Y, X, flags = packed_state([x.shape[1] for x in xs], 3, cfg)[1]                   # the full-length clip, in the middle of the table
    assert np.array_equal(Y, wpe_engine.stft(xs[1], cfg["n_fft"], cfg["hop"]).cpu().numpy()) and not flags.any()
    X128 = wn.wpe(Y.astype(np.complex128), c["taps"], c["delay"], c["iterations"])
    bar = max(2e-7, wn.rel_rms(wn.wpe(Y, c["taps"], c["delay"], c["iterations"]), X128))
    err = wn.rel_rms(X, X128)
    print(f"case B packed: device {err:.2e}, bar {bar:.2e}")
    assert err <= bar, (err, bar)


def test_case_c_packed_bits(pack):
    assert_wave_equals_singles([case_clip("C", 9000, 611), case_clip("C", 20001, 612), case_clip("C")], cfg_of("C"))


@pytest.mark.parametrize("name,lengths", [("F", (3000, 700, 1500)), ("G", (1200, 3000)), ("H", (2000, 900))])
def test_wide_geometries_at_a_shortened_length(pack, name, lengths):
    """F: 32 channels, two 4 x 4 blocks per thread; G and H: more than 32 channels, the 32-frame tile.  The 700-sample clip of F has
    fewer frames than K = 64, so its factorisation stops: it must keep the single call's bits all the same."""
    from egregora_amd import wpe_engine
    cfg = cfg_of(name)
    xs = [case_clip(name, n, 620 + i) for i, n in enumerate(lengths)]
    assert_wave_equals_singles(xs, cfg)
    if name == "F":
        state = packed_state(list(lengths), 32, cfg)
        assert state[1][2].all() and not state[0][2].any()                           # flags: the short clip's guard, not its neighbour's
        assert wpe_engine.frames(700, 64, 16) < 64


def test_all_zero_clip_between_two_normal_ones(pack):
    cfg = dict(n_fft=64, hop=16, taps=3, delay=1, iterations=2)
    xs = [noise(2, 4000, 631), torch.zeros(2, 2500, device="cuda"), noise(2, 3100, 632)]
    assert_wave_equals_singles(xs, cfg, equal_nan=True)
    flags = [s[2] for s in packed_state([4000, 2500, 3100], 2, cfg)]
    assert flags[1].all() and not flags[0].any() and not flags[2].any()               # the silent clip's guard fires in every bin


def test_three_hundred_small_clips(pack):
    rnd = random.Random(11)
    lengths = [rnd.randint(800, 3200) for _ in range(300)]                            # 0.05 - 0.2 s at 16 kHz
    g = torch.Generator().manual_seed(640)
    flat = (0.1 * torch.randn(2, sum(lengths), generator=g)).cuda()
    xs, pos = [], 0
    for n in lengths:
        xs.append(flat[:, pos:pos + n].contiguous())
        pos += n
    assert_wave_equals_singles(xs, dict(n_fft=64, hop=16, taps=3, delay=1, iterations=2))


def test_repeatability(pack):
    from egregora_amd import wpe_engine
    xs = [noise(2, n, 650 + i) for i, n in enumerate((5000, 16000, 333))]
    cfg = dict(n_fft=256, hop=64, taps=10, delay=3, iterations=3)
    a = [y.clone() for y in wpe_engine.dereverb_many(xs, **cfg)]
    b = wpe_engine.dereverb_many(xs, **cfg)
    assert all(torch.equal(p, q) for p, q in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------- wpe_many, node, CLI
def test_dereverb_many_over_mixed_channel_counts(pack, monkeypatch):
    from egregora_amd import egregora_audio_enhance_wpe as ew, wpe_engine, wpe_many
    w = dict(taps=4, delay=2, iterations=2, n_fft=256, hop=64)
    shapes = [(1, 8000), (2, 4000), (3, 3000), (1, 7000), (2, 4500), (3, 2500), (2, 60000), (1, 8500), (2, 3900), (3, 2800), (1, 6000),
              (2, 4100), (3, 3100), (1, 5000), (3, 2000)]
    rates = [16000, 22050, 48000, 8000, 44100]
    clips = [(noise(c, n, 700 + i).cpu() if i % 2 else noise(c, n, 700 + i), rates[i % len(rates)]) for i, (c, n) in enumerate(shapes)]
    budget = wpe_engine.many_workspace_bytes([3000, 2500, 2800], 3, 256, 64, 4) + 4096
    monkeypatch.setenv("EGREGORA_WPE_WAVE_GB", repr(budget / (1 << 30)))
    stats = {}
    ys = wpe_many.dereverb_many(clips, stats=stats, **w)
    assert stats["alone"] == 1 and stats["waves"] == len(stats["wave_bytes"]) == len(stats["wave_clips"])
    assert all(0 < b <= budget for b in stats["wave_bytes"])
    for c in (1, 2, 3):
        assert sum(1 for wave in stats["wave_clips"] if shapes[wave[0]][0] == c) >= 2, (c, stats)
    assert sorted(i for wave in stats["wave_clips"] for i in wave) == [i for i in range(len(shapes)) if i != 6]
    node = ew.Egregora_WPE_Dereverb()
    for i, ((x, sr), y) in enumerate(zip(clips, ys)):
        (ref,) = node.execute({"waveform": x.cpu()[None], "sample_rate": sr}, w["taps"], w["delay"], w["iterations"], w["n_fft"], w["hop"], True)
        assert not y.is_cuda and y.dtype == torch.float32 and torch.equal(y, ref["waveform"][0]), i


def test_refusals_leave_the_buffers_untouched(pack):
    from egregora_amd import native, wpe_engine
    L = native.lib()
    ARG, UNS = 1, 3
    lengths, C = [3000, 1000], 2
    tab, xf, yf = wpe_engine.clip_table(lengths, C, 256, 64)
    need = wpe_engine.many_workspace_bytes(lengths, C, 256, 64, 4)
    assert need > 0
    x = noise(1, xf, 800).reshape(-1)
    y = torch.full((yf,), 7.25, device="cuda")
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")
    T = lambda rows: (ctypes.c_int64 * (3 * len(rows)))(*[int(v) for r in rows for v in r])
    many_frames = (2 ** 31 - 4096) * 64

    def call(tab=tab, n=2, C=C, n_fft=256, hop=64, taps=4, delay=2, iters=2, x=native.ptr(x), y=native.ptr(y), ws=native.ptr(ws), nb=need):
        return L.egr_wpemany_dereverb(x, tab, n, C, n_fft, hop, taps, delay, iters, y, ws, nb, native.stream_ptr())

    cases = [
        ("n_clips = 0", dict(n=0), ARG), ("null x", dict(x=None), ARG), ("null y", dict(y=None), ARG), ("null ws", dict(ws=None), ARG),
        ("null table", dict(tab=None), ARG), ("negative x offset", dict(tab=T([(-4, 3000, 0), (6000, 1000, 8000)])), ARG),
        ("negative y offset", dict(tab=T([(0, 3000, -1), (6000, 1000, 8000)])), ARG),
        ("n = 0", dict(tab=T([(0, 3000, 0), (6000, 0, 8000)])), ARG), ("workspace one byte short", dict(nb=need - 1), ARG),
        ("iterations = 0", dict(iters=0), ARG),
        ("hop does not divide n_fft", dict(n_fft=1024, hop=192), UNS), ("n_fft / hop < 2", dict(hop=256), UNS),
        ("odd n_fft", dict(n_fft=255, hop=85), UNS), ("n_fft > 4096", dict(n_fft=8192, hop=2048), UNS),
        ("n_fft / 2 with a prime factor 17", dict(n_fft=68, hop=34), UNS), ("K > 64", dict(taps=33), UNS),
        ("history > 128", dict(taps=1, delay=129), UNS), ("LDS", dict(C=64, taps=1, delay=123, n_fft=64, hop=16), UNS),
        ("2^31 - 4096 frames", dict(tab=T([(0, 3000, 0), (6000, many_frames, 8000)])), UNS),
    ]
    for why, kw, want in cases:
        rc = call(**kw)
        assert rc == want, (why, rc, native.last_error())
    torch.cuda.synchronize()
    assert bool((y == 7.25).all()) and bool((ws == 0x5A).all())
    # the same buffers are good for the call itself
    assert call() == 0
    torch.cuda.synchronize()
    for i, n in enumerate(lengths):
        o = wpe_engine.out_length(n, 256, 64)
        want = wpe_engine.dereverb(x[tab[3 * i]:tab[3 * i] + C * n].view(C, n), 256, 64, 4, 2, 2)
        assert torch.equal(y[tab[3 * i + 2]:tab[3 * i + 2] + C * o].view(C, o), want)


def test_batch_node_and_cli(pack, tmp_path):
    """The opt-in list node on three tiny WAV files ([B,C,T] counts as B clips) and the directory front end on the same files."""
    from egregora_amd import dac_batch, egregora_audio_enhance_wpe as ew, egregora_audio_enhance_wpe_batch as eb, wavio, wpe_batch
    single, node = ew.Egregora_WPE_Dereverb(), eb.Egregora_WPE_DereverbBatch()
    assert eb.Egregora_WPE_DereverbBatch.INPUT_IS_LIST and eb.Egregora_WPE_DereverbBatch.OUTPUT_IS_LIST == (True,)
    assert node.INPUT_TYPES() == single.INPUT_TYPES()
    names = ("a.wav", "b.wav", "sub/c.wav")
    ind, outd = tmp_path / "in", tmp_path / "out"
    (ind / "sub").mkdir(parents=True)
    for i, (name, n) in enumerate(zip(names, (4000, 4000, 2777))):
        wavio.write_wav_pcm16(str(ind / name), noise(2, n, 900 + i).cpu().numpy().T, 16000)
    xs = [dac_batch.read_clip(ind / name)[0] for name in names]                      # what the files hold
    assert all(tuple(x.shape) == (2, n) for x, n in zip(xs, (4000, 4000, 2777)))
    audio = [{"waveform": torch.stack(xs[:2]), "sample_rate": 16000, "meta": {"k": 1}}, {"waveform": xs[2][None], "sample_rate": 16000}]
    (outs,) = node.execute(audio, taps=[4], delay=[2], iterations=[2], n_fft=[256], hop=[64], use_float32=[True])
    assert isinstance(outs, list) and len(outs) == 3
    for x, o in zip(xs, outs):
        (ref,) = single.execute({"waveform": x[None], "sample_rate": 16000}, 4, 2, 2, 256, 64, True)
        assert o["sample_rate"] == 16000 and torch.equal(o["waveform"], ref["waveform"])
        assert o["meta"]["wpe"] == ref["meta"]["wpe"] == {"taps": 4, "delay": 2, "iterations": 2, "n_fft": 256, "hop": 64}
    assert outs[0]["meta"]["k"] == 1
    assert wpe_batch.main(["--in-dir", str(ind), "--out-dir", str(outd), "--taps", "4", "--delay", "2", "--iterations", "2", "--n-fft", "256",
                           "--hop", "64"]) == 0
    for name, o in zip(names, outs):
        y, sr = dac_batch.read_clip(outd / name)
        assert sr == 16000
        # the file holds the PCM_16 writer's rounding of the node's samples; the reader divides by 32768
        want = tmp_path / "want.wav"
        wavio.write_wav_pcm16(str(want), o["waveform"][0].numpy().T, 16000)
        assert torch.equal(y, dac_batch.read_clip(want)[0])
