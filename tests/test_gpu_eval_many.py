"""Many-pair metrics and many-clip loudness on the device against the single-clip calls on each pair / clip.

Pair metrics: per[] and the two order statistics are BIT-EQUAL to egr_stft_mag x 2 + egr_lsd_frames + egr_order_stats2; lsd_mean_db is
within one float32 ulp of device_ops.lsd (which sums in double with atomics: only the final rounding can differ); si_sdr_db within
1e-9 dB of device_ops.si_sdr on pairs of 20-60 dB (4 n 2^-53 10 / ln 10 = 2e-9 at n = 2^20; the pairs here are far shorter), a pair
scored against itself only > 150 dB.  A pair's eight numbers are the same bits alone, among 37, in reversed order and on a second run.
Loudness: block values and peaks BIT-EQUAL to loudness.engine per clip.

Grids: every new kernel's grid equals its work count (frames, chunks, thread chunks, blocks, 256-sample peak tiles of all items
together).  HIP launches no grid of 2^32 work-items or more, so the totals consumed by 256-thread workgroups are capped at 2^24 - 1,
the pairs (one 1024-thread workgroup each) at 2^22 - 1, the thread chunks at 64 (2^26 - 1); the host refuses more before any copy
or launch (tests/test_eval_many_host.py holds the accept / refuse edges).  None walks laps.
"""
import numpy as np
import pytest
import torch

from conftest import gjson

pytestmark = pytest.mark.gpu

CHUNK = 4096                      # EGR_METRICS_CHUNK
N_FFT, HOP = 512, 64


def _signal(rng, c, n):
    t = np.arange(n) / 8000.0
    x = np.stack([0.3 * np.sin(2 * np.pi * (200.0 + 170.0 * k) * t + k) for k in range(c)]) + 0.05 * rng.standard_normal((c, n))
    return x.astype(np.float32)


def _pair(rng, ca, cb, ta, tb, snr_db=35.0):
    """(reference [ca, ta], processed [cb, tb]): the processed side is the reference's mono, scaled, plus noise snr_db below it."""
    n = max(ta, tb)
    ref = _signal(rng, ca, n)
    mono = ref.mean(axis=0)
    noise = rng.standard_normal((cb, n)) * (np.sqrt(np.mean(mono ** 2) + 1e-12) * 10 ** (-snr_db / 20.0))
    proc = (0.97 * mono[None, :] + noise).astype(np.float32)
    return torch.from_numpy(ref[:, :ta].copy()), torch.from_numpy(proc[:, :tb].copy())


def _wave37():
    """37 ragged pairs at (n_fft, hop) = (512, 64): the lengths around the frame rule, the percentile edges (1 and 2 frames; 21
    frames, where 0.95 * 20 is an integer), the lengths around the SI-SDR chunk, mono / stereo / three channels on either side, and
    sides of unequal length (row stride != n)."""
    rng = np.random.Generator(np.random.PCG64(37))
    shapes = [
        (1, 1, 1, 1), (2, 1, 1, 9), (1, 1, N_FFT - 1, N_FFT - 1), (1, 2, N_FFT, N_FFT), (2, 2, N_FFT + HOP - 1, N_FFT + HOP - 1),
        (1, 1, N_FFT + HOP, N_FFT + HOP), (3, 1, N_FFT + HOP, N_FFT + HOP + 300), (1, 1, N_FFT + 20 * HOP, N_FFT + 20 * HOP),
        (2, 3, N_FFT + 20 * HOP + 63, N_FFT + 20 * HOP + 5), (1, 1, 5000, 5000), (2, 1, 6000, 5000), (1, 2, 4321, 7000),
        (1, 1, CHUNK - 1, CHUNK - 1), (2, 2, CHUNK, CHUNK), (1, 1, CHUNK + 1, CHUNK + 1), (1, 2, 2 * CHUNK + 3, 2 * CHUNK + 3),
        (3, 3, 2 * CHUNK + 3, CHUNK + 1), (1, 1, 20000, 20000),
    ]
    while len(shapes) < 37:
        shapes.append((1 + int(rng.integers(3)), 1 + int(rng.integers(3)), 1 + int(rng.integers(9000)), 1 + int(rng.integers(9000))))
    return [_pair(rng, *s) for s in shapes]


def _flat(pairs):
    """The pairs' sides laid back to back at their full lengths in two flat device buffers, and the table rows."""
    a = torch.cat([r.reshape(-1) for r, _ in pairs]).cuda()
    b = torch.cat([p.reshape(-1) for _, p in pairs]).cuda()
    rows, oa, ob = [], 0, 0
    for r, p in pairs:
        rows.append((oa, r.shape[0], r.shape[1], ob, p.shape[0], p.shape[1], min(r.shape[1], p.shape[1])))
        oa += r.numel()
        ob += p.numel()
    return a, b, rows


def _single(pair, n_fft, hop):
    """The single-clip calls on one pair, as the node makes them: (per[] bits, the two order statistics, lsd mean, lsd p95, si_sdr)."""
    from egregora_amd import device_ops, native
    r, p = pair
    n = min(r.shape[1], p.shape[1])
    a, b = r[:, :n].contiguous().cuda(), p[:, :n].contiguous().cuda()
    L = native.lib()
    SA, SB = device_ops._stft_frames(a, n_fft, hop), device_ops._stft_frames(b, n_fft, hop)
    frames, nb = SA.shape
    per = torch.empty((frames,), dtype=torch.float32, device="cuda")
    native.check(L.egr_lsd_frames(native.ptr(SA), native.ptr(SB), frames, nb, native.ptr(per), native.stream_ptr()), "egr_lsd_frames")
    _, lo, hi = device_ops.lsd_ranks(frames)
    o2 = torch.empty((2,), dtype=torch.float32, device="cuda")
    native.check(L.egr_order_stats2(native.ptr(per), frames, lo, hi, native.ptr(o2), native.stream_ptr()), "egr_order_stats2")
    mean, p95 = device_ops.lsd(a, b, n_fft, hop)
    return per.cpu().numpy(), o2.cpu().numpy(), mean, p95, device_ops.si_sdr(a, b)


def _split_per(per, rows, n_fft, hop):
    out, pos = [], 0
    for r in rows:
        f = 1 + max(0, (r[6] - n_fft) // hop)
        out.append(per[pos:pos + f])
        pos += f
    assert pos == len(per)
    return out


def _check_against_single(pairs, n_fft, hop):
    from egregora_amd import device_ops, eval_many
    a, b, rows = _flat(pairs)
    out8, per, launches = device_ops.metrics_pairs(a, b, rows, n_fft, hop, 3, want_per=True)
    assert launches == 6
    pers = _split_per(per, rows, n_fft, hop)
    worst_si = 0.0
    for i, pair in enumerate(pairs):
        s_per, s_o2, s_mean, s_p95, s_si = _single(pair, n_fft, hop)
        assert pers[i].tobytes() == s_per.tobytes(), f"pair {i}: per[] differs from egr_stft_mag x 2 + egr_lsd_frames"
        assert np.float32(out8[i, 1]).tobytes() == s_o2[0].tobytes() and np.float32(out8[i, 2]).tobytes() == s_o2[1].tobytes(), i
        assert out8[i, 3] == len(s_per)
        got = eval_many.metrics_finish(out8[i], True, True)
        ulp = float(np.spacing(np.float32(s_mean)))
        print(f"pair {i}: n={rows[i][6]} frames={len(s_per)} lsd {got['lsd_mean_db']!r} vs {s_mean!r}  si_sdr {got['si_sdr_db']!r} vs {s_si!r}")
        assert abs(got["lsd_mean_db"] - s_mean) <= ulp, (i, got["lsd_mean_db"], s_mean)
        assert got["lsd_p95_db"] == s_p95, (i, got["lsd_p95_db"], s_p95)
        if 20.0 <= s_si <= 60.0:
            worst_si = max(worst_si, abs(got["si_sdr_db"] - s_si))
            assert abs(got["si_sdr_db"] - s_si) <= 1e-9, (i, got["si_sdr_db"], s_si)
        else:                                   # a pair of a few samples: both paths add the same few terms
            assert abs(got["si_sdr_db"] - s_si) <= 1e-9 or (got["si_sdr_db"] > 150.0 and s_si > 150.0), (i, got["si_sdr_db"], s_si)
    print(f"worst |si_sdr many - single| on the 20-60 dB pairs: {worst_si:.3e} dB")
    return out8, pers


@pytest.fixture(scope="module")
def wave37(pack):
    pairs = _wave37()
    out8, pers = _check_against_single(pairs, N_FFT, HOP)
    return pairs, out8, pers


def test_wave_of_37_against_the_single_calls(wave37):
    """Frame-rule lengths, percentile edges, chunk edges, downmixes and strides: the checks run in the fixture."""
    pairs, out8, pers = wave37
    ns = [min(r.shape[1], p.shape[1]) for r, p in pairs]
    for n in (1, N_FFT - 1, N_FFT, N_FFT + HOP - 1, N_FFT + HOP, N_FFT + 20 * HOP, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3):
        assert n in ns
    assert {int(f) for f in out8[:, 3]} >= {1, 2, 21}
    assert any(r.shape[1] != p.shape[1] for r, p in pairs) and {r.shape[0] for r, _ in pairs} == {1, 2, 3}
    assert len(pairs) == 37 and sum(len(p) for p in pers) == int(out8[:, 3].sum())


def test_independence_order_and_repeat(wave37):
    from egregora_amd import device_ops
    pairs, out8, pers = wave37
    a, b, rows = _flat(pairs)
    again, per2, _ = device_ops.metrics_pairs(a, b, rows, N_FFT, HOP, 3, want_per=True)
    assert again.tobytes() == out8.tobytes() and per2.tobytes() == np.concatenate(pers).tobytes()           # a second run
    rev = list(reversed(pairs))
    ra, rb, rrows = _flat(rev)
    rout, rper, _ = device_ops.metrics_pairs(ra, rb, rrows, N_FFT, HOP, 3, want_per=True)
    assert rout[::-1].tobytes() == out8.tobytes()                                                        # reversed order
    for got, want in zip(_split_per(rper, rrows, N_FFT, HOP), reversed(pers)):
        assert got.tobytes() == want.tobytes()
    for i, pair in enumerate(pairs):                                                                     # alone
        xa, xb, xrows = _flat([pair])
        one, oper, launches = device_ops.metrics_pairs(xa, xb, xrows, N_FFT, HOP, 3, want_per=True)
        assert one[0].tobytes() == out8[i].tobytes() and oper.tobytes() == pers[i].tobytes() and launches == 6, i


def test_lsd_only_and_si_sdr_only(wave37):
    from egregora_amd import device_ops
    pairs, out8, _ = wave37
    a, b, rows = _flat(pairs)
    lsd_only, _, l1 = device_ops.metrics_pairs(a, b, rows, N_FFT, HOP, device_ops.METRICS_LSD)
    si_only, _, l2 = device_ops.metrics_pairs(a, b, rows, N_FFT, HOP, device_ops.METRICS_SI_SDR)
    assert (l1, l2) == (2, 4)
    assert lsd_only[:, :4].tobytes() == out8[:, :4].tobytes() and si_only[:, 4:].tobytes() == out8[:, 4:].tobytes()
    assert not lsd_only[:, 4:].any() and not si_only[:, :4].any()           # terms that were not asked for are not written


@pytest.mark.parametrize("n_fft,hop,lengths", [(2176, 544, (2176 + 544, 2176 + 2 * 544 + 17)), (8192, 2048, (8192 + 2048, 8192 + 2 * 2048))])
def test_generic_radix_stage_and_the_lds_limit(pack, n_fft, hop, lengths):
    """n_fft = 2176 = 2^7 * 17 runs one generic radix-17 stage; at 8192 the two transform buffers take the whole 64 KB of dynamic LDS and
    side A's 17 magnitudes per thread wait in registers.  Two and three frames each."""
    rng = np.random.Generator(np.random.PCG64(n_fft))
    pairs = [_pair(rng, 2, 1, lengths[0], lengths[0] + 100), _pair(rng, 1, 2, lengths[1], lengths[1])]
    out8, _ = _check_against_single(pairs, n_fft, hop)
    assert [int(f) for f in out8[:, 3]] == [2, 3]


def test_metrics_many_host_and_device_tensors_waves_and_stats(wave37, monkeypatch):
    from egregora_amd import egregora_audio_eval_pack as ep, eval_many
    pairs, out8, _ = wave37
    want = [eval_many.metrics_finish(out8[i], True, True) for i in range(len(pairs))]
    s1, s37 = {}, {}
    assert eval_many.metrics_many(pairs[:1], N_FFT, HOP, stats=s1) == want[:1]
    assert eval_many.metrics_many(pairs, N_FFT, HOP, stats=s37) == want                                   # host tensors, one wave
    assert s1["waves"] == s37["waves"] == 1 and s1["launches"] == s37["launches"] == 6 and s37["library_calls"] == 1
    on_dev = [(r.cuda(), p[0].cuda() if p.shape[0] == 1 else p.cuda()) for r, p in pairs]                 # device tensors, some [T]
    assert eval_many.metrics_many(on_dev, N_FFT, HOP) == want
    # a budget of three average pairs: several waves, each within the budget or a single pair, results in the caller's order
    need = [eval_many.pair_bytes(r.shape[0], r.shape[1], p.shape[0], p.shape[1], N_FFT, HOP, 3) for r, p in pairs]
    budget = 3 * sum(need) // len(need)
    monkeypatch.setenv("EGREGORA_EVAL_WAVE_GB", repr(budget / (1 << 30)))
    st = {}
    assert eval_many.metrics_many(pairs, N_FFT, HOP, stats=st) == want
    assert st["waves"] > 3 and st["launches"] == 6 * st["waves"] and st["wave_launches"] == [6] * st["waves"]
    assert sorted(i for w in st["wave_items"] for i in w) == list(range(37))
    for w in st["wave_items"]:
        assert len(w) == 1 or sum(need[i] for i in w) <= budget
    monkeypatch.delenv("EGREGORA_EVAL_WAVE_GB")
    # the node on one pair gives the dictionary of the wave (LSD mean to the float32 ulp, see the module docstring)
    (d,) = ep.Metrics_LSD_SISDR().execute({"waveform": pairs[10][0][None], "sample_rate": 8000}, {"waveform": pairs[10][1][None], "sample_rate": 8000},
                                          N_FFT, HOP)
    assert list(d) == list(want[10]) and d["lsd_p95_db"] == want[10]["lsd_p95_db"]
    assert abs(d["lsd_mean_db"] - want[10]["lsd_mean_db"]) <= float(np.spacing(np.float32(d["lsd_mean_db"])))
    assert abs(d["si_sdr_db"] - want[10]["si_sdr_db"]) <= 1e-9


def _golden_signals():
    """The seeded pair of tests/golden/make_golden_eval.py (the inputs of fixture G10)."""
    rng = np.random.Generator(np.random.PCG64(10))
    n = 60000
    t = np.arange(n) / 48000.0
    a = np.stack([0.3 * np.sin(2 * np.pi * 330 * t) + 0.1 * np.sin(2 * np.pi * 7000 * t) + 0.02 * rng.standard_normal(n),
                  0.25 * np.sin(2 * np.pi * 500 * t + 0.3) + 0.02 * rng.standard_normal(n)]).astype(np.float32)
    b = (a * np.float32(0.97) + 2e-3 * rng.standard_normal(a.shape)).astype(np.float32)[:, :59000]
    return a, b


def test_batch_node_reproduces_the_golden_pair(pack):
    """Fixture G10 through the batch node at the tolerances of tests/test_eval_nodes.py: 2e-5 relative on LSD, 1e-6 dB on SI-SDR."""
    from egregora_amd import egregora_audio_eval_batch as eb
    g = gjson("g10_eval")
    a, b = _golden_signals()
    A = {"waveform": torch.from_numpy(a)[None], "sample_rate": 48000}
    B = {"waveform": torch.from_numpy(b)[None], "sample_rate": 48000}
    node = eb.Metrics_LSD_SISDR_Batch()
    for name, kw in (("metrics_default", {}), ("metrics_1024_256", dict(n_fft=[1024], hop=[256])), ("metrics_lsd_only", dict(compute_si_sdr=[False]))):
        (outs,) = node.execute([A, A], [B, A], **kw)            # the golden pair, and the reference against itself
        got, self_ = outs
        want = g[name]
        assert sorted(got) == sorted(want)
        for k in ("lsd_mean_db", "lsd_p95_db"):
            assert abs(got[k] - want[k]) <= 2e-5 * want[k], (name, k, got[k], want[k])
            assert abs(self_[k] - 1e-6) < 1e-9                  # the sqrt(1e-12) floor
        if "si_sdr_db" in want:
            assert abs(got["si_sdr_db"] - want["si_sdr_db"]) <= 1e-6, (got["si_sdr_db"], want["si_sdr_db"])
            assert self_["si_sdr_db"] > 150.0
    # a [B,C,T] waveform counts as B clips
    two = {"waveform": torch.stack([torch.from_numpy(a), torch.from_numpy(a)]), "sample_rate": 48000}
    (outs,) = node.execute([two], [B, B])
    assert len(outs) == 2 and outs[0] == outs[1] and abs(outs[0]["si_sdr_db"] - g["metrics_default"]["si_sdr_db"]) <= 1e-6


# ---------------------------------------------------------------------------------------------------------------- loudness
def _loud_lengths(sr):
    from egregora_amd import loudness
    L, _ = loudness.chunking(sr)              # the launcher's own chunk length (egr_kweight_chunking), not a restatement of its rule
    blk, hop, st, st_hop = int(round(0.4 * sr)), int(round(0.1 * sr)), 3 * sr, sr
    return [1, blk - 1, blk, blk + 1, blk + hop, st - 1, st, st + 1, st + st_hop, L - 1, L, L + 1, 64 * L - 1, 64 * L, 64 * L + 1]


def _loud_clips(sr, ch, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    clips = [torch.from_numpy(0.5 * _signal(rng, ch, n)) for n in _loud_lengths(sr)]
    clips[-1][0, -1] = 4.0 * ch                    # the peak of the last clip sits in its last sample
    return clips


def test_rate_groups_differ_in_k_l_w(pack):
    from egregora_amd import loudness
    (l8, w8), (l16, w16) = loudness.chunking(8000), loudness.chunking(16000)
    assert l8 != l16 and w8 != w16 and 1 < l8 < l16
    assert {l8 - 1, l8, l8 + 1, 64 * l8 - 1, 64 * l8, 64 * l8 + 1} <= set(_loud_lengths(8000))


@pytest.mark.parametrize("sr", [8000, 16000])
@pytest.mark.parametrize("ch", [1, 2, 5])
def test_loudness_tracks_bit_equal_to_the_single_calls(pack, sr, ch):
    """Channels 1 and 2 take the register paths (CT = 1, 2), 5 the generic CT = 0 path.  Lengths: 1; around the 400 ms block; block +
    hop; around the 3 s block; 3 s + 1 s; around a thread chunk L and a workgroup's 64 L.  oversample 4 and 1."""
    from egregora_amd import loudness
    xs = [x.cuda() for x in _loud_clips(sr, ch, 100 * ch + sr // 8000)]
    for up in (4, 1):
        st = {}
        many = loudness.engine_many(xs, sr, True, up, stats=st)
        assert st == {"library_calls": 1, "launches": 4}
        st1 = {}
        loudness.engine_many(xs[:1], sr, True, up, stats=st1)
        assert st1 == st                                              # the launches do not depend on the number of clips
        for i, x in enumerate(xs):
            a, b, pk = loudness.engine(x, sr, True, up)
            ma, mb, mpk = many[i]
            assert ma.tobytes() == a.tobytes() and mb.tobytes() == b.tobytes(), (i, x.shape)
            assert np.float32(mpk).tobytes() == np.float32(pk).tobytes(), (i, mpk, pk)
        assert many[-1][2] >= 3.0                                     # the planted last sample is seen
    st = {}
    no_peak = loudness.engine_many(xs, sr, False, 0, stats=st)
    assert st["launches"] == 2 and all(p is None and len(b) == 0 for _, b, p in no_peak)
    assert all(m[0].tobytes() == n[0].tobytes() for m, n in zip(many, no_peak))


def test_loudness_many_mixed_list_in_the_callers_order(pack, monkeypatch):
    from egregora_amd import egregora_audio_eval_batch as eb, eval_many, loudness
    clips = []
    for j, (sr, ch) in enumerate([(8000, 1), (16000, 2), (8000, 5), (8000, 1), (16000, 1), (8000, 2), (16000, 2)]):
        for x in _loud_clips(sr, ch, 900 + j)[2 + j::5]:
            clips.append((x, sr))
    clips = clips[::2] + clips[1::2]                                    # rates and channel counts interleaved
    want = [loudness.measure(x.cuda(), sr) for x, sr in clips]
    st = {}
    assert eval_many.loudness_many(clips, stats=st) == want             # host tensors
    groups = len({(sr, x.shape[0]) for x, sr in clips})
    assert st["waves"] == st["library_calls"] == groups and st["launches"] == 4 * groups
    assert sorted(i for w in st["wave_items"] for i in w) == list(range(len(clips)))
    assert eval_many.loudness_many([(x.cuda(), sr) for x, sr in clips], True, 1) == [loudness.measure(x.cuda(), sr, True, 1) for x, sr in clips]
    no_peak = eval_many.loudness_many(clips, compute_true_peak=False)
    assert no_peak == [loudness.measure(x.cuda(), sr, False) for x, sr in clips] and "true_peak_dbfs" not in no_peak[0]
    monkeypatch.setenv("EGREGORA_EVAL_WAVE_GB", repr(300000 / (1 << 30)))       # about one long clip per wave
    st = {}
    assert eval_many.loudness_many(clips, stats=st) == want and st["waves"] > groups
    monkeypatch.delenv("EGREGORA_EVAL_WAVE_GB")
    (outs,) = eb.Loudness_Meter_1770_Batch().execute([{"waveform": x[None], "sample_rate": sr} for x, sr in clips[:5]], [True], [4])
    assert outs == want[:5]


def test_eval_batch_cli_scores_two_directories(pack, tmp_path, capsys):
    """eval_batch.py in process: one JSON line per pair, the corpus means last; an unpaired and an unreadable file make the status 1."""
    import json
    from egregora_amd import eval_batch, eval_many, wavio
    rng = np.random.Generator(np.random.PCG64(5))
    ref, proc = tmp_path / "ref", tmp_path / "proc"
    (ref / "sub").mkdir(parents=True)
    (proc / "sub").mkdir(parents=True)
    for name, ch, n in (("a", 1, 9000), ("sub/b", 2, 12001)):
        r, p = _pair(rng, ch, ch, n, n - 500)
        wavio.write_wav_pcm16(str(ref / f"{name}.wav"), (0.5 * r).numpy().T, 16000)
        wavio.write_wav_pcm16(str(proc / f"{name}.wav"), (0.5 * p).numpy().T, 16000)
    out = tmp_path / "scores.jsonl"
    assert eval_batch.main(["--ref-dir", str(ref), "--proc-dir", str(proc), "--out", str(out), "--loudness", "--n-fft", "512", "--hop", "64"]) == 0
    lines = [json.loads(ln) for ln in out.read_text().splitlines()]
    assert [ln.get("file") for ln in lines[:-1]] == ["a", "sub/b"] and lines[-1]["pairs"] == 2
    for ln in lines[:-1]:
        rx, px = eval_batch.read_clip(ref / f"{ln['file']}.wav"), eval_batch.read_clip(proc / f"{ln['file']}.wav")
        (m,) = eval_many.metrics_many([(rx[0], px[0])], 512, 64)
        assert {k: ln[k] for k in m} == m and 20.0 < ln["si_sdr_db"] < 60.0
        assert [ln["ref_loudness"], ln["proc_loudness"]] == eval_many.loudness_many([rx, px])
    for k in ("lsd_mean_db", "lsd_p95_db", "si_sdr_db"):
        assert abs(lines[-1]["mean"][k] - (lines[0][k] + lines[1][k]) / 2) <= 1e-12 * abs(lines[0][k])
    (ref / "broken.wav").write_bytes(b"not a wave file")
    (proc / "broken.wav").write_bytes(b"not a wave file")
    (proc / "extra.wav").write_bytes((proc / "a.wav").read_bytes())
    capsys.readouterr()
    assert eval_batch.main(["--ref-dir", str(ref), "--proc-dir", str(proc), "--n-fft", "512", "--hop", "64"]) == 1
    cap = capsys.readouterr()
    assert "UNPAIRED" in cap.err and "extra.wav" in cap.err and "SKIP broken" in cap.err
    assert json.loads(cap.out.splitlines()[-1])["pairs"] == 2 and len(cap.out.splitlines()) == 3
