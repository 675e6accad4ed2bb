"""The windowed-sinc resampler on the device (csrc/egr_resample_sinc.hip, SPEC.md 4f) against the float64 yardstick of
tests/sinc_refs.py, and its call forms against each other bit for bit: staged vs direct variant, many-clip vs single call, the node
switch, the codec helper, resample_many and the batch node."""
import numpy as np
import pytest
import torch

import sinc_refs as R

pytestmark = pytest.mark.gpu

WINDOWS = [("sinc_interp_hann", None), ("sinc_interp_kaiser", 5.0), ("sinc_interp_kaiser", 14.769)]
NODE = dict(lowpass_filter_width=64, rolloff=0.945, method="sinc_interp_kaiser")


def _check(got, x, src, dst, lpw, rolloff, method, beta, what):
    want, bound = R.resample_f64(x, src, dst, lpw, rolloff, method, beta)
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{what}: max |diff| {err.max():.3e}, largest share of the bound {worst:.3f}")
    assert np.isfinite(got).all() and (err <= bound).all(), (what, float(err.max()), worst)


@pytest.mark.parametrize("method,beta", WINDOWS)
@pytest.mark.parametrize("case", R.CASES, ids=[f"{c[0][0]}to{c[0][1]}" for c in R.CASES])
def test_parity_with_the_float64_definition(pack, case, method, beta):
    """Every output within (S + 1) 2^-24 sum |K32 x| + L 2^-50 max|x| of the full-kernel float64 conv1d.  The grids of all four
    kernels equal the work count (one thread per output, no stride loop), so there is no lap to pass."""
    from egregora_amd import resample
    (src, dst, lpw, rolloff), (o, n, width) = case
    assert resample.design_sinc(src, dst, lpw, rolloff, method, beta)[2][:3] == (o, n, width)
    for N in R.lengths(o, n):
        for C in (1, 2):
            x = R.signal(C, N, 100 + N + C)
            y = resample.resample_sinc(torch.from_numpy(x).cuda(), src, dst, lowpass_filter_width=lpw, rolloff=rolloff, method=method,
                                       beta=beta)
            assert y.shape == (C, -(-N * n // o))
            _check(y, x, src, dst, lpw, rolloff, method, beta, f"{src}->{dst} {method} {beta} C={C} N={N}")


@pytest.mark.parametrize("case", [c for c in R.CASES if c[0][:2] != (8000, 8001)], ids=lambda c: f"{c[0][0]}to{c[0][1]}")
def test_direct_variant_forced_equals_staged_bit_for_bit(pack, case):
    from egregora_amd import resample
    (src, dst, lpw, rolloff), (o, n, width) = case
    assert resample.sinc_staged(o, n, width)
    kw = dict(lowpass_filter_width=lpw, rolloff=rolloff, method="sinc_interp_kaiser", beta=14.769)
    for N in R.lengths(o, n) + [20000]:
        x = torch.from_numpy(R.signal(2, N, 7 + N)).cuda()
        a = resample.resample_sinc(x, src, dst, **kw)
        b = resample.resample_sinc(x, src, dst, flags=resample.SINC_FORCE_DIRECT, **kw)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (src, dst, N)


def test_direct_variant_taken_by_itself_meets_the_bound(pack):
    """96:1 at lowpass_filter_width 64: width 6502, 13006 taps per output; the span of a tile is far above the LDS budget."""
    from egregora_amd import resample
    src, dst, lpw, rolloff = 384000, 4000, 64, 0.945
    _, _, (o, n, width, run) = resample.design_sinc(src, dst, lpw, rolloff, "sinc_interp_kaiser", 14.769)
    assert (o, n, width) == (96, 1, 6502) and run <= 2 * width + 2 and not resample.sinc_staged(o, n, width)
    assert not resample.sinc_staged(8000, 8001, 7)
    x = R.signal(2, 3000, 5)
    y = resample.resample_sinc(torch.from_numpy(x).cuda(), src, dst, lowpass_filter_width=lpw, rolloff=rolloff, method="sinc_interp_kaiser",
                               beta=14.769)
    _check(y, x, src, dst, lpw, rolloff, "sinc_interp_kaiser", 14.769, "384000->4000")


TRACK_CLIPS = [(1, 1), (2, 100), (1, 257), (3, 300), (1, 1), (2, 1000), (1, 2), (2, 5000), (1, 777)]       # (channels, samples)


@pytest.mark.parametrize("flags", [0, 1], ids=["own_variant", "forced_direct"])
@pytest.mark.parametrize("src,dst,kw", [(44100, 48000, dict(NODE, beta=14.769)), (48000, 32000, dict(NODE, beta=5.0)),
                                        (16000, 48000, {}), (8000, 8001, {})], ids=["44k1to48k", "48kto32k", "16kto48k", "8000to8001"])
def test_tracks_equal_the_single_call_bit_for_bit(pack, src, dst, kw, flags):
    """Ragged clips (one sample among them) whose outputs start inside 256-output tiles.  The input buffer carries NaN in front of,
    between and behind the tracks -- a read outside a clip would poison an output -- and the output buffer carries sentinels in
    front of and behind the written stretch; both must be intact."""
    from egregora_amd import resample
    dev = torch.device("cuda")
    table, first_tap, geo = resample.sinc_filter_for(dev, src, dst, **kw)
    o, n, width, run = geo
    xs = [torch.from_numpy(R.signal(c, T, 40 + i)) for i, (c, T) in enumerate(TRACK_CLIPS)]
    gap = 37
    parts, ins, lens, pos = [torch.full((gap,), float("nan"))], [], [], gap
    for x in xs:
        for c in range(x.shape[0]):
            parts += [x[c], torch.full((gap,), float("nan"))]
            ins.append(pos)
            lens.append(x.shape[1])
            pos += x.shape[1] + gap
    flat = torch.cat(parts).cuda()
    nan_at = torch.isnan(flat).clone()
    tab, total = resample.sinc_track_table(ins, lens, o, n)
    starts = tab[:, 2] % 256
    assert (starts != 0).sum() >= 4 and total > 3 * 256                     # several tracks start inside a tile
    front = 5
    ybuf = torch.full((front + total + 300,), -7.0, device=dev)
    resample.sinc_tracks(flat, torch.from_numpy(tab).cuda(), total, geo, table, first_tap, ybuf[front:], flags)
    torch.cuda.synchronize()
    assert bool((ybuf[:front] == -7.0).all()) and bool((ybuf[front + total:] == -7.0).all())
    assert torch.equal(torch.isnan(flat), nan_at) and int(nan_at.sum()) == gap * (len(ins) + 1)
    y = ybuf[front:front + total]
    assert bool(torch.isfinite(y).all())
    t = 0
    for x in xs:
        want = resample.resample_sinc(x.cuda(), src, dst, **kw)
        for c in range(x.shape[0]):
            off, n_out = int(tab[t, 2]), int(tab[t, 3])
            assert n_out == want.shape[1]
            assert torch.equal(y[off:off + n_out].view(torch.int32), want[c].view(torch.int32)), (src, dst, flags, tuple(x.shape), c)
            t += 1
    got = resample.resample_sinc_group([x.cuda() for x in xs], src, dst, flags=flags, **kw)
    for x, g in zip(xs, got):
        assert torch.equal(g, resample.resample_sinc(x.cuda(), src, dst, **kw))


def _audio(x, sr):
    return {"waveform": torch.from_numpy(x)[None], "sample_rate": sr}


def test_node_torchaudio_mode_follows_the_switch(pack, monkeypatch):
    from egregora_amd import device_ops, resample
    node = pack.NODE_CLASS_MAPPINGS["Resample Audio (HQ)"]()
    x = R.signal(2, 4410, 3)
    xd = torch.from_numpy(x).cuda()
    monkeypatch.delenv("EGREGORA_SINC_RESAMPLE", raising=False)
    off = node.execute(_audio(x, 44100), 48000, "torchaudio", 9.0)[0]
    want = device_ops.resample_linear(xd, int(round(4410 * (48000 / 44100)))).cpu().numpy()
    assert off["sample_rate"] == 48000 and np.array_equal(off["samples"], want)
    monkeypatch.setenv("EGREGORA_SINC_RESAMPLE", "1")                       # read at call time: same node object
    outs = {}
    for beta in (9.0, 14.769):
        got = node.execute(_audio(x, 44100), 48000, "torchaudio", beta)[0]
        want = resample.resample_sinc(xd, 44100, 48000, lowpass_filter_width=64, rolloff=0.945, method="sinc_interp_kaiser", beta=beta)
        assert got["sample_rate"] == 48000 and np.array_equal(got["samples"], want.cpu().numpy())
        _check(want, x, 44100, 48000, 64, 0.945, "sinc_interp_kaiser", beta, f"node beta {beta}")
        outs[beta] = got["samples"]
    assert outs[9.0].shape == outs[14.769].shape == (2, 4800) and not np.array_equal(outs[9.0], outs[14.769])
    for mode in ("auto", "scipy_polyphase"):                                # untouched by the switch
        got = node.execute(_audio(x, 44100), 48000, mode, 9.0)[0]
        assert np.array_equal(got["samples"], resample.resample_hq(xd, 44100, 48000).cpu().numpy())
    got = node.execute(_audio(x, 44100), 48000, "linear", 9.0)[0]
    assert np.array_equal(got["samples"], off["samples"])


def test_codec_helper_follows_the_switch(pack, monkeypatch):
    from egregora_amd import resample
    xs = [torch.from_numpy(R.signal(c, T, 60 + T)).cuda() for c, T in ((1, 1), (2, 3000), (1, 4411))]
    monkeypatch.delenv("EGREGORA_SINC_RESAMPLE", raising=False)
    assert not resample.reference_torchaudio_enabled()
    for x, g in zip(xs, resample.codec_resample(xs, 48000, 44100)):
        assert torch.equal(resample.codec_resample(x, 48000, 44100), resample.resample_hq(x, 48000, 44100))
        assert torch.equal(g, resample.resample_hq(x, 48000, 44100))
    monkeypatch.setenv("EGREGORA_SINC_RESAMPLE", "1")
    assert resample.reference_torchaudio_enabled()
    for x, g in zip(xs, resample.codec_resample(xs, 48000, 44100)):
        want = resample.resample_sinc(x, 48000, 44100)                      # torchaudio's defaults: Hann, 6, 0.99
        assert torch.equal(resample.codec_resample(x, 48000, 44100), want) and torch.equal(g, want)
        assert not torch.equal(want, resample.resample_hq(x, 48000, 44100)) or x.shape[1] == 1
        _check(want, x.cpu().numpy(), 48000, 44100, 6, 0.99, "sinc_interp_hann", None, f"codec {tuple(x.shape)}")


MANY = [(1, 1, 16000), (2, 20000, 44100), (1, 4097, 22050), (2, 333, 16000), (1, 9000, 48000), (2, 2, 44100), (1, 12345, 22050)]


@pytest.mark.parametrize("mode", ["torchaudio", "scipy_polyphase"])
def test_resample_many_and_batch_node(pack, monkeypatch, mode):
    """Three source rates, mono and stereo, 1 to 20 000 samples, one clip already at the target: the bits of the single call per clip
    and one library call per distinct source rate."""
    from egregora_amd import egregora_audio_resample_batch as nb, native, resample, resample_many as rm
    clips = [(torch.from_numpy(R.signal(c, T, 80 + i)), sr) for i, (c, T, sr) in enumerate(MANY)]
    L = native.lib()
    calls = {"egr_resample_sinc_tracks": 0, "egr_resample_poly_tracks": 0}

    def counted(name):
        real = getattr(L, name)

        def f(*a):
            calls[name] += 1
            return real(*a)
        return f
    for name in calls:
        monkeypatch.setattr(L, name, counted(name), raising=False)
    stats = {}
    ys = rm.resample_many(clips, 48000, mode, 11.0, stats=stats)
    mine, other = ("egr_resample_sinc_tracks", "egr_resample_poly_tracks") if mode == "torchaudio" else \
        ("egr_resample_poly_tracks", "egr_resample_sinc_tracks")
    assert calls[mine] == 3 == stats["calls"] and calls[other] == 0 and stats["groups"] == {16000: 2, 44100: 2, 22050: 2}

    def single(x, sr):
        if sr == 48000:
            return x
        if mode == "torchaudio":
            return resample.resample_sinc(x.cuda(), sr, 48000, beta=11.0, **rm.NODE_FILTER).cpu()
        return resample.resample_hq(x.cuda(), sr, 48000).cpu()
    for (x, sr), y in zip(clips, ys):
        assert not y.is_cuda and torch.equal(y, single(x, sr)), (mode, tuple(x.shape), sr)
    # the list node: a [B,C,T] dict counts as B clips
    stack = {"waveform": torch.stack([clips[1][0][:, :500], clips[5][0].repeat(1, 250)]), "sample_rate": 44100}
    before = dict(calls)
    res = nb.Resample_Audio_HQ_Batch().execute([_audio(clips[0][0].numpy(), 16000), stack, _audio(clips[4][0].numpy(), 48000)], [48000], [mode],
                                               [11.0])[0]
    assert len(res) == 4 and calls[mine] - before[mine] == 2 and calls[other] == 0
    for a, (x, sr) in zip(res, [clips[0], (stack["waveform"][0], 44100), (stack["waveform"][1], 44100), clips[4]]):
        assert a["sample_rate"] == 48000 and np.array_equal(a["samples"], single(x.contiguous(), sr).numpy())
