"""FlashSR's packed path on the device: the three many-track glue kernels bit for bit against the per-clip entry points, and
flashsr_engine.upscale_many against oracles built from existing functions (tiny layer table, win = 3840, hop = win - 375)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

WIN, HOP = 3840, 3840 - 375
# the lengths around the chunk boundaries (1, 1, 1, 2, 2 and 3 chunks) and one longer clip
LENGTHS = (1, 3839, 3840, 3841, WIN + HOP, WIN + HOP + 1, 20000)
# seven clips mixing 1, 2 and 3 channels, one per length
SHAPES = tuple(zip((1, 2, 3, 1, 2, 3, 1), LENGTHS))
BOUND = 2e-5        # tests/test_devices_partition.py: tile choice follows a forward's row count


def _rand(shape, seed):
    return 0.3 * torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _layout(shapes):
    """Clips back to back in one flat buffer -> (offsets, total)."""
    offs, pos = [], 0
    for Cn, T in shapes:
        offs.append(pos)
        pos += Cn * T
    return offs, pos


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def test_chunk_gather_tracks_equals_chunk_gather_per_clip(pack):
    from egregora_amd import device_ops as ops, flashsr_engine as E
    shapes = SHAPES
    offs, total = _layout(shapes)
    xs = [_rand(s, 10 + i).cuda() for i, s in enumerate(shapes)]
    flat = torch.cat([x.reshape(-1) for x in xs])
    t = E.wave_tables(shapes, offs, WIN, HOP)
    rows = ops.chunk_gather_tracks(flat, torch.from_numpy(t["rows"]).cuda(), WIN, HOP)
    want = torch.cat([ops.chunk_gather(x, WIN, HOP, 0, E.n_chunks_for(x.shape[1], WIN, HOP)).view(-1, WIN) for x in xs])
    assert rows.shape == want.shape == (t["n_rows"], WIN) and torch.equal(rows, want)


@pytest.mark.parametrize("lp", [WIN, WIN - 7])
def test_wola_tracks_equals_wola_stitch_per_clip(pack, lp):
    from egregora_amd import device_ops as ops, flashsr_engine as E
    shapes = SHAPES
    offs, _ = _layout(shapes)
    t = E.wave_tables(shapes, offs, WIN, HOP)
    preds = _rand((t["n_rows"], lp), 3).cuda()
    got = ops.wola_tracks(preds, torch.from_numpy(t["tracks"]).cuda(), t["total_out"], WIN, HOP)
    assert got.numel() == t["total_out"]
    r = 0
    for (Cn, T), (off, _, _) in zip(shapes, t["clip_out"]):
        n = E.n_chunks_for(T, WIN, HOP)
        want = ops.wola_stitch(preds[r:r + n * Cn].view(n, Cn, lp).contiguous(), T, WIN, HOP)
        assert torch.equal(got[off:off + Cn * T].view(Cn, T), want), (Cn, T, lp)
        r += n * Cn


@pytest.mark.parametrize("src,dst,lens", [(16000, 48000, (1, 2, 9, 10, 11, 4001)), (44100, 48000, (1, 10, 11, 1470, 5000)),
                                          (48000, 44100, (1, 10, 11, 1470, 5000))])
def test_resample_poly_tracks_equals_resample_hq(pack, src, dst, lens):
    from egregora_amd import device_ops as ops, flashsr_engine as E, resample
    up, down = resample.rates(src, dst)
    assert (up, down) == {(16000, 48000): (3, 1), (44100, 48000): (160, 147), (48000, 44100): (147, 160)}[(src, dst)]
    chans = [1 + i % 3 for i in range(len(lens))]                                       # 1, 2, 3, 1, 2(, 3) channels
    xs = [_rand((c, n), 20 + i).cuda() for i, (c, n) in enumerate(zip(chans, lens))]
    flat = torch.cat([x.reshape(-1) for x in xs] + [torch.zeros(3, device="cuda")])
    ins, n_ins, pos = [], [], 0
    for x in xs:
        for c in range(x.shape[0]):
            ins.append(pos + c * x.shape[1])
            n_ins.append(x.shape[1])
        pos += x.numel()
    tab, total = resample.poly_track_table(ins, n_ins, up, down)
    h, half = resample.filter_for(up, down, flat.device)
    assert half == 10 * max(up, down)
    y = torch.full((total + 5,), 7.0, device="cuda")
    ops.resample_poly_tracks(flat, torch.from_numpy(tab).cuda(), total, up, down, h, half, y)
    assert bool((y[total:] == 7.0).all())                                                # nothing behind total_out is written
    o = 0
    for x in xs:
        want = resample.resample_hq(x, src, dst)
        assert torch.equal(y[o:o + want.numel()].view(want.shape), want), (src, dst, tuple(x.shape))
        o += want.numel()
    assert o == total


# ---------------------------------------------------------------- engine
@pytest.fixture(scope="module")
def tiny(pack):
    from egregora_amd import flashsr_arch as A, flashsr_engine as E
    cfg = A.tiny_config()
    assert cfg.chunk == WIN
    eng = E.FlashSREngine(cfg, A.init_params(cfg, 0))
    E.set_engine(eng)
    yield eng
    E.set_engine(None)
    eng.close()


def _mixed_clips():
    """Ten clips: rates 16 000, 44 100 and 48 000, mono and stereo, 1 to 13 chunks at 48 kHz (one clip of a single sample): 2, 2, 4, 18, 2, 3,
    12, 1, 2 and 26 rows, three waves at max_rows = 32."""
    spec = [(2, 3840, 48000), (1, 1281, 16000), (2, 3530, 44100), (2, 30000, 48000), (2, 1280, 16000), (1, 6800, 44100),
            (2, 20000, 48000), (1, 1, 16000), (1, 3841, 48000), (2, 14000, 16000)]
    return [(_rand((c, n), 40 + i), sr) for i, (c, n, sr) in enumerate(spec)]


@pytest.fixture(scope="module")
def mixed(tiny):
    """The mixed list, each clip's single-clip result (infer_spans + wola_stitch, the node's flow) and the packed results."""
    from egregora_amd import audio_glue as ag, device_ops as ops, flashsr_engine as E, resample
    clips = _mixed_clips()
    alone = {}
    for lowpass in (False, True):
        outs = []
        for x, sr in clips:
            x48 = resample.resample_hq(x.cuda(), sr, 48000)
            n = len(ag.spans(x48.shape[1], WIN, HOP))
            outs.append(ops.wola_stitch(E.infer_spans(x48, n, WIN, HOP, lowpass), x48.shape[1], WIN, HOP).cpu())
        alone[lowpass] = outs
    return clips, alone


def _oracle(eng, clips, lowpass, max_rows):
    """Per wave of plan_waves: resample_hq and chunk_gather per clip, ONE infer_rows on the concatenated rows and ids, wola_stitch
    per clip -- existing functions only."""
    from egregora_amd import device_ops as ops, flashsr_engine as E, resample
    x48 = [resample.resample_hq(x.cuda(), sr, 48000) for x, sr in clips]
    counts = [x.shape[0] * E.n_chunks_for(x.shape[1], WIN, HOP) for x in x48]
    out = [None] * len(clips)
    for wave in E.plan_waves(counts, max_rows):
        rows, ids = [], []
        for i in wave:
            Cn, T = x48[i].shape
            n = E.n_chunks_for(T, WIN, HOP)
            rows.append(ops.chunk_gather(x48[i], WIN, HOP, 0, n).view(-1, WIN))
            ids.append(torch.arange(n * Cn, dtype=torch.int64, device="cuda"))           # k * C + c in chunk-major, channel order
        preds = E.infer_rows(eng, torch.cat(rows), torch.cat(ids), E.SEED, lowpass=lowpass)
        r = 0
        for i in wave:
            Cn, T = x48[i].shape
            n = E.n_chunks_for(T, WIN, HOP)
            out[i] = ops.wola_stitch(preds[r:r + n * Cn].view(n, Cn, WIN).contiguous(), T, WIN, HOP).cpu()
            r += n * Cn
    return out


@pytest.mark.parametrize("lowpass", [False, True])
def test_upscale_many_equals_the_per_wave_oracle_bit_for_bit(tiny, mixed, lowpass):
    from egregora_amd import flashsr_engine as E
    clips, alone = mixed
    stats = {}
    got = E.upscale_many(clips, lowpass, win=WIN, hop=HOP, max_rows=32, eng=tiny, stats=stats)
    want = _oracle(tiny, clips, lowpass, 32)
    assert stats["waves"] == [[0, 1, 2, 3, 4, 5], [6, 7, 8], [9]] and stats["rows"] == [31, 15, 26] and [i for w in stats["waves"] for i in w] == list(range(len(clips)))
    assert len(got) == len(clips)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.device.type == "cpu" and g.dtype == torch.float32 and g.shape == w.shape and torch.equal(g, w), i
    # alone against packed: the same rows in forwards of other row counts
    for i, (g, a) in enumerate(zip(got, alone[lowpass])):
        rel = _rel(g, a)
        print(f"clip {i} lowpass={lowpass}: packed vs alone rel L2 {rel:.3e}")
        assert g.shape == a.shape and rel < BOUND, (i, rel)


def test_one_clip_equals_the_single_clip_path_bit_for_bit(tiny, mixed):
    from egregora_amd import flashsr_engine as E
    clips, alone = mixed
    for i in (0, 2, 6, 7):
        (got,) = E.upscale_many([clips[i]], False, win=WIN, hop=HOP, eng=tiny)
        assert torch.equal(got, alone[False][i]), i
    # a clip that already lies on the device, and output_sr != 48000 as the node's second resample
    from egregora_amd import resample
    x, sr = clips[2]
    (got,) = E.upscale_many([(x.cuda(), sr)], False, 44100, win=WIN, hop=HOP, eng=tiny)
    assert torch.equal(got, resample.resample_hq(alone[False][2].cuda(), 48000, 44100).cpu())


def test_order_independence_and_input_order(tiny, mixed):
    from egregora_amd import flashsr_engine as E
    clips, alone = mixed
    s1, s2 = {}, {}
    fwd = E.upscale_many(clips, False, win=WIN, hop=HOP, max_rows=1024, eng=tiny, stats=s1)
    rev = E.upscale_many(clips[::-1], False, win=WIN, hop=HOP, max_rows=1024, eng=tiny, stats=s2)
    assert s1["waves"] == [list(range(len(clips)))] and s2["waves"] == s1["waves"] and s1["rows"] == s2["rows"]
    for i, (a, b) in enumerate(zip(fwd, rev[::-1])):
        rel = _rel(b, a)
        print(f"clip {i}: reversed vs forward rel L2 {rel:.3e}")
        assert a.shape == b.shape == alone[False][i].shape and rel < BOUND, (i, rel)
        assert _rel(a, alone[False][i]) < BOUND


def test_library_calls_follow_rates_not_clips(tiny):
    from egregora_amd import flashsr_engine as E
    three = [(_rand((1, 1300), 1), 16000), (_rand((2, 3600), 2), 44100), (_rand((1, 3900), 3), 48000)]
    twelve = [(_rand((1 + i % 2, 1200 + 37 * i), 50 + i), (16000, 44100, 48000)[i % 3]) for i in range(12)]
    s3, s12 = {}, {}
    E.upscale_many(three, False, win=WIN, hop=HOP, max_rows=1024, eng=tiny, stats=s3)
    E.upscale_many(twelve, False, win=WIN, hop=HOP, max_rows=1024, eng=tiny, stats=s12)
    assert len(s3["waves"]) == len(s12["waves"]) == 1
    assert s3["library_calls"] == s12["library_calls"] == [5]          # two resampled rates + gather + infer + WOLA
    s = {}
    E.upscale_many(twelve, False, 44100, win=WIN, hop=HOP, max_rows=1024, eng=tiny, stats=s)
    assert s["library_calls"] == [6]                                   # + the output resample
    s = {}
    E.upscale_many([c for c in twelve if c[1] == 48000], False, win=WIN, hop=HOP, max_rows=1024, eng=tiny, stats=s)
    assert s["library_calls"] == [3]


def test_a_clip_without_samples_takes_the_single_clip_path(tiny, mixed):
    from egregora_amd import egregora_audio_super_resolution as node, flashsr_engine as E
    clips, alone = mixed
    empty = torch.zeros(2, 0)
    lst = [clips[0], (empty, 48000), clips[3]]
    stats = {}
    got = E.upscale_many(lst, False, win=WIN, hop=HOP, eng=tiny, stats=stats)
    want = node.upscale_48k(empty.cuda(), False).cpu()                 # the single-clip path's answer: [1, 1] zeros
    assert tuple(want.shape) == (1, 1) and torch.equal(got[1], want)
    assert stats["waves"] == [[0, 2]]
    both = E.upscale_many([clips[0], clips[3]], False, win=WIN, hop=HOP, eng=tiny)
    assert torch.equal(got[0], both[0]) and torch.equal(got[2], both[1])
    # a clip the single-clip path rejects gets that path's error, with its place in the list
    with pytest.raises(RuntimeError, match=r"clip 1: .*egr_resample_poly"):
        E.upscale_many([clips[0], (empty, 16000)], False, win=WIN, hop=HOP, eng=tiny)
    with pytest.raises(RuntimeError, match=r"clip 2: "):
        E.upscale_many([clips[0], clips[3], (torch.zeros(5), 16000)], False, win=WIN, hop=HOP, eng=tiny)
