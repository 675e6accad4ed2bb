"""Many clips in one ragged pass (egr_dfn3_enhance_tracks / egr_dfn2_enhance_tracks, DfnEngine.enhance_many): every
clip gets the bits of the single call on that clip alone, whatever shares the pass with it; the workspace follows the sum of the
lengths; nothing survives a call; what the call cannot take is refused before anything is allocated.  No tolerance anywhere:
torch.equal against eng.enhance(clip)."""
import gc

import numpy as np
import pytest
import torch

import dfn2_torch as R2
import dfn3_torch as R3
from dfn3_check import speechy
from test_gpu_dfn_segmented import CONFIGS2, CONFIGS3

pytestmark = pytest.mark.gpu

# test 1's clips, deliberately unsorted: (n, channels).  n = 17 gives 2 frames = conv_lookahead: every feature row is in the zeroed tail
CLIPS = ((4800, 2), (17, 1), (24000, 1), (480, 3), (479, 2), (3 * 480 + 17, 1))
MAX_FRAMES = 524287


def _engine(which, d):
    from egregora_amd import dfn2_engine, dfn2_weights, dfn_engine, dfn_weights
    if which == "dfn3":
        return dfn_engine.Dfn3Engine(dfn_weights.load(d), torch.cuda.current_device())
    return dfn2_engine.Dfn2Engine(dfn2_weights.load(d), torch.cuda.current_device())


@pytest.fixture(scope="module")
def models(pack, tmp_path_factory):
    """(which, config name or None) -> (directory, cfg, engine); directories and engines are made once."""
    from egregora_amd import native
    native.require_device()
    root = tmp_path_factory.mktemp("dfn_tracks")
    made = {}

    def get(which, name=None):
        if (which, name) not in made:
            R, model = (R3, "DeepFilterNet3") if which == "dfn3" else (R2, "DeepFilterNet2")
            d = root / which / (name or "default") / model
            if name is None:
                cfg, _ = R.write_model_dir(d, seed=5)
            else:
                matrix = R3.MATRIX if which == "dfn3" else R2.MATRIX2
                cfg, _ = R.write_model_dir(d, seed=11, cfg_text=R.config_text(**matrix[name]))
            made[(which, name)] = (d, cfg, _engine(which, d))
        return made[(which, name)]
    yield get
    made.clear()
    gc.collect()


@pytest.fixture(scope="module")
def default_set(models):
    """which -> (test 1's clips on the device, each clip's single-call output): computed once, never written to."""
    made = {}

    def get(which):
        if which not in made:
            eng = models(which)[2]
            clips = [speechy(3 + i, n, C).cuda() for i, (n, C) in enumerate(CLIPS)]
            made[which] = (clips, [eng.enhance(x) for x in clips])
        return made[which]
    yield get
    made.clear()


def one_call(eng, clips, gap=3):
    """The clips through ONE enhance_tracks call: a flat buffer with `gap` samples of NaN between the tracks (the table's offsets need
    not be back to back, and what lies between tracks is never read into a result) -> the clips' outputs."""
    fill = torch.full((gap,), float("nan"), device=clips[0].device)
    offs, lens, parts, pos = [], [], [fill], gap
    for x in clips:
        C, T = x.shape
        for c in range(C):
            parts += [x[c], fill]
            offs.append(pos)
            lens.append(T)
            pos += T + gap
    y = eng.enhance_tracks(torch.cat(parts), offs, lens)
    out, k = [], 0
    for x in clips:
        C, T = x.shape
        out.append(torch.stack([y[offs[k + c]:offs[k + c] + T] for c in range(C)]))
        k += C
    return out


def assert_same(got, want, what):
    """got, want: lists of [C,T] outputs.  A failure names the clip, the channel, the first differing sample and the max difference."""
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape, (what, "clip", i, tuple(a.shape), tuple(b.shape))
        ne = ~((a == b) | (torch.isnan(a) & torch.isnan(b)))          # torch.equal, with NaN equal to NaN at the same place
        if not bool(ne.any()):
            continue
        for c in range(a.shape[0]):
            if bool(ne[c].any()):
                first = int(ne[c].nonzero()[0])
                raise AssertionError((what, "clip", i, "channel", c, "first differing sample", first,
                                      "max |diff|", float((a - b).abs().nan_to_num(nan=float("inf")).max())))


# ---------------------------------------------------------------- 1
@pytest.mark.parametrize("which", ["dfn3", "dfn2"])
def test_packed_equals_alone_default_config(models, default_set, which):
    eng = models(which)[2]
    clips, want = default_set(which)
    assert all(bool(torch.isfinite(w).all()) for w in want) and float(want[2].abs().max()) > 0
    assert_same(one_call(eng, clips), want, which)
    assert_same(eng.enhance_many(clips), want, (which, "enhance_many"))


# ---------------------------------------------------------------- 2
# The clip of 1e30 has 479 samples: 2 frames = conv_lookahead, so its feature rows are all in the zeroed tail, as test 1's n = 17.
# That is the only kind of 1e30 clip whose own output float32 can hold.  With live features the unit-normalised spectrum grows with
# the square root of the amplitude (about 5e15 at 1e30) and the deep-filter coefficients, tanh(df_out) + df_convp(c0), are linear
# in it, so coefs * spec (spec about 6e29 at 1e30) is beyond float32's 3.4e38 in the single call as well: the network's own
# arithmetic, not the ragged pass.  The next test packs such a long 1e30 clip too and holds everything but its finiteness.
HUGE_N = 479


@pytest.mark.parametrize("which", ["dfn3", "dfn2"])
def test_neighbours_do_not_bleed(models, which):
    """Conv history, scan tail, deep-filter lookahead and overlap-add reads across a track boundary would all show here."""
    eng = models(which)[2]
    x = speechy(21, 4800, 2).cuda()
    want = eng.enhance(x)
    zeros = torch.zeros(1, 1900, device="cuda")
    huge = torch.full((1, HUGE_N), 1e30, device="cuda")
    nan = lambda n: torch.full((2, n), float("nan"), device="cuda")
    a = one_call(eng, [speechy(22, 3000, 1).cuda(), x, speechy(23, 700, 2).cuda()])
    b = one_call(eng, [huge, x, zeros])
    c = one_call(eng, [nan(960), x, nan(500)])
    assert_same([a[1], b[1], c[1]], [want] * 3, which)
    assert_same([b[2]], [eng.enhance(zeros)], (which, "zeros"))
    assert_same([b[0]], [eng.enhance(huge)], (which, "1e30"))
    assert float(b[0].abs().max()) > 1e25, (which, "the 1e30 clip's output is of its input's size", float(b[0].abs().max()))
    for name, ys in (("speech", a), ("1e30 / zeros", b), ("nan", [c[1]])):          # every output except the NaN clips'
        for k, y in enumerate(ys):
            assert bool(torch.isfinite(y).all()), (which, name, "clip", k, "finite share", float(torch.isfinite(y).float().mean()))


@pytest.mark.parametrize("which", ["dfn3", "dfn2"])
def test_a_long_huge_neighbour_does_not_bleed_either(models, which):
    """A 1e30 clip with live features (2000 samples, 6 frames) in front of the clip: its own output is not finite in float32, packed
    or alone (measured on these models with stage() after enhance(): spec 6.0e29, coefs 5.0e14 / 2.3e14, so 13 % of spec_e is past
    3.4e38 and the synthesis makes NaN of inf - inf; every stage before spec_e is finite), and it still has the bits of the single
    call, NaN for NaN; the clip behind it and the zero clip are untouched by its inf and NaN rows."""
    eng = models(which)[2]
    x = speechy(21, 4800, 2).cuda()
    zeros = torch.zeros(1, 1900, device="cuda")
    huge = torch.full((1, 2000), 1e30, device="cuda")
    got = one_call(eng, [huge, x, zeros])
    want = [eng.enhance(huge), eng.enhance(x), eng.enhance(zeros)]
    assert_same(got, want, which)
    assert bool(torch.isfinite(got[1]).all()) and bool(torch.isfinite(got[2]).all())


# ---------------------------------------------------------------- 3
@pytest.mark.parametrize("which,name", [("dfn3", c) for c in CONFIGS3] + [("dfn2", c) for c in CONFIGS2])
def test_packed_equals_alone_over_the_history_kinds(models, which, name):
    eng = models(which, name)[2]
    clips = [speechy(len(name), 24000, 2).cuda(), speechy(1 + len(name), 1000, 1).cuda(), speechy(2 + len(name), 17, 1).cuda()]
    want = [eng.enhance(x) for x in clips]
    assert bool(torch.isfinite(want[0]).all()) and float(want[0].abs().max()) > 0
    assert_same(one_call(eng, clips), want, (which, name))


# ---------------------------------------------------------------- 4
@pytest.mark.parametrize("which", ["dfn3", "dfn2"])
def test_more_rows_than_compute_units(models, which):
    eng = models(which)[2]
    rng = np.random.default_rng(4)
    lens = [int(n) for n in rng.integers(480, 2401, size=300)]
    base = speechy(31, sum(lens), 1).cuda()
    cuts = np.cumsum([0] + lens)
    clips = [base[:, int(cuts[i]):int(cuts[i + 1])].contiguous() for i in range(300)]
    got = one_call(eng, clips, gap=1)
    assert all(bool(torch.isfinite(y).all()) for y in got)
    pick = sorted(int(i) for i in rng.choice(300, size=20, replace=False))
    assert_same([got[i] for i in pick], [eng.enhance(clips[i]) for i in pick], (which, pick))


# ---------------------------------------------------------------- 5
@pytest.mark.parametrize("which", ["dfn3", "dfn2"])
def test_workspace_follows_the_sum(models, which):
    d, cfg, ready = models(which)
    lens = [48000] + [480] * 9                                       # 102 + 9 * 3 = 129 frames; 10 x 48000 would be 1020
    need = ready.tracks_workspace_bytes(lens)
    assert 0 < need < ready.workspace_bytes(10, 48000) / 4
    assert ready.tracks_workspace_bytes(lens + [480]) > need
    assert ready.tracks_workspace_bytes(lens[:-1]) < need
    eng = _engine(which, d)                                          # a fresh handle: it holds nothing yet
    try:
        assert eng.workspace_held() == 0
        x = speechy(5, sum(lens), 1).cuda().reshape(-1)
        offs = [int(o) for o in np.cumsum([0] + lens[:-1])]
        y = eng.enhance_tracks(x, offs, lens)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(y).all())
        assert eng.workspace_held() == need
    finally:
        del eng
        gc.collect()


# ---------------------------------------------------------------- 6
@pytest.mark.parametrize("which", ["dfn3", "dfn2"])
def test_nothing_survives_a_call(models, default_set, which):
    d, cfg, eng = models(which)
    clips, want = default_set(which)
    x = clips[0]
    one, seg = eng.enhance(x), eng.enhance(x, seg_frames=7)
    assert torch.equal(one, want[0]) and torch.equal(seg, want[0])
    first = one_call(eng, clips)
    with pytest.raises(RuntimeError, match="stages belong to one-pass calls"):
        eng.stage("mask")
    again = one_call(eng, clips)
    assert_same(again, first, (which, "twice"))
    assert_same(first, want, which)
    assert torch.equal(eng.enhance(x, seg_frames=7), seg)             # segmented right after a tracks call
    one_call(eng, clips[3:])
    assert torch.equal(eng.enhance(x), one)                           # one pass right after a tracks call
    assert eng.stage("mask").numel() == ((x.shape[1] + cfg["fft_size"]) // cfg["hop_size"]) * x.shape[0] * cfg["nb_erb"]
    assert_same(one_call(eng, clips), want, (which, "after the others"))


# ---------------------------------------------------------------- 7
@pytest.mark.parametrize("which", ["dfn3", "dfn2"])
def test_refusals(models, which):
    d, cfg, eng = models(which)
    eng.enhance(speechy(1, 480, 1).cuda())
    held = eng.workspace_held()
    x = torch.zeros(1, device="cuda")                                 # the checks come before any read: lengths only
    hop = cfg["hop_size"]
    lens = [hop * 180000] * 3                                         # 3 x 180002 frames, each track within the limit on its own
    assert all((n + cfg["fft_size"]) // hop <= MAX_FRAMES for n in lens) and sum((n + cfg["fft_size"]) // hop for n in lens) > MAX_FRAMES
    with pytest.raises(RuntimeError, match="frames"):
        eng.enhance_tracks(x, [0, 0, 0], lens)
    assert eng.tracks_workspace_bytes(lens) == 0
    assert eng.tracks_workspace_bytes(lens[:2]) > 0                   # 360004 frames are within the limit
    with pytest.raises(RuntimeError):
        eng.enhance_tracks(x, [0, 0], [1, 0])                         # n = 0
    with pytest.raises(RuntimeError):
        eng.enhance_tracks(x, [-1], [1])
    with pytest.raises(RuntimeError):
        eng.enhance_tracks(x, [], [])                                 # n_tracks = 0
    assert eng.tracks_workspace_bytes([]) == 0 and eng.tracks_workspace_bytes([4, 0]) == 0
    torch.cuda.synchronize()
    assert eng.workspace_held() == held


# ---------------------------------------------------------------- 8
@pytest.mark.parametrize("which", ["dfn3", "dfn2"])
def test_enhance_many_across_waves(models, default_set, which, monkeypatch):
    """A budget of the 3-channel 480-sample clip plus the 17-sample one (11 frames): the 24000-sample and the 4800-sample clips are
    over it alone and go through enhance(), the other four need three waves.  enhance() cuts in multiples of SEGMENT_STEP frames and
    its smallest segment (64 frames) is more than this whole clip set, so the step is lowered for the test; the budget holds for
    both paths."""
    from egregora_amd import dfn_engine
    eng = models(which)[2]
    clips, want = default_set(which)
    budget = eng.tracks_workspace_bytes([480] * 3 + [17])
    monkeypatch.setattr(dfn_engine, "SEGMENT_STEP", 2)
    assert eng.segment_workspace_bytes(2, 2) <= budget < eng.tracks_workspace_bytes([24000])
    monkeypatch.setenv(dfn_engine.WORKSPACE_GB_ENV, repr(budget / 2 ** 30))
    assert dfn_engine.workspace_budget_bytes() == budget
    stats = {}
    got = eng.enhance_many(clips, stats=stats)
    assert len(stats["waves"]) >= 3 and 2 in stats["alone"], stats
    assert sorted([i for w in stats["waves"] for i in w] + stats["alone"]) == list(range(len(clips)))
    assert_same(got, want, (which, stats))
