"""Long inputs in segments (egr_dfn3_enhance_segmented / egr_dfn2_enhance_segmented): the segmented pass gives the
bits of the one-pass call, whatever the segment length, for both models and over every kind of history a cut has to carry; its
workspace follows the segment length, not the input's; nothing survives a call.  No tolerance anywhere: torch.equal."""
import gc

import pytest
import torch

import dfn2_torch as R2
import dfn3_torch as R3
from dfn3_check import speechy

pytestmark = pytest.mark.gpu

# every kind of history: conv_kernel / conv_kernel_inp / pathway rows, both lookaheads (and none), deep-filter orders, overlap 2 and 4,
# layer counts, widths, the grouped / dense / shuffled GRUs
CONFIGS3 = ("conv_kernel_2_3", "hop240", "conv_la4", "lookaheads0", "pad_none", "order1_la0", "order3_la2", "pathway_kt1", "layers4_3",
            "H100_100_lin4", "cornerA", "cornerB")
CONFIGS2 = ("gru_groups1", "gru_groups16", "shuffle", "h12", "skip_grouped", "conv_kernel_2_3", "hop240", "conv_la0", "conv_la4",
            "order3_la1", "cornerA", "cornerB")


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
    root = tmp_path_factory.mktemp("dfn_seg")
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


def frames_of(cfg, n):
    return (n + cfg["fft_size"]) // cfg["hop_size"]


def differing(a, b):
    """Where two outputs differ, for the failure message: (first differing sample per channel, max |a - b|)."""
    ne = (a != b)
    return [int(ne[c].nonzero()[0]) if bool(ne[c].any()) else None for c in range(a.shape[0])], float((a - b).abs().max())


@pytest.mark.parametrize("C", [1, 2, 3])
@pytest.mark.parametrize("which", ["dfn3", "dfn2"])
def test_bit_identity_default_config(models, which, C):
    d, cfg, eng = models(which)
    for n in (17, 3 * cfg["hop_size"] + 17, 48000):
        nF = frames_of(cfg, n)
        x = speechy(C + n % 11, n, C).cuda()
        want = eng.enhance(x)
        assert bool(torch.isfinite(want).all()) and (n < 1000 or float(want.abs().max()) > 0)
        for s in sorted({s for s in (1, 3, 32, nF - 1, nF, nF + 5) if s >= 1}):
            got = eng.enhance(x, seg_frames=s)
            assert torch.equal(want, got), (which, C, n, s, differing(want, got))


@pytest.mark.parametrize("which,name", [("dfn3", c) for c in CONFIGS3] + [("dfn2", c) for c in CONFIGS2])
def test_bit_identity_over_the_history_kinds(models, which, name):
    d, cfg, eng = models(which, name)
    x = speechy(len(name), 24000, 2).cuda()
    want = eng.enhance(x)
    assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0
    for s in (1, 7):
        got = eng.enhance(x, seg_frames=s)
        assert torch.equal(want, got), (which, name, s, differing(want, got))


@pytest.mark.parametrize("which", ["dfn3", "dfn2"])
def test_workspace_follows_the_segment_not_the_input(models, which):
    d, cfg, _ = models(which)
    eng = _engine(which, d)                                   # a fresh handle: it holds nothing yet
    try:
        assert eng.workspace_held() == 0
        n = 192000
        x = speechy(3, n, 2).cuda()
        y = eng.enhance(x, seg_frames=32)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(y).all())
        assert eng.workspace_held() == eng.segment_workspace_bytes(2, 32)
        assert eng.workspace_held() < eng.workspace_bytes(2, n) / 4
        assert eng.segment_workspace_bytes(2, 32) < eng.segment_workspace_bytes(2, 64) < eng.segment_workspace_bytes(3, 64)
    finally:
        del eng
        gc.collect()


def test_no_state_leaks_between_calls_or_engines(models):
    _, cfg3, e3 = models("dfn3")
    _, cfg2, e2 = models("dfn2")
    xa, xb = speechy(41, 30000, 2).cuda(), speechy(42, 21000, 2).cuda()
    for eng in (e3, e2):
        wa, wb = eng.enhance(xa), eng.enhance(xb)
        # segmented, one pass, segmented
        assert torch.equal(eng.enhance(xa, seg_frames=5), wa)
        assert torch.equal(eng.enhance(xa), wa)
        assert torch.equal(eng.enhance(xa, seg_frames=5), wa)
        # segmented twice in a row on different inputs, then the first again (other lengths, other segment counts)
        assert torch.equal(eng.enhance(xa, seg_frames=9), wa)
        assert torch.equal(eng.enhance(xb, seg_frames=9), wb)
        assert torch.equal(eng.enhance(xa, seg_frames=9), wa)
    # the two models' calls interleaved
    w3, w2 = e3.enhance(xa), e2.enhance(xa)
    got = [e3.enhance(xa, seg_frames=4), e2.enhance(xa, seg_frames=6), e3.enhance(xb, seg_frames=6), e2.enhance(xb, seg_frames=4),
           e3.enhance(xa, seg_frames=6), e2.enhance(xa, seg_frames=4)]
    assert torch.equal(got[0], w3) and torch.equal(got[4], w3) and torch.equal(got[1], w2) and torch.equal(got[5], w2)
    assert torch.equal(got[2], e3.enhance(xb)) and torch.equal(got[3], e2.enhance(xb))


@pytest.mark.parametrize("which", ["dfn3", "dfn2"])
def test_surface(models, which):
    d, cfg, eng = models(which)
    x = speechy(2, 4800, 1).cuda()
    want = eng.enhance(x)
    assert eng.stage("mask").numel() == frames_of(cfg, 4800) * cfg["nb_erb"]
    assert torch.equal(eng.enhance(x, seg_frames=4), want)
    with pytest.raises(RuntimeError, match="stages belong to one-pass calls"):
        eng.stage("mask")
    with pytest.raises(RuntimeError, match="seg_frames"):
        eng.enhance(x, seg_frames=0)
    assert torch.equal(eng.enhance(x), want)
    assert eng.stage("mask").numel() == frames_of(cfg, 4800) * cfg["nb_erb"]          # stages are back after a one-pass call
    assert eng.segment_plan(4800, 4, 0).net_hi == 4


def test_node_takes_the_segmented_path_under_a_small_budget(pack, models, monkeypatch):
    """The node calls enhance(x48): with a workspace budget below the one-pass need it runs in 64-frame segments, same waveform."""
    from egregora_amd import dfn_engine
    d, cfg, eng = models("dfn2")                              # the node's default model
    monkeypatch.setenv("EGREGORA_DFN_MODEL_DIR", str(d))
    chosen = []
    real = dfn_engine.choose_path

    def spy(*a):
        chosen.append(real(*a))
        return chosen[-1]
    monkeypatch.setattr(dfn_engine, "choose_path", spy)
    x = speechy(9, 2 * 48000, 2)
    A = {"waveform": x[None], "sample_rate": 48000, "meta": {}}
    node = pack.NODE_CLASS_MAPPINGS["Egregora_DeepFilterNet_Denoise"]()
    monkeypatch.delenv(dfn_engine.WORKSPACE_GB_ENV, raising=False)
    (one,) = node.execute(A)
    assert chosen == [None]
    # between the needs of 64 and of 128 frames, below the one-pass need of the 2 s
    budget = eng.segment_workspace_bytes(2, 96)
    assert eng.segment_workspace_bytes(2, 64) <= budget < eng.segment_workspace_bytes(2, 128) and budget < eng.workspace_bytes(2, 96000)
    monkeypatch.setenv(dfn_engine.WORKSPACE_GB_ENV, repr(budget / 2 ** 30))
    (seg,) = node.execute(A)
    assert chosen == [None, 64]
    assert torch.equal(one["waveform"], seg["waveform"])
    assert float((one["waveform"] - x[None]).abs().max()) > 0
