"""Native DeepFilterNet2 (egr_dfn2_* in csrc/egr_dfn3.hip, through dfn2_engine.py) against the plain-PyTorch restatement
tests/dfn2_torch.py, mirroring tests/test_gpu_dfn3.py.

Synthetic model directory (the recalled DeepFilterNet2 default config.ini, seeded random weights).  Gates (dfn2_check, DeepFilterNet3's
margins unchanged): relative rms against the float64 restatement <= 1.5x the float32 restatement's own error + 3e-7 and <= 1e-4 on
every stage read back after one call (cumulative) and on y; local per-stage gates (each stage restated from the device's own inputs:
rms as above, max-abs <= 3x float32's + 3e-7).  The node tests leave `dfn_model` at its default, DeepFilterNet2.
"""
import gc
import math

import pytest
import torch

import dfn2_check as K
import dfn2_torch as R
import dfn3_torch as R3
from dfn2_check import FLOOR, gate, rel, speechy

pytestmark = pytest.mark.gpu


def _engine(d):
    from egregora_amd import dfn2_engine, dfn2_weights
    return dfn2_engine.Dfn2Engine(dfn2_weights.load(d), torch.cuda.current_device())


@pytest.fixture(scope="module")
def model(pack, tmp_path_factory):
    from egregora_amd import native
    native.require_device()
    d = tmp_path_factory.mktemp("dfn2") / "DeepFilterNet2"
    cfg, sd = R.write_model_dir(d, seed=5)
    return d, cfg, sd, _engine(d)


@pytest.fixture(scope="module")
def model_hop240(pack, tmp_path_factory):
    from egregora_amd import native
    native.require_device()
    d = tmp_path_factory.mktemp("dfn2_240") / "DeepFilterNet2"
    cfg, sd = R.write_model_dir(d, seed=5, cfg_text=R.config_text(hop_size=240))
    return d, cfg, sd, _engine(d)


def test_every_stage_cumulative_and_local(model):
    d, cfg, sd, eng = model
    x = speechy(1, 48000, 2)
    y = eng.enhance(x.cuda())
    torch.cuda.synchronize()
    cum, dev, _ = K.cumulative(eng, x, y, cfg, sd)
    print("\nDFN2 cumulative (device, fp32):", {k: f"{a:.2e}/{b:.2e}" for k, (a, b) in cum.items()})
    loc = K.local(eng, x, y, cfg, sd, dev)
    print("DFN2 local (rms, rms fp32, max, max fp32):", K.fmt(loc))


@pytest.mark.parametrize("seconds,C", [(1.0, 1), (1.0, 2), (10.0, 1), (10.0, 2), (7.3, 1), (7.3, 2)])
def test_end_to_end_lengths_and_channels(model, seconds, C):
    d, cfg, sd, eng = model
    n = int(round(seconds * 48000)) + (17 if seconds == 7.3 else 0)
    x = speechy(int(seconds * 10) + C, n, C)
    y = eng.enhance(x.cuda()).cpu()
    assert y.shape == x.shape and bool(torch.isfinite(y).all())
    y64 = R.enhance(x, cfg, sd, torch.float64)
    y32 = R.enhance(x, cfg, sd, torch.float32)
    gate(f"{seconds}s x{C}", y, y64, y32)
    if C == 2:
        y1 = eng.enhance(x[1:].cuda().contiguous()).cpu()
        assert rel(y1, y64[1:]) <= 1.5 * rel(y32[1:], y64[1:]) + FLOOR


def test_sixty_seconds_do_not_drift(model):
    """6 000 recurrence steps: the error of the last ten seconds is no larger than that of the first ten (no drift)."""
    d, cfg, sd, eng = model
    x = speechy(60, 60 * 48000, 1)
    y = eng.enhance(x.cuda()).cpu()
    y64 = R.enhance(x, cfg, sd, torch.float64)
    y32 = R.enhance(x, cfg, sd, torch.float32)
    gate("60 s", y, y64, y32)
    w = 10 * 48000
    e_first, e_last = rel(y[:, :w], y64[:, :w]), rel(y[:, -w:], y64[:, -w:])
    e32_last = rel(y32[:, -w:], y64[:, -w:])
    assert e_last <= 2.0 * e_first + FLOOR and e_last <= 1.5 * e32_last + FLOOR, (e_first, e_last, e32_last)


@pytest.mark.parametrize("T", [1, 2, 479, 480, 481, 959, 960, 961])
@pytest.mark.parametrize("which", ["default", "hop240"])
def test_short_lengths(model, model_hop240, which, T):
    d, cfg, sd, eng = model if which == "default" else model_hop240
    x = speechy(T, T, 2)
    y = eng.enhance(x.cuda())
    torch.cuda.synchronize()
    assert y.shape == x.shape and bool(torch.isfinite(y).all())
    n, ng = K.stage_counts(cfg, 2, T)
    assert all(eng.stage(k).numel() == v for k, v in n.items())
    assert [eng.stage("gru0", g).numel() for g in range(len(ng))] == ng == [eng.stage("sum0", g).numel() for g in range(len(ng))]
    cum, dev, _ = K.cumulative(eng, x, y, cfg, sd)
    loc = K.local(eng, x, y, cfg, sd, dev)
    print(f"\nDFN2 {which} T={T} y (device, fp32): {cum['y'][0]:.2e}/{cum['y'][1]:.2e}; local:", K.fmt(loc))


def test_digital_silence_gives_exact_zero(model):
    d, cfg, sd, eng = model
    x = torch.zeros(2, 2 * 48000)
    y = eng.enhance(x.cuda())
    torch.cuda.synchronize()
    assert not y.any()
    for name in K.PICK:
        assert bool(torch.isfinite(eng.stage(name)).all()), name
    for g in range(K.n_grus(cfg)):
        assert bool(torch.isfinite(eng.stage("gru0", g)).all()) and bool(torch.isfinite(eng.stage("sum0", g)).all()), g
    assert not eng.stage("spec").any() and not eng.stage("spec_e").any() and not eng.stage("feat_spec").any()


def test_long_silence_then_speech_keeps_the_norm_state_finite(pack, tmp_path):
    """norm_tau 0.1: 12 s of zeros drive the unit-norm state into the float32 subnormals; the 3 s of speech after it are gated."""
    d = tmp_path / "DeepFilterNet2"
    cfg, sd = R.write_model_dir(d, seed=7, cfg_text=R.config_text(norm_tau=0.1))
    eng = _engine(d)
    w = 3 * 48000
    x = torch.cat([torch.zeros(1, 12 * 48000), speechy(12, w, 1)], 1)
    y = eng.enhance(x.cuda()).cpu()
    assert bool(torch.isfinite(y).all())
    for name in K.PICK:
        assert bool(torch.isfinite(eng.stage(name)).all()), name
    y64 = R.enhance(x, cfg, sd, torch.float64)
    y32 = R.enhance(x, cfg, sd, torch.float32)
    assert bool(torch.isfinite(y32).all())
    gate("silence + speech", y, y64, y32)
    gate("last 3 s", y[:, -w:], y64[:, -w:], y32[:, -w:])
    del eng
    gc.collect()


def _square(n):
    t = torch.arange(n, dtype=torch.float64)
    return torch.where(torch.sin(2 * torch.pi * 220.0 * t / 48000) >= 0, 1.0, -1.0).float()[None].repeat(2, 1)


@pytest.mark.parametrize("level", ["1e-6", "square", "dc"])
def test_signal_levels(model, level):
    d, cfg, sd, eng = model
    s = speechy(21, 48000, 2)
    x = {"1e-6": s * 1e-6, "square": _square(48000), "dc": s + 0.5}[level].contiguous()
    y = eng.enhance(x.cuda())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y).all())
    cum, dev, _ = K.cumulative(eng, x, y, cfg, sd)
    loc = K.local(eng, x, y, cfg, sd, dev)
    print(f"\nDFN2 level {level} y (device, fp32): {cum['y'][0]:.2e}/{cum['y'][1]:.2e}; local:", K.fmt(loc))


@pytest.mark.parametrize("C", [3, 5, 8])
def test_channels_are_bit_exact_independent(model, C):
    d, cfg, sd, eng = model
    x = speechy(30 + C, 48000, C).cuda()
    y = eng.enhance(x).cpu()
    for c in range(C):
        yc = eng.enhance(x[c:c + 1].contiguous()).cpu()
        assert torch.equal(yc[0], y[c]), (C, c, float((yc[0] - y[c]).abs().max()))


def test_engine_state_repeat_regrow_and_interleave(pack, model, model_hop240, tmp_path):
    """One engine: identical calls give identical bits; 1 s stereo -> 7.3 s mono -> 1 s stereo gives a fresh engine's bits and
    stage() reports each call's own counts.  Two DeepFilterNet2 engines of different configs and a DeepFilterNet3 engine, their calls
    interleaved on one stream, each give the bits they give alone."""
    from egregora_amd import dfn_engine, dfn_weights
    d, cfg, sd, eng = model
    d2, cfg2, sd2, eng2 = model_hop240
    d3 = tmp_path / "DeepFilterNet3"
    R3.write_model_dir(d3, seed=5)
    eng3 = dfn_engine.Dfn3Engine(dfn_weights.load(d3), torch.cuda.current_device())
    a, b = speechy(41, 48000, 2), speechy(42, int(7.3 * 48000) + 17, 1)
    fresh = _engine(d)
    want = {k: fresh.enhance(v.cuda()).cpu() for k, v in (("a", a), ("b", b))}
    del fresh
    gc.collect()
    y1 = eng.enhance(a.cuda()).cpu()
    y2 = eng.enhance(a.cuda()).cpu()
    assert torch.equal(y1, y2) and torch.equal(y1, want["a"])
    for key, x in (("a", a), ("b", b), ("a", a)):
        y = eng.enhance(x.cuda()).cpu()
        assert torch.equal(y, want[key]), key
        n, ng = K.stage_counts(cfg, x.shape[0], x.shape[1])
        assert {k: eng.stage(k).numel() for k in n} == n
        assert [eng.stage("gru0", g).numel() for g in range(len(ng))] == ng
    alone2 = {k: eng2.enhance(v.cuda()).cpu() for k, v in (("a", a), ("b", b))}
    alone3 = {k: eng3.enhance(v.cuda()).cpu() for k, v in (("a", a), ("b", b))}
    for key, x in (("b", b), ("a", a), ("a", a), ("b", b)):
        xd = x.cuda()
        r1, r3, r2 = eng.enhance(xd), eng3.enhance(xd), eng2.enhance(xd)          # enqueued back to back on the current stream
        assert torch.equal(r1.cpu(), want[key]) and torch.equal(r3.cpu(), alone3[key]) and torch.equal(r2.cpu(), alone2[key])
    del eng3
    gc.collect()


@pytest.mark.parametrize("sr", [44100, 48000])
def test_node_default_model_runs_natively(pack, model, monkeypatch, sr):
    """The node with `dfn_model` left at its default (DeepFilterNet2) and a DeepFilterNet2 directory runs the native pass; it equals
    the node with the restatement registered, under the cumulative gate.  (Before the native DeepFilterNet2 it raised.)"""
    from egregora_amd import egregora_audio_enhance_extras as X
    d, cfg, sd, eng = model
    monkeypatch.setenv("EGREGORA_DFN_MODEL_DIR", str(d))
    x = speechy(7, int(2.5 * sr), 2, sr)
    A = {"waveform": x[None], "sample_rate": sr, "meta": {}}
    node = pack.NODE_CLASS_MAPPINGS["Egregora_DeepFilterNet_Denoise"]()
    kw = dict(post_gain_db=0.0, limit_ceiling=False, adaptive_vad_source="none", strength=1.0)
    assert X._ENHANCER is None
    (nat,) = node.execute(A, **kw)
    outs = {}
    try:
        for dt in (torch.float64, torch.float32):
            X.set_enhancer(R.enhancer(cfg, sd, dt))
            (outs[dt],) = node.execute(A, **kw)
    finally:
        X.set_enhancer(None)
    yn, y64, y32 = (o["waveform"] for o in (nat, outs[torch.float64], outs[torch.float32]))
    assert yn.shape == y64.shape == x[None].shape and nat["sample_rate"] == sr
    assert nat["meta"]["deepfilternet"]["model"] == "DeepFilterNet2"
    gate(f"node {sr}", yn, y64, y32)
    assert rel(yn, x[None]) > 1e-2
    (default,) = node.execute(A)                                             # every widget at its default
    assert bool(torch.isfinite(default["waveform"]).all())


def test_c5_cut_down_with_the_default_denoiser(pack, model, monkeypatch):
    """BASELINE C5 in small: DeepFilterNet2 (the node default) denoise -> FlashSR (random weights) -> Fat-Llama, no stage bypassed."""
    from egregora_amd import flashsr_arch as A_, flashsr_engine as E
    d, cfg, sd, eng = model
    monkeypatch.setenv("EGREGORA_DFN_MODEL_DIR", str(d))
    x = speechy(55, 3 * 44100, 2, 44100)
    A = {"waveform": x[None], "sample_rate": 44100}
    dn = pack.NODE_CLASS_MAPPINGS["Egregora_DeepFilterNet_Denoise"]()
    up = pack.NODE_CLASS_MAPPINGS["EgregoraAudioUpscaler"]()
    fl = pack.NODE_CLASS_MAPPINGS["EgregoraFatLlamaGPU"]()
    fcfg = A_.FlashSRConfig()
    E.set_engine(E.FlashSREngine(fcfg, A_.init_params(fcfg, 0)))
    try:
        (den,) = dn.execute(A)
        assert den["sample_rate"] == 44100 and tuple(den["waveform"].shape) == (1, 2, x.shape[1])
        assert rel(den["waveform"], x[None]) > 1e-2
        (mid,) = up.run(den, False, "96000")
        (out,) = fl.run("wav", 20, 0.6, 3072, True, False, AUDIO=mid)
    finally:
        E.set_engine(None)
    y = out["waveform"]
    n96 = int(math.ceil(x.shape[1] * 48000 / 44100)) * 2
    assert out["sample_rate"] == 96000 and y.shape[:2] == (1, 2) and abs(y.shape[2] - n96) <= 4 and bool(torch.isfinite(y).all())
    assert 0.0 < float(y.abs().max()) <= 1.0


def test_workspace_and_time_gru(model):
    """workspace_bytes is what enhance grows to; time_gru runs every layer kind (grouped here) and reports a positive step time."""
    d, cfg, sd, eng = model
    assert eng.workspace_bytes(2, 48000) > 0
    assert eng.time_gru(0, 2, 200) > 0.0 and eng.time_gru(K.n_grus(cfg) - 1, 1, 200) > 0.0
