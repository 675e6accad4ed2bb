"""Native DeepFilterNet3 (csrc/egr_dfn3.hip through dfn_engine.py) against the plain-PyTorch restatement tests/dfn3_torch.py.

Synthetic model directory (DeepFilterNet3-default config.ini, seeded random weights).  Gate, per stage and end to end: the relative
rms error against the float64 restatement is at most 1.5x the float32 restatement's own error plus a few float32 ulps, and below an
absolute cap.  Stages are read back with egr_dfn3_stage after one enhance call, so each carries the error of everything before it.
"""
import math

import numpy as np
import pytest
import torch

import dfn3_torch as R

pytestmark = pytest.mark.gpu
FLOOR, CAP = 3e-7, 1e-4


def speechy(seed, n, C, sr=48000):
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(n) / sr
    env = 0.5 + 0.5 * np.sin(2 * np.pi * 2.3 * t) ** 2
    x = np.stack([env * sum(np.sin(2 * np.pi * f * (1 + 0.01 * c) * t) / (k + 1) for k, f in enumerate((150, 310, 620, 1240, 2900)))
                  + 0.05 * rng.standard_normal(n) for c in range(C)])
    return torch.from_numpy((0.4 * x / np.abs(x).max()).astype(np.float32))


@pytest.fixture(scope="module")
def model(pack, tmp_path_factory):
    from egregora_amd import dfn_engine, dfn_weights, native
    native.require_device()
    d = tmp_path_factory.mktemp("dfn") / "DeepFilterNet3"
    cfg, sd = R.write_model_dir(d, seed=5)
    eng = dfn_engine.Dfn3Engine(dfn_weights.load(d), torch.cuda.current_device())
    return d, cfg, sd, eng


def rel(a, ref):
    a, ref = a.double().cpu().reshape(-1), ref.double().cpu().reshape(-1)
    return float((a - ref).norm() / max(float(ref.norm()), 1e-300))


def gate(name, got, r64, r32, floor=FLOOR, cap=CAP):
    e, e32 = rel(got, r64), rel(r32, r64)
    assert e <= 1.5 * e32 + floor and e <= cap, (name, e, e32)
    return e, e32


def nhwc(t):
    return t.permute(0, 2, 3, 1)


def test_every_stage_against_the_float64_restatement(model):
    d, cfg, sd, eng = model
    x = speechy(1, 48000, 2)
    y = eng.enhance(x.cuda())
    torch.cuda.synchronize()
    y64, s64 = R.enhance(x, cfg, sd, torch.float64, stages=True)
    y32, s32 = R.enhance(x, cfg, sd, torch.float32, stages=True)
    C, T = x.shape
    nF = (T + cfg["fft_size"]) // cfg["hop_size"]
    pick = {
        "spec": lambda s: torch.view_as_real(s["spec"]),
        "feat_erb": lambda s: s["feat_erb"][:, 0],
        "feat_spec": lambda s: s["feat_spec"].permute(0, 2, 3, 1),
        "e0": lambda s: nhwc(s["e0"]), "e1": lambda s: nhwc(s["e1"]), "e2": lambda s: nhwc(s["e2"]), "e3": lambda s: nhwc(s["e3"]),
        "c0": lambda s: nhwc(s["c0"]), "emb": lambda s: s["emb"], "mask": lambda s: s["mask"], "coefs": lambda s: s["coefs"],
        "spec_e": lambda s: torch.view_as_real(s["spec_e"]),
    }
    report = {}
    for name, f in pick.items():
        ref = f(s64)
        got = eng.stage(name).cpu().reshape(ref.shape)
        report[name] = gate(name, got, ref, f(s32))
    n_gru = len(s64["grus"])
    assert n_gru == 1 + (cfg["emb_num_layers"] - 1) + cfg["df_num_layers"]
    for g in range(n_gru):
        ref = s64["grus"][g]
        got = eng.stage("gru0", g).cpu().reshape(ref.shape)
        report[f"gru{g}"] = gate(f"gru{g}", got, ref, s32["grus"][g])
    report["y"] = gate("y", y, y64, y32)
    assert nF == s64["spec"].shape[1]
    print("\nDFN3 stage errors (device, torch fp32) vs float64:", {k: f"{a:.2e}/{b:.2e}" for k, (a, b) in report.items()})


@pytest.mark.parametrize("seconds,C", [(1.0, 1), (1.0, 2), (10.0, 1), (10.0, 2), (7.3, 1), (7.3, 2)])
def test_end_to_end_lengths_and_channels(model, seconds, C):
    d, cfg, sd, eng = model
    n = int(round(seconds * 48000)) + (17 if seconds == 7.3 else 0)         # an odd length, not a multiple of the hop
    x = speechy(int(seconds * 10) + C, n, C)
    y = eng.enhance(x.cuda()).cpu()
    assert y.shape == x.shape and bool(torch.isfinite(y).all())
    y64 = R.enhance(x, cfg, sd, torch.float64)
    y32 = R.enhance(x, cfg, sd, torch.float32)
    gate(f"{seconds}s x{C}", y, y64, y32)
    if C == 2:                                                                 # channels are independent
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


@pytest.mark.parametrize("sr", [44100, 48000])
def test_node_native_equals_the_node_with_the_restatement_registered(pack, model, monkeypatch, sr):
    from egregora_amd import egregora_audio_enhance_extras as X
    d, cfg, sd, eng = model
    monkeypatch.setenv("EGREGORA_DFN_MODEL_DIR", str(d))
    x = speechy(7, int(2.5 * sr), 2, sr)
    A = {"waveform": x[None], "sample_rate": sr, "meta": {}}
    node = pack.NODE_CLASS_MAPPINGS["Egregora_DeepFilterNet_Denoise"]()
    kw = dict(dfn_model="DeepFilterNet3", post_gain_db=0.0, limit_ceiling=False, adaptive_vad_source="none", strength=1.0)
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
    gate(f"node {sr}", yn, y64, y32)
    assert rel(yn, x[None]) > 1e-2                                             # the stage really ran (not bypassed)
    (default,) = node.execute(A, dfn_model="DeepFilterNet3")                   # the default mix path with the native backend
    assert bool(torch.isfinite(default["waveform"]).all())


def test_c5_cut_down_with_the_denoiser_stage(pack, model, monkeypatch):
    """BASELINE C5 in small: DeepFilterNet3 denoise -> FlashSR (random weights) -> Fat-Llama, no stage bypassed."""
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
        (den,) = dn.execute(A, dfn_model="DeepFilterNet3")
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
