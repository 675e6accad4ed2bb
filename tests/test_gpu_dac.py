"""Native Descript Audio Codec on the device (csrc/egr_dac.hip, SPEC.md 4e) against the float64 restatement tests/dac_torch.py, with
the gates of tests/dac_check.py: every encoder and decoder block through egr_dac_stage, the quantiser alone on 2 000 frames (optimality
of each chosen code on the device's own path, the arithmetic given the codes, equality with float64's codes off the near-ties), encode
end to end, the decoder, and the two nodes."""
import os

import pytest
import torch

import dac_check as K
import dac_torch as R

pytestmark = pytest.mark.gpu
_ENGINES = {}


def engine(pack, name):
    from egregora_amd import dac_engine, dac_weights
    if name not in _ENGINES:
        cfg, sd, _, _ = K.model(name)
        _ENGINES[name] = dac_engine.DacEngine(dac_weights.DacModel(cfg, sd), torch.cuda.current_device())
        _ENGINES[name].keep_stages(True)                     # the quantiser tests read the residual entering every stage
    return _ENGINES[name]


def check_codes(label, codes_dev, codes64, marg, tau):
    """Equality with float64's codes on the frames whose float64 margins all exceed 2 tau; returns that frame mask [rows, F]."""
    safe = K.safe_frames(marg, 2 * tau)
    excluded = 1.0 - float(safe.double().mean())
    same = (codes_dev == codes64).all(dim=1)
    print(f"  {label}: tau {tau:.2e}, frames left out at 2 tau: {excluded:.3%}, frames with equal codes: {float(same.double().mean()):.3%}")
    assert excluded <= K.MAX_EXCLUDED, excluded
    assert bool(same[safe].all()), (label, int((~same[safe]).sum()))
    return safe & same


# ---- these three run before the module's first device call (file order)
def test_node_refusals_before_any_device_work(pack, tmp_path, monkeypatch):
    from egregora_amd import dac_engine, dac_weights, egregora_audio_codec_dac as nodes
    from conftest import gjson
    g = gjson("g17_dac_surface")
    empty = tmp_path / "none"
    empty.mkdir()
    monkeypatch.setenv("EGREGORA_DAC_MODEL_DIR", str(empty))
    monkeypatch.setenv("HOME", str(tmp_path))
    monkeypatch.setattr(dac_weights, "pack_root", lambda: tmp_path / "a" / "b" / "pack")     # so that models/audio/dac/ is empty too
    assert dac_weights.discover("16khz") is None
    with pytest.raises(RuntimeError) as e:
        nodes.Egregora_DAC_Encode().execute({"waveform": torch.zeros(1, 1, 100), "sample_rate": 16000}, "16khz")
    assert str(e.value) == dac_weights.not_found_message("16khz")
    with pytest.raises(ValueError) as e:
        nodes.Egregora_DAC_Decode().execute({"model_type": "44khz", "latents": []})
    assert str(e.value) == g["empty_error"] == "codes.latents empty"
    # the workspace budget: a tiny limit refuses the call and names the variable
    cfg, sd, _, _ = K.model("S")
    R.write_checkpoint(empty / "weights_44khz_test.pth", R.CONFIGS["S"], sd)
    monkeypatch.setenv(dac_engine.WORKSPACE_GB_ENV, "1e-6")
    with pytest.raises(RuntimeError, match=r"EGREGORA_DAC_WORKSPACE_GB = 1e-06"):
        nodes.Egregora_DAC_Encode().execute({"waveform": torch.zeros(1, 1, 1000), "sample_rate": 44100})


@pytest.mark.parametrize("name", ["S", "O", "W", "G"])
def test_encoder_stages(pack, name):
    cfg, sd, n64, n32 = K.model(name)
    f = K.forward(name)
    eng = engine(pack, name)
    z, codes = eng.encode(f["x"].cuda())
    torch.cuda.synchronize()
    n_pad, frames, _ = eng.lengths(f["x"].shape[1])
    assert tuple(z.shape) == (R.ROWS, cfg["latent_dim"], frames) and tuple(codes.shape) == (R.ROWS, cfg["n_codebooks"], frames)
    assert codes.dtype == torch.int32 and int(codes.min()) >= 0 and int(codes.max()) < cfg["codebook_size"]
    print(f"{name}: encoder")
    for i, (r64, r32) in enumerate(zip(f["enc64"], f["enc32"])):
        K.gate(f"enc{i}", eng.stage("enc", i).cpu(), K.cl(r64), K.cl(r32))
    # encode end to end: the codes off the near-ties, z on the frames whose codes all agree
    tau = K.e2e_tau(name)
    ok = check_codes(f"{name} end to end", codes.cpu().long(), f["codes64"], K.margins(f["sims64"]), tau)
    ok &= (f["codes32"] == f["codes64"]).all(dim=1)               # z32 is a yardstick only where the fp32 path chose the same codes
    assert float(ok.double().mean()) >= 1 - K.MAX_EXCLUDED
    pick = lambda t: t.double().cpu().transpose(1, 2)[ok]          # [frames kept, latent]
    K.gate("z", pick(z), pick(f["z64"]), pick(f["z32"]))


@pytest.mark.parametrize("name", ["S", "W", "G"])
def test_quantiser_alone(pack, name):
    cfg, sd, n64, n32 = K.model(name)
    v = K.vq_case(name)
    eng = engine(pack, name)
    z, codes = eng.quantize(v["ze"].cuda())
    torch.cuda.synchronize()
    codes = codes.cpu().long()
    tau = v["tau"]
    print(f"{name}: quantiser alone, tau {tau:.2e}")
    assert 2 * tau <= K.MARGIN_CAP
    # (a) optimality on the device's own path: the chosen code's float64 similarity is within tau of the best, stage by stage
    worst = 0.0
    with torch.no_grad():
        for q in range(cfg["n_codebooks"]):
            r = eng.stage("vq_in", q).cpu().double().reshape(K.VQ_ROWS, K.VQ_FRAMES, cfg["latent_dim"]).transpose(1, 2)
            s = n64.similarities(r, q)
            gap = s.max(dim=-1).values - s.gather(-1, codes[:, q].unsqueeze(-1)).squeeze(-1)
            worst = max(worst, float(gap.max()))
            if q == 0:
                assert torch.equal(r.float(), v["ze"])            # the first stage's input is ze itself
        print(f"  (a) largest similarity gap of a chosen code: {worst:.2e}")
        assert worst <= tau, (worst, tau)
        # (b) the arithmetic given the codes
        z64 = n64.quantize(v["ze"], codes=codes)[0]
        z32 = n32.quantize(v["ze"], codes=codes)[0]
    K.gate("(b) z from the device's codes", z.cpu(), z64, z32)
    # (c) the same path as float64 off the near-ties
    check_codes(f"(c) {name}", codes, v["codes64"], v["margins"], tau)


@pytest.mark.parametrize("name", ["S", "O", "W", "G"])
def test_decoder_stages(pack, name):
    cfg, sd, n64, n32 = K.model(name)
    f = K.forward(name)
    eng = engine(pack, name)
    y = eng.decode(f["zin"].cuda())
    torch.cuda.synchronize()
    assert tuple(y.shape) == (R.ROWS, eng.lengths(f["x"].shape[1])[2]) == tuple(f["y64"].shape)
    print(f"{name}: decoder")
    for i, (r64, r32) in enumerate(zip(f["dec64"], f["dec32"])):
        K.gate(f"dec{i}", eng.stage("dec", i).cpu(), K.cl(r64), K.cl(r32))
    K.gate("y", y.cpu(), f["y64"], f["y32"])


def test_nodes_round_trip(pack, tmp_path, monkeypatch):
    from egregora_amd import dac_engine, egregora_audio_codec_dac as nodes
    cfg, sd, n64, n32 = K.model("S")
    R.write_checkpoint(tmp_path / "weights_44khz_test.pth", R.CONFIGS["S"], sd)
    monkeypatch.setenv("EGREGORA_DAC_MODEL_DIR", str(tmp_path))
    x = torch.stack([R.test_signal(2, 1003, 11), R.test_signal(2, 1003, 12)])       # [2, 2, 1003] at the model rate
    enc, dec = nodes.Egregora_DAC_Encode(), nodes.Egregora_DAC_Decode()
    d, log = enc.execute({"waveform": x, "sample_rate": 44100}, "44khz", "cpu")
    assert log == "DAC encode ok: model=44khz, B=2, C=2, sr=44100->44100"
    assert sorted(d) == ["codes", "latents", "model_sample_rate", "model_type", "sample_rate"]
    assert (d["model_type"], d["sample_rate"], d["model_sample_rate"]) == ("44khz", 44100, 44100)
    n_pad, frames, n_dec = dac_engine.lengths(cfg, 1003)
    for zl, c in zip(d["latents"], d["codes"]):
        assert isinstance(zl, list) and len(zl) == 1
        assert zl[0].dtype == torch.float32 and not zl[0].is_cuda and tuple(zl[0].shape) == (2, cfg["latent_dim"], frames)
        assert c.dtype == torch.int64 and tuple(c.shape) == (2, cfg["n_codebooks"], frames)
    with pytest.raises(RuntimeError, match="egr_dac_stage"):              # the residual dumps are off unless asked for
        dac_engine.engine(tmp_path / "weights_44khz_test.pth").stage("vq_in", 0)
    n_cached = len(dac_engine._CACHE)
    (audio, log2) = dec.execute(d, "auto")
    assert len(dac_engine._CACHE) == n_cached                             # the second node reuses the cached handle
    assert log2 == "DAC decode ok: model=44khz, B=2, C=2, 44100->44100"
    y = audio["waveform"]
    assert tuple(y.shape) == (2, 2, n_dec) and y.dtype == torch.float32 and audio["sample_rate"] == 44100
    print("S: node round trip")
    with torch.no_grad():
        for b in range(2):
            r = {}
            for tag, net in (("64", n64), ("32", n32)):
                ze = net.encode_stages(x[b])[-1]
                z, codes, ins, sims = net.quantize(ze)
                r[tag] = (z, codes, sims, net.decode_stages(z)[1])
            agree = (d["codes"][b] == r["64"][1]).all(dim=1) & (r["32"][1] == r["64"][1]).all(dim=1)       # [C, frames]
            print(f"  batch {b}: frames whose codes agree {float(agree.double().mean()):.3%}")
            assert float(agree.double().mean()) >= 1 - K.MAX_EXCLUDED
            pick = lambda t: t.double().transpose(1, 2)[agree]
            K.gate(f"z[{b}]", pick(d["latents"][b][0]), pick(r["64"][0]), pick(r["32"][0]))
            assert bool(agree.all())                                      # y depends on every frame within the receptive field
            K.gate(f"y[{b}]", y[b], r["64"][3], r["32"][3])
    # a [latent, frames] entry decodes as one row
    one = dict(d, latents=[d["latents"][0][0][0]])
    (a1, _) = dec.execute(one)
    assert tuple(a1["waveform"].shape) == (1, 1, n_dec) and torch.equal(a1["waveform"][0, 0], y[0, 0])


def test_nodes_at_another_rate(pack, tmp_path, monkeypatch):
    """Shapes, finiteness and sample-rate bookkeeping only (DAC-Q2: this pack's polyphase resampler on both sides)."""
    from egregora_amd import dac_engine, egregora_audio_codec_dac as nodes
    cfg, sd, _, _ = K.model("S")
    R.write_checkpoint(tmp_path / "weights_44khz_test.pth", R.CONFIGS["S"], sd)
    monkeypatch.setenv("EGREGORA_DAC_MODEL_DIR", str(tmp_path))
    x = R.test_signal(1, 800, 13)[None]
    d, log = nodes.Egregora_DAC_Encode().execute({"waveform": x, "sample_rate": 22050})
    assert log == "DAC encode ok: model=44khz, B=1, C=1, sr=22050->44100" and (d["sample_rate"], d["model_sample_rate"]) == (22050, 44100)
    n_pad, frames, n_dec = dac_engine.lengths(cfg, 1600)
    assert tuple(d["latents"][0][0].shape) == (1, cfg["latent_dim"], frames)
    (audio, log2) = nodes.Egregora_DAC_Decode().execute(d)
    assert log2 == "DAC decode ok: model=44khz, B=1, C=1, 44100->22050"
    y = audio["waveform"]
    assert audio["sample_rate"] == 22050 and tuple(y.shape) == (1, 1, (n_dec + 1) // 2) and bool(torch.isfinite(y).all())
