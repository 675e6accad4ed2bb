"""The codec's batch nodes (egregora_audio_codec_dac_batch.py) on the device: a list of AUDIO values at two rates
through Egregora_DAC_EncodeBatch and Egregora_DAC_DecodeBatch on a temporary checkpoint of config S, judged by the gates of
tests/dac_check.py against the float64 restatement run on the signal the single path hands the codec (the polyphase resample of the
22.05 kHz clip)."""
import pytest
import torch

import dac_check as K
import dac_torch as R
from test_gpu_dac_segmented import check_codes

pytestmark = pytest.mark.gpu


def restate(x):
    """K.forward's dictionary for an arbitrary x [rows, n] of config S, and its e2e tau."""
    cfg, sd, n64, n32 = K.model("S")
    out = {"x": x}
    with torch.no_grad():
        for tag, net in (("64", n64), ("32", n32)):
            enc = net.encode_stages(x)
            out["z" + tag], out["codes" + tag], _, out["sims" + tag] = net.quantize(enc[-1])
        out["zin"] = out["z64"].float()
        for tag, net in (("64", n64), ("32", n32)):
            out["y" + tag] = net.decode_stages(out["zin"])[1]
    agree = torch.ones_like(out["codes64"][:, 0], dtype=torch.bool)
    tau = 0.0
    for q in range(out["codes64"].shape[1]):                    # dac_check.e2e_tau's rule
        d = (out["sims32"][q].double() - out["sims64"][q]).abs().amax(dim=-1)
        if agree.any():
            tau = max(tau, float(d[agree].max()))
        agree &= out["codes32"][:, q] == out["codes64"][:, q]
    return out, K.TAU_X * tau


def judge(label, f, tau, z, codes):
    """The code rule and the z gate of tests/test_gpu_dac_segmented.py::check_encode (the DICT carries no ze)."""
    ok = check_codes(label, codes.cpu().long(), f["codes64"], K.margins(f["sims64"]), tau)
    ok &= (f["codes32"] == f["codes64"]).all(dim=1)
    assert float(ok.double().mean()) >= 1 - K.MAX_EXCLUDED
    pick = lambda t: t.double().cpu().transpose(1, 2)[ok]
    K.gate(f"{label} z", pick(z), pick(f["z64"]), pick(f["z32"]))
    return ok


def test_batch_nodes_on_a_list_at_two_rates(pack, tmp_path, monkeypatch):
    from egregora_amd import dac_engine as E, egregora_audio_codec_dac as single, egregora_audio_codec_dac_batch as B, resample
    cfg, sd, _, _ = K.model("S")
    R.write_checkpoint(tmp_path / "weights_44khz_test.pth", R.CONFIGS["S"], sd)
    monkeypatch.setenv("EGREGORA_DAC_MODEL_DIR", str(tmp_path))
    f = K.forward("S", 1003)
    x = torch.stack([f["x"], f["x"].flip(0)])                                   # [2, 2, 1003] at the model's rate
    mono = R.test_signal(1, 500, 31)                                            # [1, 500] at half the model's rate
    up = resample.resample_hq(mono.cuda(), 22050, 44100).cpu()                  # what the single path hands the codec
    g, tau_g = restate(up)
    audio = [{"waveform": x, "sample_rate": 44100}, {"waveform": mono, "sample_rate": 22050}]
    dicts, logs = B.Egregora_DAC_EncodeBatch().execute(audio=audio, model_type=["44khz"], device=["auto"])
    assert len(dicts) == len(logs) == 2
    # keys, types and shapes are the single node's
    for a, d, log in zip(audio, dicts, logs):
        d1, log1 = single.Egregora_DAC_Encode().execute(a, "44khz")
        assert log == log1 and set(d) == set(d1) and all(d[k] == d1[k] for k in ("model_type", "sample_rate", "model_sample_rate"))
        assert len(d["latents"]) == len(d1["latents"]) and len(d["codes"]) == len(d1["codes"])
        for (z,), (z1,), c, c1 in zip(d["latents"], d1["latents"], d["codes"], d1["codes"]):
            assert z.shape == z1.shape and z.dtype == z1.dtype == torch.float32 and z.device.type == "cpu"
            assert c.shape == c1.shape and c.dtype == c1.dtype == torch.int64 and c.device.type == "cpu"
    print("S: batch encode node")
    tau = K.e2e_tau("S", 1003)
    flip = lambda t: t.flip(0)
    for b, want in enumerate((lambda t: t, flip)):
        fb = {k: want(f[k]) for k in ("codes64", "codes32", "z64", "z32")}
        fb["sims64"] = [want(s) for s in f["sims64"]]
        judge(f"[2,2,1003] element {b}", fb, tau, dicts[0]["latents"][b][0], dicts[0]["codes"][b])
    judge("mono 22.05 kHz", g, tau_g, dicts[1]["latents"][0][0], dicts[1]["codes"][0])
    # the round trip through both batch nodes, against the restatement's decode of the device's own latents
    audios, logs2 = B.Egregora_DAC_DecodeBatch().execute(codes=dicts, device=["auto"])
    n_dec = E.lengths(cfg, 1003)[2]
    assert tuple(audios[0]["waveform"].shape) == (2, 2, n_dec) and audios[0]["sample_rate"] == 44100
    a1, _ = single.Egregora_DAC_Decode().execute(dicts[1])
    assert audios[1]["waveform"].shape == a1["waveform"].shape and audios[1]["sample_rate"] == 22050
    assert logs2[0] == "DAC decode ok: model=44khz, B=2, C=2, 44100->44100"
    _, _, n64, n32 = K.model("S")
    print("S: batch decode node")
    with torch.no_grad():
        for b in range(2):
            zin = dicts[0]["latents"][b][0]
            K.gate(f"y[{b}]", audios[0]["waveform"][b], n64.decode_stages(zin)[1], n32.decode_stages(zin)[1])
        zin = dicts[1]["latents"][0][0]
        y64, y32 = n64.decode_stages(zin)[1], n32.decode_stages(zin)[1]
    # the 22.05 kHz result is the resample of the decode: judged at the model's rate through the same resample of the references
    down = lambda t: resample.resample_hq(t.float().cuda(), 44100, 22050).cpu()
    K.gate("y mono at 22.05 kHz", audios[1]["waveform"][0], down(y64), down(y32.double()))
    # a codes-only DICT decodes to the same audio
    (again, _) = B.Egregora_DAC_DecodeBatch().execute(codes=[{k: v for k, v in d.items() if k != "latents"} for d in dicts])
    assert all(torch.equal(u["waveform"], v["waveform"]) for u, v in zip(audios, again))
