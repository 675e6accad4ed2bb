"""The opt-in batch node of the DeepFilterNet stage (egregora_audio_enhance_dfn_batch.py, dfn_many.denoise_many) on the
native engines: every clip of a list gets exactly what the single node gives it alone -- waveform bits, rate and meta."""
import gc

import pytest
import torch

import dfn2_torch as R2
import dfn3_torch as R3
from dfn3_check import speechy

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model_dirs(pack, tmp_path_factory):
    from egregora_amd import native
    native.require_device()
    root = tmp_path_factory.mktemp("dfn_batch_node")
    dirs = {}
    for R, model in ((R3, "DeepFilterNet3"), (R2, "DeepFilterNet2")):
        dirs[model] = root / model
        R.write_model_dir(dirs[model], seed=5)
    yield dirs
    gc.collect()


@pytest.fixture(scope="module")
def audios():
    """Four list elements, five clips: 16 / 44.1 / 48 kHz, mono and stereo, 0.2 - 1 s; the 48 kHz element is a [2,2,T] batch."""
    return [
        {"waveform": speechy(1, 3200, 1, sr=16000)[None], "sample_rate": 16000, "meta": {"name": "a"}},
        {"waveform": speechy(2, 22050, 2, sr=44100)[None], "sample_rate": 44100},
        {"waveform": torch.stack([speechy(3, 48000, 2), speechy(4, 48000, 2)]), "sample_rate": 48000, "meta": {"name": "c"}},
        {"waveform": speechy(5, 4800, 2, sr=16000)[None], "sample_rate": 16000, "meta": {}},
    ]


@pytest.mark.parametrize("vad", ["rms", "none"])
@pytest.mark.parametrize("stereo_mode", ["per_channel", "downmix_mono"])
@pytest.mark.parametrize("dfn_model", ["DeepFilterNet2", "DeepFilterNet3"])
def test_batch_node_equals_the_single_node_clip_by_clip(pack, model_dirs, audios, monkeypatch, dfn_model, stereo_mode, vad):
    from egregora_amd import dfn_many, egregora_audio_enhance_dfn_batch as B
    monkeypatch.setenv("EGREGORA_DFN_MODEL_DIR", str(model_dirs[dfn_model]))
    assert dfn_many.native_engine(dfn_model) is not None                       # the packed path, not the clip-by-clip loop
    single = pack.NODE_CLASS_MAPPINGS["Egregora_DeepFilterNet_Denoise"]()
    widgets = dict(stereo_mode=stereo_mode, adaptive_vad_source=vad, strength=0.7, post_gain_db=1.0)
    want = []
    for a in audios:
        for b in range(a["waveform"].shape[0]):
            one = dict(a, waveform=a["waveform"][b:b + 1])
            want.append(single.execute(one, dfn_model, **widgets)[0])
    stats = {}
    real = dfn_many.denoise_many
    monkeypatch.setattr(dfn_many, "denoise_many", lambda clips, model, **w: real(clips, model, stats=stats, **w))
    (got,) = B.Egregora_DeepFilterNet_DenoiseBatch().execute(audio=list(audios), dfn_model=[dfn_model],
                                                             **{k: [v] for k, v in widgets.items()})
    assert stats["packed"] is True and len(stats["waves"]) == 1 and stats["alone"] == []
    assert len(got) == len(want) == 5
    for i, (g, w) in enumerate(zip(got, want)):
        assert g["sample_rate"] == w["sample_rate"] and g["meta"] == w["meta"], (i, g["meta"], w["meta"])
        gw, ww = g["waveform"], w["waveform"]
        assert gw.dtype == torch.float32 and gw.device.type == "cpu" and gw.is_contiguous() and gw.shape == ww.shape, (i, gw.shape, ww.shape)
        assert gw.shape[1] == (1 if stereo_mode == "downmix_mono" else audios[(0, 1, 2, 2, 3)[i]]["waveform"].shape[1])
        assert torch.equal(gw, ww), (dfn_model, stereo_mode, vad, "clip", i, float((gw - ww).abs().max()))
        assert bool(torch.isfinite(gw).all()) and float(gw.abs().max()) > 0
