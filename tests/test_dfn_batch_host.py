"""Host side of the DeepFilterNet batch path: the wave planner of DfnEngine.enhance_many, the opt-in batch node's
registration and surface, the directory CLI -- no device (dfn_many.denoise_many is replaced where a test reaches it)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
KEY = "Egregora_DeepFilterNet_DenoiseBatch"
FLAG = "EGREGORA_DENOISE_BATCH_NODES"


# ---------------------------------------------------------------- plan_waves
def _check_plan(E, channels, frames, per_row, fixed, budget, max_frames):
    rows = [c * f for c, f in zip(channels, frames)]
    bytes_for = lambda idx: fixed + per_row * sum(rows[i] for i in idx)
    waves, alone = E.plan_waves(channels, frames, bytes_for, budget, max_frames)
    flat = [i for w in waves for i in w]
    assert sorted(flat + alone) == list(range(len(frames)))                     # every clip in exactly one wave, or alone (whole)
    assert alone == sorted(alone)
    for i in range(len(frames)):
        over = rows[i] > max_frames or bytes_for([i]) > budget
        assert (i in alone) == over                                              # alone exactly when over a limit on its own
    for n, w in enumerate(waves):
        assert w and sum(rows[i] for i in w) <= max_frames and bytes_for(w) <= budget
        fr = [frames[i] for i in w]
        assert fr == sorted(fr, reverse=True)                                    # longest first
        for a, b in zip(w, w[1:]):
            assert frames[a] > frames[b] or a < b                                # ties keep their input order
        if n + 1 < len(waves):                                                   # a wave closes only before the clip that does not fit
            nxt = waves[n + 1][0]
            assert sum(rows[i] for i in w) + rows[nxt] > max_frames or bytes_for(w + [nxt]) > budget
            assert frames[w[-1]] >= frames[nxt]
    # the input order is restored from the plan: results placed by index cover every slot once
    slots = [None] * len(frames)
    for k, i in enumerate(flat + alone):
        assert slots[i] is None
        slots[i] = k
    assert None not in slots
    return waves, alone


def test_plan_waves_properties(pack):
    from egregora_amd import dfn_engine as E
    rng = np.random.default_rng(0)
    for case in range(300):
        n = int(rng.integers(0, 40))
        channels = [int(c) for c in rng.integers(1, 4, size=n)]
        frames = [int(f) for f in rng.integers(2, 400, size=n)]
        per_row, fixed = int(rng.integers(1, 50)), int(rng.integers(0, 100))
        budget = int(rng.integers(200, 40000))
        max_frames = int(rng.integers(50, 3000))
        _check_plan(E, channels, frames, per_row, fixed, budget, max_frames)


def test_plan_waves_written_out(pack):
    from egregora_amd import dfn_engine as E
    rows_bytes = lambda ch, fr: (lambda idx: 10 * sum(ch[i] * fr[i] for i in idx))
    ch, fr = [1, 2, 1, 1, 3], [5, 9, 9, 2, 100]
    # by frames: 4 (300 rows: over max_frames, alone), then 1, 2 (tie: input order), 0, 3
    assert E.plan_waves(ch, fr, rows_bytes(ch, fr), 10 ** 9, 30) == ([[1, 2], [0, 3]], [4])
    # the byte budget closes a wave the same way: 18 + 9 rows = 270 bytes fit 300, 5 more do not
    assert E.plan_waves(ch, fr, rows_bytes(ch, fr), 300, 10 ** 6) == ([[1, 2], [0, 3]], [4])
    assert E.plan_waves([], [], lambda idx: 0, 1, 1) == ([], [])
    assert E.plan_waves([2], [7], lambda idx: 1, 1, 14) == ([[0]], [])
    assert E.plan_waves([2], [7], lambda idx: 1, 1, 13) == ([], [0])
    assert E.ONE_PASS_MAX_FRAMES == 524287


# ---------------------------------------------------------------- registration
_DUMP = r"""
import json, sys
sys.path.insert(0, %r)
from packload import load_pack
p = load_pack()
out = {"keys": sorted(p.NODE_CLASS_MAPPINGS), "display": {k: p.NODE_DISPLAY_NAME_MAPPINGS.get(k) for k in p.NODE_CLASS_MAPPINGS}}
print("DUMP" + json.dumps(out))
"""


def _import_in_child(flag):
    env = {k: v for k, v in os.environ.items() if k != FLAG}
    if flag is not None:
        env[FLAG] = flag
    args = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", _DUMP % str(ROOT)]
    r = subprocess.run(args, env=env, cwd=str(ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("DUMP")][-1][4:])


def test_denoise_batch_node_registration_is_opt_in():
    base = _import_in_child(None)
    assert KEY not in base["keys"]
    assert _import_in_child("0")["keys"] == base["keys"]
    on = _import_in_child("1")
    assert sorted(set(on["keys"]) - set(base["keys"])) == [KEY]
    assert on["display"][KEY] == "Egregora DeepFilterNet Denoise (batch)"


# ---------------------------------------------------------------- node surface
def test_denoise_batch_node_surface_and_batch_expansion(pack, monkeypatch):
    from egregora_amd import dfn_many, egregora_audio_enhance_dfn_batch as B
    single = pack.NODE_CLASS_MAPPINGS["Egregora_DeepFilterNet_Denoise"]
    node = B.NODE_CLASS_MAPPINGS[KEY]
    assert node.INPUT_TYPES() == single.INPUT_TYPES()
    assert node.INPUT_IS_LIST is True and node.OUTPUT_IS_LIST == (True,) and node.RETURN_TYPES == single.RETURN_TYPES == ("AUDIO",)
    assert node.FUNCTION == single.FUNCTION == "execute" and node.CATEGORY == single.CATEGORY
    assert set(dfn_many.WIDGET_DEFAULTS) | {"audio", "dfn_model"} == set(single.INPUT_TYPES()["required"])
    for k, v in dfn_many.WIDGET_DEFAULTS.items():                                   # the single node's own defaults
        assert single.INPUT_TYPES()["required"][k][1]["default"] == v, k
    seen = {}

    def fake(clips, dfn_model="DeepFilterNet2", **kw):
        seen.update(clips=clips, model=dfn_model, kw=kw)
        return [x.to(torch.float64) * 2 for x, _ in clips]                          # wrong dtype on purpose: the node packages

    monkeypatch.setattr(dfn_many, "denoise_many", fake)
    g = torch.Generator().manual_seed(0)
    wf3 = torch.randn(3, 2, 50, generator=g)
    wf1 = torch.randn(1, 20, generator=g)
    (outs,) = node().execute(audio=[{"waveform": wf3, "sample_rate": 16000, "meta": {"tag": 7}}, {"waveform": wf1, "sample_rate": 44100},
                                    torch.ones(2, 6)],
                             dfn_model=["DeepFilterNet3"], strength=[0.25], stereo_mode=["per_channel"], adaptive_vad_source=["none"],
                             device=["auto"])
    clips = seen["clips"]
    assert [tuple(x.shape) for x, _ in clips] == [(2, 50)] * 3 + [(1, 20), (2, 6)] and [sr for _, sr in clips] == [16000] * 3 + [44100, 48000]
    assert all(torch.equal(clips[b][0], wf3[b]) for b in range(3))                  # a [B,C,T] waveform counts as B clips
    assert seen["model"] == "DeepFilterNet3"
    assert seen["kw"] == dict(strength=0.25, stereo_mode="per_channel", adaptive_vad_source="none", device="auto")     # lists unwrapped
    assert isinstance(outs, list) and len(outs) == 5
    for n, (o, (x, sr)) in enumerate(zip(outs, clips)):
        w = o["waveform"]
        assert o["sample_rate"] == sr and w.dtype == torch.float32 and w.device.type == "cpu" and w.is_contiguous()
        assert tuple(w.shape) == (1,) + tuple(x.shape) and torch.equal(w[0], x * 2)
        m = o["meta"]["deepfilternet"]
        assert m["model"] == "DeepFilterNet3" and m["strength"] == 0.25 and m["adaptive_vad_source"] == "none" and m["ceiling"] == 0.98
        assert (o["meta"].get("tag") == 7) == (n < 3)                               # the input's own meta is kept
    with pytest.raises(TypeError):
        node().execute(audio=[torch.ones(2, 6)], no_such_widget=[1])


# ---------------------------------------------------------------- CLI
def test_cli_arguments_pairing_and_skips(pack, monkeypatch, tmp_path, capsys):
    import importlib.util
    from egregora_amd import dfn_many, wavio
    spec = importlib.util.spec_from_file_location("dfn_batch_cli", ROOT / "comfyui-egregora-audio-super-resolution_amd" / "dfn_batch.py")
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    # the batch rule counts channels x frames at 48 kHz
    assert cli.clip_frames(1, 480, 48000) == 3 and cli.clip_frames(2, 16000, 16000) == 2 * 102 and cli.clip_frames(1, 17, 48000) == 2
    a = cli.parser().parse_args(["--model", "DeepFilterNet3", "--in-dir", "i", "--out-dir", "o"])
    assert {k: v for k, v in cli.widgets_of(a).items()} == {k: v for k, v in dfn_many.WIDGET_DEFAULTS.items() if k in cli.widgets_of(a)}
    with pytest.raises(SystemExit):
        cli.parser().parse_args(["--model", "DeepFilterNet1", "--in-dir", "i", "--out-dir", "o"])
    src, dst = tmp_path / "in", tmp_path / "out"
    (src / "b" / "deep").mkdir(parents=True)
    rng = np.random.default_rng(1)
    made = {"z.wav": (1, 16000, 300), "a.wav": (2, 44100, 410), "b/m.wav": (1, 48000, 170), "b/deep/k.wav": (2, 24000, 90)}
    for rel, (ch, sr, n) in made.items():
        wavio.write_wav_pcm16(str(src / rel), (0.1 * rng.standard_normal((n, ch))).astype(np.float32), sr)
    (src / "b" / "broken.wav").write_bytes(b"RIFF\x00\x00\x00\x00WAVEnot a wave file")
    (src / "notes.txt").write_text("not audio")
    assert [str(p) for p in cli.discover(src)] == ["a.wav", "b/broken.wav", "b/deep/k.wav", "b/m.wav", "z.wav"]
    calls = []

    def fake(clips, dfn_model="DeepFilterNet2", **kw):
        calls.append(([(tuple(x.shape), sr) for x, sr in clips], dfn_model, kw))
        return [torch.full(tuple(x.shape), 0.25) for x, _ in clips]

    monkeypatch.setattr(dfn_many, "denoise_many", fake)
    monkeypatch.setenv("EGREGORA_DFN_MODEL_DIR", "unset-by-the-test")               # --model-dir overwrites it; monkeypatch restores
    # frames (channels x frames at 48 kHz): a.wav 4, k.wav 4, m.wav 2, z.wav 3; a budget of 7 closes a batch before k.wav and before z.wav
    rc = cli.main(["--model", "DeepFilterNet3", "--model-dir", str(tmp_path / "m"), "--in-dir", str(src), "--out-dir", str(dst),
                   "--max-frames", "7", "--strength", "0.5", "--adaptive-vad-source", "none", "--no-limit-ceiling"])
    out = capsys.readouterr().out
    assert os.environ["EGREGORA_DFN_MODEL_DIR"] == str(tmp_path / "m")
    assert rc == 1 and out.rstrip().endswith("OK") and "SKIP b/broken.wav" in out
    assert [c[0] for c in calls] == [[((2, 410), 44100)], [((2, 90), 24000), ((1, 170), 48000)], [((1, 300), 16000)]]
    for c in calls:
        assert c[1] == "DeepFilterNet3" and c[2]["strength"] == 0.5 and c[2]["adaptive_vad_source"] == "none" and c[2]["limit_ceiling"] is False
        assert c[2]["stereo_mode"] == "per_channel" and c[2]["ceiling"] == 0.98
    written = sorted(str(p.relative_to(dst)) for p in dst.rglob("*") if p.is_file())
    assert written == ["a.wav", "b/deep/k.wav", "b/m.wav", "z.wav"]
    for rel, (ch, sr, n) in made.items():                                           # each output pairs with its input: rate, channels, length
        y, rate = wavio.read_wav(str(dst / rel))
        assert rate == sr and y.reshape(n, -1).shape == (n, ch)
        assert rel in out
    (src / "b" / "broken.wav").unlink()
    assert cli.main(["--model", "DeepFilterNet2", "--in-dir", str(src), "--out-dir", str(tmp_path / "out2")]) == 0
    assert sum(len(c[0]) for c in calls[3:]) == 4 and len(calls[3:]) == 1           # the default budget: one batch
