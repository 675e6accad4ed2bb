"""Host side of FlashSR's packed path (flashsr_engine.upscale_many): the wave rule, the int64 tables the ragged glue kernels read,
the opt-in batch node's surface and the directory CLI -- no device (upscale_many itself is replaced where a test reaches it)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
WIN, HOP = 3840, 3840 - 375
LENGTHS = (1, 3839, 3840, 3841, WIN + HOP, WIN + HOP + 1)


# ---------------------------------------------------------------- plan_waves
def test_plan_waves_keeps_order_and_never_splits_a_clip(pack, monkeypatch):
    from egregora_amd import flashsr_engine as E
    monkeypatch.setattr(E, "ROWS_PER_PASS", 32)
    # written out by hand: 2 + 2 fit, 30 would make 34 -> new wave; 30 + 1 fit, 64 would not -> new wave; 64 is over the budget
    # and stands alone; the last clip opens a wave of its own
    assert E.plan_waves([2, 2, 30, 1, 64, 2], 32) == [[0, 1], [2, 3], [4], [5]]
    rng = np.random.default_rng(0)
    for max_rows in (32, 64, 100, 1024):
        rows = [int(r) for r in rng.integers(0, 90, size=200)]
        waves = E.plan_waves(rows, max_rows)
        budget = E.wave_budget(max_rows)
        flat = [i for w in waves for i in w]
        assert flat == [i for i, r in enumerate(rows) if r > 0]                       # input order, every clip once, zero rows in no wave
        for n, w in enumerate(waves):
            total = sum(rows[i] for i in w)
            assert total <= budget or len(w) == 1                                      # an oversize clip is alone
            if n + 1 < len(waves):
                assert total + rows[waves[n + 1][0]] > budget                          # a wave closes only before the clip that would not fit
    assert E.plan_waves([], 32) == [] and E.plan_waves([0, 0], 32) == []
    assert E.plan_waves([0, 3, 0, 500, 0], 32) == [[1], [3]]


def test_wave_budget_is_a_multiple_of_rows_per_pass(pack, monkeypatch):
    from egregora_amd import flashsr_engine as E
    monkeypatch.setattr(E, "ROWS_PER_PASS", 32)
    assert [E.wave_budget(m) for m in (32, 33, 63, 64, 100, 1024, 1055)] == [32, 32, 32, 64, 96, 1024, 1024]
    assert E.wave_budget(5) == 32                                                      # never below one pass
    monkeypatch.delenv("EGREGORA_FLASHSR_BATCH_ROWS", raising=False)
    assert E.wave_budget(None) == 1024
    monkeypatch.setenv("EGREGORA_FLASHSR_BATCH_ROWS", "200")
    assert E.wave_budget(None) == 192
    monkeypatch.setattr(E, "ROWS_PER_PASS", 24)
    assert E.wave_budget(100) == 96
    assert E.plan_waves([50, 50], 100) == [[0], [1]]                                    # 100 rounds to 96: the two no longer share a wave


# ---------------------------------------------------------------- tables
def test_chunk_counts_equal_audio_glue_spans(pack):
    from egregora_amd import audio_glue as ag, flashsr_engine as E
    assert [E.n_chunks_for(n, WIN, HOP) for n in LENGTHS] == [1, 1, 1, 2, 2, 3]
    for n in LENGTHS + (0, 20000, 245760, 245761, 2880000):
        for win, hop in ((WIN, HOP), (ag.CHUNK_SAMPLES, ag.HOP_SAMPLES)):
            assert E.n_chunks_for(n, win, hop) == len(ag.spans(n, win, hop)), (n, win, hop)
    assert E.clip_rows(2, 16000, 16000, ag.CHUNK_SAMPLES, ag.HOP_SAMPLES) == 2          # 1 s at 16 kHz: 48000 samples, one chunk
    assert E.clip_rows(2, 1281, 16000, WIN, HOP) == 4                                   # 3843 samples at 48 kHz: two chunks
    assert E.clip_rows(3, 0, 48000, WIN, HOP) == 0
    assert E.resampled_len(11, 44100, 48000) == -(-11 * 160 // 147) and E.resampled_len(7, 48000, 48000) == 7


def test_wave_tables_against_spans(pack):
    """A mono, a stereo and a 3-channel clip side by side, for every length around the chunk boundaries."""
    from egregora_amd import audio_glue as ag, flashsr_engine as E
    for T in LENGTHS:
        shapes = [(1, T), (2, T + 1), (3, max(1, T - 1))]
        offsets, pos = [], 7                                                            # the flat input need not start at 0
        for Cn, n in shapes:
            offsets.append(pos)
            pos += Cn * n + 5                                                           # nor be gap-free
        t = E.wave_tables(shapes, offsets, WIN, HOP)
        rows, ids, tracks = t["rows"], t["ids"], t["tracks"]
        assert rows.dtype == ids.dtype == tracks.dtype == np.int64 and rows.flags.c_contiguous and tracks.flags.c_contiguous
        r = tr = out = 0
        for (Cn, n), off, (co, cc, cn) in zip(shapes, offsets, t["clip_out"]):
            sp = ag.spans(n, WIN, HOP)
            assert (co, cc, cn) == (out, Cn, n)
            for c in range(Cn):                                                         # one table row per track
                assert tracks[tr + c].tolist() == [r + c, Cn, len(sp), n, out + c * n]
            for k, (start, _) in enumerate(sp):                                         # chunk-major, then channel: [n, C, win]
                assert start == k * HOP
                for c in range(Cn):
                    assert rows[r].tolist() == [off + c * n, n, k] and ids[r] == k * Cn + c
                    r += 1
            tr += Cn
            out += Cn * n
        assert r == len(rows) == len(ids) == t["n_rows"] and tr == len(tracks) and out == t["total_out"]
    empty = E.wave_tables([], [], WIN, HOP)
    assert empty["rows"].shape == (0, 3) and empty["tracks"].shape == (0, 5) and empty["total_out"] == 0


def test_resample_table(pack):
    from egregora_amd import resample
    tab, total = resample.poly_track_table([100, 0, 50], [1, 11, 4001], 160, 147)
    n_out = [-(-n * 160 // 147) for n in (1, 11, 4001)]
    assert tab.dtype == np.int64 and tab.tolist() == [[100, 1, 0, n_out[0]], [0, 11, n_out[0], n_out[1]], [50, 4001, n_out[0] + n_out[1], n_out[2]]]
    assert total == sum(n_out)
    assert resample.poly_track_table([0], [10], 3, 1)[0].tolist() == [[0, 10, 0, 30]]


# ---------------------------------------------------------------- node surface
_DUMP = r"""
import json, sys
sys.path.insert(0, %r)
from packload import load_pack
p = load_pack()
out = {"keys": sorted(p.NODE_CLASS_MAPPINGS), "display": {k: p.NODE_DISPLAY_NAME_MAPPINGS.get(k) for k in p.NODE_CLASS_MAPPINGS}}
print("DUMP" + json.dumps(out))
"""


def _import_in_child(flag):
    env = {k: v for k, v in os.environ.items() if k != "EGREGORA_BATCH_NODES"}
    if flag is not None:
        env["EGREGORA_BATCH_NODES"] = flag
    args = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", _DUMP % str(ROOT)]
    r = subprocess.run(args, env=env, cwd=str(ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("DUMP")][-1][4:])


def test_batch_node_registration_is_opt_in():
    base = _import_in_child(None)
    assert "EgregoraAudioUpscalerBatch" not in base["keys"]
    assert _import_in_child("0")["keys"] == base["keys"]
    on = _import_in_child("1")
    assert sorted(set(on["keys"]) - set(base["keys"])) == ["EgregoraAudioUpscalerBatch"]
    assert on["display"]["EgregoraAudioUpscalerBatch"] == "🎧 Audio Super Resolution (FlashSR, batch)"


def test_batch_node_surface_and_batch_expansion(pack, monkeypatch):
    from egregora_amd import egregora_audio_super_resolution_batch as B, flashsr_engine as E
    single = pack.NODE_CLASS_MAPPINGS["EgregoraAudioUpscaler"]
    node = B.NODE_CLASS_MAPPINGS["EgregoraAudioUpscalerBatch"]
    assert node.INPUT_TYPES() == single.INPUT_TYPES() and list(node.INPUT_TYPES()["required"]) == ["audio", "lowpass_input", "output_sr"]
    assert node.INPUT_IS_LIST is True and node.OUTPUT_IS_LIST == (True,) and node.RETURN_TYPES == ("AUDIO",)
    assert node.FUNCTION == single.FUNCTION == "run" and node.CATEGORY == single.CATEGORY
    seen = {}

    def fake(clips, lowpass, output_sr=48000, **kw):
        seen.update(clips=clips, lowpass=lowpass, output_sr=output_sr)
        return [x.to(torch.float64) * 2 for x, _ in clips]                              # wrong dtype on purpose: the node packages

    monkeypatch.setattr(E, "upscale_many", fake)
    g = torch.Generator().manual_seed(0)
    wf3 = torch.randn(3, 2, 50, generator=g)
    wf1 = torch.randn(1, 1, 20, generator=g)
    (outs,) = node().run(audio=[{"waveform": wf3, "sample_rate": 16000}, {"waveform": wf1, "sample_rate": 44100},
                                (np.arange(12, dtype=np.float32).reshape(6, 2), 48000)],
                         lowpass_input=[True], output_sr=["44100"])
    clips = seen["clips"]
    assert [tuple(x.shape) for x, _ in clips] == [(2, 50)] * 3 + [(1, 20), (2, 6)] and [sr for _, sr in clips] == [16000] * 3 + [44100, 48000]
    assert all(torch.equal(clips[b][0], wf3[b]) for b in range(3))                      # B clips, not batch element 0 only
    assert seen["lowpass"] is True and seen["output_sr"] == 44100
    assert isinstance(outs, list) and len(outs) == 5
    for o, (x, _) in zip(outs, clips):
        w = o["waveform"]
        assert o["sample_rate"] == 44100 and w.dtype == torch.float32 and w.device.type == "cpu" and w.is_contiguous()
        assert tuple(w.shape) == (1,) + tuple(x.shape) and torch.equal(w[0], x * 2)
    # the single node keeps "batch element 0 only"
    from egregora_amd import audio_glue
    assert torch.equal(audio_glue.upscaler_input({"waveform": wf3, "sample_rate": 16000})[0], wf3[0])


# ---------------------------------------------------------------- CLI
def test_cli_discovers_sorted_mirrors_the_tree_and_skips_unreadable(pack, monkeypatch, tmp_path, capsys):
    import importlib.util
    from egregora_amd import flashsr_engine as E, wavio
    spec = importlib.util.spec_from_file_location("flashsr_batch_cli", ROOT / "comfyui-egregora-audio-super-resolution_amd" / "flashsr_batch.py")
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    src, dst = tmp_path / "in", tmp_path / "out"
    (src / "b" / "deep").mkdir(parents=True)
    rng = np.random.default_rng(1)
    made = {"z.wav": (1, 16000, 30), "a.wav": (2, 44100, 41), "b/m.wav": (1, 48000, 17), "b/deep/k.wav": (2, 24000, 9)}
    for rel, (ch, sr, n) in made.items():
        wavio.write_wav_pcm16(str(src / rel), (0.1 * rng.standard_normal((n, ch))).astype(np.float32), sr)
    (src / "b" / "broken.wav").write_bytes(b"RIFF\x00\x00\x00\x00WAVEnot a wave file")
    (src / "notes.txt").write_text("not audio")
    assert [str(p) for p in cli.discover(src)] == ["a.wav", "b/broken.wav", "b/deep/k.wav", "b/m.wav", "z.wav"]
    calls = []

    def fake(clips, lowpass, output_sr=48000, **kw):
        calls.append(([(tuple(x.shape), sr) for x, sr in clips], lowpass, output_sr, kw.get("max_rows")))
        return [torch.full((x.shape[0], 2 * x.shape[1]), 0.25) for x, _ in clips]

    monkeypatch.setattr(E, "upscale_many", fake)
    monkeypatch.setenv("EGREGORA_FLASHSR_CKPT_DIR", str(tmp_path))                      # main() only sets it when absent: nothing leaks
    rc = cli.main(["--ckpt-dir", str(tmp_path), "--in-dir", str(src), "--out-dir", str(dst), "--target-sr", "44100", "--max-rows", "40"])
    out = capsys.readouterr().out
    assert rc == 1 and out.rstrip().endswith("OK") and "SKIP b/broken.wav" in out
    order = [c for call in calls for c in call[0]]
    assert order == [((2, 41), 44100), ((2, 9), 24000), ((1, 17), 48000), ((1, 30), 16000)]       # sorted, the broken file left out
    assert all(c[1] is False and c[2] == 44100 and c[3] == E.wave_budget(40) for c in calls)
    written = sorted(str(p.relative_to(dst)) for p in dst.rglob("*") if p.is_file())
    assert written == ["a.wav", "b/deep/k.wav", "b/m.wav", "z.wav"]
    for rel, (ch, sr, n) in made.items():
        y, rate = wavio.read_wav(str(dst / rel))
        assert rate == 44100 and y.reshape(2 * n, -1).shape == (2 * n, ch)
        assert rel in out
    # every file readable: exit status 0
    (src / "b" / "broken.wav").unlink()
    assert cli.main(["--ckpt-dir", str(tmp_path), "--in-dir", str(src), "--out-dir", str(tmp_path / "out2")]) == 0
