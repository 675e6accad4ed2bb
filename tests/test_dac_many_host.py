"""Many clips in one padded pass of the Descript Audio Codec, everything that needs no device: the masking rule in
float64 on the restatement tests/dac_torch.py (rows of their own lengths inside tensors of the longest, noise in the tails; without the
mask it fails), the per-level length tables, plan_waves, the egr_dacmany_* symbols, the opt-in batch nodes and the directory CLI's
.npz round trip with the engine stubbed."""
import ctypes
import importlib.util
import json
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import dac_check as K
import dac_torch as R

ROOT = Path(__file__).resolve().parent.parent
KEYS = ["Egregora_DAC_DecodeBatch", "Egregora_DAC_EncodeBatch"]
FLAG = "EGREGORA_CODEC_BATCH_NODES"
SYMBOLS = ["egr_dacmany_decode", "egr_dacmany_encode", "egr_dacmany_workspace_bytes"]
# (n, rows, seed) per clip: the sets of tests/test_gpu_dac_many.py
CLIPS = {"S": ((2051, 2, 3), (1003, 1, 21), (333, 1, 22), (9, 1, 23), (1, 1, 24), (777, 2, 25), (1024, 1, 26)),
         "O": ((2051, 2, 3), (1003, 1, 21), (11, 1, 22), (333, 2, 23)),
         "G": ((1205, 2, 3), (601, 1, 21), (120, 1, 22))}
NOISE = 1e3


# ---------------------------------------------------------------- the masking rule
class RaggedNet(R.Net):
    """R.Net on rows of their own lengths inside tensors of the longest: before every snake each row's tail (positions at or beyond
    its own length at that level) is overwritten with NOISE-scale noise -- whatever the convolutions left there -- and, with mask
    on, the snake's output is zero there.  levels: {padded length of a level: per-row valid lengths [rows]}."""

    def __init__(self, sd, cfg, levels, mask):
        super().__init__(sd, cfg, torch.float64)
        self.levels, self.mask, self.g = levels, mask, torch.Generator().manual_seed(99)

    def tail(self, L):
        return torch.arange(L)[None, None, :] >= self.levels[L][:, None, None]            # [rows, 1, L]

    def snake(self, x, name):
        t = self.tail(x.shape[-1])
        x = torch.where(t, NOISE * torch.randn(x.shape, generator=self.g, dtype=torch.float64), x)
        y = super().snake(x, name)
        return torch.where(t, torch.zeros_like(y), y) if self.mask else y


def level_table(E, cfg, kind, own):
    """{padded length of the level: tensor of the rows' own lengths there}, from dac_engine.level_lengths."""
    per_row = [E.level_lengths(cfg, kind, v) for v in own]
    padded = [max(col) for col in zip(*per_row)]
    assert len(set(padded)) == len(padded)                                                # a level is known by its padded length
    return {L: torch.tensor([lv[i] for lv in per_row]) for i, L in enumerate(padded)}


def ragged_case(E, name, mask):
    """-> [(ze alone, ze in the wave, y alone, y in the wave)] per row, each cut to the row's own length."""
    cfg, sd, n64, _ = K.model(name)
    xs = [R.test_signal(rows, n, seed)[r] for n, rows, seed in CLIPS[name] for r in range(rows)]
    ns = [x.shape[0] for x in xs]
    frames = [E.lengths(cfg, n)[1] for n in ns]
    x = torch.zeros(len(xs), max(ns))
    for r, v in enumerate(xs):
        x[r, :v.shape[0]] = v                                                             # zeros outside [0, n): k_dac_conv_in's rule
    g = torch.Generator().manual_seed(5)
    zin = NOISE * torch.randn(len(xs), cfg["latent_dim"], max(frames), generator=g, dtype=torch.float64)
    out = []
    with torch.no_grad():
        alone = [(n64.encode_stages(v[None])[-1][0], ) for v in xs]
        zs = [n64.quantize(a[0][None])[0][0] for a in alone]
        for r, z in enumerate(zs):
            zin[r, :, :frames[r]] = z
            if mask:
                zin[r, :, frames[r]:] = 0.0                                               # the mask kernel's rule
        enc = RaggedNet(sd, cfg, level_table(E, cfg, E.ENCODE, ns), mask).encode_stages(x)[-1]
        y = RaggedNet(sd, cfg, level_table(E, cfg, E.DECODE, frames), mask).decode_stages(zin)[1]
        for r in range(len(xs)):
            ya = n64.decode_stages(zs[r][None])[1][0]
            out.append((alone[r][0], enc[r, :, :frames[r]], ya, y[r, :ya.shape[0]]))
    return out


@pytest.mark.parametrize("name", ["S", "O", "G"])
def test_masked_snakes_give_every_row_its_single_call_in_float64(pack, name):
    from egregora_amd import dac_engine as E
    worst = 0.0
    for ze1, ze2, y1, y2 in ragged_case(E, name, True):
        worst = max(worst, K.rel(ze2, ze1), K.rel(y2, y1))
    print(f"{name}: largest relative difference, padded against alone: {worst:.2e}")
    assert worst <= 1e-12


def test_without_the_mask_the_rows_see_their_tails(pack):
    from egregora_amd import dac_engine as E
    diffs = [max(K.rel(ze2, ze1), K.rel(y2, y1)) for ze1, ze2, y1, y2 in ragged_case(E, "S", False)]
    print("S without the mask:", " ".join(f"{d:.1e}" for d in diffs))
    assert max(diffs[2:]) > 1e-3                                                          # every row shorter than the longest
    assert all(d > 1e-12 for d in diffs[2:])


# ---------------------------------------------------------------- length tables
@pytest.mark.parametrize("name", ["S", "O", "W", "G"])
def test_level_lengths_follow_the_restatements_shapes(pack, name):
    from egregora_amd import dac_engine as E
    cfg, sd, n64, n32 = K.model(name)
    h = R.hop(cfg)
    for n in (1, h - 1, h + 1, 333, R.LENGTHS[name]):
        n_pad, F, n_dec = E.lengths(cfg, n)
        enc = E.level_lengths(cfg, E.ENCODE, n)
        dec = E.level_lengths(cfg, E.DECODE, F)
        assert len(enc) == len(cfg["encoder_rates"]) + 1 and len(dec) == len(cfg["decoder_rates"]) + 1
        assert enc[0] == n_pad and enc[-1] == F and dec[0] == F and dec[-1] == n_dec
        for i, s in enumerate(cfg["encoder_rates"]):
            assert enc[i + 1] == E.conv_length(enc[i], s)
        for i, s in enumerate(cfg["decoder_rates"]):
            assert dec[i + 1] == E.convtr_length(dec[i], s)
        if name != "W" or n <= h + 1:                                                     # (the 44 kHz widths are slow on a CPU)
            with torch.no_grad():
                st = n32.encode_stages(torch.zeros(1, n))
                ds, y = n32.decode_stages(torch.zeros(1, cfg["latent_dim"], F))
            assert [t.shape[-1] for t in st[:-1]] == enc and [t.shape[-1] for t in ds] == dec
    assert E.default_pad_frames(15) == 15 and E.default_pad_frames(16) == 16 and E.default_pad_frames(17) == 32 and E.default_pad_frames(1) == 1
    assert E.padded_samples(cfg, E.ENCODE, 7) == 7 * h and E.padded_samples(cfg, E.DECODE, 7) == E.decoded_length(cfg, 7)


# ---------------------------------------------------------------- plan_waves
def _check_plan(E, clips, per_cell, fixed, budget, samples_per_frame, share=None):
    bytes_for = lambda rows, pad: fixed + per_cell * rows * pad
    samples_for = lambda pad: pad * samples_per_frame
    waves, alone = E.plan_waves(clips, bytes_for, budget, samples_for, share)
    limit = E.MAX_PAD_SHARE if share is None else share
    seen = sorted([i for w in waves for i in w.clips] + list(alone))
    assert seen == list(range(len(clips)))                                                # whole clips, each once
    flat = [i for w in waves for i in w.clips]
    key = [(-clips[i][1], i) for i in flat]
    assert key == sorted(key)                                                             # longest first, ties in input order
    ok = lambda rows, pad: (rows <= E.MANY_MAX_ROWS and rows * samples_for(pad) < E.MANY_MAX_SAMPLES and rows * pad <= E.MANY_MAX_FRAMES
                            and bytes_for(rows, pad) <= budget)
    for w in waves:
        assert w.rows == sum(clips[i][0] for i in w.clips) and w.pad_frames == E.default_pad_frames(clips[w.clips[0]][1])
        assert ok(w.rows, w.pad_frames), w
        if len(w.clips) > 1:
            used = sum(clips[i][0] * clips[i][1] for i in w.clips)
            assert 1 - used / (w.rows * w.pad_frames) <= limit + 1e-12, w
    for i in alone:
        assert not ok(clips[i][0], E.default_pad_frames(clips[i][1])), i
    # greedy: the clip that opens wave k + 1 did not fit wave k
    for a, b in zip(waves, waves[1:]):
        r, f = clips[b.clips[0]]
        rows, used = a.rows + r, sum(clips[i][0] * clips[i][1] for i in a.clips) + r * f
        assert not ok(rows, a.pad_frames) or 1 - used / (rows * a.pad_frames) > limit, (a, b)
    return waves, alone


def test_plan_waves_properties(pack):
    from egregora_amd import dac_engine as E
    rng = np.random.default_rng(3)
    for trial in range(40):
        n = int(rng.integers(1, 30))
        clips = [(int(rng.integers(1, 3)), int(rng.integers(1, 1200))) for _ in range(n)]
        budget = int(rng.choice([10 ** 4, 10 ** 5, 10 ** 7]))
        _check_plan(E, clips, 64, 1000, budget, 512, float(rng.choice([0.1, 0.25, 0.5])))
    # every limit closes a wave on its own
    clips = [(2, 1024)] * 8
    waves, alone = _check_plan(E, clips, 1, 0, 10 ** 12, 512)
    assert len(waves) == 1 and not alone
    waves, _ = _check_plan(E, clips, 1, 0, 4 * 1024 + 1, 512)                             # bytes: two clips a wave
    assert [len(w.clips) for w in waves] == [2] * 4
    waves, _ = _check_plan(E, clips, 0, 1, 10, E.MANY_MAX_SAMPLES // (1024 * 6) + 1)      # rows x samples: 6 rows would reach 2^31
    assert [w.rows for w in waves] == [4, 4, 4, 4]
    big = [(2, E.MANY_MAX_FRAMES // 4)] * 3
    waves, alone = _check_plan(E, big, 0, 1, 10, 1)                                       # rows x pad_frames: 4 rows are the bound
    assert [w.rows for w in waves] == [4, 2] and not alone
    waves, alone = _check_plan(E, [(1, 100), (1, 1000), (1, 400), (1, 760)], 1, 0, 10 ** 9, 8, 0.25)      # share: 1000 pads to 1008; 400 would leave 0.29 empty
    assert [w.clips for w in waves] == [(1, 3), (2,), (0,)] and not alone
    # a clip above a limit on its own takes the single path, the others are planned
    waves, alone = _check_plan(E, [(1, 50), (3, 4000), (1, 48)], 1, 0, 5000, 8, 0.25)
    assert alone == [1] and [w.clips for w in waves] == [(0, 2)]
    with pytest.raises(ValueError):
        E.plan_waves([(0, 5)], lambda r, p: 1, 10, lambda p: p)
    assert 0.0 < E.MAX_PAD_SHARE <= 0.25                                                  # the default is read at the call
    waves, _ = _check_plan(E, [(1, 1000), (1, 990), (1, 500)], 1, 0, 10 ** 9, 8)
    assert [w.clips for w in waves] == [(0, 1), (2,)]


# ---------------------------------------------------------------- symbols
def test_many_symbols_are_declared_exported_and_bound(pack):
    from egregora_amd import native
    txt = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "egregora_amd.h").read_text(), flags=re.S)
    declared = sorted(s for s in set(re.findall(r"\b(egr_[a-z0-9_]+)\s*\(", txt)) if s.startswith("egr_dacmany_"))
    assert declared == SYMBOLS
    lib = ctypes.CDLL(str(native.LIB_PATH))
    for s in SYMBOLS:
        assert hasattr(lib, s) and s in native.SIGNATURES, s
    assert native.lib().egr_abi_version() == native.ABI_VERSION == 5
    assert native.lib().egr_dacmany_workspace_bytes(None, 1, 16, 0) == 0                  # no handle: nothing to size


# ---------------------------------------------------------------- registration
_DUMP = """
import json, sys
sys.path.insert(0, %r)
from packload import load_pack
p = load_pack()
print("DUMP" + json.dumps({"keys": sorted(p.NODE_CLASS_MAPPINGS), "display": dict(p.NODE_DISPLAY_NAME_MAPPINGS)}))
"""


def _import_in_child(flag):
    env = {k: v for k, v in os.environ.items() if not (k.startswith("EGREGORA_") and k.endswith("_NODES"))}
    if flag is not None:
        env[FLAG] = flag
    args = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", _DUMP % str(ROOT)]
    r = subprocess.run(args, env=env, cwd=str(ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("DUMP")][-1][4:])


def test_batch_nodes_are_opt_in():
    base = _import_in_child(None)
    assert not set(KEYS) & set(base["keys"])
    assert _import_in_child("0")["keys"] == base["keys"]
    on = _import_in_child("1")
    assert sorted(set(on["keys"]) - set(base["keys"])) == KEYS
    assert on["display"][KEYS[1]] == "Egregora DAC Encode (batch)" and on["display"][KEYS[0]] == "Egregora DAC Decode (batch)"


def test_batch_nodes_have_the_single_nodes_surface_and_expand_batches(pack, monkeypatch):
    from egregora_amd import dac_many, egregora_audio_codec_dac as single, egregora_audio_codec_dac_batch as B
    for key, one in (("Egregora_DAC_EncodeBatch", single.Egregora_DAC_Encode), ("Egregora_DAC_DecodeBatch", single.Egregora_DAC_Decode)):
        node = B.NODE_CLASS_MAPPINGS[key]
        assert node.INPUT_TYPES() == one.INPUT_TYPES() and node.RETURN_TYPES == one.RETURN_TYPES and node.RETURN_NAMES == one.RETURN_NAMES
        assert node.INPUT_IS_LIST is True and node.OUTPUT_IS_LIST == (True, True) and node.FUNCTION == "execute" and node.CATEGORY == one.CATEGORY
    seen = {}

    def fake_encode(clips, model_type="44khz", **kw):
        seen.update(clips=clips, model_type=model_type)
        return [{"z": torch.full((x.shape[0], 4, 3), float(i)), "codes": torch.full((x.shape[0], 2, 3), i, dtype=torch.int64), "sample_rate": sr,
                 "model_sample_rate": 44100, "n_samples": x.shape[1]} for i, (x, sr) in enumerate(clips)]

    monkeypatch.setattr(dac_many, "encode_many", fake_encode)
    wf3 = torch.randn(3, 2, 50, generator=torch.Generator().manual_seed(0))
    dicts, logs = B.Egregora_DAC_EncodeBatch().execute(audio=[{"waveform": wf3, "sample_rate": 16000}, {"waveform": torch.ones(1, 20), "sample_rate": 44100}],
                                                       model_type=["24khz"], device=["auto"])
    assert seen["model_type"] == "24khz" and [tuple(x.shape) for x, _ in seen["clips"]] == [(2, 50)] * 3 + [(1, 20)]
    assert all(torch.equal(seen["clips"][b][0], wf3[b]) for b in range(3))                # a [B,C,T] waveform counts as B clips
    assert len(dicts) == len(logs) == 2 and logs[0] == "DAC encode ok: model=24khz, B=3, C=2, sr=16000->44100"
    assert [set(d) for d in dicts] == [{"model_type", "sample_rate", "model_sample_rate", "latents", "codes"}] * 2
    assert [len(d["latents"]) for d in dicts] == [3, 1] and [d["sample_rate"] for d in dicts] == [16000, 44100]
    assert float(dicts[0]["latents"][2][0][0, 0, 0]) == 2.0 and int(dicts[1]["codes"][0][0, 0, 0]) == 3 and isinstance(dicts[0]["latents"][0], list)

    def fake_decode(items, model_type="44khz", **kw):
        seen.update(items=items, model_type=model_type)
        return [torch.full((d["z" if "z" in d else "codes"].shape[0], 7), float(i)) for i, d in enumerate(items)]

    monkeypatch.setattr(dac_many, "decode_many", fake_decode)
    audios, logs = B.Egregora_DAC_DecodeBatch().execute(codes=[dicts[0], {k: v for k, v in dicts[1].items() if k != "latents"}], device=["auto"])
    assert ["z" in d for d in seen["items"]] == [True] * 3 + [False] and [d["sample_rate"] for d in seen["items"]] == [16000] * 3 + [44100]
    assert [tuple(a["waveform"].shape) for a in audios] == [(3, 2, 7), (1, 1, 7)] and [a["sample_rate"] for a in audios] == [16000, 44100]
    assert float(audios[0]["waveform"][2, 0, 0]) == 2.0 and float(audios[1]["waveform"][0, 0, 0]) == 3.0
    assert logs[1] == "DAC decode ok: model=24khz, B=1, C=1, 44100->44100"
    with pytest.raises(ValueError, match="codes.latents empty"):
        B.Egregora_DAC_DecodeBatch().execute(codes=[{"model_type": "44khz"}])


# ---------------------------------------------------------------- CLI
def test_cli_npz_round_trip(pack, monkeypatch, tmp_path, capsys):
    from egregora_amd import dac_many, wavio
    spec = importlib.util.spec_from_file_location("dac_batch_cli", ROOT / "comfyui-egregora-audio-super-resolution_amd" / "dac_batch.py")
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    with pytest.raises(SystemExit):
        cli.parser().parse_args(["--model-type", "48khz", "--in-dir", "i", "--out-dir", "o"])
    src, mid, dst = tmp_path / "in", tmp_path / "codes", tmp_path / "out"
    (src / "b").mkdir(parents=True)
    rng = np.random.default_rng(1)
    made = {"z.wav": (1, 16000, 300), "a.wav": (2, 44100, 410), "b/m.wav": (1, 48000, 170)}
    for rel, (ch, sr, n) in made.items():
        wavio.write_wav_pcm16(str(src / rel), (0.1 * rng.standard_normal((n, ch))).astype(np.float32), sr)
    (src / "b" / "broken.wav").write_bytes(b"RIFF\x00\x00\x00\x00WAVEnot a wave file")
    NCB, HOP = 3, 8
    calls = []

    def fake_encode(clips, model_type="44khz", **kw):
        calls.append(("enc", [(tuple(x.shape), sr) for x, sr in clips], model_type))
        return [{"z": None, "codes": torch.full((x.shape[0], NCB, -(-x.shape[1] // HOP)), 5, dtype=torch.int64), "sample_rate": sr,
                 "model_sample_rate": 44100, "n_samples": x.shape[1]} for x, sr in clips]

    def fake_decode(items, model_type="44khz", **kw):
        calls.append(("dec", [(tuple(d["codes"].shape), d["codes"].dtype, d["sample_rate"]) for d in items], model_type))
        return [torch.full((d["codes"].shape[0], d["codes"].shape[2] * HOP), 0.25) for d in items]      # longer than n_samples: trimmed

    monkeypatch.setattr(dac_many, "encode_many", fake_encode)
    monkeypatch.setattr(dac_many, "decode_many", fake_decode)
    monkeypatch.setenv("EGREGORA_DAC_MODEL_DIR", "unset-by-the-test")
    rc = cli.main(["--model-type", "44khz", "--model-dir", str(tmp_path / "m"), "--in-dir", str(src), "--out-dir", str(mid)])
    out = capsys.readouterr().out
    assert os.environ["EGREGORA_DAC_MODEL_DIR"] == str(tmp_path / "m")
    assert rc == 1 and out.rstrip().endswith("OK") and "SKIP b/broken.wav" in out
    assert calls == [("enc", [((2, 410), 44100), ((1, 170), 48000), ((1, 300), 16000)], "44khz")]
    assert sorted(str(p.relative_to(mid)) for p in mid.rglob("*") if p.is_file()) == ["a.npz", "b/m.npz", "z.npz"]
    for rel, (ch, sr, n) in made.items():
        with np.load(str((mid / rel).with_suffix(".npz"))) as f:
            assert sorted(f.files) == ["codes", "model_sample_rate", "model_type", "n_samples", "sample_rate"]
            assert f["codes"].dtype == np.int32 and f["codes"].shape == (ch, NCB, -(-n // HOP)) and int(f["codes"].max()) == 5
            assert int(f["sample_rate"]) == sr and int(f["model_sample_rate"]) == 44100 and str(f["model_type"]) == "44khz" and int(f["n_samples"]) == n
    assert cli.main(["--model-type", "44khz", "--in-dir", str(mid), "--out-dir", str(dst), "--decode", "--max-seconds", "0.012"]) == 0
    # channel-seconds: a 0.0186, m 0.0035, z 0.0188: a budget of 0.012 puts every file in a batch of its own
    assert [c[0] for c in calls[1:]] == ["dec"] * 3 and calls[1][1] == [((2, NCB, 52), torch.int32, 44100)]
    for rel, (ch, sr, n) in made.items():
        y, rate = wavio.read_wav(str(dst / rel))
        assert rate == sr and y.reshape(n, -1).shape == (n, ch)                           # trimmed to n_samples at the original rate
    with pytest.raises(SystemExit, match="model type"):
        cli.main(["--model-type", "24khz", "--in-dir", str(mid), "--out-dir", str(dst), "--decode"])
