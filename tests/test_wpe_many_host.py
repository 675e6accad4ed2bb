"""Many-clip WPE, everything that needs no device: the wave planner, the host-only workspace entry point and its
refusals, the exported symbols, the opt-in registration of the batch node, the widget and passthrough rules of wpe_many, and a host walk
of the new index code of csrc/egr_wpe_index.h under the address and undefined-behaviour sanitizers (a stand-alone program)."""
import ctypes
import json
import os
import re
import shutil
import subprocess
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
KEY = "Egregora_WPE_DereverbBatch"
SYMBOLS = ["egr_wpemany_dereverb", "egr_wpemany_workspace_bytes"]
SINGLE = ["egr_wpe_dereverb", "egr_wpe_frames", "egr_wpe_istft", "egr_wpe_iterate", "egr_wpe_stft", "egr_wpe_workspace_bytes"]

_DUMP = """
import json, sys
sys.path.insert(0, %r)
from packload import load_pack
p = load_pack()
print("DUMP" + json.dumps({"keys": sorted(p.NODE_CLASS_MAPPINGS), "display_keys": sorted(p.NODE_DISPLAY_NAME_MAPPINGS)}))
"""
_SWITCHES = ("EGREGORA_ENHANCE_NODES", "EGREGORA_ENHANCE_BATCH_NODES", "EGREGORA_EVAL_NODES")


def _keys_in_child(**flags):
    env = {k: v for k, v in os.environ.items() if k not in _SWITCHES}
    env.update(flags)
    args = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", _DUMP % str(ROOT)]
    r = subprocess.run(args, env=env, cwd=str(ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("DUMP")][-1][4:])


def _table(rows):
    return (ctypes.c_int64 * (3 * len(rows)))(*[int(v) for r in rows for v in r])


def test_plan_waves(pack):
    from egregora_amd import wpe_engine, wpe_many
    specs = [(1, 40000), (2, 32000), (1, 30000), (2, 500000), (1, 44000), (2, 16000), (3, 9000), (1, 12000), (2, 20000), (1, 400)]
    w = dict(n_fft=256, hop=64, taps=5)
    one = lambda i: wpe_engine.many_workspace_bytes([specs[i][1]], specs[i][0], w["n_fft"], w["hop"], w["taps"])
    budget = one(1) + one(5) + 4096                     # the two short stereo clips fit one wave, the 500000-sample clip fits none
    assert one(3) > budget > max(one(i) for i in range(len(specs)) if i != 3)
    waves, alone, wave_bytes = wpe_many.plan_waves(specs, budget, **w)
    assert alone == [3]
    assert sorted([i for wv in waves for i in wv] + alone) == list(range(len(specs)))       # every clip exactly once
    assert len(waves) == len(wave_bytes)
    for wv, b in zip(waves, wave_bytes):
        assert len({specs[i][0] for i in wv}) == 1 and wv == sorted(wv)                           # one channel count, input order
        need = wpe_engine.many_workspace_bytes([specs[i][1] for i in wv], specs[wv[0]][0], w["n_fft"], w["hop"], w["taps"])
        assert 0 < need == b <= budget
    assert [1, 5] in waves and sum(1 for wv in waves if specs[wv[0]][0] == 1) >= 2                # mono needs more than one wave
    # a roomy budget: one wave per channel count, nobody alone; the environment variable is the default budget
    waves, alone, _ = wpe_many.plan_waves(specs, 1 << 40, **w)
    assert alone == [] and sorted(map(tuple, waves)) == [(0, 2, 4, 7, 9), (1, 3, 5, 8), (6,)]
    old = os.environ.get("EGREGORA_WPE_WAVE_GB")
    os.environ["EGREGORA_WPE_WAVE_GB"] = repr(budget / (1 << 30))
    try:
        assert wpe_many.plan_waves(specs, **w)[1] == [3]
    finally:
        if old is None:
            del os.environ["EGREGORA_WPE_WAVE_GB"]
        else:
            os.environ["EGREGORA_WPE_WAVE_GB"] = old
    assert wpe_many.DEFAULT_WAVE_GB == 16.0 and wpe_many.plan_waves([]) == ([], [], [])


def test_workspace_bytes_and_refused_tables(pack):
    from egregora_amd import native, wpe_engine
    L = native.lib()
    for lengths in ([16000], [16000, 1, 63, 48000, 777]):
        tab, xf, yf = wpe_engine.clip_table(lengths, 2, 256, 64)
        many = L.egr_wpemany_workspace_bytes(tab, len(lengths), 2, 256, 64, 10)
        singles = sum(L.egr_wpe_workspace_bytes(2, n, 256, 64, 10) for n in lengths)
        assert many >= singles > 0 and many - singles <= 256 + 96 * len(lengths)                  # the blocks plus small tables
        assert xf == 2 * sum(lengths) and yf == 2 * sum(wpe_engine.out_length(n, 256, 64) for n in lengths)
        lay = wpe_engine.many_layout(lengths, 2, 256, 64)
        assert max(v["flags"] for v in lay) < many and sorted(v["Y"] for v in lay)[0] == 0
    ok = [(0, 1000, 0), (2000, 500, 4000)]
    assert L.egr_wpemany_workspace_bytes(_table(ok), 2, 2, 256, 64, 10) > 0
    frames_limit = (2 ** 31 - 4096) * 64                                                           # n of about 2^31 - 4096 frames
    refused = {
        "no clips": (_table(ok), 0, 2, 256, 64, 10),
        "null table": (None, 2, 2, 256, 64, 10),
        "no channels": (_table(ok), 2, 0, 256, 64, 10),
        "negative x offset": (_table([(-1, 1000, 0)]), 1, 2, 256, 64, 10),
        "negative y offset": (_table([(0, 1000, -8)]), 1, 2, 256, 64, 10),
        "n = 0": (_table([(0, 1000, 0), (2000, 0, 4000)]), 2, 2, 256, 64, 10),
        "hop does not divide": (_table(ok), 2, 2, 1024, 192, 10),
        "n_fft / hop < 2": (_table(ok), 2, 2, 256, 256, 10),
        "odd n_fft": (_table(ok), 2, 1, 255, 85, 3),
        "n_fft > 4096": (_table(ok), 2, 1, 8192, 2048, 3),
        "prime factor 17": (_table(ok), 2, 1, 68, 34, 3),
        "K > 64": (_table(ok), 2, 3, 256, 64, 22),
        "taps < 1": (_table(ok), 2, 2, 256, 64, 0),
        "too many frames": (_table([(0, 1000, 0), (2000, frames_limit, 4000)]), 2, 1, 256, 64, 3),
    }
    for why, args in refused.items():
        assert L.egr_wpemany_workspace_bytes(*args) == 0, why
    assert L.egr_wpemany_workspace_bytes(_table([(0, frames_limit - 4096 * 64, 0)]), 1, 1, 256, 64, 3) > 0      # just inside


def test_symbols_are_declared_exported_and_bound(pack):
    from egregora_amd import native
    txt = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "egregora_amd.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(egr_[a-z0-9_]+)\s*\(", txt))
    assert sorted(s for s in declared if s.startswith("egr_wpemany_")) == SYMBOLS
    assert sorted(s for s in declared if s.startswith("egr_wpe_")) == SINGLE                       # no new symbol takes that prefix
    lib = ctypes.CDLL(str(native.LIB_PATH))
    for s in SYMBOLS:
        assert hasattr(lib, s) and s in native.SIGNATURES, s
    assert native.lib().egr_abi_version() == native.ABI_VERSION == 5


def test_batch_node_registration_is_opt_in():
    base = _keys_in_child()
    assert KEY not in base["keys"] and KEY not in base["display_keys"]
    enh = _keys_in_child(EGREGORA_ENHANCE_NODES="1")
    assert KEY not in enh["keys"] and "Egregora_WPE_Dereverb" in enh["keys"]
    assert _keys_in_child(EGREGORA_ENHANCE_BATCH_NODES="0")["keys"] == base["keys"]
    on = _keys_in_child(EGREGORA_ENHANCE_BATCH_NODES="1")
    assert sorted(set(on["keys"]) - set(base["keys"])) == [KEY] and on["keys"] == on["display_keys"]


def test_widgets_limits_and_passthrough(pack, capsys):
    from egregora_amd import egregora_audio_enhance_wpe as ew, egregora_audio_enhance_wpe_batch as eb, wpe_many
    x = torch.randn(2, 500, generator=torch.Generator().manual_seed(3))
    with pytest.raises(TypeError, match="tapz"):
        wpe_many.dereverb_many([(x, 16000)], tapz=3)
    with pytest.raises(TypeError, match="tapz"):
        wpe_many.meta_for({}, tapz=3)
    with pytest.raises(TypeError):
        eb.Egregora_WPE_DereverbBatch().execute([{"waveform": x[None], "sample_rate": 16000}], tapz=[3])
    # K > 64 and a bad n_fft raise before any device is asked for (this machine may have none)
    with pytest.raises(RuntimeError, match="K <= 64"):
        wpe_many.dereverb_many([(x, 16000), (torch.zeros(3, 4000), 16000)], taps=22, n_fft=256, hop=64)
    with pytest.raises(RuntimeError, match="<= 4096"):
        wpe_many.dereverb_many([(x, 16000)], n_fft=8192, hop=2048)
    with pytest.raises(ValueError):
        wpe_many.dereverb_many([(torch.zeros(500), 16000)])
    # unsupported framings and empty clips come back unchanged, with the reference's warning, without a device
    for n_fft, hop in ((256, 256), (1024, 192), (256, 1024)):
        stats = {}
        ys = wpe_many.dereverb_many([(x, 16000), (x[:1].double(), 8000)], stats=stats, taps=5, delay=2, iterations=2, n_fft=n_fft, hop=hop)
        assert torch.equal(ys[0], x) and torch.equal(ys[1], x[:1]) and ys[1].dtype == torch.float32
        assert stats == {"waves": 0, "alone": 0, "wave_bytes": [], "wave_clips": []}
        assert capsys.readouterr().out.count("Warning: WPE processing failed") == 2
    (y,) = wpe_many.dereverb_many([(torch.zeros(2, 0), 16000)])
    assert tuple(y.shape) == (2, 0) and "Warning: WPE processing failed: empty input" in capsys.readouterr().out
    assert wpe_many.dereverb_many([]) == []
    # the meta is the single node's
    (single,) = ew.Egregora_WPE_Dereverb().execute({"waveform": x[None], "sample_rate": 16000, "meta": {"k": 1}}, 5, 2, 2, 256, 256, True)
    assert wpe_many.meta_for({"k": 1}, taps=5, delay=2, iterations=2, n_fft=256, hop=256) == single["meta"]
    assert wpe_many.meta_for(None)["wpe"] == {"taps": 10, "delay": 3, "iterations": 3, "n_fft": 1024, "hop": 256}
    # the batch node passes through the same way: list in, list out, a [B,C,T] dict counts as B clips
    (outs,) = eb.Egregora_WPE_DereverbBatch().execute([{"waveform": torch.stack([x, -x]), "sample_rate": 16000, "meta": {"k": 1}},
                                                       {"waveform": x[None, :1], "sample_rate": 8000}],
                                                      taps=[5], delay=[2], iterations=[2], n_fft=[256], hop=[256], use_float32=[True])
    assert [tuple(o["waveform"].shape) for o in outs] == [(1, 2, 500), (1, 2, 500), (1, 1, 500)]
    assert torch.equal(outs[1]["waveform"][0], -x) and outs[0]["meta"] == single["meta"] and outs[2]["sample_rate"] == 8000


def test_many_index_code_under_host_sanitizers(tmp_path):
    """The many-clip part of csrc/egr_wpe_index.h compiled for the host with -fsanitize=address,undefined and walked over ragged
    tables (tools/wpemany_host_check.cpp); tools/wpe_host_check.cpp, which includes the same header, must still build."""
    rocm_clang = Path(os.environ.get("ROCM_PATH", "/opt/rocm")) / "llvm" / "bin" / "clang++"
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or (str(rocm_clang) if rocm_clang.exists() else None)
    assert cxx is not None, "no host C++ compiler, not even ROCm's clang++: the sanitizer walk cannot run"
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    exe = tmp_path / "wpemany_host_check"
    r = subprocess.run([cxx] + flags + [str(ROOT / "tools" / "wpemany_host_check.cpp"), "-o", str(exe)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "all tables pass" in r.stdout and "thousand " in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    r = subprocess.run([cxx] + flags + ["-fsyntax-only", str(ROOT / "tools" / "wpe_host_check.cpp")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
