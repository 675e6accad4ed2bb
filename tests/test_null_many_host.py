"""The many-pair null test, everything that needs no device: the exported symbols, the host-only workspace entry points
and their refusals (each names the pair or row in egr_last_error), the grouping by transform length and by (rate, channels), the wave
planner, the opt-in registration of the two batch nodes, the list rules of the nodes, and a host walk of csrc/egr_null_index.h under the
address and undefined-behaviour sanitizers (a stand-alone program)."""
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
KEYS = ["Audio Null Test (batch)", "Null Test (Full) (batch)"]
SYMBOLS = ["egr_nullmany_delays", "egr_nullmany_delays_workspace_bytes", "egr_nullmany_mix", "egr_nullmany_mix_workspace_bytes",
           "egr_nullmany_shift_fir", "egr_nullmany_shift_fir_workspace_bytes"]
GRID_256 = (2 ** 32 - 1) // 256

_DUMP = """
import json, sys
sys.path.insert(0, %r)
from packload import load_pack
p = load_pack()
print("DUMP" + json.dumps({"keys": sorted(p.NODE_CLASS_MAPPINGS), "display_keys": sorted(p.NODE_DISPLAY_NAME_MAPPINGS)}))
"""
_SWITCHES = ("EGREGORA_EVAL_NODES", "EGREGORA_EVAL_BATCH_NODES", "EGREGORA_ENHANCE_NODES", "EGREGORA_ENHANCE_BATCH_NODES",
             "EGREGORA_NULLTEST_BATCH_NODES", "EGREGORA_BATCH_NODES", "EGREGORA_CODEC_NODES", "EGREGORA_CODEC_BATCH_NODES",
             "EGREGORA_DENOISE_BATCH_NODES", "EGREGORA_FATLLAMA_BATCH_NODES")


def _keys_in_child(**flags):
    env = {k: v for k, v in os.environ.items() if k not in _SWITCHES}
    env.update(flags)
    args = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", _DUMP % str(ROOT)]
    r = subprocess.run(args, env=env, cwd=str(ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("DUMP")][-1][4:])


def _tab(rows):
    flat = [int(v) for r in rows for v in r]
    return (ctypes.c_int64 * len(flat))(*flat)


def test_symbols_are_declared_exported_and_bound(pack):
    from egregora_amd import native
    txt = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "egregora_amd.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(egr_[a-z0-9_]+)\s*\(", txt))
    assert sorted(s for s in declared if s.startswith("egr_nullmany_")) == SYMBOLS
    assert sorted(s for s in native.SIGNATURES if s.startswith("egr_nullmany_")) == SYMBOLS
    lib = ctypes.CDLL(str(native.LIB_PATH))
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    assert native.lib().egr_abi_version() == native.ABI_VERSION == 5


def test_delays_workspace_sizes_and_refusals(pack):
    from egregora_amd import native
    L = native.lib()
    f = L.egr_nullmany_delays_workspace_bytes
    # (offset a, channels a, stride a, offset b, channels b, stride b, n_common, max_shift); 2 * 256 IS 512: the length stays
    ok = [(0, 1, 300, 300, 2, 256, 256, 160), (900, 3, 200, 1500, 1, 400, 200, 254), (2000, 1, 129, 2200, 1, 129, 129, 0)]
    size = f(_tab(ok), 3, 512)
    rows = 3 * 3 * 512 * 8                                                   # z, the correlation and the passes' state: 24 n bytes per pair
    assert 3 * 8 * 8 + rows <= size <= 3 * 8 * 8 + rows + 4 * 256
    refused = {
        "empty side": ((ok + [(0, 1, 10, 0, 1, 10, 0, 5)], 4, 512), "pair 3: a common length below 1"),
        "stride below n": ((ok[:1] + [(0, 1, 199, 0, 1, 400, 200, 5)], 2, 512), "pair 1: channels outside 1 .. 65535 or a row stride below n"),
        "no channels": (([(0, 0, 300, 300, 1, 300, 256, 5)] + ok, 4, 512), "pair 0: channels"),
        "max_shift = n/2 - 1": ((ok + [(0, 1, 256, 0, 1, 256, 256, 255)], 4, 512), "pair 3: max_shift out of range"),
        "max_shift < 0": ((ok[:2] + [(0, 1, 256, 0, 1, 256, 256, -1)], 3, 512), "pair 2: max_shift out of range"),
        "one sample past the power of two": ((ok + [(0, 1, 257, 0, 1, 257, 257, 5)], 4, 512), "pair 3: its common length 257 belongs to the transform length 1024"),
        "a shorter group's pair": ((ok + [(0, 1, 128, 0, 1, 128, 128, 5)], 4, 512), "pair 3: its common length 128 belongs to the transform length 256"),
        "negative offset": ((ok + [(-4, 1, 256, 0, 1, 256, 256, 5)], 4, 512), "pair 3: an offset"),
        "offset past the index type": ((ok + [(2 ** 62, 1, 256, 0, 1, 256, 256, 5)], 4, 512), "pair 3: an offset"),
        "n not a power of two": ((ok, 3, 500), "n=500"),
        "no pairs": ((ok, 0, 512), "no pairs"),
        "a group over 65535 rows": ((ok, 65536, 512), "pair 65535"),
    }
    for why, ((rows_, n_pairs, n), msg) in refused.items():
        assert f(_tab(rows_), n_pairs, n) == 0, why
        assert msg in native.last_error(), (why, native.last_error())
    # totals over one grid: pack tiles of all pairs together stay at or below 2^24 - 1 workgroups
    big_n = 2 ** 24
    per = big_n // 256
    row = (0, 1, big_n // 2, 0, 1, big_n // 2, big_n // 2, 5)
    fits = GRID_256 // per
    assert f(_tab([row] * fits), fits, big_n) > 0
    assert f(_tab([row] * (fits + 1)), fits + 1, big_n) == 0 and f"pair {fits}: the running total" in native.last_error()
    # the call refuses the same tables before it touches a pointer: it needs a plan for the length first, so only its null-plan refusal is host-only
    assert L.egr_nullmany_delays(None, None, None, _tab(ok), 3, None, None, 0, None, None) != 0 and "null plan" in native.last_error()


def test_shift_fir_workspace_sizes_and_refusals(pack):
    from egregora_amd import native
    L = native.lib()
    f = L.egr_nullmany_shift_fir_workspace_bytes
    # (input offset, n_in, shift, taps row or -1, output offset, n_out)
    ok = [(0, 300, 3, 0, 0, 255), (300, 300, -2, 1, 255, 256), (600, 1, 0, -1, 511, 257), (700, 9000, 9000, -1, 768, 300)]
    size = f(_tab(ok), 4, 2, 64)
    assert 4 * 8 * 8 <= size <= 4 * 8 * 8 + 256
    assert f(_tab([r[:3] + (-1,) + r[4:] for r in ok]), 4, 0, 0) == size               # no row has taps: no table, taps = 0
    refused = {
        "empty input": ((ok + [(0, 0, 0, -1, 0, 10)], 5, 2, 64), "row 4: a length below 1"),
        "empty output": (([(0, 10, 0, -1, 0, 0)] + ok, 5, 2, 64), "row 0: a length below 1"),
        "taps row past the table": ((ok + [(0, 10, 0, 2, 0, 10)], 5, 2, 64), "row 4: its row of the taps table"),
        "taps row without a table": ((ok[:1], 1, 0, 0), "row 0: its row of the taps table"),
        "negative offset": ((ok + [(0, 10, 0, -1, -1, 10)], 5, 2, 64), "row 4: an offset"),
        "shift past the index type": ((ok + [(0, 10, 2 ** 62, -1, 0, 10)], 5, 2, 64), "row 4: an offset"),
        "tile total": ((ok + [(0, 10, 0, -1, 0, 256 * GRID_256)], 5, 2, 64), "row 4: the running total"),
        "too many taps": ((ok, 4, 2, 4097), "taps=4097"),
        "a table without taps": ((ok, 4, 2, 0), "taps=0"),
        "no rows": ((ok, 0, 2, 64), "no rows"),
    }
    for why, (args, msg) in refused.items():
        assert f(_tab(args[0]), *args[1:]) == 0, why
        assert msg in native.last_error(), (why, native.last_error())
    assert f(_tab([(0, 10, 0, -1, 0, 256 * GRID_256)]), 1, 0, 0) > 0                  # the last tile of one grid
    rc = L.egr_nullmany_shift_fir(None, _tab(ok + [(0, 0, 0, -1, 0, 10)]), 5, None, 2, 64, None, None, 0, None, None)
    assert rc != 0 and "row 4: a length below 1" in native.last_error()
    rc = L.egr_nullmany_shift_fir(None, _tab(ok), 4, None, 2, 64, None, None, 0, None, None)
    assert rc != 0 and "null pointer" in native.last_error()
    fake = ctypes.c_void_p(4096)
    rc = L.egr_nullmany_shift_fir(fake, _tab(ok), 4, fake, 2, 64, fake, ctypes.c_void_p(4100), 1 << 30, None, None)
    assert rc != 0 and "8-byte aligned" in native.last_error()


def test_mix_workspace_sizes_and_refusals(pack):
    from egregora_amd import native
    L = native.lib()
    f = L.egr_nullmany_mix_workspace_bytes
    # (offset a, channels a, stride a, offset b, channels b, stride b, n, output offset)
    ok = [(0, 2, 5000, 10000, 2, 6000, 5000, 0), (30000, 1, 4097, 40000, 1, 4097, 4097, 10000), (50000, 3, 10, 50100, 3, 10, 1, 14097)]
    size = f(_tab(ok), 3)
    chunks = 2 + 2 + 1
    assert 3 * 8 * 8 + 3 * 16 + chunks * 64 <= size <= 3 * 8 * 8 + 3 * 16 + chunks * 64 + 3 * 256
    refused = {
        "empty side": ((ok + [(0, 1, 10, 0, 1, 10, 0, 0)], 4), "pair 3: a length below 1"),
        "channel mismatch": ((ok[:1] + [(0, 2, 10, 0, 1, 10, 10, 0)], 2), "pair 1: operands could not be broadcast together"),
        "stride below n": (([(0, 1, 9, 0, 1, 10, 10, 0)] + ok, 4), "pair 0: channels outside 1 .. 65535 or a row stride below n"),
        "negative output offset": ((ok + [(0, 1, 10, 0, 1, 10, 10, -2)], 4), "pair 3: an offset"),
        "chunk total": ((ok + [(0, 1, 4096 * GRID_256, 0, 1, 4096 * GRID_256, 4096 * GRID_256, 0)], 4), "pair 3: the running total"),
        "no pairs": ((ok, 0), "no pairs"),
    }
    for why, (args, msg) in refused.items():
        assert f(_tab(args[0]), *args[1:]) == 0, why
        assert msg in native.last_error(), (why, native.last_error())
    assert f(_tab([(0, 1, 4096 * GRID_256, 0, 1, 4096 * GRID_256, 4096 * GRID_256, 0)]), 1) > 0
    rc = L.egr_nullmany_mix(None, None, _tab(ok[:1] + [(0, 2, 10, 0, 1, 10, 10, 0)]), None, 2, None, None, None, None, None, 0, None, None)
    assert rc != 0 and "pair 1: operands could not be broadcast together" in native.last_error()
    rc = L.egr_nullmany_mix(None, None, _tab(ok), None, 3, None, None, None, None, None, 0, None, None)
    assert rc != 0 and "null pointer" in native.last_error()
    fake = ctypes.c_void_p(4096)
    prm = (ctypes.c_float * 12)(*([1.0, 1.0, -1.0, 0.0] * 3))
    rc = L.egr_nullmany_mix(fake, fake, _tab(ok), prm, 3, fake, fake, None, fake, ctypes.c_void_p(4104), 1 << 30, None, None)
    assert rc != 0 and "16-byte aligned" in native.last_error()
    prm[6] = 0.5                                                               # a sign that is neither 1 nor -1
    rc = L.egr_nullmany_mix(fake, fake, _tab(ok), prm, 3, fake, fake, None, fake, fake, 1 << 30, None, None)
    assert rc != 0 and "pair 1: sign" in native.last_error()
    prm[6], prm[11] = -1.0, 1.0                                                # a least-squares factor in the sums-only mode
    rc = L.egr_nullmany_mix(fake, fake, _tab(ok), prm, 3, None, None, None, fake, fake, 1 << 30, None, None)
    assert rc != 0 and "pair 2: a least-squares factor" in native.last_error()


def test_grouping_and_wave_planner(pack):
    from egregora_amd import device_ops, eval_many, null_many
    # the single rule `while n < na + nb` on the common length: a total that IS a power of two stays at that length
    for nc, n in ((1, 2), (128, 256), (129, 512), (255, 512), (256, 512), (257, 1024), (4096, 8192), (4097, 16384)):
        assert null_many.transform_length(nc) == n == device_ops.xcorr_transform_length(nc, nc), nc
    assert device_ops.xcorr_transform_length(300, 212) == 512 and device_ops.xcorr_transform_length(300, 213) == 1024
    groups = null_many.transform_groups([256, 300, 257, 129, 9000, 512])
    assert list(groups.items()) == [(512, [0, 3]), (1024, [1, 2, 5]), (32768, [4])]
    lv = null_many.level_groups([(8000, 1), (8000, 2), (16000, 1), (8000, 1), (8000, 2)])
    assert list(lv.items()) == [((8000, 1), [0, 3]), ((8000, 2), [1, 4]), ((16000, 1), [2])]
    assert null_many.max_shift_samples(8000, 20) == 160 and null_many.max_shift_samples(44100, 200) == int(44100 * 0.2)
    # a pair's own need bounds its share of every call from above: samples, four outputs, 24 n bytes of the transform group, metrics
    b = null_many.pair_bytes(2, 6000, 1, 5000, 512, 64)
    assert b >= 4 * (2 * 6000 + 5000) + 16 * 6000 + 24 * 16384
    assert b == null_many.pair_bytes(2, 6000, 1, 5000, 512, 64) and null_many.pair_bytes(2, 6000, 1, 5001, 512, 64) > b
    assert null_many.pair_work(6000, 5000, 512, 64) == max(16384 // 256, 1 + (6000 - 512) // 64)
    x = [(torch.zeros(1, 3000), torch.zeros(1, 3000))] * 5
    one = null_many.pair_bytes(1, 3000, 1, 3000)
    assert null_many._waves(x, max_bytes=2 * one) == [[0, 1], [2, 3], [4]] and null_many._waves(x, max_bytes=1 << 40) == [[0, 1, 2, 3, 4]]
    assert null_many._waves(x) == [[0, 1, 2, 3, 4]] and eval_many.DEFAULT_WAVE_GB == 4.0
    assert null_many._MAX_PLANS >= 4 and null_many._PLANS is not __import__("egregora_amd.fatllama_engine", fromlist=["_PLANS"])._PLANS
    assert null_many._rates(8000, 2, "t") == [(8000, 8000)] * 2 and null_many._rates([(8000, 16000), 44100], 2, "t") == [(8000, 16000), (44100, 44100)]
    with pytest.raises(ValueError, match="2 pairs against 1"):
        null_many._rates([8000], 2, "t")


def test_host_finish_is_the_single_path_s(pack):
    """device_ops.xcorr_delay / integrated_lufs, apply_delay and null_stage end in the functions the many-pair path calls."""
    import inspect
    import numpy as np
    from egregora_amd import device_ops, egregora_null_test_suite as ns, null_many
    assert "xcorr_refine(" in inspect.getsource(device_ops.xcorr_delay) and "lufs_gate(" in inspect.getsource(device_ops.integrated_lufs)
    assert "delay_rule(" in inspect.getsource(ns.apply_delay) and "corr_finish(" in inspect.getsource(ns.null_stage)
    src = inspect.getsource(null_many)
    for name in ("xcorr_refine(", "lufs_gate(", "delay_rule(", "corr_finish(", "lsd_finish("):
        assert name in src, name
    o = torch.tensor([0.0, 0.25, 1.0, 0.5])
    o[:1].view(torch.int32)[0] = -7
    lag = device_ops.xcorr_refine(o, 512)
    assert lag == -7 + (0.25 - 0.5) / (2 * (0.25 - 2.0 + 0.5))
    o[:1].view(torch.int32)[0] = -256                                          # the index at the edge: no refinement
    assert device_ops.xcorr_refine(o, 512) == -256.0
    # apply_delay's rule: no delay, integer only, both signs with a fraction, everything shifted out
    assert ns.delay_rule(5e-7, 64, 100) == (0, None) and ns.delay_rule(-3.0000004, 64, 100) == (-3, None)
    s, h = ns.delay_rule(2.25, 64, 100)
    assert s == 2 and h.size == 64 and np.array_equal(h, ns.frac_delay_taps(0.25, 64))
    s, h = ns.delay_rule(-2.25, 8, 100)
    assert s == -2 and h.size == 16 and np.array_equal(h, ns.frac_delay_taps(0.25, 8))
    assert ns.delay_rule(100.0, 64, 100) == (100, None) and ns.delay_rule(-250.0, 64, 100) == (-100, None)
    ms = np.array([1e-3, 2e-3, 1e-9, 4e-3])
    assert device_ops.lufs_gate(ms) == float(-0.691 + 10.0 * np.log10(np.mean((ms + 1e-20)[[0, 1, 3]])))
    assert ns.corr_finish(0.0, 0.0, 2.0, 4.0, 1.0, 10, True) == 1.0 and ns.corr_finish(0.0, 0.0, 2.0, 4.0, 1.0, 10, False) == -1.0


def test_empty_lists_bad_items_and_list_rules_need_no_device(pack):
    from egregora_amd import egregora_null_test_batch as nb, egregora_null_test_suite as ns, null_many
    stats = {}
    for call in (null_many.delays_many, null_many.align_many, null_many.gain_match_many, null_many.null_test_many, null_many.full_many):
        assert call([], 8000, stats=stats) == [] and all(stats[k] == 0 for k in null_many.STAT_KEYS)
    assert null_many.shift_fir_many([], [], 64) == []
    x = torch.zeros(2, 100)
    with pytest.raises(ValueError, match="item 1"):
        null_many.full_many([(x, x), (x, torch.zeros(2, 0))], 8000)
    with pytest.raises(ValueError, match="item 0"):
        null_many.delays_many([(torch.zeros(1, 2, 100), x)], 8000)
    with pytest.raises(ValueError, match="item 1: sample rate 0"):
        null_many.align_many([(x, x), (x, x)], [8000, 0])
    with pytest.raises(ValueError, match="item 0: Sample rate mismatch after alignment stage"):
        null_many.null_test_many([(x, x)], [(8000, 16000)])
    with pytest.raises(ValueError, match="one delay and one output length per clip"):
        null_many.shift_fir_many([x, x], [0.0], 64)
    a = {"waveform": torch.zeros(3, 2, 50), "sample_rate": 8000}
    one = {"waveform": torch.zeros(1, 2, 50), "sample_rate": 8000}
    refs, procs = nb._paired([a, one], [one, a], "t")                        # [B,C,T] counts as B clips
    assert len(refs) == len(procs) == 4 and all(c["samples"].shape == (2, 50) for c in refs + procs)
    with pytest.raises(ValueError, match="3 reference clips against 1 processed"):
        nb.Null_Test_Full_Batch().execute([a], [one])
    with pytest.raises(ValueError, match="3 reference clips against 1 processed"):
        nb.Audio_Null_Test_Batch().execute([a], [one])
    with pytest.raises(ValueError, match="Sample rate mismatch after alignment stage"):
        nb.Audio_Null_Test_Batch().execute([one], [dict(one, sample_rate=16000)])
    assert nb.Audio_Null_Test_Batch().execute([], []) == ([], []) and nb.Null_Test_Full_Batch().execute([], []) == ([], [], [], [], [])
    assert nb.Audio_Null_Test_Batch.INPUT_IS_LIST is True and nb.Audio_Null_Test_Batch.OUTPUT_IS_LIST == (True, True)
    assert nb.Null_Test_Full_Batch.INPUT_IS_LIST is True and nb.Null_Test_Full_Batch.OUTPUT_IS_LIST == (True,) * 5
    assert nb.Audio_Null_Test_Batch.INPUT_TYPES() == ns.Audio_Null_Test.INPUT_TYPES()
    full, single = nb.Null_Test_Full_Batch.INPUT_TYPES(), ns.Null_Test_Full.INPUT_TYPES()
    assert full["required"] == single["required"]
    assert list(full["optional"]) == [k for k in single["optional"] if not k.startswith("draw_")] and len(single["optional"]) - len(full["optional"]) == 3
    assert all(full["optional"][k] == single["optional"][k] for k in full["optional"])
    assert nb.Null_Test_Full_Batch.RETURN_TYPES == ("AUDIO", "AUDIO", "FLOAT", "FLOAT", "DICT")
    assert nb.Null_Test_Full_Batch.RETURN_NAMES == ns.Null_Test_Full.RETURN_NAMES[:5] and "IMAGE" not in nb.Null_Test_Full_Batch.RETURN_TYPES
    assert nb.Audio_Null_Test_Batch.RETURN_TYPES == ns.Audio_Null_Test.RETURN_TYPES


def test_batch_node_registration_is_opt_in():
    base = _keys_in_child()
    assert not set(KEYS) & set(base["keys"]) and base["keys"] == base["display_keys"]
    assert {"Audio Align (XCorr)", "Audio Gain Match", "Audio Null Test", "Null Test (Full)"} <= set(base["keys"])
    assert _keys_in_child(EGREGORA_NULLTEST_BATCH_NODES="0")["keys"] == base["keys"]
    assert _keys_in_child(EGREGORA_EVAL_BATCH_NODES="1")["keys"] != base["keys"] and not set(KEYS) & set(_keys_in_child(EGREGORA_EVAL_BATCH_NODES="1")["keys"])
    on = _keys_in_child(EGREGORA_NULLTEST_BATCH_NODES="1")
    assert sorted(set(on["keys"]) - set(base["keys"])) == KEYS and on["keys"] == on["display_keys"]


def test_index_header_under_host_sanitizers(tmp_path):
    """csrc/egr_null_index.h compiled for the host with -fsanitize=address,undefined and walked over ragged tables that hold the tile,
    chunk and group edges (tools/nullmany_host_check.cpp)."""
    rocm_clang = Path(os.environ.get("ROCM_PATH", "/opt/rocm")) / "llvm" / "bin" / "clang++"
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or (str(rocm_clang) if rocm_clang.exists() else None)
    assert cxx is not None, "no host C++ compiler, not even ROCm's clang++: the sanitizer walk cannot run"
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    exe = tmp_path / "nullmany_host_check"
    r = subprocess.run([cxx] + flags + [str(ROOT / "tools" / "nullmany_host_check.cpp"), "-o", str(exe)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "all tables pass" in r.stdout and "refusals ok" in r.stdout and "thousand " in r.stdout and \
        "transform lengths ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


def test_null_batch_pairs_files_by_relative_path(pack, tmp_path):
    from egregora_amd import null_batch
    ref, proc = tmp_path / "ref", tmp_path / "proc"
    for d, names in ((ref, ["a.wav", "sub/b.flac", "only_ref.wav"]), (proc, ["a.flac", "sub/b.wav", "sub/only_proc.wav"])):
        for n in names:
            (d / n).parent.mkdir(parents=True, exist_ok=True)
            (d / n).write_bytes(b"")
    pairs, alone = null_batch.pair_up(ref, proc)
    assert [k for k, _, _ in pairs] == ["a", "sub/b"] and len(alone) == 2
    args = null_batch.parser().parse_args(["--ref-dir", "R", "--proc-dir", "P"])
    assert (args.align_max_shift_ms, args.fir_len, args.match_mode, args.n_fft, args.hop) == (200, 64, "LUFS-I", 2048, 512)
    assert args.fractional and not args.least_squares_scale and args.compute_lsd and not args.compute_hf_residual
    assert (args.out, args.write_null, args.write_matched) == (None, None, None)
    assert null_batch.parser().parse_args(["--ref-dir", "R", "--proc-dir", "P", "--no-fractional", "--least-squares-scale"]).fractional is False
