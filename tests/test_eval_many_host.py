"""Many-pair metrics and many-clip loudness, everything that needs no device: the exported symbols, the host-only
workspace entry points and their refusals (each names the pair or clip in egr_last_error), the wave planner, the opt-in registration
of the two batch nodes, the list rules of the nodes, and a host walk of csrc/egr_eval_index.h under the address and undefined-behaviour
sanitizers (a stand-alone program)."""
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
KEYS = ["Loudness Meter (BS1770) (batch)", "Metrics (LSD + SI-SDR) (batch)"]
SYMBOLS = ["egr_loudness_tracks", "egr_loudness_tracks_workspace_bytes", "egr_metrics_pairs", "egr_metrics_pairs_frames",
           "egr_metrics_pairs_workspace_bytes"]
GRID_256, MAX_PAIRS = (2 ** 32 - 1) // 256, (2 ** 32 - 1) // 1024         # HIP launches no grid of 2^32 work-items or more

_DUMP = """
import json, sys
sys.path.insert(0, %r)
from packload import load_pack
p = load_pack()
print("DUMP" + json.dumps({"keys": sorted(p.NODE_CLASS_MAPPINGS), "display_keys": sorted(p.NODE_DISPLAY_NAME_MAPPINGS)}))
"""
_SWITCHES = ("EGREGORA_EVAL_NODES", "EGREGORA_EVAL_BATCH_NODES", "EGREGORA_ENHANCE_NODES", "EGREGORA_ENHANCE_BATCH_NODES")


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
    assert sorted(s for s in declared if s.startswith(("egr_metrics_", "egr_loudness_tracks"))) == SYMBOLS
    lib = ctypes.CDLL(str(native.LIB_PATH))
    for s in SYMBOLS + ["egr_kweight_chunking"]:
        assert hasattr(lib, s) and s in native.SIGNATURES, s
    assert native.lib().egr_abi_version() == native.ABI_VERSION == 5


def test_metrics_workspace_sizes_and_refusals(pack):
    from egregora_amd import device_ops, native
    L = native.lib()
    ok = [(0, 1, 5000, 5000, 2, 6000, 5000), (17000, 3, 700, 20000, 1, 600, 600)]
    sizes = {f: L.egr_metrics_pairs_workspace_bytes(_tab(ok), 2, 512, 64, f) for f in (1, 2, 3)}
    frames = (1 + (5000 - 512) // 64) + (1 + (600 - 512) // 64)
    chunks = 2 + 1
    table = 2 * 12 * 8
    assert sizes[1] >= table + 4 * frames and sizes[2] >= table + 16 * chunks and sizes[3] >= table + 4 * frames + 16 * chunks
    assert max(sizes.values()) <= table + 4 * frames + 16 * chunks + 3 * 256                 # the three sections, each padded to 256 bytes
    assert device_ops.metrics_pairs_workspace_bytes(ok, 512, 64, 3) == sizes[3]
    assert L.egr_metrics_pairs_workspace_bytes(_tab(ok), 2, 2176, 544, 1) > 0              # 2^7 * 17: the generic radix stage
    assert L.egr_metrics_pairs_workspace_bytes(_tab(ok), 2, 8192, 2048, 1) > 0
    big = 2 ** 62
    # (rows, n_pairs, n_fft, hop, flags) -> what egr_last_error must say
    refused = {
        "n = 0": ((ok + [(0, 1, 10, 0, 1, 10, 0)], 3, 512, 64, 3), "pair 2: n < 1"),
        "n < 0": (([(0, 1, 10, 0, 1, 10, -4)] + ok, 3, 512, 64, 3), "pair 0: n < 1"),
        "no channels": ((ok[:1] + [(0, 0, 10, 0, 1, 10, 10)], 2, 512, 64, 3), "pair 1: channels"),
        "stride below n": ((ok[:1] + [(0, 1, 9, 0, 1, 10, 10)], 2, 512, 64, 3), "pair 1: channels outside 1 .. 65535 or a row stride below n"),
        "negative offset": ((ok + [(0, 1, 10, -8, 1, 10, 10)], 3, 512, 64, 3), "pair 2: an offset"),
        "offset past the index type": ((ok + [(big, 1, 10, 0, 1, 10, 10)], 3, 512, 64, 3), "pair 2: an offset"),
        "frame total": (([(0, 1, 2 ** 31 + 600, 0, 1, 2 ** 31 + 600, 2 ** 31 + 600)], 1, 512, 1, 1), "pair 0: the running total"),
        "frame total of two": (([(0, 1, 2 ** 23 + 600, 0, 1, 2 ** 23 + 600, 2 ** 23 + 600)] * 2, 2, 512, 1, 1), "pair 1: the running total"),
        "chunk total": (([(0, 1, 4096 * (GRID_256 + 1), 0, 1, 4096 * (GRID_256 + 1), 4096 * (GRID_256 + 1))], 1, 8192, 4096, 2), "pair 0: the running total"),
        "too many pairs": ((ok, MAX_PAIRS + 1, 512, 64, 3), f"n_pairs={MAX_PAIRS + 1}"),
        "odd n_fft": ((ok, 2, 511, 64, 3), "n_fft=511"),
        "n_fft above 8192": ((ok, 2, 8320, 64, 3), "n_fft=8320"),
        "prime factor 131": ((ok, 2, 2 * 131, 64, 3), "prime factor"),
        "hop = 0": ((ok, 2, 512, 0, 3), "hop=0"),
        "no pairs": ((ok, 0, 512, 64, 3), "no pairs"),
        "flags = 0": ((ok, 2, 512, 64, 0), "flags=0"),
        "flags = 4": ((ok, 2, 512, 64, 4), "flags=4"),
    }
    for why, ((rows, n, n_fft, hop, flags), msg) in refused.items():
        assert L.egr_metrics_pairs_workspace_bytes(_tab(rows), n, n_fft, hop, flags) == 0, why
        assert msg in native.last_error(), (why, native.last_error())
    assert L.egr_metrics_pairs_workspace_bytes(None, 2, 512, 64, 3) == 0 and "no pairs" in native.last_error()
    # the call itself refuses the same tables before it touches a pointer (all of them null here) or the device
    rc = L.egr_metrics_pairs(None, None, _tab(ok + [(0, 1, 10, 0, 1, 10, 0)]), 3, 512, 64, 3, None, None, None, None, 0, None, None)
    assert rc != 0 and "pair 2: n < 1" in native.last_error()
    rc = L.egr_metrics_pairs(None, None, _tab(ok), 2, 512, 64, 3, None, None, None, None, 0, None, None)
    assert rc != 0 and "null pointer" in native.last_error()
    # the edges of one grid of 256-thread workgroups: 2^24 - 1 frames, 2^24 - 1 chunks (the planner refuses too many pairs before it
    # reads the table, so that refusal above needs no table of 2^22 rows)
    assert GRID_256 == 2 ** 24 - 1 and MAX_PAIRS == 2 ** 22 - 1
    n_last = 512 + GRID_256 - 1
    assert L.egr_metrics_pairs_frames(_tab([(0, 1, n_last, 0, 1, n_last, n_last)]), 1, 512, 1) == GRID_256
    assert L.egr_metrics_pairs_workspace_bytes(_tab([(0, 1, n_last, 0, 1, n_last, n_last)]), 1, 512, 1, 1) > 0
    assert L.egr_metrics_pairs_workspace_bytes(_tab([(0, 1, n_last + 1, 0, 1, n_last + 1, n_last + 1)]), 1, 512, 1, 1) == 0
    assert "pair 0: the running total" in native.last_error() and L.egr_metrics_pairs_frames(_tab([(0, 1, n_last + 1, 0, 1, n_last + 1, n_last + 1)]), 1, 512, 1) == 0
    n_last = 4096 * GRID_256
    assert L.egr_metrics_pairs_workspace_bytes(_tab([(0, 1, n_last, 0, 1, n_last, n_last)]), 1, 8192, 4096, 2) > 0
    assert L.egr_metrics_pairs_workspace_bytes(_tab([(0, 1, n_last + 1, 0, 1, n_last + 1, n_last + 1)]), 1, 8192, 4096, 2) == 0
    assert L.egr_metrics_pairs_frames(_tab(ok), 2, 512, 64) == frames
    # a workspace that is not 16-byte aligned is refused before anything is copied (no pointer here is ever read)
    fake = ctypes.c_void_p(4096)
    rc = L.egr_metrics_pairs(fake, fake, _tab(ok), 2, 512, 64, 3, fake, fake, None, ctypes.c_void_p(4096 + 8), 1 << 30, None, None)
    assert rc != 0 and "16-byte aligned" in native.last_error()
    with pytest.raises(RuntimeError, match="`device` is required"):
        device_ops.metrics_pairs(4096, 4096, ok, 512, 64, 3)


def test_loudness_workspace_sizes_and_refusals(pack):
    import math
    import numpy as np
    from egregora_amd import loudness, native
    L = native.lib()
    k = float(np.float32(math.exp(-2 * math.pi * (60.0 / 4000.0))))
    ok = [(0, 9000), (18000, 1), (18002, 3200)]
    size = L.egr_loudness_tracks_workspace_bytes(_tab(ok), 3, 2, k, 3200, 800, 24000, 8000, 4)
    mono = 4 * (9000 + 1 + 3200)
    assert 3 * 8 * 8 + mono <= size <= 3 * 8 * 8 + mono + 2 * 256
    assert loudness.many_workspace_bytes([9000, 1, 3200], 2, 8000, True, 4) == size
    assert L.egr_loudness_tracks_workspace_bytes(_tab(ok), 3, 5, k, 3200, 800, 0, 0, 0) == size            # the workspace holds mono only
    refused = {
        "n = 0": ((ok + [(30000, 0)], 4, 2, k, 3200, 800, 24000, 8000, 4), "clip 3: n < 1"),
        "negative offset": (([(-2, 100)] + ok, 4, 2, k, 3200, 800, 24000, 8000, 4), "clip 0: an offset"),
        "tile total": (([(0, 2 ** 33)] + ok, 4, 1, k, 3200, 800, 24000, 8000, 64), "clip 0: the running total"),
        "no clips": ((ok, 0, 2, k, 3200, 800, 24000, 8000, 4), "no clips"),
        "no channels": ((ok, 3, 0, k, 3200, 800, 24000, 8000, 4), "channels=0"),
        "k = 1": ((ok, 3, 2, 1.0, 3200, 800, 24000, 8000, 4), "k=1"),
        "block = 0": ((ok, 3, 2, k, 0, 800, 24000, 8000, 4), "bad block family"),
        "hop_b = 0": ((ok, 3, 2, k, 3200, 800, 24000, 0, 4), "bad block family"),
        "up = 65": ((ok, 3, 2, k, 3200, 800, 24000, 8000, 65), "bad block family"),
    }
    for why, (args, msg) in refused.items():
        assert L.egr_loudness_tracks_workspace_bytes(_tab(args[0]), *args[1:]) == 0, why
        assert msg in native.last_error(), (why, native.last_error())
    rc = L.egr_loudness_tracks(None, _tab(ok + [(30000, 0)]), 4, 2, 1 - k, k, 3200, 800, 24000, 8000, 4, None, 0, None, None, 0, None, None)
    assert rc != 0 and "clip 3: n < 1" in native.last_error()
    # the edges of one grid of 256-thread workgroups: 2^24 - 1 peak tiles, 2^24 - 1 blocks
    n_last = 256 * GRID_256 // 8
    assert L.egr_loudness_tracks_workspace_bytes(_tab([(0, n_last)]), 1, 1, k, 3200, 800, 24000, 8000, 8) > 0
    assert L.egr_loudness_tracks_workspace_bytes(_tab([(0, n_last + 1)]), 1, 1, k, 3200, 800, 24000, 8000, 8) == 0
    assert "clip 0: the running total" in native.last_error()
    assert L.egr_loudness_tracks_workspace_bytes(_tab([(0, 10 + GRID_256 - 1)]), 1, 1, k, 10, 1, 0, 0, 0) > 0
    assert L.egr_loudness_tracks_workspace_bytes(_tab([(0, 10 + GRID_256)]), 1, 1, k, 10, 1, 0, 0, 0) == 0
    fake = ctypes.c_void_p(4096)
    rc = L.egr_loudness_tracks(fake, _tab(ok), 3, 2, 1 - k, k, 3200, 800, 24000, 8000, 4, fake, 8, fake, ctypes.c_void_p(4100), 1 << 30, None, None)
    assert rc != 0 and "8-byte aligned" in native.last_error()
    # the chunking of the K-weighting kernels is the library's own statement
    from egregora_amd import loudness as ld
    Lc, W = ld.chunking(8000)
    assert W == max(64, math.ceil(26.0 / -math.log(k))) and Lc == (W + 2) // 3 and ld.chunking(16000) != (Lc, W)
    assert L.egr_kweight_chunking(1.0, ctypes.byref(ctypes.c_int()), ctypes.byref(ctypes.c_int())) != 0


def test_wave_planner(pack):
    from egregora_amd import eval_many
    need = [400, 300, 500, 2000, 100, 100, 100, 900]
    waves = eval_many.plan_waves(need, 1000)
    assert waves == [[0, 1], [2], [3], [4, 5, 6], [7]]                  # input order; item 3 is over the budget by itself: its own wave
    for w in waves:
        assert sum(need[i] for i in w) <= 1000 or len(w) == 1
    assert sorted(i for w in waves for i in w) == list(range(len(need)))
    assert eval_many.plan_waves(need, 1 << 40) == [list(range(len(need)))]
    assert eval_many.plan_waves([], 1000) == [] and eval_many.DEFAULT_WAVE_GB == 4.0
    # a wave also closes before its frames, chunks, blocks or tiles pass what one grid holds, or its items the pair cap
    assert eval_many.plan_waves([1] * 6, 1000, item_work=[5, 5, 5, 30, 1, 9], max_work=10) == [[0, 1], [2], [3], [4, 5]]
    assert eval_many.plan_waves([1] * 5, 1000, max_items=2) == [[0, 1], [2, 3], [4]]
    from egregora_amd import device_ops as dops
    assert dops.MAX_GRID_256 == GRID_256 and dops.MAX_PAIRS == MAX_PAIRS
    assert eval_many.pair_work(5000, 6000, 512, 64) == 1 + (5000 - 512) // 64 and eval_many.pair_work(9000, 9000, 8192, 4096) == 3
    assert eval_many.clip_work(32000, 8000, 8) == 1000 and eval_many.clip_work(32000, 8000, 0) == 1 + (32000 - 3200) // 800
    old = os.environ.get("EGREGORA_EVAL_WAVE_GB")
    os.environ["EGREGORA_EVAL_WAVE_GB"] = repr(1000 / (1 << 30))
    try:
        assert eval_many.plan_waves(need) == waves and eval_many.wave_budget() == 1000
    finally:
        if old is None:
            del os.environ["EGREGORA_EVAL_WAVE_GB"]
        else:
            os.environ["EGREGORA_EVAL_WAVE_GB"] = old
    # a pair's own need: its workspace from the entry point plus both sides' samples
    from egregora_amd import device_ops
    b = eval_many.pair_bytes(2, 6000, 1, 5000, 512, 64, 3)
    assert b == device_ops.metrics_pairs_workspace_bytes([(0, 2, 6000, 12000, 1, 5000, 5000)], 512, 64, 3) + 4 * (12000 + 5000)


def test_empty_lists_bad_items_and_list_rules_need_no_device(pack):
    from egregora_amd import egregora_audio_eval_batch as eb, eval_many
    stats = {}
    assert eval_many.metrics_many([], stats=stats) == [] and stats["waves"] == 0 and stats["library_calls"] == 0 and stats["launches"] == 0
    assert eval_many.loudness_many([], stats=stats) == [] and stats["waves"] == 0
    x = torch.zeros(2, 100)
    assert eval_many.metrics_many([(x, x), (x[0], x)], compute_lsd=False, compute_si_sdr=False) == [{}, {}]
    with pytest.raises(ValueError, match="item 1"):
        eval_many.metrics_many([(x, x), (x, torch.zeros(2, 0))])
    with pytest.raises(ValueError, match="item 0"):
        eval_many.metrics_many([(torch.zeros(1, 2, 100), x)])
    with pytest.raises(ValueError, match="item 1"):
        eval_many.loudness_many([(x, 8000), (torch.zeros(0), 8000)])
    with pytest.raises(RuntimeError, match="n_fft=511"):                     # the library's host arithmetic, before any device is asked for
        eval_many.metrics_many([(x, x)], n_fft=511)
    a = {"waveform": torch.zeros(3, 2, 50), "sample_rate": 8000}
    assert [c["samples"].shape for c in eb.clips_of(a)] == [(2, 50)] * 3            # [B,C,T] counts as B clips
    assert [c["samples"].shape for c in eb.clips_of({"sr": 16000, "samples": torch.zeros(70, 2).numpy()})] == [(2, 70)]
    node = eb.Metrics_LSD_SISDR_Batch()
    with pytest.raises(ValueError, match="3 reference clips against 1 processed"):
        node.execute([a], [{"waveform": torch.zeros(1, 2, 50), "sample_rate": 8000}], [512], [64], [True], [True])
    for cls in (eb.Metrics_LSD_SISDR_Batch, eb.Loudness_Meter_1770_Batch):
        assert cls.INPUT_IS_LIST is True and cls.OUTPUT_IS_LIST == (True,)
    from egregora_amd import egregora_audio_eval_loudness as el, egregora_audio_eval_pack as ep
    assert eb.Metrics_LSD_SISDR_Batch.INPUT_TYPES() == ep.Metrics_LSD_SISDR.INPUT_TYPES()
    assert eb.Loudness_Meter_1770_Batch.INPUT_TYPES() == el.Loudness_Meter_1770.INPUT_TYPES()


def test_host_finish_is_the_single_path_s(pack):
    """device_ops.lsd / si_sdr and loudness.measure end in the functions metrics_many / loudness_many call."""
    import inspect
    from egregora_amd import device_ops, eval_many, loudness
    assert "lsd_finish(" in inspect.getsource(device_ops.lsd) and "si_sdr_finish(" in inspect.getsource(device_ops.si_sdr)
    assert "measure_finish(" in inspect.getsource(loudness.measure)
    row = [12.5, 1.0, 3.0, 8.0, 0.0, 0.0, 4.0, 1e-4]
    got = eval_many.metrics_finish(row, True, True)
    mean, p95 = device_ops.lsd_finish(12.5, 1.0, 3.0, 8)
    assert list(got) == ["lsd_mean_db", "lsd_p95_db", "si_sdr_db"]
    assert got == {"lsd_mean_db": mean, "lsd_p95_db": p95, "si_sdr_db": device_ops.si_sdr_finish(4.0, 1e-4)}
    assert device_ops.lsd_ranks(8) == (0.95 * 7, 6, 7) and device_ops.lsd_ranks(1)[1:] == (0, 0) and device_ops.lsd_ranks(21)[1:] == (19, 20)


def test_batch_node_registration_is_opt_in():
    base = _keys_in_child()
    assert not set(KEYS) & set(base["keys"]) and not set(KEYS) & set(base["display_keys"])
    ev = _keys_in_child(EGREGORA_EVAL_NODES="1")
    assert not set(KEYS) & set(ev["keys"]) and "Loudness Meter (BS1770)" in ev["keys"]
    assert _keys_in_child(EGREGORA_EVAL_BATCH_NODES="0")["keys"] == base["keys"]
    on = _keys_in_child(EGREGORA_EVAL_BATCH_NODES="1")
    assert sorted(set(on["keys"]) - set(base["keys"])) == KEYS and on["keys"] == on["display_keys"]


def test_index_header_under_host_sanitizers(tmp_path):
    """csrc/egr_eval_index.h compiled for the host with -fsanitize=address,undefined and walked over ragged tables that hold the edge
    lengths of the frame rule, the chunking and the thread chunks (tools/evalmany_host_check.cpp)."""
    rocm_clang = Path(os.environ.get("ROCM_PATH", "/opt/rocm")) / "llvm" / "bin" / "clang++"
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or (str(rocm_clang) if rocm_clang.exists() else None)
    assert cxx is not None, "no host C++ compiler, not even ROCm's clang++: the sanitizer walk cannot run"
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    exe = tmp_path / "evalmany_host_check"
    r = subprocess.run([cxx] + flags + [str(ROOT / "tools" / "evalmany_host_check.cpp"), "-o", str(exe)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "all tables pass" in r.stdout and "refusals ok" in r.stdout and "thousand " in r.stdout, \
        (r.stdout[-2000:], r.stderr[-2000:])


def test_eval_batch_pairs_files_by_relative_path(pack, tmp_path):
    from egregora_amd import eval_batch
    ref, proc = tmp_path / "ref", tmp_path / "proc"
    for d, names in ((ref, ["a.wav", "sub/b.flac", "only_ref.wav", "notes.txt"]), (proc, ["a.flac", "sub/b.wav", "sub/only_proc.wav"])):
        for n in names:
            (d / n).parent.mkdir(parents=True, exist_ok=True)
            (d / n).write_bytes(b"")
    pairs, alone = eval_batch.pair_up(ref, proc)
    assert [(k, str(r.relative_to(ref)), str(p.relative_to(proc))) for k, r, p in pairs] == [("a", "a.wav", "a.flac"), ("sub/b", "sub/b.flac", "sub/b.wav")]
    assert alone == sorted([str(ref / "only_ref.wav"), str(proc / "sub" / "only_proc.wav")])
    args = eval_batch.parser().parse_args(["--ref-dir", "R", "--proc-dir", "P"])
    assert (args.n_fft, args.hop, args.loudness, args.out) == (2048, 512, False, None)
