"""The windowed-sinc resampler without a GPU (SPEC.md 4f): the host design against the float64 yardstick of tests/sinc_refs.py, a
numpy model of the kernels' walk (the rules of csrc/egr_sinc_index.h transcribed), the index header under the host sanitizers, the
refusals, and the node surface."""
import json
import os
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import sinc_refs as R

ROOT = Path(__file__).resolve().parent.parent
TILE, LDS_FLOATS = 256, 4096                       # SINC_TILE, SINC_LDS_FLOATS (csrc/egr_sinc_index.h)
WINDOWS = [("sinc_interp_hann", None), ("sinc_interp_kaiser", 5.0), ("sinc_interp_kaiser", 14.769)]
IDS = [f"{c[0][0]}to{c[0][1]}" for c in R.CASES]


# ---------------------------------------------------------------- design
@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_design_is_the_float32_cast_of_the_definition_inside_the_run(pack, case):
    from egregora_amd import resample
    (src, dst, lpw, rolloff), want = case
    for method, beta in WINDOWS:
        table, first_tap, (o, n, width, run) = resample.design_sinc(src, dst, lpw, rolloff, method, beta)
        K, tu, geo = R.kernel_f64(src, dst, lpw, rolloff, method, beta)
        assert (o, n, width) == want == geo
        L = 2 * width + o
        assert table.dtype == np.float32 and table.shape == (run, n) and table.flags["C_CONTIGUOUS"]
        assert first_tap.dtype == np.int32 and first_tap.shape == (n,) and first_tap.min() >= 0 and int(first_tap.max()) + run <= L
        inside = (tu.abs() < lpw).numpy()
        counts = inside.sum(axis=1)
        assert run == counts.max() <= 2 * width + 2
        assert (np.diff(inside.astype(np.int8), axis=1) != 0).sum(axis=1).max() <= 2          # one contiguous stretch per phase
        full = np.zeros((n, L), dtype=np.float32)
        rows = np.arange(n)
        for s in range(run):
            full[rows, first_tap + s] = table[s]
        K32 = K.to(torch.float32).numpy()
        assert np.array_equal(full.view(np.uint32)[inside], K32.view(np.uint32)[inside])       # bit for bit at every tap with |t| < lpw
        assert not full[~inside].any()                                                         # nothing else is kept
        if (~inside).any():
            assert np.abs(K.numpy()[~inside]).max() <= 2.0 ** -50                              # every dropped tap is round-off
        assert resample.design_sinc(src, dst, lpw, rolloff, method, beta)[0] is table          # designed once per parameter tuple


def test_kaiser_beta_changes_the_table(pack):
    from egregora_amd import resample
    tabs = [resample.design_sinc(44100, 48000, 64, 0.945, "sinc_interp_kaiser", b)[0] for b in (5.0, 14.769, 20.0)]
    assert tabs[0].shape == tabs[1].shape == tabs[2].shape
    assert not np.array_equal(tabs[0], tabs[1]) and not np.array_equal(tabs[1], tabs[2]) and not np.array_equal(tabs[0], tabs[2])
    default = resample.design_sinc(44100, 48000, 64, 0.945, "sinc_interp_kaiser")[0]
    assert np.array_equal(default, resample.design_sinc(44100, 48000, 64, 0.945, "sinc_interp_kaiser", 14.769656459379492)[0])


# ---------------------------------------------------------------- numpy model of the kernels' walk
def _fma_run(table, p, xs):
    """sinc_sample: the taps in ascending order, one float32 fused multiply-add each (the float32 x float32 product is exact in
    float64; the sum is rounded to float32 once more)."""
    acc = np.zeros(len(p), dtype=np.float32)
    for s in range(table.shape[0]):
        acc = (table[s, p].astype(np.float64) * xs[:, s].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
    return acc


def model(x, table, first_tap, geo, staged):
    """One channel through the single call's grid with egr_sinc_index.h's rules: frame and phase of a flat output, the clamped first
    tap, the tile's span and slots (staged) or the zero-padded global reads (direct)."""
    o, n, width, run = geo
    L, n_in = 2 * width + o, len(x)
    n_out = -(-n_in * n // o)
    y = np.zeros(n_out, dtype=np.float32)
    taps = np.arange(run)
    for m0 in range(0, n_out, TILE):
        m = np.arange(m0, min(n_out, m0 + TILE))
        i, p = m // n, m % n
        f = np.clip(first_tap[p].astype(np.int64), 0, L - run)
        if staged:
            i0, i1 = m0 // n, int(m[-1]) // n
            lo, span = i0 * o - width, (i1 - i0) * o + L
            assert span <= ((n + TILE - 2) // n) * o + L <= LDS_FLOATS
            k = lo + np.arange(span)
            lds = np.where((k >= 0) & (k < n_in), x[np.clip(k, 0, n_in - 1)], np.float32(0))
            slot = (i - i0) * o + f
            assert slot.min() >= 0 and slot.max() + run <= span
            xs = lds[slot[:, None] + taps[None, :]]
        else:
            k = (i * o + f - width)[:, None] + taps[None, :]
            xs = np.where((k >= 0) & (k < n_in), x[np.clip(k, 0, n_in - 1)], np.float32(0))
        y[m] = _fma_run(table, p, xs.astype(np.float32))
    return y


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_index_model_stays_within_the_bound(pack, case):
    from egregora_amd import resample
    (src, dst, lpw, rolloff), (o, n, width) = case
    method, beta = "sinc_interp_kaiser", 14.769
    table, first_tap, geo = resample.design_sinc(src, dst, lpw, rolloff, method, beta)
    staged = resample.sinc_staged(o, n, width)
    assert staged == (((n + TILE - 2) // n) * o + 2 * width + o <= LDS_FLOATS) == ((src, dst) != (8000, 8001))
    lens = R.lengths(o, n)
    assert {1, 2, o + 1} <= set(lens) and any(-(-N * n // o) in (255, 256, 257, 511, 512, 513) for N in lens)
    worst = 0.0
    for N in lens:
        x = R.signal(1, N, 300 + N)
        want, bound = R.resample_f64(x, src, dst, lpw, rolloff, method, beta)
        direct = model(x[0], table, first_tap, geo, False)
        assert direct.shape == want[0].shape == (-(-N * n // o),)
        if staged:
            assert np.array_equal(model(x[0], table, first_tap, geo, True).view(np.uint32), direct.view(np.uint32)), N
        err = np.abs(direct.astype(np.float64) - want[0])
        assert (err <= bound[0]).all(), (N, float(err.max()))
        worst = max(worst, float((err / np.maximum(bound[0], 1e-300)).max()))
    print(f"{src}->{dst}: the model's largest share of the bound {worst:.3f}")


# ---------------------------------------------------------------- host check
def test_index_header_under_host_sanitizers(tmp_path):
    """csrc/egr_sinc_index.h compiled for the host with -fsanitize=address,undefined and walked over tile edges, clips of one sample,
    tracks that start inside a tile, o = 1, n = 1, n above a tile and every refusal (tools/sinc_host_check.cpp)."""
    rocm_clang = Path(os.environ.get("ROCM_PATH", "/opt/rocm")) / "llvm" / "bin" / "clang++"
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or (str(rocm_clang) if rocm_clang.exists() else None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    exe = tmp_path / "sinc_host_check"
    r = subprocess.run([cxx] + flags + [str(ROOT / "tools" / "sinc_host_check.cpp"), "-o", str(exe)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "all walks pass" in r.stdout and "refusals ok" in r.stdout and "thousand tracks" in r.stdout and \
        "n = 1" in r.stdout and "o = 1" in r.stdout and "n above a tile" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


# ---------------------------------------------------------------- refusals
def test_design_refusals(pack, monkeypatch):
    from egregora_amd import resample
    monkeypatch.delenv("EGREGORA_SINC_TABLE_MB", raising=False)
    with pytest.raises(ValueError, match="383999:384000"):                       # 384000 phases x 514 taps: 753 MiB, above the default 256
        resample.design_sinc(383999, 384000, 128, 0.5)
    monkeypatch.setenv("EGREGORA_SINC_TABLE_MB", "1")
    with pytest.raises(ValueError, match="8000:8001.*EGREGORA_SINC_TABLE_MB = 1"):
        resample.design_sinc(8000, 8001, 64, 0.945, "sinc_interp_kaiser", 7.5)
    assert resample.design_sinc(44100, 48000, 64, 0.945, "sinc_interp_kaiser", 7.5)[2] == (147, 160, 68, 136)     # 85 KiB: below 1 MiB
    for src, dst in ((0, 48000), (48000, 0), (-44100, 48000)):
        with pytest.raises(ValueError, match="at least 1"):
            resample.design_sinc(src, dst)
    with pytest.raises(ValueError, match="method"):
        resample.design_sinc(44100, 48000, method="kaiser_window")
    with pytest.raises(ValueError, match="empty"):
        resample.sinc_track_table([0, 5], [5, 0], 147, 160)
    tab, total = resample.sinc_track_table([0, 7], [1, 147], 147, 160)
    assert tab.tolist() == [[0, 1, 0, 2], [7, 147, 2, 160]] and total == 162


def test_c_calls_refuse_from_integers_alone(pack):
    """Every refusal of the index header comes back from both C calls as EGR_ERR_ARG / EGR_ERR_UNSUPPORTED with a text, before any
    pointer is looked at (all pointers are null here) and before anything is launched: this runs without a GPU."""
    from egregora_amd import native
    L = native.lib()
    ARG, UNSUPPORTED = 1, 3                      # EGR_ERR_ARG, EGR_ERR_UNSUPPORTED (include/egregora_amd.h)

    def single(ch=2, n_in=100, o=147, n=160, width=68, run=136, flags=0, n_out=109):
        return L.egr_resample_sinc(None, ch, n_in, o, n, width, run, None, None, flags, None, n_out, None), native.last_error()

    def tracks(nt=3, total=1000, o=147, n=160, width=68, run=136, flags=0):
        return L.egr_resample_sinc_tracks(None, None, nt, total, o, n, width, run, None, None, flags, None, None), native.last_error()
    cap = (2 ** 32 - 1) // 256 * 256
    for got, code, text in [
            (single(), ARG, "null pointer"), (tracks(), ARG, "null pointer"),
            (single(n_in=0, n_out=0), ARG, "below 1"), (single(ch=0), ARG, "channels"), (single(ch=65536), ARG, "channels"),
            (single(n_out=108), ARG, "ceil"), (single(o=0), ARG, "range"), (single(n=-3), ARG, "range"), (single(width=0), ARG, "range"),
            (single(run=0), ARG, "range"), (single(run=2 * 68 + 147 + 1), ARG, "range"), (single(flags=2), ARG, "flag"),
            (single(n_in=2 ** 50, n_out=1), ARG, "offset cap"), (single(o=2 ** 24, n=2 ** 24, width=68, run=33), UNSUPPORTED, "table cap"),
            (single(ch=1, n_in=cap + 1, o=1, n=1, width=7, run=13, n_out=cap + 1), UNSUPPORTED, "one launch"),
            (tracks(nt=0), ARG, "below 1"), (tracks(total=0), ARG, "below 1"), (tracks(nt=11, total=10), ARG, "more tracks"),
            (tracks(total=cap + 1), UNSUPPORTED, "one launch"), (tracks(run=0), ARG, "range"), (tracks(flags=4), ARG, "flag"),
            (tracks(o=2 ** 24, n=2 ** 24, run=33), UNSUPPORTED, "table cap")]:
        assert got[0] == code and text in got[1], (got, code, text)


# ---------------------------------------------------------------- node surface
_DUMP = """
import json, sys
sys.path.insert(0, %r)
from packload import load_pack
p = load_pack()
print("DUMP" + json.dumps({"keys": sorted(p.NODE_CLASS_MAPPINGS), "display_keys": sorted(p.NODE_DISPLAY_NAME_MAPPINGS)}))
"""
DEFAULT_KEYS = ["Audio Align (XCorr)", "Audio Gain Match", "Audio Null Test", "Audio Plotter", "EgregoraAudioUpscaler", "EgregoraFatLlamaCPU",
                "EgregoraFatLlamaGPU", "Egregora_DeepFilterNet_Denoise", "Metrics (LSD + SI-SDR)", "Null Test (Full)", "Resample Audio (HQ)"]


def _keys_in_child(**flags):
    env = {k: v for k, v in os.environ.items() if not (k.startswith("EGREGORA_") and (k.endswith("_NODES") or k == "EGREGORA_SINC_RESAMPLE"))}
    env.update(flags)
    args = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", _DUMP % str(ROOT)]
    r = subprocess.run(args, env=env, cwd=str(ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("DUMP")][-1][4:])


def test_node_surface_and_registration(pack):
    from egregora_amd import egregora_audio_resample_batch as nb
    node = pack.NODE_CLASS_MAPPINGS["Resample Audio (HQ)"]
    rng = lambda d, lo, hi, st: {"default": d, "min": lo, "max": hi, "step": st}
    assert node.INPUT_TYPES() == {"required": {"audio": ("AUDIO", {}), "target_sr": ("INT", rng(48000, 4000, 384000, 1))},
                                  "optional": {"mode": (["auto", "scipy_polyphase", "torchaudio", "linear"], {}),
                                               "kaiser_beta": ("FLOAT", rng(14.769, 5.0, 20.0, 0.1))}}
    assert (node.RETURN_TYPES, node.RETURN_NAMES, node.FUNCTION, node.CATEGORY) == (("AUDIO",), ("audio_out",), "execute", "Egregora/Utils")
    b = nb.Resample_Audio_HQ_Batch
    assert b.INPUT_TYPES() == node.INPUT_TYPES() and b.INPUT_IS_LIST and b.OUTPUT_IS_LIST == (True,) and b.RETURN_TYPES == node.RETURN_TYPES
    base = _keys_in_child()
    assert base["keys"] == DEFAULT_KEYS == base["display_keys"]
    assert _keys_in_child(EGREGORA_SINC_RESAMPLE="1") == base and _keys_in_child(EGREGORA_RESAMPLE_BATCH_NODES="0") == base
    on = _keys_in_child(EGREGORA_RESAMPLE_BATCH_NODES="1")
    assert sorted(set(on["keys"]) - set(base["keys"])) == ["Resample Audio (HQ) (batch)"] and on["keys"] == on["display_keys"]


def test_switch_is_read_at_call_time(pack, monkeypatch):
    from egregora_amd import resample
    monkeypatch.delenv("EGREGORA_SINC_RESAMPLE", raising=False)
    assert not resample.reference_torchaudio_enabled()
    monkeypatch.setenv("EGREGORA_SINC_RESAMPLE", "1")
    assert resample.reference_torchaudio_enabled()
    monkeypatch.setenv("EGREGORA_SINC_RESAMPLE", "0")
    assert not resample.reference_torchaudio_enabled()


def test_resample_many_host_rules(pack):
    """What resample_many decides before it touches the device: clips at the target pass through, bad clips and modes are refused."""
    from egregora_amd import resample_many as rm
    x = torch.from_numpy(R.signal(2, 100, 1))
    stats = {}
    ys = rm.resample_many([(x, 48000), (x[:1].double(), 48000)], 48000, "torchaudio", stats=stats)
    assert stats == {"calls": 0, "groups": {}} and torch.equal(ys[0], x) and ys[1].dtype == torch.float32
    with pytest.raises(ValueError, match="mode"):
        rm.resample_many([(x, 44100)], 48000, "linear")
    with pytest.raises(ValueError, match="clip 1"):
        rm.resample_many([(x, 44100), (x[0], 44100)], 48000)
