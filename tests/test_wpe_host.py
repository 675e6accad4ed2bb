"""WPE dereverberation (SPEC.md 4d), everything that needs no device: opt-in registration and the node surface against fixture G16
(captured from the reference by tests/golden/make_golden_wpe.py), the exported symbols, the float64 restatement's framing
(tests/wpe_numpy.py), the passthrough and limit rules of the node, the condition classes of the inputs the GPU tests rest on
(tests/wpe_cases.py), and a host walk of the kernel's index code under the address and undefined-behaviour sanitizers."""
import ctypes
import json
import os
import re
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import wpe_cases
import wpe_numpy as wn
from conftest import gjson

ROOT = Path(__file__).resolve().parent.parent
KEY = "Egregora_WPE_Dereverb"
SYMBOLS = ["egr_wpe_dereverb", "egr_wpe_frames", "egr_wpe_istft", "egr_wpe_iterate", "egr_wpe_stft", "egr_wpe_workspace_bytes"]

_DUMP = """
import inspect, json, sys
sys.path.insert(0, %r)
from packload import load_pack
p = load_pack()
out = {"keys": sorted(p.NODE_CLASS_MAPPINGS), "display_keys": sorted(p.NODE_DISPLAY_NAME_MAPPINGS), "surface": {}}
k = %r
if k in p.NODE_CLASS_MAPPINGS:
    c = p.NODE_CLASS_MAPPINGS[k]
    it = c.INPUT_TYPES()
    out["surface"][k] = {"INPUT_TYPES": it, "widget_order": {a: list(v.keys()) for a, v in it.items()},
                         "RETURN_TYPES": list(c.RETURN_TYPES), "RETURN_NAMES": list(getattr(c, "RETURN_NAMES", ())), "FUNCTION": c.FUNCTION,
                         "CATEGORY": c.CATEGORY, "signature": str(inspect.signature(getattr(c, c.FUNCTION))),
                         "display": p.NODE_DISPLAY_NAME_MAPPINGS[k], "class_name": c.__name__}
print("DUMP" + json.dumps(out))
"""


def _import_in_child(flag):
    env = {k: v for k, v in os.environ.items() if k not in ("EGREGORA_ENHANCE_NODES", "EGREGORA_EVAL_NODES")}
    if flag is not None:
        env["EGREGORA_ENHANCE_NODES"] = flag
    args = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", _DUMP % (str(ROOT), KEY)]
    r = subprocess.run(args, env=env, cwd=str(ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("DUMP")][-1]
    return json.loads(line[4:])


@pytest.fixture(scope="module")
def node(pack):
    from egregora_amd import egregora_audio_enhance_wpe as ew
    return ew.Egregora_WPE_Dereverb()


def test_registration_is_opt_in_and_surface_equals_reference():
    g = gjson("g16_wpe_surface")
    base = _import_in_child(None)
    assert KEY not in base["keys"] and KEY not in base["display_keys"]
    assert _import_in_child("0")["keys"] == base["keys"]                  # only "1" switches the node on
    on = _import_in_child("1")
    assert sorted(set(on["keys"]) - set(base["keys"])) == [KEY] and on["keys"] == on["display_keys"]
    assert on["surface"][KEY] == json.loads(json.dumps(g["surface"][KEY]))


def test_symbols_are_declared_exported_and_bound(pack):
    from egregora_amd import native
    txt = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "egregora_amd.h").read_text(), flags=re.S)
    declared = sorted(s for s in set(re.findall(r"\b(egr_[a-z0-9_]+)\s*\(", txt)) if s.startswith("egr_wpe_"))
    assert declared == SYMBOLS
    lib = ctypes.CDLL(str(native.LIB_PATH))
    for s in SYMBOLS:
        assert hasattr(lib, s) and s in native.SIGNATURES, s
    L = native.lib()
    assert L.egr_abi_version() == native.ABI_VERSION == 5
    # host-only entry points: the frame count and workspace size follow SPEC WPE-P1 / P3
    for n, n_fft, hop in ((1, 256, 64), (63, 256, 128), (16000, 256, 64), (64000, 768, 192), (20000, 4096, 1024)):
        assert L.egr_wpe_frames(n, n_fft, hop) == wn.frame_count(n, n_fft, hop)
    for n_fft, hop in ((256, 256), (1024, 192), (256, 1024)):
        assert L.egr_wpe_frames(1000, n_fft, hop) == 0 and L.egr_wpe_workspace_bytes(2, 1000, n_fft, hop, 10) == 0
    fr, bins = wn.frame_count(32000, 256, 64), 129
    assert L.egr_wpe_workspace_bytes(2, 32000, 256, 64, 10) >= 2 * bins * 2 * fr * 8 + 2 * bins * fr * 8 + bins * 4


@pytest.mark.parametrize("n_fft,hop", [(256, 64), (256, 128), (768, 192), (4096, 1024)])
@pytest.mark.parametrize("T", [1, 63, 1000])
def test_restatement_round_trip(n_fft, hop, T):
    """WPE-P2's defining property: synthesis(analysis(y)) = y on [0, T), and the output length follows the formula."""
    rng = np.random.Generator(np.random.PCG64(1000 * n_fft + T))
    y = rng.standard_normal((2, T))
    Y = wn.analysis(y, n_fft, hop)
    frames = -(-(T + n_fft - 2 * hop) // hop) + 1
    assert Y.shape == (n_fft // 2 + 1, 2, frames) and Y.dtype == np.complex128
    z = wn.synthesis(Y, n_fft, hop)
    assert z.shape == (2, frames * hop - (n_fft - hop)) and z.shape[1] >= T
    assert np.max(np.abs(z[:, :T] - y)) <= 1e-12
    assert np.max(np.abs(z[:, T:])) <= 1e-12                               # the zero padding comes back as zeros


def test_engine_windows_equal_restatement(pack):
    from egregora_amd import wpe_engine
    for n_fft, hop in ((256, 64), (768, 192), (4096, 1024)):
        assert np.array_equal(wpe_engine.window(n_fft), wn.window(n_fft))
        assert np.allclose(wpe_engine.synthesis_window(n_fft, hop), wn.synthesis_window(n_fft, hop), rtol=1e-15, atol=0)
        assert wpe_engine.frames(12345, n_fft, hop) == wn.frame_count(12345, n_fft, hop)
        assert wpe_engine.out_length(12345, n_fft, hop) == wn.out_length(12345, n_fft, hop)


@pytest.mark.parametrize("n_fft,hop", [(256, 256), (1024, 192), (256, 1024)])
def test_unsupported_framing_passes_the_input_through(node, n_fft, hop, capsys):
    """WPE-P3: no device is touched, the input comes back unchanged with the reference's warning and meta."""
    g = gjson("g16_wpe_surface")["passthrough"]
    x = torch.randn(2, 2, 500, generator=torch.Generator().manual_seed(3))
    (out,) = node.execute({"waveform": x.clone(), "sample_rate": 16000, "meta": {"k": 1}}, 5, 2, 2, n_fft, hop, True)
    assert torch.equal(out["waveform"], x) and out["waveform"].dtype == torch.float32 and out["sample_rate"] == 16000
    assert sorted(out.keys()) == g["keys"] and sorted(out["meta"].keys()) == g["meta_keys"]
    assert out["meta"]["wpe"] == dict(g["wpe_meta"], n_fft=n_fft, hop=hop)
    assert "Warning: WPE processing failed" in capsys.readouterr().out


def test_empty_input_passes_through(node, capsys):
    (out,) = node.execute({"waveform": torch.zeros(1, 2, 0), "sample_rate": 16000})
    assert tuple(out["waveform"].shape) == (1, 2, 0) and out["meta"]["wpe"]["taps"] == 10
    assert "Warning: WPE processing failed" in capsys.readouterr().out


def test_limits_raise(node, pack):
    """WPE-P7: K = channels * taps <= 64, n_fft even and <= 4096; a RuntimeError names the limit before any device work."""
    from egregora_amd import wpe_engine
    with pytest.raises(RuntimeError, match="K <= 64"):
        node.execute({"waveform": torch.zeros(1, 3, 4000), "sample_rate": 16000}, 22, 3, 1, 256, 64, True)
    with pytest.raises(RuntimeError, match="<= 4096"):
        node.execute({"waveform": torch.zeros(1, 1, 4000), "sample_rate": 16000}, 3, 1, 1, 8192, 2048, True)
    with pytest.raises(RuntimeError, match="even"):
        wpe_engine.check_limits(1, 3, 255)
    wpe_engine.check_limits(2, 32, 4096)                                   # K = 64 is inside


@pytest.mark.parametrize("name", sorted(wpe_cases.CASES))
def test_case_condition_class(name):
    """The GPU tests compare forward errors on the well-conditioned cases and backward errors on the hard ones; this pins which is
    which.  Spectra are rounded to complex64 first, as the device holds them."""
    c = wpe_cases.CASES[name]
    Y = wn.analysis(wpe_cases.case_signal(name), c["n_fft"], c["hop"]).astype(np.complex64)
    cond = wn.max_condition(Y, c["taps"], c["delay"], c["iterations"])
    print(f"case {name}: max cond(R) {cond:.2e}")
    if c["cls"] == "well":
        assert cond <= wpe_cases.WELL_MAX_COND, cond
    else:
        assert cond > wpe_cases.HARD_MIN_COND, cond
    X = wn.wpe(Y.astype(np.complex128), c["taps"], c["delay"], c["iterations"])
    assert wn.rel_rms(X, Y.astype(np.complex128)) > 0.1                   # dereverberation changes these inputs


def test_restatement_guard_and_filter_definition():
    """WPE-P5 in the restatement: a silent bin and an input with fewer frames than K keep X = Y; elsewhere X = Y - G^H Ytilde
    solves the normal equations R G = P."""
    c = wpe_cases.CASES["A"]
    Y = wn.analysis(wpe_cases.case_signal("A"), c["n_fft"], c["hop"])
    Y[7] = 0.0
    X, G, ok, R, P = wn.iterate(Y, wn.psd_inverse(Y), c["taps"], c["delay"])
    assert not ok[7] and ok.sum() == len(ok) - 1 and np.array_equal(X[7], Y[7]) and np.all(np.isfinite(X))
    res = np.linalg.norm(R[ok] @ G[ok] - P[ok], axis=(1, 2))
    assert np.all(res <= 1e-12 * (np.linalg.norm(R[ok], axis=(1, 2)) * np.linalg.norm(G[ok], axis=(1, 2)) + np.linalg.norm(P[ok], axis=(1, 2))))
    short = wn.analysis(wpe_cases.signal(1, 300, 9), 256, 64)
    assert short.shape[2] < 10
    Xs, _, oks, _, _ = wn.iterate(short, wn.psd_inverse(short), 10, 3)
    assert not oks.any() and np.array_equal(Xs, short)


def test_kernel_index_code_under_host_sanitizers(tmp_path):
    """csrc/egr_wpe_index.h (tile walk, history indexing, block ownership of k_wpe_iter) compiled for the host with
    -fsanitize=address,undefined and walked thread by thread against the sequential definition (tools/wpe_host_check.cpp)."""
    rocm_clang = Path(os.environ.get("ROCM_PATH", "/opt/rocm")) / "llvm" / "bin" / "clang++"    # the build needs ROCm, so this one exists
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or (str(rocm_clang) if rocm_clang.exists() else None)
    assert cxx is not None, "no host C++ compiler, not even ROCm's clang++: the sanitizer walk cannot run"
    exe = tmp_path / "wpe_host_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        str(ROOT / "tools" / "wpe_host_check.cpp"), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "all shapes pass" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
