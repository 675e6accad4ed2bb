"""The evaluation pack's loudness meter, 1770 gain match and ABX nodes against fixture G15 (captured from the reference's
egregora_audio_eval_pack.py by tests/golden/make_golden_loudness.py) -- everything that needs no device: opt-in registration and
node surfaces, the ABX nodes, the exported symbols, and the host half of loudness.py (gate, level series, loudness range), which
must return the reference's floats bit for bit when it is given the reference's block energies."""
import ctypes
import inspect
import json
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from conftest import gjson
from loudness_cases import KEYS, abx_inputs, aud, block_mean_squares, case_signal

ROOT = Path(__file__).resolve().parent.parent

_DUMP = """
import inspect, json, sys
sys.path.insert(0, %r)
from packload import load_pack
p = load_pack()
out = {"keys": sorted(p.NODE_CLASS_MAPPINGS), "display_keys": sorted(p.NODE_DISPLAY_NAME_MAPPINGS), "surface": {}}
for k in %r:
    if k in p.NODE_CLASS_MAPPINGS:
        c = p.NODE_CLASS_MAPPINGS[k]
        it = c.INPUT_TYPES()
        out["surface"][k] = {"INPUT_TYPES": it, "widget_order": {a: list(v.keys()) for a, v in it.items()},
                             "RETURN_TYPES": list(c.RETURN_TYPES), "RETURN_NAMES": list(c.RETURN_NAMES), "FUNCTION": c.FUNCTION,
                             "CATEGORY": c.CATEGORY, "signature": str(inspect.signature(getattr(c, c.FUNCTION))),
                             "display": p.NODE_DISPLAY_NAME_MAPPINGS[k], "class_name": c.__name__}
print("DUMP" + json.dumps(out))
"""


def _import_in_child(flag):
    env = {k: v for k, v in os.environ.items() if k != "EGREGORA_EVAL_NODES"}
    if flag is not None:
        env["EGREGORA_EVAL_NODES"] = flag
    args = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", _DUMP % (str(ROOT), KEYS)]
    r = subprocess.run(args, env=env, cwd=str(ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("DUMP")][-1]
    return json.loads(line[4:])


def test_registration_is_opt_in_and_surfaces_equal_reference():
    g = gjson("g15_loudness")
    base = _import_in_child(None)
    assert base["keys"] == base["display_keys"] == sorted([
        "EgregoraAudioUpscaler", "EgregoraFatLlamaGPU", "EgregoraFatLlamaCPU", "Metrics (LSD + SI-SDR)", "Resample Audio (HQ)",
        "Egregora_DeepFilterNet_Denoise", "Audio Align (XCorr)", "Audio Gain Match", "Audio Null Test", "Audio Plotter", "Null Test (Full)"])
    assert _import_in_child("0")["keys"] == base["keys"]                  # only "1" switches the nodes on
    on = _import_in_child("1")
    assert sorted(set(on["keys"]) - set(base["keys"])) == sorted(KEYS) and set(base["keys"]) <= set(on["keys"])
    assert on["keys"] == on["display_keys"]
    for key in KEYS:
        assert on["surface"][key] == json.loads(json.dumps(g["surface"][key])), key


def test_module_mappings_without_the_switch(pack):
    """The module carries its own mappings whatever the environment says (the package merges them on request)."""
    from egregora_amd import egregora_audio_eval_loudness as el
    g = gjson("g15_loudness")
    assert list(el.NODE_CLASS_MAPPINGS) == list(KEYS) == list(el.NODE_DISPLAY_NAME_MAPPINGS)
    for key in KEYS:
        cls = el.NODE_CLASS_MAPPINGS[key]
        assert cls.__name__ == g["surface"][key]["class_name"] and isinstance(cls.RETURN_TYPES, tuple)
        assert str(inspect.signature(cls.execute)) == g["surface"][key]["signature"]


def test_abx_nodes_reproduce_reference(pack):
    from egregora_amd import egregora_audio_eval_loudness as el
    g = gjson("g15_loudness")["abx"]
    A, B = abx_inputs()
    prep = el.ABX_Prepare()
    assert [prep.execute(aud(A, 48000), aud(B, 48000), 1.0, s)[3] for s in range(8)] == g["x_is"]
    assert {m["x_is"] for m in g["x_is"]} == {"A", "B"}                  # the seeds exercise both picks
    for c in g["clips"]:
        a_c, b_c, x_c, meta = prep.execute(aud(A, 48000, {"name": "A"}), aud(B, 48000, {"name": "B"}), random_seed=3, **c["kwargs"])
        assert [list(d["waveform"].shape) for d in (a_c, b_c, x_c)] == c["shapes"] and meta == c["meta"]
        assert x_c is (a_c if meta["x_is"] == "A" else b_c) and x_c["meta"] == c["x_meta"]
        assert sorted(a_c.keys()) == c["keys"] and a_c["sample_rate"] == c["sr"] and a_c["samples"].dtype == np.float32
        assert [float(v) for v in a_c["samples"].ravel()[:3]] == c["first"]
        s = int(round(c["kwargs"].get("start_seconds", 0.0) * 48000))
        if a_c["samples"].shape[0] == 2 and a_c["samples"].shape[1] > 2:
            assert np.array_equal(a_c["samples"], A[:, s:s + a_c["samples"].shape[1]])
            assert np.array_equal(b_c["samples"], B[:, s:s + b_c["samples"].shape[1]])
    judge = el.ABX_Judge()
    for c in g["judge"]:
        assert judge.execute(c["meta"], c["guess"]) == (c["result"],)


def test_new_symbols_are_declared_exported_and_bound(pack):
    from egregora_amd import native
    hdr = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "egregora_amd.h").read_text(), flags=re.S)
    lib = ctypes.CDLL(str(native.LIB_PATH))
    for name, nargs in (("egr_loudness_frames", 15), ("egr_true_peak", 8)):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and len(native.SIGNATURES[name][1]) == nargs
    assert native.ABI_VERSION == 5 and "#define EGR_ABI_VERSION 5" in hdr


def test_loudness_nodes_have_no_cpu_fallback(pack):
    import torch
    from egregora_amd import egregora_audio_eval_loudness as el
    if torch.cuda.is_available():
        return                                   # the GPU file runs the nodes
    a = aud(np.zeros((2, 4800), np.float32), 48000)
    with pytest.raises(RuntimeError, match="No AMD GPU|no CPU fallback"):
        el.Loudness_Meter_1770().execute(a)
    with pytest.raises(RuntimeError, match="No AMD GPU|no CPU fallback"):
        el.Audio_Gain_Match_1770().execute(a, a)


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_host_half_reproduces_reference_bit_for_bit(pack, name):
    """Block energies formed by numpy from the oracle's restatement of the reference's K-weighting loop, then loudness.py's gate,
    series and range: every level equals the reference meter's float exactly."""
    from egregora_amd import loudness
    from oracle import nulltest as on
    e = gjson("g15_loudness")["cases"][name]
    x = case_signal(e)
    assert list(x.shape) == e["measured_shape"]
    mono = on.k_weight(e["sr"], x).mean(axis=0)
    ms_a = block_mean_squares(mono, e["sr"], 0.400, 0.100)
    ms_b = block_mean_squares(mono, e["sr"], 3.0, 1.0)
    assert (len(ms_a), len(ms_b)) == (loudness.block_shape(e["sr"], 0.400, 0.100, e["n"])[2], loudness.block_shape(e["sr"], 3.0, 1.0, e["n"])[2])
    st = loudness.series(ms_b)
    assert st.dtype == np.float32
    got = {"lufs_integrated": loudness.gate(ms_a), "lufs_momentary": float(loudness.series(ms_a).mean()),
           "lufs_short_term": float(st.mean()), "lra": loudness.lra(st)}
    want = e["ref"]["4"]
    for k, v in got.items():
        assert v == want[k], (name, k, v, want[k])


def test_fixture_keeps_clear_of_the_gates():
    g = gjson("g15_loudness")
    assert sorted(g["cases"]) == ["a", "b", "c", "d", "e", "f1", "f1000"]
    for name, e in g["cases"].items():
        assert e["gate_margin_db"] >= 0.01, (name, e["gate_margin_db"])
    assert len(g["cases"]["d"]["f64"]["4"]) == 5 and g["cases"]["d"]["ref"]["4"]["lra"] > 1.0     # a range that means something
    assert sorted(g["cases"]["a"]["ref"]) == ["1", "4", "8"]
