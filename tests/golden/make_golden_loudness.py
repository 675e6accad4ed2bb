#!/usr/bin/env python3
"""Golden fixture G15: the reference's `Loudness Meter (BS1770)`, `Audio Gain Match (1770)`, `ABX Prepare` and `ABX Judge` nodes
(egregora_audio_eval_pack.py:132-382) on seeded signals, captured by importing the reference's module.  Data only: inputs are
regenerated from seeds by the tests (`signal`, `gain_inputs`, `abx_inputs` below are restated there); outputs, node surfaces
and the reference's wall time are stored.

  python tests/golden/make_golden_loudness.py REFERENCE_DIR      # writes tests/golden/g15_loudness.json, g15_loudness.npz

Next to every meter dictionary the same quantities from a float64 restatement (scipy.signal.lfilter form of the one-pole filter,
everything downstream in double): the distance between the two is the reference's own float32 round-off and sets the tests' bar.
`gate_margin_db` is the smallest distance of a 400 ms block from the -10 dB gate and of a short-term value from the LRA gate; the
signals are built so that no block sits near a gate (asserted here: >= 0.01 dB), because a value that crosses one moves the
result by whole blocks, not by round-off.
"""
import importlib.util
import inspect
import json
import math
import os
import sys
import time
from pathlib import Path

import numpy as np
import scipy.signal as sps
import torch

REF = Path(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("EGREGORA_REFERENCE", "reference"))
OUT = Path(__file__).resolve().parent
KEYS = ("ABX Prepare", "ABX Judge", "Loudness Meter (BS1770)", "Audio Gain Match (1770)")

# name -> (sample rate, channels, samples, PCG64 seed)
CASES = {"a": (48000, 2, 60000, 151), "b": (44100, 1, 185220, 152), "c": (11025, 3, 70000, 153), "d": (8000, 1, 112000, 154),
         "e": (384000, 2, 200000, 155), "f1000": (48000, 2, 1000, 156), "f1": (48000, 2, 1, 157)}
OVERSAMPLE = {"a": (4, 1, 8)}


def signal(sr, channels, n, seed):
    """[C,n] float32: per channel a tone plus white noise (own frequency, own noise: decorrelated) under a 2 s on/off envelope,
    1.2 s at level 1.0 then 0.8 s at level 0.003, edges on multiples of 100 ms."""
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(n) / float(sr)
    env = np.where(np.mod(np.floor(t * 10.0 + 1e-9), 20.0) < 12.0, 1.0, 0.003)
    rows = [(0.2 * np.sin(2 * np.pi * (440.0 + 170.0 * c) * t + 0.7 * c) + 0.05 * rng.standard_normal(n)) * env for c in range(channels)]
    return np.stack(rows).astype(np.float32)


def gain_inputs():
    """(ref [2,60000] @ 48 kHz, in [2,60000] @ 48 kHz, in441 [2,55125] @ 44.1 kHz)"""
    ref = signal(48000, 2, 60000, 161)
    rng = np.random.Generator(np.random.PCG64(162))
    x = (0.41 * signal(48000, 2, 60000, 163) + 0.002 * rng.standard_normal((2, 60000))).astype(np.float32)
    x441 = (0.66 * signal(44100, 2, 55125, 164)).astype(np.float32)
    return ref, x, x441


GAIN_CASES = (("lufs", "in", {}), ("rms", "in", dict(mode="RMS")), ("clipped", "in", dict(mode="LUFS-I", max_gain_db=1.0)),
              ("rate", "in441", dict(mode="LUFS-I")))


def abx_inputs():
    """A [2,60000], B [2,50000] @ 48 kHz"""
    rng = np.random.Generator(np.random.PCG64(171))
    return (0.1 * rng.standard_normal((2, 60000))).astype(np.float32), (0.1 * rng.standard_normal((2, 50000))).astype(np.float32)


ABX_CLIPS = (dict(clip_seconds=1.0, start_seconds=0.25), dict(clip_seconds=1.0, start_seconds=0.9), dict(clip_seconds=10.0),
             dict(clip_seconds=1.0, start_seconds=2.0))


def aud(x, sr, meta=None):
    d = {"waveform": torch.from_numpy(np.ascontiguousarray(x))[None], "sample_rate": sr}
    if meta is not None:
        d["meta"] = meta
    return d


def meter_f64(sr, x, oversample):
    """The meter in double: (dict in the reference's key order, gate margin in dB)."""
    k = math.exp(-2 * math.pi * (60.0 / (sr * 0.5)))
    xd = x.astype(np.float64)
    y = xd - sps.lfilter([1.0 - k], [1.0, -k], xd, axis=1)
    y[:, 1:] += 0.02 * (y[:, 1:] - y[:, :-1])
    mono = y.mean(axis=0)

    def blocks(w_s, h_s):
        w, h = max(1, int(round(w_s * sr))), max(1, int(round(h_s * sr)))
        frames = 1 + max(0, (mono.shape[0] - w) // h)
        return np.asarray([float(np.mean(mono[i * h:i * h + w] ** 2)) for i in range(frames)])

    ms = blocks(0.400, 0.100) + 1e-20
    ungated = -0.691 + 10.0 * np.log10(np.mean(ms))
    per = -0.691 + 10.0 * np.log10(ms)
    keep = per >= ungated - 10.0
    margin = float(np.min(np.abs(per - (ungated - 10.0))))
    integrated = float(-0.691 + 10.0 * np.log10(np.mean(ms[keep] if np.any(keep) else ms)))
    mom = -0.691 + 10.0 * np.log10(blocks(0.400, 0.100) + 1e-20)
    st = -0.691 + 10.0 * np.log10(blocks(3.0, 1.0) + 1e-20)
    gate = np.percentile(st, 10.0) - 20.0
    margin = min(margin, float(np.min(np.abs(st - gate))))
    pool = st[st > gate]
    if pool.size == 0:
        pool = st
    peak = float(np.max(np.abs(sps.resample_poly(xd.mean(axis=0), oversample, 1))))
    d = {"lufs_integrated": integrated, "lufs_momentary": float(mom.mean()), "lufs_short_term": float(st.mean()),
         "lra": float(np.percentile(pool, 95.0) - np.percentile(pool, 10.0)), "true_peak_dbfs": 20.0 * math.log10(peak + 1e-20)}
    return d, margin


def surf(cls, display):
    it = cls.INPUT_TYPES()
    return {"INPUT_TYPES": it, "widget_order": {k: list(v.keys()) for k, v in it.items()}, "RETURN_TYPES": list(cls.RETURN_TYPES),
            "RETURN_NAMES": list(cls.RETURN_NAMES), "FUNCTION": cls.FUNCTION, "CATEGORY": cls.CATEGORY,
            "signature": str(inspect.signature(getattr(cls, cls.FUNCTION))), "display": display, "class_name": cls.__name__}


def main():
    spec = importlib.util.spec_from_file_location("ref_eval", REF / "egregora_audio_eval_pack.py")
    ev = importlib.util.module_from_spec(spec)
    sys.modules["ref_eval"] = ev
    spec.loader.exec_module(ev)
    g, arrs = {"cases": {}, "gain": {}, "abx": {}, "surface": {}}, {}

    meter = ev.Loudness_Meter_1770()
    for name, (sr, ch, n, seed) in CASES.items():
        x = signal(sr, ch, n, seed)
        seen = ev.to_internal_audio(aud(x, sr))["samples"]          # what the reference measures after its own AUDIO coercion
        e = {"sr": sr, "channels": ch, "n": n, "seed": seed, "measured_shape": list(seen.shape), "ref": {}, "f64": {}}
        for os_ in OVERSAMPLE.get(name, (4,)):
            t0 = time.perf_counter()
            (m,) = meter.execute(aud(x, sr), True, os_)
            dt = time.perf_counter() - t0
            assert list(m) == ["lufs_integrated", "lufs_momentary", "lufs_short_term", "lra", "true_peak_dbfs"]
            e["ref"][str(os_)] = m
            e["f64"][str(os_)], margin = meter_f64(sr, seen, os_)
            if name == "a" and os_ == 4:
                g["reference_meter_seconds"] = {"case": "a", "seconds": dt, "samples": n, "channels": ch, "sr": sr}
        (m,) = meter.execute(aud(x, sr), False)
        e["keys_without_true_peak"] = list(m)
        e["gate_margin_db"] = margin
        if not name.startswith("f"):                                 # (f): a single block, which is its own gate reference
            assert margin >= 0.01, (name, margin)
        g["cases"][name] = e
        print(name, e["measured_shape"], {k: (v, e["f64"]["4"][k], abs(v - e["f64"]["4"][k])) for k, v in e["ref"]["4"].items()}, "margin", margin)

    ref, x, x441 = gain_inputs()
    ins = {"in": (x, 48000), "in441": (x441, 44100)}
    for name, which, kw in GAIN_CASES:
        xi, sri = ins[which]
        out, gdb, rl, il = ev.Audio_Gain_Match_1770().execute(aud(ref, 48000), aud(xi, sri, {"tag": name}), **kw)
        arrs[f"gain_{name}"] = out["samples"][:, ::29].copy()
        g["gain"][name] = {"input": which, "kwargs": kw, "gain_db": gdb, "ref_level": rl, "in_level": il, "shape": list(out["waveform"].shape),
                           "sr": out["sample_rate"], "meta": out["meta"], "keys": sorted(out.keys()),
                           "max_abs": float(np.abs(out["samples"]).max())}
        print("gain", name, gdb, rl, il, out["waveform"].shape)

    A, B = abx_inputs()
    prep = ev.ABX_Prepare()
    g["abx"]["x_is"] = [prep.execute(aud(A, 48000), aud(B, 48000), 1.0, s)[3] for s in range(8)]
    g["abx"]["clips"] = []
    for kw in ABX_CLIPS:
        a_c, b_c, x_c, meta = prep.execute(aud(A, 48000, {"name": "A"}), aud(B, 48000, {"name": "B"}), random_seed=3, **kw)
        g["abx"]["clips"].append({"kwargs": kw, "shapes": [list(d["waveform"].shape) for d in (a_c, b_c, x_c)], "meta": meta,
                                  "x_meta": x_c["meta"], "keys": sorted(a_c.keys()), "sr": a_c["sample_rate"],
                                  "first": [float(v) for v in a_c["samples"].ravel()[:3]]})
    judge = ev.ABX_Judge()
    g["abx"]["judge"] = [{"meta": m, "guess": gs, "result": judge.execute(m, gs)[0]}
                         for m, gs in (({"x_is": "A", "seed": 1}, "A"), ({"x_is": "A", "seed": 1}, "B"), ({"x_is": "b"}, "b"), ({}, "A"))]

    for key in KEYS:
        g["surface"][key] = surf(ev.NODE_CLASS_MAPPINGS[key], ev.NODE_DISPLAY_NAME_MAPPINGS[key])
    np.savez_compressed(OUT / "g15_loudness.npz", **arrs)
    (OUT / "g15_loudness.json").write_text(json.dumps(g, indent=1, sort_keys=True, ensure_ascii=False) + "\n", encoding="utf-8")
    print("wrote g15_loudness.json / g15_loudness.npz; reference meter on case (a):", g["reference_meter_seconds"])


if __name__ == "__main__":
    main()
