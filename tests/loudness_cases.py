"""Seeded inputs of fixture G15 (restated from tests/golden/make_golden_loudness.py, which cannot be imported without the
reference tree) and the numpy block energies the reference's meter forms, shared by test_eval_loudness.py and
test_gpu_eval_loudness.py."""
import numpy as np
import torch

KEYS = ("ABX Prepare", "ABX Judge", "Loudness Meter (BS1770)", "Audio Gain Match (1770)")
METER_KEYS = ["lufs_integrated", "lufs_momentary", "lufs_short_term", "lra", "true_peak_dbfs"]


def signal(sr, channels, n, seed):
    """[C,n] float32: per channel a tone plus white noise under a 2 s on/off envelope (1.2 s at 1.0, 0.8 s at 0.003)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(n) / float(sr)
    env = np.where(np.mod(np.floor(t * 10.0 + 1e-9), 20.0) < 12.0, 1.0, 0.003)
    rows = [(0.2 * np.sin(2 * np.pi * (440.0 + 170.0 * c) * t + 0.7 * c) + 0.05 * rng.standard_normal(n)) * env for c in range(channels)]
    return np.stack(rows).astype(np.float32)


def case_signal(entry):
    return signal(entry["sr"], entry["channels"], entry["n"], entry["seed"])


def gain_inputs():
    ref = signal(48000, 2, 60000, 161)
    rng = np.random.Generator(np.random.PCG64(162))
    x = (0.41 * signal(48000, 2, 60000, 163) + 0.002 * rng.standard_normal((2, 60000))).astype(np.float32)
    x441 = (0.66 * signal(44100, 2, 55125, 164)).astype(np.float32)
    return ref, {"in": (x, 48000), "in441": (x441, 44100)}


def abx_inputs():
    rng = np.random.Generator(np.random.PCG64(171))
    return (0.1 * rng.standard_normal((2, 60000))).astype(np.float32), (0.1 * rng.standard_normal((2, 50000))).astype(np.float32)


def aud(x, sr, meta=None):
    d = {"waveform": torch.from_numpy(np.ascontiguousarray(x))[None], "sample_rate": sr}
    if meta is not None:
        d["meta"] = meta
    return d


def block_mean_squares(mono, sr, window_s, hop_s):
    """The reference's block loop (egregora_audio_eval_pack.py:157-167, :180-187) on a float32 mono signal."""
    w, h = max(1, int(round(window_s * sr))), max(1, int(round(hop_s * sr)))
    frames = 1 + max(0, (mono.shape[0] - w) // h)
    out = []
    for i in range(frames):
        seg = mono[i * h:i * h + w].astype(np.float64)
        out.append(float(np.mean(seg * seg)))
    return np.asarray(out)
