#!/usr/bin/env python3
"""Times of the loudness meter and the 1770 gain match on one MI355X (profiles/loudness.md).

  python tools/loudness_timing.py [--seconds 60] [--repeats 15] [--out FILE.json]

60 s of 48 kHz stereo, measured two ways that alternate inside one process, each after a warm-up call, each call ended by a device
synchronise, median / min / max of the repeats:
  fused     the nodes as shipped: one egr_loudness_frames (+ one egr_true_peak) per measurement (loudness.py)
  composed  what the library offered before: the reference's call shape on the null-test suite's kernels, i.e. four rounds of
            device_ops.k_weight + block_mean_squares (integrated, momentary, short-term, LRA) and mono_mean -> resample_hq ->
            max |.| for the true peak; for the gain match two device_ops.integrated_lufs
`node` rows go through the node (AUDIO dict on the host in, host -> device copy included); `device` rows start from a tensor on the
device.  Both ways must return the same floats (the kernels are bit-identical); the script fails otherwise.  The reference's CPU
time is the one recorded in fixture G15, scaled by length.
"""
import argparse
import json
import math
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from packload import load_pack
    load_pack()
    from egregora_amd import device_ops, egregora_audio_eval_loudness as el, loudness, native, resample
    arch = native.require_device()
    sr, n = 48000, int(round(a.seconds * 48000))
    rng = np.random.Generator(np.random.PCG64(0))
    t = np.arange(n) / sr
    x = np.stack([0.2 * np.sin(2 * np.pi * 440 * t), 0.2 * np.sin(2 * np.pi * 610 * t + 0.7)]) + 0.05 * rng.standard_normal((2, n))
    x = x.astype(np.float32)
    y = (0.41 * x[:, ::-1]).astype(np.float32).copy()
    A, B = ({"waveform": torch.from_numpy(v)[None], "sample_rate": sr} for v in (x, y))
    xt = torch.from_numpy(x).cuda()

    def composed_measure(xd, oversample=4):
        def ms(w_s, h_s):
            w, h, _ = loudness.block_shape(sr, w_s, h_s, xd.shape[1])
            return device_ops.block_mean_squares(device_ops.k_weight(xd, sr), w, h)
        st = loudness.series(ms(3.0, 1.0))
        out = {"lufs_integrated": loudness.gate(ms(0.400, 0.100)), "lufs_momentary": float(loudness.series(ms(0.400, 0.100)).mean()),
               "lufs_short_term": float(st.mean()), "lra": loudness.lra(loudness.series(ms(3.0, 1.0)))}
        up = resample.resample_hq(device_ops.mono_mean(xd)[None], 1, oversample)
        out["true_peak_dbfs"] = 20.0 * math.log10(float(up.abs().max().cpu()) + 1e-20)
        return out

    def to_dev(audio):
        return torch.from_numpy(np.ascontiguousarray(el.to_internal_audio(audio)["samples"])).cuda()

    def composed_gain():
        r, v = to_dev(A), to_dev(B)
        rl, il = device_ops.integrated_lufs(r, sr), device_ops.integrated_lufs(v, sr)
        g = float(np.clip(rl - il, -12.0, 12.0))
        return device_ops.scale(v, 10 ** (g / 20.0)).cpu().numpy(), g, rl, il

    meter, gain = el.Loudness_Meter_1770(), el.Audio_Gain_Match_1770()
    ways = {
        "meter device fused": lambda: loudness.measure(xt, sr, True, 4),
        "meter device composed": lambda: composed_measure(xt),
        "meter node fused": lambda: meter.execute(A)[0],
        "meter node composed": lambda: composed_measure(to_dev(A)),
        "gain match node fused": lambda: gain.execute(A, B)[1:],
        "gain match node composed": lambda: composed_gain()[1:],
    }
    results = {k: fn() for k, fn in ways.items()}                # warm-up, and the identity check
    torch.cuda.synchronize()
    for kind in ("meter device", "meter node", "gain match node"):
        f, c = results[kind + " fused"], results[kind + " composed"]
        if f != c:
            raise SystemExit(f"{kind}: fused and composed results differ: {f} vs {c}")
    times = {k: [] for k in ways}
    for _ in range(a.repeats):
        for k, fn in ways.items():                               # alternate the ways inside every repeat
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    g15 = json.loads((ROOT / "tests" / "golden" / "g15_loudness.json").read_text())["reference_meter_seconds"]
    ref_s = g15["seconds"] * (n * 2) / (g15["samples"] * g15["channels"])
    out = {"arch": arch, "device": torch.cuda.get_device_name(0), "seconds_of_audio": a.seconds, "sr": sr, "channels": 2, "repeats": a.repeats,
           "ms": {k: {"median": 1e3 * statistics.median(v), "min": 1e3 * min(v), "max": 1e3 * max(v)} for k, v in times.items()},
           "meter": results["meter device fused"],
           "reference_cpu_meter_seconds_scaled": ref_s, "reference_cpu_meter_seconds_fixture": g15}
    for k, v in out["ms"].items():
        print(f"{k:28s} median {v['median']:9.3f} ms   min {v['min']:9.3f}   max {v['max']:9.3f}")
    print(f"reference meter on the CPU, fixture time scaled by length: {ref_s:.1f} s")
    print("RESULT " + json.dumps(out))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
