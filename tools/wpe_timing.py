#!/usr/bin/env python3
"""Time of WPE dereverberation on one MI355X (profiles/wpe.md).

  python tools/wpe_timing.py [--seconds 60] [--repeats 10] [--out FILE.json]

60 s of 48 kHz stereo at the node's default widgets (taps 10, delay 3, 3 iterations, n_fft 1024, hop 256).  `device`: one
egr_wpe_dereverb on a tensor that is already on the device; `node`: Egregora_WPE_Dereverb.execute on a host AUDIO dict, copies
included.  Every call follows a warm-up call and ends in a device synchronise; median / min / max of the repeats.  The bytes are
what the kernels read and write, counted from the shapes.  Without a device the script fails; it has no fallback.
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from packload import load_pack
    load_pack()
    from egregora_amd import egregora_audio_enhance_wpe as ew, native, wpe_engine
    import wpe_cases
    arch = native.require_device()
    sr, C, taps, delay, iters, n_fft, hop = 48000, 2, 10, 3, 3, 1024, 256
    n = int(round(a.seconds * sr))
    x = wpe_cases.signal(C, n, 7)
    xt = torch.from_numpy(x).cuda()
    audio = {"waveform": torch.from_numpy(x)[None], "sample_rate": sr}
    node = ew.Egregora_WPE_Dereverb()
    ways = {"device": lambda: wpe_engine.dereverb(xt, n_fft, hop, taps, delay, iters),
            "node": lambda: node.execute(audio, taps, delay, iters, n_fft, hop, True)[0]["waveform"]}
    first = {k: fn() for k, fn in ways.items()}
    torch.cuda.synchronize()
    if not torch.equal(first["device"].cpu(), first["node"][0]):
        raise SystemExit("node and device results differ")
    times = {k: [] for k in ways}
    for _ in range(a.repeats):
        for k, fn in ways.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    fr, bins = wpe_engine.frames(n, n_fft, hop), n_fft // 2 + 1
    spec, inv = bins * C * fr * 8, bins * fr * 8
    hist = (delay + taps - 1) / 64.0
    nbytes = {"stft": C * n * 4 + spec, "iteration": 2 * spec * (1 + hist) + 3 * inv, "first iteration extra": spec + 2 * inv,
              "last iteration": 2 * spec * (1 + hist) + inv + spec, "istft": spec * (8 + n_fft // hop - 1) / 8 + C * n * 4}
    y = first["device"].cpu().numpy()
    out = {"arch": arch, "device": torch.cuda.get_device_name(0), "seconds_of_audio": a.seconds, "sr": sr, "channels": C,
           "widgets": {"taps": taps, "delay": delay, "iterations": iters, "n_fft": n_fft, "hop": hop}, "repeats": a.repeats,
           "frames": fr, "bins": bins, "bytes": nbytes,
           "ms": {k: {"median": 1e3 * statistics.median(v), "min": 1e3 * min(v), "max": 1e3 * max(v)} for k, v in times.items()},
           "change_against_input": float(np.linalg.norm(y[:, :n] - x) / np.linalg.norm(x))}
    for k, v in out["ms"].items():
        print(f"{k:8s} median {v['median']:9.3f} ms   min {v['min']:9.3f}   max {v['max']:9.3f}")
    print("RESULT " + json.dumps(out))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
