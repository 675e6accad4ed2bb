"""Corpus timing of the many-clip evaluation (profiles/eval_batch.md): the seeded corpus of tools/flashsr_batch_timing.py (200 clips of
2-12 s at 16, 24, 44.1 and 48 kHz, mono and stereo), each clip paired with a noisy copy (30 dB below it), at the nodes' default
widgets (n_fft 2048, hop 512; true peak at 4x), one process, one GPU.  Per metric family two pairs of sides:
  metrics loop / packed                 -- device_ops.lsd + si_sdr per pair on host tensors uploaded pair by pair (what the node
                                           does) against eval_many.metrics_many on the same host tensors,
  metrics device loop / device packed   -- the same on tensors that already sit on the device,
  loudness loop / packed, device loop / device packed -- loudness.measure per clip against eval_many.loudness_many.
The single path is the baseline; this change does not alter it.  The sides ALTERNATE inside every round (one warm-up round, then
--runs timed rounds); a host clock around work that ends with a device synchronisation; the figure is the median with the min and
max of the rounds.  Before the rounds the packed results are compared with the loop's under the tolerances of
tests/test_gpu_eval_many.py: lsd_p95 and every loudness value equal, lsd_mean within one float32 ulp, si_sdr within 1e-9 dB.

usage: python tools/eval_batch_timing.py [--clips 200] [--runs 5] [--out FILE.json]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))


def stats_of(ts):
    return dict(seconds_median=statistics.median(ts), seconds_min=min(ts), seconds_max=max(ts), seconds=[round(t, 4) for t in ts])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=200)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from packload import load_pack
    load_pack()
    from flashsr_batch_timing import corpus
    from egregora_amd import device_ops, eval_many, loudness, native
    arch = native.require_device()
    clips = corpus(args.clips, 7, torch)
    g = torch.Generator().manual_seed(11)
    pairs = [(x, (x + x.pow(2).mean().sqrt() * 10 ** (-30 / 20.0) * torch.randn(x.shape, generator=g)).float()) for x, _ in clips]
    pairs_dev = [(a.cuda().contiguous(), b.cuda().contiguous()) for a, b in pairs]
    clips_dev = [(a, sr) for (a, _), (_, sr) in zip(pairs_dev, clips)]
    sync = torch.cuda.synchronize

    def one(a, b):
        mean, p95 = device_ops.lsd(a, b)
        return {"lsd_mean_db": mean, "lsd_p95_db": p95, "si_sdr_db": device_ops.si_sdr(a, b)}

    sides = dict(
        metrics_loop=lambda: [one(a.cuda(), b.cuda()) for a, b in pairs],
        metrics_packed=lambda: eval_many.metrics_many(pairs),
        metrics_device_loop=lambda: [one(a, b) for a, b in pairs_dev],
        metrics_device_packed=lambda: eval_many.metrics_many(pairs_dev),
        loudness_loop=lambda: [loudness.measure(x.cuda(), sr) for x, sr in clips],
        loudness_packed=lambda: eval_many.loudness_many(clips),
        loudness_device_loop=lambda: [loudness.measure(x, sr) for x, sr in clips_dev],
        loudness_device_packed=lambda: eval_many.loudness_many(clips_dev),
    )

    def timed(f):
        sync()
        t0 = time.perf_counter()
        out = f()
        sync()
        return time.perf_counter() - t0, out

    outs = {k: timed(f)[1] for k, f in sides.items()}              # warm-up round, and the comparison of the results

    def metrics_agree(loop, packed):
        worst_si, ok = 0.0, True
        for s, m in zip(loop, packed):
            ok &= m["lsd_p95_db"] == s["lsd_p95_db"] and abs(m["lsd_mean_db"] - s["lsd_mean_db"]) <= float(np.spacing(np.float32(s["lsd_mean_db"])))
            worst_si = max(worst_si, abs(m["si_sdr_db"] - s["si_sdr_db"]))
        return bool(ok and worst_si <= 1e-9), worst_si

    m_ok, m_si = metrics_agree(outs["metrics_loop"], outs["metrics_packed"])
    d_ok, d_si = metrics_agree(outs["metrics_device_loop"], outs["metrics_device_packed"])
    l_ok = outs["loudness_loop"] == outs["loudness_packed"] == outs["loudness_device_loop"] == outs["loudness_device_packed"]
    ms, ls = {}, {}
    eval_many.metrics_many(pairs_dev, stats=ms)
    eval_many.loudness_many(clips_dev, stats=ls)
    del outs
    ts = {k: [] for k in sides}
    for _ in range(args.runs):
        for k, f in sides.items():
            ts[k].append(timed(f)[0])
    res = dict(arch=arch, device=torch.cuda.get_device_name(0), clips=len(clips), audio_seconds=sum(x.shape[1] / sr for x, sr in clips),
               widgets=dict(n_fft=2048, hop=512, compute_true_peak=True, oversample=4), runs=args.runs,
               metrics_agree=bool(m_ok and d_ok), worst_si_sdr_difference_db=max(m_si, d_si), loudness_equal=bool(l_ok),
               wave_budget_GB=eval_many.DEFAULT_WAVE_GB,
               # read from the code: a pair on the single path is 6 library calls = 7 kernel launches and 2 memsets, and 3 blocking reads
               metrics=dict(waves=ms["waves"], library_calls=dict(loop=6 * len(clips), packed=ms["library_calls"]),
                            launches=dict(loop=7 * len(clips), packed=ms["launches"]), host_reads=dict(loop=3 * len(clips), packed=ms["waves"])),
               loudness=dict(waves=ls["waves"], library_calls=dict(loop=2 * len(clips), packed=ls["library_calls"]),
                             launches=dict(loop=4 * len(clips), packed=ls["launches"]), host_reads=dict(loop=len(clips), packed=ls["waves"])),
               **{k: stats_of(v) for k, v in ts.items()})
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    return 0 if (m_ok and d_ok and l_ok) else 1


if __name__ == "__main__":
    sys.exit(main())
