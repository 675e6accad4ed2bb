"""Timing of the windowed-sinc resampler (profiles/resample_sinc.md), one process, one GPU.

1. Kernels: 60 s of stereo audio, 44.1 -> 48 kHz and 48 -> 44.1 kHz, at the filter of the Resample Audio (HQ) node's "torchaudio" mode
   (lowpass_filter_width 64, rolloff 0.945, Kaiser 14.769), device tensors in and out:
     staged -- egr_resample_sinc as it chooses by itself for these ratios (the input span of a tile in LDS),
     direct -- the same call with EGR_SINC_FORCE_DIRECT (x from global memory),
     poly   -- the existing egr_resample_poly (resample.resample_hq: scipy's polyphase definition, another filter).
   The staged and direct results are compared bit for bit before anything is timed.
2. Corpus: the seeded corpus of tools/flashsr_batch_timing.py (200 clips of 2-12 s at 16, 24, 44.1 and 48 kHz, mono and stereo) to
   48 kHz in mode "torchaudio": resample_many (one library call per source rate, one upload, one download) against one
   resample.resample_sinc call per clip (upload, call, download per clip): the single-clip path of this same build; and the same two
   sides on tensors that already sit on the device and stay there (to_host=False).
The sides ALTERNATE inside every round (one warm-up round, then --runs timed rounds); a host clock around work that ends with a device
synchronisation, --reps calls per timing for the kernels; the figure is the median with the min and max of the rounds.

usage: python tools/bench_resample_sinc.py [--clips 200] [--runs 5] [--reps 20] [--seconds 60] [--out FILE.json]
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
    return dict(seconds_median=statistics.median(ts), seconds_min=min(ts), seconds_max=max(ts), seconds=[round(t, 6) for t in ts])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=200)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from packload import load_pack
    load_pack()
    from flashsr_batch_timing import corpus
    from egregora_amd import native, resample, resample_many as rm
    arch = native.require_device()
    sync = torch.cuda.synchronize
    kw = dict(rm.NODE_FILTER, beta=14.769)

    def timed(f, reps=1):
        sync()
        t0 = time.perf_counter()
        for _ in range(reps):
            out = f()
        sync()
        return (time.perf_counter() - t0) / reps, out

    res = dict(arch=arch, device=torch.cuda.get_device_name(0), runs=args.runs, reps=args.reps, filter=dict(kw), kernels={})
    ok = True
    for src, dst in ((44100, 48000), (48000, 44100)):
        x = (0.1 * torch.randn(2, int(args.seconds * src), generator=torch.Generator().manual_seed(src))).cuda()
        _, _, (o, n, width, run) = resample.design_sinc(src, dst, **kw)
        sides = dict(staged=lambda: resample.resample_sinc(x, src, dst, **kw),
                     direct=lambda: resample.resample_sinc(x, src, dst, flags=resample.SINC_FORCE_DIRECT, **kw),
                     poly=lambda: resample.resample_hq(x, src, dst))
        outs = {k: timed(f)[1] for k, f in sides.items()}                  # warm-up round, and the comparison
        same = bool(torch.equal(outs["staged"].view(torch.int32), outs["direct"].view(torch.int32)))
        ok &= same and resample.sinc_staged(o, n, width)
        n_out = outs["staged"].shape[1]
        del outs
        ts = {k: [] for k in sides}
        for _ in range(args.runs):
            for k, f in sides.items():
                ts[k].append(timed(f, args.reps)[0])
        entry = dict(o=o, n=n, width=width, run=run, channels=2, n_in=x.shape[1], n_out=n_out, staged_equals_direct=same,
                     taps_per_output=dict(sinc=run, poly=-(-(2 * 10 * max(o, n) + 1) // n)), **{k: stats_of(v) for k, v in ts.items()})
        entry["direct_over_staged"] = entry["direct"]["seconds_median"] / entry["staged"]["seconds_median"]
        entry["staged_over_poly"] = entry["staged"]["seconds_median"] / entry["poly"]["seconds_median"]
        res["kernels"][f"{src}->{dst}"] = entry
        del x

    clips = corpus(args.clips, 7, torch)
    clips_dev = [(x.cuda().contiguous(), sr) for x, sr in clips]
    sides = dict(per_clip=lambda: [resample.resample_sinc(x.cuda(), sr, 48000, **kw).cpu() for x, sr in clips],
                 many=lambda: rm.resample_many(clips, 48000, "torchaudio", 14.769),
                 per_clip_device=lambda: [resample.resample_sinc(x, sr, 48000, **kw) for x, sr in clips_dev],
                 many_device=lambda: rm.resample_many(clips_dev, 48000, "torchaudio", 14.769, to_host=False))
    outs = {k: timed(f)[1] for k, f in sides.items()}
    equal = all(torch.equal(a, b) and torch.equal(a, c.cpu()) and torch.equal(a, d.cpu())
                for a, b, c, d in zip(outs["per_clip"], outs["many"], outs["per_clip_device"], outs["many_device"]))
    ok &= equal
    st = {}
    rm.resample_many(clips, 48000, "torchaudio", 14.769, stats=st)
    del outs
    ts = {k: [] for k in sides}
    for _ in range(args.runs):
        for k, f in sides.items():
            ts[k].append(timed(f)[0])
    res["corpus"] = dict(clips=len(clips), audio_seconds=sum(x.shape[1] / sr for x, sr in clips), target_sr=48000, mode="torchaudio",
                         results_equal=bool(equal), library_calls=dict(per_clip=sum(sr != 48000 for _, sr in clips), many=st["calls"]),
                         **{k: stats_of(v) for k, v in ts.items()})
    res["corpus"]["per_clip_over_many"] = res["corpus"]["per_clip"]["seconds_median"] / res["corpus"]["many"]["seconds_median"]
    res["corpus"]["per_clip_device_over_many_device"] = (res["corpus"]["per_clip_device"]["seconds_median"] /
                                                         res["corpus"]["many_device"]["seconds_median"])
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
