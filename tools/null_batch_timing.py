"""Corpus timing of the many-pair null test (profiles/null_batch.md): the seeded corpus of tools/flashsr_batch_timing.py (200 clips of
2-12 s at 16, 24, 44.1 and 48 kHz, mono and stereo), each clip paired with a copy that is delayed by a known fractional amount within
+-8 ms, scaled within +-6 dB and carries noise 30 dB below it, at the widgets of `Null Test (Full)` (200 ms, fractional, 64 taps,
LUFS-I, n_fft 2048, hop 512), one process, one GPU.  Two pairs of sides:
  loop / packed                 -- align_stage -> gain_stage -> null_stage per pair on host tensors uploaded pair by pair (what the node
                                   does) against null_many.full_many on the same host tensors,
  device loop / device packed   -- the same on tensors that already sit on the device.
The stage functions are the single path, which this change does not alter.  The sides ALTERNATE inside every round (one warm-up round,
then --runs timed rounds); a host clock around work that ends with a device synchronisation; the figure is the median with the min
and max of the rounds.  Before the rounds the packed results are compared with the loop's under the bounds of
tests/test_gpu_null_many.py and the recovery of the known delays is printed.  Also measured: egr_nullmany_shift_fir alone on the
corpus' rows (64 and 255 taps), and the creation of the transform plans per group (a cold call of delays_many against a warm one).

usage: python tools/null_batch_timing.py [--clips 200] [--runs 5] [--out FILE.json]
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
    from egregora_amd import egregora_null_test_suite as ns, native, null_many
    arch = native.require_device()
    clips = corpus(args.clips, 7, torch)
    g = torch.Generator().manual_seed(13)
    pairs, srs, known = [], [], []
    for x, sr in clips:                                # corpus construction (not timed): a spectral delay of the zero-padded clip
        d = float((torch.rand(1, generator=g) * 2 - 1) * 0.008 * sr)
        gain = 10 ** (float(torch.rand(1, generator=g) * 12 - 6) / 20.0)
        n = x.shape[1]
        f = torch.fft.rfftfreq(2 * n, device="cuda", dtype=torch.float64)
        X = torch.fft.rfft(torch.nn.functional.pad(x.cuda().double(), (0, n)), dim=1)
        y = torch.fft.irfft(X * torch.exp(-2j * np.pi * f * d), 2 * n, dim=1)[:, :n].float().cpu()
        y = gain * y + x.pow(2).mean().sqrt() * 10 ** (-30 / 20.0) * torch.randn(x.shape, generator=g)
        pairs.append((x.contiguous(), y.contiguous()))
        srs.append(sr)
        known.append(d)
    pairs_dev = [(a.cuda().contiguous(), b.cuda().contiguous()) for a, b in pairs]
    sync = torch.cuda.synchronize

    def one(a, b, sr):
        aligned, lag = ns.align_stage(a, b, sr, 200, True, 64)
        matched, gain_db, _, _ = ns.gain_stage(a, aligned, sr, "LUFS-I")
        null, metrics = ns.null_stage(a, matched, sr, True, False, True, True, True, True, False, 2048, 512)
        return matched, null, float(1000.0 * lag / sr), float(gain_db), metrics

    sides = dict(
        loop=lambda: [one(a.cuda(), b.cuda(), sr) for (a, b), sr in zip(pairs, srs)],
        packed=lambda: null_many.full_many(pairs, srs),
        device_loop=lambda: [one(a, b, sr) for (a, b), sr in zip(pairs_dev, srs)],
        device_packed=lambda: null_many.full_many(pairs_dev, srs),
    )

    def timed(f):
        sync()
        t0 = time.perf_counter()
        out = f()
        sync()
        return time.perf_counter() - t0, out

    # the transform plans of the many-path: a cold call creates one per transform length, a warm one finds them
    null_many.release_plans()
    st = {}
    cold = timed(lambda: null_many.delays_many(pairs_dev, srs, 200, stats=st))[0]
    warm = timed(lambda: null_many.delays_many(pairs_dev, srs, 200))[0]
    lengths = sorted({null_many.transform_length(min(a.shape[1], b.shape[1])) for a, b in pairs})

    outs = {k: timed(f)[1] for k, f in sides.items()}              # warm-up round, and the comparison of the results

    def agree(loop, packed):
        w = dict(bits=True, rms=0.0, corr_ulps=0.0, lsd_ulps=0.0, equal=True)
        for s, m in zip(loop, packed):
            w["bits"] &= torch.equal(s[0].view(torch.int32), m[0].view(torch.int32)) and torch.equal(s[1].view(torch.int32), m[1].view(torch.int32))
            w["equal"] &= s[2:4] == m[2:4] and all(s[4][k] == m[4][k] for k in ("null_lufs", "lsd_p95_db", "overshoot_count", "clipped_pct", "scale_k"))
            w["rms"] = max(w["rms"], abs(s[4]["null_rms_dbfs"] - m[4]["null_rms_dbfs"]))
            for key, k in (("corr_ulps", "corr_coef"), ("lsd_ulps", "lsd_mean_db")):
                w[key] = max(w[key], abs(s[4][k] - m[4][k]) / float(np.spacing(np.float32(max(abs(s[4][k]), abs(m[4][k]))))))
        w["ok"] = bool(w["bits"] and w["equal"] and w["rms"] <= 1e-9 and w["corr_ulps"] <= 1.0 and w["lsd_ulps"] <= 1.0)
        return w

    a_host, a_dev = agree(outs["loop"], outs["packed"]), agree(outs["device_loop"], outs["device_packed"])
    recovered = [abs(o[2] * sr / 1000.0 - (d - 1)) for o, sr, d in zip(outs["device_packed"], srs, known)]
    print(f"agreement host {a_host} device {a_dev}", file=sys.stderr)
    print(f"known delays recovered (lag = d - 1, quirk Q8): median {statistics.median(recovered):.4f}, worst {max(recovered):.4f} samples", file=sys.stderr)
    fs = {}
    null_many.full_many(pairs_dev, srs, stats=fs)

    # the ragged shift + FIR alone on the corpus' own rows and compensating delays
    xp = [b for _, b in pairs_dev]
    comp = [-(o[2] * sr / 1000.0) for o, sr in zip(outs["device_packed"], srs)]
    n_outs = [a.shape[1] for a, _ in pairs_dev]
    del outs
    fir = {}
    for taps in (64, 255):
        null_many.shift_fir_many(xp, comp, taps, n_outs)
        fir[str(taps)] = stats_of([timed(lambda: null_many.shift_fir_many(xp, comp, taps, n_outs))[0] for _ in range(args.runs)])

    ts = {k: [] for k in sides}
    for _ in range(args.runs):
        for k, f in sides.items():
            ts[k].append(timed(f)[0])
    P = len(pairs)
    res = dict(arch=arch, device=torch.cuda.get_device_name(0), pairs=P, audio_seconds=sum(x.shape[1] / sr for x, sr in clips),
               widgets=dict(align_max_shift_ms=200, fractional=True, fir_len=64, match_mode="LUFS-I", n_fft=2048, hop=512), runs=args.runs,
               agreement=dict(host=a_host, device=a_dev), delay_recovery_samples=dict(median=statistics.median(recovered), worst=max(recovered)),
               wave_budget_GB=4.0, packed_stats=fs,
               # read from align_stage / gain_stage / null_stage at these widgets: 2 mono_mean, gcc_phat (pack, 3 passes, peak), shift_fir,
               # 3 x (kweight + frame_meansq), eltwise, null_mix, pair_stats, 2 stft_mag + lsd_frames + sum_f64 + order_stats2: 19 library
               # calls = 22 kernel launches (and 3 memsets); blocking reads: the lag, 3 levels, null_mix, pair_stats, and the LSD's two
               loop_counts=dict(library_calls=19 * P, launches=22 * P, host_reads=8 * P),
               transform_lengths=lengths, plan_creation=dict(cold_delays_many_seconds=cold, warm_delays_many_seconds=warm,
                                                              groups=st.get("transform_groups"), seconds_per_length=(cold - warm) / max(1, len(lengths))),
               shift_fir=fir, **{k: stats_of(v) for k, v in ts.items()})
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    return 0 if (a_host["ok"] and a_dev["ok"]) else 1


if __name__ == "__main__":
    sys.exit(main())
