"""Corpus timing of the Descript Audio Codec's many-clip path (profiles/dac_batch.md): the seeded corpus of tools/flashsr_batch_timing.py
(clips of 2-12 s at 16, 24, 44.1 and 48 kHz, mono and stereo) through tools/dac_timing.py's synthetic model of the 44 kHz default size,
one process, one GPU, on the clips' 44.1 kHz device tensors:
  per clip -- one DacEngine.encode / decode call per clip (the only path before the many calls),
  packed   -- DacEngine.encode_many / decode_many (one egr_dacmany_encode / _decode per wave of plan_waves).
The two paths ALTERNATE inside every round (one warm-up round, then `--runs` timed rounds); a host clock around work that ends with a
device synchronisation (the per-clip loop is bound by the host's launches, which events on the stream would not see); the figure is the
median with the spread of the rounds.  The packed pass is also timed at MAX_PAD_SHARE in --shares, with the padding share
1 - sum(frames) / sum(rows x pad_frames) each leaves.  Library calls are counted; launches per call are counted from the layer list (a
contraction counts once: split-K adds a reduction launch where the launcher chooses it).  Kernel shares come from a run of its own:
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o dac_many -- python tools/dac_batch_timing.py --runs 1 --packed-only

usage: python tools/dac_batch_timing.py [--clips 200] [--runs 5] [--shares 0.02,0.05,0.1,0.25,0.5] [--packed-only] [--out FILE.json]
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
sys.path.insert(0, str(ROOT / "tools"))


def stats_of(ts):
    return dict(seconds_median=statistics.median(ts), seconds_min=min(ts), seconds_max=max(ts))


def launches_per_call(cfg, kind):
    """Kernel and memset launches of one walk: units are 2 snakes + 2 contractions, a block adds a snake and its strided convolution
    (encode) or a snake, a GEMM and the gather (decode)."""
    n = len(cfg["encoder_rates"] if kind == 0 else cfg["decoder_rates"])
    if kind == 0:
        return 1 + 1 + n * (3 * 4 + 2) + 2 + 1 + 1          # memset, conv_in, blocks, snake + out conv, quantiser, transpose
    return 1 + 1 + 1 + 1 + n * (3 + 3 * 4) + 1 + 1          # memset, transpose, absmax, in conv, blocks, snake, conv_out


def pad_share(waves, frames, rows):
    used = sum(frames[i] * rows[i] for w in waves for i in w.clips)
    cells = sum(w.rows * w.pad_frames for w in waves)
    return 1.0 - used / cells if cells else 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=200)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--shares", default="0.02,0.05,0.1,0.25,0.5")
    ap.add_argument("--packed-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from packload import load_pack
    load_pack()
    import dac_torch as R
    from flashsr_batch_timing import corpus
    from egregora_amd import dac_engine as E, dac_weights, native, resample
    arch = native.require_device()
    cfg = R.config("W")
    eng = E.DacEngine(dac_weights.DacModel(cfg, R.synthetic_state_dict(cfg, 17)), torch.cuda.current_device())
    sr_model = cfg["sample_rate"]
    clips = corpus(args.clips, 7, torch)
    xs = [(x.cuda() if sr == sr_model else resample.resample_hq(x.cuda(), sr, sr_model)).contiguous() for x, sr in clips]
    rows = [x.shape[0] for x in xs]
    frames = [eng.lengths(x.shape[1])[1] for x in xs]
    sync = torch.cuda.synchronize
    res = dict(arch=arch, device=torch.cuda.get_device_name(0), clips=len(xs), rows=sum(rows), audio_seconds=sum(x.shape[1] / sr for x, sr in clips),
               row_frames=sum(f * r for f, r in zip(frames, rows)), model="synthetic, 44 kHz default size", runs=args.runs,
               default_max_pad_share=E.MAX_PAD_SHARE, workspace_budget_GB=E.workspace_budget_gb())

    def per_clip_encode():
        sync()
        t0 = time.perf_counter()
        out = [eng.encode(x) for x in xs]
        sync()
        return time.perf_counter() - t0, out

    def packed_encode():
        st = {}
        sync()
        t0 = time.perf_counter()
        out = eng.encode_many(xs, stats=st)
        sync()
        return time.perf_counter() - t0, out, st

    _, enc, st_e = packed_encode()
    zs = [z for z, _ in enc]

    def per_clip_decode():
        sync()
        t0 = time.perf_counter()
        out = [eng.decode(z) for z in zs]
        sync()
        return time.perf_counter() - t0, out

    def packed_decode():
        st = {}
        sync()
        t0 = time.perf_counter()
        out = eng.decode_many(zs, stats=st)
        sync()
        return time.perf_counter() - t0, out, st

    _, ys, st_d = packed_decode()
    if not args.packed_only:
        # the two paths agree to fp32 round-off (not bit for bit: the launcher chooses tiles from the padded shape)
        _, enc1 = per_clip_encode()
        _, ys1 = per_clip_decode()
        agree = sum(float((a[1] == b[1]).double().mean()) * a[1].shape[-1] for a, b in zip(enc, enc1)) / sum(frames)
        ydiff = max(float((a - b).norm() / b.norm()) for a, b in zip(ys, ys1))
        res["packed_vs_per_clip"] = dict(code_agreement=agree, decode_rel_l2_max=ydiff)
        print(f"packed against per clip: codes equal on {agree:.4%} of the frames, decode rel L2 at most {ydiff:.2e}", flush=True)
        del enc1, ys1
    del enc, ys
    for name, kind, a_fn, b_fn, st in (("encode", 0, per_clip_encode, packed_encode, st_e), ("decode", 1, per_clip_decode, packed_decode, st_d)):
        ta, tb = [], []
        for r in range(args.runs):
            if not args.packed_only:
                ta.append(a_fn()[0])
            tb.append(b_fn()[0])
            print(f"[{name}] round {r}: per clip {ta[-1] if ta else float('nan'):.3f} s, packed {tb[-1]:.3f} s", flush=True)
        w = st["waves"]
        per = launches_per_call(cfg, kind)
        out = dict(packed=stats_of(tb), waves=len(w), alone=len(st["alone"]), clips_per_wave=[len(v.clips) for v in w], rows_per_wave=[v.rows for v in w],
                   pad_frames_per_wave=[v.pad_frames for v in w], padding_share=pad_share(w, frames, rows), launches_per_call=per,
                   library_calls=dict(per_clip=len(xs), packed=len(w) + len(st["alone"])),
                   launches=dict(per_clip=per * len(xs), packed=per * (len(w) + len(st["alone"]))))
        if ta:
            out.update(per_clip=stats_of(ta), speedup=statistics.median(ta) / statistics.median(tb))
        res[name] = out
    res["workspace_held_GB"] = eng.workspace_held() / 1e9
    sweep = {}
    for s in [float(v) for v in args.shares.split(",") if v]:
        E.MAX_PAD_SHARE = s
        rec = {}
        for name, fn in (("encode", packed_encode), ("decode", packed_decode)):
            fn()
            ts, st = [], None
            for _ in range(args.runs):
                t, _, st = fn()
                ts.append(t)
            rec[name] = dict(stats_of(ts), waves=len(st["waves"]), padding_share=pad_share(st["waves"], frames, rows))
        sweep[str(s)] = rec
        print(f"MAX_PAD_SHARE {s}: " + json.dumps(rec), flush=True)
    res["max_pad_share_sweep"] = sweep
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main()
