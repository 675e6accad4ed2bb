"""Corpus timing of FlashSR's packed path (profiles/flashsr_batch.md): a seeded corpus of short clips through
  per-clip -- the single node, EgregoraAudioUpscaler.run once per clip (host AUDIO dict in, host AUDIO dict out), and
  packed   -- flashsr_engine.upscale_many on the whole list (host tensors in, host tensors out),
full-size synthetic weights, one process, one GPU.  The two paths ALTERNATE inside every round (one warm-up round, then `--runs`
timed rounds; a host clock around work that ends with its results on the host); the figure is the median, with the spread of the
rounds.  Both are repeated on an engine built under EGREGORA_FLASHSR_SPLIT=f16x1 (the fast mode).  The first timed-size results of
the two paths are compared clip by clip (relative L2) before any figure is reported.

usage: python tools/flashsr_batch_timing.py [--clips 200] [--runs 5] [--max-rows N] [--modes f16x2,f16x1] [--out FILE.json]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

RATES = (16000, 24000, 44100, 48000)


def corpus(n, seed, torch):
    """n clips of 2-12 s at 16, 24, 44.1 and 48 kHz, mono and stereo: low-passed noise bursts at speech-like level."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(n):
        sr = RATES[int(torch.randint(0, len(RATES), (1,), generator=g))]
        ch = 1 + int(torch.randint(0, 2, (1,), generator=g))
        secs = 2.0 + 10.0 * float(torch.rand(1, generator=g))
        out.append((0.1 * torch.randn(ch, int(secs * sr), generator=g), sr))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=200)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--max-rows", type=int, default=None)
    ap.add_argument("--modes", default="f16x2,f16x1")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from packload import load_pack
    pack = load_pack()
    from egregora_amd import flashsr_arch as A, flashsr_engine as E
    clips = corpus(args.clips, 7, torch)
    audio_s = sum(x.shape[1] / sr for x, sr in clips)
    node = pack.NODE_CLASS_MAPPINGS["EgregoraAudioUpscaler"]()
    cfg = A.FlashSRConfig()
    P = A.init_params(cfg, 0)
    res = dict(clips=len(clips), audio_seconds=audio_s, rows=sum(E.clip_rows(x.shape[0], x.shape[1], sr, cfg.chunk, E.audio_glue.HOP_SAMPLES)
                                                               for x, sr in clips),
               rows_per_pass=E.ROWS_PER_PASS, wave_budget=E.wave_budget(args.max_rows), modes={})
    for mode in args.modes.split(","):
        E.FlashSREngine.SPLIT = mode                     # what EGREGORA_FLASHSR_SPLIT sets: frozen per engine at construction
        eng = E.FlashSREngine(cfg, P)
        E.set_engine(eng)
        eng.warmup(2)

        def per_clip():
            t0 = time.perf_counter()
            ys = [node.run(audio={"waveform": x[None], "sample_rate": sr}, lowpass_input=False, output_sr="48000")[0]["waveform"][0]
                  for x, sr in clips]
            return time.perf_counter() - t0, ys

        def packed():
            st = {}
            t0 = time.perf_counter()
            ys = E.upscale_many(clips, False, 48000, max_rows=args.max_rows, stats=st)
            return time.perf_counter() - t0, ys, st

        _, ya = per_clip()                               # warm-up round: every shape both paths use
        _, yb, st = packed()
        rel = max(float((b.double() - a.double()).norm() / a.double().norm()) for a, b in zip(ya, yb))
        print(f"[{mode}] warm-up done; packed vs per-clip worst relative L2 over {len(clips)} clips: {rel:.3e}", flush=True)
        ta, tb = [], []
        for r in range(args.runs):
            ta.append(per_clip()[0])
            tb.append(packed()[0])
            print(f"[{mode}] round {r}: per-clip {ta[-1]:.3f} s, packed {tb[-1]:.3f} s", flush=True)
        calls_a = sum(3 + (sr != 48000) for _, sr in clips)          # gather + infer + WOLA (+ resample) per clip
        row = lambda t, calls: dict(seconds_median=statistics.median(t), seconds_min=min(t), seconds_max=max(t),
                                    clips_per_s=len(clips) / statistics.median(t), audio_seconds_per_s=audio_s / statistics.median(t),
                                    library_calls=calls)
        res["modes"][mode] = dict(per_clip=row(ta, calls_a), packed=row(tb, sum(st["library_calls"])), waves=len(st["waves"]),
                                  rows_per_wave=st["rows"], worst_rel_l2_packed_vs_per_clip=rel,
                                  speedup=statistics.median(ta) / statistics.median(tb))
        print(json.dumps({mode: res["modes"][mode]}), flush=True)
        E.set_engine(None)
        eng.close()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
