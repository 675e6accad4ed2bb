"""Corpus timing of the Fat-Llama many-clip path (profiles/fatllama_batch.md): the seeded corpus of tools/flashsr_batch_timing.py
(corpus(200, 7): clips of 2-12 s, mono and stereo), each clip at the length FlashSR returns it (48 kHz), through the node's default
widgets at 800 iterations, one process per run, one GPU:
  --mode single -- one EgregoraFatLlamaGPU call per clip (fatllama_engine.node_run; plans come and go in its LRU of 8),
  --mode packed -- fatllama_many.enhance_many over the whole corpus (wave creation included).
A run is one fresh process: a warm-up call on a 0.1 s clip (library load, HIP start-up), then a host clock around the corpus that ends
with a device synchronisation; the clips are on the device before the clock starts and the results stay there on both sides
(enhance_many's one download is inside its clock).  The reference side is meant to run on the parent commit's library
(EGREGORA_AMD_LIB), the runs of the two sides alternating; every run appends one JSON line to --out.

usage: [EGREGORA_AMD_LIB=parent.so] python tools/fatllama_batch_timing.py --mode {single,packed} [--clips 200] [--iters 800] --out FILE.jsonl
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))


def corpus48(n, seed, torch):
    """The FlashSR corpus at the stage's output: every clip at 48 kHz, its duration kept."""
    from flashsr_batch_timing import corpus
    g = torch.Generator().manual_seed(seed + 1)
    return [(0.1 * torch.randn(x.shape[0], int(round(x.shape[1] * 48000.0 / sr)), generator=g), 48000) for x, sr in corpus(n, seed, torch)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", required=True, choices=["single", "packed"])
    ap.add_argument("--clips", type=int, default=200)
    ap.add_argument("--iters", type=int, default=800)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import os
    import torch
    from packload import load_pack
    load_pack()
    from egregora_amd import fatllama_engine as fe
    clips = [(x.cuda(), sr) for x, sr in corpus48(args.clips, 7, torch)]
    widgets = (args.iters, 0.6, 1411, True, True)          # max_iterations, threshold_value, target_bitrate_kbps, normalize, autoscale
    fe.node_run(torch.zeros(2, 4801), 48000, 3, *widgets[1:])
    fe.release_plans()
    torch.cuda.synchronize()
    rec = {"mode": args.mode, "lib": os.environ.get("EGREGORA_AMD_LIB", "tree"), "clips": len(clips), "iters": args.iters,
           "audio_s": sum(x.shape[1] / sr for x, sr in clips), "rows": sum(x.shape[0] for x, _ in clips)}
    if args.mode == "single":          # (nothing but fatllama_engine: this mode also runs from a checkout without the many-clip path)
        t0 = time.perf_counter()
        keep = [fe.node_run(x, sr, *widgets)[0] for x, sr in clips]
        torch.cuda.synchronize()
        rec["seconds"] = time.perf_counter() - t0
    else:
        from egregora_amd import fatllama_many as fm
        stats = {}
        t0 = time.perf_counter()
        keep = fm.enhance_many(clips, *widgets, stats=stats)
        torch.cuda.synchronize()
        rec["seconds"] = time.perf_counter() - t0
        rec.update(waves=stats["waves"], wave_rows=stats["rows"], padding=stats["padding"], fallbacks=stats["fallbacks"])
        # launches of the loop per direction: 4 per iteration and pipeline; a clip alone runs min(2, states) pipelines, a wave 2
        specs = [(x.shape[1], fm._request(x, sr, widgets[2])[0], 0, x.shape[0]) for x, sr in clips]
        kinds = [fm.query([s])["clips"][0]["kind"] for s in specs]
        states = [(s[3] + 1) // 2 if k == 2 else s[3] for s, k in zip(specs, kinds)]
        rec["loop_launches_single"] = sum(4 * args.iters * min(2, k) for k in states)
        in_waves = {i for w in stats["wave_clips"] for i in w}
        rec["loop_launches_packed"] = 4 * args.iters * 2 * stats["waves"] + sum(4 * args.iters * min(2, k) for i, k in enumerate(states) if i not in in_waves)
    del keep
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
