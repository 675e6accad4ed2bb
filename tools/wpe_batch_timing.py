"""Corpus timing of the WPE many-clip path (profiles/wpe_batch.md): the seeded corpus of tools/flashsr_batch_timing.py (200 clips of
2-12 s at 16, 24, 44.1 and 48 kHz, mono and stereo) at the node's default widgets (taps 10, delay 3, 3 iterations, n_fft 1024, hop 256),
one process, one GPU:
  node loop -- one Egregora_WPE_Dereverb.execute per clip, host tensor in, host tensor out (the only path before the many-clip call),
  packed    -- wpe_many.dereverb_many on the same host tensors (one egr_wpemany_dereverb per wave of plan_waves),
and, to separate the transfers from the launches, the same pair on tensors that already sit on the device:
  device loop   -- one wpe_engine.dereverb per clip,
  device packed -- wpe_engine.dereverb_many per wave of the same plan.
The sides ALTERNATE inside every round (one warm-up round, then --runs timed rounds); a host clock around work that ends with a device
synchronisation (the loops are bound by the host's launches and round trips, which events on the stream would not see); the figure is
the median with the min and max of the rounds.  Before the rounds the packed results are compared with the loop's, clip by clip
(torch.equal).  Library calls and launches are counted from the plan: a call is 2 + iterations launches whatever it holds.

usage: python tools/wpe_batch_timing.py [--clips 200] [--runs 5] [--out FILE.json]
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
    import torch
    from packload import load_pack
    load_pack()
    from flashsr_batch_timing import corpus
    from egregora_amd import egregora_audio_enhance_wpe as ew, native, wpe_engine, wpe_many
    arch = native.require_device()
    w = dict(wpe_many.WIDGET_DEFAULTS)
    cfg = dict(n_fft=w["n_fft"], hop=w["hop"], taps=w["taps"], delay=w["delay"], iterations=w["iterations"])
    clips = corpus(args.clips, 7, torch)
    node = ew.Egregora_WPE_Dereverb()
    sync = torch.cuda.synchronize
    waves, alone, wave_bytes = wpe_many.plan_waves([tuple(x.shape) for x, _ in clips], n_fft=cfg["n_fft"], hop=cfg["hop"], taps=cfg["taps"])
    xs_dev = [x.cuda().contiguous() for x, _ in clips]
    per_call = 2 + cfg["iterations"]

    def node_loop():
        return [node.execute({"waveform": x[None], "sample_rate": sr}, **w)[0]["waveform"][0] for x, sr in clips]

    def packed():
        return wpe_many.dereverb_many(clips, **w)

    def device_loop():
        return [wpe_engine.dereverb(x, **cfg) for x in xs_dev]

    def device_packed():
        out = [None] * len(xs_dev)
        for wave in waves:
            for i, y in zip(wave, wpe_engine.dereverb_many([xs_dev[i] for i in wave], **cfg)):
                out[i] = y
        for i in alone:
            out[i] = wpe_engine.dereverb(xs_dev[i], **cfg)
        return out

    def timed(f):
        sync()
        t0 = time.perf_counter()
        out = f()
        sync()
        return time.perf_counter() - t0, out

    sides = dict(node_loop=node_loop, packed=packed, device_loop=device_loop, device_packed=device_packed)
    # warm-up round, and the identity of the results
    outs = {k: timed(f)[1] for k, f in sides.items()}
    same = all(torch.equal(a, b) for a, b in zip(outs["node_loop"], outs["packed"])) and \
        all(torch.equal(a.cpu(), b) for a, b in zip(outs["device_packed"], outs["node_loop"])) and \
        all(torch.equal(a.cpu(), b) for a, b in zip(outs["device_loop"], outs["node_loop"]))
    del outs
    ts = {k: [] for k in sides}
    for _ in range(args.runs):
        for k, f in sides.items():
            ts[k].append(timed(f)[0])
    res = dict(arch=arch, device=torch.cuda.get_device_name(0), clips=len(clips), channel_rows=sum(x.shape[0] for x, _ in clips),
               audio_seconds=sum(x.shape[1] / sr for x, sr in clips), widgets=cfg, runs=args.runs, results_bit_equal=bool(same),
               waves=len(waves), alone=len(alone), wave_clips=[len(v) for v in waves], wave_bytes=wave_bytes,
               wave_budget_GB=wpe_many.DEFAULT_WAVE_GB,
               library_calls=dict(loop=len(clips), packed=len(waves) + len(alone)),
               launches=dict(loop=len(clips) * per_call, packed=(len(waves) + len(alone)) * per_call),
               **{k: stats_of(v) for k, v in ts.items()})
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
