"""Corpus timing of the DeepFilterNet batch path (profiles/dfn_batch.md): the seeded corpus of tools/flashsr_batch_timing.py (clips of
2-12 s at 16, 24, 44.1 and 48 kHz, mono and stereo) through the synthetic default model of each network, one process, one GPU:
  engine  -- one clip per DfnEngine.enhance call against DfnEngine.enhance_many, on the clips' 48 kHz device tensors,
  node    -- Egregora_DeepFilterNet_Denoise.execute once per clip against the batch node on the whole list (host in, host out),
  vad_mix -- the per-clip egr_dfn_vad_gains / egr_dfn_mix calls of the packed path alone (their share of the packed node time).
The two paths of a pair ALTERNATE inside every round (one warm-up round, then `--runs` timed rounds); a host clock around work that
ends with a device synchronisation (the per-clip loop is bound by the host's launches, which events on the stream would not see);
the figure is the median with the spread of the rounds.  Packed and per-clip results are compared with torch.equal before any figure
is reported.  Next to the measured ratio stands the one the recurrences alone predict from egr_dfn*_time_gru's time per step:
sum over clips of layers x frames x step time, against waves x layers x frames of the wave's longest clip x step time.

usage: python tools/dfn_batch_timing.py [--clips 200] [--runs 5] [--models DeepFilterNet3,DeepFilterNet2] [--skip-node] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))


def stats_of(ts):
    return dict(seconds_median=statistics.median(ts), seconds_min=min(ts), seconds_max=max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=200)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--models", default="DeepFilterNet3,DeepFilterNet2")
    ap.add_argument("--skip-node", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from packload import load_pack
    pack = load_pack()
    import dfn2_torch
    import dfn3_torch
    from flashsr_batch_timing import corpus
    from egregora_amd import dfn2_engine, dfn_engine, dfn_many, egregora_audio_enhance_dfn_batch as B, native, resample
    from egregora_amd import egregora_audio_enhance_extras as X
    native.require_device()
    clips = corpus(args.clips, 7, torch)
    audio_s = sum(x.shape[1] / sr for x, sr in clips)
    sync = torch.cuda.synchronize
    x48 = [resample.resample_hq(x.cuda(), sr, 48000).contiguous() for x, sr in clips]
    res = dict(clips=len(clips), audio_seconds=audio_s, tracks=sum(x.shape[0] for x in x48), models={})
    tmp = tempfile.TemporaryDirectory()
    single = pack.NODE_CLASS_MAPPINGS["Egregora_DeepFilterNet_Denoise"]()
    batch = B.Egregora_DeepFilterNet_DenoiseBatch()
    for model in args.models.split(","):
        d = Path(tmp.name) / model
        if model == "DeepFilterNet3":
            dfn3_torch.write_model_dir(d, seed=0)
            eng = dfn_engine.engine(d)
        else:
            dfn2_torch.write_model_dir(d, seed=0)
            eng = dfn2_engine.engine(d)
        os.environ["EGREGORA_DFN_MODEL_DIR"] = str(d)
        frames = [eng.frames_of(x.shape[1]) for x in x48]
        out = dict(frames=sum(f * x.shape[0] for f, x in zip(frames, x48)))

        def per_clip():
            sync()
            t0 = time.perf_counter()
            ys = [eng.enhance(x) for x in x48]
            sync()
            return time.perf_counter() - t0, ys

        def packed():
            st = {}
            sync()
            t0 = time.perf_counter()
            ys = eng.enhance_many(x48, stats=st)
            sync()
            return time.perf_counter() - t0, ys, st

        _, ya = per_clip()
        _, yb, st = packed()
        assert all(torch.equal(a, b) for a, b in zip(ya, yb)), "packed and per-clip outputs differ"
        del ya, yb
        ta, tb = [], []
        for r in range(args.runs):
            ta.append(per_clip()[0])
            tb.append(packed()[0])
            print(f"[{model}] engine round {r}: per-clip {ta[-1]:.3f} s, packed {tb[-1]:.3f} s", flush=True)
        n_gru = eng.model.cfg["emb_num_layers"] + eng.model.cfg["df_num_layers"]
        step_us = [eng.time_gru(layer, 2, 20000) for layer in range(n_gru)]
        rec_clip = sum(step_us) * 1e-6 * sum(frames)
        rec_packed = sum(step_us) * 1e-6 * sum(max(frames[i] for i in w) for w in st["waves"])
        out["engine"] = dict(per_clip=stats_of(ta), packed=stats_of(tb), speedup=statistics.median(ta) / statistics.median(tb),
                             waves=len(st["waves"]), alone=len(st["alone"]), clips_per_wave=[len(w) for w in st["waves"]],
                             workspace_held_GB=eng.workspace_held() / 1e9, gru_us_per_step=step_us,
                             recurrence_seconds_per_clip_predicted=rec_clip, recurrence_seconds_packed_predicted=rec_packed,
                             recurrence_ratio_predicted=rec_clip / rec_packed)
        if not args.skip_node:
            def node_loop():
                t0 = time.perf_counter()
                ys = [single.execute({"waveform": x[None], "sample_rate": sr}, model)[0]["waveform"][0] for x, sr in clips]
                return time.perf_counter() - t0, ys

            def node_batch():
                t0 = time.perf_counter()
                (outs,) = batch.execute(audio=[{"waveform": x[None], "sample_rate": sr} for x, sr in clips], dfn_model=[model])
                return time.perf_counter() - t0, [o["waveform"][0] for o in outs]

            _, ya = node_loop()
            _, yb = node_batch()
            assert all(torch.equal(a, b) for a, b in zip(ya, yb)), "batch node and single node outputs differ"
            del ya, yb
            ta, tb = [], []
            for r in range(args.runs):
                ta.append(node_loop()[0])
                tb.append(node_batch()[0])
                print(f"[{model}] node round {r}: single node {ta[-1]:.3f} s, batch node {tb[-1]:.3f} s", flush=True)
            # the per-clip VAD gains + mix calls of the packed path, alone
            dry = [x.cuda() for x, _ in clips]
            tm = []
            for r in range(args.runs + 1):
                sync()
                t0 = time.perf_counter()
                for d_, d48, (_, sr) in zip(dry, x48, clips):
                    X.mix_on_device(d_, d_, d48, sr, 0.65, "equal_power", "more_on_noise", 0.45, 0.90, 60, 0.5, True, 0.98)
                sync()
                tm.append(time.perf_counter() - t0)
            tm = tm[1:]
            out["node"] = dict(single_loop=stats_of(ta), batch=stats_of(tb), speedup=statistics.median(ta) / statistics.median(tb),
                               vad_mix_per_clip_calls=stats_of(tm), vad_mix_share_of_batch=statistics.median(tm) / statistics.median(tb))
        res["models"][model] = out
        print(json.dumps({model: out}), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
