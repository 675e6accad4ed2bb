#!/usr/bin/env python3
"""Stand-alone timing of the native DeepFilterNet2 forward pass (egr_dfn2_*, csrc/egr_dfn3.hip) on one MI355X.

Prints one JSON line and, with --out, writes it to a file (profiles/dfn2_timing.json): xRT (seconds of audio per second of wall time)
for 60 s and 30 min of 48 kHz stereo, the workspace per frame, every GroupedGRU layer's time per step, and the recurrence comparison
of DESIGN.md 7.2: egr_dfn2_time_gru on the default config's layers (H = 256, G = 8) against egr_dfn3_time_gru on a dense H = 256
DeepFilterNet3 layer, in one process, alternating, --reps repeats each (medians and their ratio), plus G = 1 and G = 16.
  python tools/dfn2_timing.py [--model-dir DIR] [--skip-long] [--pass-only] [--out profiles/dfn2_timing.json]
Without --model-dir a discovered DeepFilterNet2 directory is used, else a synthetic one (the recalled DeepFilterNet2 default config,
random weights: the timing does not depend on the weight values).
"""
import argparse
import datetime
import json
import platform
import statistics
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model-dir", default=None)
    ap.add_argument("--skip-long", action="store_true", help="no 30 min run")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20000, help="recurrence steps per time_gru launch")
    ap.add_argument("--out", default=None)
    ap.add_argument("--pass-only", action="store_true", help="only the 60 s stereo pass (a profiler run of its own)")
    a = ap.parse_args()
    import torch
    from packload import load_pack
    load_pack()
    from egregora_amd import dfn2_engine, dfn2_weights, dfn_engine, dfn_weights, native
    import dfn2_torch
    import dfn3_torch
    arch = native.require_device()
    tmp = tempfile.TemporaryDirectory()
    d = Path(a.model_dir) if a.model_dir else dfn2_weights.discover()
    synthetic = d is None
    if synthetic:
        d = Path(tmp.name) / "DeepFilterNet2"
        dfn2_torch.write_model_dir(d, seed=0)
    dev = torch.cuda.current_device()
    eng = dfn2_engine.Dfn2Engine(dfn2_weights.load(d), dev)
    cfg = eng.model.cfg
    out = {"model_dir": "synthetic" if synthetic else str(d), "box": f"{platform.node()} {arch} {torch.cuda.get_device_name(dev)}",
           "date": datetime.datetime.now().isoformat(timespec="seconds"),
           "config": {k: cfg[k] for k in ("fft_size", "hop_size", "emb_hidden_dim", "df_hidden_dim", "gru_groups", "lin_groups",
                                          "emb_num_layers", "df_num_layers")}}
    g = torch.Generator(device="cuda").manual_seed(0)
    for name, secs, reps in (("60s_stereo", 60, a.reps), ("30min_stereo", 1800, 1)):
        if (a.skip_long or a.pass_only) and secs > 60:
            continue
        n = secs * 48000
        nF = (n + cfg["fft_size"]) // cfg["hop_size"]
        ws = eng.workspace_bytes(2, n)
        out[f"{name}_workspace_GB"] = round(ws / 1e9, 3)
        out[f"{name}_workspace_bytes_per_channel_frame"] = round(ws / (2 * nF))
        x = 0.1 * torch.randn(2, n, device="cuda", generator=g)
        eng.enhance(x[:, :48000].contiguous())
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            y = eng.enhance(x)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        assert bool(torch.isfinite(y).all())
        out[f"{name}_s"] = round(min(ts), 4)
        out[f"{name}_xRT"] = round(secs / min(ts), 1)
        del x, y
        torch.cuda.empty_cache()
    if a.pass_only:
        print(json.dumps(out))
        return
    n_gru = cfg["emb_num_layers"] + cfg["df_num_layers"]
    out["gru_us_per_step"] = [round(eng.time_gru(layer, 2, a.steps), 3) for layer in range(n_gru)]

    # the recurrence comparison: grouped (this config's encoder layer) against DeepFilterNet3's dense H = 256 layer, alternating
    d3 = Path(tmp.name) / "DeepFilterNet3"
    dfn3_torch.write_model_dir(d3, seed=0)                     # DeepFilterNet3 default: emb_hidden_dim = 256
    eng3 = dfn_engine.Dfn3Engine(dfn_weights.load(d3), dev)
    grouped, dense = [], []
    for _ in range(a.reps):
        grouped.append(eng.time_gru(1, 2, a.steps))            # the ERB decoder's first layer: H -> H, G groups
        dense.append(eng3.time_gru(1, 2, a.steps))
    mg, md = statistics.median(grouped), statistics.median(dense)
    out["recurrence"] = {"steps": a.steps, "channels": 2, "H": cfg["emb_hidden_dim"], "G": cfg["gru_groups"],
                         "grouped_us_per_step": [round(v, 3) for v in grouped], "dense_us_per_step": [round(v, 3) for v in dense],
                         "grouped_median": round(mg, 3), "dense_median": round(md, 3), "ratio_grouped_over_dense": round(mg / md, 3)}
    for G in (1, 16):
        dg = Path(tmp.name) / f"G{G}" / "DeepFilterNet2"
        dfn2_torch.write_model_dir(dg, seed=0, cfg_text=dfn2_torch.config_text(gru_groups=G))
        e = dfn2_engine.Dfn2Engine(dfn2_weights.load(dg), dev)
        out["recurrence"][f"G{G}_median"] = round(statistics.median(e.time_gru(1, 2, a.steps) for _ in range(a.reps)), 3)
        del e
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
