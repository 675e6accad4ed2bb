#!/usr/bin/env python3
"""Stand-alone timing of the native DeepFilterNet3 forward pass (csrc/egr_dfn3.hip) on one MI355X.

Prints one JSON line: xRT (seconds of audio per second of wall time) for 60 s and 30 min of 48 kHz stereo, and the recurrence
kernel's time per step for every GRU layer (k_dfn_gru alone, two channels = two workgroups, events around one launch).
  python tools/dfn3_timing.py [--model-dir DIR] [--skip-long]
Without --model-dir a discovered DeepFilterNet3 directory is used, else a synthetic one (DeepFilterNet3-default config, random
weights: the timing does not depend on the weight values).
"""
import argparse
import json
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
    a = ap.parse_args()
    import torch
    from packload import load_pack
    load_pack()
    from egregora_amd import dfn_engine, dfn_weights, native
    native.require_device()
    d = Path(a.model_dir) if a.model_dir else dfn_weights.discover()
    tmp = None
    if d is None:
        import dfn3_torch
        tmp = tempfile.TemporaryDirectory()
        d = Path(tmp.name) / "DeepFilterNet3"
        dfn3_torch.write_model_dir(d, seed=0)
    eng = dfn_engine.Dfn3Engine(dfn_weights.load(d), torch.cuda.current_device())
    L = native.lib()
    out = {"model_dir": "synthetic" if tmp else str(d)}
    g = torch.Generator(device="cuda").manual_seed(0)
    for name, secs, reps in (("60s_stereo", 60, a.reps), ("30min_stereo", 1800, 1)):
        if a.skip_long and secs > 60:
            continue
        n = secs * 48000
        out[f"{name}_workspace_GB"] = round(L.egr_dfn3_workspace_bytes(eng.h, 2, n) / 1e9, 2)
        x = 0.1 * torch.randn(2, n, device="cuda", generator=g)
        eng.enhance(x[:, :48000].contiguous())            # warm-up (workspace, code objects)
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
    n_gru = eng.model.cfg["emb_num_layers"] + eng.model.cfg["df_num_layers"]          # encoder 1 + ERB decoder (emb - 1) + DF decoder
    out["gru_us_per_step"] = [round(eng.time_gru(layer, 2, 20000), 3) for layer in range(n_gru)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
