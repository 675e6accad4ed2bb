#!/usr/bin/env python3
"""Timing and identity record of the segmented DeepFilterNet pass (profiles/dfn_segmented.md) on one MI355X.

  python tools/dfn_segmented_timing.py --run LABEL --lines FILE [--root CHECKOUT]
      one process, one measurement of each kind, appended to FILE as one JSON line tagged LABEL: for the synthetic default model of
      both networks the wall time of 60 s of 48 kHz stereo in one pass and (where the checkout has the segmented call) in segments of
      1024, 4096 and 16384 frames, the workspace the handle holds after each, egr_dfn*_time_gru per step, and the SHA-256 of the
      one-pass and of the segmented output of one fixed second of stereo.  --root names another checkout of this repository (its
      Python package and its built library are used): the parent commit, to alternate with this tree.
  python tools/dfn_segmented_timing.py --summarise FILE --out profiles/dfn_segmented.json
      medians, minima and maxima per label, the ratios against the label `parent`, and the identity verdicts.
"""
import argparse
import hashlib
import json
import platform
import statistics
import sys
import tempfile
import time
from pathlib import Path

SEGMENTS = (1024, 4096, 16384)


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def run(label, root, lines):
    sys.path.insert(0, str(root))
    sys.path.insert(0, str(root / "tests"))
    import torch
    from packload import load_pack
    load_pack()
    from egregora_amd import dfn2_engine, dfn2_weights, dfn_engine, dfn_weights, native
    import dfn2_torch
    import dfn3_torch
    from dfn3_check import speechy
    arch = native.require_device()
    dev = torch.cuda.current_device()
    tmp = tempfile.TemporaryDirectory()
    out = {"label": label, "box": f"{platform.node()} {arch} {torch.cuda.get_device_name(dev)}"}
    g = torch.Generator(device="cuda").manual_seed(0)
    n = 60 * 48000
    x = 0.1 * torch.randn(2, n, device="cuda", generator=g)
    x1 = speechy(1, 48000, 2).cuda()
    for name, R, W, E in (("dfn3", dfn3_torch, dfn_weights, dfn_engine.Dfn3Engine), ("dfn2", dfn2_torch, dfn2_weights, dfn2_engine.Dfn2Engine)):
        d = Path(tmp.name) / name / ("DeepFilterNet3" if name == "dfn3" else "DeepFilterNet2")
        R.write_model_dir(d, seed=0)
        segmented = hasattr(E, "segment_workspace_bytes")
        r = {"one_pass_workspace_bytes": None, "sha_1s_one_pass": None}

        def timed(eng, **kw):
            eng.enhance(x1, **kw)                               # warm-up: the kernels' first launch
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            y = eng.enhance(x, **kw)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert bool(torch.isfinite(y).all())
            return dt, sha(y)

        eng = E(W.load(d), dev)
        r["sha_1s_one_pass"] = sha(eng.enhance(x1))
        r["one_pass_s"], r["sha_60s_one_pass"] = timed(eng)
        r["one_pass_workspace_bytes"] = eng.workspace_bytes(2, n)
        cfg = eng.model.cfg
        n_gru = cfg["emb_num_layers"] + cfg["df_num_layers"]
        r["gru_us_per_step"] = [round(eng.time_gru(layer, 2, 20000), 3) for layer in range(n_gru)]
        del eng
        torch.cuda.empty_cache()
        if segmented:
            for s in SEGMENTS:
                eng = E(W.load(d), dev)                         # a fresh handle: what it holds afterwards is this call's workspace
                r[f"seg{s}_sha_1s"] = sha(eng.enhance(x1, seg_frames=7))
                r[f"seg{s}_s"], r[f"seg{s}_sha_60s"] = timed(eng, seg_frames=s)
                r[f"seg{s}_workspace_bytes"] = eng.workspace_held()
                del eng
                torch.cuda.empty_cache()
        out[name] = r
    with open(lines, "a") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out))


def summarise(lines, dst):
    rows = [json.loads(ln) for ln in Path(lines).read_text().splitlines() if ln.strip()]
    labels = sorted({r["label"] for r in rows})
    res = {"box": rows[0]["box"], "runs_per_label": {lb: sum(r["label"] == lb for r in rows) for lb in labels}}
    for m in ("dfn3", "dfn2"):
        o = {}
        for lb in labels:
            rs = [r[m] for r in rows if r["label"] == lb]
            for key in sorted({k for r in rs for k in r if k.endswith("_s")}):
                v = [r[key] for r in rs if key in r]
                o[f"{lb}.{key}"] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
            o[f"{lb}.gru_us_per_step_median"] = [round(statistics.median(c), 3) for c in zip(*(r["gru_us_per_step"] for r in rs))]
            for key in sorted({k for r in rs for k in r if k.endswith("workspace_bytes")}):
                o[f"{lb}.{key}"] = rs[0][key]
        shas1 = {r[m][k] for r in rows for k in r[m] if k.endswith("sha_1s") or k == "sha_1s_one_pass"}
        shas60 = {r[m][k] for r in rows for k in r[m] if k.endswith("sha_60s") or k == "sha_60s_one_pass"}
        o["identical_bits_1s_every_label_and_path"] = len(shas1) == 1
        o["identical_bits_60s_every_label_and_path"] = len(shas60) == 1
        if "parent" in labels and "this" in labels:
            p = o["parent.one_pass_s"]
            o["one_pass_median_within_parent_spread"] = p["min"] <= o["this.one_pass_s"]["median"] <= p["max"]
            for key in ["one_pass_s"] + [f"seg{s}_s" for s in SEGMENTS]:
                if f"this.{key}" in o:
                    o[f"ratio_this_{key}_over_parent_one_pass"] = round(o[f"this.{key}"]["median"] / p["median"], 3)
        res[m] = o
    Path(dst).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", default=None)
    ap.add_argument("--root", default=str(Path(__file__).resolve().parents[1]))
    ap.add_argument("--lines", default=None)
    ap.add_argument("--summarise", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.summarise:
        summarise(a.summarise, a.out)
    else:
        run(a.run, Path(a.root).resolve(), a.lines)


if __name__ == "__main__":
    main()
