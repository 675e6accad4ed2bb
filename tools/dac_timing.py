#!/usr/bin/env python3
"""Time of the native Descript Audio Codec on one MI355X (profiles/dac.md, profiles/dac_timing.json).

  python tools/dac_timing.py [--seconds 60] [--repeats 20] [--out FILE.json]
  python tools/dac_timing.py --kernels          # host only: the contraction kernel the launcher picks per layer class
  python tools/dac_timing.py --seg-frames 64,256,1024,F [--rows 1]      # the same input in segments (profiles/dac_segmented.md)
  python tools/dac_timing.py --seconds 600 --rows 2 --auto               # the engine's own path choice under its workspace budget

60 s of mono audio at 44.1 kHz through a seeded synthetic model of the 44 kHz default size (tests/dac_torch.py; no real checkpoint
is needed for a time).  `encode` (encoder + quantiser) and `decode` are timed separately on tensors that are already on the device;
every call follows a warm-up call and ends in a device synchronise; median / min / max of the repeats.  --seg-frames times
egr_dacseg_encode / egr_dacseg_decode per segment length on a fresh handle each (so that the workspace held is that
length's), and names the kernels of an interior window's layers; F stands for the file's frame count (one window).  The flops are the dense
multiply-adds of the convolutions counted from the shapes.  These figures are reported, not gated.  Without a device the timing fails;
it has no fallback.  Kernel shares come from a run of its own:
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o dac -- python tools/dac_timing.py --repeats 1
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


def layers(cfg, dac_engine, rows, n):
    """(class, Cin, Cout, k, stride, dil, pad, L_in, L_out) of every convolution the launcher serves, and the dense flops of all."""
    n_pad, frames, _ = dac_engine.lengths(cfg, n)
    out, flops = [], 0.0

    def add(name, ci, co, k, s, d, p, li, lo):
        nonlocal flops
        out.append((name, ci, co, k, s, d, p, li, lo))
        flops += 2.0 * rows * lo * ci * co * k

    def units(side, C, L):
        for d in (1, 3, 9):
            add(f"{side} unit k7 d{d} C{C}", C, C, 7, 1, d, 3 * d, L, L)
            add(f"{side} unit k1 C{C}", C, C, 1, 1, 1, 0, L, L)

    C, L = cfg["encoder_dim"], n_pad
    flops += 2.0 * rows * L * C * 7
    for s in cfg["encoder_rates"]:
        units("enc", C, L)
        lo = dac_engine.conv_length(L, s)
        add(f"enc down s{s} C{C}", C, 2 * C, 2 * s, s, 1, (s + 1) // 2, L, lo)
        C, L = 2 * C, lo
    add("enc out k3", C, cfg["latent_dim"], 3, 1, 1, 1, L, L)
    enc_flops = flops + 2.0 * rows * L * cfg["n_codebooks"] * (2 * cfg["latent_dim"] + cfg["codebook_size"]) * cfg["codebook_dim"]
    flops = 0.0
    C, L = cfg["decoder_dim"], frames
    add("dec in k7", cfg["latent_dim"], C, 7, 1, 1, 3, L, L)
    for s in cfg["decoder_rates"]:
        add(f"dec up s{s} C{C} (GEMM onto taps)", C, 2 * s * (C // 2), 1, 1, 1, 0, L, L)
        C, L = C // 2, dac_engine.convtr_length(L, s)
        units("dec", C, L)
    flops += 2.0 * rows * L * C * 7
    return out, enc_flops, flops


def layer_kernels(cfg, native, dac_engine, rows, n):
    """{layer class: kernel name} from egr_conv_kernel_name (host only), on the operand scheme egr_dac.hip uses."""
    res = {}
    for name, ci, co, k, s, d, p, li, lo in layers(cfg, dac_engine, rows, n)[0]:
        gemm = "GEMM" in name
        f = dict(x=256, y=256, bias=256, B=rows * li if gemm else rows, W=1 if gemm else li, Cin=ci, OW=1 if gemm else lo, Cout=co, KW=k,
                 stride=s, dil=d, pad_l=p)
        if "k1" in name:
            f["res"] = 256
        if ci % 16 == 0:
            f.update(w3=256, sch=1, w_scale=1.0, row_amax=256, batch_rows=rows)
        else:
            f["w"] = 256
        kn, ks, _ = native.conv_kernel_name(**f)
        res[name] = kn + (f" split-K {ks}" if ks > 1 else "")
    return res


def timed(fn, repeats):
    import torch
    fn()                                                        # warm-up
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}


def segmented(a, cfg, rows, n, arch):
    """--seg-frames / --auto: a fresh handle per segment length; ms, workspace held, kernels of an interior window."""
    import torch
    from egregora_amd import dac_engine as E, dac_weights, native
    import dac_torch as R
    model = dac_weights.DacModel(cfg, R.synthetic_state_dict(cfg, 17))
    x = R.test_signal(rows, n, 9).cuda()
    F = E.lengths(cfg, n)[1]
    hop = R.hop(cfg)
    runs = []
    todo = [None] if a.auto else [F if s.strip() == "F" else int(s) for s in a.seg_frames.split(",")]
    for seg in todo:
        eng = E.DacEngine(model, torch.cuda.current_device())
        rec = {"seg_frames": seg, "rows": rows, "samples": n, "frames": F}
        z, codes = eng.encode(x, seg_frames=seg)
        rec["encode_ms"] = timed(lambda: eng.encode(x, seg_frames=seg), a.repeats)
        rec["held_after_encode"] = eng.workspace_held()
        rec["chosen_encode"] = eng.last_seg_frames if seg is None else seg
        y = eng.decode(z, seg_frames=seg)
        rec["decode_ms"] = timed(lambda: eng.decode(z, seg_frames=seg), a.repeats)
        rec["held"] = eng.workspace_held()
        rec["chosen_decode"] = eng.last_seg_frames if seg is None else seg
        rec["one_pass_workspace"] = eng.workspace_bytes(rows, n)
        rec["finite"] = bool(torch.isfinite(y).all())
        s_eff = rec["chosen_encode"]
        if s_eff is not None and s_eff < F:                     # an interior window's layers (encode's margins; decode's differ by 2 + 2 frames)
            i = E.segment_count(cfg, E.ENCODE, n, s_eff) // 2
            p = E.segment_plan(cfg, E.ENCODE, n, s_eff, i)
            rec["window_frames"] = p.win_hi - p.win_lo
            rec["layer_kernels"] = layer_kernels(cfg, native, E, rows, (p.win_hi - p.win_lo) * hop)
        runs.append(rec)
        print(f"seg_frames {seg}: encode {rec['encode_ms']['median']:.2f} ms ({rec['encode_ms']['min']:.2f} .. {rec['encode_ms']['max']:.2f}), "
              f"decode {rec['decode_ms']['median']:.2f} ms ({rec['decode_ms']['min']:.2f} .. {rec['decode_ms']['max']:.2f}), held {rec['held'] / 2 ** 20:.1f} MiB "
              f"(one pass {rec['one_pass_workspace'] / 2 ** 20:.1f} MiB), chose {rec['chosen_encode']} / {rec['chosen_decode']}, window {rec.get('window_frames')}")
        del eng, z, codes, y
        torch.cuda.empty_cache()
    out = {"arch": arch, "device": torch.cuda.get_device_name(0), "seconds_of_audio": a.seconds, "repeats": a.repeats, "runs": runs}
    print("RESULT " + json.dumps(out))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--out", default="")
    ap.add_argument("--rows", type=int, default=1)
    ap.add_argument("--seg-frames", default="", help="comma-separated segment lengths in frames; F = the whole file")
    ap.add_argument("--auto", action="store_true", help="time DacEngine.encode / decode on the path they choose themselves")
    a = ap.parse_args()
    import torch
    from packload import load_pack
    load_pack()
    from egregora_amd import dac_engine, dac_weights, native
    import dac_torch as R
    cfg = R.config("W")
    rows, n = a.rows, int(round(a.seconds * cfg["sample_rate"]))
    kern = layer_kernels(cfg, native, dac_engine, rows, n)
    if a.kernels:
        for k, v in kern.items():
            print(f"{k:40s} {v}")
        return
    arch = native.require_device()
    if a.seg_frames or a.auto:
        return segmented(a, cfg, rows, n, arch)
    eng = dac_engine.DacEngine(dac_weights.DacModel(cfg, R.synthetic_state_dict(cfg, 17)), torch.cuda.current_device())
    x = R.test_signal(rows, n, 9).cuda()
    z, codes = eng.encode(x)
    y = eng.decode(z)
    torch.cuda.synchronize()
    ways = {"encode": lambda: eng.encode(x), "decode": lambda: eng.decode(z)}
    times = {k: [] for k in ways}
    for _ in range(a.repeats):
        for k, fn in ways.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    _, enc_flops, dec_flops = layers(cfg, dac_engine, rows, n)
    ms = {k: {"median": 1e3 * statistics.median(v), "min": 1e3 * min(v), "max": 1e3 * max(v)} for k, v in times.items()}
    out = {"arch": arch, "device": torch.cuda.get_device_name(0), "seconds_of_audio": a.seconds, "sample_rate": cfg["sample_rate"], "rows": rows,
           "samples": n, "frames": int(z.shape[-1]), "decoded": int(y.shape[-1]), "repeats": a.repeats, "model": "synthetic, 44 kHz default size",
           "dense_gflop": {"encode": enc_flops / 1e9, "decode": dec_flops / 1e9}, "ms": ms,
           "tflops_dense_over_call_time": {"encode": enc_flops / 1e9 / ms["encode"]["median"], "decode": dec_flops / 1e9 / ms["decode"]["median"]},
           "workspace_bytes": eng.workspace_bytes(rows, n), "finite": bool(torch.isfinite(y).all()), "layer_kernels": kern}
    for k, v in ms.items():
        print(f"{k:8s} median {v['median']:9.3f} ms   min {v['min']:9.3f}   max {v['max']:9.3f}")
    print("RESULT " + json.dumps(out))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
