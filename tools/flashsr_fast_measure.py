"""Measurements of FlashSR's one-term fast mode (profiles/flashsr_fast.md), all against the default mode of the same build in one
process on one GPU:

  kernels  -- per contraction instantiation of the full-size graph at 13 rows (one of the two row groups of a 26-row pass), from the
              handle's own profile (egr_flashsr_profile): ms per launch under scheme 1 and under scheme 2, the two INTERLEAVED on
              one live handle (egr_flashsr_set_split 1 / 3), median of 5 after 2 warm-ups, with the spread of the five;
  accuracy -- one full-size row of the synthetic-weights table against the float64 run of the same graph, stage by stage
              (egr_flashsr_forward under set_split 2 and 4), and the waveform's LSD (2048 / 512, the reference's metric).

usage: python tools/flashsr_fast_measure.py [kernels] [accuracy] [--out FILE.json]
"""
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def twin(name):
    if name.startswith(("k_conv_s3<", "k_conv1d_s3<")) and name.endswith(", 1>"):
        return name[:-2] + "2>"
    if name.startswith("k_conv3x3_isp<"):
        return name[:-1] + ", 2>"
    return None


def kernels(eng, cfg, torch, rows=13, warm=2, reps=5):
    x = (0.2 * torch.randn(rows, cfg.chunk, generator=torch.Generator().manual_seed(5))).cuda()
    ids = torch.arange(rows, dtype=torch.int64, device="cuda")
    runs = {"f16x2": [], "f16x1": []}
    for i in range(warm + reps):
        for mode in ("f16x2", "f16x1"):
            eng.set_split(mode)
            prof = eng.c_profile(lambda: eng.c_infer(x, ids, 1))
            torch.cuda.synchronize()
            if i >= warm:
                runs[mode].append(prof)
    eng.set_split("f16x2")
    out = []
    for name in sorted(runs["f16x2"][0]):
        t = twin(name)
        n = runs["f16x2"][0][name][0]
        a = [p[name][2] / p[name][0] for p in runs["f16x2"]]
        row = dict(kernel=name, launches=n, ms_per_launch=statistics.median(a), spread=max(a) - min(a), total_ms=statistics.median(a) * n)
        if t and all(t in p for p in runs["f16x1"]):
            b = [p[t][2] / p[t][0] for p in runs["f16x1"]]
            row.update(twin=t, twin_ms_per_launch=statistics.median(b), twin_spread=max(b) - min(b), twin_total_ms=statistics.median(b) * n,
                       ratio=statistics.median(b) / statistics.median(a), wins=statistics.median(a) - statistics.median(b) > max(a) - min(a))
        elif name in runs["f16x1"][0]:
            b = [p[name][2] / p[name][0] for p in runs["f16x1"]]
            row.update(same_kernel_in_the_mode_ms_per_launch=statistics.median(b))
        out.append(row)
    tot = {m: statistics.median(sum(v[2] for v in p.values()) for p in runs[m]) for m in runs}
    return dict(rows=rows, contraction_ms_per_forward=tot, kernels=out)


def accuracy(eng, cfg, P, torch):
    from oracle import metrics as om
    from test_gpu_flashsr import f64_forward_on_gpu, nchw, rel_l2
    x = 0.2 * torch.randn(1, cfg.chunk, generator=torch.Generator().manual_seed(5))
    ids = torch.zeros(1, dtype=torch.int64, device="cuda")
    nz = eng.noise(1, ids, 1)
    f64 = {}
    y64 = f64_forward_on_gpu(x, nchw(nz.cpu()), P, cfg, f64)
    out = {}
    for mode in ("f16x2+forward", "f16x1+forward"):
        eng.set_split(mode)
        st = {}
        y = eng.c_forward(x.cuda(), nz, stages=st).cpu()
        errs = {k: rel_l2(st[k].permute(0, 3, 1, 2) if st[k].dim() == 4 else st[k], f64[k].cpu()) for k in ("mel", "z_cond", "v", "z0", "mel_hat")}
        errs["y"] = rel_l2(y, y64)
        lsd = om.lsd_audio(y64.double().numpy().reshape(-1), y.double().numpy().reshape(-1), 2048, 512)
        errs["lsd_2048_512_db"] = float(lsd[0])
        errs["lsd_256_64_db"] = float(om.lsd_audio(y64.double().numpy().reshape(-1), y.double().numpy().reshape(-1), 256, 64)[0])
        out[mode.split("+")[0]] = errs
    eng.set_split("f16x2")
    return out


def main():
    import torch
    from packload import load_pack
    load_pack()
    from egregora_amd import flashsr_arch as A
    from tools.flashsr_pydriver import PyDriverEngine
    what = [a for a in sys.argv[1:] if not a.startswith("--")] or ["kernels", "accuracy"]
    cfg = A.FlashSRConfig()
    P = A.init_params(cfg, 0)
    eng = PyDriverEngine(cfg, P)
    res = {}
    if "accuracy" in what:
        res["accuracy_one_full_size_row_vs_float64"] = accuracy(eng, cfg, P, torch)
        print(json.dumps(res["accuracy_one_full_size_row_vs_float64"], indent=1), flush=True)
    if "kernels" in what:
        res["kernels"] = kernels(eng, cfg, torch)
        for r in res["kernels"]["kernels"]:
            print(json.dumps(r), flush=True)
        print(json.dumps(res["kernels"]["contraction_ms_per_forward"]), flush=True)
    if "--out" in sys.argv:
        Path(sys.argv[sys.argv.index("--out") + 1]).write_text(json.dumps(res, indent=1))
    eng.close()


if __name__ == "__main__":
    main()
