"""Gates of the native DeepFilterNet3 (csrc/egr_dfn3.hip) against the restatement tests/dfn3_torch.py, shared by the GPU tests.

Two kinds, both measured against the float64 restatement and scaled by the float32 restatement's own error on the same input:
  cumulative: every stage read back after one enhance call and compared with the restatement run from x, so a stage carries the
              error of every stage before it (relative rms <= 1.5x fp32's + FLOOR, and <= CAP);
  local:      every stage fed the device's own read-back inputs (eng.stage) and restated alone, so the bound is that stage's own
              precision: relative rms <= 1.5x fp32's + FLOOR, max-abs / reference rms <= 3x fp32's + FLOOR.
"""
import numpy as np
import torch

import dfn3_torch as R

FLOOR, CAP = 3e-7, 1e-4
RMS_X, MAX_X = 1.5, 3.0


def speechy(seed, n, C, sr=48000):
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(n) / sr
    env = 0.5 + 0.5 * np.sin(2 * np.pi * 2.3 * t) ** 2
    x = np.stack([env * sum(np.sin(2 * np.pi * f * (1 + 0.01 * c) * t) / (k + 1) for k, f in enumerate((150, 310, 620, 1240, 2900)))
                  + 0.05 * rng.standard_normal(n) for c in range(C)])
    return torch.from_numpy((0.4 * x / np.abs(x).max()).astype(np.float32))


def rel(a, ref):
    a, ref = a.double().cpu().reshape(-1), ref.double().cpu().reshape(-1)
    return float((a - ref).norm() / max(float(ref.norm()), 1e-300))


def maxrel(a, ref):
    """max |a - ref| over the rms of ref."""
    a, ref = a.double().cpu().reshape(-1), ref.double().cpu().reshape(-1)
    if ref.numel() == 0:
        return 0.0
    rms = float(ref.norm()) / ref.numel() ** 0.5
    return float((a - ref).abs().max()) / max(rms, 1e-300)


def gate(name, got, r64, r32, floor=FLOOR, cap=CAP):
    e, e32 = rel(got, r64), rel(r32, r64)
    assert e <= RMS_X * e32 + floor and e <= cap, (name, e, e32)
    return e, e32


def nhwc(t):
    return t.permute(0, 2, 3, 1)


def nchw(t):
    return t.permute(0, 3, 1, 2)


# restatement stage (upstream shapes) -> the device layout of egr_dfn3_stage (include/egregora_amd.h)
PICK = {
    "spec": lambda s: torch.view_as_real(s["spec"]),
    "feat_erb": lambda s: s["feat_erb"][:, 0],
    "feat_spec": lambda s: s["feat_spec"].permute(0, 2, 3, 1),
    "e0": lambda s: nhwc(s["e0"]), "e1": lambda s: nhwc(s["e1"]), "e2": lambda s: nhwc(s["e2"]), "e3": lambda s: nhwc(s["e3"]),
    "c0": lambda s: nhwc(s["c0"]), "emb": lambda s: s["emb"], "mask": lambda s: s["mask"], "coefs": lambda s: s["coefs"],
    "spec_e": lambda s: torch.view_as_real(s["spec_e"]),
}


def n_grus(cfg):
    return 1 + (cfg["emb_num_layers"] - 1) + cfg["df_num_layers"]


def stage_counts(cfg, C, T):
    """Element counts egr_dfn3_stage reports after a call on [C, T]."""
    nF = (T + cfg["fft_size"]) // cfg["hop_size"]
    R_, Fq, E, nb, ch = C * nF, cfg["fft_size"] // 2 + 1, cfg["nb_erb"], cfg["nb_df"], cfg["conv_ch"]
    n = {"spec": R_ * Fq * 2, "feat_erb": R_ * E, "feat_spec": R_ * nb * 2, "e0": R_ * E * ch, "e1": R_ * (E // 2) * ch,
         "e2": R_ * (E // 4) * ch, "e3": R_ * (E // 4) * ch, "c0": R_ * nb * ch, "emb": R_ * ch * E // 4, "mask": R_ * E,
         "coefs": R_ * nb * 2 * cfg["df_order"], "spec_e": R_ * Fq * 2}
    H = [cfg["emb_hidden_dim"]] * cfg["emb_num_layers"] + [cfg["df_hidden_dim"]] * cfg["df_num_layers"]
    return n, [R_ * h for h in H]


def device_stages(eng, s64):
    """Every stage of the last enhance call in the restatement's shapes (float64, CPU), shaped after the float64 stage dict."""
    out = {}
    for name, f in PICK.items():
        out[name] = eng.stage(name).cpu().double().reshape(f(s64).shape)
    out["grus"] = [eng.stage("gru0", g).cpu().double().reshape(s64["grus"][g].shape) for g in range(len(s64["grus"]))]
    return out


def to_restatement(d):
    """Device layouts (device_stages) -> the restatement's own shapes (complex spectra, NCHW maps)."""
    cpx = lambda t: torch.complex(t[..., 0].contiguous(), t[..., 1].contiguous())
    return {"spec": cpx(d["spec"]), "feat_erb": d["feat_erb"][:, None], "feat_spec": d["feat_spec"].permute(0, 3, 1, 2),
            "e0": nchw(d["e0"]), "e1": nchw(d["e1"]), "e2": nchw(d["e2"]), "e3": nchw(d["e3"]), "c0": nchw(d["c0"]),
            "emb": d["emb"], "mask": d["mask"], "coefs": d["coefs"], "spec_e": cpx(d["spec_e"]), "grus": d["grus"]}


def cumulative(eng, x, y, cfg, sd, r=None):
    """Cumulative gates on every stage and on y after eng.enhance(x) -> y.  Returns ({stage: (device, fp32) rms error}, stage dicts)."""
    x = x.cpu()
    if r is None:
        r = (R.enhance(x, cfg, sd, torch.float64, stages=True), R.enhance(x, cfg, sd, torch.float32, stages=True))
    (y64, s64), (y32, s32) = r
    dev = device_stages(eng, s64)
    report = {}
    for name, f in PICK.items():
        report[name] = gate(name, dev[name], f(s64), f(s32))
    assert len(s64["grus"]) == n_grus(cfg)
    for g in range(len(s64["grus"])):
        report[f"gru{g}"] = gate(f"gru{g}", dev["grus"][g], s64["grus"][g], s32["grus"][g])
    report["y"] = gate("y", y.cpu(), y64, y32)
    return report, dev, r


def local_stage_refs(dev, cfg, sd, T, dtype):
    """Each stage restated alone in `dtype` from the device's read-back inputs: {stage: restatement-shaped tensor}."""
    def cast(v):                                   # exact: the device values are float32
        if v.is_complex():
            return v.to(torch.complex128 if dtype == torch.float64 else torch.complex64)
        return v.to(dtype)
    d = {k: ([cast(g) for g in v] if k == "grus" else cast(v)) for k, v in to_restatement(dev).items()}
    net = R.Net(cfg, sd, dtype)
    ne = cfg["emb_num_layers"] - 1
    g = d["grus"]
    out = {}
    with torch.no_grad():
        out["feat_erb"], out["feat_spec"] = R.shifted_features(d["spec"], cfg)
        out["e0"] = net.e0(d["feat_erb"])
        out["e1"] = net.e_next(1, d["e0"])
        out["e2"] = net.e_next(2, d["e1"])
        out["e3"] = net.e_next(3, d["e2"])
        out["c0"] = net.c0(d["feat_spec"])
        grus = [net.gru_enc(d["e3"], d["c0"])]
        out["emb"] = net.emb(g[0])
        for k in range(ne):
            grus.append(net.erb_gru(k, d["emb"] if k == 0 else g[k]))
        out["mask"] = net.mask(g[ne], d["e0"], d["e1"], d["e2"], d["e3"])
        for k in range(cfg["df_num_layers"]):
            grus.append(net.df_gru(k, d["emb"] if k == 0 else g[ne + k]))
        out["coefs"] = net.coefs(g[-1], d["emb"], d["c0"])
        out["spec_e"] = net.assemble(d["spec"], d["mask"], d["coefs"])
        out["y"] = R.synthesis(d["spec_e"], cfg, T)
        out["grus"] = grus
    return out


def _layout(name, t):
    """A restatement-shaped local result in the device layout."""
    if name in ("spec_e",):
        return torch.view_as_real(t)
    if name == "feat_erb":
        return t[:, 0]
    if name == "feat_spec":
        return t.permute(0, 2, 3, 1)
    if name in ("e0", "e1", "e2", "e3", "c0"):
        return nhwc(t)
    return t


def local(eng, x, y, cfg, sd, dev, r64=None, floor=FLOOR):
    """Local gates: every stage against its float64 restatement from the device's own inputs.  The spectrum's local input is x, so
    its gate is the cumulative one.  Returns {stage: (rms, rms fp32, max, max fp32)}."""
    T = x.shape[1]
    ref = {torch.float64: local_stage_refs(dev, cfg, sd, T, torch.float64),
           torch.float32: local_stage_refs(dev, cfg, sd, T, torch.float32)}
    x64 = x.cpu().double()
    a64, a32 = R.analysis(x64, cfg), R.analysis(x.cpu().float(), cfg)
    names = ["feat_erb", "feat_spec", "e0", "e1", "e2", "e3", "c0", "emb", "mask", "coefs", "spec_e"]
    pairs = [("spec", dev["spec"], torch.view_as_real(a64), torch.view_as_real(a32))]
    pairs += [(n, dev[n], _layout(n, ref[torch.float64][n]), _layout(n, ref[torch.float32][n])) for n in names]
    pairs += [(f"gru{g}", dev["grus"][g], ref[torch.float64]["grus"][g], ref[torch.float32]["grus"][g]) for g in range(n_grus(cfg))]
    pairs.append(("y", y.cpu(), ref[torch.float64]["y"], ref[torch.float32]["y"]))
    report, bad = {}, []
    for name, got, r64_, r32_ in pairs:
        got = got.reshape(r64_.shape)
        e, e32, m, m32 = rel(got, r64_), rel(r32_, r64_), maxrel(got, r64_), maxrel(r32_, r64_)
        report[name] = (e, e32, m, m32)
        if not (e <= RMS_X * e32 + floor and m <= MAX_X * m32 + floor):
            bad.append((name, e, e32, m, m32))
    assert not bad, bad
    return report


def fmt(report):
    return {k: "/".join(f"{a:.2e}" for a in v) for k, v in report.items()}
