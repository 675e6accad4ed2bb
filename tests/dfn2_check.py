"""Gates of the native DeepFilterNet2 (egr_dfn2_*, csrc/egr_dfn3.hip) against the restatement tests/dfn2_torch.py, shared by the
GPU tests.  The margins are DeepFilterNet3's (dfn3_check: FLOOR, CAP, RMS_X, MAX_X, rel, maxrel, gate), imported unchanged:
  cumulative: every stage read back after one enhance call and compared with the restatement run from x (relative rms <= 1.5x
              fp32's + FLOOR, and <= CAP);
  local:      every stage fed the device's own read-back inputs and restated alone (relative rms <= 1.5x fp32's + FLOOR, max-abs /
              reference rms <= 3x fp32's + FLOOR).
Stages: DeepFilterNet3's names plus alpha, and per GroupedGRU layer i (encoder, ERB decoder, DF decoder) gru{i} (the layer output as
passed on, after the P4 shuffle) and sum{i} (the running sum of its module's layer outputs).
"""
import torch

import dfn2_torch as R
from dfn3_check import CAP, FLOOR, MAX_X, RMS_X, gate, maxrel, nchw, nhwc, rel, speechy  # noqa: F401 (the DFN3 gates, unchanged)

PICK = {
    "spec": lambda s: torch.view_as_real(s["spec"]),
    "feat_erb": lambda s: s["feat_erb"][:, 0],
    "feat_spec": lambda s: s["feat_spec"].permute(0, 2, 3, 1),
    "e0": lambda s: nhwc(s["e0"]), "e1": lambda s: nhwc(s["e1"]), "e2": lambda s: nhwc(s["e2"]), "e3": lambda s: nhwc(s["e3"]),
    "c0": lambda s: nhwc(s["c0"]), "emb": lambda s: s["emb"], "mask": lambda s: s["mask"], "coefs": lambda s: s["coefs"],
    "alpha": lambda s: s["alpha"], "spec_e": lambda s: torch.view_as_real(s["spec_e"]),
}


def n_grus(cfg):
    return cfg["emb_num_layers"] + cfg["df_num_layers"]


def layer_plan(cfg):
    """[(prefix, layer index within its module, module layer count)] for the global GroupedGRU layer indices."""
    ne, nd = cfg["emb_num_layers"] - 1, cfg["df_num_layers"]
    return ([("enc.emb_gru", 0, 1)] + [("erb_dec.emb_gru", l, ne) for l in range(ne)] + [("df_dec.df_gru", l, nd) for l in range(nd)])


def stage_counts(cfg, C, T):
    """Element counts egr_dfn2_stage reports after a call on [C, T] -> (named stages, per-layer counts)."""
    nF = (T + cfg["fft_size"]) // cfg["hop_size"]
    R_, Fq, E, nb, ch = C * nF, cfg["fft_size"] // 2 + 1, cfg["nb_erb"], cfg["nb_df"], cfg["conv_ch"]
    n = {"spec": R_ * Fq * 2, "feat_erb": R_ * E, "feat_spec": R_ * nb * 2, "e0": R_ * E * ch, "e1": R_ * (E // 2) * ch,
         "e2": R_ * (E // 4) * ch, "e3": R_ * (E // 4) * ch, "c0": R_ * nb * ch, "emb": R_ * cfg["emb_hidden_dim"], "mask": R_ * E,
         "coefs": R_ * nb * 2 * cfg["df_order"], "alpha": R_, "spec_e": R_ * Fq * 2}
    H = [cfg["emb_hidden_dim"]] * cfg["emb_num_layers"] + [cfg["df_hidden_dim"]] * cfg["df_num_layers"]
    return n, [R_ * h for h in H]


def device_stages(eng, s64):
    out = {}
    for name, f in PICK.items():
        out[name] = eng.stage(name).cpu().double().reshape(f(s64).shape)
    out["grus"] = [eng.stage("gru0", g).cpu().double().reshape(s64["grus"][g].shape) for g in range(len(s64["grus"]))]
    out["sums"] = [eng.stage("sum0", g).cpu().double().reshape(s64["sums"][g].shape) for g in range(len(s64["sums"]))]
    return out


def cumulative(eng, x, y, cfg, sd, r=None):
    """Cumulative gates on every stage and on y after eng.enhance(x) -> y.  Returns ({stage: (device, fp32) rms error}, stages, r)."""
    x = x.cpu()
    if r is None:
        r = (R.enhance(x, cfg, sd, torch.float64, stages=True), R.enhance(x, cfg, sd, torch.float32, stages=True))
    (y64, s64), (y32, s32) = r
    dev = device_stages(eng, s64)
    report = {}
    for name, f in PICK.items():
        report[name] = gate(name, dev[name], f(s64), f(s32))
    assert len(s64["grus"]) == n_grus(cfg)
    for g in range(n_grus(cfg)):
        report[f"gru{g}"] = gate(f"gru{g}", dev["grus"][g], s64["grus"][g], s32["grus"][g])
        report[f"sum{g}"] = gate(f"sum{g}", dev["sums"][g], s64["sums"][g], s32["sums"][g])
    report["y"] = gate("y", y.cpu(), y64, y32)
    return report, dev, r


def to_restatement(d):
    cpx = lambda t: torch.complex(t[..., 0].contiguous(), t[..., 1].contiguous())
    return {"spec": cpx(d["spec"]), "feat_erb": d["feat_erb"][:, None], "feat_spec": d["feat_spec"].permute(0, 3, 1, 2),
            "e0": nchw(d["e0"]), "e1": nchw(d["e1"]), "e2": nchw(d["e2"]), "e3": nchw(d["e3"]), "c0": nchw(d["c0"]),
            "emb": d["emb"], "mask": d["mask"], "coefs": d["coefs"], "alpha": d["alpha"], "spec_e": cpx(d["spec_e"]),
            "grus": d["grus"], "sums": d["sums"]}


def local_stage_refs(dev, cfg, sd, T, dtype):
    """Each stage restated alone in `dtype` from the device's read-back inputs."""
    def cast(v):                                   # exact: the device values are float32
        if v.is_complex():
            return v.to(torch.complex128 if dtype == torch.float64 else torch.complex64)
        return v.to(dtype)
    d = {k: ([cast(g) for g in v] if k in ("grus", "sums") else cast(v)) for k, v in to_restatement(dev).items()}
    net = R.Net2(cfg, sd, dtype)
    g, s = d["grus"], d["sums"]
    plan = layer_plan(cfg)
    last_erb, last = cfg["emb_num_layers"] - 1, n_grus(cfg) - 1
    out = {}
    with torch.no_grad():
        out["feat_erb"], out["feat_spec"] = R.shifted_features(d["spec"], cfg)
        out["e0"] = net.e0(d["feat_erb"])
        out["e1"] = net.e_next(1, d["e0"])
        out["e2"] = net.e_next(2, d["e1"])
        out["e3"] = net.e_next(3, d["e2"])
        out["c0"] = net.c0(d["feat_spec"])
        grus, sums = [], []
        for i, (prefix, l, n) in enumerate(plan):
            if i == 0:
                xin, acc = net.emb_in(d["e3"], d["c0"]), None
            elif l == 0:
                xin, acc = d["emb"], None
            else:
                xin, acc = g[i - 1], s[i - 1]
            y, a = net.ggru_step(xin, prefix, l, n, acc)
            grus.append(y)
            sums.append(a)
        out["grus"], out["sums"] = grus, sums
        out["emb"] = sums[0]
        out["mask"] = net.mask2(s[last_erb], d["e0"], d["e1"], d["e2"], d["e3"])
        c = net.df_c(s[last], d["emb"])
        out["alpha"] = net.alpha(c)
        out["coefs"] = net.coefs2(c, d["c0"])
        out["spec_e"] = net.assemble2(d["spec"], d["mask"], d["coefs"], d["alpha"])
        out["y"] = R.synthesis(d["spec_e"], cfg, T)
    return out


def _layout(name, t):
    if name == "spec_e":
        return torch.view_as_real(t)
    if name == "feat_erb":
        return t[:, 0]
    if name == "feat_spec":
        return t.permute(0, 2, 3, 1)
    if name in ("e0", "e1", "e2", "e3", "c0"):
        return nhwc(t)
    return t


def local(eng, x, y, cfg, sd, dev, floor=FLOOR):
    """Local gates: every stage against its float64 restatement from the device's own inputs.  The spectrum's local input is x, so
    its gate is the cumulative one.  Returns {stage: (rms, rms fp32, max, max fp32)}."""
    T = x.shape[1]
    ref = {torch.float64: local_stage_refs(dev, cfg, sd, T, torch.float64),
           torch.float32: local_stage_refs(dev, cfg, sd, T, torch.float32)}
    x64 = x.cpu().double()
    a64, a32 = R.analysis(x64, cfg), R.analysis(x.cpu().float(), cfg)
    names = ["feat_erb", "feat_spec", "e0", "e1", "e2", "e3", "c0", "emb", "mask", "alpha", "coefs", "spec_e"]
    pairs = [("spec", dev["spec"], torch.view_as_real(a64), torch.view_as_real(a32))]
    pairs += [(n, dev[n], _layout(n, ref[torch.float64][n]), _layout(n, ref[torch.float32][n])) for n in names]
    for i in range(n_grus(cfg)):
        pairs.append((f"gru{i}", dev["grus"][i], ref[torch.float64]["grus"][i], ref[torch.float32]["grus"][i]))
        pairs.append((f"sum{i}", dev["sums"][i], ref[torch.float64]["sums"][i], ref[torch.float32]["sums"][i]))
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
