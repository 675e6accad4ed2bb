"""Plain-PyTorch restatement of DeepFilterNet3 as `df.enhance.enhance(model, df_state, x)` runs it (SPEC.md, "DeepFilterNet3
(UPSTREAM-RECALL)"), in float32 or float64: libdf analysis, ERB / complex features with their exponential norms, the encoder,
both decoders (torch.nn.GRU for the recurrences), ERB mask + deep filter, libdf synthesis, the n_fft pad and the n_fft - hop trim.

It is written in the upstream modules' own NCHW shapes (not in the device layout), and is the yardstick of tests/test_gpu_dfn3.py
and a `set_enhancer` backend for the node tests.  Also builds the synthetic model directory the tests use (the real checkpoint is
not in the test images): a DeepFilterNet3-default config.ini and a seeded random state dict with the key table's names / shapes.
"""
import math
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

CONFIG_INI = """[train]
model = deepfilternet3

[df]
sr = 48000
fft_size = 960
hop_size = 480
nb_erb = 32
nb_df = 96
norm_tau = 1
lsnr_max = 35
lsnr_min = -15
min_nb_erb_freqs = 2
df_order = 5
df_lookahead = 2
pad_mode = input_specf

[deepfilternet]
conv_lookahead = 2
conv_ch = 64
conv_depthwise = True
convt_depthwise = True
conv_kernel = 1,3
convt_kernel = 1,3
conv_kernel_inp = 3,3
emb_hidden_dim = 256
emb_num_layers = 3
emb_gru_skip_enc = none
emb_gru_skip = none
df_hidden_dim = 256
df_gru_skip = groupedlinear
df_pathway_kernel_size_t = 5
enc_concat = False
df_num_layers = 2
df_n_iter = 1
lin_groups = 16
enc_lin_groups = 32
mask_pf = False
"""


def W():
    from egregora_amd import dfn_weights
    return dfn_weights


def synthetic_state_dict(cfg: dict, seed: int = 0):
    """Seeded random tensors with the key table's names and shapes (PyTorch-default-like uniform fan-in scaling)."""
    dw = W()
    g = torch.Generator().manual_seed(seed)
    u = lambda shape, a: (torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * a
    fb, ifb = dw.erb_matrices(dw.erb_widths(cfg["sr"], cfg["fft_size"], cfg["nb_erb"], cfg["min_nb_erb_freqs"]))
    sd = {}
    for name, shape in dw.expected_table(cfg).items():
        if name == "erb_fb":
            t = fb.double()
        elif name == "mask.erb_inv_fb":
            t = ifb.double()
        elif name.endswith("num_batches_tracked"):
            sd[name] = torch.tensor(0, dtype=torch.int64)
            continue
        elif name.endswith("running_mean") or (name.endswith(".bias") and len(shape) == 1 and "gru" not in name and "fc" not in name):
            t = u(shape, 0.1)
        elif name.endswith("running_var"):
            t = 0.5 + torch.rand(shape, generator=g, dtype=torch.float64)
        elif len(shape) == 1 and "gru" not in name and "fc" not in name:            # BatchNorm weight
            t = 0.8 + 0.4 * torch.rand(shape, generator=g, dtype=torch.float64)
        elif ".gru." in name:
            t = u(shape, 1.0 / math.sqrt(shape[-1] if "weight" in name else shape[0] // 3))
        elif len(shape) == 3:                                                          # grouped linear [G, I, H/G]
            t = u(shape, 1.0 / math.sqrt(shape[1]))
        else:                                                                          # conv / linear
            t = u(shape, 1.0 / math.sqrt(max(1, int(np.prod(shape[1:])))))
        sd[name] = t.float()
    return sd


def write_model_dir(d: Path, seed: int = 0, cfg_text: str = CONFIG_INI, epoch: int = 120):
    """A DeepFilterNet model directory (config.ini + checkpoints/model_<epoch>.ckpt.best) -> (cfg, state dict)."""
    d = Path(d)
    (d / "checkpoints").mkdir(parents=True, exist_ok=True)
    (d / "config.ini").write_text(cfg_text, encoding="utf-8")
    cfg = W().parse_config(d / "config.ini")
    sd = synthetic_state_dict(cfg, seed)
    torch.save(sd, d / "checkpoints" / f"model_{epoch}.ckpt.best")
    return cfg, sd


# ------------------------------------------------------------------------------------------------ signal path
def vorbis_window(n_fft: int) -> torch.Tensor:
    """libdf: sin(pi/2 sin^2(pi (i + 0.5) / n_fft)) in double, stored as float32."""
    h = n_fft // 2
    i = torch.arange(n_fft, dtype=torch.float64)
    s = torch.sin(0.5 * math.pi * (i + 0.5) / h)
    return torch.sin(0.5 * math.pi * s * s).float()


def analysis(x: torch.Tensor, cfg: dict) -> torch.Tensor:
    """[C, T] -> complex [C, nF, n_fft/2+1]: enhance's n_fft right pad, then libdf frame_analysis (n_fft - hop samples of frame
    memory starting at zero, window, FFT, times wnorm = 2 hop / n_fft^2)."""
    n, hop = cfg["fft_size"], cfg["hop_size"]
    C, T = x.shape
    nF = (T + n) // hop
    xp = torch.cat([x.new_zeros(C, n - hop), x, x.new_zeros(C, n)], 1)
    fr = xp.unfold(1, n, hop)[:, :nF]
    w = vorbis_window(n).to(x.dtype)
    wnorm = torch.tensor(1.0 / (n * n / (2 * hop)), dtype=torch.float32).to(x.dtype)
    return torch.fft.rfft(fr * w, dim=-1) * wnorm


def synthesis(spec: torch.Tensor, cfg: dict, T: int) -> torch.Tensor:
    """libdf frame_synthesis (unnormalised inverse real FFT, window, overlap-add), then enhance's trim [n_fft - hop, +T)."""
    n, hop = cfg["fft_size"], cfg["hop_size"]
    C, nF, _ = spec.shape
    w = vorbis_window(n).to(spec.real.dtype)
    fr = torch.fft.irfft(spec, n=n, dim=-1, norm="forward") * w                 # [C, nF, n]
    out = spec.real.new_zeros(C, nF * hop + n)
    for m in range(n // hop):
        out[:, m * hop:m * hop + nF * hop] += fr[:, :, m * hop:(m + 1) * hop].reshape(C, -1)
    d = n - hop
    return out[:, d:d + T]


def features(spec: torch.Tensor, cfg: dict):
    """-> (feat_erb [C, 1, nF, E], feat_spec [C, 2, nF, nb_df]) before the lookahead shift (df.enhance.df_features)."""
    dw = W()
    a = dw.norm_alpha(cfg)
    widths = dw.erb_widths(cfg["sr"], cfg["fft_size"], cfg["nb_erb"], cfg["min_nb_erb_freqs"])
    fb, _ = dw.erb_matrices(widths)
    rdt = spec.real.dtype
    pw = (spec.real ** 2 + spec.imag ** 2) @ fb.to(rdt)
    db = 10.0 * torch.log10(pw + 1e-10)
    E, nbdf = cfg["nb_erb"], cfg["nb_df"]
    s = torch.linspace(-60.0, -90.0, E, dtype=torch.float32).to(rdt).expand(spec.shape[0], E).clone()
    erb = torch.empty_like(db)
    for t in range(db.shape[1]):
        s = db[:, t] * (1 - a) + s * a
        erb[:, t] = (db[:, t] - s) / 40.0
    us = torch.linspace(0.001, 0.0001, nbdf, dtype=torch.float32).to(rdt).expand(spec.shape[0], nbdf).clone()
    cs = spec[:, :, :nbdf]
    cf = torch.empty_like(cs)
    for t in range(cs.shape[1]):
        us = cs[:, t].abs() * (1 - a) + us * a
        cf[:, t] = cs[:, t] / torch.sqrt(us)
    return erb[:, None], torch.stack([cf.real, cf.imag], 1)


def _shift(x: torch.Tensor, la: int) -> torch.Tensor:
    """DfNet.pad_feat: ConstantPad2d((0, 0, -la, la)) on the time axis (dim 2)."""
    if la <= 0:
        return x
    return F.pad(x, (0, 0, -la, la))


class Net:
    def __init__(self, cfg: dict, sd: dict, dtype=torch.float64):
        self.cfg, self.dt = cfg, dtype
        self.sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}

    def bn(self, x, p):
        sd = self.sd
        sh = (1, -1, 1, 1)
        return (x - sd[p + ".running_mean"].view(sh)) / torch.sqrt(sd[p + ".running_var"].view(sh) + 1e-5) * sd[p + ".weight"].view(sh) + \
            sd[p + ".bias"].view(sh)

    def conv(self, x, w, fstride=1, groups=1):
        kt, kf = w.shape[2], w.shape[3]
        if kt > 1:
            x = F.pad(x, (0, 0, kt - 1, 0))
        return F.conv2d(x, w, padding=(0, kf // 2), stride=(1, fstride), groups=groups)

    def convt(self, x, w, fstride, groups):
        kf = w.shape[3]
        return F.conv_transpose2d(x, w, padding=(0, kf // 2), output_padding=(0, kf // 2), stride=(1, fstride), groups=groups)

    def gl(self, x, w):
        b, t, _ = x.shape
        g, i, h = w.shape
        return torch.einsum("btgi,gih->btgh", x.reshape(b, t, g, i), w).reshape(b, t, g * h)

    def gru(self, x, prefix, n, outs):
        sd = self.sd
        H = sd[prefix + ".weight_hh_l0"].shape[1]
        m = torch.nn.GRU(x.shape[-1], H, num_layers=1, batch_first=True).to(self.dt)
        for k in range(n):
            with torch.no_grad():
                m.weight_ih_l0.copy_(sd[f"{prefix}.weight_ih_l{k}"])
                m.weight_hh_l0.copy_(sd[f"{prefix}.weight_hh_l{k}"])
                m.bias_ih_l0.copy_(sd[f"{prefix}.bias_ih_l{k}"])
                m.bias_hh_l0.copy_(sd[f"{prefix}.bias_hh_l{k}"])
                x, _ = m(x)
            outs.append(x)
        return x

    def forward(self, spec: torch.Tensor, feat_erb, feat_spec, st: dict):
        cfg, sd = self.cfg, self.sd
        C = cfg["conv_ch"]
        relu = torch.relu
        la = cfg["conv_lookahead"] if cfg["pad_mode"].startswith("input") else 0
        fe, fs = _shift(feat_erb, la), _shift(feat_spec, la)
        st["feat_erb"], st["feat_spec"] = fe, fs
        e0 = relu(self.bn(self.conv(fe, sd["enc.erb_conv0.1.weight"]), "enc.erb_conv0.2"))
        es = [e0]
        for i, fstr in ((1, 2), (2, 2), (3, 1)):
            y = self.conv(es[-1], sd[f"enc.erb_conv{i}.0.weight"], fstr, C)
            es.append(relu(self.bn(self.conv(y, sd[f"enc.erb_conv{i}.1.weight"]), f"enc.erb_conv{i}.2")))
        e0, e1, e2, e3 = es
        c0 = relu(self.bn(self.conv(self.conv(fs, sd["enc.df_conv0.1.weight"], 1, 2), sd["enc.df_conv0.2.weight"]), "enc.df_conv0.3"))
        c1 = relu(self.bn(self.conv(self.conv(c0, sd["enc.df_conv1.0.weight"], 2, C), sd["enc.df_conv1.1.weight"]), "enc.df_conv1.2"))
        cemb = relu(self.gl(c1.permute(0, 2, 3, 1).flatten(2), sd["enc.df_fc_emb.0.weight"]))
        emb = e3.permute(0, 2, 3, 1).flatten(2) + cemb
        grus = []
        x = relu(self.gl(emb, sd["enc.emb_gru.linear_in.0.weight"]))
        x = self.gru(x, "enc.emb_gru.gru", 1, grus)
        emb = relu(self.gl(x, sd["enc.emb_gru.linear_out.0.weight"]))
        st.update(e0=e0, e1=e1, e2=e2, e3=e3, c0=c0, emb=emb)
        # ERB decoder
        b, _, t, f8 = e3.shape
        x = relu(self.gl(emb, sd["erb_dec.emb_gru.linear_in.0.weight"]))
        x = self.gru(x, "erb_dec.emb_gru.gru", cfg["emb_num_layers"] - 1, grus)
        d = relu(self.gl(x, sd["erb_dec.emb_gru.linear_out.0.weight"])).view(b, t, f8, -1).permute(0, 3, 1, 2)
        def p(e, i):                                   # pathway conv: groups = in_ch / (in_ch per group) from the weight shape
            w = sd[f"erb_dec.conv{i}p.0.weight"]
            return relu(self.bn(self.conv(e, w, 1, C // w.shape[1]), f"erb_dec.conv{i}p.1"))
        y = self.conv(p(e3, 3) + d, sd["erb_dec.convt3.0.weight"], 1, C)
        d = relu(self.bn(self.conv(y, sd["erb_dec.convt3.1.weight"]), "erb_dec.convt3.2"))
        for i, e in ((2, e2), (1, e1)):
            y = self.convt(p(e, i) + d, sd[f"erb_dec.convt{i}.0.weight"], 2, C)
            d = relu(self.bn(self.conv(y, sd[f"erb_dec.convt{i}.1.weight"]), f"erb_dec.convt{i}.2"))
        m = torch.sigmoid(self.bn(self.conv(p(e0, 0) + d, sd["erb_dec.conv0_out.0.weight"]), "erb_dec.conv0_out.1"))   # [B, 1, T, E]
        # DF decoder
        x = relu(self.gl(emb, sd["df_dec.df_gru.linear_in.0.weight"]))
        c = self.gru(x, "df_dec.df_gru.gru", cfg["df_num_layers"], grus)
        if cfg["df_gru_skip"] == "groupedlinear":
            c = c + self.gl(emb, sd["df_dec.df_skip.weight"])
        O2 = 2 * cfg["df_order"]
        gp = C // sd["df_dec.df_convp.1.weight"].shape[1]
        cp = relu(self.bn(self.conv(self.conv(c0, sd["df_dec.df_convp.1.weight"], 1, gp), sd["df_dec.df_convp.2.weight"]), "df_dec.df_convp.3"))
        coefs = torch.tanh(self.gl(c, sd["df_dec.df_out.0.weight"])).view(b, t, cfg["nb_df"], O2) + cp.permute(0, 2, 3, 1)
        st.update(grus=grus, mask=m[:, 0], coefs=coefs)
        # mask + deep filter
        _, inv = W().erb_matrices(W().erb_widths(cfg["sr"], cfg["fft_size"], cfg["nb_erb"], cfg["min_nb_erb_freqs"]))
        spec_m = spec * (m[:, 0] @ inv.to(self.dt))
        O, L, nb = cfg["df_order"], cfg["df_lookahead"], cfg["nb_df"]
        sp = F.pad(spec[:, :, :nb].transpose(1, 2), (O - 1 - L, L))                 # [B, nb, T + O - 1]
        co = torch.complex(coefs[..., 0::2], coefs[..., 1::2])                      # [B, T, nb, O]
        y = sum(sp[:, :, n:n + t].transpose(1, 2) * co[..., n] for n in range(O))
        out = spec_m.clone()
        out[:, :, :nb] = y
        return out


def enhance(x: torch.Tensor, cfg: dict, sd: dict, dtype=torch.float64, stages: bool = False):
    """x [C, T] -> y [C, T] in `dtype` (and the stage dict when `stages`)."""
    x = x.to(dtype)
    st = {}
    spec = analysis(x, cfg)
    fe, fs = features(spec, cfg)
    spec_e = Net(cfg, sd, dtype).forward(spec, fe, fs, st)
    y = synthesis(spec_e, cfg, x.shape[1])
    st.update(spec=spec, spec_e=spec_e, y=y)
    return (y, st) if stages else y


def enhancer(cfg: dict, sd: dict, dtype=torch.float32):
    """A set_enhancer backend: fn(x48 [1, T], model_name) -> [1, T] float32."""
    def fn(x, model_name=""):
        with torch.no_grad():
            return enhance(x.detach().cpu().float(), cfg, sd, dtype).float()
    return fn
