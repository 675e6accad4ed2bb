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


# The configurations the native forward pass claims (dfn_weights.check_supported), each a config_text override set; every entry
# changes one thing from the default unless its name says otherwise.  tests/test_gpu_dfn3_configs.py runs each on the device,
# tests/test_dfn3_weights.py loads each and runs it through this restatement.
MATRIX = {
    "hop240": dict(hop_size=240),                                                   # 4-way overlap-add
    "fft512_nbdf64": dict(fft_size=512, hop_size=256, nb_df=64),
    "fft3072": dict(fft_size=3072, hop_size=768),                                   # > 64 KiB of dynamic LDS in analysis / synthesis
    "fft4096": dict(fft_size=4096, hop_size=1024),
    "H128_128": dict(emb_hidden_dim=128, df_hidden_dim=128),
    "H256_96": dict(emb_hidden_dim=256, df_hidden_dim=96),
    "H100_100_lin4": dict(emb_hidden_dim=100, df_hidden_dim=100, lin_groups=4),    # H not a multiple of 16
    "conv_kernel_2_3": dict(conv_kernel="2,3"),                                     # causal taps in the depthwise convs
    "conv_kernel_1_5": dict(conv_kernel="1,5"),                                     # kf != convt_kf
    "conv_kernel_inp_1_3": dict(conv_kernel_inp="1,3"),
    "pathway_kt1": dict(df_pathway_kernel_size_t=1),
    "lookaheads0": dict(conv_lookahead=0, df_lookahead=0),
    "pad_none": dict(pad_mode="none"),
    "order1_la0": dict(df_order=1, df_lookahead=0),
    "order3_la2": dict(df_order=3, df_lookahead=2),
    "skip_none": dict(df_gru_skip="none"),
    "layers2_1": dict(emb_num_layers=2, df_num_layers=1),
    "layers4_3": dict(emb_num_layers=4, df_num_layers=3),
    "lin1_enclin1": dict(lin_groups=1, enc_lin_groups=1),
    "ch16": dict(conv_ch=16),
    "ch32": dict(conv_ch=32),
    "erb4": dict(nb_erb=4),                                                         # e3 one bin wide
    "erb16": dict(nb_erb=16),
    "erb24": dict(nb_erb=24),
    "erb64_min1": dict(nb_erb=64, min_nb_erb_freqs=1),
    "nbdf64": dict(nb_df=64),
    "nbdf480": dict(nb_df=480),
    "tau0.1": dict(norm_tau=0.1),
    "conv_la4": dict(conv_lookahead=4),
    "cornerA": dict(fft_size=1024, hop_size=256, nb_erb=24, nb_df=64, df_order=3, df_lookahead=0, conv_lookahead=0,
                    emb_hidden_dim=128, df_hidden_dim=64, lin_groups=8, enc_lin_groups=16, conv_ch=32, emb_num_layers=2,
                    df_num_layers=1, df_gru_skip="none", df_pathway_kernel_size_t=3),
    "cornerB": dict(fft_size=4096, hop_size=2048, nb_erb=48, nb_df=192, df_order=7, df_lookahead=3, conv_lookahead=3,
                    emb_hidden_dim=252, df_hidden_dim=196, lin_groups=4, enc_lin_groups=16, conv_ch=48, emb_num_layers=4,
                    df_num_layers=3, norm_tau=0.5),
}

# Configurations load() must refuse, with a fragment of the listing error each must carry
REJECTED = {
    "conv_kernel_1_4": (dict(conv_kernel="1,4"), "conv_kernel = (1, 4)"),
    "conv_kernel_inp_3_4": (dict(conv_kernel_inp="3,4"), "conv_kernel_inp = (3, 4)"),
    "convt_kernel_1_5": (dict(convt_kernel="1,5"), "convt_kernel = (1, 5)"),
    "both_kernels_1_5": (dict(conv_kernel="1,5", convt_kernel="1,5"), "convt_kernel = (1, 5)"),
    "convt_kernel_2_3": (dict(convt_kernel="2,3"), "convt_kernel = (2, 3)"),
    "H100_lin16": (dict(emb_hidden_dim=100, df_hidden_dim=100), "do not split over 16 groups"),
    "enc_lin7": (dict(enc_lin_groups=7), "enc.df_fc_emb: 3072 -> 512 features do not split over 7 groups"),
    "H257": (dict(emb_hidden_dim=257), "emb_hidden_dim = 257"),
    "emb_layers1": (dict(emb_num_layers=1), "emb_num_layers = 1"),
    "gru_layers9": (dict(emb_num_layers=5, df_num_layers=4), "9 GRU layers in total"),
    "sr16000": (dict(sr=16000), "sr = 16000"),
    "fft8192": (dict(fft_size=8192, hop_size=4096), "fft_size 8192"),
    "erb68": (dict(nb_erb=68, min_nb_erb_freqs=1), "nb_erb = 68"),
    "nbdf_odd": (dict(nb_df=95), "nb_df = 95"),
    "df_la_ge_order": (dict(df_order=3, df_lookahead=3), "df_lookahead = 3"),
    "tau0": (dict(norm_tau=0), "norm_tau = 0.0"),
}


def config_text(**overrides) -> str:
    """CONFIG_INI with the named keys' values replaced (pairs as "a,b" strings or tuples); an unknown key raises."""
    lines = CONFIG_INI.splitlines()
    left = dict(overrides)
    for i, ln in enumerate(lines):
        k = ln.split("=")[0].strip()
        if "=" in ln and k in left:
            v = left.pop(k)
            if isinstance(v, (tuple, list)):
                v = ",".join(str(int(a)) for a in v)
            lines[i] = f"{k} = {v}"
    if left:
        raise KeyError(f"config_text: no such key in CONFIG_INI: {sorted(left)}")
    return "\n".join(lines) + "\n"


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
    # libdf's band_mean_norm_erb / band_unit_norm take alpha as an f32 and form 1 - alpha in f32: the recursions' coefficients are
    # those two float32 values, in either dtype (the double 1 - alpha differs from them by ~1e-6 relative)
    a = float(np.float32(dw.norm_alpha(cfg)))
    a1 = float(np.float32(1.0) - np.float32(a))
    widths = dw.erb_widths(cfg["sr"], cfg["fft_size"], cfg["nb_erb"], cfg["min_nb_erb_freqs"])
    fb, _ = dw.erb_matrices(widths)
    rdt = spec.real.dtype
    pw = (spec.real ** 2 + spec.imag ** 2) @ fb.to(rdt)
    db = 10.0 * torch.log10(pw + 1e-10)
    E, nbdf = cfg["nb_erb"], cfg["nb_df"]
    s = torch.linspace(-60.0, -90.0, E, dtype=torch.float32).to(rdt).expand(spec.shape[0], E).clone()
    erb = torch.empty_like(db)
    for t in range(db.shape[1]):
        s = db[:, t] * a1 + s * a
        erb[:, t] = (db[:, t] - s) / 40.0
    us = torch.linspace(0.001, 0.0001, nbdf, dtype=torch.float32).to(rdt).expand(spec.shape[0], nbdf).clone()
    cs = spec[:, :, :nbdf]
    cf = torch.empty_like(cs)
    for t in range(cs.shape[1]):
        us = cs[:, t].abs() * a1 + us * a
        cf[:, t] = cs[:, t] / torch.sqrt(us)
    return erb[:, None], torch.stack([cf.real, cf.imag], 1)


def _shift(x: torch.Tensor, la: int) -> torch.Tensor:
    """DfNet.pad_feat: ConstantPad2d((0, 0, -la, la)) on the time axis (dim 2).  When la >= nF every frame is shifted out: all-zero
    features (what k_dfn_norm_scan writes; SPEC.md DFN3-P4), where F.pad would ask for a negative length."""
    if la <= 0:
        return x
    if la >= x.shape[2]:
        return torch.zeros_like(x)
    return F.pad(x, (0, 0, -la, la))


def shifted_features(spec: torch.Tensor, cfg: dict):
    """-> (feat_erb, feat_spec) as the encoder sees them: the norms, then DfNet.pad_feat in the "input*" pad modes."""
    fe, fs = features(spec, cfg)
    la = cfg["conv_lookahead"] if cfg["pad_mode"].startswith("input") else 0
    return _shift(fe, la), _shift(fs, la)


class Net:
    """The network between the features and the enhanced spectrum, one method per stage (tests/test_gpu_dfn3*.py feed each the
    device's own read-back inputs).  Shapes are upstream's: e* / c0 [B, ch, T, F], GRU outputs / emb [B, T, H], mask [B, T, E],
    coefs [B, T, nb_df, 2 df_order]."""

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

    def gru_layer(self, x, prefix, k):
        """Layer k of the torch.nn.GRU stored under prefix."""
        sd = self.sd
        H = sd[prefix + ".weight_hh_l0"].shape[1]
        m = torch.nn.GRU(x.shape[-1], H, num_layers=1, batch_first=True).to(self.dt)
        with torch.no_grad():
            m.weight_ih_l0.copy_(sd[f"{prefix}.weight_ih_l{k}"])
            m.weight_hh_l0.copy_(sd[f"{prefix}.weight_hh_l{k}"])
            m.bias_ih_l0.copy_(sd[f"{prefix}.bias_ih_l{k}"])
            m.bias_hh_l0.copy_(sd[f"{prefix}.bias_hh_l{k}"])
            x, _ = m(x)
        return x

    # ---- encoder
    def e0(self, fe):
        sd = self.sd
        return torch.relu(self.bn(self.conv(fe, sd["enc.erb_conv0.1.weight"]), "enc.erb_conv0.2"))

    def e_next(self, i, e):
        """e_i (i = 1, 2, 3) from e_{i-1}."""
        sd = self.sd
        y = self.conv(e, sd[f"enc.erb_conv{i}.0.weight"], 2 if i < 3 else 1, self.cfg["conv_ch"])
        return torch.relu(self.bn(self.conv(y, sd[f"enc.erb_conv{i}.1.weight"]), f"enc.erb_conv{i}.2"))

    def c0(self, fs):
        sd = self.sd
        return torch.relu(self.bn(self.conv(self.conv(fs, sd["enc.df_conv0.1.weight"], 1, 2), sd["enc.df_conv0.2.weight"]), "enc.df_conv0.3"))

    def gru_enc(self, e3, c0):
        """The encoder's GRU layer: emb0 = e3 + relu(df_fc_emb(df_conv1(c0))) through relu(linear_in)."""
        sd = self.sd
        c1 = torch.relu(self.bn(self.conv(self.conv(c0, sd["enc.df_conv1.0.weight"], 2, self.cfg["conv_ch"]), sd["enc.df_conv1.1.weight"]),
                                "enc.df_conv1.2"))
        cemb = torch.relu(self.gl(c1.permute(0, 2, 3, 1).flatten(2), sd["enc.df_fc_emb.0.weight"]))
        emb = e3.permute(0, 2, 3, 1).flatten(2) + cemb
        x = torch.relu(self.gl(emb, sd["enc.emb_gru.linear_in.0.weight"]))
        return self.gru_layer(x, "enc.emb_gru.gru", 0)

    def emb(self, g0):
        return torch.relu(self.gl(g0, self.sd["enc.emb_gru.linear_out.0.weight"]))

    # ---- ERB decoder
    def erb_gru(self, k, x):
        """ERB-decoder GRU layer k: from emb (through relu(linear_in)) for k = 0, else from layer k - 1."""
        if k == 0:
            x = torch.relu(self.gl(x, self.sd["erb_dec.emb_gru.linear_in.0.weight"]))
        return self.gru_layer(x, "erb_dec.emb_gru.gru", k)

    def mask(self, g, e0, e1, e2, e3):
        """The ERB mask [B, T, E] from the last ERB-decoder GRU layer and the encoder's e0 - e3."""
        sd, C = self.sd, self.cfg["conv_ch"]
        relu = torch.relu
        b, _, t, f8 = e3.shape
        d = relu(self.gl(g, sd["erb_dec.emb_gru.linear_out.0.weight"])).view(b, t, f8, -1).permute(0, 3, 1, 2)

        def p(e, i):                                   # pathway conv: groups = in_ch / (in_ch per group) from the weight shape
            w = sd[f"erb_dec.conv{i}p.0.weight"]
            return relu(self.bn(self.conv(e, w, 1, C // w.shape[1]), f"erb_dec.conv{i}p.1"))
        y = self.conv(p(e3, 3) + d, sd["erb_dec.convt3.0.weight"], 1, C)
        d = relu(self.bn(self.conv(y, sd["erb_dec.convt3.1.weight"]), "erb_dec.convt3.2"))
        for i, e in ((2, e2), (1, e1)):
            y = self.convt(p(e, i) + d, sd[f"erb_dec.convt{i}.0.weight"], 2, C)
            d = relu(self.bn(self.conv(y, sd[f"erb_dec.convt{i}.1.weight"]), f"erb_dec.convt{i}.2"))
        return torch.sigmoid(self.bn(self.conv(p(e0, 0) + d, sd["erb_dec.conv0_out.0.weight"]), "erb_dec.conv0_out.1"))[:, 0]

    # ---- DF decoder
    def df_gru(self, k, x):
        """DF-decoder GRU layer k: from emb (through relu(linear_in)) for k = 0, else from layer k - 1."""
        if k == 0:
            x = torch.relu(self.gl(x, self.sd["df_dec.df_gru.linear_in.0.weight"]))
        return self.gru_layer(x, "df_dec.df_gru.gru", k)

    def coefs(self, c, emb, c0):
        """Deep-filter coefficients [B, T, nb_df, 2 df_order] from the last DF GRU layer, emb (skip) and c0 (pathway)."""
        cfg, sd, C = self.cfg, self.sd, self.cfg["conv_ch"]
        if cfg["df_gru_skip"] == "groupedlinear":
            c = c + self.gl(emb, sd["df_dec.df_skip.weight"])
        b, t = c.shape[:2]
        O2 = 2 * cfg["df_order"]
        gp = C // sd["df_dec.df_convp.1.weight"].shape[1]
        cp = torch.relu(self.bn(self.conv(self.conv(c0, sd["df_dec.df_convp.1.weight"], 1, gp), sd["df_dec.df_convp.2.weight"]),
                                "df_dec.df_convp.3"))
        return torch.tanh(self.gl(c, sd["df_dec.df_out.0.weight"])).view(b, t, cfg["nb_df"], O2) + cp.permute(0, 2, 3, 1)

    # ---- mask + deep filter
    def assemble(self, spec, mask, coefs):
        """spec_e: the ERB mask through the inverse map, bins below nb_df replaced by the deep filter."""
        cfg = self.cfg
        t = spec.shape[1]
        _, inv = W().erb_matrices(W().erb_widths(cfg["sr"], cfg["fft_size"], cfg["nb_erb"], cfg["min_nb_erb_freqs"]))
        spec_m = spec * (mask @ inv.to(self.dt))
        O, L, nb = cfg["df_order"], cfg["df_lookahead"], cfg["nb_df"]
        sp = F.pad(spec[:, :, :nb].transpose(1, 2), (O - 1 - L, L))                 # [B, nb, T + O - 1]
        co = torch.complex(coefs[..., 0::2], coefs[..., 1::2])                      # [B, T, nb, O]
        y = sum(sp[:, :, n:n + t].transpose(1, 2) * co[..., n] for n in range(O))
        out = spec_m.clone()
        out[:, :, :nb] = y
        return out

    def forward(self, spec: torch.Tensor, fe, fs, st: dict):
        """The stages composed; fills st with every intermediate the device reads back."""
        cfg = self.cfg
        es = [self.e0(fe)]
        for i in (1, 2, 3):
            es.append(self.e_next(i, es[-1]))
        e0, e1, e2, e3 = es
        c0 = self.c0(fs)
        grus = [self.gru_enc(e3, c0)]
        emb = self.emb(grus[0])
        x = emb
        for k in range(cfg["emb_num_layers"] - 1):
            x = self.erb_gru(k, x)
            grus.append(x)
        m = self.mask(x, e0, e1, e2, e3)
        x = emb
        for k in range(cfg["df_num_layers"]):
            x = self.df_gru(k, x)
            grus.append(x)
        coefs = self.coefs(x, emb, c0)
        st.update(feat_erb=fe, feat_spec=fs, e0=e0, e1=e1, e2=e2, e3=e3, c0=c0, emb=emb, grus=grus, mask=m, coefs=coefs)
        return self.assemble(spec, m, coefs)


def enhance(x: torch.Tensor, cfg: dict, sd: dict, dtype=torch.float64, stages: bool = False):
    """x [C, T] -> y [C, T] in `dtype` (and the stage dict when `stages`)."""
    x = x.to(dtype)
    st = {}
    spec = analysis(x, cfg)
    fe, fs = shifted_features(spec, cfg)
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
