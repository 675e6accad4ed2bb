"""Plain-PyTorch restatement of DeepFilterNet2 as `df.enhance.enhance(model, df_state, x)` runs it (SPEC.md "4c. DeepFilterNet2
(UPSTREAM-RECALL)"), in float32 or float64, in the upstream modules' own NCHW shapes.  The signal path (analysis, features with
their norms, the lookahead shift, synthesis) and the convolution helpers are dfn3_torch's; what is DeepFilterNet2's own is here:
GroupedLinear (P3), GroupedGRU (P4, one torch.nn.GRU per group), the decoders (P5, P6) and mask-then-deep-filter with alpha (P7).

It is the yardstick of tests/test_gpu_dfn2*.py and a `set_enhancer` backend for the node tests, and builds the synthetic model
directories the tests use: a config.ini after the recalled DeepFilterNet2 default (UNVERIFIED against a released config.ini) and a
seeded random state dict with the key table's names and shapes.
"""
import math
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

from dfn3_torch import Net as Net3
from dfn3_torch import _shift, analysis, features, synthesis  # noqa: F401 (re-exported for the DFN2 tests)

# The recalled DeepFilterNet2 default (UNVERIFIED): [df] as DeepFilterNet3's default, [deepfilternet] the DeepFilterNet2 keys.
CONFIG_INI = """[train]
model = deepfilternet2

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
conv_kernel_inp = 3,3
emb_hidden_dim = 256
emb_num_layers = 3
df_hidden_dim = 256
df_num_layers = 2
gru_type = grouped
gru_groups = 8
lin_groups = 8
group_shuffle = False
df_output_layer = groupedlinear
df_gru_skip = none
df_pathway_kernel_size_t = 5
dfop_method = real_unfold
enc_concat = False
df_n_iter = 1
mask_pf = False
"""

# The configurations the native forward pass claims (dfn2_weights.check_supported), each a config_text override set; every entry
# changes one axis from the default unless its name says otherwise.  tests/test_gpu_dfn2_configs.py runs each on the device,
# tests/test_dfn2_weights.py loads each and runs it through this restatement.
MATRIX2 = {
    "gru_groups1": dict(gru_groups=1),                                              # one dense layer per GroupedGRU layer, H = 256
    "gru_groups2": dict(gru_groups=2),
    "gru_groups4": dict(gru_groups=4),
    "gru_groups16": dict(gru_groups=16),
    "lin_groups1": dict(lin_groups=1),
    "lin_groups4": dict(lin_groups=4),
    "shuffle": dict(group_shuffle=True),
    "h12": dict(emb_hidden_dim=96, df_hidden_dim=96),                               # h = H / G = 12, not a multiple of 16
    "H256_128": dict(df_hidden_dim=128),                                            # emb_hidden_dim != df_hidden_dim
    "df_out_linear": dict(df_output_layer="linear"),
    "skip_grouped": dict(df_gru_skip="groupedlinear"),
    "layers2_1": dict(emb_num_layers=2, df_num_layers=1),
    "layers4_3": dict(emb_num_layers=4, df_num_layers=3),
    "hop240": dict(hop_size=240),
    "fft512_nbdf64": dict(fft_size=512, hop_size=256, nb_df=64),
    "fft4096": dict(fft_size=4096, hop_size=1024),
    "conv_la0": dict(conv_lookahead=0),
    "conv_la4": dict(conv_lookahead=4),
    "order3_la1": dict(df_order=3, df_lookahead=1),
    "erb16": dict(nb_erb=16),
    "nbdf480": dict(nb_df=480),
    "ch16": dict(conv_ch=16),
    "conv_kernel_2_3": dict(conv_kernel="2,3"),
    "pathway_kt1": dict(df_pathway_kernel_size_t=1),
    "tau0.1": dict(norm_tau=0.1),
    "cornerA": dict(fft_size=1024, hop_size=256, nb_erb=24, nb_df=64, df_order=3, df_lookahead=0, conv_lookahead=0, conv_ch=32,
                    emb_hidden_dim=128, df_hidden_dim=64, gru_groups=4, lin_groups=2, group_shuffle=True, emb_num_layers=2,
                    df_num_layers=1, df_gru_skip="groupedlinear", df_output_layer="linear", df_pathway_kernel_size_t=3),
    "cornerB": dict(fft_size=4096, hop_size=2048, nb_erb=48, nb_df=192, df_order=7, df_lookahead=3, conv_lookahead=3, conv_ch=48,
                    emb_hidden_dim=192, df_hidden_dim=96, gru_groups=16, lin_groups=4, group_shuffle=True, emb_num_layers=4,
                    df_num_layers=3, norm_tau=0.5, conv_kernel="2,3"),
}

# Configurations load() must refuse, with a fragment of the listing error each must carry
REJECTED2 = {
    "squeeze": (dict(gru_type="squeeze"), "gru_type = 'squeeze'"),
    "gru_groups3": (dict(gru_groups=3), "do not split over gru_groups = 3"),
    "lin_groups7": (dict(lin_groups=7), "do not split over lin_groups = 7"),
    "df_n_iter2": (dict(df_n_iter=2), "df_n_iter = 2"),
    "enc_concat": (dict(enc_concat=True), "enc_concat = True"),
    "mask_pf": (dict(mask_pf=True), "mask_pf = True"),
    "conv_la1_df_la2": (dict(conv_lookahead=1), "conv_lookahead = 1 (0 or >= df_lookahead = 2)"),
    "df_out_conv": (dict(df_output_layer="conv"), "df_output_layer = 'conv'"),
    "skip_identity": (dict(df_gru_skip="identity"), "df_gru_skip = 'identity'"),
    "H257": (dict(emb_hidden_dim=257), "emb_hidden_dim = 257"),
    "gru_layers9": (dict(emb_num_layers=5, df_num_layers=4), "9 GRU layers in total"),
    "dfop_complex": (dict(dfop_method="complex_strided"), "dfop_method = 'complex_strided'"),
    "sr16000": (dict(sr=16000), "sr = 16000"),
    "conv_kernel_1_4": (dict(conv_kernel="1,4"), "conv_kernel = (1, 4)"),
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
    from egregora_amd import dfn2_weights
    return dfn2_weights


def synthetic_state_dict(cfg: dict, seed: int = 0):
    """Seeded random tensors with the key table's names and shapes (PyTorch-default-like uniform fan-in scaling)."""
    dw = W()
    g = torch.Generator().manual_seed(seed)
    u = lambda shape, a: (torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * a
    fb, ifb = dw.erb_matrices(dw.erb_widths(cfg["sr"], cfg["fft_size"], cfg["nb_erb"], cfg["min_nb_erb_freqs"]))
    table = dw.expected_table(cfg)
    sd = {}
    for name, shape in table.items():
        is_bn = any(name.endswith(s) for s in (".running_mean", ".running_var", ".num_batches_tracked")) or \
            (len(shape) == 1 and name.rsplit(".", 1)[0] + ".running_mean" in table)
        if name == "erb_fb":
            t = fb.double()
        elif name == "mask.erb_inv_fb":
            t = ifb.double()
        elif name.endswith("num_batches_tracked"):
            sd[name] = torch.tensor(0, dtype=torch.int64)
            continue
        elif name.endswith("running_mean") or (is_bn and name.endswith(".bias")):
            t = u(shape, 0.1)
        elif name.endswith("running_var"):
            t = 0.5 + torch.rand(shape, generator=g, dtype=torch.float64)
        elif is_bn:                                                                    # BatchNorm weight
            t = 0.8 + 0.4 * torch.rand(shape, generator=g, dtype=torch.float64)
        elif ".grus." in name:                                                         # nn.GRU: U(-1/sqrt(h), 1/sqrt(h))
            t = u(shape, 1.0 / math.sqrt(table[name.rsplit(".", 1)[0] + ".weight_hh_l0"][1]))
        elif name.endswith(".bias"):                                                   # nn.Linear bias: U(-1/sqrt(fan_in))
            t = u(shape, 1.0 / math.sqrt(table[name[:-5] + ".weight"][-1]))
        elif len(shape) == 3:                                                          # GroupedLinearEinsum [G, I, H/G]
            t = u(shape, 1.0 / math.sqrt(shape[1]))
        else:                                                                          # conv / linear
            t = u(shape, 1.0 / math.sqrt(max(1, int(np.prod(shape[1:])))))
        sd[name] = t.float()
    return sd


def write_model_dir(d: Path, seed: int = 0, cfg_text: str = CONFIG_INI, epoch: int = 96):
    """A DeepFilterNet2 model directory (config.ini + checkpoints/model_<epoch>.ckpt.best) -> (cfg, state dict)."""
    d = Path(d)
    (d / "checkpoints").mkdir(parents=True, exist_ok=True)
    (d / "config.ini").write_text(cfg_text, encoding="utf-8")
    cfg = W().parse_config(d / "config.ini")
    sd = synthetic_state_dict(cfg, seed)
    torch.save(sd, d / "checkpoints" / f"model_{epoch}.ckpt.best")
    return cfg, sd


# ------------------------------------------------------------------------------------------------ signal path
def shifted_features(spec: torch.Tensor, cfg: dict):
    """-> (feat_erb, feat_spec) as the encoder sees them: the norms, then DfNet's ConstantPad2d((0, 0, -la, la)) whenever
    conv_lookahead > 0 (SPEC DFN2-P1; pad_mode is not read)."""
    fe, fs = features(spec, cfg)
    la = cfg["conv_lookahead"]
    return _shift(fe, la), _shift(fs, la)


def shuffle(x: torch.Tensor, G: int) -> torch.Tensor:
    """SPEC DFN2-P3: output index g h + j takes pre-shuffle index j G + g (x.view(..., h, G).transpose(-1, -2))."""
    if G <= 1:
        return x
    shp = x.shape
    return x.reshape(*shp[:-1], shp[-1] // G, G).transpose(-1, -2).reshape(shp)


class Net2(Net3):
    """The DeepFilterNet2 network between the features and the enhanced spectrum, one method per stage.  The encoder convs, the
    ERB decoder's pathway / transposed convs and the DF pathway conv are DeepFilterNet3's (dfn3_torch.Net)."""

    def glin(self, x, prefix, G, shuf):
        """GroupedLinear (SPEC DFN2-P3): one nn.Linear with bias per group, then the shuffle when shuf and G > 1."""
        sd = self.sd
        I = x.shape[-1] // G
        y = torch.cat([F.linear(x[..., g * I:(g + 1) * I], sd[f"{prefix}.layers.{g}.weight"], sd[f"{prefix}.layers.{g}.bias"])
                       for g in range(G)], -1)
        return shuffle(y, G) if shuf else y

    def ggru_layer(self, x, prefix, l):
        """Layer l of a GroupedGRU (SPEC DFN2-P4) before the inter-layer shuffle: G torch.nn.GRU on the input slices, h0 = 0."""
        sd, G = self.sd, self.cfg["gru_groups"]
        I = x.shape[-1] // G
        outs = []
        for g in range(G):
            p = f"{prefix}.grus.{l}.layers.{g}"
            h = sd[p + ".weight_hh_l0"].shape[1]
            m = torch.nn.GRU(I, h, num_layers=1, batch_first=True).to(self.dt)
            with torch.no_grad():
                for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"):
                    getattr(m, n).copy_(sd[f"{p}.{n}"])
                y, _ = m(x[..., g * I:(g + 1) * I])
            outs.append(y)
        return torch.cat(outs, -1)

    def ggru_step(self, x, prefix, l, n_layers, acc):
        """One GroupedGRU layer as the node composes it: -> (layer output after the P4 shuffle, running sum of layer outputs)."""
        cfg = self.cfg
        y = self.ggru_layer(x, prefix, l)
        if cfg["group_shuffle"] and l < n_layers - 1:
            y = shuffle(y, cfg["gru_groups"])
        return y, (y if acc is None else acc + y)

    def ggru(self, x, prefix, n_layers):
        """GroupedGRU(add_outputs=True): -> (list of layer outputs, list of running sums); the module output is the last sum."""
        ys, ss, acc = [], [], None
        for l in range(n_layers):
            x, acc = self.ggru_step(x, prefix, l, n_layers, acc)
            ys.append(x)
            ss.append(acc)
        return ys, ss

    # ---- encoder (SPEC DFN2-P2)
    def emb_in(self, e3, c0):
        """emb = e3 flattened + GroupedLinear(df_conv1(c0) flattened) (no activation): the encoder GroupedGRU's input."""
        sd, cfg = self.sd, self.cfg
        c1 = torch.relu(self.bn(self.conv(self.conv(c0, sd["enc.df_conv1.0.weight"], 2, cfg["conv_ch"]), sd["enc.df_conv1.1.weight"]),
                                "enc.df_conv1.2"))
        cemb = self.glin(c1.permute(0, 2, 3, 1).flatten(2), "enc.df_fc_emb", cfg["lin_groups"], cfg["group_shuffle"])
        return e3.permute(0, 2, 3, 1).flatten(2) + cemb

    # ---- ERB decoder (SPEC DFN2-P5)
    def mask2(self, s, e0, e1, e2, e3):
        """The ERB mask [B, T, E] from the ERB decoder's GroupedGRU output s and the encoder's e0 - e3."""
        sd, cfg, C = self.sd, self.cfg, self.cfg["conv_ch"]
        relu = torch.relu
        b, _, t, f8 = e3.shape
        d = relu(self.glin(s, "erb_dec.fc_emb.0", cfg["lin_groups"], cfg["group_shuffle"])).view(b, t, f8, -1).permute(0, 3, 1, 2)

        def p(e, i):
            w = sd[f"erb_dec.conv{i}p.0.weight"]
            return relu(self.bn(self.conv(e, w, 1, C // w.shape[1]), f"erb_dec.conv{i}p.1"))
        y = self.conv(p(e3, 3) + d, sd["erb_dec.convt3.0.weight"], 1, C)
        d = relu(self.bn(self.conv(y, sd["erb_dec.convt3.1.weight"]), "erb_dec.convt3.2"))
        for i, e in ((2, e2), (1, e1)):
            y = self.convt(p(e, i) + d, sd[f"erb_dec.convt{i}.0.weight"], 2, C)
            d = relu(self.bn(self.conv(y, sd[f"erb_dec.convt{i}.1.weight"]), f"erb_dec.convt{i}.2"))
        return torch.sigmoid(self.bn(self.conv(p(e0, 0) + d, sd["erb_dec.conv0_out.0.weight"]), "erb_dec.conv0_out.1"))[:, 0]

    # ---- DF decoder (SPEC DFN2-P6)
    def df_c(self, s, emb):
        """c = the DF GroupedGRU output s (+ the GroupedLinearEinsum skip of emb)."""
        if self.cfg["df_gru_skip"] == "groupedlinear":
            return s + self.gl(emb, self.sd["df_dec.df_skip.weight"])
        return s

    def alpha(self, c):
        """alpha [B, T] = sigmoid(Linear(H_df -> 1)(c))."""
        sd = self.sd
        return torch.sigmoid(F.linear(c, sd["df_dec.df_fc_a.0.weight"], sd["df_dec.df_fc_a.0.bias"]))[..., 0]

    def coefs2(self, c, c0):
        """Deep-filter coefficients [B, T, nb_df, 2 df_order]: tanh(df_out(c)) + the df_convp pathway of c0."""
        cfg, sd, C = self.cfg, self.sd, self.cfg["conv_ch"]
        b, t = c.shape[:2]
        O2 = 2 * cfg["df_order"]
        gp = C // sd["df_dec.df_convp.1.weight"].shape[1]
        cp = torch.relu(self.bn(self.conv(self.conv(c0, sd["df_dec.df_convp.1.weight"], 1, gp), sd["df_dec.df_convp.2.weight"]),
                                "df_dec.df_convp.3"))
        if cfg["df_output_layer"] == "linear":
            o = F.linear(c, sd["df_dec.df_out.0.weight"], sd["df_dec.df_out.0.bias"])
        else:
            o = self.gl(c, sd["df_dec.df_out.0.weight"])
        return torch.tanh(o).view(b, t, cfg["nb_df"], O2) + cp.permute(0, 2, 3, 1)

    # ---- mask, then deep filter (SPEC DFN2-P7)
    def assemble2(self, spec, mask, coefs, alpha):
        cfg = self.cfg
        t = spec.shape[1]
        _, inv = W().erb_matrices(W().erb_widths(cfg["sr"], cfg["fft_size"], cfg["nb_erb"], cfg["min_nb_erb_freqs"]))
        spec_m = spec * (mask @ inv.to(self.dt))
        O, L, nb = cfg["df_order"], cfg["df_lookahead"], cfg["nb_df"]
        sf = spec_m[:, :, :nb]
        sp = F.pad(sf.transpose(1, 2), (O - 1 - L, L))                              # [B, nb, T + O - 1]
        co = torch.complex(coefs[..., 0::2], coefs[..., 1::2])                      # [B, T, nb, O]
        y = sum(sp[:, :, n:n + t].transpose(1, 2) * co[..., n] for n in range(O))
        a = alpha[..., None]
        out = spec_m.clone()
        out[:, :, :nb] = y * a + sf * (1 - a)
        return out

    def forward(self, spec: torch.Tensor, fe, fs, st: dict):
        """The stages composed; fills st with every intermediate the device reads back."""
        cfg = self.cfg
        es = [self.e0(fe)]
        for i in (1, 2, 3):
            es.append(self.e_next(i, es[-1]))
        e0, e1, e2, e3 = es
        c0 = self.c0(fs)
        ys, ss = self.ggru(self.emb_in(e3, c0), "enc.emb_gru", 1)
        emb = ss[-1]
        y2, s2 = self.ggru(emb, "erb_dec.emb_gru", cfg["emb_num_layers"] - 1)
        m = self.mask2(s2[-1], e0, e1, e2, e3)
        y3, s3 = self.ggru(emb, "df_dec.df_gru", cfg["df_num_layers"])
        c = self.df_c(s3[-1], emb)
        alpha = self.alpha(c)
        coefs = self.coefs2(c, c0)
        st.update(feat_erb=fe, feat_spec=fs, e0=e0, e1=e1, e2=e2, e3=e3, c0=c0, emb=emb, grus=ys + y2 + y3, sums=ss + s2 + s3, mask=m,
                  coefs=coefs, alpha=alpha)
        return self.assemble2(spec, m, coefs, alpha)


def enhance(x: torch.Tensor, cfg: dict, sd: dict, dtype=torch.float64, stages: bool = False):
    """x [C, T] -> y [C, T] in `dtype` (and the stage dict when `stages`)."""
    x = x.to(dtype)
    st = {}
    spec = analysis(x, cfg)
    fe, fs = shifted_features(spec, cfg)
    spec_e = Net2(cfg, sd, dtype).forward(spec, fe, fs, st)
    y = synthesis(spec_e, cfg, x.shape[1])
    st.update(spec=spec, spec_e=spec_e, y=y)
    return (y, st) if stages else y


def enhancer(cfg: dict, sd: dict, dtype=torch.float32):
    """A set_enhancer backend: fn(x48 [1, T], model_name) -> [1, T] float32."""
    def fn(x, model_name=""):
        with torch.no_grad():
            return enhance(x.detach().cpu().float(), cfg, sd, dtype).float()
    return fn
