"""DeepFilterNet2 model directory discovery, config.ini, checkpoint validation and packing for the native denoiser (SPEC.md
"4c. DeepFilterNet2 (UPSTREAM-RECALL)").  Function for function the DeepFilterNet3 module dfn_weights.py, whose helpers (ERB bank,
norm alpha, BatchNorm folding, checkpoint reading, search path) are used as they are.

A directory serves DeepFilterNet2 only when its config.ini names the model (`[train] model = deepfilternet2`, SPEC DFN2-P8), so a
DeepFilterNet3 directory -- EGREGORA_DFN_MODEL_DIR included -- is skipped by this search and never loaded as DeepFilterNet2.
Every hyperparameter comes from config.ini; the layer counts, widths and group counts the checkpoint's tensor shapes imply are
checked against it, and every tensor name and shape against the committed key table `dfn2_keymap.json`.  Anything unmapped,
missing or mismatched raises with the full list.
"""
import configparser
import json
import math
import re
from pathlib import Path
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import dfn_weights
from .dfn_weights import checkpoint_file, erb_matrices, erb_widths, fold_bn, norm_alpha, read_state_dict

MODEL = "DeepFilterNet2"
MODEL_ID = "deepfilternet2"                 # [train] model
KEYMAP_PATH = Path(__file__).resolve().parent / "dfn2_keymap.json"

_INT, _FLOAT, _STR, _BOOL, _PAIR = int, float, str, "bool", "pair"
PARAMS = [
    ("df", "sr", _INT), ("df", "fft_size", _INT), ("df", "hop_size", _INT), ("df", "nb_erb", _INT), ("df", "nb_df", _INT),
    ("df", "norm_tau", _FLOAT), ("df", "lsnr_max", _INT), ("df", "lsnr_min", _INT), ("df", "min_nb_erb_freqs", _INT),
    ("df", "df_order", _INT), ("df", "df_lookahead", _INT),
    ("deepfilternet", "gru_type", _STR), ("deepfilternet", "gru_groups", _INT), ("deepfilternet", "lin_groups", _INT),
    ("deepfilternet", "group_shuffle", _BOOL), ("deepfilternet", "df_output_layer", _STR), ("deepfilternet", "dfop_method", _STR),
    ("deepfilternet", "conv_ch", _INT), ("deepfilternet", "conv_kernel", _PAIR), ("deepfilternet", "conv_kernel_inp", _PAIR),
    ("deepfilternet", "conv_depthwise", _BOOL), ("deepfilternet", "convt_depthwise", _BOOL), ("deepfilternet", "conv_lookahead", _INT),
    ("deepfilternet", "emb_hidden_dim", _INT), ("deepfilternet", "emb_num_layers", _INT), ("deepfilternet", "df_hidden_dim", _INT),
    ("deepfilternet", "df_num_layers", _INT), ("deepfilternet", "df_gru_skip", _STR),
    ("deepfilternet", "df_pathway_kernel_size_t", _INT), ("deepfilternet", "enc_concat", _BOOL), ("deepfilternet", "df_n_iter", _INT),
    ("deepfilternet", "mask_pf", _BOOL),
]
MAX_GRU_LAYERS = dfn_weights.MAX_GRU_LAYERS     # EGR_DFN3_MAX_GRU, shared by egr_dfn2_*
MAX_NB_ERB = dfn_weights.MAX_NB_ERB
DFOP_METHODS = ("real_unfold",)                 # the DFN3-P5 window: sum over df_order taps of the padded spectrum times the coefficients


# ------------------------------------------------------------------------------------------------ discovery
def model_id(d: Path) -> str:
    """`[train] model` of d/config.ini, lower case ('' when absent or unreadable)."""
    cp = configparser.ConfigParser()
    try:
        cp.read(str(Path(d) / "config.ini"), encoding="utf-8")
    except (configparser.Error, OSError, UnicodeDecodeError):
        return ""
    return cp.get("train", "model", fallback="").strip().lower()


def is_model_dir(d: Path) -> bool:
    return dfn_weights.is_model_dir(d) and model_id(d) == MODEL_ID


def discover(model: str = MODEL) -> Optional[Path]:
    """The first of dfn_weights.candidate_dirs("DeepFilterNet2") that holds a DeepFilterNet2 model directory, else None.  The
    function is looked up on the module at call time (tests monkeypatch dfn_weights.pack_root)."""
    if model != MODEL:
        return None
    for d in dfn_weights.candidate_dirs(MODEL):
        if is_model_dir(d):
            return d
    return None


# ------------------------------------------------------------------------------------------------ config
def parse_config(path: Path) -> dict:
    """config.ini -> {key: value} for every entry of PARAMS; raises listing every absent or unreadable key."""
    cp = configparser.ConfigParser()
    cp.read(str(path), encoding="utf-8")
    cfg, bad = {}, []
    for sec, key, typ in PARAMS:
        if not cp.has_option(sec, key):
            bad.append(f"[{sec}] {key}: missing")
            continue
        raw = cp.get(sec, key).strip()
        try:
            if typ == _BOOL:
                v = raw.lower() in ("1", "true", "yes", "on")
                if raw.lower() not in ("1", "0", "true", "false", "yes", "no", "on", "off"):
                    raise ValueError(raw)
            elif typ == _PAIR:
                v = tuple(int(s) for s in raw.split(","))
                if len(v) != 2:
                    raise ValueError(raw)
            elif typ == _STR:
                v = raw.lower()
            else:
                v = typ(raw)
        except ValueError:
            bad.append(f"[{sec}] {key}: cannot read {raw!r}")
            continue
        cfg[key] = v
    if bad:
        raise RuntimeError(f"DeepFilterNet2 config {path} is incomplete:\n  " + "\n  ".join(bad))
    return cfg


def check_supported(cfg: dict):
    """The structure variants the native forward pass implements; anything else raises with the full list.  Accepts exactly what
    egr_dfn2_create and its run accept; every accepted variant runs (tests/test_gpu_dfn2_configs.py)."""
    bad = []
    want = {"gru_type": "grouped", "conv_depthwise": True, "convt_depthwise": True, "enc_concat": False, "df_n_iter": 1,
            "mask_pf": False}
    for k, v in want.items():
        if cfg[k] != v:
            bad.append(f"{k} = {cfg[k]!r} (supported: {v!r})")
    if cfg["dfop_method"] not in DFOP_METHODS:
        bad.append(f"dfop_method = {cfg['dfop_method']!r} (supported: {DFOP_METHODS})")
    if cfg["df_output_layer"] not in ("linear", "groupedlinear"):
        bad.append(f"df_output_layer = {cfg['df_output_layer']!r} (supported: 'linear', 'groupedlinear')")
    if cfg["df_gru_skip"] not in ("none", "groupedlinear"):
        bad.append(f"df_gru_skip = {cfg['df_gru_skip']!r} (supported: 'none', 'groupedlinear')")
    if not cfg["norm_tau"] > 0:
        bad.append(f"norm_tau = {cfg['norm_tau']} (> 0)")
    if cfg["sr"] != 48000:
        bad.append(f"sr = {cfg['sr']} (the node always hands the model a 48 kHz signal)")
    for k in ("conv_kernel", "conv_kernel_inp"):
        kt, kf = cfg[k]
        if kt < 1 or kf < 1 or kf % 2 == 0:
            bad.append(f"{k} = {cfg[k]} (time extent >= 1, odd frequency extent)")
    if cfg["df_pathway_kernel_size_t"] < 1:
        bad.append(f"df_pathway_kernel_size_t = {cfg['df_pathway_kernel_size_t']} (>= 1)")
    if cfg["hop_size"] < 1 or cfg["fft_size"] < 2 or cfg["fft_size"] % cfg["hop_size"] or cfg["fft_size"] % 2 or cfg["fft_size"] > 4096:
        bad.append(f"fft_size {cfg['fft_size']} must be even, <= 4096 and a multiple of hop_size {cfg['hop_size']}")
    if cfg["nb_erb"] < 4 or cfg["nb_erb"] % 4 or cfg["nb_erb"] > MAX_NB_ERB or cfg["nb_df"] < 2 or cfg["nb_df"] % 2:
        bad.append(f"nb_erb = {cfg['nb_erb']} (multiple of 4, <= {MAX_NB_ERB}), nb_df = {cfg['nb_df']} (even)")
    if cfg["nb_df"] > cfg["fft_size"] // 2 + 1:
        bad.append(f"nb_df = {cfg['nb_df']} / fft_size = {cfg['fft_size']} out of range")
    for k in ("emb_hidden_dim", "df_hidden_dim"):
        if not 1 <= cfg[k] <= 256:
            bad.append(f"{k} = {cfg[k]} (the recurrence kernels hold 1 <= H <= 256)")
    n_gru = cfg["emb_num_layers"] + cfg["df_num_layers"]
    if cfg["emb_num_layers"] < 2 or cfg["df_num_layers"] < 1 or n_gru > MAX_GRU_LAYERS:
        bad.append(f"emb_num_layers = {cfg['emb_num_layers']} (>= 2: one encoder layer, at least one ERB-decoder layer), "
                   f"df_num_layers = {cfg['df_num_layers']} (>= 1), {n_gru} GRU layers in total (<= {MAX_GRU_LAYERS})")
    if cfg["df_order"] < 1 or cfg["conv_lookahead"] < 0 or cfg["df_lookahead"] < 0 or cfg["df_lookahead"] > cfg["df_order"] - 1:
        bad.append(f"df_order = {cfg['df_order']}, conv_lookahead = {cfg['conv_lookahead']}, df_lookahead = {cfg['df_lookahead']} "
                   "out of range")
    elif 0 < cfg["conv_lookahead"] < cfg["df_lookahead"]:
        bad.append(f"conv_lookahead = {cfg['conv_lookahead']} (0 or >= df_lookahead = {cfg['df_lookahead']})")
    if cfg["conv_ch"] < 1 or cfg["lin_groups"] < 1 or cfg["gru_groups"] < 1:
        bad.append(f"conv_ch = {cfg['conv_ch']}, lin_groups = {cfg['lin_groups']}, gru_groups = {cfg['gru_groups']} (>= 1)")
    elif not bad:
        emb = cfg["conv_ch"] * cfg["nb_erb"] // 4
        He, Hd, G, Gl = cfg["emb_hidden_dim"], cfg["df_hidden_dim"], cfg["gru_groups"], cfg["lin_groups"]
        # every GroupedGRU splits its input and its width evenly over gru_groups
        for name, i, o in (("enc.emb_gru", emb, He), ("erb_dec.emb_gru", He, He), ("df_dec.df_gru", He, Hd)):
            if i % G or o % G:
                bad.append(f"{name}: {i} -> {o} features do not split over gru_groups = {G}")
        # every GroupedLinear / GroupedLinearEinsum splits its input and its output evenly over lin_groups
        lins = [("enc.df_fc_emb", cfg["conv_ch"] * cfg["nb_df"] // 2, emb), ("erb_dec.fc_emb", He, emb)]
        if cfg["df_gru_skip"] == "groupedlinear":
            lins.append(("df_dec.df_skip", He, Hd))
        if cfg["df_output_layer"] == "groupedlinear":
            lins.append(("df_dec.df_out", Hd, cfg["nb_df"] * 2 * cfg["df_order"]))
        for name, i, o in lins:
            if i % Gl or o % Gl:
                bad.append(f"{name}: {i} -> {o} features do not split over lin_groups = {Gl}")
    if bad:
        raise RuntimeError("DeepFilterNet2 config not supported by the native forward pass:\n  " + "\n  ".join(bad))


def derived_vars(cfg: dict) -> dict:
    """Names the key table's shape expressions use."""
    v = dict(cfg)
    v.update(kt_inp=cfg["conv_kernel_inp"][0], kf_inp=cfg["conv_kernel_inp"][1], kt=cfg["conv_kernel"][0], kf=cfg["conv_kernel"][1],
             n_freqs=cfg["fft_size"] // 2 + 1, emb_dim=cfg["conv_ch"] * cfg["nb_erb"] // 4, df_out_ch=2 * cfg["df_order"],
             df_path_groups=math.gcd(cfg["conv_ch"], 2 * cfg["df_order"]))
    return v


# ------------------------------------------------------------------------------------------------ key table
def expected_table(cfg: dict, keymap_path: Optional[Path] = None) -> Dict[str, Tuple[int, ...]]:
    """{tensor name: shape} the key table prescribes for this config."""
    spec = json.loads(Path(keymap_path or KEYMAP_PATH).read_text(encoding="utf-8"))
    env = derived_vars(cfg)
    ev = lambda s: int(eval(str(s), {"__builtins__": {}}, env))      # noqa: S307 (repo-owned JSON, integer expressions)
    out = {}
    for e in spec["entries"]:
        if "when" in e and not eval(e["when"], {"__builtins__": {}}, env):  # noqa: S307
            continue
        shape = tuple(ev(s) for s in e["shape"])
        ls = range(ev(e["l"][0]), ev(e["l"][1])) if "l" in e else [None]
        gs = range(env[e["g"]]) if "g" in e else [None]
        for l in ls:
            for g in gs:
                out[e["name"].replace("{l}", str(l)).replace("{g}", str(g))] = shape
    return out


def _count(sd, pattern: str) -> int:
    """Distinct values of the single (\\d+) group of pattern among the tensor names."""
    return len({m.group(1) for k in sd for m in [re.fullmatch(pattern, k)] if m})


def layer_table(sd: Dict[str, torch.Tensor]) -> dict:
    """Layer counts, widths and group counts read from the tensor shapes alone (no config)."""
    t = {}
    def get(name):
        return sd[name].shape if name in sd else None
    s = get("enc.erb_conv0.1.weight")
    if s is not None:
        t["conv_ch"], t["conv_kernel_inp"] = int(s[0]), (int(s[2]), int(s[3]))
    s = get("enc.erb_conv1.0.weight")
    if s is not None:
        t["conv_kernel"] = (int(s[2]), int(s[3]))
    s = get("erb_fb")
    if s is not None:
        t["fft_size"], t["nb_erb"] = 2 * (int(s[0]) - 1), int(s[1])
    G = _count(sd, r"enc\.emb_gru\.grus\.0\.layers\.(\d+)\.weight_hh_l0")
    if G:
        t["gru_groups"] = G
        t["emb_hidden_dim"] = G * int(sd["enc.emb_gru.grus.0.layers.0.weight_hh_l0"].shape[1])
    s = get("df_dec.df_gru.grus.0.layers.0.weight_hh_l0")
    if s is not None and G:
        t["df_hidden_dim"] = G * int(s[1])
    t["emb_num_layers"] = _count(sd, r"enc\.emb_gru\.grus\.(\d+)\..*") + _count(sd, r"erb_dec\.emb_gru\.grus\.(\d+)\..*")
    t["df_num_layers"] = _count(sd, r"df_dec\.df_gru\.grus\.(\d+)\..*")
    Gl = _count(sd, r"enc\.df_fc_emb\.layers\.(\d+)\.weight")
    if Gl:
        t["lin_groups"] = Gl
        if "conv_ch" in t:
            t["nb_df"] = 2 * Gl * int(sd["enc.df_fc_emb.layers.0.weight"].shape[1]) // t["conv_ch"]
    s = get("df_dec.df_convp.1.weight")
    if s is not None:
        t["df_order"], t["df_pathway_kernel_size_t"] = int(s[0]) // 2, int(s[2])
    t["df_gru_skip"] = "groupedlinear" if "df_dec.df_skip.weight" in sd else "none"
    s = get("df_dec.df_out.0.weight")
    if s is not None:
        t["df_output_layer"] = "linear" if "df_dec.df_out.0.bias" in sd else "groupedlinear"
    return t


def validate(sd: Dict[str, torch.Tensor], cfg: dict, keymap_path: Optional[Path] = None):
    """Raise with every unmapped / missing / mismatched tensor and every config field the shapes contradict."""
    want = expected_table(cfg, keymap_path)
    unmapped = sorted(k for k in sd if k not in want)
    missing = sorted(k for k in want if k not in sd)
    wrong = sorted(f"{k}: checkpoint {tuple(sd[k].shape)} != table {want[k]}" for k in want if k in sd and tuple(sd[k].shape) != want[k])
    lt = layer_table(sd)
    conflict = sorted(f"{k}: shapes say {v!r}, config.ini says {cfg[k]!r}" for k, v in lt.items() if k in cfg and cfg[k] != v)
    if unmapped or missing or wrong or conflict:
        parts = []
        for title, lst in (("unmapped tensors", unmapped), ("missing tensors", missing), ("shape mismatches", wrong),
                           ("config / checkpoint disagreements", conflict)):
            if lst:
                parts.append(f"{title} ({len(lst)}):\n    " + "\n    ".join(lst))
        raise RuntimeError("DeepFilterNet2 checkpoint does not match dfn2_keymap.json / config.ini:\n  " + "\n  ".join(parts))
    widths = erb_widths(cfg["sr"], cfg["fft_size"], cfg["nb_erb"], cfg["min_nb_erb_freqs"])
    fb, ifb = erb_matrices(widths)
    if not (torch.allclose(sd["erb_fb"].float(), fb, atol=1e-6) and torch.allclose(sd["mask.erb_inv_fb"].float(), ifb, atol=1e-6)):
        raise RuntimeError(f"DeepFilterNet2 checkpoint: erb_fb / mask.erb_inv_fb differ from the ERB bank of config.ini (widths {widths})")


# ------------------------------------------------------------------------------------------------ packing
def pack_order(cfg: dict) -> List[Tuple[str, str]]:
    """(tensor name, kind) in the order egr_dfn2_create reads them (csrc/egr_dfn3.hip, egr_dfn2_create).  kind "w": the tensor as
    stored (torch layout, fp32); "bn": a BatchNorm folded to eval-mode per-channel scale then shift.  A grouped module's tensors
    come group after group for each parameter, so each parameter is one [G][...] block."""
    G, Gl = cfg["gru_groups"], cfg["lin_groups"]
    o = [("enc.erb_conv0.1.weight", "w"), ("enc.erb_conv0.2", "bn")]
    for i in (1, 2, 3):
        o += [(f"enc.erb_conv{i}.0.weight", "w"), (f"enc.erb_conv{i}.1.weight", "w"), (f"enc.erb_conv{i}.2", "bn")]
    o += [("enc.df_conv0.1.weight", "w"), ("enc.df_conv0.2.weight", "w"), ("enc.df_conv0.3", "bn"),
          ("enc.df_conv1.0.weight", "w"), ("enc.df_conv1.1.weight", "w"), ("enc.df_conv1.2", "bn")]

    def glin(prefix):
        return [(f"{prefix}.layers.{g}.{p}", "w") for p in ("weight", "bias") for g in range(Gl)]

    def ggru(prefix, n):
        return [(f"{prefix}.grus.{l}.layers.{g}.{p}", "w") for l in range(n)
                for p in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0") for g in range(G)]
    o += glin("enc.df_fc_emb") + ggru("enc.emb_gru", 1)
    o += ggru("erb_dec.emb_gru", cfg["emb_num_layers"] - 1) + glin("erb_dec.fc_emb.0")
    for i in (3, 2, 1):
        o += [(f"erb_dec.conv{i}p.0.weight", "w"), (f"erb_dec.conv{i}p.1", "bn"), (f"erb_dec.convt{i}.0.weight", "w"),
              (f"erb_dec.convt{i}.1.weight", "w"), (f"erb_dec.convt{i}.2", "bn")]
    o += [("erb_dec.conv0p.0.weight", "w"), ("erb_dec.conv0p.1", "bn"), ("erb_dec.conv0_out.0.weight", "w"), ("erb_dec.conv0_out.1", "bn")]
    o += ggru("df_dec.df_gru", cfg["df_num_layers"])
    if cfg["df_gru_skip"] == "groupedlinear":
        o += [("df_dec.df_skip.weight", "w")]
    o += [("df_dec.df_out.0.weight", "w")]
    if cfg["df_output_layer"] == "linear":
        o += [("df_dec.df_out.0.bias", "w")]
    o += [("df_dec.df_fc_a.0.weight", "w"), ("df_dec.df_fc_a.0.bias", "w")]
    o += [("df_dec.df_convp.1.weight", "w"), ("df_dec.df_convp.2.weight", "w"), ("df_dec.df_convp.3", "bn")]
    return o


def pack(sd: Dict[str, torch.Tensor], cfg: dict) -> np.ndarray:
    parts = []
    for name, kind in pack_order(cfg):
        if kind == "bn":
            s, t = fold_bn(sd, name)
            parts += [s.float().reshape(-1), t.float().reshape(-1)]
        else:
            parts.append(sd[name].float().reshape(-1))
    return torch.cat(parts).numpy().astype(np.float32)


class DFN2Model:
    """A validated DeepFilterNet2 model directory: config (dict), state dict, ERB widths, norm alpha, packed fp32 weights."""

    def __init__(self, cfg: dict, sd: Dict[str, torch.Tensor], directory: Optional[Path] = None):
        check_supported(cfg)
        validate(sd, cfg)
        self.cfg, self.sd, self.dir = cfg, sd, directory
        self.widths = erb_widths(cfg["sr"], cfg["fft_size"], cfg["nb_erb"], cfg["min_nb_erb_freqs"])
        self.alpha = norm_alpha(cfg)

    def packed(self) -> np.ndarray:
        return pack(self.sd, self.cfg)


def load(model_dir: Optional[Path] = None) -> DFN2Model:
    d = Path(model_dir) if model_dir else discover()
    if d is None:
        raise RuntimeError("no DeepFilterNet2 model directory found; searched:\n  " +
                           "\n  ".join(map(str, dfn_weights.candidate_dirs(MODEL))))
    ck = checkpoint_file(d)
    if not (d / "config.ini").is_file() or ck is None:
        raise RuntimeError(f"{d} is not a DeepFilterNet model directory (config.ini + checkpoints/*.ckpt.best)")
    if model_id(d) != MODEL_ID:
        raise RuntimeError(f"{d} holds [train] model = {model_id(d)!r}, not {MODEL_ID!r}")
    return DFN2Model(parse_config(d / "config.ini"), read_state_dict(ck), d)
