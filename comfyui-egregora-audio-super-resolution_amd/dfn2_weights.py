"""DeepFilterNet2 model directory discovery, config.ini, checkpoint validation and packing for the native denoiser (SPEC.md
"4c. DeepFilterNet2 (UPSTREAM-RECALL)").  Everything the two models share (config parsing, the key-table and checkpoint checks, the
ERB bank, norm alpha, BatchNorm folding, packing, the search path) is dfn_weights.py's; this module holds what is DeepFilterNet2's.

A directory serves DeepFilterNet2 only when its config.ini names the model (`[train] model = deepfilternet2`, SPEC DFN2-P8), so a
DeepFilterNet3 directory -- EGREGORA_DFN_MODEL_DIR included -- is skipped by this search and never loaded as DeepFilterNet2.
Every hyperparameter comes from config.ini; the layer counts, widths and group counts the checkpoint's tensor shapes imply are
checked against it, and every tensor name and shape against the committed key table `dfn2_keymap.json`.  Anything unmapped,
missing or mismatched raises with the full list.
"""
import configparser
import math
import re
import sys
from pathlib import Path
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import dfn_weights
from .dfn_weights import checkpoint_file, erb_matrices, erb_widths, fold_bn, norm_alpha, read_state_dict  # noqa: F401 (kept importable here)

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
    return dfn_weights.parse_config(path, PARAMS, MODEL)


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
    dfn_weights.check_common(cfg, bad, "the recurrence kernels hold")
    if 0 < cfg["conv_lookahead"] < cfg["df_lookahead"] <= cfg["df_order"] - 1:
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
    return dfn_weights.expected_table(cfg, keymap_path or KEYMAP_PATH, derived_vars(cfg))


def _count(sd, pattern: str) -> int:
    """Distinct values of the single (\\d+) group of pattern among the tensor names."""
    return len({m.group(1) for k in sd for m in [re.fullmatch(pattern, k)] if m})


def layer_table(sd: Dict[str, torch.Tensor]) -> dict:
    """Layer counts, widths and group counts read from the tensor shapes alone (no config)."""
    t = dfn_weights.layer_table_common(sd)
    def get(name):
        return sd[name].shape if name in sd else None
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
    s = get("df_dec.df_out.0.weight")
    if s is not None:
        t["df_output_layer"] = "linear" if "df_dec.df_out.0.bias" in sd else "groupedlinear"
    return t


def validate(sd: Dict[str, torch.Tensor], cfg: dict, keymap_path: Optional[Path] = None):
    """Raise with every unmapped / missing / mismatched tensor and every config field the shapes contradict."""
    dfn_weights.validate_against(sd, cfg, expected_table(cfg, keymap_path), layer_table(sd), MODEL, KEYMAP_PATH.name)


# ------------------------------------------------------------------------------------------------ packing
def pack_order(cfg: dict) -> List[Tuple[str, str]]:
    """(tensor name, kind) in the order egr_dfn2_create reads them (csrc/egr_dfn3.hip, egr_dfn2_create).  kind "w": the tensor as
    stored (torch layout, fp32); "bn": a BatchNorm folded to eval-mode per-channel scale then shift.  A grouped module's tensors
    come group after group for each parameter, so each parameter is one [G][...] block."""
    G, Gl = cfg["gru_groups"], cfg["lin_groups"]

    def glin(prefix):
        return [(f"{prefix}.layers.{g}.{p}", "w") for p in ("weight", "bias") for g in range(Gl)]

    def ggru(prefix, n):
        return [(f"{prefix}.grus.{l}.layers.{g}.{p}", "w") for l in range(n)
                for p in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0") for g in range(G)]
    o = dfn_weights.encoder_order() + glin("enc.df_fc_emb") + ggru("enc.emb_gru", 1)
    o += ggru("erb_dec.emb_gru", cfg["emb_num_layers"] - 1) + glin("erb_dec.fc_emb.0")
    o += dfn_weights.erb_decoder_order() + ggru("df_dec.df_gru", cfg["df_num_layers"])
    if cfg["df_gru_skip"] == "groupedlinear":
        o += [("df_dec.df_skip.weight", "w")]
    o += [("df_dec.df_out.0.weight", "w")]
    if cfg["df_output_layer"] == "linear":
        o += [("df_dec.df_out.0.bias", "w")]
    return o + [("df_dec.df_fc_a.0.weight", "w"), ("df_dec.df_fc_a.0.bias", "w")] + dfn_weights.DF_PATHWAY_ORDER


def pack(sd: Dict[str, torch.Tensor], cfg: dict) -> np.ndarray:
    return dfn_weights.pack_tensors(sd, pack_order(cfg))


class DFN2Model(dfn_weights.Model):
    weights = sys.modules[__name__]


def load(model_dir: Optional[Path] = None) -> DFN2Model:
    d, ck = dfn_weights.model_files(model_dir, None if model_dir else discover(), MODEL)
    if model_id(d) != MODEL_ID:
        raise RuntimeError(f"{d} holds [train] model = {model_id(d)!r}, not {MODEL_ID!r}")
    return DFN2Model(parse_config(d / "config.ini"), read_state_dict(ck), d)
