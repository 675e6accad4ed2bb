"""DeepFilterNet3 model directory discovery, config.ini, checkpoint validation and packing for the native denoiser
(SPEC.md "DeepFilterNet3 (UPSTREAM-RECALL)").

A model directory is what upstream's `df` keeps per model: `config.ini` plus `checkpoints/*.ckpt.best` (a state dict saved
with torch.save).  It is looked for, in this order, in
  1. EGREGORA_DFN_MODEL_DIR
  2. models/audio/deepfilternet/<model> at both places `models/` can mean (flashsr_weights.candidate_dirs, quirk Q2)
  3. df's own cache, ~/.cache/DeepFilterNet/<model>
No download is attempted.  Every hyperparameter comes from config.ini; the layer counts and widths the checkpoint's tensor
shapes imply are checked against it, and every tensor name and shape against the committed key table `dfn3_keymap.json`.
Anything unmapped, missing or mismatched raises with the full list.
"""
import configparser
import json
import math
import os
import re
import sys
from pathlib import Path
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

MODEL = "DeepFilterNet3"
KEYMAP_PATH = Path(__file__).resolve().parent / "dfn3_keymap.json"
BN_EPS = 1e-5

# (section, key, type) of every hyperparameter the forward pass reads; all must be present in config.ini
_INT, _FLOAT, _STR, _BOOL, _PAIR = int, float, str, "bool", "pair"
PARAMS = [
    ("df", "sr", _INT), ("df", "fft_size", _INT), ("df", "hop_size", _INT), ("df", "nb_erb", _INT), ("df", "nb_df", _INT),
    ("df", "norm_tau", _FLOAT), ("df", "lsnr_max", _INT), ("df", "lsnr_min", _INT), ("df", "min_nb_erb_freqs", _INT),
    ("df", "df_order", _INT), ("df", "df_lookahead", _INT), ("df", "pad_mode", _STR),
    ("deepfilternet", "conv_lookahead", _INT), ("deepfilternet", "conv_ch", _INT), ("deepfilternet", "conv_depthwise", _BOOL),
    ("deepfilternet", "convt_depthwise", _BOOL), ("deepfilternet", "conv_kernel", _PAIR), ("deepfilternet", "convt_kernel", _PAIR),
    ("deepfilternet", "conv_kernel_inp", _PAIR), ("deepfilternet", "emb_hidden_dim", _INT), ("deepfilternet", "emb_num_layers", _INT),
    ("deepfilternet", "emb_gru_skip_enc", _STR), ("deepfilternet", "emb_gru_skip", _STR), ("deepfilternet", "df_hidden_dim", _INT),
    ("deepfilternet", "df_gru_skip", _STR), ("deepfilternet", "df_pathway_kernel_size_t", _INT), ("deepfilternet", "enc_concat", _BOOL),
    ("deepfilternet", "df_num_layers", _INT), ("deepfilternet", "df_n_iter", _INT), ("deepfilternet", "lin_groups", _INT),
    ("deepfilternet", "enc_lin_groups", _INT), ("deepfilternet", "mask_pf", _BOOL),
]


# ------------------------------------------------------------------------------------------------ discovery
def pack_root() -> Path:
    return Path(__file__).resolve().parent


def candidate_dirs(model: str = MODEL) -> List[Path]:
    """Where a `model` directory may be, in search order (duplicates removed)."""
    root = pack_root()
    env = os.environ.get("EGREGORA_DFN_MODEL_DIR", "")
    cands = [Path(env)] if env else []
    cands.append(root.parents[1] / "models" / "audio" / "deepfilternet" / model)
    if len(root.parents) > 2:
        cands.append(root.parents[2] / "models" / "audio" / "deepfilternet" / model)
    cands.append(Path(os.path.expanduser("~")) / ".cache" / "DeepFilterNet" / model)
    out, seen = [], set()
    for c in cands:
        if str(c) not in seen:
            seen.add(str(c))
            out.append(c)
    return out


def checkpoint_file(d: Path) -> Optional[Path]:
    """The newest `checkpoints/*.ckpt.best` (highest epoch number in the name), None when there is none."""
    cks = sorted(Path(d).glob("checkpoints/*.ckpt.best"))
    if not cks:
        return None
    def epoch(p: Path):
        m = re.search(r"(\d+)", p.name)
        return (int(m.group(1)) if m else -1, p.name)
    return max(cks, key=epoch)


def is_model_dir(d: Path) -> bool:
    return (Path(d) / "config.ini").is_file() and checkpoint_file(d) is not None


def discover(model: str = MODEL) -> Optional[Path]:
    """The first candidate that holds a model directory, else None (only DeepFilterNet3 is served natively)."""
    if model != MODEL:
        return None
    for d in candidate_dirs(model):
        if is_model_dir(d):
            return d
    return None


# ------------------------------------------------------------------------------------------------ config
def parse_config(path: Path, params=PARAMS, model: str = MODEL) -> dict:
    """config.ini -> {key: value} for every entry of params (a module's PARAMS); raises listing every absent or unreadable key."""
    cp = configparser.ConfigParser()
    cp.read(str(path), encoding="utf-8")
    cfg, bad = {}, []
    for sec, key, typ in params:
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
        raise RuntimeError(f"{model} config {path} is incomplete:\n  " + "\n  ".join(bad))
    return cfg


MAX_GRU_LAYERS = 8                  # EGR_DFN3_MAX_GRU (include/egregora_amd.h)
MAX_NB_ERB = 64                     # EGR_DFN3_MAX_ERB


def check_common(cfg: dict, bad: List[str], recurrence: str = "the recurrence kernel holds"):
    """The range checks of the signal path and the GRU stacks both models share; appends what is out of range to bad.  recurrence
    is the subject of the GRU-width message: DeepFilterNet2 has two recurrence kernels and says so, and the messages keep their text."""
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
            bad.append(f"{k} = {cfg[k]} ({recurrence} 1 <= H <= 256)")
    n_gru = cfg["emb_num_layers"] + cfg["df_num_layers"]
    if cfg["emb_num_layers"] < 2 or cfg["df_num_layers"] < 1 or n_gru > MAX_GRU_LAYERS:
        bad.append(f"emb_num_layers = {cfg['emb_num_layers']} (>= 2: one encoder layer, at least one ERB-decoder layer), "
                   f"df_num_layers = {cfg['df_num_layers']} (>= 1), {n_gru} GRU layers in total (<= {MAX_GRU_LAYERS})")
    if cfg["df_order"] < 1 or cfg["conv_lookahead"] < 0 or cfg["df_lookahead"] < 0 or cfg["df_lookahead"] > cfg["df_order"] - 1:
        bad.append(f"df_order = {cfg['df_order']}, conv_lookahead = {cfg['conv_lookahead']}, df_lookahead = {cfg['df_lookahead']} "
                   "out of range")


def check_supported(cfg: dict):
    """The structure variants the native forward pass implements; anything else raises (no silent approximation).  Accepts exactly
    what egr_dfn3_create and its run() accept and upstream can build; every accepted variant runs (tests/test_gpu_dfn3_configs.py)."""
    bad = []
    want = {"conv_depthwise": True, "convt_depthwise": True, "enc_concat": False, "df_n_iter": 1, "mask_pf": False,
            "emb_gru_skip_enc": "none", "emb_gru_skip": "none"}
    for k, v in want.items():
        if cfg[k] != v:
            bad.append(f"{k} = {cfg[k]!r} (supported: {v!r})")
    if not cfg["norm_tau"] > 0:
        bad.append(f"norm_tau = {cfg['norm_tau']} (> 0)")
    if cfg["sr"] != 48000:
        bad.append(f"sr = {cfg['sr']} (the node always hands the model a 48 kHz signal)")
    if cfg["df_gru_skip"] not in ("none", "groupedlinear"):
        bad.append(f"df_gru_skip = {cfg['df_gru_skip']!r} (supported: 'none', 'groupedlinear')")
    if tuple(cfg["convt_kernel"]) != (1, 3):
        bad.append(f"convt_kernel = {cfg['convt_kernel']} (supported: (1, 3), the only width a stride-2 transposed conv doubles)")
    check_common(cfg, bad)
    if cfg["conv_ch"] < 1 or cfg["lin_groups"] < 1 or cfg["enc_lin_groups"] < 1:
        bad.append(f"conv_ch = {cfg['conv_ch']}, lin_groups = {cfg['lin_groups']}, enc_lin_groups = {cfg['enc_lin_groups']} (>= 1)")
    elif not bad:
        # every grouped linear (GroupedLinearEinsum) splits its input and its output evenly over its groups
        emb = cfg["conv_ch"] * cfg["nb_erb"] // 4
        G, Ge = cfg["lin_groups"], cfg["enc_lin_groups"]
        lins = [("enc.df_fc_emb", cfg["conv_ch"] * cfg["nb_df"] // 2, emb, Ge),
                ("emb_gru linear_in", emb, cfg["emb_hidden_dim"], G), ("emb_gru linear_out", cfg["emb_hidden_dim"], emb, G),
                ("df_gru linear_in", emb, cfg["df_hidden_dim"], G),
                ("df_out", cfg["df_hidden_dim"], cfg["nb_df"] * 2 * cfg["df_order"], G)]
        if cfg["df_gru_skip"] == "groupedlinear":
            lins.append(("df_skip", emb, cfg["df_hidden_dim"], G))
        for name, i, o, g in lins:
            if i % g or o % g:
                bad.append(f"{name}: {i} -> {o} features do not split over {g} groups")
    if bad:
        raise RuntimeError("DeepFilterNet3 config not supported by the native forward pass:\n  " + "\n  ".join(bad))


def norm_alpha(cfg: dict) -> float:
    """df.utils.get_norm_alpha: exp(-hop / (sr tau)) rounded to the fewest decimals (from 3) that keep it below 1."""
    a_ = math.exp(-cfg["hop_size"] / (cfg["sr"] * cfg["norm_tau"]))
    prec, a = 3, 1.0
    while a >= 1.0:
        a = round(a_, prec)
        prec += 1
    return a


def erb_widths(sr: int, fft_size: int, nb_bands: int, min_nb_freqs: int) -> List[int]:
    """libdf's erb_fb band widths (float32 arithmetic like the Rust original); they sum to fft_size / 2 + 1."""
    f32 = np.float32
    def freq2erb(f):
        return f32(9.265) * f32(np.log1p(f32(f) / (f32(24.7) * f32(9.265))))
    def erb2freq(e):
        return f32(24.7) * f32(9.265) * (f32(np.exp(f32(e) / f32(9.265))) - f32(1.0))
    freq_width = f32(sr) / f32(fft_size)
    lo, hi = freq2erb(0.0), freq2erb(sr // 2)
    step = (hi - lo) / f32(nb_bands)
    widths, prev, over = [], 0, 0
    for i in range(1, nb_bands + 1):
        fb = int(np.round(erb2freq(lo + f32(i) * step) / freq_width))
        nb = fb - prev - over
        if nb < min_nb_freqs:
            over = min_nb_freqs - nb
            nb = min_nb_freqs
        else:
            over = 0
        widths.append(nb)
        prev = fb
    widths[-1] += 1
    too_large = sum(widths) - (fft_size // 2 + 1)
    if too_large > 0:
        widths[-1] -= too_large
    if sum(widths) != fft_size // 2 + 1 or min(widths) < 1:
        raise RuntimeError(f"ERB widths {widths} do not tile {fft_size // 2 + 1} bins")
    return widths


def erb_matrices(widths: List[int]) -> Tuple[torch.Tensor, torch.Tensor]:
    """df.modules.erb_fb: (forward [F, E] normalised per band, inverse [E, F] of ones) as DfNet registers them."""
    n = sum(widths)
    fb = torch.zeros(n, len(widths))
    b = 0
    for i, w in enumerate(widths):
        fb[b:b + w, i] = 1.0
        b += w
    return fb / fb.sum(dim=0), fb.t().contiguous()


def derived_vars(cfg: dict) -> dict:
    """Names the key table's shape expressions use."""
    v = dict(cfg)
    v.update(kt_inp=cfg["conv_kernel_inp"][0], kf_inp=cfg["conv_kernel_inp"][1], kt=cfg["conv_kernel"][0], kf=cfg["conv_kernel"][1],
             convt_kt=cfg["convt_kernel"][0], convt_kf=cfg["convt_kernel"][1],
             n_freqs=cfg["fft_size"] // 2 + 1, emb_dim=cfg["conv_ch"] * cfg["nb_erb"] // 4, df_out_ch=2 * cfg["df_order"],
             df_path_groups=math.gcd(cfg["conv_ch"], 2 * cfg["df_order"]), enc_gru_layers=1, erb_gru_layers=cfg["emb_num_layers"] - 1)
    return v


# ------------------------------------------------------------------------------------------------ key table
def expected_table(cfg: dict, keymap_path: Optional[Path] = None, env: Optional[dict] = None) -> Dict[str, Tuple[int, ...]]:
    """{tensor name: shape} the key table prescribes for this config; env: the names its expressions use (derived_vars(cfg)).  An
    entry repeats over '{k}' for the layer count named by 'layers', or over '{l}' for the layer range 'l' = [first, end expression]
    and over '{g}' for the group count named by 'g'."""
    spec = json.loads(Path(keymap_path or KEYMAP_PATH).read_text(encoding="utf-8"))
    env = env or derived_vars(cfg)
    ev = lambda s: int(eval(str(s), {"__builtins__": {}}, env))      # noqa: S307 (repo-owned JSON, integer expressions)
    out = {}
    for e in spec["entries"]:
        if "when" in e and not eval(e["when"], {"__builtins__": {}}, env):  # noqa: S307
            continue
        shape = tuple(ev(s) for s in e["shape"])
        if "layers" in e:
            layers = range(env[e["layers"]])
        elif "l" in e:
            layers = range(ev(e["l"][0]), ev(e["l"][1]))
        else:
            layers = [None]
        groups = range(env[e["g"]]) if "g" in e else [None]
        for l in layers:
            name = e["name"].replace("{k}", str(l)).replace("{l}", str(l))
            for g in groups:
                out[name.replace("{g}", str(g))] = shape
    return out


def layer_table_common(sd: Dict[str, torch.Tensor]) -> dict:
    """What the convolutions, the ERB bank and df_skip say in both models' checkpoints."""
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
    s = get("df_dec.df_convp.1.weight")
    if s is not None:
        t["df_order"], t["df_pathway_kernel_size_t"] = int(s[0]) // 2, int(s[2])
    t["df_gru_skip"] = "groupedlinear" if "df_dec.df_skip.weight" in sd else "none"
    return t


def layer_table(sd: Dict[str, torch.Tensor]) -> dict:
    """Layer counts and widths read from the tensor shapes alone (no config)."""
    def nlayers(prefix):
        return len([k for k in sd if re.fullmatch(re.escape(prefix) + r"\.weight_hh_l\d+", k)])
    t = layer_table_common(sd)
    def get(name):
        return sd[name].shape if name in sd else None
    s = get("enc.emb_gru.gru.weight_hh_l0")
    if s is not None:
        t["emb_hidden_dim"] = int(s[1])
    s = get("df_dec.df_gru.gru.weight_hh_l0")
    if s is not None:
        t["df_hidden_dim"] = int(s[1])
    t["emb_num_layers"] = nlayers("enc.emb_gru.gru") + nlayers("erb_dec.emb_gru.gru")
    t["df_num_layers"] = nlayers("df_dec.df_gru.gru")
    s = get("enc.emb_gru.linear_in.0.weight")
    if s is not None:
        t["lin_groups"] = int(s[0])
    s = get("enc.df_fc_emb.0.weight")
    if s is not None:
        t["enc_lin_groups"] = int(s[0])
        if "conv_ch" in t:
            t["nb_df"] = 2 * int(s[0]) * int(s[1]) // t["conv_ch"]
    return t


def validate_against(sd: Dict[str, torch.Tensor], cfg: dict, want: Dict[str, Tuple[int, ...]], lt: dict, model: str, keymap: str):
    """Raise with every unmapped / missing / mismatched tensor against the expected table `want` and every config field the layer
    table `lt` contradicts; model and the key table's file name go into the messages."""
    unmapped = sorted(k for k in sd if k not in want)
    missing = sorted(k for k in want if k not in sd)
    wrong = sorted(f"{k}: checkpoint {tuple(sd[k].shape)} != table {want[k]}" for k in want if k in sd and tuple(sd[k].shape) != want[k])
    conflict = sorted(f"{k}: shapes say {v!r}, config.ini says {cfg[k]!r}" for k, v in lt.items() if k in cfg and cfg[k] != v)
    if unmapped or missing or wrong or conflict:
        parts = []
        for title, lst in (("unmapped tensors", unmapped), ("missing tensors", missing), ("shape mismatches", wrong),
                           ("config / checkpoint disagreements", conflict)):
            if lst:
                parts.append(f"{title} ({len(lst)}):\n    " + "\n    ".join(lst))
        raise RuntimeError(f"{model} checkpoint does not match {keymap} / config.ini:\n  " + "\n  ".join(parts))
    widths = erb_widths(cfg["sr"], cfg["fft_size"], cfg["nb_erb"], cfg["min_nb_erb_freqs"])
    fb, ifb = erb_matrices(widths)
    if not (torch.allclose(sd["erb_fb"].float(), fb, atol=1e-6) and torch.allclose(sd["mask.erb_inv_fb"].float(), ifb, atol=1e-6)):
        raise RuntimeError(f"{model} checkpoint: erb_fb / mask.erb_inv_fb differ from the ERB bank of config.ini (widths {widths})")


def validate(sd: Dict[str, torch.Tensor], cfg: dict, keymap_path: Optional[Path] = None):
    """Raise with every unmapped / missing / mismatched tensor and every config field the shapes contradict."""
    validate_against(sd, cfg, expected_table(cfg, keymap_path), layer_table(sd), MODEL, KEYMAP_PATH.name)


def read_state_dict(path: Path) -> Dict[str, torch.Tensor]:
    sd = torch.load(str(path), map_location="cpu", weights_only=True)
    for w in ("state_dict", "model"):
        if isinstance(sd, dict) and w in sd and isinstance(sd[w], dict):
            sd = sd[w]
    if not isinstance(sd, dict):
        raise RuntimeError(f"{path}: not a state dict")
    return {k.replace("clc_dec", "df_dec"): v for k, v in sd.items() if torch.is_tensor(v)}


# ------------------------------------------------------------------------------------------------ packing
# The conv stacks both models pack alike (WeightCursor::encoder_convs / erb_decoder_convs / df_pathway_convs, csrc/egr_dfn3.hip)
def encoder_order() -> List[Tuple[str, str]]:
    o = [("enc.erb_conv0.1.weight", "w"), ("enc.erb_conv0.2", "bn")]
    for i in (1, 2, 3):
        o += [(f"enc.erb_conv{i}.0.weight", "w"), (f"enc.erb_conv{i}.1.weight", "w"), (f"enc.erb_conv{i}.2", "bn")]
    return o + [("enc.df_conv0.1.weight", "w"), ("enc.df_conv0.2.weight", "w"), ("enc.df_conv0.3", "bn"),
                ("enc.df_conv1.0.weight", "w"), ("enc.df_conv1.1.weight", "w"), ("enc.df_conv1.2", "bn")]


def erb_decoder_order() -> List[Tuple[str, str]]:
    o = []
    for i in (3, 2, 1):
        o += [(f"erb_dec.conv{i}p.0.weight", "w"), (f"erb_dec.conv{i}p.1", "bn"), (f"erb_dec.convt{i}.0.weight", "w"),
              (f"erb_dec.convt{i}.1.weight", "w"), (f"erb_dec.convt{i}.2", "bn")]
    return o + [("erb_dec.conv0p.0.weight", "w"), ("erb_dec.conv0p.1", "bn"), ("erb_dec.conv0_out.0.weight", "w"),
                ("erb_dec.conv0_out.1", "bn")]


DF_PATHWAY_ORDER = [("df_dec.df_convp.1.weight", "w"), ("df_dec.df_convp.2.weight", "w"), ("df_dec.df_convp.3", "bn")]


def pack_order(cfg: dict) -> List[Tuple[str, str]]:
    """(tensor name, kind) in the order egr_dfn3_create reads them (csrc/egr_dfn3.hip).  kind "w": the tensor as stored (torch
    layout, fp32); "bn": a BatchNorm folded to eval-mode per-channel scale then shift."""
    o = encoder_order() + [("enc.df_fc_emb.0.weight", "w")]

    def sq(prefix, n):
        r = [(f"{prefix}.linear_in.0.weight", "w")]
        for k in range(n):
            r += [(f"{prefix}.gru.{p}_l{k}", "w") for p in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        return r
    o += sq("enc.emb_gru", 1) + [("enc.emb_gru.linear_out.0.weight", "w")]
    o += sq("erb_dec.emb_gru", cfg["emb_num_layers"] - 1) + [("erb_dec.emb_gru.linear_out.0.weight", "w")]
    o += erb_decoder_order() + sq("df_dec.df_gru", cfg["df_num_layers"])
    if cfg["df_gru_skip"] == "groupedlinear":
        o += [("df_dec.df_skip.weight", "w")]
    return o + [("df_dec.df_out.0.weight", "w")] + DF_PATHWAY_ORDER


def fold_bn(sd, prefix) -> Tuple[torch.Tensor, torch.Tensor]:
    w, b = sd[prefix + ".weight"].double(), sd[prefix + ".bias"].double()
    m, v = sd[prefix + ".running_mean"].double(), sd[prefix + ".running_var"].double()
    s = w / torch.sqrt(v + BN_EPS)
    return s, b - m * s


def pack_tensors(sd: Dict[str, torch.Tensor], order: List[Tuple[str, str]]) -> np.ndarray:
    """The tensors of a pack order as one fp32 array."""
    parts = []
    for name, kind in order:
        if kind == "bn":
            s, t = fold_bn(sd, name)
            parts += [s.float().reshape(-1), t.float().reshape(-1)]
        else:
            parts.append(sd[name].float().reshape(-1))
    return torch.cat(parts).numpy().astype(np.float32)


def pack(sd: Dict[str, torch.Tensor], cfg: dict) -> np.ndarray:
    return pack_tensors(sd, pack_order(cfg))


class Model:
    """A validated model directory: config (dict), state dict, ERB widths, norm alpha, packed fp32 weights.  check_supported,
    validate and pack are those of `weights`, the weights module a subclass names."""
    weights = None

    def __init__(self, cfg: dict, sd: Dict[str, torch.Tensor], directory: Optional[Path] = None):
        self.weights.check_supported(cfg)
        self.weights.validate(sd, cfg)
        self.cfg, self.sd, self.dir = cfg, sd, directory
        self.widths = erb_widths(cfg["sr"], cfg["fft_size"], cfg["nb_erb"], cfg["min_nb_erb_freqs"])
        self.alpha = norm_alpha(cfg)

    def packed(self) -> np.ndarray:
        return self.weights.pack(self.sd, self.cfg)


class DFN3Model(Model):
    weights = sys.modules[__name__]


def model_files(model_dir: Optional[Path], found: Optional[Path], model: str) -> Tuple[Path, Path]:
    """(directory, checkpoint file) of model_dir, or of `found` (the module's discover()) when it is None; raises when neither is
    a model directory."""
    d = Path(model_dir) if model_dir else found
    if d is None:
        raise RuntimeError(f"no {model} model directory found; searched:\n  " + "\n  ".join(map(str, candidate_dirs(model))))
    ck = checkpoint_file(d)
    if not (d / "config.ini").is_file() or ck is None:
        raise RuntimeError(f"{d} is not a DeepFilterNet model directory (config.ini + checkpoints/*.ckpt.best)")
    return d, ck


def load(model_dir: Optional[Path] = None) -> DFN3Model:
    d, ck = model_files(model_dir, None if model_dir else discover(), MODEL)
    return DFN3Model(parse_config(d / "config.ini"), read_state_dict(ck), d)
