"""Descript Audio Codec checkpoint discovery, validation and packing for the native codec (SPEC.md 4e, UPSTREAM-RECALL).

A checkpoint is one `torch.save` file `{"state_dict": ..., "metadata": {"kwargs": {...}}}` named `weights_<model_type>_*.pth`
(upstream's file names, recalled).  It is looked for, in this order, in
  1. EGREGORA_DAC_MODEL_DIR
  2. models/audio/dac/ at both places `models/` can mean (as dfn_weights.candidate_dirs)
  3. upstream's own cache, ~/.cache/descript/dac/
No download is attempted.  The hyper-parameters come from metadata.kwargs (DAC-P1 defaults); the layer table the tensor shapes imply
must agree with them, and every tensor name and shape with the name patterns of `dac_keymap.json`.  Anything unmapped, missing or
mismatched raises with the full list.  Weight norm is folded here in float64 (DAC-P2) and the tensors are handed to egr_dac_create as
one fp32 blob in `expected_table` order.
"""
import json
import os
from pathlib import Path
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

KEYMAP_PATH = Path(__file__).resolve().parent / "dac_keymap.json"
MODEL_TYPES = ("44khz", "24khz", "16khz")
DEFAULTS = {"encoder_dim": 64, "encoder_rates": [2, 4, 8, 8], "latent_dim": None, "decoder_dim": 1536, "decoder_rates": [8, 8, 4, 2],
            "n_codebooks": 9, "codebook_size": 1024, "codebook_dim": 8, "sample_rate": 44100}
# DAC-P9: what egr_dac_create accepts (csrc/egr_dac.hip check_config)
MAX_RATES, MAX_RATE, MAX_WIDTH, MAX_CODEBOOKS, MAX_CB_FLOATS, MAX_CB_DIM = 8, 16, 2048, 32, 16384, 64
DILATIONS = (1, 3, 9)


# ------------------------------------------------------------------------------------------------ discovery
def pack_root() -> Path:
    return Path(__file__).resolve().parent


def candidate_dirs() -> List[Path]:
    """Where a checkpoint may be, in search order (duplicates removed)."""
    root = pack_root()
    env = os.environ.get("EGREGORA_DAC_MODEL_DIR", "")
    cands = [Path(env)] if env else []
    cands.append(root.parents[1] / "models" / "audio" / "dac")
    if len(root.parents) > 2:
        cands.append(root.parents[2] / "models" / "audio" / "dac")
    cands.append(Path(os.path.expanduser("~")) / ".cache" / "descript" / "dac")
    out, seen = [], set()
    for c in cands:
        if str(c) not in seen:
            seen.add(str(c))
            out.append(c)
    return out


def discover(model_type: str = "44khz") -> Optional[Path]:
    """The first `weights_<model_type>_*.pth` of the first candidate directory that holds one, else None.  Never fetches."""
    for d in candidate_dirs():
        files = sorted(Path(d).glob(f"weights_{model_type}_*.pth")) if Path(d).is_dir() else []
        if files:
            return files[-1]
    return None


def not_found_message(model_type: str) -> str:
    return (f"No DAC checkpoint weights_{model_type}_*.pth found in EGREGORA_DAC_MODEL_DIR, models/audio/dac/ or "
            "~/.cache/descript/dac/ (this pack never downloads).")


# ------------------------------------------------------------------------------------------------ config
def config_from_kwargs(kwargs: dict) -> dict:
    """metadata.kwargs with DAC-P1's defaults filled in; latent_dim None -> encoder_dim * 2^len(encoder_rates)."""
    cfg = dict(DEFAULTS)
    for k in DEFAULTS:
        if k in kwargs and kwargs[k] is not None:
            cfg[k] = kwargs[k]
    cfg["encoder_rates"] = [int(r) for r in cfg["encoder_rates"]]
    cfg["decoder_rates"] = [int(r) for r in cfg["decoder_rates"]]
    if cfg["latent_dim"] is None:
        cfg["latent_dim"] = int(cfg["encoder_dim"]) * 2 ** len(cfg["encoder_rates"])
    for k in ("encoder_dim", "latent_dim", "decoder_dim", "n_codebooks", "codebook_size", "codebook_dim", "sample_rate"):
        cfg[k] = int(cfg[k])
    return cfg


def hop(cfg: dict) -> int:
    return int(np.prod(cfg["encoder_rates"], dtype=np.int64))


def check_supported(cfg: dict):
    """DAC-P9: raises RuntimeError with every limit the config breaks (exactly what egr_dac_create refuses)."""
    bad = []
    for side, rates in (("encoder", cfg["encoder_rates"]), ("decoder", cfg["decoder_rates"])):
        if not 1 <= len(rates) <= MAX_RATES:
            bad.append(f"{side}_rates has {len(rates)} entries (1 .. {MAX_RATES})")
        bad += [f"{side} rate {r} outside 1 .. {MAX_RATE}" for r in rates if not 1 <= r <= MAX_RATE]
    for k in ("encoder_dim", "decoder_dim", "latent_dim", "n_codebooks", "codebook_size", "codebook_dim"):
        if cfg[k] < 1:
            bad.append(f"{k} = {cfg[k]} is not positive")
    widths = {"encoder": cfg["encoder_dim"] * 2 ** len(cfg["encoder_rates"]), "decoder": cfg["decoder_dim"], "latent": cfg["latent_dim"]}
    bad += [f"{k} width {v} above {MAX_WIDTH}" for k, v in widths.items() if v > MAX_WIDTH]
    if cfg["decoder_dim"] % 2 ** len(cfg["decoder_rates"]):
        bad.append(f"decoder_dim {cfg['decoder_dim']} does not halve {len(cfg['decoder_rates'])} times")
    if cfg["n_codebooks"] > MAX_CODEBOOKS:
        bad.append(f"n_codebooks {cfg['n_codebooks']} above {MAX_CODEBOOKS}")
    if cfg["codebook_size"] * cfg["codebook_dim"] > MAX_CB_FLOATS:
        bad.append(f"codebook_size * codebook_dim = {cfg['codebook_size'] * cfg['codebook_dim']} above {MAX_CB_FLOATS} (a codebook must fit in LDS)")
    if cfg["codebook_dim"] > MAX_CB_DIM:
        bad.append(f"codebook_dim {cfg['codebook_dim']} above {MAX_CB_DIM}")
    if bad:
        raise RuntimeError("DAC config outside the supported range (no CPU fallback in this pack):\n  " + "\n  ".join(bad))


# ------------------------------------------------------------------------------------------------ names and shapes
def keymap(path: Optional[Path] = None) -> dict:
    return json.loads(Path(path or KEYMAP_PATH).read_text())


def expected_table(cfg: dict, keymap_path: Optional[Path] = None) -> List[Tuple[str, str, Tuple[int, ...]]]:
    """(kind, name, shape) of every tensor group in pack order.  kind: conv / convtr (name + .weight_g / .weight_v / .bias, shape of
    weight_v), alpha ([1, C, 1]), codebook ([K, cd])."""
    km = keymap(keymap_path)
    out = []

    def unit(side, i, j, C):
        f = dict(i=i, j=j)
        out.append(("alpha", km[side]["unit_snake1"].format(**f), (1, C, 1)))
        out.append(("conv", km[side]["unit_conv7"].format(**f), (C, C, 7)))
        out.append(("alpha", km[side]["unit_snake2"].format(**f), (1, C, 1)))
        out.append(("conv", km[side]["unit_conv1"].format(**f), (C, C, 1)))

    e, ne = km["encoder"], len(cfg["encoder_rates"])
    C = cfg["encoder_dim"]
    out.append(("conv", e["conv_in"], (C, 1, 7)))
    for i, s in enumerate(cfg["encoder_rates"], start=1):
        for j in range(len(DILATIONS)):
            unit("encoder", i, j, C)
        out.append(("alpha", e["block_snake"].format(i=i), (1, C, 1)))
        out.append(("conv", e["block_down"].format(i=i), (2 * C, C, 2 * s)))
        C *= 2
    out.append(("alpha", e["snake_out"].format(n1=ne + 1), (1, C, 1)))
    out.append(("conv", e["conv_out"].format(n2=ne + 2), (cfg["latent_dim"], C, 3)))
    q = km["quantizer"]
    for i in range(cfg["n_codebooks"]):
        out.append(("conv", q["in_proj"].format(q=i), (cfg["codebook_dim"], cfg["latent_dim"], 1)))
        out.append(("codebook", q["codebook"].format(q=i), (cfg["codebook_size"], cfg["codebook_dim"])))
        out.append(("conv", q["out_proj"].format(q=i), (cfg["latent_dim"], cfg["codebook_dim"], 1)))
    d_, nd = km["decoder"], len(cfg["decoder_rates"])
    C = cfg["decoder_dim"]
    out.append(("conv", d_["conv_in"], (C, cfg["latent_dim"], 7)))
    for i, s in enumerate(cfg["decoder_rates"], start=1):
        out.append(("alpha", d_["block_snake"].format(i=i), (1, C, 1)))
        out.append(("convtr", d_["block_up"].format(i=i), (C, C // 2, 2 * s)))
        C //= 2
        for j in range(len(DILATIONS)):
            unit("decoder", i, j + 2, C)
    out.append(("alpha", d_["snake_out"].format(n1=nd + 1), (1, C, 1)))
    out.append(("conv", d_["conv_out"].format(n2=nd + 2), (1, C, 7)))
    return out


def tensor_names(table) -> Dict[str, Tuple[int, ...]]:
    """state-dict name -> shape for an expected_table."""
    want = {}
    for kind, name, shape in table:
        if kind in ("conv", "convtr"):
            g = (shape[0], 1, 1)
            bias = shape[1] if kind == "convtr" else shape[0]
            want[name + ".weight_g"], want[name + ".weight_v"], want[name + ".bias"] = g, tuple(shape), (bias,)
        else:
            want[name] = tuple(shape)
    return want


def layer_table(sd: Dict[str, torch.Tensor]) -> dict:
    """The hyper-parameters the tensor shapes imply (DAC-P1): widths and depths from the conv shapes, a stride as kernel / 2 of its
    resampling conv.  Raises RuntimeError when a tensor it needs is absent."""
    km = keymap()

    def shape(name):
        if name not in sd:
            raise RuntimeError(f"DAC checkpoint: tensor {name} is missing, the layer table cannot be derived")
        return tuple(sd[name].shape)

    def count(pattern):
        n = 0
        while pattern.format(i=n + 1, q=n) in sd:
            n += 1
        return n

    e, d, q = km["encoder"], km["decoder"], km["quantizer"]
    ne, nd = count(e["block_down"] + ".weight_v"), count(d["block_up"] + ".weight_v")
    ncb = count(q["codebook"])
    if not (ne and nd and ncb):
        raise RuntimeError(f"DAC checkpoint: found {ne} encoder blocks, {nd} decoder blocks, {ncb} codebooks; each must be at least 1")
    cb = shape(q["codebook"].format(q=0))
    return {"encoder_dim": shape(e["conv_in"] + ".weight_v")[0],
            "encoder_rates": [shape(e["block_down"].format(i=i) + ".weight_v")[2] // 2 for i in range(1, ne + 1)],
            "latent_dim": shape(e["conv_out"].format(n2=ne + 2) + ".weight_v")[0],
            "decoder_dim": shape(d["conv_in"] + ".weight_v")[0],
            "decoder_rates": [shape(d["block_up"].format(i=i) + ".weight_v")[2] // 2 for i in range(1, nd + 1)],
            "n_codebooks": ncb, "codebook_size": cb[0], "codebook_dim": cb[1]}


def validate(sd: Dict[str, torch.Tensor], cfg: dict):
    """Every tensor name and shape against the key map, the derived layer table against cfg; raises with the full list."""
    lt = layer_table(sd)
    bad = [f"{k}: the tensor shapes imply {lt[k]}, metadata.kwargs says {cfg[k]}" for k in lt if lt[k] != cfg[k]]
    want = tensor_names(expected_table(cfg))
    bad += [f"missing tensor {k} {want[k]}" for k in want if k not in sd]
    bad += [f"unmapped tensor {k} {tuple(sd[k].shape)}" for k in sd if k not in want]
    bad += [f"shape of {k}: {tuple(sd[k].shape)}, expected {want[k]}" for k in want if k in sd and tuple(sd[k].shape) != want[k]]
    if bad:
        raise RuntimeError("DAC checkpoint does not match the layer table (dac_keymap.json):\n  " + "\n  ".join(bad))


# ------------------------------------------------------------------------------------------------ packing
def fold_weight_norm(g: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """DAC-P2: w = g v / ||v||, the norm over every axis but 0 (the output channel of a Conv1d, the INPUT channel of a
    ConvTranspose1d); float64, rounded to fp32 once."""
    v64, g64 = v.to(torch.float64), g.to(torch.float64)
    nrm = v64.reshape(v64.shape[0], -1).norm(dim=1).reshape((-1,) + (1,) * (v64.dim() - 1))
    return (g64 * v64 / nrm).to(torch.float32)


def pack(sd: Dict[str, torch.Tensor], cfg: dict) -> np.ndarray:
    """The fp32 blob egr_dac_create reads: expected_table order; a conv / convtr as (folded weight in torch layout, bias), a snake as
    its alpha [C], a codebook as stored."""
    parts = []
    for kind, name, _ in expected_table(cfg):
        if kind in ("conv", "convtr"):
            parts.append(fold_weight_norm(sd[name + ".weight_g"], sd[name + ".weight_v"]).reshape(-1))
            parts.append(sd[name + ".bias"].to(torch.float32).reshape(-1))
        else:
            parts.append(sd[name].to(torch.float32).reshape(-1))
    return np.ascontiguousarray(torch.cat(parts).numpy(), dtype=np.float32)


class DacModel:
    def __init__(self, cfg: dict, sd: Dict[str, torch.Tensor], path: Optional[Path] = None):
        self.cfg, self.sd, self.path = cfg, sd, path

    def packed(self) -> np.ndarray:
        return pack(self.sd, self.cfg)


def load(path: Path) -> DacModel:
    """Read, validate and range-check one checkpoint (DAC-P1, P9)."""
    obj = torch.load(str(path), map_location="cpu", weights_only=True)
    if not (isinstance(obj, dict) and "state_dict" in obj and isinstance(obj.get("metadata"), dict) and "kwargs" in obj["metadata"]):
        raise RuntimeError(f"{path}: not a DAC checkpoint (want a dict with state_dict and metadata.kwargs)")
    cfg = config_from_kwargs(obj["metadata"]["kwargs"])
    sd = {k: v for k, v in obj["state_dict"].items() if torch.is_tensor(v)}
    check_supported(cfg)
    validate(sd, cfg)
    return DacModel(cfg, sd, Path(path))
