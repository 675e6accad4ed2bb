"""Native DeepFilterNet backends of `Egregora DeepFilterNet Denoise` (egr_dfn3_* / egr_dfn2_* in libegregora_amd.so, csrc/egr_dfn3.hip).

One handle per (model directory, device), created from a validated model directory (dfn_weights.load / dfn2_weights.load) and kept
for the life of the process.  enhance() takes the 48 kHz signal while it is on the device and returns the denoised signal there, on
the current stream.  DfnEngine is the engine of both models; this module holds the DeepFilterNet3 one, dfn2_engine.py the other.
"""
import ctypes as C
import threading
from pathlib import Path
from typing import Dict, Optional, Tuple

import torch

from . import dfn_weights, native

_CACHE: Dict[Tuple[str, str, int], "DfnEngine"] = {}
_LOCK = threading.Lock()


def config_common(s, m):
    """The fields both config structs fill alike, from a validated model m."""
    c, sd = m.cfg, m.sd
    s.kt_inp, s.kf_inp = c["conv_kernel_inp"]
    s.kt, s.kf = c["conv_kernel"]
    s.df_gru_skip = 1 if c["df_gru_skip"] == "groupedlinear" else 0
    s.df_pathway_kt = int(c["df_pathway_kernel_size_t"])
    s.path_groups = int(c["conv_ch"]) // int(sd["erb_dec.conv3p.0.weight"].shape[1])
    s.df_path_groups = int(c["conv_ch"]) // int(sd["df_dec.df_convp.1.weight"].shape[1])
    s.norm_alpha = float(m.alpha)
    for i, w in enumerate(m.widths):
        s.erb_widths[i] = int(w)


def config_c(m: "dfn_weights.DFN3Model") -> native.Dfn3ConfigC:
    c = m.cfg
    s = native.Dfn3ConfigC()
    s.struct_bytes = C.sizeof(native.Dfn3ConfigC)
    for f in ("sr", "fft_size", "hop_size", "nb_erb", "nb_df", "df_order", "df_lookahead", "emb_hidden_dim", "emb_num_layers",
              "df_hidden_dim", "df_num_layers", "lin_groups", "enc_lin_groups", "conv_ch"):
        setattr(s, f, int(c[f]))
    # DfNet.pad_feat shifts the features by conv_lookahead only in the "input*" pad modes (SPEC.md DFN3-P4)
    s.conv_lookahead = int(c["conv_lookahead"]) if c["pad_mode"].startswith("input") else 0
    s.convt_kf = c["convt_kernel"][1]
    config_common(s, m)
    return s


class DfnEngine:
    """A subclass names its C symbols' prefix, its stage table (native.DFN*_STAGE), the stage names that take a layer index, its
    weights module and its config_c."""
    prefix, stages, indexed, weights, config_c = "", {}, (), None, None

    def __init__(self, model, device: int):
        self.model, self.device = model, int(device)
        self._cfg = self.config_c(model)
        w = model.packed()
        h = C.c_void_p()
        native.check(self._fn("create")(C.byref(h), C.byref(self._cfg), w.ctypes.data_as(C.c_void_p), int(w.size), self.device),
                     f"{self.prefix}_create")
        self.h = h

    def _fn(self, name: str):
        return getattr(native.lib(), f"{self.prefix}_{name}")

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self._fn("destroy")(self.h)
        except Exception:           # noqa: BLE001 (interpreter shutdown)
            pass

    def enhance(self, x48: torch.Tensor) -> torch.Tensor:
        """x48 [C, T] float32 on this engine's device -> [C, T] on the same device, enqueued on the current stream."""
        if x48.dim() != 2 or not x48.is_cuda or x48.device.index != self.device:
            raise ValueError(f"{self.prefix}: expected [C, T] on cuda:{self.device}, got {tuple(x48.shape)} on {x48.device}")
        x = x48.to(torch.float32).contiguous()
        y = torch.empty_like(x)
        with torch.cuda.device(self.device):
            native.check(self._fn("enhance")(self.h, native.ptr(x), x.shape[0], x.shape[1], native.ptr(y), native.stream_ptr()),
                         f"{self.prefix}_enhance")
        return y

    def workspace_bytes(self, channels: int, n: int) -> int:
        return int(self._fn("workspace_bytes")(self.h, int(channels), int(n)))

    def stage(self, name: str, layer: int = 0) -> torch.Tensor:
        """An intermediate of the last enhance call as a flat float32 device tensor (layouts: include/egregora_amd.h); the names in
        `indexed` take the GRU layer index."""
        f, what = self._fn("stage"), f"{self.prefix}_stage"
        sid = self.stages[name] + (layer if name in self.indexed else 0)
        n = C.c_int64()
        native.check(f(self.h, sid, None, 0, C.byref(n), native.stream_ptr()), what)
        out = torch.empty(n.value, dtype=torch.float32, device=f"cuda:{self.device}")
        native.check(f(self.h, sid, native.ptr(out), n.value, C.byref(n), native.stream_ptr()), what)
        return out

    def time_gru(self, layer: int = 0, channels: int = 2, steps: int = 20000) -> float:
        us = C.c_double()
        native.check(self._fn("time_gru")(self.h, layer, channels, steps, C.byref(us)), f"{self.prefix}_time_gru")
        return us.value


def cached(cls, model_dir: Optional[Path] = None, device: Optional[int] = None) -> DfnEngine:
    """The cached `cls` engine of (model directory, device); discovery by cls.weights when model_dir is None."""
    d = Path(model_dir) if model_dir else cls.weights.discover()
    if d is None:
        raise RuntimeError(f"no {cls.weights.MODEL} model directory found")
    dev = torch.cuda.current_device() if device is None else int(device)
    key = (cls.prefix, str(d.resolve()), dev)
    with _LOCK:
        if key not in _CACHE:
            _CACHE[key] = cls(cls.weights.load(d), dev)
        return _CACHE[key]


class Dfn3Engine(DfnEngine):
    prefix, stages, indexed, weights = "egr_dfn3", native.DFN3_STAGE, ("gru0",), dfn_weights
    config_c = staticmethod(config_c)

    def stage(self, name: str, gru: int = 0) -> torch.Tensor:
        return super().stage(name, gru)


def engine(model_dir: Optional[Path] = None, device: Optional[int] = None) -> Dfn3Engine:
    """The cached engine of (model directory, device); discovery when model_dir is None."""
    return cached(Dfn3Engine, model_dir, device)
