"""Native DeepFilterNet2 backend of `Egregora DeepFilterNet Denoise` (egr_dfn2_* in libegregora_amd.so, csrc/egr_dfn3.hip).

One handle per (model directory, device), created from a validated model directory (dfn2_weights.load) and kept for the life of the
process, as dfn_engine.py does for DeepFilterNet3.  enhance() takes the 48 kHz signal while it is on the device and returns the
denoised signal there, on the current stream.
"""
import ctypes as C
import threading
from pathlib import Path
from typing import Dict, Optional, Tuple

import torch

from . import dfn2_weights, native

_CACHE: Dict[Tuple[str, int], "Dfn2Engine"] = {}
_LOCK = threading.Lock()


def config_c(m: "dfn2_weights.DFN2Model") -> native.Dfn2ConfigC:
    c, sd = m.cfg, m.sd
    s = native.Dfn2ConfigC()
    s.struct_bytes = C.sizeof(native.Dfn2ConfigC)
    for f in ("sr", "fft_size", "hop_size", "nb_erb", "nb_df", "df_order", "df_lookahead", "conv_lookahead", "emb_hidden_dim",
              "emb_num_layers", "df_hidden_dim", "df_num_layers", "gru_groups", "lin_groups", "conv_ch"):
        setattr(s, f, int(c[f]))
    s.group_shuffle = int(bool(c["group_shuffle"]))
    s.kt_inp, s.kf_inp = c["conv_kernel_inp"]
    s.kt, s.kf = c["conv_kernel"]
    s.df_gru_skip = 1 if c["df_gru_skip"] == "groupedlinear" else 0
    s.df_output_layer = 1 if c["df_output_layer"] == "linear" else 0
    s.df_pathway_kt = int(c["df_pathway_kernel_size_t"])
    s.path_groups = int(c["conv_ch"]) // int(sd["erb_dec.conv3p.0.weight"].shape[1])
    s.df_path_groups = int(c["conv_ch"]) // int(sd["df_dec.df_convp.1.weight"].shape[1])
    s.norm_alpha = float(m.alpha)
    for i, w in enumerate(m.widths):
        s.erb_widths[i] = int(w)
    return s


class Dfn2Engine:
    def __init__(self, model: "dfn2_weights.DFN2Model", device: int):
        self.model, self.device = model, int(device)
        L = native.lib()
        self._cfg = config_c(model)
        w = model.packed()
        h = C.c_void_p()
        native.check(L.egr_dfn2_create(C.byref(h), C.byref(self._cfg), w.ctypes.data_as(C.c_void_p), int(w.size), self.device),
                     "egr_dfn2_create")
        self.h = h

    def __del__(self):
        try:
            if getattr(self, "h", None):
                native.lib().egr_dfn2_destroy(self.h)
        except Exception:           # noqa: BLE001 (interpreter shutdown)
            pass

    def enhance(self, x48: torch.Tensor) -> torch.Tensor:
        """x48 [C, T] float32 on this engine's device -> [C, T] on the same device, enqueued on the current stream."""
        if x48.dim() != 2 or not x48.is_cuda or x48.device.index != self.device:
            raise ValueError(f"egr_dfn2: expected [C, T] on cuda:{self.device}, got {tuple(x48.shape)} on {x48.device}")
        x = x48.to(torch.float32).contiguous()
        y = torch.empty_like(x)
        with torch.cuda.device(self.device):
            native.check(native.lib().egr_dfn2_enhance(self.h, native.ptr(x), x.shape[0], x.shape[1], native.ptr(y), native.stream_ptr()),
                         "egr_dfn2_enhance")
        return y

    def workspace_bytes(self, channels: int, n: int) -> int:
        return int(native.lib().egr_dfn2_workspace_bytes(self.h, int(channels), int(n)))

    def stage(self, name: str, layer: int = 0) -> torch.Tensor:
        """An intermediate of the last enhance call as a flat float32 device tensor (layouts: include/egregora_amd.h); "gru0" and
        "sum0" take the GroupedGRU layer index."""
        L = native.lib()
        sid = native.DFN2_STAGE[name] + (layer if name in ("gru0", "sum0") else 0)
        n = C.c_int64()
        native.check(L.egr_dfn2_stage(self.h, sid, None, 0, C.byref(n), native.stream_ptr()), "egr_dfn2_stage")
        out = torch.empty(n.value, dtype=torch.float32, device=f"cuda:{self.device}")
        native.check(L.egr_dfn2_stage(self.h, sid, native.ptr(out), n.value, C.byref(n), native.stream_ptr()), "egr_dfn2_stage")
        return out

    def time_gru(self, layer: int = 0, channels: int = 2, steps: int = 20000) -> float:
        us = C.c_double()
        native.check(native.lib().egr_dfn2_time_gru(self.h, layer, channels, steps, C.byref(us)), "egr_dfn2_time_gru")
        return us.value


def engine(model_dir: Optional[Path] = None, device: Optional[int] = None) -> Dfn2Engine:
    """The cached engine of (model directory, device); discovery when model_dir is None."""
    d = Path(model_dir) if model_dir else dfn2_weights.discover()
    if d is None:
        raise RuntimeError("no DeepFilterNet2 model directory found")
    dev = torch.cuda.current_device() if device is None else int(device)
    key = (str(d.resolve()), dev)
    with _LOCK:
        if key not in _CACHE:
            _CACHE[key] = Dfn2Engine(dfn2_weights.load(d), dev)
        return _CACHE[key]
