"""Descript Audio Codec on the device (SPEC.md 4e; csrc/egr_dac.hip): one handle per (checkpoint file, device), encode / quantize /
decode / stage over the C ABI.  Rows are mono signals (DAC-Q1).  One pass only: a call whose workspace would exceed
EGREGORA_DAC_WORKSPACE_GB (default 64, DeepFilterNet's choice, not a measurement) raises RuntimeError naming the limit.  There is no
CPU path.
"""
import ctypes as C
import os
import threading
from pathlib import Path
from typing import Optional, Tuple

import torch

from . import dac_weights, native

WORKSPACE_GB_ENV, WORKSPACE_GB_DEFAULT = "EGREGORA_DAC_WORKSPACE_GB", "64"
_CACHE = {}
_LOCK = threading.Lock()


def workspace_budget_gb() -> float:
    return float(os.environ.get(WORKSPACE_GB_ENV, WORKSPACE_GB_DEFAULT))


def workspace_budget_bytes() -> int:
    return int(workspace_budget_gb() * 2 ** 30)


def conv_length(L: int, s: int) -> int:
    """torch's Conv1d(k = 2 s, stride s, padding ceil(s / 2)) output length."""
    num = L + 2 * ((s + 1) // 2) - 2 * s
    return 0 if num < 0 else num // s + 1


def convtr_length(L: int, s: int) -> int:
    """torch's ConvTranspose1d(k = 2 s, stride s, padding ceil(s / 2)) output length: L s for even s, L s - 1 for odd s."""
    return (L - 1) * s - 2 * ((s + 1) // 2) + 2 * s


def decoded_length(cfg: dict, frames: int) -> int:
    L = frames
    for s in cfg["decoder_rates"]:
        L = convtr_length(L, s) if L >= 1 else 0
    return L


def lengths(cfg: dict, n: int) -> Tuple[int, int, int]:
    """(n_padded, frames, n_decoded) of an n-sample row: the Python twin of egr_dac_lengths (DAC-P7)."""
    h = dac_weights.hop(cfg)
    n_pad = -(-n // h) * h
    L = n_pad
    for s in cfg["encoder_rates"]:
        L = conv_length(L, s)
    return n_pad, L, decoded_length(cfg, L)


def config_c(cfg: dict) -> native.DacConfigC:
    c = native.DacConfigC()
    c.struct_bytes = C.sizeof(native.DacConfigC)
    for k in ("sample_rate", "encoder_dim", "decoder_dim", "latent_dim", "n_codebooks", "codebook_size", "codebook_dim"):
        setattr(c, k, int(cfg[k]))
    for name, n_name, vals in (("enc_rates", "n_enc", cfg["encoder_rates"]), ("dec_rates", "n_dec", cfg["decoder_rates"])):
        if len(vals) > native.DAC_MAX_RATES:
            raise RuntimeError(f"DAC: {len(vals)} rates; the C ABI holds {native.DAC_MAX_RATES}")
        setattr(c, n_name, len(vals))
        arr = getattr(c, name)
        for i, v in enumerate(vals):
            arr[i] = int(v)
    return c


def lengths_c(cfg: dict, n: int) -> Tuple[int, int, int]:
    """egr_dac_lengths (host only, no device or handle)."""
    a, b, d = C.c_int64(), C.c_int64(), C.c_int64()
    cc = config_c(cfg)
    native.check(native.lib().egr_dac_lengths(C.byref(cc), int(n), C.byref(a), C.byref(b), C.byref(d)), "egr_dac_lengths")
    return a.value, b.value, d.value


class DacEngine:
    def __init__(self, model: "dac_weights.DacModel", device: int):
        self.model, self.cfg, self.device = model, model.cfg, int(device)
        dac_weights.check_supported(self.cfg)
        self._cfg = config_c(self.cfg)
        w = model.packed()
        h = C.c_void_p()
        native.check(native.lib().egr_dac_create(C.byref(h), C.byref(self._cfg), w.ctypes.data_as(C.c_void_p), int(w.size), self.device),
                     "egr_dac_create")
        self.h = h

    def __del__(self):
        try:
            if getattr(self, "h", None):
                native.lib().egr_dac_destroy(self.h)
        except Exception:           # noqa: BLE001 (interpreter shutdown)
            pass

    def lengths(self, n: int) -> Tuple[int, int, int]:
        return lengths(self.cfg, n)

    def workspace_bytes(self, rows: int, n: int) -> int:
        return int(native.lib().egr_dac_workspace_bytes(self.h, int(rows), int(n)))

    def _rows(self, x: torch.Tensor, what: str, dims: int) -> torch.Tensor:
        if x.dim() != dims or not x.is_cuda or x.device.index != self.device or 0 in x.shape:
            raise ValueError(f"DAC {what}: expected a non-empty {dims}-D tensor on cuda:{self.device}, got {tuple(x.shape)} on {x.device}")
        return x.to(torch.float32).contiguous()

    def _budget(self, rows: int, n: int):
        need, budget = self.workspace_bytes(rows, n), workspace_budget_bytes()
        if need > budget:
            raise RuntimeError(f"DAC: {rows} rows of {n} samples need a workspace of {need / 2 ** 20:.1f} MiB, above the limit "
                               f"{WORKSPACE_GB_ENV} = {workspace_budget_gb():g} (one pass only; windowed compress is out of scope)")

    def _outputs(self, rows: int, frames: int):
        dev = f"cuda:{self.device}"
        return (torch.empty((rows, self.cfg["latent_dim"], frames), dtype=torch.float32, device=dev),
                torch.empty((rows, self.cfg["n_codebooks"], frames), dtype=torch.int32, device=dev))

    def encode(self, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """x [rows, n] -> (z [rows, latent, frames] float32, codes [rows, n_codebooks, frames] int32), on the current stream."""
        x = self._rows(x, "encode", 2)
        rows, n = x.shape
        self._budget(rows, n)
        z, codes = self._outputs(rows, self.lengths(n)[1])
        with torch.cuda.device(self.device):
            native.check(native.lib().egr_dac_encode(self.h, native.ptr(x), rows, n, native.ptr(z), native.ptr(codes), native.stream_ptr()),
                         "egr_dac_encode")
        return z, codes

    def quantize(self, ze: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """The quantiser alone (DAC-P8): ze [rows, latent, frames] -> (z, codes)."""
        ze = self._rows(ze, "quantize", 3)
        rows, lat, frames = ze.shape
        if lat != self.cfg["latent_dim"]:
            raise ValueError(f"DAC quantize: {lat} channels, the model's latent_dim is {self.cfg['latent_dim']}")
        self._budget(rows, frames * dac_weights.hop(self.cfg))      # (the quantiser's buffers are a subset of encode's)
        z, codes = self._outputs(rows, frames)
        with torch.cuda.device(self.device):
            native.check(native.lib().egr_dac_quantize(self.h, native.ptr(ze), rows, frames, native.ptr(z), native.ptr(codes),
                                                       native.stream_ptr()), "egr_dac_quantize")
        return z, codes

    def decode(self, z: torch.Tensor) -> torch.Tensor:
        """z [rows, latent, frames] -> y [rows, n_decoded] (not trimmed: DAC-P7)."""
        z = self._rows(z, "decode", 3)
        rows, lat, frames = z.shape
        if lat != self.cfg["latent_dim"]:
            raise ValueError(f"DAC decode: {lat} channels, the model's latent_dim is {self.cfg['latent_dim']}")
        self._budget(rows, frames * dac_weights.hop(self.cfg))
        y = torch.empty((rows, decoded_length(self.cfg, frames)), dtype=torch.float32, device=z.device)
        with torch.cuda.device(self.device):
            native.check(native.lib().egr_dac_decode(self.h, native.ptr(z), rows, frames, native.ptr(y), native.stream_ptr()), "egr_dac_decode")
        return y

    def keep_stages(self, enable: bool = True):
        """Have the quantiser write the residual entering each stage ("vq_in"; n_codebooks extra latent frames per frame: off by default)."""
        native.check(native.lib().egr_dac_set_stages(self.h, int(bool(enable))), "egr_dac_set_stages")

    def stage(self, name: str, index: int = 0) -> torch.Tensor:
        """An intermediate of the last call as a flat float32 device tensor: "enc" / "dec" index 0 = the input convolution, then the
        blocks ("enc" n_enc + 1: the encoder output), "vq_in" i: the residual entering quantiser stage i (after keep_stages()); channels-last."""
        return native.read_stage(native.lib().egr_dac_stage, "egr_dac_stage", self.device, self.h, native.DAC_STAGE[name], int(index))


def engine(path: Path, device: Optional[int] = None) -> DacEngine:
    """The cached engine of (checkpoint file, device)."""
    dev = torch.cuda.current_device() if device is None else int(device)
    key = (str(Path(path).resolve()), dev)
    with _LOCK:
        if key not in _CACHE:
            _CACHE[key] = DacEngine(dac_weights.load(Path(path)), dev)
        return _CACHE[key]
