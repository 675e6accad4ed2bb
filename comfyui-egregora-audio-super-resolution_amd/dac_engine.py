"""Descript Audio Codec on the device (SPEC.md 4e; csrc/egr_dac.hip): one handle per (checkpoint file, device), encode / quantize /
decode / from_codes / stage over the C ABI.  Rows are mono signals (DAC-Q1).  A call whose one-pass workspace fits
EGREGORA_DAC_WORKSPACE_GB (default 64, DeepFilterNet's choice, not a measurement) runs in one pass; a longer one runs in segments of
the most frames that fit (choose_path; DESIGN.md 7.6.1: exact segmentation of the one-pass function, not upstream's window scheme),
and only when not even SEGMENT_STEP frames fit does it raise RuntimeError naming the limit.  There is no CPU path.
"""
import ctypes as C
import os
import threading
from pathlib import Path
from typing import Callable, NamedTuple, Optional, Tuple

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


ENCODE, DECODE = 0, 1                       # EGR_DAC_ENCODE / EGR_DAC_DECODE
SEGMENT_ALIGN = 16                          # interior windows are widened to a multiple of this many frames (DAC_SEG_ALIGN)
# choose_path picks segment lengths in multiples of this many frames.  2048 is the shortest power of two at which the launcher still
# gives every dilation-1 and dilation-3 unit of the 44 kHz model, mono, the k_conv1d_s3 instantiation it has in one pass (shorter
# windows leave too few workgroups and it turns to split-K: profiles/dac_segmented.md); its margins (8 + 8 frames, widened to a
# multiple of 16) are under 1 % of the work, its workspace about 3 GiB a row.
SEGMENT_STEP = 2048


class Segment(NamedTuple):
    """egr_dac_segment (include/egregora_amd.h): half-open ranges.  keep, win: latent frames; in: samples of x (encode) or frames of
    z (decode); out: frames (encode) or samples of y (decode)."""
    keep_lo: int
    keep_hi: int
    win_lo: int
    win_hi: int
    in_lo: int
    in_hi: int
    out_lo: int
    out_hi: int


class SegmentC(C.Structure):
    _fields_ = [(f, C.c_int64) for f in Segment._fields]


def layer_list(cfg: dict, kind: int):
    """(transposed, k, stride, dilation, padding) of every convolution of one side, input to output."""
    units = [t for d in (1, 3, 9) for t in ((False, 7, 1, d, 3 * d), (False, 1, 1, 1, 0))]
    out = [(False, 7, 1, 1, 3)]
    if kind == ENCODE:
        for s in cfg["encoder_rates"]:
            out += units + [(False, 2 * s, s, 1, (s + 1) // 2)]
        return out + [(False, 3, 1, 1, 1)]
    for s in cfg["decoder_rates"]:
        out += [(True, 2 * s, s, 1, (s + 1) // 2)] + units
    return out + [(False, 7, 1, 1, 3)]


def segment_margins(cfg: dict, kind: int) -> Tuple[int, int]:
    """Frames a window needs on the (left, right) of the frames it keeps: the outputs of kept frame 0 walked back through the layers
    (a Conv1d output o reads o s - p + t d; a ConvTranspose1d output j receives input i where j = i s - p + t)."""
    per = 1
    for s in cfg["encoder_rates" if kind == ENCODE else "decoder_rates"]:
        per *= s
    lo, hi = (0, 0) if kind == ENCODE else (0, per - 1)
    for tr, k, s, d, p in reversed(layer_list(cfg, kind)):
        if tr:
            lo, hi = -((-(lo + p - (k - 1))) // s), (hi + p) // s
        else:
            lo, hi = lo * s - p, hi * s - p + (k - 1) * d
    if kind == ENCODE:
        return max(0, -(lo // per)), max(0, -((-(hi + 1 - per)) // per))
    return max(0, -lo), max(0, hi)


def segment_count(cfg: dict, kind: int, length: int, seg_frames: int) -> int:
    F = lengths(cfg, length)[1] if kind == ENCODE else length
    return -(-F // seg_frames)


def segment_plan(cfg: dict, kind: int, length: int, seg_frames: int, index: int) -> Segment:
    """Segment `index` of an input of `length` (n samples for ENCODE, frames for DECODE) cut every seg_frames latent frames: the
    Python twin of egr_dacseg_plan."""
    if kind not in (ENCODE, DECODE) or length < 1 or seg_frames < 1 or min(cfg["encoder_rates"] + cfg["decoder_rates"]) < 2:
        raise ValueError("segment_plan: bad argument")
    per = 1
    for s in cfg["encoder_rates" if kind == ENCODE else "decoder_rates"]:
        per *= s
    F = lengths(cfg, length)[1] if kind == ENCODE else length
    nseg = -(-F // seg_frames)
    if F < 1 or not 0 <= index < nseg:
        raise ValueError(f"segment_plan: segment {index} of {nseg}")
    ml, mr = segment_margins(cfg, kind)
    k0 = index * seg_frames
    k1 = min(F, k0 + seg_frames)
    w0, w1 = max(0, k0 - ml), min(F, k1 + mr)
    extra = -(w1 - w0) % SEGMENT_ALIGN                  # widen: left first, then right
    t = min(extra, w0)
    w0, extra = w0 - t, extra - t
    w1 += min(extra, F - w1)
    if kind == ENCODE:
        return Segment(k0, k1, w0, w1, w0 * per, min(length, w1 * per), k0, k1)
    n_dec = decoded_length(cfg, F)
    return Segment(k0, k1, w0, w1, w0, w1, min(n_dec, k0 * per), n_dec if index == nseg - 1 else min(n_dec, k1 * per))


def segment_plan_c(cfg: dict, kind: int, length: int, seg_frames: int, index: int) -> Tuple[Segment, int]:
    """(segment, number of segments) from egr_dacseg_plan (host only: needs no GPU)."""
    sc, cnt, cc = SegmentC(), C.c_int64(), config_c(cfg)
    native.check(native.lib().egr_dacseg_plan(C.byref(cc), kind, int(length), int(seg_frames), int(index), C.byref(sc), C.byref(cnt)),
                 "egr_dacseg_plan")
    return Segment(*(int(getattr(sc, f)) for f in Segment._fields)), int(cnt.value)


def choose_path(frames: int, one_pass_bytes: int, budget_bytes: int, bytes_for: Callable[[int], int], what: str = "DAC") -> Optional[int]:
    """None: one pass (its workspace is within the budget, so everything measured on that path stays on it).  Else the segment
    length: the largest multiple of SEGMENT_STEP frames, up to the first that covers `frames`, whose workspace bytes_for(seg_frames)
    fits (bytes_for grows with seg_frames); raises when even SEGMENT_STEP frames do not fit."""
    if one_pass_bytes <= budget_bytes:
        return None
    need = bytes_for(SEGMENT_STEP)
    if need > budget_bytes:
        raise RuntimeError(f"{what}: a segment of {SEGMENT_STEP} frames needs a workspace of {need / 2 ** 20:.1f} MiB, above the limit "
                           f"{WORKSPACE_GB_ENV} = {workspace_budget_gb():g}")
    lo, hi = 1, max(1, -(-frames // SEGMENT_STEP))                                              # in steps; lo fits
    if bytes_for(hi * SEGMENT_STEP) <= budget_bytes:
        return hi * SEGMENT_STEP
    while hi - lo > 1:                                                                          # hi does not fit
        mid = (lo + hi) // 2
        if bytes_for(mid * SEGMENT_STEP) <= budget_bytes:
            lo = mid
        else:
            hi = mid
    return lo * SEGMENT_STEP


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
        self.last_seg_frames = None      # what the last encode / decode that chose its own path took (None: one pass)

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

    def segment_workspace_bytes(self, rows: int, seg_frames: int, n: int, kind: int = ENCODE) -> int:
        """The workspace of a segmented call on n samples a row: a part that depends on (rows, seg_frames) only, plus whole-length
        buffers of at most 3 latent_dim floats per frame and row."""
        return int(native.lib().egr_dacseg_workspace_bytes(self.h, int(rows), int(seg_frames), int(n), int(kind)))

    def workspace_held(self) -> int:
        """Bytes of workspace the handle holds now (it grows to the largest call so far and is kept)."""
        return int(native.lib().egr_dacseg_workspace_held(self.h))

    def _budget(self, rows: int, n: int):
        need, budget = self.workspace_bytes(rows, n), workspace_budget_bytes()
        if need > budget:
            raise RuntimeError(f"DAC: {rows} rows of {n} samples need a workspace of {need / 2 ** 20:.1f} MiB, above the limit "
                               f"{WORKSPACE_GB_ENV} = {workspace_budget_gb():g} (the quantiser alone runs in one pass)")

    def _path(self, rows: int, n: int, frames: int, kind: int, seg_frames: Optional[int]) -> Optional[int]:
        """seg_frames as given, else choose_path's: None for one pass."""
        if seg_frames is not None:
            if int(seg_frames) < 1:
                raise ValueError(f"DAC: seg_frames = {seg_frames}")
            return int(seg_frames)
        s = choose_path(frames, self.workspace_bytes(rows, n), workspace_budget_bytes(),
                        lambda f: self.segment_workspace_bytes(rows, f, n, kind), f"DAC: {rows} rows of {n} samples")
        self.last_seg_frames = s
        return s

    def _outputs(self, rows: int, frames: int):
        dev = f"cuda:{self.device}"
        return (torch.empty((rows, self.cfg["latent_dim"], frames), dtype=torch.float32, device=dev),
                torch.empty((rows, self.cfg["n_codebooks"], frames), dtype=torch.int32, device=dev))

    def encode(self, x: torch.Tensor, seg_frames: Optional[int] = None, return_ze: bool = False):
        """x [rows, n] -> (z [rows, latent, frames] float32, codes [rows, n_codebooks, frames] int32), on the current stream.
        seg_frames None: one pass when its workspace fits the budget, else segments (choose_path); a number: segments of that many
        frames.  return_ze (segments only): also the encoder output ze [rows, latent, frames]."""
        x = self._rows(x, "encode", 2)
        rows, n = x.shape
        frames = self.lengths(n)[1]
        seg = self._path(rows, n, frames, ENCODE, seg_frames)
        if return_ze and seg is None:
            raise ValueError("DAC encode: return_ze needs seg_frames")
        z, codes = self._outputs(rows, frames)
        ze = torch.empty_like(z) if return_ze else None
        with torch.cuda.device(self.device):
            if seg is None:
                native.check(native.lib().egr_dac_encode(self.h, native.ptr(x), rows, n, native.ptr(z), native.ptr(codes), native.stream_ptr()),
                             "egr_dac_encode")
            else:
                native.check(native.lib().egr_dacseg_encode(self.h, native.ptr(x), rows, n, native.ptr(z), native.ptr(codes),
                                                                   native.ptr(ze) if return_ze else None, seg, native.stream_ptr()),
                             "egr_dacseg_encode")
        return (z, codes, ze) if return_ze else (z, codes)

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

    def decode(self, z: torch.Tensor, seg_frames: Optional[int] = None) -> torch.Tensor:
        """z [rows, latent, frames] -> y [rows, n_decoded] (not trimmed: DAC-P7); seg_frames as in encode."""
        z = self._rows(z, "decode", 3)
        rows, lat, frames = z.shape
        if lat != self.cfg["latent_dim"]:
            raise ValueError(f"DAC decode: {lat} channels, the model's latent_dim is {self.cfg['latent_dim']}")
        seg = self._path(rows, frames * dac_weights.hop(self.cfg), frames, DECODE, seg_frames)
        y = torch.empty((rows, decoded_length(self.cfg, frames)), dtype=torch.float32, device=z.device)
        with torch.cuda.device(self.device):
            if seg is None:
                native.check(native.lib().egr_dac_decode(self.h, native.ptr(z), rows, frames, native.ptr(y), native.stream_ptr()), "egr_dac_decode")
            else:
                native.check(native.lib().egr_dacseg_decode(self.h, native.ptr(z), rows, frames, native.ptr(y), seg, native.stream_ptr()),
                             "egr_dacseg_decode")
        return y

    def from_codes(self, codes: torch.Tensor) -> torch.Tensor:
        """codes [rows, n_codebooks, frames] (any integer dtype) -> z [rows, latent, frames]: the sum of the stages' out_proj of the
        chosen codebook rows, with the bits of the z of the encode that produced the codes.  Codes outside [0, codebook_size)
        raise ValueError before any device call."""
        if codes.dim() != 3 or not codes.is_cuda or codes.device.index != self.device or 0 in codes.shape or codes.is_floating_point():
            raise ValueError(f"DAC from_codes: expected non-empty integer codes [rows, n_codebooks, frames] on cuda:{self.device}, got "
                             f"{tuple(codes.shape)} {codes.dtype} on {codes.device}")
        rows, ncb, frames = codes.shape
        if ncb != self.cfg["n_codebooks"]:
            raise ValueError(f"DAC from_codes: {ncb} codebooks, the model has {self.cfg['n_codebooks']}")
        lo, hi = int(codes.min()), int(codes.max())
        if lo < 0 or hi >= self.cfg["codebook_size"]:
            raise ValueError(f"DAC from_codes: codes span [{lo}, {hi}], outside [0, {self.cfg['codebook_size']})")
        c32 = codes.to(torch.int32).contiguous()
        z = torch.empty((rows, self.cfg["latent_dim"], frames), dtype=torch.float32, device=codes.device)
        with torch.cuda.device(self.device):
            native.check(native.lib().egr_dacseg_from_codes(self.h, native.ptr(c32), rows, frames, native.ptr(z), native.stream_ptr()),
                         "egr_dacseg_from_codes")
        return z

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
