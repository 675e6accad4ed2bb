"""Native DeepFilterNet backends of `Egregora DeepFilterNet Denoise` (egr_dfn3_* / egr_dfn2_* in libegregora_amd.so, csrc/egr_dfn3.hip).

One handle per (model directory, device), created from a validated model directory (dfn_weights.load / dfn2_weights.load) and kept
for the life of the process.  enhance() takes the 48 kHz signal while it is on the device and returns the denoised signal there, on
the current stream.  DfnEngine is the engine of both models; this module holds the DeepFilterNet3 one, dfn2_engine.py the other.

A long input runs in segments of `seg_frames` network frames with the state carried across the cuts (egr_dfn*_enhance_segmented,
DESIGN.md 7.3): the same bits as the one-pass call, a workspace that depends on seg_frames and not on the length.  enhance() picks the
path with choose_path() from the workspace budget EGREGORA_DFN_WORKSPACE_GB.

Many clips go through enhance_many(): their channels run side by side in one ragged pass per wave (egr_dfn*_enhance_tracks,
DESIGN.md 7.7), every clip with the bits of enhance() on it alone; plan_waves() packs the waves under the same budget.
"""
import ctypes as C
import os
import threading
from pathlib import Path
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import dfn_weights, native
from .many_common import budget_bytes, track_rows

_CACHE: Dict[Tuple[str, str, int], "DfnEngine"] = {}
_LOCK = threading.Lock()


ONE_PASS_MAX_FRAMES = (2 ** 31 - 1) // 4096     # egr_dfn*_enhance refuses more frames ("input too long")
SEGMENT_STEP = 64                               # choose_path picks segment lengths in multiples of this many frames
WORKSPACE_GB_ENV = "EGREGORA_DFN_WORKSPACE_GB"
# A choice, not a measurement: above the 52 GB of the longest case the repository documents (30 minutes of stereo), so
# every run measured so far stays on the one-pass path.  The two paths give the same bits, so the switch does not show in the output.
WORKSPACE_GB_DEFAULT = 64.0


class Segment(NamedTuple):
    """egr_dfn_segment (include/egregora_amd.h): half-open ranges, frames except out (samples); hi <= lo is an empty range."""
    net_lo: int
    net_hi: int
    scan_lo: int
    scan_hi: int
    spec_lo: int
    spec_hi: int
    asm_lo: int
    asm_hi: int
    out_lo: int
    out_hi: int


class SegmentC(C.Structure):
    _fields_ = [(f, C.c_int64) for f in Segment._fields]


def segment_count(fft_size: int, hop_size: int, n: int, seg_frames: int) -> int:
    return ((n + fft_size) // hop_size - 1) // seg_frames + 1


def segment_plan(fft_size: int, hop_size: int, conv_lookahead: int, df_order: int, df_lookahead: int, n: int, seg_frames: int,
                 index: int) -> Segment:
    """Segment `index` of a file of n samples cut every seg_frames network frames: the Python twin of egr_dfn_segment_plan.  The
    norms see input frame t + conv_lookahead for network frame t; mask, deep filter and synthesis lag the network by df_lookahead
    frames; a sample is written once all fft/hop frames over it are synthesised."""
    if not (fft_size > 0 and hop_size > 0 and fft_size % hop_size == 0 and conv_lookahead >= 0 and df_order >= 1
            and 0 <= df_lookahead < df_order and n >= 1 and seg_frames >= 1):
        raise ValueError("segment_plan: bad argument")
    nF, ov = (n + fft_size) // hop_size, fft_size // hop_size
    nseg = segment_count(fft_size, hop_size, n, seg_frames)
    if not 0 <= index < nseg:
        raise ValueError(f"segment_plan: segment {index} of {nseg}")
    first, last = index == 0, index == nseg - 1
    a = index * seg_frames
    b = nF if last else a + seg_frames
    scan_lo = 0 if first else min(nF, a + conv_lookahead)
    scan_hi = nF if last else min(nF, b + conv_lookahead)
    asm_lo = max(0, a - df_lookahead)
    asm_hi = nF if last else b - df_lookahead              # at or below asm_lo (even negative): nothing to assemble yet
    spec_lo = max(0, asm_lo - (df_order - 1 - df_lookahead))
    spec_hi = max(scan_hi, min(nF, asm_hi + df_lookahead))
    out_lo = 0 if first else min(n, max(0, asm_lo - ov + 1) * hop_size)
    out_hi = n if last else min(n, max(0, asm_hi - ov + 1) * hop_size)
    return Segment(a, b, scan_lo, scan_hi, spec_lo, spec_hi, asm_lo, asm_hi, out_lo, out_hi)


def segment_plan_c(fft_size: int, hop_size: int, conv_lookahead: int, df_order: int, df_lookahead: int, n: int, seg_frames: int,
                   index: int) -> Tuple[Segment, int]:
    """(segment, number of segments) from egr_dfn_segment_plan (host only: needs no GPU)."""
    sc, cnt = SegmentC(), C.c_int64()
    native.check(native.lib().egr_dfn_segment_plan(fft_size, hop_size, conv_lookahead, df_order, df_lookahead, n, seg_frames, index,
                                                   C.byref(sc), C.byref(cnt)), "egr_dfn_segment_plan")
    return Segment(*(int(getattr(sc, f)) for f in Segment._fields)), int(cnt.value)


def workspace_budget_bytes() -> int:
    return budget_bytes(WORKSPACE_GB_ENV, WORKSPACE_GB_DEFAULT)


def choose_path(nF: int, one_pass_bytes: int, budget_bytes: int, bytes_for: Callable[[int], int]) -> Optional[int]:
    """None: run the nF frames in one pass (they are within its limit and its workspace within the budget).  Else the segment length:
    the largest multiple of SEGMENT_STEP frames whose workspace bytes_for(seg_frames) fits the budget (bytes_for grows with
    seg_frames) and that a segment can have; raises when even SEGMENT_STEP frames do not fit."""
    if nF <= ONE_PASS_MAX_FRAMES and one_pass_bytes <= budget_bytes:
        return None
    if bytes_for(SEGMENT_STEP) > budget_bytes:
        raise RuntimeError(f"DeepFilterNet: a segment of {SEGMENT_STEP} frames needs {bytes_for(SEGMENT_STEP)} bytes of workspace, "
                           f"the budget ({WORKSPACE_GB_ENV}) is {budget_bytes}")
    lo, hi = 1, ONE_PASS_MAX_FRAMES // SEGMENT_STEP                                             # in steps; lo fits
    if bytes_for(hi * SEGMENT_STEP) <= budget_bytes:
        return hi * SEGMENT_STEP
    while hi - lo > 1:                                                                          # hi does not fit
        mid = (lo + hi) // 2
        if bytes_for(mid * SEGMENT_STEP) <= budget_bytes:
            lo = mid
        else:
            hi = mid
    return lo * SEGMENT_STEP


def plan_waves(channels: Sequence[int], frames: Sequence[int], bytes_for: Callable[[List[int]], int], budget_bytes: int,
               max_frames: int = ONE_PASS_MAX_FRAMES) -> Tuple[List[List[int]], List[int]]:
    """Waves of enhance_many: (clip indices per wave, clips that run alone).  Clip i has channels[i] tracks of frames[i] frames each;
    bytes_for(indices) is the workspace of one ragged call over those clips (it grows with every clip added).  A clip stays whole.
    The clips are taken by frame count, longest first (ties in input order), so that the recurrences of a wave's rows end together,
    and a wave closes before the clip that would take it past budget_bytes or past max_frames frames in all.  A clip over either
    limit on its own is in no wave but in the second list: it runs through enhance(), which segments."""
    order = sorted(range(len(frames)), key=lambda i: -int(frames[i]))
    rows = lambda i: int(channels[i]) * int(frames[i])
    waves: List[List[int]] = []
    alone: List[int] = []
    cur: List[int] = []
    used = 0
    for i in order:
        if rows(i) > max_frames or bytes_for([i]) > budget_bytes:
            alone.append(i)
            continue
        if cur and (used + rows(i) > max_frames or bytes_for(cur + [i]) > budget_bytes):
            waves.append(cur)
            cur, used = [], 0
        cur.append(i)
        used += rows(i)
    if cur:
        waves.append(cur)
    return waves, sorted(alone)


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

    def enhance(self, x48: torch.Tensor, seg_frames: Optional[int] = None) -> torch.Tensor:
        """x48 [C, T] float32 on this engine's device -> [C, T] on the same device, enqueued on the current stream.  seg_frames: run
        in segments of that many frames; None: one pass when the file is within its limit and its workspace within the budget
        (EGREGORA_DFN_WORKSPACE_GB), else the longest segments that fit (choose_path).  Both paths give the same bits."""
        if x48.dim() != 2 or not x48.is_cuda or x48.device.index != self.device:
            raise ValueError(f"{self.prefix}: expected [C, T] on cuda:{self.device}, got {tuple(x48.shape)} on {x48.device}")
        x = x48.to(torch.float32).contiguous()
        y = torch.empty_like(x)
        ch, n = x.shape
        if seg_frames is None and n >= 1:
            nF = (n + self._cfg.fft_size) // self._cfg.hop_size
            one_pass = self.workspace_bytes(ch, n) if nF <= ONE_PASS_MAX_FRAMES else 0
            seg_frames = choose_path(nF, one_pass, workspace_budget_bytes(), lambda s: self.segment_workspace_bytes(ch, s))
        with torch.cuda.device(self.device):
            if seg_frames is None:
                native.check(self._fn("enhance")(self.h, native.ptr(x), ch, n, native.ptr(y), native.stream_ptr()), f"{self.prefix}_enhance")
            else:
                native.check(self._fn("enhance_segmented")(self.h, native.ptr(x), ch, n, native.ptr(y), int(seg_frames), native.stream_ptr()),
                             f"{self.prefix}_enhance_segmented")
        return y

    def frames_of(self, n: int) -> int:
        """Frames of an n-sample track: (n + fft_size) // hop_size."""
        return (int(n) + self._cfg.fft_size) // self._cfg.hop_size

    @staticmethod
    def _track_table(offsets: Sequence[int], lengths: Sequence[int]):
        import numpy as np
        tab = np.ascontiguousarray(np.stack([np.asarray(offsets, dtype=np.int64).reshape(-1),
                                             np.asarray(lengths, dtype=np.int64).reshape(-1)], axis=1))
        return tab, tab.ctypes.data_as(C.c_void_p)

    def tracks_workspace_bytes(self, lengths: Sequence[int]) -> int:
        """The workspace of enhance_tracks over tracks of these lengths (it follows the sum of their frames); 0 for a set of lengths
        the call refuses."""
        tab, p = self._track_table([0] * len(lengths), lengths)
        return int(self._fn("tracks_workspace_bytes")(self.h, p, len(lengths)))

    def enhance_tracks(self, x: torch.Tensor, offsets: Sequence[int], lengths: Sequence[int], y: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One ragged pass (egr_dfn*_enhance_tracks).  x: a flat float32 buffer on this engine's device; track b (one
        channel of one clip) is x[offsets[b] : offsets[b] + lengths[b]], its output lands at the same place of y (flat, x's size when
        not given; what no track covers is left unwritten).  Every track gets the bits enhance() gives it alone."""
        if x.dim() != 1 or not x.is_cuda or x.device.index != self.device or x.dtype != torch.float32 or not x.is_contiguous():
            raise ValueError(f"{self.prefix}: expected a flat contiguous float32 buffer on cuda:{self.device}")
        if len(offsets) != len(lengths):
            raise ValueError(f"{self.prefix}: {len(offsets)} offsets, {len(lengths)} lengths")
        y = torch.empty_like(x) if y is None else y
        tab, p = self._track_table(offsets, lengths)
        with torch.cuda.device(self.device):
            native.check(self._fn("enhance_tracks")(self.h, native.ptr(x), p, len(lengths), native.ptr(y), native.stream_ptr()),
                         f"{self.prefix}_enhance_tracks")
        return y

    def enhance_many(self, rows: Sequence[torch.Tensor], stats: Optional[dict] = None) -> List[torch.Tensor]:
        """rows: [C_i, T_i] float32 tensors on this engine's device -> tensors of the same shapes there, on the current stream, each
        with the bits of enhance() on that clip alone.  The clips are packed into waves (plan_waves: workspace budget
        EGREGORA_DFN_WORKSPACE_GB, at most ONE_PASS_MAX_FRAMES frames), one enhance_tracks call per wave; a clip over a limit on its own
        goes through enhance(), which segments.  The results of a wave are views of that wave's one output buffer.  stats, when
        given, receives waves (clip indices per wave) and alone."""
        for i, x in enumerate(rows):
            if not torch.is_tensor(x) or x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1 or not x.is_cuda or x.device.index != self.device:
                raise ValueError(f"{self.prefix}: clip {i}: expected a non-empty [C, T] tensor on cuda:{self.device}")
        shapes = [(int(x.shape[0]), int(x.shape[1])) for x in rows]
        frames = [self.frames_of(T) for _, T in shapes]
        lengths_of = lambda idx: [shapes[i][1] for i in idx for _ in range(shapes[i][0])]
        waves, alone = plan_waves([c for c, _ in shapes], frames, lambda idx: self.tracks_workspace_bytes(lengths_of(idx)),
                                  workspace_budget_bytes())
        out: List[Optional[torch.Tensor]] = [None] * len(rows)
        for i in alone:
            out[i] = self.enhance(rows[i])
        for idx in waves:
            x = torch.cat([rows[i].to(torch.float32).reshape(-1) for i in idx])
            offs, lens = track_rows([shapes[i] for i in idx])
            y = self.enhance_tracks(x, offs, lens)
            pos = 0
            for i in idx:
                c, T = shapes[i]
                out[i] = y[pos:pos + c * T].view(c, T)
                pos += c * T
        if stats is not None:
            stats["waves"], stats["alone"] = [list(w) for w in waves], list(alone)
        return out

    def workspace_bytes(self, channels: int, n: int) -> int:
        return int(self._fn("workspace_bytes")(self.h, int(channels), int(n)))

    def segment_workspace_bytes(self, channels: int, seg_frames: int) -> int:
        """The workspace of a segmented call: it depends on the segment length, not on the input's."""
        return int(self._fn("segment_workspace_bytes")(self.h, int(channels), int(seg_frames)))

    def workspace_held(self) -> int:
        """Bytes of workspace the handle holds now (it grows to the largest call so far and is kept)."""
        return int(self._fn("workspace_held")(self.h))

    def segment_plan(self, n: int, seg_frames: int, index: int) -> Segment:
        """Segment `index` of an n-sample input as this model's handle cuts it."""
        c = self._cfg
        return segment_plan(c.fft_size, c.hop_size, c.conv_lookahead, c.df_order, c.df_lookahead, n, seg_frames, index)

    def stage(self, name: str, layer: int = 0) -> torch.Tensor:
        """An intermediate of the last enhance call as a flat float32 device tensor (layouts: include/egregora_amd.h); the names in
        `indexed` take the GRU layer index."""
        sid = self.stages[name] + (layer if name in self.indexed else 0)
        return native.read_stage(self._fn("stage"), f"{self.prefix}_stage", self.device, self.h, sid)

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
