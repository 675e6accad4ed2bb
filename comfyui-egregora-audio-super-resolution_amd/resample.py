"""Sample-rate conversion for the FlashSR node on the device.

Mirrors the branch of the reference's `_resample_hq` that runs when scipy is present and soxr is not
(egregora_audio_super_resolution.py:178-187; requirements.txt lists scipy, not soxr): per channel
`scipy.signal.resample_poly(x, up=dst/g, down=src/g)` with the default Kaiser(5.0) design, float32 data.
The FIR is designed on the host (numpy restatement of scipy.signal.firwin, a few thousand taps at most) and the
polyphase evaluation runs in csrc/egr_glue.hip::k_resample_poly with scipy's accumulation order.

The second half of the file is the reference's other resampler, torchaudio.functional.resample (windowed sinc, SPEC.md 4f):
design_sinc / resample_sinc / resample_sinc_group on csrc/egr_resample_sinc.hip, used by the nodes only under
EGREGORA_SINC_RESAMPLE=1 (reference_torchaudio_enabled, codec_resample).
"""
from math import gcd

import numpy as np
import torch

from . import device_ops, native
from .many_common import clip_views, track_rows

_FILTERS = {}


def design_filter(up: int, down: int, beta: float = 5.0):
    """float32 taps h (already multiplied by `up`) and half length, as scipy.signal.resample_poly builds them:
    firwin(2*half+1, 1/max(up,down), window=('kaiser', beta)) with half = 10*max(up,down)."""
    mx = max(up, down)
    half = 10 * mx
    numtaps = 2 * half + 1
    cutoff = 1.0 / mx
    m = np.arange(numtaps, dtype=np.float64) - 0.5 * (numtaps - 1)
    h = cutoff * np.sinc(cutoff * m)            # ideal low-pass (fs = 2): right band edge only
    h *= np.kaiser(numtaps, beta)
    h /= np.sum(h)                              # unit gain at DC (scale=True)
    h32 = h.astype(np.float32)
    h32 *= np.float32(up)                       # scipy: h *= up after the cast to x.dtype
    return h32, half


def rates(src_sr: int, dst_sr: int):
    g = gcd(int(src_sr), int(dst_sr))
    return int(dst_sr) // g, int(src_sr) // g


def filter_for(up: int, down: int, device):
    """(taps on `device`, half) of design_filter(up, down), designed once per (up, down, device)."""
    key = (up, down, str(device))
    if key not in _FILTERS:
        h, half = design_filter(up, down)
        _FILTERS[key] = (torch.from_numpy(h).to(device), half)
    return _FILTERS[key]


def resample_hq(x_ct: torch.Tensor, src_sr: int, dst_sr: int) -> torch.Tensor:
    """[C,T] float32 CUDA -> [C, ceil(T*up/down)] float32 CUDA."""
    if int(src_sr) == int(dst_sr):
        return x_ct.to(torch.float32)
    if not (x_ct.is_cuda and x_ct.dim() == 2):
        raise RuntimeError("resample_hq wants a [C,T] tensor on the GPU")
    x = x_ct.to(torch.float32).contiguous()
    up, down = rates(src_sr, dst_sr)
    h, half = filter_for(up, down, x.device)
    C, n_in = x.shape
    n_out = (n_in * up + down - 1) // down
    y = torch.empty((C, n_out), dtype=torch.float32, device=x.device)
    native.check(native.lib().egr_resample_poly(native.ptr(x), C, n_in, up, down, native.ptr(h), half, native.ptr(y),
                                                n_out, native.stream_ptr()), "egr_resample_poly")
    return y


def poly_track_table(in_offsets, n_ins, up: int, down: int):
    """egr_resample_poly_tracks' table for one rate group: int64 [T,4] rows (in offset, n_in, out offset, n_out) with
    n_out = ceil(n_in * up / down) and the outputs back to back from 0; -> (table, total_out)."""
    n_in = np.asarray(n_ins, dtype=np.int64).reshape(-1)
    n_out = (n_in * up + down - 1) // down
    ends = np.cumsum(n_out)
    tab = np.stack([np.asarray(in_offsets, dtype=np.int64).reshape(-1), n_in, ends - n_out, n_out], axis=1)
    return np.ascontiguousarray(tab), int(ends[-1]) if len(ends) else 0


def poly_group_flat(flat: torch.Tensor, shapes, src_sr: int, dst_sr: int, y: torch.Tensor = None):
    """One egr_resample_poly_tracks call on clips that already lie back to back in `flat` ([C_i][T_i] each, shapes = [(C_i, T_i)]):
    -> (y, table); many_common.clip_views(y, table, shapes) are the clips' results.  y: a flat device buffer to write from its
    start, or None for a fresh one."""
    up, down = rates(src_sr, dst_sr)
    tab, total = poly_track_table(*track_rows(shapes), up, down)
    h, half = filter_for(up, down, flat.device)
    if y is None:
        y = torch.empty(total, dtype=torch.float32, device=flat.device)
    device_ops.resample_poly_tracks(flat, torch.from_numpy(tab).to(flat.device), total, up, down, h, half, y)
    return y, tab


def resample_poly_group(xs, src_sr: int, dst_sr: int):
    """[C_i, T_i] device tensors at src_sr -> [C_i, ceil(T_i up / down)] at dst_sr with one egr_resample_poly_tracks call: the bits of
    resample_hq on each."""
    shapes = [tuple(x.shape) for x in xs]
    flat = torch.cat([x.to(torch.float32).reshape(-1) for x in xs])
    return clip_views(*poly_group_flat(flat, shapes, src_sr, dst_sr), shapes)


# ------------------------------------------------------------------ windowed sinc: torchaudio.functional.resample's definition
# SPEC.md 4f.  The reference's "torchaudio" mode of Resample Audio (HQ) (egregora_audio_eval_pack.py:512-515) and its codec path
# (egregora_audio_enhance_extras.py:66-75, :777) call torchaudio; this pack does not depend on it and restates the definition:
# per-phase taps designed here in float64 (numpy), evaluated by csrc/egr_resample_sinc.hip from a compact tap-major table.
SINC_BETA = 14.769656459379492            # torchaudio's default Kaiser beta
SINC_METHODS = ("sinc_interp_hann", "sinc_interp_kaiser")
SINC_FORCE_DIRECT = 0x1                   # EGR_SINC_FORCE_DIRECT (include/egregora_amd.h)
SINC_MAX_RATE = 1 << 24                   # SINC_MAX_RATE (csrc/egr_sinc_index.h)
_SINC_DESIGNS = {}
_SINC_FILTERS = {}


def reference_torchaudio_enabled() -> bool:
    """EGREGORA_SINC_RESAMPLE == "1", read when called: the "torchaudio" mode of Resample Audio (HQ) and the codec's rate conversion
    then use the windowed-sinc kernel as the reference uses torchaudio.  Unset, every node computes what it did before."""
    import os
    return os.environ.get("EGREGORA_SINC_RESAMPLE") == "1"


def sinc_geometry(src_sr: int, dst_sr: int, lowpass_filter_width: int = 6, rolloff: float = 0.99):
    """(o, n, base, width) of the definition: o = src / g, n = dst / g, base = min(o, n) rolloff, width = ceil(lpw o / base)."""
    src_sr, dst_sr = int(src_sr), int(dst_sr)
    if src_sr < 1 or dst_sr < 1:
        raise ValueError(f"design_sinc: sample rates must be at least 1 (got {src_sr} -> {dst_sr})")
    if int(lowpass_filter_width) < 1 or not (0.0 < float(rolloff) <= 1.0):
        raise ValueError(f"design_sinc: lowpass_filter_width must be at least 1 and rolloff in (0, 1] (got {lowpass_filter_width}, {rolloff})")
    g = gcd(src_sr, dst_sr)
    o, n = src_sr // g, dst_sr // g
    base = min(o, n) * float(rolloff)
    width = int(np.ceil(int(lowpass_filter_width) * o / base))
    return o, n, base, width


def sinc_taps_f64(p: np.ndarray, j: np.ndarray, o: int, n: int, base: float, width: int, lpw: int, method: str, beta: float):
    """float64 (taps K, unclamped t) of phases p [P] at the taps j [P][W] (0 <= j < L = 2 width + o), elementwise the definition."""
    tu = (-p.astype(np.float64)[:, None] / n + (j - width).astype(np.float64) / o) * base
    t = np.clip(tu, -float(lpw), float(lpw))
    if method == "sinc_interp_hann":
        win = np.cos(np.pi * t / (2.0 * lpw)) ** 2
    else:
        win = np.i0(beta * np.sqrt(1.0 - (t / lpw) ** 2)) / np.i0(beta)
    a = np.pi * t
    snc = np.where(a == 0.0, 1.0, np.sin(a) / np.where(a == 0.0, 1.0, a))
    return snc * win * (base / o), tu


def design_sinc(src_sr: int, dst_sr: int, lowpass_filter_width: int = 6, rolloff: float = 0.99, method: str = "sinc_interp_hann",
                beta=None):
    """-> (table, first_tap, (o, n, width, run)): the compact device table of the windowed-sinc filter, designed in float64 and
    cast to float32.  table float32 [run][n], tap-major: table[s][p] is tap first_tap[p] + s of phase p, the taps with
    |t| < lowpass_filter_width (one contiguous stretch per phase), zero filled to the longest stretch `run`; first_tap int32 [n],
    each inside [0, 2 width + o - run].  The dropped taps are the clamped ones: float64 round-off, at most 2^-50.
    Designed once per parameter tuple.  ValueError (naming the reduced ratio) when n (2 width + 2) floats exceed
    EGREGORA_SINC_TABLE_MB (default 256) or the ratio is beyond the kernel's range."""
    import os
    if method not in SINC_METHODS:
        raise ValueError(f"design_sinc: method must be one of {SINC_METHODS} (got {method!r})")
    beta = SINC_BETA if beta is None else float(beta)
    lpw = int(lowpass_filter_width)
    key = (int(src_sr), int(dst_sr), lpw, float(rolloff), method, beta if method == "sinc_interp_kaiser" else None)
    hit = _SINC_DESIGNS.get(key)
    if hit is not None:
        return hit
    o, n, base, width = sinc_geometry(src_sr, dst_sr, lpw, rolloff)
    L = 2 * width + o
    bound = min(L, 2 * width + 2)
    cap_mb = float(os.environ.get("EGREGORA_SINC_TABLE_MB", "256"))
    if o > SINC_MAX_RATE or n > SINC_MAX_RATE or n * bound * 4 > cap_mb * 2 ** 20 or n * bound > 2 ** 29:
        raise ValueError(f"design_sinc: {src_sr} -> {dst_sr} reduces to {o}:{n}: a table of {n} phases x {bound} taps "
                         f"({n * bound * 4 / 2 ** 20:.1f} MiB) is above EGREGORA_SINC_TABLE_MB = {cap_mb:g} or the kernel's range")
    # |t| < lpw  <=>  |j - width - p o / n| < lpw o / base <= width: the stretch of phase p lies inside the W taps from floor(p o / n) - 1
    W = min(L, 2 * width + 4)
    p = np.arange(n, dtype=np.int64)
    j0 = np.clip(p * o // n - 1, 0, L - W)
    j = j0[:, None] + np.arange(W)[None, :]
    K, tu = sinc_taps_f64(p, j, o, n, base, width, lpw, method, beta)
    inside = np.abs(tu) < lpw
    count = inside.sum(axis=1)
    first = j0 + np.argmax(inside, axis=1)
    run = int(count.max())
    first_tap = np.minimum(first, L - run)           # a late, short stretch starts earlier: its extra leading taps are zeros
    col = first_tap[:, None] + np.arange(run)[None, :] - j0[:, None]            # column of K per table entry
    ok = (col >= 0) & (col < W)
    colc = np.clip(col, 0, W - 1)
    ok &= np.take_along_axis(inside, colc, axis=1)
    table = np.where(ok, np.take_along_axis(K, colc, axis=1), 0.0).astype(np.float32)
    out = (np.ascontiguousarray(table.T), first_tap.astype(np.int32), (o, n, width, run))
    _SINC_DESIGNS[key] = out
    return out


def sinc_filter_for(device, src_sr: int, dst_sr: int, lowpass_filter_width: int = 6, rolloff: float = 0.99,
                    method: str = "sinc_interp_hann", beta=None):
    """(table, first_tap) on `device` and (o, n, width, run) of design_sinc, uploaded once per parameter tuple and device."""
    table, first_tap, geo = design_sinc(src_sr, dst_sr, lowpass_filter_width, rolloff, method, beta)
    key = (id(table), str(device))
    hit = _SINC_FILTERS.get(key)
    if hit is None:
        hit = (torch.from_numpy(table).to(device), torch.from_numpy(first_tap).to(device), table)     # table: keeps id() alive
        _SINC_FILTERS[key] = hit
    return hit[0], hit[1], geo


def sinc_staged(o: int, n: int, width: int) -> bool:
    """The kernel variant egr_resample_sinc takes by itself (sinc_staged of csrc/egr_sinc_index.h): staged when the input span of a
    256-output tile, ((n + 254) // n) o + 2 width + o floats, is at most 4096; from (o, n, width) alone."""
    return ((n + 254) // n) * o + 2 * width + o <= 4096


def sinc_out_len(n_in: int, o: int, n: int) -> int:
    return (int(n_in) * n + o - 1) // o


def resample_sinc(x_ct: torch.Tensor, src_sr: int, dst_sr: int, *, flags: int = 0, **params) -> torch.Tensor:
    """[C,T] float32 on the device -> [C, ceil(T n / o)]: torchaudio.functional.resample(x, src_sr, dst_sr, **params) restated
    (params: lowpass_filter_width, rolloff, method, beta as design_sinc takes them; egr_resample_sinc)."""
    if int(src_sr) == int(dst_sr):
        return x_ct.to(torch.float32)
    if not (x_ct.is_cuda and x_ct.dim() == 2):
        raise RuntimeError("resample_sinc wants a [C,T] tensor on the GPU")
    x = x_ct.to(torch.float32).contiguous()
    table, first_tap, (o, n, width, run) = sinc_filter_for(x.device, src_sr, dst_sr, **params)
    C, n_in = x.shape
    n_out = sinc_out_len(n_in, o, n)
    y = torch.empty((C, n_out), dtype=torch.float32, device=x.device)
    native.check(native.lib().egr_resample_sinc(native.ptr(x), C, n_in, o, n, width, run, native.ptr(table), native.ptr(first_tap),
                                                int(flags), native.ptr(y), n_out, native.stream_ptr()), "egr_resample_sinc")
    return y


def sinc_track_table(ins, lens, o: int, n: int):
    """egr_resample_sinc_tracks' table for one rate group (sinc_track_fill of csrc/egr_sinc_index.h): int64 [T,4] rows
    (in offset, n_in, out offset, n_out = ceil(n_in n / o)) with the outputs back to back, and their total."""
    tab = np.zeros((len(ins), 4), dtype=np.int64)
    pos = 0
    for t, (off, n_in) in enumerate(zip(ins, lens)):
        if n_in < 1:
            raise ValueError(f"sinc_track_table: track {t} is empty")
        n_out = sinc_out_len(n_in, o, n)
        tab[t] = (off, n_in, pos, n_out)
        pos += n_out
    if pos > (2 ** 32 - 1) // 256 * 256:
        raise ValueError(f"sinc_track_table: {pos} outputs are more than one call holds")
    return tab, pos


def sinc_group_flat(flat: torch.Tensor, shapes, src_sr: int, dst_sr: int, y: torch.Tensor = None, *, flags: int = 0, **params):
    """One egr_resample_sinc_tracks call on clips that already lie back to back in `flat` ([C_i][T_i] each, shapes = [(C_i, T_i)]):
    -> (y, table); many_common.clip_views(y, table, shapes) are the clips' results.  y: a flat device buffer to write from its
    start, or None for a fresh one."""
    table, first_tap, (o, n, width, run) = sinc_filter_for(flat.device, src_sr, dst_sr, **params)
    tab, total = sinc_track_table(*track_rows(shapes), o, n)
    if y is None:
        y = torch.empty(total, dtype=torch.float32, device=flat.device)
    sinc_tracks(flat, torch.from_numpy(tab).to(flat.device), total, (o, n, width, run), table, first_tap, y, flags)
    return y, tab


def resample_sinc_group(xs, src_sr: int, dst_sr: int, *, flags: int = 0, **params):
    """[C_i, T_i] device tensors at src_sr -> [C_i, ceil(T_i n / o)] at dst_sr with one egr_resample_sinc_tracks call: the bits of
    resample_sinc on each (the twin of resample_poly_group)."""
    if int(src_sr) == int(dst_sr):
        return [x.to(torch.float32) for x in xs]
    shapes = [tuple(x.shape) for x in xs]
    flat = torch.cat([x.to(torch.float32).reshape(-1) for x in xs])
    return clip_views(*sinc_group_flat(flat, shapes, src_sr, dst_sr, flags=flags, **params), shapes)


def sinc_tracks(x: torch.Tensor, tab_dev: torch.Tensor, total_out: int, geo, table: torch.Tensor, first_tap: torch.Tensor,
                y: torch.Tensor, flags: int = 0) -> torch.Tensor:
    """egr_resample_sinc_tracks on flat device buffers: y[0 .. total_out) is written."""
    o, n, width, run = geo
    if y.numel() < total_out:
        raise RuntimeError("sinc_tracks: output buffer shorter than total_out")
    native.check(native.lib().egr_resample_sinc_tracks(native.ptr(x), native.ptr(tab_dev), tab_dev.shape[0], int(total_out), o, n, width,
                                                       run, native.ptr(table), native.ptr(first_tap), int(flags), native.ptr(y),
                                                       native.stream_ptr()), "egr_resample_sinc_tracks")
    return y


# The codec's rate conversion (Egregora_DAC_Encode / _Decode, dac_many): the reference calls torchaudio.functional.resample with its
# defaults there (Hann, lowpass_filter_width 6, rolloff 0.99); this pack's polyphase kernel is deviation DAC-Q2 and stays the default.
def codec_resample(x, src_sr: int, dst_sr: int):
    """One [C,T] device tensor, or a list of them (one library call for the list), from src_sr to dst_sr: resample_sinc /
    resample_sinc_group at torchaudio's defaults when reference_torchaudio_enabled(), else resample_hq / resample_poly_group."""
    many = isinstance(x, (list, tuple))
    if reference_torchaudio_enabled():
        return resample_sinc_group(x, src_sr, dst_sr) if many else resample_sinc(x, src_sr, dst_sr)
    if many:
        return resample_poly_group(x, src_sr, dst_sr)
    return resample_hq(x, src_sr, dst_sr)
