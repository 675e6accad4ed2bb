"""The evaluation pack's loudness meter (reference egregora_audio_eval_pack.py:132-214) on the device.

Per sample everything runs in libegregora_amd.so: `egr_loudness_frames` K-weights every channel, takes the channel mean and
forms the 400 ms / 100 ms and 3 s / 1 s block mean squares in one call (csrc/egr_glue.hip: k_kweight_mono, k_frame_meansq);
`egr_true_peak` takes the maximum of the oversampled channel mean without storing it (k_true_peak).  What is left -- a few hundred
block values at most -- stays on the host in the reference's own numpy expressions, so equal block energies give the reference's
floats bit for bit: the -10 LU gate (:168-174), the float32 level series (:183-188), the percentile range (:191-200).
"""
import math

import numpy as np
import torch

from . import native, resample

_TAPS = {}


def block_shape(sr: int, window_s: float, hop_s: float, n: int):
    """(block, hop, frames) of the reference's series (:157-159, :180-182)."""
    w = max(1, int(round(window_s * sr)))
    h = max(1, int(round(hop_s * sr)))
    return w, h, 1 + max(0, (int(n) - w) // h)


def _rows(x_ct: torch.Tensor) -> torch.Tensor:
    x = x_ct[None, :] if x_ct.dim() == 1 else x_ct
    x = x.contiguous()
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] >= 1):
        raise RuntimeError("loudness: want a non-empty [C,N] float32 CUDA tensor")
    return x


def _taps(oversample: int, device):
    key = (int(oversample), str(device))
    if key not in _TAPS:
        h, half = resample.design_filter(int(oversample), 1)
        _TAPS[key] = (torch.from_numpy(h).to(device), half)
    return _TAPS[key]


def engine(x_ct: torch.Tensor, sr: int, short_term: bool = True, oversample: int = 0):
    """-> (ms_a, ms_b, peak): float64 host arrays of the 400 ms / 100 ms and (short_term) 3 s / 1 s block mean squares of the K-weighted
    channel mean, and (oversample >= 1) the linear true peak, else None.  One egr_loudness_frames, at most one egr_true_peak, one
    device -> host copy."""
    x = _rows(x_ct)
    C, n = x.shape
    k = math.exp(-2 * math.pi * (60.0 / (sr * 0.5)))
    wa, ha, fa = block_shape(sr, 0.400, 0.100, n)
    wb, hb, fb = block_shape(sr, 3.0, 1.0, n) if short_term else (1, 1, 0)
    mono = torch.empty((n,), dtype=torch.float32, device=x.device)
    buf = torch.empty((fa + fb + 1,), dtype=torch.float64, device=x.device)       # block values, then the 4-byte peak slot
    base = buf.data_ptr()
    L = native.lib()
    native.check(L.egr_loudness_frames(native.ptr(x), C, n, float(np.float32(1 - k)), float(np.float32(k)), wa, ha, fa, wb, hb, fb,
                                       native.ptr(mono), base, base + 8 * fa if fb else None, native.stream_ptr()), "egr_loudness_frames")
    if oversample:
        h, half = (None, 0) if int(oversample) == 1 else _taps(oversample, x.device)
        native.check(L.egr_true_peak(native.ptr(x), C, n, int(oversample), native.ptr(h) if h is not None else None, half,
                                     base + 8 * (fa + fb), native.stream_ptr()), "egr_true_peak")
    host = buf.cpu()
    ms = host[:fa + fb].numpy()
    peak = float(host[fa + fb:].view(torch.float32)[0]) if oversample else None
    return ms[:fa], ms[fa:], peak


def chunking(sr: int):
    """(L, W) of the K-weighting kernels at this rate, from the library (egr_kweight_chunking): a thread owns L samples and restarts
    the recurrence W samples ahead of them."""
    import ctypes as C
    k = math.exp(-2 * math.pi * (60.0 / (sr * 0.5)))
    L, W = C.c_int(0), C.c_int(0)
    native.check(native.lib().egr_kweight_chunking(float(np.float32(k)), C.byref(L), C.byref(W)), "egr_kweight_chunking")
    return L.value, W.value


def flat_offsets(xs):
    """(base pointer, [offset in floats]) of contiguous float32 CUDA tensors of one device: the tables of the many-clip calls address
    every clip from the lowest data pointer, so tensors that already sit on the device are not gathered into one buffer first."""
    base = min(x.data_ptr() for x in xs)
    return base, [(x.data_ptr() - base) // 4 for x in xs]


def many_args(lengths, sr: int, short_term: bool):
    """Host side of one egr_loudness_tracks call: (k, (blk_a, hop_a, blk_b, hop_b), [frames_a], [frames_b]) for clips of `lengths` samples."""
    k = math.exp(-2 * math.pi * (60.0 / (sr * 0.5)))
    wa, ha, _ = block_shape(sr, 0.400, 0.100, 1)
    wb, hb, _ = block_shape(sr, 3.0, 1.0, 1) if short_term else (0, 0, 0)
    fa = [block_shape(sr, 0.400, 0.100, n)[2] for n in lengths]
    fb = [block_shape(sr, 3.0, 1.0, n)[2] if short_term else 0 for n in lengths]
    return k, (wa, ha, wb, hb), fa, fb


def many_workspace_bytes(lengths, channels: int, sr: int, short_term: bool = True, oversample: int = 0) -> int:
    """egr_loudness_tracks_workspace_bytes for clips of `lengths` samples laid back to back (host only; 0: refused)."""
    import ctypes as C
    k, (wa, ha, wb, hb), _, _ = many_args(lengths, sr, short_term)
    rows, pos = [], 0
    for n in lengths:
        rows += [pos, int(n)]
        pos += int(channels) * int(n)
    tab = (C.c_int64 * len(rows))(*rows)
    return int(native.lib().egr_loudness_tracks_workspace_bytes(tab, len(lengths), int(channels), float(np.float32(k)), wa, ha, wb, hb,
                                                                int(oversample)))


def engine_many(xs, sr: int, short_term: bool = True, oversample: int = 0, stats: dict = None):
    """engine() for many clips of one sample rate and one channel count: xs = [C,N] float32 CUDA tensors -> [(ms_a, ms_b, peak)] with
    the bits engine() gives each clip.  One egr_loudness_tracks call, one device -> host copy."""
    import ctypes as C
    xs = [_rows(x) for x in xs]
    Cn = xs[0].shape[0]
    if any(x.shape[0] != Cn or x.device != xs[0].device for x in xs):
        raise RuntimeError("loudness.engine_many: the clips of one call share a channel count and a device")
    lengths = [x.shape[1] for x in xs]
    k, (wa, ha, wb, hb), fa, fb = many_args(lengths, sr, short_term)
    base, offs = flat_offsets(xs)
    tab = (C.c_int64 * (2 * len(xs)))(*[v for o, n in zip(offs, lengths) for v in (o, n)])
    L = native.lib()
    kf = float(np.float32(k))
    need = int(L.egr_loudness_tracks_workspace_bytes(tab, len(xs), Cn, kf, wa, ha, wb, hb, int(oversample)))
    if need == 0:
        raise RuntimeError(f"egr_loudness_tracks refused: {native.last_error()}")
    dev = xs[0].device
    ta, tb = sum(fa), sum(fb)
    buf = torch.empty((ta + tb + (len(xs) + 1) // 2,), dtype=torch.float64, device=dev)      # block values, then the 4-byte peak slots
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    h, half = (None, 0) if int(oversample) <= 1 else _taps(oversample, dev)
    launches = C.c_int(0)
    native.check(L.egr_loudness_tracks(C.c_void_p(base), tab, len(xs), Cn, float(np.float32(1 - k)), kf, wa, ha, wb, hb, int(oversample),
                                       native.ptr(h) if h is not None else None, half, native.ptr(buf), native.ptr(ws), need,
                                       C.byref(launches), native.stream_ptr()), "egr_loudness_tracks")
    host = buf.cpu()
    ms = host[:ta + tb].numpy()
    peaks = host[ta + tb:].view(torch.float32)
    if stats is not None:
        stats["library_calls"] = stats.get("library_calls", 0) + 1
        stats["launches"] = stats.get("launches", 0) + launches.value
    out, pa, pb = [], 0, ta
    for i in range(len(xs)):
        out.append((ms[pa:pa + fa[i]], ms[pb:pb + fb[i]], float(peaks[i]) if oversample else None))
        pa, pb = pa + fa[i], pb + fb[i]
    return out


def measure_finish(ms_a, ms_b, peak, compute_true_peak: bool) -> dict:
    """The meter node's dictionary from the block values and the peak: measure and eval_many.loudness_many both end here."""
    st = series(ms_b)
    out = {"lufs_integrated": float(gate(ms_a)), "lufs_momentary": float(series(ms_a).mean()), "lufs_short_term": float(st.mean()),
           "lra": float(lra(st))}
    if compute_true_peak:
        out["true_peak_dbfs"] = float(20.0 * math.log10(peak + 1e-20))
    return out


def gate(ms: np.ndarray) -> float:
    """Block mean squares -> gated loudness, the reference's expressions (:168-174)."""
    ms = np.asarray(ms) + 1e-20
    lufs_ungated = -0.691 + 10.0 * np.log10(np.mean(ms))
    gate_ = lufs_ungated - 10.0
    mask = (-0.691 + 10.0 * np.log10(ms)) >= gate_
    if np.any(mask):
        ms = ms[mask]
    return float(-0.691 + 10.0 * np.log10(np.mean(ms)))


def series(ms: np.ndarray) -> np.ndarray:
    """Block mean squares -> the float32 level series of lufs_series (:183-188)."""
    out = np.empty((len(ms),), dtype=np.float32)
    for i in range(len(ms)):
        out[i] = -0.691 + 10.0 * np.log10(float(ms[i]) + 1e-20)
    return out


def lra(st: np.ndarray) -> float:
    """Short-term series -> loudness range (lra_short_term, :191-200)."""
    if st.size == 0:
        return 0.0
    gate_ = np.percentile(st, 10.0) - 20.0
    pool = st[st > gate_]
    if pool.size == 0:
        pool = st
    return float(np.percentile(pool, 95.0) - np.percentile(pool, 10.0))


def integrated(x_ct: torch.Tensor, sr: int) -> float:
    """integrated_lufs (:153-174) of a [C,N] CUDA signal."""
    return gate(engine(x_ct, sr, short_term=False)[0])


def true_peak_dbfs(x_ct: torch.Tensor, oversample: int = 4) -> float:
    """true_peak_dbfs (:203-214, scipy branch) of a [C,N] CUDA signal."""
    x = _rows(x_ct)
    slot = torch.empty((1,), dtype=torch.float32, device=x.device)
    h, half = (None, 0) if int(oversample) == 1 else _taps(oversample, x.device)
    native.check(native.lib().egr_true_peak(native.ptr(x), x.shape[0], x.shape[1], int(oversample), native.ptr(h) if h is not None else None,
                                            half, native.ptr(slot), native.stream_ptr()), "egr_true_peak")
    return 20.0 * math.log10(float(slot.cpu()[0]) + 1e-20)


def measure(x_ct: torch.Tensor, sr: int, compute_true_peak: bool = True, oversample: int = 4) -> dict:
    """The meter node's dictionary (Loudness_Meter_1770.execute, :324-333), keys in the reference's order."""
    ms_a, ms_b, peak = engine(x_ct, sr, True, int(oversample) if compute_true_peak else 0)
    return measure_finish(ms_a, ms_b, peak, compute_true_peak)
