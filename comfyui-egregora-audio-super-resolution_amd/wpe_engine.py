"""WPE dereverberation on the device (SPEC.md 4d; csrc/egr_wpe.hip): framing, limits, the staged C calls and the whole chain.

Spectra are complex64 [bins][channels][frames]; every statistic, the factorisation and the filter sum run in double on the device
(WPE-P6).  There is no CPU path: a configuration outside the limits raises RuntimeError, a framing outside WPE-P3 is reported by
`framing_supported` so that the node can pass its input through as the reference's `except` branch does.
`dereverb_many` runs a list of clips of one channel count in one egr_wpemany_dereverb call.
"""
import numpy as np
import torch

from . import native

MAX_K = 64          # channels * taps (WPE-P7)
MAX_N_FFT = 4096
_WS = {}            # str(device) -> uint8 workspace, one per device, grown on demand


def window(n_fft: int) -> np.ndarray:
    """Periodic Blackman analysis window (WPE-P1), float64."""
    i = np.arange(n_fft, dtype=np.float64)
    return 0.42 - 0.5 * np.cos(2 * np.pi * i / n_fft) + 0.08 * np.cos(4 * np.pi * i / n_fft)


def synthesis_window(n_fft: int, hop: int) -> np.ndarray:
    """w[i] / sum_k w[(i mod hop) + k hop]^2 (WPE-P2), float64."""
    w = window(n_fft)
    den = (w.reshape(n_fft // hop, hop) ** 2).sum(axis=0)
    return w / np.tile(den, n_fft // hop)


def framing_supported(n_fft: int, hop: int) -> bool:
    """WPE-P3: hop divides n_fft and n_fft / hop >= 2."""
    return hop >= 1 and n_fft >= 2 and n_fft % hop == 0 and n_fft // hop >= 2


def check_k(channels: int, taps: int):
    """WPE-P7, the filter: raises RuntimeError naming the limit."""
    if channels * taps > MAX_K:
        raise RuntimeError(f"WPE: channels * taps = {channels * taps} exceeds the limit K <= {MAX_K} (no CPU fallback in this pack)")


def check_n_fft(n_fft: int):
    """WPE-P7, the transform: raises RuntimeError naming the limit."""
    if n_fft % 2 or n_fft > MAX_N_FFT:
        raise RuntimeError(f"WPE: n_fft = {n_fft} must be even and <= {MAX_N_FFT} (no CPU fallback in this pack)")


def check_limits(channels: int, taps: int, n_fft: int):
    """WPE-P7: raises RuntimeError naming the limit."""
    check_k(channels, taps)
    check_n_fft(n_fft)


def frames(n: int, n_fft: int, hop: int) -> int:
    return -(-(n + n_fft - 2 * hop) // hop) + 1


def out_length(n: int, n_fft: int, hop: int) -> int:
    return frames(n, n_fft, hop) * hop - (n_fft - hop)


def _rows(x: torch.Tensor) -> torch.Tensor:
    x = x.contiguous()
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] >= 1):
        raise RuntimeError("WPE: want a non-empty [C,T] float32 CUDA tensor")
    return x


def workspace(device, nbytes: int) -> torch.Tensor:
    ws = _WS.get(str(device))
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty((int(nbytes),), dtype=torch.uint8, device=device)
        _WS[str(device)] = ws
    return ws


def stft(x: torch.Tensor, n_fft: int, hop: int) -> torch.Tensor:
    """[C,T] float32 -> complex64 [bins][C][frames] (egr_wpe_stft)."""
    x = _rows(x)
    C, n = x.shape
    check_n_fft(n_fft)
    Y = torch.empty((n_fft // 2 + 1, C, frames(n, n_fft, hop)), dtype=torch.complex64, device=x.device)
    native.check(native.lib().egr_wpe_stft(native.ptr(x), C, n, n_fft, hop, native.ptr(Y), native.stream_ptr()), "egr_wpe_stft")
    return Y


def istft(Y: torch.Tensor, n_fft: int, hop: int) -> torch.Tensor:
    """complex64 [bins][C][frames] -> [C][frames * hop - (n_fft - hop)] float32 (egr_wpe_istft)."""
    Y = Y.contiguous()
    bins, C, fr = Y.shape
    if not (Y.is_cuda and Y.dtype == torch.complex64 and bins == n_fft // 2 + 1):
        raise RuntimeError("WPE: want complex64 CUDA spectra [n_fft / 2 + 1][C][frames]")
    n_out = fr * hop - (n_fft - hop)
    y = torch.empty((C, n_out), dtype=torch.float32, device=Y.device)
    native.check(native.lib().egr_wpe_istft(native.ptr(Y), C, fr, n_fft, hop, native.ptr(y), n_out, native.stream_ptr()), "egr_wpe_istft")
    return y


def iterate(Y: torch.Tensor, inv, taps: int, delay: int, want_x=True, want_g=False, want_inv=True):
    """One WPE-P4 iteration on every bin (egr_wpe_iterate).  inv: float64 [bins][frames] or None (formed from Y).
    -> dict with X (complex64), G (complex128 [bins][K][C]), inv (float64, the next iteration's), flags (int32 [bins]) as asked."""
    Y = Y.contiguous()
    bins, C, fr = Y.shape
    if not (Y.is_cuda and Y.dtype == torch.complex64):
        raise RuntimeError("WPE: want complex64 CUDA spectra [bins][C][frames]")
    check_k(C, taps)
    dev = Y.device
    out = {"flags": torch.empty((bins,), dtype=torch.int32, device=dev)}
    if want_x:
        out["X"] = torch.empty_like(Y)
    if want_g:
        out["G"] = torch.empty((bins, C * taps, C), dtype=torch.complex128, device=dev)
    if want_inv:
        out["inv"] = torch.empty((bins, fr), dtype=torch.float64, device=dev)
    ws = None
    if inv is None:
        ws = torch.empty((bins, fr), dtype=torch.float64, device=dev)      # the first iteration leaves its own weights here
    else:
        inv = inv.contiguous()
        if not (inv.is_cuda and inv.dtype == torch.float64 and tuple(inv.shape) == (bins, fr)):
            raise RuntimeError("WPE: inv must be float64 CUDA [bins][frames]")
    p = lambda k: native.ptr(out[k]) if k in out else None
    native.check(native.lib().egr_wpe_iterate(native.ptr(Y), native.ptr(inv) if inv is not None else None, bins, C, fr, taps, delay,
                                              p("X"), p("G"), p("inv"), p("flags"), native.ptr(ws) if ws is not None else None,
                                              ws.numel() * 8 if ws is not None else 0,
                                              native.stream_ptr()), "egr_wpe_iterate")
    return out


def dereverb(x: torch.Tensor, n_fft: int, hop: int, taps: int, delay: int, iterations: int) -> torch.Tensor:
    """[C,T] float32 CUDA -> [C][frames * hop - (n_fft - hop)]: stft, `iterations` iterations, istft in one call (egr_wpe_dereverb)."""
    x = _rows(x)
    C, n = x.shape
    check_limits(C, taps, n_fft)
    if not framing_supported(n_fft, hop):
        raise RuntimeError(f"WPE: hop = {hop} must divide n_fft = {n_fft} with n_fft / hop >= 2")
    L = native.lib()
    n_out = out_length(n, n_fft, hop)
    nbytes = int(L.egr_wpe_workspace_bytes(C, n, n_fft, hop, taps))
    ws = workspace(x.device, nbytes)
    y = torch.empty((C, n_out), dtype=torch.float32, device=x.device)
    native.check(L.egr_wpe_dereverb(native.ptr(x), C, n, n_fft, hop, taps, delay, iterations, native.ptr(y), n_out, native.ptr(ws),
                                    ws.numel(), native.stream_ptr()), "egr_wpe_dereverb")
    return y


def clip_table(lengths, channels: int, n_fft: int, hop: int):
    """The host table of egr_wpemany_*: clips packed one after the other in x and in y.  lengths: samples per channel of each clip ->
    (ctypes int64 [n][3] of (offset in x, n, offset in y), floats of x, floats of y)."""
    import ctypes
    tab = (ctypes.c_int64 * (3 * len(lengths)))()
    xo = yo = 0
    for i, n in enumerate(lengths):
        tab[3 * i], tab[3 * i + 1], tab[3 * i + 2] = xo, int(n), yo
        xo += channels * int(n)
        yo += channels * out_length(int(n), n_fft, hop) if n >= 1 else 0
    return tab, xo, yo


def many_workspace_bytes(lengths, channels: int, n_fft: int, hop: int, taps: int) -> int:
    """egr_wpemany_workspace_bytes of a wave of clips (host only): 0 for a wave the call would refuse."""
    tab, _, _ = clip_table(lengths, channels, n_fft, hop)
    return int(native.lib().egr_wpemany_workspace_bytes(tab, len(lengths), channels, n_fft, hop, taps))


def many_layout(lengths, channels: int, n_fft: int, hop: int):
    """Where egr_wpemany_dereverb keeps each clip in its workspace (include/egregora_amd.h): per clip, in input order, the byte offsets
    {"Y", "X", "inv0", "inv1", "flags"} and "frames".  The blocks follow one another longest clip first, equal lengths in input order."""
    bins = n_fft // 2 + 1
    al = lambda b: (b + 255) & ~255
    out, off = [None] * len(lengths), 0
    for i in sorted(range(len(lengths)), key=lambda i: -int(lengths[i])):
        fr = frames(int(lengths[i]), n_fft, hop)
        spec, inv = al(bins * channels * fr * 8), al(bins * fr * 8)
        out[i] = {"Y": off, "X": off + spec, "inv0": off + 2 * spec, "inv1": off + 2 * spec + inv, "flags": off + 2 * spec + 2 * inv,
                  "frames": fr}
        off += 2 * spec + 2 * inv + al(bins * 4)
    return out


def dereverb_many(xs, n_fft: int, hop: int, taps: int, delay: int, iterations: int):
    """A list of [C, T_i] float32 CUDA tensors of one channel count -> [C, out_length(T_i)] tensors, each the bits of `dereverb` on
    that clip alone, in ONE egr_wpemany_dereverb call: 2 + iterations launches whatever the number of clips.  The results are views
    of one flat tensor."""
    xs = [_rows(x) for x in xs]
    if not xs:
        return []
    C = xs[0].shape[0]
    if any(x.shape[0] != C or x.device != xs[0].device for x in xs):
        raise RuntimeError("WPE: the clips of one call share a channel count and a device")
    check_limits(C, taps, n_fft)
    if not framing_supported(n_fft, hop):
        raise RuntimeError(f"WPE: hop = {hop} must divide n_fft = {n_fft} with n_fft / hop >= 2")
    L = native.lib()
    lengths = [x.shape[1] for x in xs]
    tab, x_floats, y_floats = clip_table(lengths, C, n_fft, hop)
    nbytes = int(L.egr_wpemany_workspace_bytes(tab, len(xs), C, n_fft, hop, taps))
    if nbytes == 0:
        raise RuntimeError("WPE: egr_wpemany_workspace_bytes refuses this wave (limits of include/egregora_amd.h)")
    dev = xs[0].device
    x = xs[0].reshape(-1) if len(xs) == 1 else torch.cat([v.reshape(-1) for v in xs])
    y = torch.empty((y_floats,), dtype=torch.float32, device=dev)
    ws = workspace(dev, nbytes)
    native.check(L.egr_wpemany_dereverb(native.ptr(x), tab, len(xs), C, n_fft, hop, taps, delay, iterations, native.ptr(y), native.ptr(ws),
                                        ws.numel(), native.stream_ptr()), "egr_wpemany_dereverb")
    return [y[tab[3 * i + 2]:tab[3 * i + 2] + C * out_length(n, n_fft, hop)].view(C, -1) for i, n in enumerate(lengths)]
