"""numpy / scipy references for tests/test_gpu_glue_laps.py: every glue and metric kernel of csrc/egr_glue.hip restated on the
host, float32 where the kernel documents a float32 order (bit-exact cases), float64 where the test holds a rounding bound.
Nothing here touches the device."""
import numpy as np

F32 = np.float32
U24, U52 = 2.0 ** -24, 2.0 ** -52


def lap_n(lap: int) -> int:
    """Two full laps of a grid-stride kernel whose launcher stops at `lap` elements, and a ragged third one."""
    return 2 * lap + 3 * 256 + 37


def where_bad(bad, lap: int, what: str) -> str:
    """One line on the flat indices that failed a comparison, for the assertion message: how many, first, last, and how many of them
    lie inside the first lap (a launcher that loses later laps fails only past it)."""
    idx = np.flatnonzero(np.asarray(bad).reshape(-1))
    if idx.size == 0:
        return f"{what}: all equal"
    return (f"{what}: {idx.size} bad of {np.asarray(bad).size}, first {int(idx[0])}, last {int(idx[-1])}, "
            f"{int((idx < lap).sum())} inside the first lap of {lap}")


def bits_differ(got, want) -> np.ndarray:
    """Elementwise: the float32 bit patterns differ."""
    return np.ascontiguousarray(got, F32).view(np.uint32) != np.ascontiguousarray(want, F32).view(np.uint32)


# ---------------------------------------------------------------- float32 restatements (kernel's stated order)
def mono_mean32(x, n=None):
    """numpy's float32 .mean(axis=0): rows added in order, one division (k_mono_mean)."""
    x = np.asarray(x, F32)
    n = x.shape[1] if n is None else n
    m = x[0, :n].copy()
    for c in range(1, x.shape[0]):
        m = m + x[c, :n]
    return m / F32(x.shape[0]) if x.shape[0] > 1 else m


def gather_rows(flat, rows, win, hop):
    """egr_chunk_gather_tracks: row r = flat[off + k hop ...][:win] of the track (off, T, k), zero behind the track's end."""
    out = np.zeros((len(rows), win), F32)
    for r, (off, T, k) in enumerate(np.asarray(rows).tolist()):
        a = k * hop
        L = max(0, min(win, T - a))
        out[r, :L] = flat[off + a:off + a + L]
    return out


def shift_fir32(x, shift, h, n_out):
    """egr_shift_fir: s[i] = x[i - shift] inside [0, n_in) else 0; np.convolve(s, h, "same") with the float32 products added in
    order of k (taps = 0: s itself); cut or zero-padded to n_out."""
    x = np.asarray(x, F32)
    C, n = x.shape
    s = np.zeros_like(x)
    if abs(shift) < n:
        if shift >= 0:
            s[:, shift:] = x[:, :n - shift]
        else:
            s[:, :n + shift] = x[:, -shift:]
    y = s
    if h is not None and len(h):
        taps, off = len(h), (len(h) - 1) // 2
        pad = np.zeros((C, n + 2 * taps), F32)
        pad[:, taps:taps + n] = s
        y = np.zeros_like(s)
        for k in range(taps):                       # y[i] += h[k] * s[i + off - k]
            a = taps + off - k
            y = y + F32(h[k]) * pad[:, a:a + n]
    out = np.zeros((C, n_out), F32)
    m = min(n, n_out)
    out[:, :m] = y[:, :m]
    return out


def shift_fir64(x, shift, h, n_out):
    """The same through np.convolve(..., "same") in float64 (checks shift_fir32's indexing, not its rounding)."""
    x = np.asarray(x, np.float64)
    C, n = x.shape
    s = np.zeros_like(x)
    if abs(shift) < n:
        if shift >= 0:
            s[:, shift:] = x[:, :n - shift]
        else:
            s[:, :n + shift] = x[:, -shift:]
    if h is not None and len(h):
        s = np.stack([np.convolve(s[c], np.asarray(h, np.float64), "same") for c in range(C)])
    out = np.zeros((C, n_out))
    m = min(n, n_out)
    out[:, :m] = s[:, :m]
    return out


def dfn_mix32(dry, wet, gd, gw, hop, gain, limit, ceiling):
    """egr_dfn_mix in numpy float32, unfused: clip(g_dry[f] dry + g_wet[f] wet, -1, 1) * gain with f = min(i / hop, frames - 1), then the
    limiter on the peak of the whole tensor and the final clamp.  -> (y, peak before the limiter)."""
    C, T = dry.shape
    f = np.minimum(np.arange(T) // hop, gd.shape[1] - 1)
    y = np.empty_like(dry)
    for c in range(C):
        v = gd[c, f] * dry[c] + gw[c, f] * wet[c]
        y[c] = np.clip(v, F32(-1), F32(1))
    if gain is not None:
        y = y * F32(gain)
    peak = F32(np.abs(y).max())
    if limit and float(peak) > ceiling and peak > 0:
        y = y * F32(ceiling / float(peak))
    return np.clip(y, F32(-1), F32(1)).astype(F32), float(peak)


# ---------------------------------------------------------------- polyphase resampling in float64 on the float32 taps
def _upfirdn(h, x, up, down, half, n_out):
    """y[m] = sum_k h[m down - k up + half] x[k] for m < n_out, by scipy.signal.upfirdn: the taps are shifted by leading zeros so that
    m down + half falls on upfirdn's own grid, as scipy.signal.resample_poly does."""
    from scipy.signal import upfirdn
    pre = down - half % down
    skip = (half + pre) // down
    need = (skip + n_out - 1) * down + 1 - ((len(x) - 1) * up + pre + len(h))
    hp = np.concatenate([np.zeros(pre), h, np.zeros(max(0, need))])
    y = upfirdn(hp, x, up, down)
    return y[skip:skip + n_out]


def poly64(x, h32, up, down, half):
    """-> (y, S): the rational-rate FIR of k_resample_poly on float32 input and taps evaluated in float64, and S[m] = sum |h| |x|, the
    same evaluation on the magnitudes."""
    x = np.asarray(x, np.float64)
    h = np.asarray(h32, np.float64)
    n_out = (len(x) * up + down - 1) // down
    return _upfirdn(h, x, up, down, half, n_out), _upfirdn(np.abs(h), np.abs(x), up, down, half, n_out)


def poly_terms(up, half):
    """Taps that can meet one output: every up-th tap of 2 half + 1."""
    return (2 * half) // up + 1


def poly_direct(x, h32, up, down, half):
    """The definition by an explicit loop (slow; checks poly64 on short inputs)."""
    x = np.asarray(x, np.float64)
    h = np.asarray(h32, np.float64)
    n_out = (len(x) * up + down - 1) // down
    y = np.zeros(n_out)
    for m in range(n_out):
        t = m * down + half
        for k in range(len(x)):
            j = t - k * up
            if 0 <= j < len(h):
                y[m] += h[j] * x[k]
    return y


def n_out_of(n_in, up, down):
    return (n_in * up + down - 1) // down


def n_in_for(n_out, up, down):
    """Smallest n_in whose output is at least n_out samples long."""
    return ((n_out - 1) * down + up) // up


def _fill(pos, target, up, down):
    """Tracks (n_in values) whose outputs add up to target - pos exactly: one long track and up to seven of one sample; None when the
    rate cannot reach it."""
    one = n_out_of(1, up, down)
    for k in range(8):
        need = target - pos - k * one
        if need <= 0:
            return None
        n = n_in_for(need, up, down)
        if n_out_of(n, up, down) == need:
            return [n] + [1] * k
    return None


def poly_track_plan(up, down, lap):
    """Clips (channels, n_in) for egr_resample_poly_tracks whose outputs, back to back, put: one first track of at least lap + 100
    outputs; a track start exactly on a multiple of 256; short tracks of (about) 1, 255, 256, 257 and a few thousand outputs, 1 to 3
    channels per clip, all starting past the first lap; a track start exactly on a multiple of the lap; and an end in a ragged lap past
    2 lap + 805.  -> (clips, marks) with marks = {"at256": offset, "atlap": offset}."""
    clips, pos, marks = [], 0, {}

    def add(c, n):
        nonlocal pos
        clips.append((c, n))
        pos += c * n_out_of(n, up, down)

    add(1, n_in_for(lap + 100, up, down))
    t = (pos // 256 + 1) * 256
    while _fill(pos, t, up, down) is None:
        t += 256
    for n in _fill(pos, t, up, down):
        add(1, n)
    assert pos == t
    marks["at256"] = pos
    for c, m in ((2, 255), (3, 256), (1, 1), (2, 257), (3, 5000)):
        add(c, n_in_for(m, up, down))
    t = (pos // lap + 1) * lap
    while _fill(pos, t, up, down) is None:
        t += lap
    for n in _fill(pos, t, up, down):
        add(1, n)
    assert pos == t
    marks["atlap"] = pos
    for c, m in ((2, 4001), (1, 1), (3, 255)):
        add(c, n_in_for(m, up, down))
    if pos < lap_n(lap):
        add(1, n_in_for(lap_n(lap) - pos, up, down))
    return clips, marks


# ---------------------------------------------------------------- sums in double
def sum_bound(terms):
    """Worst case of any summation order in double: n 2^-52 sum |term|."""
    t = np.asarray(terms, np.float64)
    return t.size * U52 * float(np.abs(t).sum())


def pair_terms(a, b, n, k=None):
    """The five term series of k_pair_stats: mono means in float32 (b scaled by float32(k) first), products in double."""
    x = mono_mean32(a, n).astype(np.float64)
    bb = np.asarray(b, F32)[:, :n]
    if k is not None:
        bb = bb * F32(k)
    y = mono_mean32(bb, n).astype(np.float64)
    return [x, y, x * y, x * x, y * y]


def linear64(x, n_out):
    """np.interp over the two endpoint-free grids, per row, in float64 (k_resample_linear)."""
    x = np.asarray(x, np.float64)
    t_old = np.linspace(0.0, 1.0, x.shape[1], endpoint=False)
    t_new = np.linspace(0.0, 1.0, n_out, endpoint=False)
    return np.stack([np.interp(t_new, t_old, r) for r in x])
