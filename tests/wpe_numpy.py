"""Float64 numpy restatement of SPEC.md 4d (WPE-P1 .. P5): the framing, one WPE iteration per bin and the whole chain.

Written from the definitions, not from any implementation; `dtype` switches the spectra and every later step to complex64 /
float32 (the reference's use_float32 path) so that tests can measure that path's own error against complex128.
Spectra are [bins][channels][frames], stacked row i = k * channels + d is channel d delayed by delay + k frames.
"""
import numpy as np

PSD_FLOOR = 1e-10
PIVOT_FLOOR = 1e-13


def window(n_fft):
    i = np.arange(n_fft, dtype=np.float64)
    return 0.42 - 0.5 * np.cos(2 * np.pi * i / n_fft) + 0.08 * np.cos(4 * np.pi * i / n_fft)


def synthesis_window(n_fft, hop):
    w = window(n_fft)
    den = np.zeros(hop)
    for k in range(n_fft // hop):
        den += w[k * hop:(k + 1) * hop] ** 2
    return w / np.tile(den, n_fft // hop)


def framing_supported(n_fft, hop):
    return hop >= 1 and n_fft % hop == 0 and n_fft // hop >= 2


def frame_count(n, n_fft, hop):
    return -(-(n + n_fft - 2 * hop) // hop) + 1


def out_length(n, n_fft, hop):
    return frame_count(n, n_fft, hop) * hop - (n_fft - hop)


def analysis(y, n_fft, hop, real=np.float64):
    """y [C][T] -> [bins][C][frames]; real=np.float32 runs window product and FFT in single precision."""
    y = np.asarray(y, dtype=real)
    C, T = y.shape
    frames = frame_count(T, n_fft, hop)
    pad = n_fft - hop
    buf = np.zeros((C, (frames - 1) * hop + n_fft), dtype=real)
    buf[:, pad:pad + T] = y
    idx = np.arange(frames)[:, None] * hop + np.arange(n_fft)[None, :]
    seg = buf[:, idx] * window(n_fft).astype(real)                          # [C][frames][n_fft]
    Y = np.fft.rfft(seg, axis=-1)
    assert Y.dtype == (np.complex64 if real == np.float32 else np.complex128)
    return np.ascontiguousarray(Y.transpose(2, 0, 1))


def synthesis(Y, n_fft, hop, real=np.float64):
    """[bins][C][frames] -> [C][frames * hop - (n_fft - hop)]."""
    bins, C, frames = Y.shape
    seg = np.fft.irfft(Y.transpose(1, 2, 0), n=n_fft, axis=-1).astype(real) * synthesis_window(n_fft, hop).astype(real)
    out = np.zeros((C, (frames - 1) * hop + n_fft), dtype=real)
    for t in range(frames):
        out[:, t * hop:t * hop + n_fft] += seg[:, t]
    pad = n_fft - hop
    return out[:, pad:out.shape[1] - pad]


def stack(Y, taps, delay):
    """[bins][D][T] -> Ytilde [bins][K][T]."""
    bins, D, T = Y.shape
    Yt = np.zeros((bins, taps * D, T), dtype=Y.dtype)
    for k in range(taps):
        s = delay + k
        if s < T:
            Yt[:, k * D:(k + 1) * D, s:] = Y[:, :, :T - s]
    return Yt


def psd_inverse(X):
    """inv[t] = 1 / max(p[t], 1e-10 max_t p[t]),  p[t] = mean_d |X[d, t]|^2  (per bin); real dtype follows X."""
    p = np.mean(X.real ** 2 + X.imag ** 2, axis=1)
    with np.errstate(divide="ignore"):
        return 1.0 / np.maximum(p, p.dtype.type(PSD_FLOOR) * p.max(axis=1, keepdims=True))


def correlations(Y, inv, taps, delay):
    Yt = stack(Y, taps, delay)
    with np.errstate(invalid="ignore"):
        Yw = Yt * inv[:, None, :].astype(Y.real.dtype)
        R = Yw @ Yt.conj().transpose(0, 2, 1)
        P = Yw @ Y.conj().transpose(0, 2, 1)
    return Yt, R, P


def cholesky_guarded(R):
    """Lower Cholesky factors of a stack [bins][K][K] with the WPE-P5 guard: ok[b] False where a pivot <= 1e-13 max diag."""
    A = R.copy()
    bins, K, _ = A.shape
    with np.errstate(invalid="ignore"):
        thr = A.real.dtype.type(PIVOT_FLOOR) * np.max(np.real(np.einsum("bii->bi", A)), axis=1)
    ok = np.ones(bins, dtype=bool)
    L = np.zeros_like(A)
    with np.errstate(all="ignore"):
        for k in range(K):
            piv = A[:, k, k].real
            ok &= piv > thr
            l = np.sqrt(np.where(ok, piv, 1.0))
            L[:, k, k] = l
            col = A[:, k + 1:, k] / l[:, None]
            L[:, k + 1:, k] = col
            A[:, k + 1:, k + 1:] -= col[:, :, None] * col.conj()[:, None, :]
    return L, ok


def solve_guarded(R, P):
    """G = R^-1 P by Cholesky, G = 0 and ok False where the guard fires."""
    L, ok = cholesky_guarded(R)
    bins, K, D = P.shape
    G = np.zeros_like(P)
    with np.errstate(all="ignore"):
        W = P.copy()
        for k in range(K):                                                  # L W = P
            W[:, k] = W[:, k] / L[:, k, k][:, None]
            W[:, k + 1:] -= L[:, k + 1:, k][:, :, None] * W[:, k][:, None, :]
        for k in range(K - 1, -1, -1):                                      # L^H G = W
            W[:, k] = W[:, k] / L[:, k, k][:, None]
            W[:, :k] -= L[:, k, :k].conj()[:, :, None] * W[:, k][:, None, :]
    G[ok] = W[ok]
    return G, ok


def apply_filter(Y, G, taps, delay):
    return Y - G.conj().transpose(0, 2, 1) @ stack(Y, taps, delay)


def _two_sum(s, p):
    """s + p = t + e exactly (Knuth)."""
    t = s + p
    v = t - s
    return t, (s - (t - v)) + (p - v)


def apply_filter_compensated(Y, G, taps, delay):
    """Y - G^H Ytilde for spectra whose values are complex64 numbers (held as complex128), carried to about twice double precision
    and rounded once.  Each double of G is split into its float32 rounding and the rest (at most 29 bits), so both products with a
    24-bit sample are exact in double; the running sums collect their rounding errors by two-sum.  Where the prediction cancels the
    observation, a plain double evaluation (apply_filter) is off by eps times the size of the terms, which can exceed any bound
    relative to |X|; this one is off by eps |X|."""
    assert Y.dtype == np.complex128 and np.array_equal(Y, Y.astype(np.complex64))
    Yt = stack(Y, taps, delay)
    GH = G.conj().transpose(0, 2, 1)                                        # [bins][D][K]
    out = np.empty_like(Y)
    for part in (0, 1):
        s = (Y.imag if part else Y.real).copy()
        c = np.zeros_like(s)
        for i in range(Yt.shape[1]):
            gr, gi = GH[:, :, i].real[:, :, None], GH[:, :, i].imag[:, :, None]
            zr, zi = Yt[:, i].real[:, None, :], Yt[:, i].imag[:, None, :]
            for a, z in (((-gr, zi), (-gi, zr)) if part else ((-gr, zr), (gi, zi))):
                hi = a.astype(np.float32).astype(np.float64)
                for q in (hi, a - hi):
                    s, e = _two_sum(s, q * z)
                    c += e
        if part:
            out.imag = s + c
        else:
            out.real = s + c
    return out


def iterate(Y, inv, taps, delay):
    """One WPE-P4 iteration: (X, G, ok, R, P)."""
    _, R, P = correlations(Y, inv, taps, delay)
    G, ok = solve_guarded(R, P)
    X = Y.copy()
    X[ok] = apply_filter(Y[ok], G[ok], taps, delay)
    return X, G, ok, R, P


def wpe(Y, taps, delay, iterations, collect=None):
    """`iterations` iterations on spectra Y; collect (a list) receives (inv, R, P, G, ok) per iteration."""
    X = Y
    for _ in range(iterations):
        inv = psd_inverse(X)
        X, G, ok, R, P = iterate(Y, inv, taps, delay)
        if collect is not None:
            collect.append((inv, R, P, G, ok))
    return X


def dereverb(y, n_fft, hop, taps, delay, iterations, real=np.float64):
    Y = analysis(y, n_fft, hop, real)
    return synthesis(wpe(Y, taps, delay, iterations), n_fft, hop, real)


def max_condition(Y, taps, delay, iterations):
    """Largest 2-norm condition number of R over bins and iterations (complex128)."""
    col = []
    wpe(Y.astype(np.complex128), taps, delay, iterations, col)
    worst = 0.0
    for _, R, _, _, ok in col:
        assert ok.all()
        worst = max(worst, float(np.linalg.cond(R).max()))
    return worst


def rel_rms(a, b):
    return float(np.sqrt(np.sum(np.abs(a - b) ** 2) / np.sum(np.abs(b) ** 2)))
