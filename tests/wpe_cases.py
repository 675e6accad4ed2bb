"""Inputs of the WPE tests (SPEC.md 4d): seeded reverberant mixtures whose conditioning tests/test_wpe_host.py asserts.

Every channel is s_c + 0.5 s_{c+1} (independent Gaussian sources) through its own 0.3 s exponentially decaying noise impulse
response (-60 dB at its end), plus white noise at 0.05.  Class "well": cond(R) <= 1e4 in every bin and iteration, where a forward
error against complex128 means something; class "hard": cond(R) > 1e6 somewhere, where only backward errors are compared.
If a case leaves its class after a change of the generator, change the input, not the cap.
"""
import numpy as np

SR = 16000
WELL_MAX_COND = 1e4
HARD_MIN_COND = 1e6

CASES = {
    "A": dict(channels=1, n=16000, n_fft=256, hop=64, taps=3, delay=1, iterations=1, seed=101, cls="well"),
    "B": dict(channels=3, n=32000, n_fft=256, hop=64, taps=5, delay=2, iterations=2, seed=102, cls="well"),
    "C": dict(channels=2, n=32000, n_fft=256, hop=64, taps=10, delay=3, iterations=3, seed=103, cls="hard"),
    "D": dict(channels=2, n=48000, n_fft=256, hop=64, taps=32, delay=1, iterations=2, seed=104, cls="hard"),
    "E": dict(channels=2, n=64000, n_fft=768, hop=192, taps=10, delay=3, iterations=3, seed=105, cls="hard"),
    # wide arrays on a short transform (33 bins, 753 / 503 frames), for tests/test_gpu_wpe_configs.py: F and G need two 4 x 4 blocks
    # per thread, G, H and L the 32-frame tile of more than 32 channels, L the last delay whose tile still fits in LDS
    "F": dict(channels=32, n=12000, n_fft=64, hop=16, taps=2, delay=1, iterations=2, seed=106, cls="well"),
    "G": dict(channels=64, n=12000, n_fft=64, hop=16, taps=1, delay=2, iterations=2, seed=107, cls="well"),
    "H": dict(channels=40, n=8000, n_fft=64, hop=16, taps=1, delay=1, iterations=2, seed=108, cls="well"),
    "L": dict(channels=64, n=12000, n_fft=64, hop=16, taps=1, delay=122, iterations=2, seed=111, cls="well"),
}


def signal(channels, n, seed):
    """[channels][n] float32."""
    rng = np.random.Generator(np.random.PCG64(seed))
    src = rng.standard_normal((channels + 1, n))
    L = int(0.3 * SR)
    env = np.exp(-np.log(1000.0) * np.arange(L) / L)
    out = np.empty((channels, n))
    for c in range(channels):
        rir = rng.standard_normal(L) * env
        rir[0] = 1.0
        dry = src[c] + 0.5 * src[c + 1]
        out[c] = np.convolve(dry, rir)[:n] / np.sqrt(np.sum(rir ** 2)) + 0.05 * rng.standard_normal(n)
    return (0.1 * out).astype(np.float32)


def case_signal(name):
    c = CASES[name]
    return signal(c["channels"], c["n"], c["seed"])
