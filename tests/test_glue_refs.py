"""The host references of tests/glue_refs.py against slower, plainer statements of the same definitions (no device needed): a wrong
reference would make tests/test_gpu_glue_laps.py pass or fail for the wrong reason."""
import numpy as np
import pytest

import glue_refs as R

RATES = [(3, 1), (160, 147), (147, 160), (4, 1)]


def _design(up, down):
    """The float32 Kaiser(5) taps of resample.design_filter, restated (numpy only)."""
    mx = max(up, down)
    half = 10 * mx
    m = np.arange(2 * half + 1, dtype=np.float64) - half
    h = np.sinc(m / mx) / mx * np.kaiser(2 * half + 1, 5.0)
    return (h / h.sum()).astype(np.float32) * np.float32(up), half


@pytest.mark.parametrize("up,down", RATES)
def test_poly64_is_the_polyphase_definition(up, down):
    h, half = _design(up, down)
    rng = np.random.Generator(np.random.PCG64(up))
    for n in (1, 2, 50, 333):
        x = rng.standard_normal(n).astype(np.float32)
        y, S = R.poly64(x, h, up, down, half)
        want = R.poly_direct(x, h, up, down, half)
        assert y.shape == want.shape == (R.n_out_of(n, up, down),)
        assert np.abs(y - want).max() <= 1e-13 and np.abs(S - R.poly_direct(np.abs(x), np.abs(h), up, down, half)).max() <= 1e-13
        assert (np.abs(y) <= S + 1e-15).all()
    assert R.poly_terms(up, half) == max(len(range(r, 2 * half + 1, up)) for r in range(up))


@pytest.mark.parametrize("up,down", RATES[:3])
def test_poly_track_plan_puts_the_boundaries_where_it_says(up, down):
    lap = 4096 * 256
    clips, marks = R.poly_track_plan(up, down, lap)
    starts, pos = [], 0
    for c, n in clips:
        for _ in range(c):
            starts.append(pos)
            pos += R.n_out_of(n, up, down)
    assert R.n_out_of(clips[0][1], up, down) >= lap + 100 and all(s > lap for s in starts[1:]) and pos >= R.lap_n(lap) and pos % 256 != 0
    assert marks["at256"] in starts[1:] and marks["at256"] % 256 == 0 and marks["atlap"] in starts[1:] and marks["atlap"] % lap == 0
    assert {1, 2, 3} == {c for c, _ in clips}
    for m in (1, 255, 256, 257):
        n = R.n_in_for(m, up, down)
        assert R.n_out_of(n, up, down) >= m and (n == 1 or R.n_out_of(n - 1, up, down) < m)


def test_shift_fir32_indexes_like_numpy_convolve_same():
    rng = np.random.Generator(np.random.PCG64(7))
    x = rng.standard_normal((2, 3000)).astype(np.float32)
    h = rng.standard_normal(33).astype(np.float32)
    for shift, taps, n_out in ((5, 33, 3000), (-7, 16, 2500), (0, 0, 3500), (3000, 33, 3000), (-3005, 33, 3000), (17, 32, 4000)):
        hh = h[:taps] if taps else None
        a, b = R.shift_fir32(x, shift, hh, n_out), R.shift_fir64(x, shift, hh, n_out)
        bound = max(1, taps) * R.U24 * (float(np.abs(h[:taps]).sum()) if taps else 1.0) * float(np.abs(x).max())
        assert a.dtype == np.float32 and a.shape == b.shape == (2, n_out) and np.abs(a - b).max() <= bound, (shift, taps, n_out)
        if abs(shift) >= 3000:
            assert not a.any()
        if taps == 0 and shift >= 0:
            assert np.array_equal(a[:, shift:3000], x[:, :3000 - shift]) and not a[:, :shift].any() and not a[:, 3000:].any()


def test_where_bad_counts_the_first_lap():
    bad = np.zeros(1000, bool)
    bad[[3, 600, 999]] = True
    assert R.where_bad(bad, 500, "x") == "x: 3 bad of 1000, first 3, last 999, 1 inside the first lap of 500"
    assert R.bits_differ(np.float32([0.0, 1.0]), np.float32([-0.0, 1.0])).tolist() == [True, False]
