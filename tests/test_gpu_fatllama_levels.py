"""Threshold LEVELS of the Fat-Llama loop: hard thresholds held to round-off, and levels that degenerate.

Part A.  Every other test in which the threshold removes something runs on noise, where a borderline bin may flip between two
float32 implementations, so a hard threshold is only held to 1e-6 of the output energy (an rms error of 1e-3) -- a wrong gating
decision confined to one structure (a self-paired row, the spare middle block of an odd cross radix, the ragged last column tile,
the second channel's slot of the carried maximum) touches about 1/R of the bins and passes.  Here the input's spectrum is exactly
two-level and on the bins (comb()): float64 proves on the host, before anything is launched, that in every iteration every nonzero
bin is a factor >= 3 away from the level, so every gating decision is forced and the hard threshold can be held per bin to a small
multiple of the float32 oracle's own error -- one wrongly kept or dropped bin is thousands of times that.

Part B.  The hooks with a level that is zero or whose square is subnormal: thr = 0, a channel that holds only a decayed tail (its
spectrum's squares are subnormal float32 numbers) next to a normal channel, an all-zero channel under the relative rule.  The soft
gain of wl_pair_hook<1> (csrc/egr_fatllama_wl.h) goes through v_rsq_f32, which flushes a subnormal input: the gain must still be
finite and right, and nothing may reach the ring of carried maxima that every later iteration's level is read from.

Oracle: oracle/fatllama.py with the matching FatLlamaSpec, float32 and float64 (exact=True)."""
import numpy as np
import pytest

from oracle import fatllama as ofl
from test_gpu_fatllama import run_gpu, synth
from test_gpu_fatllama_wl import rms, run, run_pz

pytestmark = pytest.mark.gpu

ITERS = 3
MIN_FACTOR = 3.0          # every nonzero bin at least this far from the level, on either side (measured on the host: 3.90 - 4.00)
MIN_REMOVED = 1e-4        # the first iteration removes more than this share of the energy (3.6e-3 - 6.5e-3)


def comb(n, seed, peak):
    """A real signal whose spectrum is a weak comb on every bin with strong tones on 1/256 of them: two levels, two decades apart."""
    rng = np.random.Generator(np.random.PCG64(seed))
    nb = (n - 1) // 2                               # bins 1 .. nb; DC and Nyquist stay empty
    ns = max(16, nb // 256)
    mag = 0.01 * rng.uniform(0.5, 1.0, nb)          # weak comb on every bin ...
    strong = rng.choice(nb, ns, replace=False)
    mag[strong] = rng.uniform(1.0, 2.0, ns)         # ... strong tones on 1/256 of them
    X = np.zeros(n // 2 + 1, np.complex128)
    X[1:nb + 1] = mag * np.exp(2j * np.pi * rng.uniform(0, 1, nb))
    x = np.fft.irfft(X, n)
    return (x / np.max(np.abs(x)) * peak).astype(np.float32)


def forced_decisions(x, thr, relative, iters):
    """The loop of SPEC.md section 3 (no pre-threshold, hard shrink) in float64 on one channel -> (the smallest factor between a
    nonzero bin and the level over all iterations, the share of the energy the first iteration removes)."""
    n = x.shape[0]
    d = x.astype(np.float64)
    worst, removed = np.inf, 0.0
    for it in range(iters):
        X = np.fft.rfft(d)
        mag = np.abs(X)
        t = thr * float(mag.max()) if relative else thr
        nz = mag[mag > 0]
        worst = min(worst, float(np.min(np.maximum(nz / t, t / nz))))
        keep = mag > t
        if it == 0:
            w = np.full(mag.shape, 2.0); w[0] = 1.0          # rfft holds one of each conjugate pair
            if n % 2 == 0:
                w[-1] = 1.0
            removed = float(np.sum(w * np.where(keep, 0.0, mag) ** 2) / np.sum(w * mag ** 2))
        d = np.fft.irfft(np.where(keep, X, 0.0), n)
    return worst, removed


def check_plan(n, split, want):
    """The planner's own plan where the table of PLANS names one (explicit splits are the caller's choice)."""
    from egregora_amd import fatllama_engine as fe
    if split is not None:
        assert 2 * split[0] * split[1] * split[2] == n
        return
    info = fe.plan_info(n, 1)
    assert info["supported"], info
    for k, v in want.items():
        assert info[k] == v, (n, k, info)


PLANS = [  # (n, explicit split, what plan_info must say, what the length reaches)
    (264600, None, {"M1": 441, "M2": 300, "levels": 2}, "k_col_wl<21,12>, k_row_wl<3,10>: odd cross radix, one self-paired row"),
    (480000, None, {"M1": 625, "M2": 384, "levels": 2}, "k_col_wl<25,8>, k_row_wl<6,8>"),
    (491520, (320, 768, 1), {}, "even row count: two self-paired rows on the LDS hook path"),
    (614400, (320, 960, 1), {}, "k_row_wl<15,8>: spare middle block"),
    (44100, (441, 50, 1), {}, "ragged last column tile, generic rows"),
    (30720, (16, 15, 64), {}, "three levels, k_colb_wl"),
    (48000, None, {"bluestein": False, "levels": 2}, "packed two-level generic plan"),
    (48624, None, {"bluestein": True, "chirpz_kind": 1}, "paired chirp-z, kind 1"),
    (4801, None, {"bluestein": True, "chirpz_kind": 2}, "paired chirp-z, kind 2: the channel pair in one state"),
]


@pytest.mark.parametrize("relative", [False, True], ids=["absolute", "relative"])
@pytest.mark.parametrize("n,split,want_plan,reaches", PLANS, ids=[str(p[0]) for p in PLANS])
def test_hard_threshold_with_forced_decisions_is_held_per_bin(pack, n, split, want_plan, reaches, relative):
    """Part A.  Two channels at different levels (a mix-up between the ring slots of the carried maximum shows), factor 1, 3
    iterations, zero insertion (y = x at factor 1; the linear rule zeroes the last sample and smears it over every bin) and no
    time-domain pre-threshold (it would destroy the two-level spectrum); absolute level 0.02 max |FFT(x)| of the louder channel or
    relative level 0.02.  Per channel, with d = out - y, G / O / D = FFT64 of d from the device / the float32 oracle / the float64 loop:
      1. max_k |G - D| <= 4 max_k |O - D|: the oracle's own error, measured here; 4 for the different factorisation (the header of
         egr_fatllama_wl.h records this project's kernels at 0.6x - 2.3x the oracle's error).  The bar must sit below a tenth of the
         weakest comb bin, so one bin kept or dropped wrongly cannot pass.
      2. max |out - oracle32| <= 2e-5 of the peak (the existing bar of the soft shrink, here for the hard threshold).
      3. the two kernel families (EGR_FL_WL = 1 / 0; the chirp-z lengths: EGR_PZ_COLWL = 1 / 0) agree to 4e-6 (max) and 4e-7 (rms) of the
         peak, the bars of test_two_barrier_kernels_agree_with_the_stage_by_stage_kernels."""
    check_plan(n, split, want_plan)
    chirpz = bool(want_plan.get("bluestein"))
    x = np.stack([comb(n, n, 8000.0), comb(n, n + 1, 2000.0)])
    x64 = x.astype(np.float64)
    spectrum = np.abs(np.fft.rfft(x64, axis=1))
    thr = 0.02 if relative else 0.02 * float(spectrum[0].max())
    variant = ("relative," if relative else "") + "zero_stuff,no_init_thr"
    spec = ofl.FatLlamaSpec(interp="zero_stuff", init_threshold="none", threshold_ref="relative_to_max" if relative else "absolute")
    # preconditions, in float64 on the host, before anything is launched: conditions, not measurements
    for c in range(2):
        factor, removed = forced_decisions(x[c], thr, relative, ITERS)
        print(f"\nn = {n} ch {c} {variant}: every nonzero bin >= {factor:.2f}x from the level, first iteration removes {removed:.2e} of the energy")
        assert factor >= MIN_FACTOR, (n, c, factor)
        assert removed > MIN_REMOVED, (n, c, removed)
    want = ofl.enhance_channels(x, 1, ITERS, thr, normalize=False, autoscale=False, spec=spec)
    exact = ofl.enhance_channels(x, 1, ITERS, thr, normalize=False, autoscale=False, spec=spec, exact=True)
    kw = {"variant": variant}
    if split is not None:
        kw["split"] = split
    if chirpz:
        got = {"1": run_pz(x, ITERS, True, thr, **kw), "0": run_pz(x, ITERS, False, thr, **kw)}
    else:
        got = {"1": run(x, ITERS, thr, True, **kw), "0": run(x, ITERS, thr, False, **kw)}
    fails = []
    for c in range(2):
        nb = (n - 1) // 2
        weakest = float(spectrum[c, 1:nb + 1].min())
        D = np.fft.rfft(exact[c] - x64[c])
        O = np.fft.rfft(want[c].astype(np.float64) - x64[c])
        err_o, top = float(np.max(np.abs(O - D))), float(np.max(np.abs(D)))
        bar = 4.0 * err_o
        assert 0.0 < bar < 0.1 * weakest, (n, c, bar, weakest)
        peak = float(np.max(np.abs(want[c])))
        for fam, out in got.items():
            assert out.shape == want.shape and np.isfinite(out).all()
            G = np.fft.rfft(out[c].astype(np.float64) - x64[c])
            err_g = float(np.max(np.abs(G - D)))
            tmax = float(np.max(np.abs(out[c] - want[c])))
            print(f"n = {n} ch {c} {variant} family {fam} ({reaches}): per bin device {err_g / top:.2e} / oracle32 {err_o / top:.2e} of max |D| = "
                  f"ratio {err_g / err_o:.2f} (bar 4; weakest comb bin {weakest / top:.2e}); time domain vs oracle32 {tmax / peak:.2e} of the peak")
            if not err_g <= bar:
                fails.append(("per bin", c, fam, err_g / err_o))
            if not tmax <= 2e-5 * peak:
                fails.append(("time domain", c, fam, tmax / peak))
        a, b = got["1"][c], got["0"][c]
        fmax, frms = float(np.max(np.abs(a - b))), rms(a - b)
        print(f"n = {n} ch {c} {variant}: families differ by max {fmax / peak:.2e}, rms {frms / peak:.2e} of the peak")
        if not (fmax <= 4e-6 * peak and frms <= 4e-7 * peak):
            fails.append(("families", c, fmax / peak, frms / peak))
    assert not fails, fails


def tail_next_to_a_normal_channel(n, seed, ch1):
    """Two channels of synth(); the second times ch1 (1e-24 / 1e-27: a decayed tail whose spectrum squares to subnormals; 0: silence)."""
    x = synth(2, n, seed, scale=8000.0, integer=False)
    x[1] *= np.float32(ch1)
    assert np.all(np.isfinite(x)) and (ch1 == 0.0 or float(np.max(np.abs(x[1]))) > 1e-30)
    return x


def spec_of(variant):
    return ofl.FatLlamaSpec(threshold_ref="relative_to_max" if "relative" in variant else "absolute",
                            threshold_kind="soft" if "soft" in variant else "hard")


DEGENERATE = [  # (case, n, variant, thr, iterations, factor on channel 1)
    ("B1", 264600, "soft", 0.0, 3, 1e-24),
    ("B1", 480000, "soft", 0.0, 3, 1e-24),
    ("B2", 264600, "relative,soft", 0.02, 3, 1e-27),
    ("B2", 480000, "relative,soft", 0.02, 3, 1e-27),
    ("B3", 264600, "relative", 0.02, 3, 1e-27),
    ("B4", 264600, "relative,soft", 0.02, 3, 0.0),
    ("B4", 264600, "relative", 0.02, 3, 0.0),
    ("B4", 48000, "relative,soft", 0.02, 3, 0.0),
    ("B4", 48000, "relative", 0.02, 3, 0.0),
    ("B4", 4801, "relative,soft", 0.02, 3, 0.0),
    ("B4", 4801, "relative", 0.02, 3, 0.0),
    ("B5", 264600, "", 0.0, 3, 1e-24),
    ("B6", 264600, "soft", 0.0, 27, 1e-24),       # past the 25 slots of the ring and the 25 iterations of the captured graph
]


@pytest.mark.parametrize("case,n,variant,thr,iters,ch1", DEGENERATE,
                         ids=[f"{c[0]}-{c[1]}-{c[2] or 'default'}" for c in DEGENERATE])
def test_degenerate_levels_stay_finite_and_stay_in_their_channel(pack, case, n, variant, thr, iters, ch1):
    """Part B.  Every output sample finite; channel 0 equals its own run on a one-channel input to the family bar (4e-6 of the
    peak: a poisoned ring or a shared slot shows) -- at n = 4801 the pair shares one complex state, so channel 0 is held to the
    float32 oracle (2e-5 of the peak) instead; a silent channel stays exactly zero where it has a state of its own; at thr = 0 the
    loop is an identity chain and the decayed channel is held to the float32 oracle at 2e-5 of ITS OWN peak; under the relative soft
    shrink (B2) it is held to the float64 loop at the variant bar (1e-6 of the output energy: derived for the device's subnormal
    squares, which keep as few as 17 significant bits near the level, not measured), and a shrink never amplifies."""
    from egregora_amd import fatllama_engine as fe
    info = fe.plan_info(n, 1)
    shared = info.get("chirpz_kind", 0) == 2
    assert shared == (n == 4801) and bool(info["bluestein"]) == (n == 4801), info
    x = tail_next_to_a_normal_channel(n, n + iters, ch1)
    spec = spec_of(variant)
    oracle = lambda sel, **kw: ofl.enhance_channels(x[sel], 1, iters, thr, normalize=False, autoscale=False, spec=spec, **kw)
    if shared:
        runs = {"-": lambda a: run_gpu(pack, a, 1, iters, thr, variant=variant)}
    else:
        runs = {"1": lambda a: run(a, iters, thr, True, variant=variant), "0": lambda a: run(a, iters, thr, False, variant=variant)}
    want0 = oracle(slice(0, 1))[0] if shared else None
    want1 = oracle(slice(1, 2))[0] if case in ("B1", "B5", "B6") else None
    exact1 = oracle(slice(1, 2), exact=True)[0] if case == "B2" else None
    fails = []
    for fam, go in runs.items():
        got = go(x)
        bad = int(np.count_nonzero(~np.isfinite(got)))
        print(f"\n{case} n = {n} {variant or 'default'} thr {thr} x{ch1:g} family {fam}: {bad} of {got.size} samples not finite "
              f"(channel 0: {int(np.count_nonzero(~np.isfinite(got[0])))}, channel 1: {int(np.count_nonzero(~np.isfinite(got[1])))})")
        if bad:
            fails.append(("not finite", fam, bad))
            continue
        if shared:
            e0, p0 = float(np.max(np.abs(got[0] - want0))), float(np.max(np.abs(want0)))
            print(f"   channel 0 vs the float32 oracle: {e0 / p0:.2e} of the peak")
            if not e0 <= 2e-5 * p0:
                fails.append(("channel 0 vs oracle", fam, e0 / p0))
        else:
            solo = go(x[:1].copy())
            e0, p0 = float(np.max(np.abs(got[0] - solo[0]))), float(np.max(np.abs(solo[0])))
            print(f"   channel 0 vs its one-channel run: {e0 / p0:.2e} of the peak")
            if not (np.isfinite(solo).all() and e0 <= 4e-6 * p0):
                fails.append(("channel 0 vs alone", fam, e0 / p0))
        if case == "B4" and not shared and np.any(got[1] != 0.0):
            fails.append(("silent channel not zero", fam, float(np.max(np.abs(got[1])))))
        if want1 is not None:
            e1, p1 = float(np.max(np.abs(got[1].astype(np.float64) - want1))), float(np.max(np.abs(want1)))
            print(f"   channel 1 vs the float32 oracle: {e1 / p1:.2e} of its own peak {p1:.2e}")
            if not e1 <= 2e-5 * p1:
                fails.append(("channel 1 vs oracle", fam, e1 / p1))
        if exact1 is not None:
            y = ofl.interpolate(x[1], 1, spec).astype(np.float64)
            g1 = got[1].astype(np.float64)
            num, den = float(np.sum((g1 - exact1) ** 2)), float(np.sum(exact1 ** 2))
            amp = float(np.sum((g1 - y) ** 2)) / float(np.sum(y ** 2))
            print(f"   channel 1 vs the float64 loop: energy-relative {num / den:.2e}; energy of out - y over energy of y {amp:.6f}")
            if not num <= 1e-6 * den:
                fails.append(("channel 1 vs float64", fam, num / den))
            if not amp <= 1.0 + 1e-3:
                fails.append(("the shrink amplified", fam, amp))
    assert not fails, fails
