"""Values of the glue and metric kernels of csrc/egr_glue.hip PAST THE FIRST GRID LAP.

Almost every kernel there is a grid-stride loop under a launcher that stops the grid at 4096, 2048 or 1024 workgroups of 256 threads,
so every real clip (one lap is 22 s at 48 kHz, 5.5 s for the sums) runs them in their second and later laps.  LAPS below names, per
entry point, the lap this module was written against and the launcher line it comes from; every lap case runs 2 lap + 3 * 256 + 37
elements (two full laps and a ragged third; a cap that doubles one day is still crossed), or the nearest size the entry point's shape
rules allow.  Where the answer is a maximum or a count, the deciding samples lie past the first lap only.

References are numpy / scipy on the host (tests/glue_refs.py, oracle/): float32 in the kernel's stated order where the kernel promises
an order (bit-exact), float64 with a rounding bound of the stated arithmetic elsewhere.  Never another device kernel.

Also here, from the same file: egr_dfn_vad_gains with three channels, egr_si_sdr_terms / egr_pair_stats with operands of different
channel counts and strides, egr_order_stats2 around its 1024-thread width and on the special keys.
"""
import numpy as np
import pytest
import torch

import glue_refs as R
from conftest import ROOT
from glue_refs import F32, U24, lap_n, where_bad
from oracle import dfn_mix as odm
from oracle import fatllama as ofl
from oracle import glue as og
from oracle import metrics as om

pytestmark = pytest.mark.gpu

LAP, LAP_MIX, LAP_SUM = 4096 * 256, 2048 * 256, 1024 * 256
# entry point -> (elements one lap covers, the launcher text in csrc/egr_glue.hip that says so)
LAPS = {
    "egr_pcm16_roundtrip": (LAP, "b > 4096 ? 4096 : b"),                                   # grid_for(n)
    "egr_mono_mean": (LAP, "k_mono_mean, dim3(grid_for(n))"),
    "egr_chunk_gather_tracks": (LAP, "dim3(grid_for((long long)n_rows * win))"),           # rows x win
    "egr_wola_stitch": (LAP, "dim3(grid_for(total), channels)"),                           # per channel
    "egr_wola_tracks": (LAP, "k_wola_tracks, dim3(grid_for(total_out))"),
    "egr_resample_poly": (LAP, "dim3(grid_for(n_out), channels)"),                         # outputs, per channel
    "egr_resample_poly_tracks": (LAP, "k_resample_poly_tracks, dim3(grid_for(total_out))"),
    "egr_shift_fir": (LAP, "long long nb = (n_out + 255) / 256;\n    if (nb > 4096) nb = 4096;\n    hipLaunchKernelGGL(k_shift_fir"),
    "egr_resample_linear": (LAP, "long long nb = (n_out + 255) / 256;\n    if (nb > 4096) nb = 4096;\n    hipLaunchKernelGGL(k_resample_linear"),
    "egr_true_peak": (LAP, "long long nb = ((long long)n * up + 255) / 256;\n    if (nb > 4096) nb = 4096;"),
    "egr_dfn_mix": (LAP_MIX, "if (nb > 2048) nb = 2048;\n    hipLaunchKernelGGL(k_dfn_mix"),                 # per channel
    "egr_dfn_mix/limit": (LAP, "if (nb2 > 4096) nb2 = 4096;\n    hipLaunchKernelGGL(k_dfn_limit"),            # over n * channels
    "egr_sum_f64": (LAP_SUM, "if (nb > 1024) nb = 1024;\n    hipLaunchKernelGGL(k_sum_f64"),
    "egr_si_sdr_terms": (LAP_SUM, "if (nb > 1024) nb = 1024;\n    for (int mode = 0; mode < 2; ++mode)\n        hipLaunchKernelGGL(k_sisdr"),
    "egr_pair_stats": (LAP_SUM, "k_pair_stats, dim3(grid_for(n) > 1024 ? 1024 : grid_for(n))"),
    "egr_null_mix": (LAP_SUM, "k_null_mix, dim3(grid_for(n) > 1024 ? 1024 : grid_for(n))"),
    "egr_band_sums": (LAP_SUM, "k_band_sums, dim3(grid_for(n) > 1024 ? 1024 : grid_for(n))"),
}
N = lap_n(LAP)                      # 2 097 957
N_MIX = lap_n(LAP_MIX)              # 1 049 381
N_SUM = 4 * LAP_SUM + 3 * 256 + 37  # 1 049 381: four laps of the sum kernels and a ragged fifth
WIN, HOP = 3840, 3840 - 375         # the small chunking of tests/test_gpu_flashsr_batch.py


def rng_for(seed):
    return np.random.Generator(np.random.PCG64(seed))


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def test_lap_table_still_describes_the_launchers():
    """Every launcher text quoted in LAPS is still in the source: a launcher that changes its cap fails here and sends its reader to
    the table (and to the sizes below, which cross a cap that doubles but not one that grows further)."""
    src = (ROOT / "comfyui-egregora-audio-super-resolution_amd" / "csrc" / "egr_glue.hip").read_text(encoding="utf-8")
    missing = [name for name, (_, text) in LAPS.items() if text not in src]
    assert not missing, missing
    assert "threadIdx.x; i < n; i += (long long)gridDim.x * 256" in src          # 256 threads a workgroup
    assert N == 2 * LAP + 805 and N_MIX == 2 * LAP_MIX + 805 and N_SUM >= 4 * LAP_SUM and N_SUM % 256 != 0 and N % 256 != 0


# ================================================================ 1. elementwise and gather kernels, bit-exact
def test_pcm16_roundtrip_past_the_lap(pack):
    from egregora_amd import device_ops as ops
    lap = LAPS["egr_pcm16_roundtrip"][0]
    x = rng_for(1).uniform(-1.6, 1.6, lap_n(lap)).astype(F32)
    got = host(ops.pcm16_roundtrip(cu(x)))
    bad = R.bits_differ(got, ofl.pcm16_read(ofl.pcm16_write(x)))
    assert not bad.any(), where_bad(bad, lap, "pcm16 round trip")
    got = host(ops.pcm16_roundtrip(cu(x), 32767.0, 1.0))
    bad = R.bits_differ(got, ofl.pcm16_write(x).astype(F32))
    assert not bad.any(), where_bad(bad, lap, "pcm16 integers")


@pytest.mark.parametrize("C", [1, 2, 3])
def test_mono_mean_past_the_lap_with_a_row_stride(pack, C):
    from egregora_amd import device_ops as ops
    lap = LAPS["egr_mono_mean"][0]
    n = lap_n(lap)
    x = rng_for(10 + C).standard_normal((C, n + 131)).astype(F32)              # stride n + 131 > n
    got = host(ops.mono_mean(cu(x), n))
    bad = R.bits_differ(got, R.mono_mean32(x, n))
    assert got.shape == (n,) and not bad.any(), where_bad(bad, lap, f"mono mean C={C}")


def _layout(shapes):
    offs, pos = [], 0
    for Cn, T in shapes:
        offs.append(pos)
        pos += Cn * T
    return offs, pos


def test_chunk_gather_tracks_past_the_lap(pack):
    from egregora_amd import device_ops as ops, flashsr_engine as E
    lap = LAPS["egr_chunk_gather_tracks"][0]
    shapes = [(2, 520000), (3, 200001), (1, 3841), (1, 1), (2, 123457)]       # 300 + 174 + 2 + 1 + 72 rows
    offs, total = _layout(shapes)
    t = E.wave_tables(shapes, offs, WIN, HOP)
    assert t["n_rows"] * WIN >= lap_n(lap)                                      # rows x win: whole rows only, 2 108 160 here
    flat = rng_for(20).standard_normal(total).astype(F32)
    got = host(ops.chunk_gather_tracks(cu(flat), cu(t["rows"]), WIN, HOP))
    want = R.gather_rows(flat, t["rows"], WIN, HOP)
    bad = R.bits_differ(got, want)
    assert got.shape == want.shape and not bad.any(), where_bad(bad, lap, "chunk_gather_tracks")


@pytest.mark.parametrize("lp", [WIN, WIN - 7])
def test_wola_stitch_past_the_lap(pack, lp):
    from egregora_amd import device_ops as ops
    lap = LAPS["egr_wola_stitch"][0]
    total = lap_n(lap)
    spans = og.chunk_spans(total, WIN, HOP)
    preds = rng_for(30 + lp).standard_normal((len(spans), 2, lp)).astype(F32)
    got = host(ops.wola_stitch(cu(preds), total, WIN, HOP))
    want = og.wola([(preds[k], s, L) for k, (s, L) in enumerate(spans)], total, WIN)
    bad = got != want
    assert got.shape == (2, total) and not bad.any(), where_bad(bad[0] | bad[1], lap, f"wola_stitch lp={lp} (index inside a channel)")


def _shift_fir(x, shift, h, n_out):
    from egregora_amd import native
    C, n_in = x.shape
    xt = cu(x)
    ht = cu(h) if h is not None else None
    y = torch.empty((C, n_out), dtype=torch.float32, device="cuda")
    native.check(native.lib().egr_shift_fir(native.ptr(xt), C, n_in, int(shift), native.ptr(ht) if ht is not None else None,
                                            0 if h is None else len(h), native.ptr(y), n_out, native.stream_ptr()), "egr_shift_fir")
    return host(y)


@pytest.mark.parametrize("name,C,n_in,shift,taps,n_out", [
    ("longer_even_taps_delay", 1, N - 1000, 37, 64, N),
    ("shorter_odd_taps_advance", 2, N + 500, -1234, 33, N),
    ("no_taps", 1, N, 5, 0, N),
    ("delay_of_the_whole_input", 1, N, N, 16, N),
    ("advance_past_the_whole_input", 1, N - 3, -(N + 2), 33, N),
])
def test_shift_fir_past_the_lap(pack, name, C, n_in, shift, taps, n_out):
    """Tolerance: the 2e-6 of test_align_node.py::test_shift_fir_kernel_vs_numpy, on the same kind of input (standard normal samples,
    unit-gain Hann-windowed sinc taps)."""
    from egregora_amd import egregora_null_test_suite as nt
    lap = LAPS["egr_shift_fir"][0]
    assert n_out >= lap_n(lap)
    x = rng_for(40 + taps).standard_normal((C, n_in)).astype(F32)
    h = nt.frac_delay_taps(0.37, taps).astype(F32) if taps else None
    assert h is None or len(h) == taps
    want = R.shift_fir32(x, shift, h, n_out)
    if h is not None:       # the float32 restatement indexes like np.convolve(..., "same"): apart by float32 round-off of the taps-term sum only
        assert np.abs(want - R.shift_fir64(x, shift, h, n_out)).max() <= taps * U24 * float(np.abs(h).sum()) * float(np.abs(x).max())
    if abs(shift) >= n_in:
        assert not want.any()
    got = _shift_fir(x, shift, h, n_out)
    bad = np.abs(got - want) > 2e-6
    print(f"shift_fir {name}: max |diff| {float(np.abs(got - want).max()):.3e}")
    assert not bad.any(), where_bad(bad.any(axis=0), lap, f"shift_fir {name} (index inside a row)")
    assert not got[:, n_in:].any()


@pytest.fixture(scope="module")
def mix_inputs():
    """Two channels over two laps of k_dfn_mix and a ragged third; 2000 frames of 480 cover 960 000 samples, so the last gain pair repeats
    over the rest.  Everything stays below 0.5 except ONE sample of channel 1 in lap two, which mixes to about 0.99."""
    lap = LAPS["egr_dfn_mix"][0]
    T, hop, nfr = lap_n(lap), 480, 2000
    assert hop * nfr < T and 2 * T >= lap_n(LAPS["egr_dfn_mix/limit"][0])
    r = rng_for(50)
    dry = r.uniform(-0.25, 0.25, (2, T)).astype(F32)
    wet = r.uniform(-0.25, 0.25, (2, T)).astype(F32)
    gd = r.uniform(0.0, 1.0, (2, nfr)).astype(F32)
    gw = r.uniform(0.0, 1.0, (2, nfr)).astype(F32)
    p = lap + 300001
    f = p // hop
    assert lap < p < 2 * lap and f < nfr
    gd[1, f], gw[1, f], dry[1, p], wet[1, p] = 0.6, 0.5, 0.9, 0.9
    return dict(dry=dry, wet=wet, gd=gd, gw=gw, hop=hop, nfr=nfr, p=p, T=T, dev=[cu(a) for a in (dry, wet, gd, gw)])


@pytest.mark.parametrize("name,gain_db,limit,ceiling", [("peak_above_ceiling", 0.0, 1, 0.98), ("peak_below_ceiling", 0.0, 1, 0.995),
                                                         ("limiter_off", 0.0, 0, 0.98), ("post_gain_peak_above", 0.5, 1, 0.98)])
def test_dfn_mix_and_limit_past_the_lap(pack, mix_inputs, name, gain_db, limit, ceiling):
    """k_dfn_mix and k_dfn_limit use __f*_rn operations only: bit-equal to unfused numpy float32."""
    from egregora_amd import native
    m = mix_inputs
    lap = LAPS["egr_dfn_mix"][0]
    gain = float(10.0 ** (gain_db / 20.0)) if gain_db else None
    want, peak = R.dfn_mix32(m["dry"], m["wet"], m["gd"], m["gw"], m["hop"], gain, limit, ceiling)
    # the one sample that decides whether the limiter acts lies in lap two
    pre, _ = R.dfn_mix32(m["dry"], m["wet"], m["gd"], m["gw"], m["hop"], gain, 0, ceiling)
    assert np.argmax(np.abs(pre[1])) == m["p"] and float(np.abs(pre[0]).max()) < 0.6 and float(np.abs(np.delete(pre[1], m["p"])).max()) < 0.6
    assert (peak > ceiling) == (name in ("peak_above_ceiling", "limiter_off", "post_gain_peak_above"))
    assert (float(np.abs(want).max()) < peak) == (name in ("peak_above_ceiling", "post_gain_peak_above"))
    dry, wet, gd, gw = m["dev"]
    y = torch.empty_like(dry)
    pk = torch.zeros(1, dtype=torch.int32, device="cuda")
    native.check(native.lib().egr_dfn_mix(native.ptr(dry), native.ptr(wet), native.ptr(gd), native.ptr(gw), 2, m["T"], m["nfr"], m["hop"],
                                          gain if gain is not None else 1.0, int(gain is not None), limit, ceiling, native.ptr(y),
                                          native.ptr(pk), native.stream_ptr()), "egr_dfn_mix")
    got = host(y)
    assert float(host(pk.view(torch.float32))[0]) == peak, (name, float(host(pk.view(torch.float32))[0]), peak)
    bad = R.bits_differ(got, want)
    assert not bad.any(), where_bad(bad[0] | bad[1], lap, f"dfn_mix {name} (index inside a channel)")


# ================================================================ 2. many-track kernels with track boundaries past the first lap
def _wola_track_clips(lap):
    """(C, T) clips, outputs back to back: a first track of lap + 100 samples; a start exactly on a multiple of 256; tracks of 255, 256,
    1, 257 and 5000 samples in clips of 1 to 3 channels, all in lap two; a start exactly on 2 lap; more short tracks in lap three."""
    clips = [(1, lap + 100), (1, 156), (2, 255), (3, 256), (1, 1), (2, 257), (3, 5000)]
    pos = sum(c * t for c, t in clips)
    clips += [(1, 2 * lap - pos), (2, 4001), (1, 1), (3, 255)]
    return clips


@pytest.mark.parametrize("lp", [WIN, WIN - 7])
def test_wola_tracks_with_boundaries_past_the_lap(pack, lp):
    from egregora_amd import device_ops as ops, flashsr_engine as E
    lap = LAPS["egr_wola_tracks"][0]
    shapes = _wola_track_clips(lap)
    offs, _ = _layout(shapes)
    t = E.wave_tables(shapes, offs, WIN, HOP)
    starts = t["tracks"][:, 4].tolist()
    assert t["total_out"] >= lap_n(lap) and t["total_out"] % 256 != 0
    assert starts[1] == lap + 100 and lap + 256 in starts and 2 * lap in starts and all(s > lap for s in starts[1:])
    preds = rng_for(60 + lp).standard_normal((t["n_rows"], lp)).astype(F32)
    got = host(ops.wola_tracks(cu(preds), cu(t["tracks"]), t["total_out"], WIN, HOP))
    want = np.empty(t["total_out"], F32)
    r = 0
    for (Cn, T), (off, _, _) in zip(shapes, t["clip_out"]):
        spans = og.chunk_spans(T, WIN, HOP)
        p = preds[r:r + len(spans) * Cn].reshape(len(spans), Cn, lp)            # chunk-major, then channel
        want[off:off + Cn * T] = og.wola([(p[k], s, L) for k, (s, L) in enumerate(spans)], T, WIN).reshape(-1)
        r += len(spans) * Cn
    assert r == t["n_rows"]
    bad = got != want
    assert got.shape == want.shape and not bad.any(), where_bad(bad, lap, f"wola_tracks lp={lp}")


RATES = [(3, 1), (160, 147), (147, 160)]


def _check_poly(got, x, h32, up, down, half):
    """-> mask of outputs outside T 2^-24 S[m] of the float64 evaluation (T = floor(2 half / up) + 1 float32 terms per output: each
    product and each addition rounds once, to first order T half-ulps of the sum of magnitudes)."""
    want, S = R.poly64(x, h32, up, down, half)
    return np.abs(got.astype(np.float64) - want) > R.poly_terms(up, half) * U24 * S, float(np.abs(got - want).max())


@pytest.mark.parametrize("up,down", RATES)
def test_resample_poly_tracks_with_boundaries_past_the_lap(pack, up, down):
    from egregora_amd import device_ops as ops, flashsr_engine as E, resample
    lap = LAPS["egr_resample_poly_tracks"][0]
    clips, marks = R.poly_track_plan(up, down, lap)
    r = rng_for(70 + up)
    xs = [(0.3 * r.standard_normal((c, n))).astype(F32) for c, n in clips]
    flat = np.concatenate([x.reshape(-1) for x in xs] + [np.zeros(3, F32)])
    ins, n_ins, pos = [], [], 0
    for x in xs:
        for c in range(x.shape[0]):
            ins.append(pos + c * x.shape[1])
            n_ins.append(x.shape[1])
        pos += x.size
    tab, total = resample.poly_track_table(ins, n_ins, up, down)
    starts = tab[:, 2].tolist()
    assert total >= lap_n(lap) and tab[0, 3] >= lap + 100 and all(s > lap for s in starts[1:])
    assert marks["at256"] in starts[1:] and marks["at256"] % 256 == 0 and marks["atlap"] in starts[1:] and marks["atlap"] % lap == 0
    h, half = resample.filter_for(up, down, torch.device("cuda", torch.cuda.current_device()))
    y = torch.full((total + 5,), 7.0, device="cuda")
    ops.resample_poly_tracks(cu(flat), cu(tab), total, up, down, h, half, y)
    got = host(y)
    assert (got[total:] == 7.0).all()                                           # nothing behind total_out is written
    h32 = host(h)
    bad = np.zeros(total, bool)
    worst = 0.0
    for (i0, n_in, o0, n_out) in tab.tolist():
        b, w = _check_poly(got[o0:o0 + n_out], flat[i0:i0 + n_in], h32, up, down, half)
        bad[o0:o0 + n_out] = b
        worst = max(worst, w)
    print(f"resample_poly_tracks {up}/{down}: max |diff| {worst:.3e} over {total} outputs of {len(starts)} tracks")
    assert not bad.any(), where_bad(bad, lap, f"resample_poly_tracks {up}/{down}")


@pytest.mark.parametrize("up,down", RATES)
def test_resample_poly_single_clip_past_the_lap(pack, up, down):
    from egregora_amd import resample
    lap = LAPS["egr_resample_poly"][0]
    C = 2 if up == 3 else 1
    n_in = R.n_in_for(lap_n(lap), up, down)
    x = (0.3 * rng_for(80 + up).standard_normal((C, n_in))).astype(F32)
    src, dst = {(3, 1): (16000, 48000), (160, 147): (44100, 48000), (147, 160): (48000, 44100)}[(up, down)]
    assert resample.rates(src, dst) == (up, down)
    got = host(resample.resample_hq(cu(x), src, dst))
    assert got.shape == (C, R.n_out_of(n_in, up, down)) and got.shape[1] >= lap_n(lap)
    h, half = resample.design_filter(up, down)
    for c in range(C):
        bad, worst = _check_poly(got[c], x[c], h, up, down, half)
        print(f"resample_poly {up}/{down} channel {c}: max |diff| {worst:.3e}")
        assert not bad.any(), where_bad(bad, lap, f"resample_poly {up}/{down} channel {c}")


# ================================================================ 3. double-precision sums over four laps and more
def _close_sums(got, terms, what):
    """Each sum against numpy float64 over the same terms: |got - want| <= n 2^-52 sum |term|, the worst case of any summation order in
    double (numpy's own pairwise sum of these terms sits far inside it)."""
    for i, (g, t) in enumerate(zip(got, terms)):
        want, bound = float(np.sum(t, dtype=np.float64)), R.sum_bound(t)
        print(f"{what}[{i}]: got {g!r} want {want!r} diff {abs(g - want):.3e} bound {bound:.3e}")
        assert abs(g - want) <= bound, (what, i, g, want, abs(g - want), bound)


def test_sum_f64_over_four_laps(pack):
    from egregora_amd import native
    assert N_SUM >= 4 * LAPS["egr_sum_f64"][0]
    v = (rng_for(90).standard_normal(N_SUM) + 0.1).astype(F32)
    out = torch.empty(1, dtype=torch.float64, device="cuda")
    vt = cu(v)
    native.check(native.lib().egr_sum_f64(native.ptr(vt), N_SUM, native.ptr(out), native.stream_ptr()), "egr_sum_f64")
    _close_sums([float(out.cpu())], [v.astype(np.float64)], "sum_f64")


# operands of different channel counts and strides: (channels a, channels b, stride a - n, stride b - n)
OPERANDS = [("2ch_2ch", 2, 2, 0, 0), ("1ch_2ch", 1, 2, 7, 64), ("3ch_1ch", 3, 1, 301, 1)]


def _operands(seed, ca, cb, pa, pb, n):
    """A pair at roughly 15 to 20 dB: both are a common signal plus independent parts per channel."""
    r = rng_for(seed)
    m = 0.3 * r.standard_normal(n + max(pa, pb))
    a = np.stack([m[:n + pa] + 0.02 * r.standard_normal(n + pa) for _ in range(ca)]).astype(F32)
    b = np.stack([0.9 * m[:n + pb] + 0.03 * r.standard_normal(n + pb) for _ in range(cb)]).astype(F32)
    return a, b


@pytest.mark.parametrize("k", [None, 0.73])
@pytest.mark.parametrize("name,ca,cb,pa,pb", OPERANDS, ids=[o[0] for o in OPERANDS])
def test_pair_stats_over_four_laps(pack, name, ca, cb, pa, pb, k):
    from egregora_amd import device_ops as ops
    n = N_SUM
    assert n >= 4 * LAPS["egr_pair_stats"][0]
    a, b = _operands(100 + ca, ca, cb, pa, pb, n)
    got = ops.pair_stats(cu(a), cu(b), n, k)
    _close_sums(got, R.pair_terms(a, b, n, k), f"pair_stats {name} k={k}")


@pytest.mark.parametrize("name,cs,csh,ps,psh", OPERANDS, ids=[o[0] for o in OPERANDS])
def test_si_sdr_terms_over_four_laps(pack, name, cs, csh, ps, psh):
    from egregora_amd import native
    n = N_SUM
    assert n >= 4 * LAPS["egr_si_sdr_terms"][0]
    s, sh = _operands(110 + cs, cs, csh, ps, psh, n)
    st, sht = cu(s), cu(sh)
    out = torch.empty(4, dtype=torch.float64, device="cuda")
    native.check(native.lib().egr_si_sdr_terms(native.ptr(st), cs, s.shape[1], native.ptr(sht), csh, sh.shape[1], n, native.ptr(out),
                                                native.stream_ptr()), "egr_si_sdr_terms")
    got = [float(v) for v in out.cpu()]
    x, y = R.mono_mean32(s, n).astype(np.float64), R.mono_mean32(sh, n).astype(np.float64)
    alpha = got[0] / (got[1] + 1e-20)                   # the second pass reads the first pass's sums
    t = alpha * x
    e = y - t
    _close_sums(got, [y * x, x * x, t * t, e * e], f"si_sdr_terms {name}")
    want_db = om.si_sdr(s[:, :n], sh[:, :n])
    got_db = float(10.0 * np.log10((got[2] + 1e-20) / (got[3] + 1e-20)))
    print(f"si_sdr {name}: got {got_db!r} dB want {want_db!r} dB")
    assert 10.0 < want_db < 30.0 and abs(got_db - want_db) <= 1e-6, (name, got_db, want_db)


@pytest.mark.parametrize("k,invert", [(0.8, True), (None, False)])
def test_null_mix_counts_only_past_the_lap(pack, k, invert):
    from egregora_amd import device_ops as ops
    lap = LAPS["egr_null_mix"][0]
    n = N_SUM
    r = rng_for(120)
    a = r.uniform(-0.4, 0.4, (2, n + 5)).astype(F32)
    b = r.uniform(-0.4, 0.4, (2, n + 33)).astype(F32)
    sgn = -1.0 if invert else 1.0
    idx = lap + 1000 + 5003 * np.arange(37)            # the 37 samples with |null| > 1: lap two only
    assert idx.min() > lap and idx.max() < 2 * lap
    a[np.arange(37) % 2, idx] = 0.9
    b[np.arange(37) % 2, idx] = 0.9 * sgn
    a[0, 2 * lap + 11], b[0, 2 * lap + 11] = 1.0, 0.0   # |null| == 1 exactly is not an over
    bk = b[:, :n] if k is None else b[:, :n] * F32(k)
    want = a[:, :n] + F32(sgn) * bk
    assert want.dtype == F32 and int((np.abs(want) > 1).sum()) == 37 and want[0, 2 * lap + 11] == 1.0
    nul, s, overs = ops.null_mix(cu(a), cu(b), n, k, invert)
    assert overs == 37
    bad = R.bits_differ(host(nul), want)
    assert not bad.any(), where_bad(bad[0] | bad[1], lap, "null (index inside a channel)")
    m = R.mono_mean32(want).astype(np.float64)
    _close_sums([s], [m * m], "null_mix sum of squares")


def test_band_sums_over_four_laps(pack):
    from egregora_amd import native
    n = N_SUM
    assert n >= 4 * LAPS["egr_band_sums"][0]
    r = rng_for(130)
    x, y = (r.standard_normal(n) + 0.05).astype(F32), (0.5 * r.standard_normal(n) - 0.02).astype(F32)
    xt, yt = cu(x), cu(y)
    out = torch.empty(6, dtype=torch.float64, device="cuda")
    native.check(native.lib().egr_band_sums(native.ptr(xt), native.ptr(yt), n, native.ptr(out), native.stream_ptr()), "egr_band_sums")
    sg = np.where(np.arange(n) % 2 == 1, -1.0, 1.0)
    xd, yd = x.astype(np.float64), y.astype(np.float64)
    _close_sums([float(v) for v in out.cpu()], [xd * xd, xd, sg * xd, yd * yd, yd, sg * yd], "band_sums")


# ================================================================ 4. linear resampling
@pytest.mark.parametrize("C,n_in,n_out", [(1, N, 1398638), (1, 700000, N), (2, 49, 343), (2, 1, 5), (3, 3, 1000)])
def test_resample_linear_vs_interp(pack, C, n_in, n_out):
    """np.interp over the two endpoint-free grids in float64; bound: one float32 ulp of the largest input, 2^-23 max |x| (the kernel
    interpolates in double and rounds once, the grids themselves differ by double round-off)."""
    from egregora_amd import device_ops as ops
    lap = LAPS["egr_resample_linear"][0]
    x = rng_for(140 + n_in % 97).standard_normal((C, n_in)).astype(F32)
    got = host(ops.resample_linear(cu(x), n_out))
    want = R.linear64(x, n_out)
    bound = 2.0 ** -23 * float(np.abs(x).max())
    bad = np.abs(got - want) > bound
    print(f"resample_linear {n_in} -> {n_out}: max |diff| {float(np.abs(got - want).max()):.3e} bound {bound:.3e}")
    assert got.shape == want.shape and not bad.any(), where_bad(bad.any(axis=0), lap, f"resample_linear {n_in} -> {n_out} (index inside a row)")


# ================================================================ 5. true peak
def _true_peak(x, up):
    from egregora_amd import loudness, native
    xt = cu(x)
    slot = torch.empty(1, dtype=torch.float32, device="cuda")
    h, half = (None, 0) if up == 1 else loudness._taps(up, xt.device)
    native.check(native.lib().egr_true_peak(native.ptr(xt), x.shape[0], x.shape[1], up, native.ptr(h) if h is not None else None, half,
                                            native.ptr(slot), native.stream_ptr()), "egr_true_peak")
    return float(slot.cpu()[0])


def test_true_peak_oversampled_with_the_peak_past_the_lap(pack):
    from egregora_amd import resample
    lap = LAPS["egr_true_peak"][0]
    up = 4
    n = (lap_n(lap) + up - 1) // up
    x = (0.1 * rng_for(150).standard_normal((2, n))).astype(F32)
    k0 = int(0.6 * n)
    x[:, k0] = (2.5, 3.5)                                # the largest |sample|: output index 4 k0 lies in lap two
    assert n * up >= lap_n(lap) and lap < up * k0 - 200 and up * k0 + 200 < 2 * lap
    h, half = resample.design_filter(up, 1)
    y, S = R.poly64(R.mono_mean32(x), h, up, 1, half)
    want = float(np.abs(y).max())
    assert lap < int(np.argmax(np.abs(y))) < 2 * lap and float(np.abs(y[:lap]).max()) < 0.5 * want and float(np.abs(y[2 * lap:]).max()) < 0.5 * want
    bound = float((R.poly_terms(up, half) * U24 * S).max())                     # |max a - max b| <= max |a - b|
    got = _true_peak(x, up)
    print(f"true_peak up=4: got {got!r} want {want!r} diff {abs(got - want):.3e} bound {bound:.3e}")
    assert abs(got - want) <= bound


def test_true_peak_without_oversampling_is_the_mono_maximum(pack):
    lap = LAPS["egr_true_peak"][0]
    n = lap_n(lap)
    x = (0.1 * rng_for(151).standard_normal((2, n))).astype(F32)
    x[:, lap + 777] = (-2.5, -3.25)
    m = R.mono_mean32(x)
    assert int(np.argmax(np.abs(m))) == lap + 777
    assert _true_peak(x, 1) == float(np.abs(m).max())


# ================================================================ 6. order statistics
def _order_arrays(n):
    r = rng_for(160 + n)
    g = r.standard_normal(n).astype(F32)
    if n > 10:
        g[::7] = g[3]
    z = r.choice(np.array([0.0, -0.0, 0.0, -0.0, 1.5, -1.5, 1e-30, -1e-30], F32), n).astype(F32)
    z[0] = -0.0
    z[-1] = 0.0
    inf = r.standard_normal(n).astype(F32)
    inf[r.integers(0, n, max(1, n // 50))] = np.inf
    inf[r.integers(0, n, max(1, n // 50))] = -np.inf
    sub = (r.integers(-1000, 1001, n).astype(np.float64) * 2.0 ** -149).astype(F32)          # multiples of the smallest subnormal
    return {"gauss_ties": g, "all_equal": np.full(n, 0.37, F32), "signed_zeros": z, "infinities": inf, "subnormals": sub}


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 4097])
def test_order_stats2_around_the_group_width_and_on_special_keys(pack, n):
    """Reference: np.sort.  Values are compared with ==, so -0.0 and +0.0 (which the radix keys order, and numpy does not) count as
    equal.  Known limit, not a case: NaN inputs.  The key order puts negative NaNs first and positive NaNs last; numpy sorts every NaN
    last, so the two disagree on arrays that hold a NaN."""
    from egregora_amd import native
    L = native.lib()
    ranks = sorted({(0, n - 1), (0, 0), (n // 2, n // 2), (n - 1, n - 1), (n // 3, min(n - 1, n // 3 + 1)),
                    (int(0.95 * (n - 1)), min(n - 1, int(0.95 * (n - 1)) + 1))})
    for name, v in _order_arrays(n).items():
        if name == "subnormals" and n > 10:
            assert (v < 0).any() and (v > 0).any() and (np.abs(v[v != 0]) < np.finfo(F32).tiny).all()
        vt = cu(v)
        srt = np.sort(v)
        for k0, k1 in ranks:
            o = torch.empty(2, device="cuda")
            native.check(L.egr_order_stats2(native.ptr(vt), n, k0, k1, native.ptr(o), native.stream_ptr()), "egr_order_stats2")
            got = host(o)
            assert got[0] == srt[k0] and got[1] == srt[k1], (name, n, k0, k1, got.tolist(), float(srt[k0]), float(srt[k1]))


# ================================================================ 7. VAD gains with three channels
def _vad_signal(n48):
    r = rng_for(170)
    t = np.arange(n48) / 48000.0
    env = (np.sin(2 * np.pi * 7.0 * t) > 0.2) * (0.5 + 0.5 * np.sin(2 * np.pi * 2.3 * t) ** 2) + 0.05
    x = np.zeros((3, n48))
    x[0] = 0.5 * env * np.sin(2 * np.pi * 220 * t) + 0.02 * r.standard_normal(n48)
    x[2] = 0.03 * env[::-1] * r.standard_normal(n48)                          # another level; channel 1 stays all-zero (p95 == 0)
    return x.astype(F32)


@pytest.mark.parametrize("n48", [480 * 50, 480 * 50 + 17, 480, 960], ids=["whole_frames", "short_last_frame", "one_frame", "two_frames"])
def test_dfn_vad_gains_three_channels(pack, n48):
    """Every mode, both curves, with and without smoothing against oracle/dfn_mix.py, at the tolerances of
    test_dfn_stage.py::test_vad_gain_tables_on_device: 1.2e-7 on the linear-curve gains, 2e-7 on the equal-power ones."""
    from egregora_amd import native
    L = native.lib()
    x = _vad_signal(n48)
    assert not x[1].any()
    xt = cu(x)
    nfr = (n48 + 479) // 480
    ws = torch.empty(int(L.egr_dfn_workspace_bytes(3, n48)), dtype=torch.uint8, device="cuda")
    probs = [odm.vad_probs_rms_48k(x[c]) for c in range(3)]
    assert all(p.shape == (nfr,) for p in probs)
    modes = {0: "off", 1: "more_on_noise", 2: "more_on_speech", 3: "gate_on_noise"}
    for smooth_ms in (0.0, 60.0):
        v = [odm.smooth_probs(p, smooth_ms) for p in probs]
        for mode, mname in modes.items():
            s = [odm.strength_per_frame(0.65, vc, mname, 0.45, 0.9) for vc in v]
            for linear in (1, 0):
                gd = torch.empty((3, nfr), device="cuda")
                gw = torch.empty((3, nfr), device="cuda")
                native.check(L.egr_dfn_vad_gains(native.ptr(xt), 3, n48, smooth_ms, mode, 0.65, 0.45, 0.9, linear, native.ptr(ws),
                                                 native.ptr(gd), native.ptr(gw), native.stream_ptr()), "egr_dfn_vad_gains")
                want = [odm.gains(sc, "linear" if linear else "equal_power") for sc in s]
                wd, ww = np.stack([w[0] for w in want]), np.stack([w[1] for w in want])
                tol = 1.2e-7 if linear else 2e-7
                ed, ew = np.abs(host(gd) - wd).max(axis=1), np.abs(host(gw) - ww).max(axis=1)
                assert ed.max() <= tol and ew.max() <= tol, (n48, smooth_ms, mname, linear, ed.tolist(), ew.tolist())
