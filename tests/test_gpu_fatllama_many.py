"""Waves of clips on one paired chirp-z plan (egr_flmany_*, fatllama_many) on the device.

Bars are the single path's: check() of tests/test_gpu_fatllama_chirpz.py against the float32 / float64 oracle for raw outputs, the
variant tests' bars of tests/test_gpu_fatllama.py for the threshold variants, one PCM_16 step (and at most 5e-2 of the samples above
half a step) behind the node's post-processing.  The largest clip of a wave, and every clip whose own convolution length is the
wave's, must equal the single call bit for bit.  The lengths are picked with the host-only queries so that each wave provably gets
the plan it is meant to test."""
import dataclasses
import os
import subprocess
import sys
import zlib
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import fatllama as ofl
from test_gpu_fatllama import run_gpu, synth
from test_gpu_fatllama_chirpz import check

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _big_prime(n):
    p, f = 1, 2
    while f * f <= n:
        while n % f == 0:
            p, n = f, n // f
        f += 1
    return max(p, n) if n > 1 else p


def near_even(n):
    """The nearest even length whose half has a prime factor above 13 (no packed plan: even/odd packing, kind 1)."""
    for d in range(0, 200, 2):
        for m in (n - d, n + d):
            if m % 2 == 0 and _big_prime(m // 2) > 13:
                return m
    raise AssertionError(n)


# (channels, n_in, factor)
WAVE1 = [(2, 2 * 7919, 1), (1, near_even(14000), 1), (3, near_even(9000), 1), (2, 4 * 1013, 1), (2, 4801, 2)]
WAVE2 = [(2, 48001, 1), (3, 33333, 1), (1, 7919, 1), (2, 101, 1), (2, 3, 1)]


def _sched_wave(L, nc, kind):
    """Three stereo clips on the plan L x nc: the largest D that fits, about 0.9 and 0.6 of it; kind 1 with an even D in the middle."""
    D0 = (L * nc + 1) // 2 - 3
    ds = [D0, int(0.9 * D0), int(0.6 * D0) | 1]
    if kind == 1:
        ds[1] += ds[1] & 1                                         # even D: the extra tile pair (g_per_xcd differs from the odd rows')
        while _big_prime(ds[1]) <= 13:
            ds[1] += 2
        return [(2, 2 * d, 1) for d in ds]
    return [(2, d | 1, 1) for d in ds]


WAVE3A, WAVE3B = _sched_wave(512, 1024, 1), _sched_wave(600, 1024, 2)

_CACHE = {}


def specs_of(clips):
    return [(n, f, 0, C) for C, n, f in clips]


def data(clips, seed=0, **kw):
    return [synth(C, n, seed=seed + n + i, **kw) for i, (C, n, f) in enumerate(clips)]


def oracle(key, clips, xs, iters, thr, **kw):
    """(float32 oracle, float64 oracle) per clip, computed once per key."""
    if key not in _CACHE:
        _CACHE[key] = [(ofl.enhance_channels(x, f, iters, thr, normalize=False, autoscale=False, **kw),
                        ofl.enhance_channels(x, f, iters, thr, normalize=False, autoscale=False, exact=True, **kw))
                       for (C, n, f), x in zip(clips, xs)]
    return _CACHE[key]


def run_wave(pack, clips, xs, iters, thr, flags=0, calls=1):
    """The clips as ONE wave -> per call, per clip, the [C, N] result."""
    from egregora_amd import fatllama_many as fm
    w = fm.Wave(specs_of(clips))
    try:
        xt = [torch.from_numpy(x).cuda() for x in xs]
        res = []
        for _ in range(calls):
            ys = w.enhance(xt, iters, thr, flags)
            torch.cuda.synchronize()
            res.append([y.cpu().numpy() for y in ys])
    finally:
        w.close()
    return res[0] if calls == 1 else res


def own_p_is_the_waves(pack, clips):
    from egregora_amd import fatllama_many as fm
    q = fm.query(specs_of(clips))
    assert q["wave"], q
    return q, [c["P"] == q["P"] for c in q["clips"]]


def check_wave(pack, key, clips, iters, thr=0.6, kind=None, plan=None):
    from egregora_amd import fatllama_engine as fe
    q, same = own_p_is_the_waves(pack, clips)
    if kind:
        assert q["kind"] == kind and all(c["kind"] == kind for c in q["clips"])
    if plan:
        assert (q["L"], q["nc"]) == plan, q
    assert sum(same) >= 1 and sum(same) < len(clips)               # somebody rides on a longer convolution than its own
    xs = data(clips)
    got = run_wave(pack, clips, xs, iters, thr)
    for i, ((C, n, f), x, g, (want, exact)) in enumerate(zip(clips, xs, got, oracle(key, clips, xs, iters, thr))):
        assert np.isfinite(g).all()
        check(g, want, exact, lsd=(f == 1))
        if same[i]:
            np.testing.assert_array_equal(g, run_gpu(pack, x, f, iters, thr), err_msg=f"clip {i}")
    fe.release_plans()
    return got


def test_kind1_wave_on_the_runtime_schedule(pack):
    """Even lengths (even/odd packing): stereo, mono and three channels, an even D among odd ones, an up-rated clip."""
    q, _ = own_p_is_the_waves(pack, WAVE1)
    assert {st["D"] % 2 for st in q["state_rows"]} == {0, 1}
    check_wave(pack, "w1", WAVE1, 3, kind=1)


def test_kind2_wave_with_odd_channel_counts_and_tiny_rows(pack):
    """Odd lengths (channel pairs): a clip of three channels ends in a one-channel state, a mono clip is one, and rows of 101 and 3
    samples sit inside a convolution of ~97 000 points."""
    q, _ = own_p_is_the_waves(pack, WAVE2)
    assert sorted(st["channels"] for st in q["state_rows"]) == [1, 1, 2, 2, 2, 2]
    check_wave(pack, "w2", WAVE2, 3, kind=2)


@pytest.mark.parametrize("switch", [None, "EGR_PZ_PAIRWL", "EGR_PZ_COLWL", "EGR_PZ_SCHED", "EGR_PZ_ROWF"])
def test_kind1_wave_on_the_scheduled_and_two_barrier_kernels(pack, monkeypatch, switch):
    """P = 512 x 1024: compile-time schedules on both passes, the thread-per-column crop and spectrum passes; an even D between two odd
    ones, so the spectrum pass's grid is the even row's and the odd rows leave workgroups idle.  Each switch set to 0 runs the
    sibling kernels on the same wave."""
    from egregora_amd import fatllama_engine as fe
    fe.release_plans()
    if switch:
        monkeypatch.setenv(switch, "0")
    q, _ = own_p_is_the_waves(pack, WAVE3A)
    if switch != "EGR_PZ_SCHED":
        assert (q["L"], q["nc"]) == (512, 1024)
        gs = {st["G"] for st in q["state_rows"]}
        assert len(gs) == 2 and len({-(-g // 8) for g in gs}) == 2     # rows with different g_per_xcd share the launch
    check_wave(pack, "w3a", WAVE3A, 2, kind=1)


def test_kind2_wave_on_the_scheduled_kernels(pack):
    check_wave(pack, "w3b", WAVE3B, 2, kind=2, plan=(600, 1024))


@pytest.mark.parametrize("variant,over,thr", [
    ("relative", {"threshold_ref": "relative_to_max"}, 0.05),
    ("relative,soft", {"threshold_ref": "relative_to_max", "threshold_kind": "soft"}, 0.02),
])
def test_relative_threshold_variants_and_graph_replay(pack, monkeypatch, variant, over, thr):
    """77 iterations: iteration 0 outside the graph, three replays of 25 captured iterations, a plain tail.  Bars of the variant tests
    of tests/test_gpu_fatllama.py: 1e-6 of the output energy (a hard threshold may flip a borderline bin), the soft shrink also
    2e-5 of the peak.  Plain launches give the same bits, and so does a second call on the same wave."""
    from egregora_amd import fatllama_engine as fe
    spec = dataclasses.replace(ofl.FatLlamaSpec(), **over)
    xs = data(WAVE1, seed=77)
    flags = fe.variant_flags(variant)
    first, second = run_wave(pack, WAVE1, xs, 77, thr, flags, calls=2)
    monkeypatch.setenv("EGR_FL_GRAPH", "0")
    plain = run_wave(pack, WAVE1, xs, 77, thr, flags)
    for (C, n, f), x, a, b, c in zip(WAVE1, xs, first, second, plain):
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(a, c)
        want = ofl.enhance_channels(x, f, 77, thr, normalize=False, autoscale=False, spec=spec)
        num = float(np.sum((a - want).astype(np.float64) ** 2)); den = float(np.sum(want.astype(np.float64) ** 2)) + 1e-30
        assert num / den < 1e-6, (variant, n, num / den)
        if "soft" in variant:
            assert float(np.max(np.abs(a - want))) <= 2e-5 * float(np.max(np.abs(want))), (variant, n)


def test_a_row_does_not_depend_on_its_neighbours(pack):
    """The same lengths with every other clip's samples replaced and the clip order permuted: a clip's bits stay."""
    for clips in (WAVE1, WAVE2):
        xs = data(clips)
        base = run_wave(pack, clips, xs, 3, 0.6)
        perm = [3, 0, 4, 2, 1]
        for keep in (1, 3):
            ys = [x if i == keep else synth(x.shape[0], x.shape[1], seed=900 + i, scale=3000.0) for i, x in enumerate(xs)]
            got = run_wave(pack, [clips[i] for i in perm], [ys[i] for i in perm], 3, 0.6)
            np.testing.assert_array_equal(got[perm.index(keep)], base[keep])


@pytest.mark.parametrize("normalize,autoscale", [(False, False), (False, True), (True, False), (True, True)])
def test_finalize_runs_over_the_clips_own_channels(pack, normalize, autoscale):
    """PCM_16 in, the node's post-processing out, against the single call per clip (bit-equal where the own P is the wave's, else one
    PCM_16 step) and against the oracle's node.  The second clip is so quiet that it quantises to silence: its peak does not trigger
    the /32768 write patch while its neighbours' peaks do (without normalisation)."""
    from egregora_amd import fatllama_engine as fe, native
    clips = [(2, 2 * 7919, 1), (2, near_even(15000), 1), (1, near_even(9000), 2), (3, 4 * 1013, 1)]
    _, same = own_p_is_the_waves(pack, clips)
    xs = [synth(C, n, seed=60 + i, scale=0.5 if i != 1 else 1e-6, integer=False) for i, (C, n, f) in enumerate(clips)]
    flags = fe._flags(normalize, autoscale, True, True, "")
    got = run_wave(pack, clips, xs, 3, 0.6, flags)
    assert not got[1].any() and got[0].any()
    for i, ((C, n, f), x, g) in enumerate(zip(clips, xs, got)):
        single = run_gpu(pack, x, f, 3, 0.6, normalize, autoscale, pcm_in=True, node_post=True)
        sr = {(2, 1): 48000, (1, 2): 48000, (3, 1): 32000}[(C, f)]          # the rate at which the node up-rates this clip by f
        assert fe.upscale_factor(sr, C, 1536) == f
        want, _ = ofl.node_run(x, sr, 3, 0.6, 1536, normalize, autoscale)
        for ref in (single, want):
            lsb = np.abs(g - ref) * 32768.0
            assert float(lsb.max()) <= 1.0 + 1e-6 and float(np.mean(lsb > 0.5)) <= 5e-2, (i, float(lsb.max()))
        if same[i]:
            np.testing.assert_array_equal(g, single, err_msg=f"clip {i}")
    assert native.FL_NODE_POST & flags
    fe.release_plans()


def test_enhance_many_over_several_waves(pack, monkeypatch):
    """Both kinds, a packed length, mono and stereo, two rates with different factors, ratio_then_int once: order, shapes, rates and
    stats, and every clip within one PCM_16 step of the single node."""
    from egregora_amd import fatllama_engine as fe, fatllama_many as fm
    monkeypatch.setattr(fm, "MAX_ROWS", 4)
    monkeypatch.setenv("EGREGORA_FATLLAMA_WAVE_SLACK", "100")
    lens = [(2, 15838, 48000), (2, 14006, 48000), (1, 9002, 48000), (2, 9602, 48000), (2, 4800, 48000), (2, 4801, 48000),
            (1, 3333, 24000), (2, 7919, 48000), (1, 4052, 96000)]
    clips = [(torch.from_numpy(synth(C, n, seed=70 + i, scale=0.5, integer=False)), sr) for i, (C, n, sr) in enumerate(lens)]
    for variant in ("", "linspace,ratio_then_int"):
        monkeypatch.setenv("EGREGORA_FATLLAMA_SPEC", variant)
        stats = {}
        res = fm.enhance_many(clips, 3, 0.6, 1536, True, True, stats=stats)
        assert len(res) == len(clips) and stats["waves"] >= 3 and stats["waves"] == len(stats["rows"]) == len(stats["padding"])
        assert all(r <= 4 for r in stats["rows"]) and all(p >= 1.0 for p in stats["padding"])
        assert stats["fallbacks"] + sum(len(w) for w in stats["wave_clips"]) == len(clips)
        if not variant:
            assert 4 not in [i for w in stats["wave_clips"] for i in w]      # the packed length runs through enhance_device
        for i, ((x, sr), (y, sr_out)) in enumerate(zip(clips, res)):
            ref, sr_ref = fe.node_run(x, sr, 3, 0.6, 1536, True, True)
            assert sr_out == sr_ref and tuple(y.shape) == tuple(ref.shape) and y.dtype == torch.float32 and not y.is_cuda
            lsb = (y - ref.cpu()).abs().numpy() * 32768.0
            assert float(lsb.max()) <= 1.0 + 1e-6 and float(np.mean(lsb > 0.5)) <= 5e-2, (variant, i, float(lsb.max()))
    fe.release_plans()


def test_refusals_come_before_any_allocation_or_launch(pack):
    import ctypes as C
    from egregora_amd import fatllama_many as fm, native
    L = native.lib()
    torch.cuda.synchronize()
    free = lambda: torch.cuda.mem_get_info()[0]

    def create(specs):
        h = C.c_void_p()
        rc = L.egr_flmany_create(C.byref(h), len(specs), *fm._arrays(specs)) if specs else \
            L.egr_flmany_create(C.byref(h), 0, None, None, None, None)
        return rc, h

    before = free()
    for specs, want in (([(15838, 1, 0, 2), (48001, 1, 0, 2)], 3), ([(15838, 1, 0, 2), (48000, 1, 0, 2)], 3),
                        ([(40000003, 1, 0, 1), (48001, 1, 0, 2)], 3), ([], 1), ([(4801, 1, 0, 600)] * 2, 3)):
        rc, h = create(specs)
        assert rc == want and not h.value, (specs, rc, native.last_error())
        assert free() == before
    rc, _ = create([(15838, 1, 0, 2), (48000, 1, 0, 2)])
    assert rc == 3 and "clip 1" in native.last_error()           # the refusal names the clip
    w = fm.Wave([(4801, 1, 0, 2), (3333, 1, 0, 2)])
    try:
        x = torch.zeros(w.x_floats, device="cuda")
        out = torch.zeros(w.out_floats, device="cuda")
        assert not out.any() and not x.any()          # (the allocator's block for the reduction's result exists before the reading)
        torch.cuda.synchronize()
        before = free()
        for iters, flags, want in ((0, 0, 1), (3, native.FL_THR_RELATIVE | native.FL_THR_RECOMPUTE, 3), (3, native.FL_DEFER_FINALIZE, 3)):
            rc = L.egr_flmany_enhance(w.h, native.ptr(x), native.ptr(out), iters, 0.6, flags, native.stream_ptr())
            assert rc == want, (iters, flags, rc)
            torch.cuda.synchronize()
            assert free() == before and not out.any()
    finally:
        w.close()


_DIGEST = r"""
import sys, zlib
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, torch
from packload import load_pack
pack = load_pack()
import test_gpu_fatllama_many as t
from egregora_amd import native
for name, clips, iters in (("w1", t.WAVE1, 3), ("w2", t.WAVE2, 3), ("w3a", t.WAVE3A, 2), ("w3b", t.WAVE3B, 2)):
    got = t.run_wave(pack, clips, t.data(clips), iters, 0.6)
    print("DIGEST", name, " ".join("%%08x" %% zlib.crc32(np.ascontiguousarray(g).tobytes()) for g in got))
print("CANARY", native.lib().egr_lds_canary_failures())
"""


def test_guard_band_library_runs_the_waves_clean(pack):
    """The library built with LDS guard bands, in a fresh process: the waves above give the regular library's bits and no guard is hit."""
    canary = ROOT / "variants" / "lib_canary.so"
    assert canary.exists(), "variants/lib_canary.so missing: build() makes it"
    code = _DIGEST % (str(ROOT), str(ROOT / "tests"))
    outs = []
    for lib in (None, canary):
        env = {k: v for k, v in os.environ.items() if k != "EGREGORA_AMD_LIB"}
        if lib:
            env["EGREGORA_AMD_LIB"] = str(lib)
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append([ln for ln in r.stdout.splitlines() if ln.startswith(("DIGEST", "CANARY"))])
    assert len(outs[0]) == 5 and outs[0][:4] == outs[1][:4]
    assert outs[0][4] == "CANARY -1" and outs[1][4] == "CANARY 0"


def test_batch_node_and_cli(pack, tmp_path, monkeypatch):
    """The opt-in list node on three tiny clips ([B,C,T] counts as B clips) and the directory front end on the same clips."""
    from egregora_amd import egregora_fat_llama_gpu_batch as B, fatllama_batch, wavio
    single = pack.NODE_CLASS_MAPPINGS["EgregoraFatLlamaGPU"]()
    node = B.EgregoraFatLlamaGPUBatch()
    assert B.EgregoraFatLlamaGPUBatch.INPUT_IS_LIST and B.EgregoraFatLlamaGPUBatch.OUTPUT_IS_LIST == (True,)
    assert set(B.EgregoraFatLlamaGPUBatch.INPUT_TYPES()["required"]) == set(single.INPUT_TYPES()["required"])
    names = ("a.wav", "b.wav", "sub/c.wav")
    ind, outd = tmp_path / "in", tmp_path / "out"
    (ind / "sub").mkdir(parents=True)
    for i, (name, n) in enumerate(zip(names, (4801, 4801, 3333))):
        wavio.write_wav_pcm16(str(ind / name), synth(2, n, seed=90 + i, scale=0.5, integer=False).T, 48000)
    xs = [fatllama_batch.read_clip(ind / name)[0].numpy() for name in names]          # what the files hold, as the node reads them
    assert all(x.shape[0] == 2 for x in xs)
    audio = [{"waveform": torch.from_numpy(np.stack(xs[:2])), "sample_rate": 48000}, {"waveform": torch.from_numpy(xs[2])[None], "sample_rate": 48000}]
    (outs,) = node.run(["wav"], [3], [0.6], [1536], [True], [True], AUDIO=audio)
    assert isinstance(outs, list) and len(outs) == 3
    for x, o in zip(xs, outs):
        (ref,) = single.run("wav", 3, 0.6, 1536, True, True, AUDIO={"waveform": torch.from_numpy(x)[None], "sample_rate": 48000})
        assert o["sample_rate"] == ref["sample_rate"] and tuple(o["waveform"].shape) == tuple(ref["waveform"].shape) == (1, 2, x.shape[1])
        lsb = (o["waveform"] - ref["waveform"]).abs().numpy() * 32768.0
        assert float(lsb.max()) <= 1.0 + 1e-6 and float(np.mean(lsb > 0.5)) <= 5e-2
    assert fatllama_batch.main(["--in-dir", str(ind), "--out-dir", str(outd), "--max-iterations", "3", "--bitrate", "1536"]) == 0
    for name, o in zip(names, outs):
        y, sr = fatllama_batch.read_clip(outd / name)
        assert sr == o["sample_rate"]
        # the file holds rint(sample x 32767), the PCM_16 writer's rule; the reader divides by 32768
        np.testing.assert_array_equal(np.rint(y.numpy() * 32768.0), np.rint(o["waveform"][0].numpy() * np.float32(32767.0)))
