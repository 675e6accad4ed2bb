"""Values of the FlashSR operator kernels of csrc/egr_nn_ops.hip PAST THE FIRST GRID LAP, on every branch their launchers can pick,
and at the widths where a kernel changes its path.

Every kernel there is a grid-stride loop under a capped grid: grid1d() stops at 8192 workgroups of 256 threads, row_grid_x() at
8192 / B workgroups per batch row, egr_layernorm_rows_ra at 16384 / batch_rows workgroups of 4 rows, egr_conv_cin1 at 8192 workgroups of
256 / (Cout / 4) pixels; production tensors take tens of laps.  LAPS names, per entry point, the items one lap covers and the launcher
text that says so.  The flat cases run 2 lap + 805 items or the nearest size the shapes allow (the Winograd cases one lap and a ragged
second); the row-grid cases get their laps from many batch rows (8192 of them leave one workgroup per row), with each row's largest |y|
planted behind the row's first lap, so a row maximum that loses later laps is wrong.

References are numpy / CPU torch on the host (tests/nn_refs.py, checked by tests/test_nn_refs.py), never a device kernel:
  bit-exact      against the float32 restatement where the kernel only moves values or adds in a written order (concat, copy, transpose,
                 tap gather, col2im, the plain Winograd transforms, EW_ADD / EW_SCALE / EW_ADD_SCALE), and the row maxima against the
                 host maximum of the device's own y;
  the suite's bound (tests/test_gpu_flashsr.py: 2e-5 max |want| + 1e-6; 3e-5 for GroupNorm, LayerNorm and snake) against float64 where
                 the kernel uses fast intrinsics or device math;
  4 x the float32 restatement's own error against float64 (the rule of tests/test_gpu_fatllama_levels.py) for conv_cin1, AXPBY, the
                 Chebyshev gain, Box-Muller, the STFT magnitudes and GroupNorm with a large mean.  The ratios are printed and recorded
                 in profiles/nn_ops_laps.md.

The Winograd lap cases use B = 2 images of 181 x 91 (2 x 91 x 46 tiles x 256 quads = lap + 46 080 items): one image is half a lap.

Switches that are read once per process (EGR_SNAKE_SPAN=0, EGR_SNAKE=tiled) run in fresh child processes (this file as a script)."""
import ctypes as C
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
for _p in (str(ROOT), str(ROOT / "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import nn_refs as N
from glue_refs import F32, bits_differ, lap_n, where_bad

pytestmark = pytest.mark.gpu
F64 = np.float64
RA = 32                       # include/egregora_amd.h EGR_ROW_AMAX_STRIDE
LAP = 8192 * 256              # grid1d(): items of one lap
SRC = ROOT / "comfyui-egregora-audio-super-resolution_amd" / "csrc"
# entry point -> (items one lap covers, the launcher text in egr_nn_ops.hip / egr_rowmax.h that says so)
LAPS = {
    "grid1d": (LAP, "(b < 1 ? 1 : (b > 8192 ? 8192 : b))"),
    "egr_tap_gather": (LAP, "k_tap_gather, dim3(grid1d((long long)B * H * W * Cout))"),
    "egr_col2im_convtr1d": (LAP, "k_col2im1d, dim3(grid1d(n))"),
    "egr_randn_base": (LAP, "k_randn, dim3(grid1d(n))"),                                            # quads
    "egr_lowpass_gain": (LAP, "k_cheby_gain, dim3(grid1d(nbins), B)"),                              # per row
    "egr_winograd_input": (LAP, "k_wino_in, dim3(grid1d(n))"),                                      # (tile, channel quad)
    "egr_winograd_output": (LAP, "k_wino_out, dim3(grid1d(n))"),
    "egr_conv_cin1": (8192, "if (nb > 8192) nb = 8192;\n    if (KH == 3) hipLaunchKernelGGL((k_conv_cin1<9>)"),      # x 256 / (Cout / 4) pixels
    "row_grid_x": (256, "cap = max_wg / (B < 1 ? 1 : B);"),                                        # one workgroup per row at B = max_wg
    "egr_eltwise_ra": (256, "k_eltwise, dim3(row_grid_x(per, batch_rows, 8192, 4)"),
    "egr_geglu_ra": (256, "k_geglu, dim3(row_grid_x(per * D, batch_rows, 8192, 4)"),
    "egr_concat_channels_ra": (256, "k_concat, dim3(row_grid_x(per * (C1 + C2), batch_rows, 8192, 4)"),
    "egr_groupnorm_nhwc_ra": (256, "k_affine_c, dim3(row_grid_x(n4, B, 8192, 2)"),                  # quads
    "egr_layernorm_rows_ra": (4, "cap = std::max<long long>(1, 16384 / batch_rows);"),              # rows per workgroup, x the cap
    "egr_snake_aa_ra": (256, "getenv(\"EGR_SNAKE_WG\") ? atoi(getenv(\"EGR_SNAKE_WG\")) : 8192;"),    # (run or span, channel)
}
BIG_B = 8192                  # batch rows that leave one workgroup per row
RATIOS = []


def rng_for(seed):
    return np.random.Generator(np.random.PCG64(seed))


def uni(r, shape, scale=1.0):
    """Uniform float32 in (-scale, scale): the quick generator for the inputs of several hundred MB."""
    a = r.random(shape, dtype=F32)
    a -= F32(0.5)
    a *= F32(2 * scale)
    return a


_KEEP = []                    # device copies made by cu() live until the test ends: the calls below take raw pointers of them


def cu(a):
    if a is None:
        return None
    _KEEP.append(torch.from_numpy(np.ascontiguousarray(a)).cuda())
    return _KEEP[-1]


@pytest.fixture(autouse=True)
def _release_device_copies():
    yield
    _KEEP.clear()


def host(t):
    return t.cpu().numpy()


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def nan_like(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def lib():
    from packload import load_pack
    load_pack()
    from egregora_amd import native
    return native.lib()


def st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ok(rc, what):
    from egregora_amd import native
    native.check(rc, what)


def over_bound(got, want, tol):
    """Mask of the suite's operator bound: |got - want| > tol max |want| + 1e-6."""
    want = np.asarray(want, F64)
    return ~(np.abs(got.astype(F64) - want) <= tol * float(np.abs(want).max()) + 1e-6)


def over_4x(got, rest32, want, what):
    """Mask of the 4x rule: |got - want| > 4 max |restatement - want|; prints and records the ratio of the maxima."""
    want = np.asarray(want, F64)
    err_r = float(np.abs(rest32.astype(F64) - want).max())
    d = np.abs(got.astype(F64) - want)
    err_g = float(d.max()) if np.isfinite(d).all() else float("inf")
    ratio = err_g / err_r if err_r > 0 else (0.0 if err_g == 0 else float("inf"))
    RATIOS.append((what, err_g, err_r, ratio))
    print(f"ratio {what}: device {err_g:.3e} / restatement {err_r:.3e} = {ratio:.2f} (bar 4)")
    return ~(d <= 4.0 * err_r)


def amax_differs(ra, y, B):
    """Rows whose row_amax slot is not, bit for bit, the host maximum of |y| over that row of the device's own y."""
    return bits_differ(host(ra)[::RA][:B], np.abs(y.reshape(B, -1)).max(axis=1))


def test_lap_table_still_describes_the_launchers():
    """Every launcher text quoted in LAPS is still in the source: a launcher that changes its cap fails here and sends its reader to
    the table and to the sizes below."""
    src = (SRC / "egr_nn_ops.hip").read_text(encoding="utf-8") + (SRC / "egr_rowmax.h").read_text(encoding="utf-8")
    missing = [name for name, (_, text) in LAPS.items() if text not in src]
    assert not missing, missing
    assert lap_n(LAP) == 2 * LAP + 805 and 2 * 91 * 46 * 256 > LAP + 4096


# ================================================================ 1. flat grid1d laps
@pytest.fixture(scope="module")
def tap_inputs():
    B, H, W, Co = 3, 500, 933, 3
    r = rng_for(1)
    P = uni(r, (B, H, W, 9 * Co))
    return dict(B=B, H=H, W=W, Co=Co, P=P, Pd=cu(P), bias=r.standard_normal(Co).astype(F32))


@pytest.mark.parametrize("with_bias", [True, False])
def test_tap_gather_past_the_lap(pack, tap_inputs, with_bias):
    t = tap_inputs
    lap = LAPS["egr_tap_gather"][0]
    n = t["B"] * t["H"] * t["W"] * t["Co"]
    assert n == 4198500 and n >= lap_n(lap)
    bias = t["bias"] if with_bias else None
    y = nan_like(t["B"], t["H"], t["W"], t["Co"])
    ok(lib().egr_tap_gather(p(t["Pd"]), p(cu(bias)), p(y), t["B"], t["H"], t["W"], 3, 3, t["Co"], 1, 1, st()), "egr_tap_gather")
    bad = bits_differ(host(y), N.tap_gather(t["P"], bias, 3, 3, t["Co"], 1, 1, F32))
    assert not bad.any(), where_bad(bad, lap, f"tap_gather bias={with_bias}")


@pytest.mark.parametrize("extras", [True, False])
def test_col2im_past_the_lap(pack, extras):
    from egregora_amd import flashsr_arch as A
    lap = LAPS["egr_col2im_convtr1d"][0]
    r_, B, Lin, Co = 5, 2, 6600, 64
    K = A.up_kernel(r_)
    Lout, pad = Lin * r_, (K - r_) // 2
    assert B * Lout * Co == 4224000 >= lap_n(lap) and K == 11
    r = rng_for(2)
    Y = uni(r, (B, Lin, K, Co))
    bias = r.standard_normal(Co).astype(F32) if extras else None
    add = uni(r, (B, Lout, Co)) if extras else None
    out = nan_like(B, Lout, Co)
    ok(lib().egr_col2im_convtr1d(p(cu(Y)), p(cu(bias)), p(cu(add)), p(out), B, Lin, Lout, Co, K, r_, pad, st()), "egr_col2im_convtr1d")
    bad = bits_differ(host(out), N.col2im(Y, bias, add, Lout, r_, pad, F32))
    assert not bad.any(), where_bad(bad, lap, f"col2im bias+add={extras}")


def _randn(per_row, rows, seed, ids, base):
    out = nan_like(rows, per_row)
    idt = None if ids is None else torch.tensor(ids, dtype=torch.int64, device="cuda")
    ok(lib().egr_randn_base(p(out), per_row, rows, seed, p(idt), base, st()), "egr_randn_base")
    return host(out)


def test_randn_past_the_lap_with_row_ids_and_id_base(pack):
    lap = LAPS["egr_randn_base"][0]
    rows, per_row, seed = 3, 5593481, 0x1F2E3D4C5B6A7988
    quads = (per_row + 3) // 4
    assert per_row % 4 == 1 and rows * quads >= lap_n(lap)
    ids = [5, 2 ** 33 + 1, 7]
    a = _randn(per_row, rows, seed, ids, 12345)                 # id_base is not used beside row_ids
    b = _randn(per_row, rows, seed, None, 2 ** 33)              # ids 2^33, 2^33 + 1, 2^33 + 2

    def items(bad):
        m = np.zeros((rows, quads * 4), bool)
        m[:, :per_row] = bad
        return m.reshape(rows, quads, 4).any(axis=2)

    for got, idl, what in ((a, ids, "row_ids"), (b, [2 ** 33 + k for k in range(3)], "id_base")):
        want, rest = N.randn(per_row, rows, seed, idl), N.randn(per_row, rows, seed, idl, single=True)
        bad = over_4x(got, rest, want, f"randn {what}")
        assert not bad.any(), where_bad(items(bad), lap, f"randn {what} (quads)")
    assert np.array_equal(a[1], b[1]) and not np.array_equal(a[0], b[0]) and not np.array_equal(a[2], b[2])


def test_chebyshev_gain_past_the_lap_with_two_cutoffs(pack):
    lap = LAPS["egr_lowpass_gain"][0]
    B, T, nb, ldm, nbins = 2, 3, 65, 80, 4195109
    assert nbins >= lap_n(lap)
    r = rng_for(4)
    mag = np.zeros((B, T, ldm), F32)
    mag[0, :, :20] = r.uniform(0.5, 1.0, (T, 20))
    mag[1, :, :45] = r.uniform(0.5, 1.0, (T, 45))
    mag[:, :, :nb] += F32(1e-4)
    cuts = N.cutoff_bin(mag, nb, 0.985)
    assert 0 < cuts[0] < cuts[1] < nb - 1
    cut, gain = torch.full((B,), -1, dtype=torch.int32, device="cuda"), nan_like(B, nbins)
    ok(lib().egr_lowpass_gain(p(cu(mag)), B, T, ldm, nb, 0.985, 48000.0, 8, 0.05, nbins, p(cut), p(gain), st()), "egr_lowpass_gain")
    assert host(cut).tolist() == cuts.tolist()
    want, rest = N.cheby_gain64(cuts, nb, 48000.0, 8, 0.05, nbins), N.cheby_gain32(cuts, nb, 48000.0, 8, 0.05, nbins)
    bad = over_4x(host(gain), rest, want, "cheby_gain")
    assert not bad.any(), where_bad(bad.any(axis=0), lap, "cheby_gain (bin inside a row)")


WB, WH, WW, WC = 2, 181, 91, 1024            # 2 x 91 x 46 tiles x 256 channel quads = lap + 46 080 items


@pytest.fixture(scope="module")
def wino_inputs():
    r = rng_for(5)
    TH, TW = N.wino_tiles(WH, WW)
    x = uni(r, (WB, WH, WW, WC), 2.0)
    x[1] *= F32(0.25)
    sc, sh = (1 + 0.1 * r.standard_normal((WB, WC))).astype(F32), (0.1 * r.standard_normal((WB, WC))).astype(F32)
    M = uni(r, (16, WB * TH * TW, WC))
    bias, res = r.standard_normal(WC).astype(F32), uni(r, (WB, WH, WW, WC))
    assert (TH, TW) == (91, 46) and LAP < WB * TH * TW * (WC // 4) < 2 * LAP
    return dict(x=x, sc=sc, sh=sh, M=M, bias=bias, res=res, TH=TH, TW=TW, d={k: cu(v) for k, v in dict(x=x, sc=sc, sh=sh, M=M, bias=bias, res=res).items()})


def _tail_rows(lap):
    """First tile row ty0 of the last image such that every item from lap - 4096 on lies in tile rows >= ty0 of that image."""
    TH, TW = N.wino_tiles(WH, WW)
    t0 = (lap - 4096) // (WC // 4) - (WB - 1) * TH * TW
    assert t0 > TW
    return t0 // TW


@pytest.mark.parametrize("mode", ["plain", "gn", "gn_silu"])
def test_winograd_input_past_the_lap(pack, wino_inputs, mode):
    """Plain: every value bit-exact.  Fused GroupNorm (+SiLU): the operator bound against float64 on every item from 4096 before the
    lap to the end (the tile rows >= ty0 of the second image; the float64 transform of everything takes over 5 s)."""
    w, lap = wino_inputs, LAPS["egr_winograd_input"][0]
    TH, TW, d = w["TH"], w["TW"], w["d"]
    P = WB * TH * TW
    V = nan_like(16, P, WC)
    gn = mode != "plain"
    ok(lib().egr_winograd_input(p(d["x"]), p(d["sc"] if gn else None), p(d["sh"] if gn else None), int(mode == "gn_silu"), WB, WH, WW, WC,
                                p(V), st()), "egr_winograd_input")
    got = host(V)
    del V
    items = lambda bad: bad.reshape(16, P, WC // 4, 4).any(axis=(0, 3)).reshape(-1)
    if not gn:
        bad = bits_differ(got, N.wino_in(w["x"], dtype=F32))
        assert not bad.any(), where_bad(items(bad), lap, "winograd_input plain (tile, channel quad)")
        return
    ty0 = _tail_rows(lap)
    sub = N.wino_in(w["x"][WB - 1:, 2 * (ty0 - 1):], w["sc"][WB - 1:], w["sh"][WB - 1:], mode == "gn_silu")      # one tile row early: its
    want = sub.reshape(16, TH - ty0 + 1, TW, WC)[:, 1:].reshape(16, -1, WC)                                      # top edge is not padding
    t0 = (WB - 1) * TH * TW + ty0 * TW
    assert t0 * (WC // 4) <= lap - 4096 and want.shape[1] == P - t0
    bad = np.isnan(got)                                                          # the fill of an element nobody wrote, anywhere
    bad[:, t0:] |= over_bound(got[:, t0:], want, 2e-5)
    assert not bad.any(), where_bad(items(bad), lap, f"winograd_input {mode} (tile, channel quad)")


@pytest.mark.parametrize("mode", ["plain", "bias_res", "bias_res_silu"])
def test_winograd_output_past_the_lap(pack, wino_inputs, mode):
    """Plain and bias + res: additions in a written order, bit-exact everywhere.  With SiLU: the operator bound against float64 from 4096
    items before the lap on."""
    w, lap = wino_inputs, LAPS["egr_winograd_output"][0]
    TH, TW, d = w["TH"], w["TW"], w["d"]
    full = mode != "plain"
    y = nan_like(WB, WH, WW, WC)
    ok(lib().egr_winograd_output(p(d["M"]), p(d["bias"] if full else None), p(d["res"] if full else None), p(y), WB, WH, WW, WC,
                                 int(mode == "bias_res_silu"), st()), "egr_winograd_output")
    got = host(y)

    def items(bad):
        m = np.zeros((WB, 2 * TH, 2 * TW, WC), bool)
        m[:, :WH, :WW] = bad
        return m.reshape(WB, TH, 2, TW, 2, WC // 4, 4).any(axis=(2, 4, 6)).reshape(-1)

    if mode != "bias_res_silu":
        bad = bits_differ(got, N.wino_out(w["M"], WH, WW, w["bias"] if full else None, w["res"] if full else None, 0, F32))
        assert not bad.any(), where_bad(items(bad), lap, f"winograd_output {mode} (tile, channel quad)")
        return
    ty0 = _tail_rows(lap)
    r0, t0 = 2 * ty0, (WB - 1) * TH * TW + ty0 * TW
    want = N.wino_out(w["M"][:, t0:], WH - r0, WW, w["bias"], w["res"][WB - 1:, r0:], 1)[0]      # the tile rows >= ty0 of the last image
    assert t0 * (WC // 4) <= lap - 4096
    bad = np.isnan(got)                                                          # the fill of an element nobody wrote, anywhere
    bad[WB - 1, r0:] |= over_bound(got[WB - 1, r0:], want, 2e-5)
    assert not bad.any(), where_bad(items(bad), lap, "winograd_output bias_res_silu (tile, channel quad)")


@pytest.mark.parametrize("name,B,H,W,Co,k,with_bias", [("3x3_cout1024", 2, 107, 80, 1024, 3, True), ("1x1_cout4", 1, 37, 29, 4, 1, True),
                                                       ("1x1_cout64", 2, 300, 441, 64, 1, True), ("3x3_cout8_nobias", 2, 9, 11, 8, 3, False)])
def test_conv_cin1_past_the_lap(pack, name, B, H, W, Co, k, with_bias):
    ppi = 256 // (Co // 4)
    lap = LAPS["egr_conv_cin1"][0] * ppi
    if name in ("3x3_cout1024", "1x1_cout64"):
        assert B * H * W >= 2 * lap + 700
    r = rng_for(6 + Co)
    x = r.standard_normal((B, H, W)).astype(F32)
    wp = N.pack_cin1((r.standard_normal((Co, k, k)) / k).astype(F32))
    bias = r.standard_normal(Co).astype(F32) if with_bias else None
    y = nan_like(B, H, W, Co)
    ok(lib().egr_conv_cin1(p(cu(x)), p(cu(wp)), p(cu(bias)), p(y), B, H, W, Co, k, k, k // 2, k // 2, st()), "egr_conv_cin1")
    want = N.conv_cin1(x, wp, bias, k, k, k // 2, k // 2)
    rest = N.conv_cin1(x, wp, bias, k, k, k // 2, k // 2, fused32=True)
    bad = over_4x(host(y), rest, want, f"conv_cin1 {name}")
    assert not bad.any(), where_bad(bad.any(axis=3), lap, f"conv_cin1 {name} (pixels)")


# ================================================================ 2. row-grid laps: one workgroup per batch row
def _row_scales(B):
    return (0.5 + (np.arange(B) % 97) / 97.0).astype(F32)


def _check_rows(got, want_mask, ra, B, lap, what):
    """(every mask here counts a NaN, the fill of an element nobody wrote, as bad)"""
    assert not want_mask.any(), where_bad(want_mask.reshape(B, -1).any(axis=0), lap, what + " (item inside a row)")
    bad = amax_differs(ra, got, B)
    assert not bad.any(), where_bad(bad, BIG_B, what + " row maxima (rows)")


EW = [("add", N.EW_ADD, "bits"), ("axpby", N.EW_AXPBY, "4x"), ("silu", N.EW_SILU, "bound"), ("scale", N.EW_SCALE, "bits"),
      ("copy", N.EW_COPY, "bits"), ("add_scale", N.EW_ADD_SCALE, "bits")]


@pytest.fixture(scope="module", params=[(BIG_B, 1061), (65535, 37)], ids=["8192x1061", "65535x37"])
def ew_inputs(request):
    B, per = request.param
    r = rng_for(7 + per)
    s = _row_scales(B)[:, None]
    a, b = r.standard_normal((B, per)).astype(F32) * s, r.standard_normal((B, per)).astype(F32) * s
    pos = (1024 + np.arange(B) % 37) if per > 1024 else np.arange(B) % per          # behind 256 x min_items (4) items of the row
    a[np.arange(B), pos] = 50 * s[:, 0]
    b[np.arange(B), pos] = 50 * s[:, 0]
    return dict(B=B, per=per, a=a, b=b, pos=pos, ad=cu(a), bd=cu(b))


@pytest.mark.parametrize("name,op,rule", EW, ids=[e[0] for e in EW])
def test_eltwise_rows_and_maxima_past_the_row_lap(pack, ew_inputs, name, op, rule):
    e, lap = ew_inputs, LAPS["egr_eltwise_ra"][0]
    B, per = e["B"], e["per"]
    s0, s1 = 0.7, -1.3
    binary = op in (N.EW_ADD, N.EW_AXPBY, N.EW_ADD_SCALE)
    y, ra = nan_like(B, per), torch.zeros(B * RA, device="cuda")
    ok(lib().egr_eltwise_ra(p(e["ad"]), p(e["bd"] if binary else None), p(y), B * per, op, s0, s1, B, p(ra), st()), "egr_eltwise_ra")
    got = host(y)
    want = N.eltwise64(e["a"], e["b"], op, s0, s1)
    assert (np.abs(want).argmax(axis=1) == e["pos"]).all()                      # the row's largest |y| is the planted one
    rest = N.eltwise32(e["a"], e["b"], op, s0, s1)
    if rule == "bits":
        bad = bits_differ(got, rest)
    elif rule == "4x":
        bad = over_4x(got, rest, want, f"eltwise {name} {B}x{per}")
    else:
        bad = over_bound(got, want, 2e-5)
    _check_rows(got, bad, ra, B, lap, f"eltwise {name} {B}x{per}")


@pytest.mark.parametrize("B,per,D", [(BIG_B, 3, 353), (65535, 1, 37)])
def test_geglu_rows_and_maxima_past_the_row_lap(pack, B, per, D):
    lap = LAPS["egr_geglu_ra"][0]
    r = rng_for(8 + D)
    s = _row_scales(B)
    u = r.standard_normal((B, per, 2 * D)).astype(F32) * s[:, None, None]
    d = (320 + np.arange(B) % 30) if per * D > 1024 else np.arange(B) % D        # item (per - 1) D + d >= 1024
    u[np.arange(B), per - 1, d] = 30 * s
    u[np.arange(B), per - 1, D + d] = 5.0
    assert per * D <= 1024 or ((per - 1) * D + d >= 1024).all()
    y, ra = nan_like(B, per, D), torch.zeros(B * RA, device="cuda")
    ok(lib().egr_geglu_ra(p(cu(u)), p(y), B * per, D, B, p(ra), st()), "egr_geglu_ra")
    got = host(y)
    want = N.geglu64(u, D)
    assert (np.abs(want).reshape(B, -1).argmax(axis=1) == (per - 1) * D + d).all()
    _check_rows(got, over_bound(got, want, 2e-5), ra, B, lap, f"geglu {B}x{per}x{D}")


@pytest.mark.parametrize("B,per,C1,C2", [(BIG_B, 3, 100, 253), (65535, 1, 5, 32)])
def test_concat_rows_and_maxima_past_the_row_lap(pack, B, per, C1, C2):
    lap = LAPS["egr_concat_channels_ra"][0]
    r = rng_for(9 + C1)
    s = _row_scales(B)[:, None, None]
    a, b = r.standard_normal((B, per, C1)).astype(F32) * s, r.standard_normal((B, per, C2)).astype(F32) * s
    c = (320 + np.arange(B) % 30) if per * (C1 + C2) > 1024 else C1 + np.arange(B) % C2
    b[np.arange(B), per - 1, c - C1] = -40 * s[:, 0, 0]
    y, ra = nan_like(B, per, C1 + C2), torch.zeros(B * RA, device="cuda")
    ok(lib().egr_concat_channels_ra(p(cu(a)), p(cu(b)), p(y), B * per, C1, C2, B, p(ra), st()), "egr_concat_channels_ra")
    got = host(y)
    want = N.concat(a, b)
    assert (np.abs(want).reshape(B, -1).argmax(axis=1) == (per - 1) * (C1 + C2) + c).all()
    _check_rows(got, bits_differ(got, want), ra, B, lap, f"concat {B}x{per}x({C1}+{C2})")


@pytest.mark.parametrize("B,HW,Cc,G,silu", [(BIG_B, 355, 8, 2, 1), (65535, 3, 4, 1, 0)])
def test_groupnorm_rows_and_maxima_past_the_row_lap(pack, B, HW, Cc, G, silu):
    lap = LAPS["egr_groupnorm_nhwc_ra"][0]                                       # quads: 710 a row at the first shape
    r = rng_for(10 + HW)
    x = r.standard_normal((B, HW, Cc)).astype(F32) * _row_scales(B)[:, None, None]
    pos = (300 + np.arange(B) % 50) if HW > 256 else np.arange(B) % HW           # quad >= 512 = 256 x min_items (2)
    ch = np.arange(B) % Cc
    x[np.arange(B), pos, ch] = 12 * _row_scales(B)
    ga, be = r.uniform(0.9, 1.1, Cc).astype(F32), (0.1 * r.standard_normal(Cc)).astype(F32)
    y, ra = nan_like(B, HW, Cc), torch.zeros(B * RA, device="cuda")
    L = lib()
    ws = torch.empty(int(L.egr_groupnorm_workspace_bytes(B, Cc, G)), dtype=torch.uint8, device="cuda")
    ok(L.egr_groupnorm_nhwc_ra(p(cu(x)), p(cu(ga)), p(cu(be)), p(y), B, HW, Cc, G, 1e-6, silu, p(ws), p(ra), st()), "egr_groupnorm_nhwc_ra")
    got = host(y)
    want = N.groupnorm64(x, ga, be, G, 1e-6, bool(silu))
    if HW > 256:
        assert (np.abs(want).reshape(B, -1).argmax(axis=1) == pos * Cc + ch).all() and (pos * Cc // 4 >= 512).all()
    bad = over_bound(got, want, 3e-5).reshape(B, -1, 4).any(axis=2)
    _check_rows(got, bad, ra, B, lap, f"groupnorm {B}x{HW}x{Cc} (quads)")


def test_layernorm_rows_ra_past_the_row_lap(pack):
    """16384 batch rows of 11 token rows: one workgroup of 4 waves a batch row, laps of 4 + 4 + 3 rows; the largest |y| of a batch
    row comes from a one-hot row (|normalised| = sqrt(C - 1), the most a row of C can reach) in the third lap."""
    lap = LAPS["egr_layernorm_rows_ra"][0]
    B, per, Cc = 16384, 11, 5
    r = rng_for(11)
    x = r.standard_normal((B, per, Cc)).astype(F32) * _row_scales(B)[:, None, None]
    row = 8 + np.arange(B) % 3
    x[np.arange(B), row] = 0
    x[np.arange(B), row, 0] = 10
    ga, be = np.array([3, 1, -1, 1, 0.5], F32), np.array([0.2, 0, 0.1, -0.1, 0], F32)
    y, ra = nan_like(B, per, Cc), torch.zeros(B * RA, device="cuda")
    ok(lib().egr_layernorm_rows_ra(p(cu(x)), p(cu(ga)), p(cu(be)), p(y), B * per, Cc, 1e-5, B, p(ra), st()), "egr_layernorm_rows_ra")
    got = host(y)
    want = N.layernorm64(x, ga, be, 1e-5)
    assert (np.abs(want).reshape(B, -1).argmax(axis=1) == row * Cc).all()
    bad = over_bound(got, want, 3e-5).any(axis=2)
    _check_rows(got, bad, ra, B, lap, "layernorm_rows_ra 16384x11x5 (token rows)")


def test_layernorm_rows_past_the_lap(pack):
    """egr_layernorm_rows groups 64 x 2053 rows into 64 batch rows: 256 workgroups of 4 rows each, laps of 1024 rows."""
    rows, Cc, lap = 64 * 2053, 8, (16384 // 64) * LAPS["egr_layernorm_rows_ra"][0]
    assert 2053 > 2 * lap
    r = rng_for(12)
    x = (2 * r.standard_normal((rows, Cc)) + 0.3).astype(F32)
    ga, be = r.standard_normal(Cc).astype(F32), r.standard_normal(Cc).astype(F32)
    y = nan_like(rows, Cc)
    ok(lib().egr_layernorm_rows(p(cu(x)), p(cu(ga)), p(cu(be)), p(y), rows, Cc, 1e-5, st()), "egr_layernorm_rows")
    bad = over_bound(host(y), N.layernorm64(x, ga, be, 1e-5), 3e-5).any(axis=1)
    assert not bad.any(), where_bad(bad.reshape(64, 2053).any(axis=0), lap, "layernorm_rows 64x2053x8 (row inside a batch row)")


# ---------------------------------------------------------------- snake
def snake_case(B, Ln, Cc, K, period=None):
    """One egr_snake_aa_ra call against float64.  Batch rows repeat with `period` (a prime, so no power-of-two mix-up of rows goes
    unseen): the float64 reference of 8192 distinct rows would take a minute.  -> dict for the assertion (JSON-able)."""
    L = lib()
    from egregora_amd import flashsr_arch as A
    period = min(B, period or B)
    r = rng_for(1000 * K + 10 * Ln + Cc)
    base = (2 * r.standard_normal((period, Ln, Cc))).astype(F32)
    base *= (0.25 + np.arange(period) % 7 / 4.0).astype(F32)[:, None, None]
    al, be = (0.5 + 0.1 * r.standard_normal(Cc)).astype(F32), (-0.3 + 0.1 * r.standard_normal(Cc)).astype(F32)
    filt = A.kaiser_sinc_filter(K)
    x = np.ascontiguousarray(np.tile(base, ((B + period - 1) // period, 1, 1))[:B])
    y, ra = nan_like(B, Ln, Cc), torch.zeros(B * RA, device="cuda")
    ok(L.egr_snake_aa_ra(p(cu(x)), p(cu(al)), p(cu(be)), p(cu(filt)), p(y), B, Ln, Cc, K, p(ra), st()), "egr_snake_aa_ra")
    got = host(y)
    _KEEP.clear()
    want = N.snake64(base, al, be, filt)
    tol = 3e-5 * float(np.abs(want).max()) + 1e-6
    bad = np.zeros((Ln, Cc), bool)
    err = 0.0
    for b0 in range(0, B, period):
        g = got[b0:b0 + period]
        d = np.abs(g.astype(F64) - want[:len(g)])
        bad |= ~(d <= tol).all(axis=0)
        err = max(err, float(np.nanmax(d)))
    nruns = (Ln + 15) // 16                                                        # items of the K = 12 kernels: (run of 16, channel)
    m = np.zeros((nruns * 16, Cc), bool)
    m[:Ln] = bad
    msg = where_bad(m.reshape(nruns, 16, Cc).any(axis=1), LAPS["egr_snake_aa_ra"][0], f"snake B={B} L={Ln} C={Cc} K={K} ((run, channel) of a row)")
    return dict(nan=bool(np.isnan(got).any()), nbad=int(bad.sum()), err=err, tol=tol, msg=msg, amax_bad=int(amax_differs(ra, got, B).sum()))


def _snake_ok(res):
    assert not res["nan"] and res["nbad"] == 0 and res["amax_bad"] == 0, res


SNAKE_BIG = (BIG_B, 1123, 8, 12, 257)        # 71 runs x 8 channels = 568 items on one workgroup (9 spans x 8 in the default kernel)
SNAKE_TILED = [(2, Ln, Cc, 12, None) for Cc in (16, 32, 64) for Ln in (1, 5, 300)] + [(3, 129, 48, 12, None), (2, 257, 70, 12, None)]


def test_snake_k12_default_kernel_one_workgroup_per_row(pack):
    _snake_ok(snake_case(*SNAKE_BIG))


@pytest.mark.parametrize("K", [8, 32])
@pytest.mark.parametrize("Ln", [1, 3, 4, 5, 257])
def test_snake_generic_kernel(pack, K, Ln):
    _snake_ok(snake_case(2, Ln, 70, K))


def _child(tmp, tag, env_add, cases):
    env = dict(os.environ, **env_add)
    for k in ("EGR_SNAKE", "EGR_SNAKE_SPAN", "EGR_SNAKE_WG"):
        if k not in env_add:
            env.pop(k, None)
    path = tmp / (tag + ".json")
    args = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [__file__, str(path), json.dumps(cases)]
    r = subprocess.run(args, env=env, cwd=str(ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(path.read_text(encoding="utf-8"))


@pytest.mark.parametrize("tag,env_add,cases", [("reg", {"EGR_SNAKE_SPAN": "0"}, [SNAKE_BIG, (2, 17, 4, 12, None)]),
                                               ("span1", {"EGR_SNAKE_SPAN": "1"}, [SNAKE_BIG]),
                                               ("tiled", {"EGR_SNAKE": "tiled"}, SNAKE_TILED)], ids=["reg", "span1", "tiled"])
def test_snake_kernels_behind_switches(pack, tmp_path, tag, env_add, cases):
    """k_snake_aa_reg (EGR_SNAKE_SPAN=0) and one-run spans (=1) walk 568 items on the row's one workgroup: two laps and a ragged third.
    EGR_SNAKE=tiled: the three k_snake_aa_tiled shapes (C 64 / 32 / 16-multiples) and, at C = 70, the generic kernel at K = 12."""
    for res in _child(tmp_path, tag, env_add, cases):
        _snake_ok(res)


# ================================================================ 3. branches of the GroupNorm statistics pass
GN_BRANCH = [("scalar_plain", 6, 3), ("scalar_plain", 8, 4), ("scalar_plain_cpg6", 24, 4), ("scalar_shuffle", 64, 32),
             ("scalar_shuffle_cpg1", 128, 128), ("scalar_shuffle_5_strides", 1280, 20), ("v4", 4, 1), ("v4_idle_threads", 24, 2),
             ("v4_256_quads", 1024, 64)]
GN_HW = [1, 15, 16, 17, 63, 64, 65, 4097, 32773]
GN_CASES = [(n, Cc, G, 77, 0) for n, Cc, G in GN_BRANCH] + [("v4_shape_off_alignment", 24, 2, 77, 1)] + \
           [(f"hw{hw}", Cc, G, hw, 0) for hw in GN_HW for Cc, G in ((6, 3), (64, 32), (24, 2))]


def _groupnorm_both(x_dev, x, ga, be, G, silu, want_ra):
    """-> (scale, shift) of egr_groupnorm_coeff and, where C % 4 == 0 and asked, (y, row_amax) of egr_groupnorm_nhwc_ra."""
    L = lib()
    B, HW, Cc = x.shape
    ws = torch.empty(int(L.egr_groupnorm_workspace_bytes(B, Cc, G)), dtype=torch.uint8, device="cuda")
    sc, sh = nan_like(B, Cc), nan_like(B, Cc)
    gd, bd = cu(ga), cu(be)
    ok(L.egr_groupnorm_coeff(p(x_dev), p(gd), p(bd), B, HW, Cc, G, 1e-6, p(ws), p(sc), p(sh), st()), "egr_groupnorm_coeff")
    out = [host(sc), host(sh), None, None]
    if want_ra:
        y, ra = nan_like(B, HW, Cc), torch.zeros(B * RA, device="cuda")
        ok(L.egr_groupnorm_nhwc_ra(p(x_dev), p(gd), p(bd), p(y), B, HW, Cc, G, 1e-6, silu, p(ws), p(ra), st()), "egr_groupnorm_nhwc_ra")
        out[2], out[3] = host(y), ra
    return out


@pytest.mark.parametrize("name,Cc,G,HW,off", GN_CASES, ids=[f"{c[0]}_c{c[1]}_g{c[2]}_hw{c[3]}" for c in GN_CASES])
def test_groupnorm_statistics_branches(pack, name, Cc, G, HW, off):
    """The scalar statistics kernel (plain and wave-shuffle), the float4 one (idle threads, 256 quads) and an x off 16-byte alignment,
    over the slab rules' edges in HW: scale / shift and x scale + shift against float64 at the GroupNorm bound."""
    B = 2
    r = rng_for(Cc * 1000 + HW)
    x = (3 * r.standard_normal((B, HW, Cc)) + 1.5).astype(F32)
    x[1] *= F32(0.1)
    ga, be = r.standard_normal(Cc).astype(F32), r.standard_normal(Cc).astype(F32)
    if off:
        buf = torch.zeros(x.size + 4, device="cuda")
        buf[1:1 + x.size] = cu(x).reshape(-1)
        xd = buf[1:1 + x.size]
        assert xd.data_ptr() % 16 == 4
    else:
        xd = cu(x)
    sc, sh, y, ra = _groupnorm_both(xd, x, ga, be, G, 1, Cc % 4 == 0 and not off)
    wsc, wsh = N.gn_coeff64(x, ga, be, G, 1e-6)
    if HW * (Cc // G) > 1:                       # (one element a group: var = 0 and the coefficients are 1e3 gamma: y itself is the check)
        assert not over_bound(sc, wsc, 3e-5).any() and not over_bound(sh, wsh, 3e-5).any(), (name, np.abs(sc - wsc).max(), np.abs(sh - wsh).max())
    want = N.groupnorm64(x, ga, be, G, 1e-6)
    bad = over_bound(x.astype(F64) * sc[:, None].astype(F64) + sh[:, None].astype(F64), want, 3e-5)
    assert not bad.any(), where_bad(bad[0] | bad[1], HW * Cc, f"groupnorm_coeff {name} C={Cc} G={G} HW={HW}")
    if y is not None:
        bad = over_bound(y, N.silu64(want), 3e-5)
        assert not np.isnan(y).any() and not bad.any(), where_bad(bad[0] | bad[1], HW * Cc, f"groupnorm_nhwc_ra {name} C={Cc} G={G} HW={HW}")
        assert not amax_differs(ra, y, B).any()


def test_groupnorm_with_a_mean_ten_times_the_deviation(pack):
    """x = 10 + N(0, 1): E[x^2] - mean^2 loses two digits, so float32 per-thread partial sums show here first.  Bar: 4 x the error of
    the restatement that sums in double (tests/nn_refs.py groupnorm32)."""
    B, HW, Cc, G = 2, 4097, 256, 8
    r = rng_for(13)
    x = (10 + r.standard_normal((B, HW, Cc))).astype(F32)
    ga, be = r.uniform(0.5, 1.5, Cc).astype(F32), (0.1 * r.standard_normal(Cc)).astype(F32)
    sc, sh, y, ra = _groupnorm_both(cu(x), x, ga, be, G, 0, True)
    want, rest = N.groupnorm64(x, ga, be, G, 1e-6), N.groupnorm32(x, ga, be, G, 1e-6)
    bad = over_4x(y, rest, want, "groupnorm mean = 10 sigma")
    assert not bad.any(), where_bad(bad[0] | bad[1], HW * Cc, "groupnorm mean = 10 sigma")
    assert not amax_differs(ra, y, B).any()


# ================================================================ 4. width edges
@pytest.mark.parametrize("cols", [1, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097])
def test_softmax_around_the_kernel_widths(pack, cols):
    r = rng_for(cols)
    s = (6 * r.standard_normal((9, cols))).astype(F32)
    s[3] = np.where(r.random(cols) < 0.5, 80, -80)
    s[4] = -80
    s[4, cols // 2] = 80
    s[5, 1::3] = -np.inf
    s[6] = 0.37
    s[7] = -np.inf
    s[7, cols - 1] = 2.5                            # one finite entry, the last
    d = cu(s)
    ok(lib().egr_softmax_rows(p(d), 9, cols, st()), "egr_softmax_rows")
    got, want = host(d), N.softmax64(s)
    bad = over_bound(got, want, 2e-5)
    assert not bad.any(), where_bad(bad.any(axis=0), 256, f"softmax cols={cols} (column)")
    assert np.abs(got.astype(F64).sum(axis=1) - 1).max() <= 1e-5 and (got[5, 1::3] == 0).all()


@pytest.mark.parametrize("Cc", [1, 3, 63, 64, 65, 1000])
def test_layernorm_around_one_wave(pack, Cc):
    r = rng_for(Cc)
    x = (2 * r.standard_normal((13, Cc)) + 0.3).astype(F32)
    ga, be = r.standard_normal(Cc).astype(F32), r.standard_normal(Cc).astype(F32)
    y = nan_like(13, Cc)
    ok(lib().egr_layernorm_rows(p(cu(x)), p(cu(ga)), p(cu(be)), p(y), 13, Cc, 1e-5, st()), "egr_layernorm_rows")
    bad = over_bound(host(y), N.layernorm64(x, ga, be, 1e-5), 3e-5)
    assert not bad.any(), where_bad(bad.any(axis=0), 64, f"layernorm C={Cc} (channel)")


@pytest.mark.parametrize("batch,R_,Cc", [(3, 33, 95), (2, 1, 64), (1, 100, 1)])
def test_transpose_ragged_against_the_tile(pack, batch, R_, Cc):
    x = rng_for(R_).standard_normal((batch, R_, Cc)).astype(F32)
    y = nan_like(batch, Cc, R_)
    ok(lib().egr_transpose_batched(p(cu(x)), p(y), batch, R_, Cc, st()), "egr_transpose_batched")
    assert not bits_differ(host(y), N.transpose(x)).any()


def _stft(x, n_fft, hop, rpad, T, t_valid, ldm, win):
    B, Ln = x.shape
    mag = nan_like(B, T, ldm)
    rc = lib().egr_stft_frames(p(cu(x)), B, Ln, n_fft, hop, rpad, T, t_valid, ldm, p(cu(win)), p(mag), st())
    return rc, host(mag)


@pytest.mark.parametrize("name,n_fft,hop,Ln,rpad,T,t_valid", [("n4", 4, 1, 300, 1, 299, 290), ("n128_reflects_both_sides", 128, 30, 90, 30, 3, 2),
                                                              ("n128", 128, 30, 3840, 49, 128, 120), ("n2048", 2048, 480, 9000, 784, 20, 17),
                                                              ("n8192", 8192, 2048, 20000, 3072, 9, 7)])
def test_stft_frames_sizes_and_zero_fill(pack, name, n_fft, hop, Ln, rpad, T, t_valid):
    r = rng_for(n_fft + Ln)
    x = (0.3 * r.standard_normal((3, Ln))).astype(F32)
    win = torch.hann_window(n_fft, periodic=True).numpy() if n_fft > 4 else np.array([0.3, 1.0, 0.7, 0.2], F32)
    ldm = n_fft // 2 + 1 + 16
    idx = N.stft_index(Ln, n_fft, hop, rpad, T)
    if name == "n128_reflects_both_sides":
        i0 = np.arange(n_fft) - rpad
        assert i0[0] < 0 and i0[-1] > Ln - 1 and (idx[0] == np.where(i0 < 0, -i0, np.where(i0 > Ln - 1, 2 * (Ln - 1) - i0, i0))).all()
    rc, got = _stft(x, n_fft, hop, rpad, T, t_valid, ldm, win)
    ok(rc, "egr_stft_frames")
    assert not got[:, t_valid:].any() and not got[:, :, n_fft // 2 + 1:].any() and not np.isnan(got).any()
    want, rest = N.stft_mag(x, n_fft, hop, rpad, T, t_valid, ldm, win), N.stft_mag(x, n_fft, hop, rpad, T, t_valid, ldm, win, single=True)
    bad = over_4x(got, rest, want, f"stft_frames {name}")
    assert not bad.any(), where_bad(bad.any(axis=(0, 2)), T, f"stft_frames {name} (frames)")


def test_silent_row_through_the_cutoff(pack):
    """STFT frames -> cutoff: the cuts of oracle/flashsr_torch.lowpass_ref, 0 for the silent row (fc then clamps to 1 Hz)."""
    import math
    import types
    from oracle import flashsr_torch as R
    cfg = types.SimpleNamespace(n_fft=128, hop=30, sr=48000)
    Ln = 3840
    t = np.arange(Ln) / cfg.sr
    x = np.stack([sum(np.sin(2 * math.pi * f0 * t + i) / (i + 1) for i, f0 in enumerate((300.0, 1200.0, 2500.0, 5800.0))), np.zeros(Ln),
                  sum(np.sin(2 * math.pi * f0 * t + i) / (i + 1) for i, f0 in enumerate((200.0, 900.0, 2900.0)))])
    x = (0.3 * x / np.abs(x).max() + 1e-4 * rng_for(14).standard_normal(x.shape) * np.array([1, 0, 1])[:, None]).astype(F32)
    _, cuts = R.lowpass_ref(torch.from_numpy(x), cfg)
    rpad = (cfg.n_fft - cfg.hop) // 2
    T, nb, ldm, nbins = (Ln + 2 * rpad - cfg.n_fft) // cfg.hop + 1, 65, 80, Ln // 2 + 1
    mag = nan_like(3, T, ldm)
    win = torch.hann_window(cfg.n_fft, periodic=True).cuda()
    L = lib()
    ok(L.egr_stft_frames(p(cu(x)), 3, Ln, cfg.n_fft, cfg.hop, rpad, T, T, ldm, p(win), p(mag), st()), "egr_stft_frames")
    cut, gain = torch.full((3,), -1, dtype=torch.int32, device="cuda"), nan_like(3, nbins)
    ok(L.egr_lowpass_gain(p(mag), 3, T, ldm, nb, 0.985, float(cfg.sr), 8, 0.05, nbins, p(cut), p(gain), st()), "egr_lowpass_gain")
    assert host(cut).tolist() == cuts and cuts[1] == 0 and 0 < cuts[2] < cuts[0]
    assert not host(mag)[1].any()
    want, rest = N.cheby_gain64(cuts, nb, cfg.sr, 8, 0.05, nbins), N.cheby_gain32(cuts, nb, cfg.sr, 8, 0.05, nbins)
    assert not over_4x(host(gain), rest, want, "cheby_gain after a silent row").any()


@pytest.mark.parametrize("name,op", [("silu", N.EW_SILU), ("copy", N.EW_COPY)])
def test_eltwise_silu_and_copy_and_empty(pack, name, op):
    n, lap = 1000003, 977 * 256                                                # odd: one batch row of 977 workgroups (4 items a thread)
    a = (3 * rng_for(15).standard_normal(n)).astype(F32)
    y = nan_like(n)
    ok(lib().egr_eltwise(p(cu(a)), None, p(y), n, op, 0.0, 0.0, st()), "egr_eltwise")
    got = host(y)
    bad = bits_differ(got, a) if op == N.EW_COPY else over_bound(got, N.eltwise64(a, None, op), 2e-5)
    assert not bad.any(), where_bad(bad, lap, f"eltwise {name}")
    y = torch.full((8,), 7.0, device="cuda")
    ok(lib().egr_eltwise(p(y), None, p(y), 0, op, 0.0, 0.0, st()), "egr_eltwise n=0")
    assert (host(y) == 7.0).all()


# ================================================================ 5. refusals: an error code, and nothing launches
def _refused(rc, *outs):
    torch.cuda.synchronize()
    assert rc != 0
    for o in outs:
        assert (host(o) == 7.0).all()


def test_refusals_return_the_error_and_launch_nothing(pack):
    L = lib()
    seven = lambda *s: torch.full(s, 7.0, device="cuda")
    BB = 65536
    a, y, ra = torch.zeros(BB, 4, device="cuda"), seven(BB, 4), seven(BB * RA)
    g4 = torch.ones(4, device="cuda")
    # batch_rows = 65536: past the grid's y limit
    _refused(L.egr_eltwise_ra(p(a), p(a), p(y), BB * 4, N.EW_ADD, 0.0, 0.0, BB, p(ra), st()), y, ra)
    _refused(L.egr_geglu_ra(p(a), p(y), BB, 2, BB, p(ra), st()), y, ra)
    _refused(L.egr_concat_channels_ra(p(a), p(a), p(y), BB, 2, 2, BB, p(ra), st()), y, ra)
    _refused(L.egr_layernorm_rows_ra(p(a), p(g4), p(g4), p(y), BB, 4, 1e-5, BB, p(ra), st()), y, ra)
    ws = torch.empty(int(L.egr_groupnorm_workspace_bytes(BB, 4, 1)), dtype=torch.uint8, device="cuda")
    _refused(L.egr_groupnorm_nhwc_ra(p(a), p(g4), p(g4), p(y), BB, 1, 4, 1, 1e-6, 0, p(ws), p(ra), st()), y, ra)
    # n % batch_rows != 0
    _refused(L.egr_eltwise_ra(p(a), p(a), p(y), 1000, N.EW_ADD, 0.0, 0.0, 7, p(ra), st()), y, ra)
    _refused(L.egr_geglu_ra(p(a), p(y), 1000, 2, 7, p(ra), st()), y, ra)
    _refused(L.egr_concat_channels_ra(p(a), p(a), p(y), 1000, 2, 2, 7, p(ra), st()), y, ra)
    _refused(L.egr_layernorm_rows_ra(p(a), p(g4), p(g4), p(y), 1000, 4, 1e-5, 7, p(ra), st()), y, ra)
    # the one-input-channel convolution: Cout / 4 must divide 256; y on 16 bytes
    x, w, yc = torch.zeros(2, 8, 8, device="cuda"), torch.zeros(16, 16, device="cuda"), seven(2 * 8 * 8 * 16 + 4)
    _refused(L.egr_conv_cin1(p(x), p(w), None, p(yc), 2, 8, 8, 12, 3, 3, 1, 1, st()), yc)
    _refused(L.egr_conv_cin1(p(x), p(w), None, C.c_void_p(yc.data_ptr() + 4), 2, 8, 8, 16, 3, 3, 1, 1, st()), yc)
    # snake: odd K, K past the 32 filter slots
    xs, ys, f = torch.zeros(2, 20, 8, device="cuda"), seven(2, 20, 8), torch.zeros(40, device="cuda")
    al = torch.zeros(8, device="cuda")
    for K in (13, 34):
        _refused(L.egr_snake_aa_ra(p(xs), p(al), p(al), p(f), p(ys), 2, 20, 8, K, p(ra), st()), ys, ra)
    # STFT: reflect padding as long as the row
    xr, win, mag = torch.zeros(2, 50, device="cuda"), torch.ones(64, device="cuda"), seven(2, 3, 48)
    _refused(L.egr_stft_frames(p(xr), 2, 50, 64, 16, 50, 3, 3, 48, p(win), p(mag), st()), mag)


def test_stft_n_fft_6_is_refused_or_right(pack):
    """n_fft = 6 passes the launcher's own checks; the tables may refuse it (then nothing launches) or serve it (then it is held like
    every other size)."""
    r = rng_for(16)
    x, win = (0.3 * r.standard_normal((2, 40))).astype(F32), r.uniform(0.2, 1, 6).astype(F32)
    B, T, ldm = 2, 30, 20
    mag = torch.full((B, T, ldm), 7.0, device="cuda")
    rc = lib().egr_stft_frames(p(cu(x)), B, 40, 6, 1, 2, T, T - 3, ldm, p(cu(win)), p(mag), st())
    torch.cuda.synchronize()
    if rc != 0:
        assert (host(mag) == 7.0).all()
        return
    got = host(mag)
    want, rest = N.stft_mag(x, 6, 1, 2, T, T - 3, ldm, win), N.stft_mag(x, 6, 1, 2, T, T - 3, ldm, win, single=True)
    assert not got[:, T - 3:].any() and not got[:, :, 4:].any()
    assert not over_4x(got, rest, want, "stft_frames n6").any()


if __name__ == "__main__":
    results = [snake_case(*c) for c in json.loads(sys.argv[2])]
    torch.cuda.synchronize()
    Path(sys.argv[1]).write_text(json.dumps(results), encoding="utf-8")
