"""The band-walking F(4x4,3x3) input transform (k_wino4_in_band) and the span-walking anti-aliased snake (k_snake_aa_span) read each
halo element once and carry it in registers; they must produce the bits of the kernels they replace (k_wino4_in, k_snake_aa_reg<16>,
still compiled: EGR_W4_BAND=0 / EGR_SNAKE_SPAN=0), for the tensor and for the row maxima.

The switches are read once per process, so each side runs in a fresh child process (this file, run as a script): one with both
switches at 0 (the replaced kernels), one with EGR_W4_BAND=4 / EGR_SNAKE_SPAN=4 (band height and span forced, so that shapes of a
few tiles / a few runs walk several tiles and runs per thread).  The test process itself runs the default choice, which at these
sizes picks short bands and spans.  All three must agree bit for bit; the Winograd V is also held to a float64 B^T d B at the
1e-5-of-the-maximum tolerance of tests/test_gpu_flashsr.py::test_winograd4_error_vs_float64.

Shapes (band height 4, span 4 runs of 16 = 64 outputs in the forced child):
  Winograd  4x4 (one tile, all four edges), 8x8, 12x20 (interior and edge tiles, 5 tile columns in a tx span of 8), 24x12 (6 tile rows:
            one whole band and a ragged one), 8x68 at C = 64 (17 tile columns: a full tx span of 16 and one more workgroup column),
            C = 16 and C = 20 (4 and 5 channel quads), B = 3 with rows of different scale (nothing carried across an image boundary).
  snake     L = 1, 5, 15, 16, 17 (both clamped ends inside one run, a ragged run), 64 (one span), 65, 195 (three spans + 3)."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
RA = 32          # include/egregora_amd.h EGR_ROW_AMAX_STRIDE

WINO_SHAPES = [(2, 4, 4, 16), (2, 8, 8, 16), (2, 8, 8, 20), (2, 12, 20, 16), (2, 12, 20, 20), (2, 24, 12, 20), (1, 8, 68, 64),
               (3, 24, 8, 16)]
WINO_MODES = [("plain", False, 0), ("gn", True, 0), ("gn_silu", True, 1)]
SNAKE_SPAN = 4 * 16
SNAKE_SHAPES = [(2, L, Cc) for Cc in (4, 32) for L in (1, 5, 15, 16, 17, SNAKE_SPAN, SNAKE_SPAN + 1, 3 * SNAKE_SPAN + 3)]


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def wino_inputs(B, H, W, Cc, gn):
    g = torch.Generator().manual_seed(1000 * H + 10 * W + Cc + B)
    x = torch.randn(B, H, W, Cc, generator=g) * (10.0 ** -torch.arange(B).float()).view(B, 1, 1, 1)      # distinct rows
    sc = 1.0 + 0.1 * torch.randn(B, Cc, generator=g) if gn else None
    sh = 0.1 * torch.randn(B, Cc, generator=g) if gn else None
    return x, sc, sh


def snake_inputs(B, L, Cc):
    g = torch.Generator().manual_seed(100 * L + Cc)
    x = 2.0 * torch.randn(B, L, Cc, generator=g)
    al = 0.5 + 0.1 * torch.randn(Cc, generator=g)
    be = -0.3 + 0.1 * torch.randn(Cc, generator=g)
    return x, al, be


def compute_all():
    """{case name: array} of every case through the public entry points, with whatever kernels this process's environment selects."""
    sys.path.insert(0, str(ROOT))
    from packload import load_pack
    load_pack()
    from egregora_amd import native, flashsr_arch as A
    L = native.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = {}
    for (B, H, W, Cc) in WINO_SHAPES:
        for name, gn, silu in WINO_MODES:
            x, sc, sh = wino_inputs(B, H, W, Cc, gn)
            x, sc, sh = x.cuda(), (sc.cuda() if gn else None), (sh.cuda() if gn else None)
            P = B * (H // 4) * (W // 4)
            V1 = torch.full((36, P, Cc), float("nan"), device="cuda")
            V2 = torch.full((36, P, Cc), float("nan"), device="cuda")
            ra = torch.zeros(B * RA, device="cuda")
            native.check(L.egr_winograd4_input(p(x), p(sc), p(sh), silu, B, H, W, Cc, p(V1), st), "wino4_in")
            native.check(L.egr_winograd4_input_ra(p(x), p(sc), p(sh), silu, B, H, W, Cc, p(V2), p(ra), st), "wino4_in_ra")
            key = "w_%d_%d_%d_%d_%s" % (B, H, W, Cc, name)
            out[key + "_V"], out[key + "_Vra"], out[key + "_ra"] = V1.cpu().numpy(), V2.cpu().numpy(), ra.cpu().numpy()
    filt = torch.from_numpy(A.kaiser_sinc_filter(12)).float().cuda()
    for (B, Ln, Cc) in SNAKE_SHAPES:
        x, al, be = (t.cuda() for t in snake_inputs(B, Ln, Cc))
        y = torch.full((B, Ln, Cc), float("nan"), device="cuda")
        ra = torch.zeros(B * RA, device="cuda")
        native.check(L.egr_snake_aa_ra(p(x), p(al), p(be), p(filt), p(y), B, Ln, Cc, 12, p(ra), st), "snake_ra")
        key = "s_%d_%d_%d" % (B, Ln, Cc)
        out[key + "_y"], out[key + "_ra"] = y.cpu().numpy(), ra.cpu().numpy()
    torch.cuda.synchronize()
    return out


def _child(tmp, tag, band, span):
    env = dict(os.environ, EGR_W4_BAND=band, EGR_SNAKE_SPAN=span)
    env.pop("EGR_SNAKE", None)
    path = tmp / (tag + ".npz")
    args = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [__file__, str(path)]
    r = subprocess.run(args, env=env, cwd=str(ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return dict(np.load(path))


@pytest.fixture(scope="module")
def sides(pack, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("halo_once")
    return {"old": _child(tmp, "old", "0", "0"), "forced": _child(tmp, "forced", "4", "4"), "default": compute_all()}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("side", ["forced", "default"])
def test_winograd_input_bits_and_row_maxima_equal_the_replaced_kernel(sides, side):
    old, new = sides["old"], sides[side]
    for (B, H, W, Cc) in WINO_SHAPES:
        for name, _, _ in WINO_MODES:
            key = "w_%d_%d_%d_%d_%s" % (B, H, W, Cc, name)
            assert not np.isnan(old[key + "_V"]).any(), key
            for k in ("_V", "_Vra", "_ra"):
                assert np.array_equal(bits(old[key + k]), bits(new[key + k])), (side, key + k)
            assert np.array_equal(bits(new[key + "_V"]), bits(new[key + "_Vra"])), (side, key)
            want = np.abs(new[key + "_V"]).reshape(36, B, -1).max(axis=(0, 2))
            assert np.array_equal(new[key + "_ra"][::RA], want), (side, key)


def _bt():
    a, b = 0.75, 1.5
    c0, c2 = a * a * b * b, -(a * a + b * b)
    return torch.tensor([[c0, 0, c2, 0, 1, 0], [0, -a * b * b, -b * b, a, 1, 0], [0, a * b * b, -b * b, -a, 1, 0],
                         [0, -b * a * a, -a * a, b, 1, 0], [0, b * a * a, -a * a, -b, 1, 0], [0, c0, 0, c2, 0, 1]], dtype=torch.float64)


@pytest.mark.parametrize("side", ["old", "forced", "default"])
def test_winograd_input_against_float64(sides, side):
    """V = B^T d B of the zero-padded (affine, SiLU) input in float64; max error <= 1e-5 of max |V|."""
    BT = _bt()
    for (B, H, W, Cc) in WINO_SHAPES:
        for name, gn, silu in WINO_MODES:
            x, sc, sh = wino_inputs(B, H, W, Cc, gn)
            v = x.double()
            if gn:
                v = v * sc.double().view(B, 1, 1, Cc) + sh.double().view(B, 1, 1, Cc)
            if silu:
                v = v * torch.sigmoid(v)
            xp = torch.zeros(B, H + 2, W + 2, Cc, dtype=torch.float64)
            xp[:, 1:-1, 1:-1] = v
            d = xp.unfold(1, 6, 4).unfold(2, 6, 4)                                # [B][TH][TW][C][r][q]
            ref = torch.einsum("ir,btxcrq,jq->ijbtxc", BT, d, BT).reshape(36, -1, Cc)
            got = torch.from_numpy(sides[side]["w_%d_%d_%d_%d_%s_V" % (B, H, W, Cc, name)]).double()
            err = float((got - ref).abs().max() / ref.abs().max())
            assert err <= 1e-5, (side, B, H, W, Cc, name, err)


@pytest.mark.parametrize("side", ["forced", "default"])
def test_snake_bits_and_row_maxima_equal_the_replaced_kernel(sides, side):
    old, new = sides["old"], sides[side]
    for (B, Ln, Cc) in SNAKE_SHAPES:
        key = "s_%d_%d_%d" % (B, Ln, Cc)
        assert not np.isnan(old[key + "_y"]).any(), key
        assert np.array_equal(bits(old[key + "_y"]), bits(new[key + "_y"])), (side, key)
        assert np.array_equal(bits(old[key + "_ra"]), bits(new[key + "_ra"])), (side, key)
        assert np.array_equal(new[key + "_ra"][::RA], np.abs(new[key + "_y"]).max(axis=(1, 2))), (side, key)


if __name__ == "__main__":
    np.savez(sys.argv[1], **compute_all())
