"""What the convolution launcher RAN is what its host-only query says it runs: for the shapes of tests/test_conv_choice.py, launched
through the C ABI, the calling thread's last-kernel name (egr_conv_last_kernel) equals egr_conv_kernel_name's answer for the same
description and the name written out there, and y matches a float64 convolution within the gates the operand schemes are already
held to -- the f32-MFMA kernel at max|diff| <= 2e-5 max|ref| + 1e-6 (tests/test_gpu_flashsr.py), the bf16- and fp16-term kernels at
maximum and rms error <= 1.25x the f32-MFMA kernel's on the same operands (+ 1e-8) and a maximum error < 2e-6 of max|ref|
(test_split3_conv_error_vs_float64, tests/test_gpu_split_h2.py).

Sizes: most shapes move a few MB (the input-stationary 3x3 ones 8 MB).  Four are large because the rule they exercise only bites at
a large row count -- the 256-row tile needs 1024 tiles of 256 x 128 (s3_bm256, h2_never_bm256: 262144 rows, about 200 MB each) and
z-streaming needs 114 row tiles (the two *_stack_streamed: about 300 MB); each still runs in about a second.  s3_bn256 and h2_bn256
(65536 rows x 512 channels) are left to the host-only test: their 3x3 siblings reach the same 128 x 256 instantiations at 6.5 MB."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from test_conv_choice import CASES

pytestmark = pytest.mark.gpu

RA = 32          # include/egregora_amd.h EGR_ROW_AMAX_STRIDE
KEYS = ["igemm_c32", "igemm_c33", "igemm_c128", "igemm_cin3", "igemm_gn", "igemm_splitk", "s3_bn256_3x3", "h2_bn256_3x3", "s3_narrow_64",
        "s3_narrow_128", "s3_not_narrow", "s3_bm256", "h2_never_bm256", "s3_stack_one_tile", "s3_stack_bias", "s3_stack_streamed",
        "h2_stack_streamed", "s3_splitk", "c1d", "c1d_cin32_h2", "c1d_w64", "c1d_h2_rows64", "c3", "c3_gn_silu", "c3_gn", "c3_bf16", "c3_h62"]


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


@pytest.mark.parametrize("key", KEYS)
def test_the_launch_runs_the_kernel_the_query_names(pack, key):
    from egregora_amd import native
    from tools.flashsr_pydriver import PyDriverEngine
    L, st = native.lib(), native.stream_ptr()
    desc, (want_name, want_ksplit, want_nzb) = CASES[key]
    d = dict(dict(B=1, H=1, W=1, OH=1, OW=1, KH=1, KW=1, dil=1, pad_t=0, pad_l=0, nz=1, sch=0, gn_silu=0), **desc)
    B, H, W, Ci, OH, OW, Co, KH, KW, dil, pt, pl, nz = (d[k] for k in ("B", "H", "W", "Cin", "OH", "OW", "Cout", "KH", "KW", "dil", "pad_t", "pad_l", "nz"))
    g = torch.Generator().manual_seed(len(key) * 1000 + Ci)
    K = KH * KW * Ci
    x = torch.randn(nz, B, H, W, Ci, generator=g).cuda()
    w = (torch.randn(nz, Co, Ci, KH, KW, generator=g) / math.sqrt(K)).cuda()
    bias = torch.randn(Co, generator=g).cuda() if "bias" in d else None
    gn = "gn_scale" in d
    sc = (1.0 + 0.1 * torch.randn(B, Ci, generator=g)).cuda() if gn else None
    sh = (0.1 * torch.randn(B, Ci, generator=g)).cuda() if gn else None
    xin = x.double()
    if gn:                                      # the loader's transform: per (image, channel) affine, then SiLU
        xin = xin * sc.double().view(1, B, 1, 1, Ci) + sh.double().view(1, B, 1, 1, Ci)
        xin = F.silu(xin) if d["gn_silu"] else xin
    if KH == 1 and KW == 1:
        ref = torch.einsum("zbhwc,zoc->zbhwo", xin, w.double()[:, :, :, 0, 0]) + (0.0 if bias is None else bias.double())
    else:
        ref = torch.stack([F.conv2d(xin[z].permute(0, 3, 1, 2), w[z].double(), None if bias is None else bias.double(), padding=(pt, pl),
                                    dilation=(1, dil)).permute(0, 2, 3, 1) for z in range(nz)])
    assert ref.shape == (nz, B, OH, OW, Co)
    wp = torch.stack([PyDriverEngine.pack_matrix(w[z].permute(2, 3, 1, 0).reshape(K, Co).contiguous().cpu()) for z in range(nz)]).cuda().contiguous()
    ns = wp.shape[1]
    zf = ns * Co * 16                           # floats per z problem of the fp32 pack
    geo = (B, H, W, Ci, OH, OW, Co, KH, KW, 1, dil, pt, pl, 0, 0, 0.0)
    zx, zy = B * H * W * Ci, B * OH * OW * Co

    xm = xin.float().contiguous() if gn else x          # the transformed operand, materialised

    def f32_launch(y, fused):
        if fused:
            native.check(L.egr_conv_nhwc_gn(p(x), p(sc), p(sh), d["gn_silu"], p(wp), p(bias), p(None), p(y), B, H, W, Ci, OH, OW, Co, KH, KW, 1, pt, pl,
                                            0, st), "egr_conv_nhwc_gn")
        elif nz > 1 and bias is None:
            native.check(L.egr_gemm_zbatched(p(xm), p(wp), p(y), nz, B, Ci, Co, zx, zf, zy, st), "egr_gemm_zbatched")
        else:
            for z in range(nz):
                native.check(L.egr_conv_nhwc(p(xm[z]), p(wp[z]), p(bias), p(None), p(None), p(y[z]), *geo, st), "egr_conv_nhwc")

    y = torch.empty(nz, B, OH, OW, Co, device="cuda")
    q = dict(d, x=x.data_ptr(), y=y.data_ptr())
    for k_, t in (("bias", bias), ("gn_scale", sc), ("gn_shift", sh)):
        if t is not None:
            q[k_] = t.data_ptr()
    if "w3" not in d:
        q["w"] = wp.data_ptr()
        if nz > 1:
            q["zw"] = zf
        f32_launch(y, gn)
    else:
        terms = 2 if d["sch"] else 3
        w3 = torch.empty(nz * ns * terms * Co * 16, dtype=torch.float16 if d["sch"] else torch.bfloat16, device="cuda")
        q["w3"] = w3.data_ptr()
        assert nz == 1 or d["zw"] == zf * terms // 8
        if not d["sch"]:
            native.check(L.egr_split3_pack(p(wp), p(w3), nz * ns, Co, st), "egr_split3_pack")
            native.check(L.egr_conv_s3(p(x), p(w3), p(bias), p(None), p(None), p(y), *geo, 1, 1, 0, 0, OH, OW, nz, zx, zf * 3 // 8, zy, st), "egr_conv_s3")
        else:
            rows = d["batch_rows"]
            ws = 2.0 ** (13 - math.ceil(math.log2(float(wp.abs().max()))))
            native.check(L.egr_split2h_pack(p(wp), p(w3), nz * ns, Co, ws, st), "egr_split2h_pack")
            ra = torch.zeros(rows * RA, device="cuda")
            native.check(L.egr_absmax_rows(p(xm), rows, xm.numel() // (rows * nz), nz, zx, p(ra), st), "egr_absmax_rows")   # (GroupNorm: of the transformed operand)
            q.update(row_amax=ra.data_ptr(), w_scale=ws)
            if gn:
                native.check(L.egr_conv_h2_gn(p(x), p(sc), p(sh), d["gn_silu"], p(w3), p(bias), p(None), p(y), B, H, W, Ci, Co, 0, ws, p(ra), p(None),
                                              p(None), st), "egr_conv_h2_gn")
            else:
                native.check(L.egr_conv_h2(p(x), p(w3), p(bias), p(None), p(None), p(y), *geo, 1, 1, 0, 0, OH, OW, nz, zx, zf * 2 // 8, zy, ws, p(ra),
                                           rows, p(None), st), "egr_conv_h2")
    ran = native.last_conv_kernel()
    assert native.conv_kernel_name(**q) == (ran, want_ksplit, want_nzb) and ran == want_name
    mx = lambda t: float((t.double() - ref).abs().max() / ref.abs().max())
    rms = lambda t: float((t.double() - ref).norm() / ref.norm())
    if "w3" not in d:
        assert float((y.double() - ref).abs().max()) <= 2e-5 * float(ref.abs().max()) + 1e-6, mx(y)
    else:
        y1 = torch.empty_like(y)
        f32_launch(y1, False)                               # (fused GroupNorm: the f32-MFMA kernel on the materialised operand)
        print(f"{key}: {ran}  max {mx(y):.2e} (f32 MFMA {mx(y1):.2e})  rms {rms(y):.2e} ({rms(y1):.2e})")
        assert mx(y) <= 1.25 * mx(y1) + 1e-8 and rms(y) <= 1.25 * rms(y1) + 1e-8, (mx(y1), mx(y), rms(y1), rms(y))
        assert mx(y) < 2e-6, mx(y)
