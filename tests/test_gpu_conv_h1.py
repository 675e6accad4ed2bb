"""The one-term fp16 operand scheme at operator level (scheme 2 of csrc/egr_nn_gemm_s3.hip: egr_conv_h1 / egr_conv_h1_gn), held to
an EXACT model and not to a loose fp16 tolerance.

Rounded-operand model: x^[b] = f16_rne(x[b] s_b) / s_b with s_b = 2^(141 - e_b), e_b the biased fp32 exponent of max |x[b]| (clamped
to [15, 254] as h2_row_scale does); w^ = plane 0 of the egr_split2h_pack output / w_scale; ref^ = the float64 contraction of x^ and
w^ plus bias and residual (then the activation).  fp16 x fp16 products are exact in fp32, so only fp32 accumulation separates the
device from ref^ -- with fewer roundings than the two-term kernel makes.
  Bar A: max |y - ref^| / max |ref^| < 2e-6 (the absolute bar scheme 1 has against float64 in tests/test_gpu_split_h2.py).  A wrong
         plane, a missed scale or a dropped slab is an O(1) error.
  Bar B, against the float64 contraction `ref` of the UNROUNDED operands, elementwise:
         |y - ref| <= 2^-11 (1 + 2^-9) A + 2e-6 max |ref|,  A = the float64 contraction of |x| and |w|.
         (RNE to fp16's 11 significand bits leaves at most 2^-11 relative error per operand in the worst case and about 2^-12.4 rms;
         summed over K >= 48 products with signs of their own the error stays far inside the bar, which every test below first
         confirms for ref^ itself -- the model, no device code involved -- before it holds the device to it.)
Inputs are randn at one level per batch row: after the row's scale no element falls below fp16's normal range.
The fused-GroupNorm kernel normalises in fp32 with a 1-ulp reciprocal, so a few elements round to the other fp16 neighbour than a
float64 model's: bar B only there, with 2^-11 (1 + 2^-8) and A formed from the float64 normalised tensor."""
import math

import pytest
import torch
import torch.nn.functional as F

from test_gpu_split_h2 import RA, h2_pack, p, ra_zeros, row_amax

pytestmark = pytest.mark.gpu

U = 2.0 ** -11


@pytest.fixture(scope="module")
def eng(pack):
    from egregora_amd import flashsr_arch as A
    from tools.flashsr_pydriver import PyDriverEngine
    cfg = A.tiny_config()
    return PyDriverEngine(cfg, A.init_params(cfg, 0))


def row_scales(x, rows):
    """s_b of the model: 2^(141 - e_b) per batch row, float64, shaped to broadcast over x viewed as [rows][-1]."""
    amax = x.reshape(rows, -1).abs().amax(dim=1).float().contiguous()
    e = ((amax.view(torch.int32) >> 23) & 0xff).clamp(15, 254)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64, device=x.device), (141 - e).double())


def round_x(x, rows):
    """x^ in float64."""
    s = row_scales(x, rows).view(rows, 1)
    xs = (x.reshape(rows, -1).double() * s).float()                 # exact: a power of two, the scaled maximum below 2^15
    return (xs.half().double() / s).view(x.shape)


def plane0(w2, ns, Co, ws):
    """w^ as the packed matrix [ns][Co][16] in float64."""
    return w2.view(ns, 2, Co, 16)[:, 0].double() / ws


def unpack_conv(wp, kh, kw, Ci, Co):
    """packed [ns][Co][16] (k = 16 s + j, ordered (ky, kx, ci)) -> conv weight [Co][Ci][kh][kw]"""
    K = kh * kw * Ci
    return wp.permute(0, 2, 1).reshape(-1, Co)[:K].view(kh, kw, Ci, Co).permute(3, 2, 0, 1).contiguous()


def conv64(x, w, pad, dil=(1, 1)):
    return F.conv2d(x.permute(0, 3, 1, 2), w, None, padding=pad, dilation=dil).permute(0, 2, 3, 1)


def check_bars(tag, y, ref_hat, ref, A, k_b=1.0 + 2.0 ** -9, bar_a=True):
    y = y.double()
    tol = U * k_b * A + 2e-6 * float(ref.abs().max())
    model_b = float(((ref_hat - ref).abs() / tol).max())
    dev_b = float(((y - ref).abs() / tol).max())
    dev_a = float((y - ref_hat).abs().max() / ref_hat.abs().max())
    print(f"{tag}: bar A {dev_a:.2e} (< 2e-6){'' if bar_a else ' [not applied]'}; bar B: device at {dev_b:.3f} of the bound, the model itself at {model_b:.3f}")
    assert model_b <= 1.0, (tag, "the rounded-operand model itself misses bar B", model_b)
    assert dev_b <= 1.0, (tag, dev_b)
    if bar_a:
        assert dev_a < 2e-6, (tag, dev_a)
    return dev_a, dev_b


def launched_name_ok(native, desc):
    last = native.last_conv_kernel()
    assert last == native.conv_kernel_name(**desc)[0] and last.endswith(", 2>"), (last, native.conv_kernel_name(**desc))
    return last


IGEMM = [(2, 16, 12, 128, 128, 3, 0, False), (1, 9, 7, 256, 96, 3, 0, False), (9, 128, 128, 32, 128, 3, 0, False), (2, 8, 4, 640, 640, 3, 0, False),
         (1, 24, 16, 64, 512, 3, 0, False), (2, 6, 6, 32, 30, 3, 0, False), (2, 8, 8, 48, 256, 1, 0, False),
         (2, 16, 12, 128, 128, 3, 1, True)]            # the last: residual and SiLU


@pytest.mark.parametrize("case", IGEMM, ids=lambda c: "x".join(str(v) for v in c))
def test_h1_conv_equals_the_rounded_operand_model(eng, case):
    from egregora_amd import native
    e, L = eng, eng.L
    B, H, W, Ci, Co, k, act, res_on = case
    g = torch.Generator().manual_seed(178)
    x = (torch.randn(B, H, W, Ci, generator=g) * (10.0 ** -torch.arange(B).float()).view(B, 1, 1, 1)).cuda()     # one level per batch row
    w = (torch.randn(Co, Ci, k, k, generator=g) / math.sqrt(Ci * k * k)).cuda()
    b = (0.1 * torch.randn(Co, generator=g)).cuda()
    r = (0.1 * torch.randn(B, H, W, Co, generator=g)).cuda() if res_on else None
    wp = e.pack_matrix(w.permute(2, 3, 1, 0).reshape(k * k * Ci, Co).contiguous()).cuda()
    ns = wp.shape[0]
    w2, ws = h2_pack(e, wp, Co)
    post = (lambda v: v * torch.sigmoid(v)) if act == 1 else (lambda v: v)
    extra = b.double() + (r.double() if res_on else 0.0)
    ref = post(conv64(x.double(), w.double(), k // 2) + extra)
    ref_hat = post(conv64(round_x(x, B), unpack_conv(plane0(w2, ns, Co, ws), k, k, Ci, Co), k // 2) + extra)
    A = conv64(x.double().abs(), w.double().abs(), k // 2)
    y = torch.full((B, H, W, Co), float("nan"), device="cuda")
    oa = ra_zeros(B)
    ra = row_amax(e, x, B)
    native.check(L.egr_conv_h1(p(x), p(w2), p(b), p(None), p(r), p(y), B, H, W, Ci, H, W, Co, k, k, 1, 1, k // 2, k // 2, 0, act, 0.0,
                               1, 1, 0, 0, H, W, 1, 0, 0, 0, ws, p(ra), B, p(oa), e._st()), "conv_h1")
    desc = dict(x=x.data_ptr(), y=y.data_ptr(), w3=w2.data_ptr(), bias=b.data_ptr(), res=r.data_ptr() if res_on else 0, B=B, H=H, W=W, OH=H, OW=W,
                Cin=Ci, Cout=Co, KH=k, KW=k, pad_t=k // 2, pad_l=k // 2, act=act, sch=2, w_scale=ws, row_amax=ra.data_ptr(), batch_rows=B,
                out_amax=oa.data_ptr())
    name = launched_name_ok(native, desc)
    for i in range(B):                               # per batch row: each at its own level (no looser than the bars over the whole tensor)
        check_bars(f"{case} {name} row {i}", y[i], ref_hat[i], ref[i], A[i])
    assert torch.equal(oa[::RA], y.abs().amax(dim=(1, 2, 3))), "out_amax is max |y| per batch row, exactly"


@pytest.mark.parametrize("case", [(3, 512, 64, 64, 7, 3), (2, 1024, 32, 32, 11, 1), (2, 256, 128, 128, 3, 5), (4, 384, 16, 32, 3, 1)],
                         ids=lambda c: "x".join(str(v) for v in c))
def test_h1_conv1d_equals_the_rounded_operand_model(eng, case):
    from egregora_amd import native
    e, L = eng, eng.L
    B, Wd, Ci, Co, k, dil = case
    g = torch.Generator().manual_seed(179)
    x = (torch.randn(B, 1, Wd, Ci, generator=g) * (10.0 ** -torch.arange(B).float()).view(B, 1, 1, 1)).cuda()
    w = (torch.randn(Co, Ci, 1, k, generator=g) / math.sqrt(Ci * k)).cuda()
    b = (0.1 * torch.randn(Co, generator=g)).cuda()
    wp = e.pack_matrix(w.permute(2, 3, 1, 0).reshape(k * Ci, Co).contiguous()).cuda()
    ns = wp.shape[0]
    w2, ws = h2_pack(e, wp, Co)
    pad = dil * (k - 1) // 2
    ref = conv64(x.double(), w.double(), (0, pad), (1, dil)) + b.double()
    ref_hat = conv64(round_x(x, B), unpack_conv(plane0(w2, ns, Co, ws), 1, k, Ci, Co), (0, pad), (1, dil)) + b.double()
    A = conv64(x.double().abs(), w.double().abs(), (0, pad), (1, dil))
    y = torch.full((B, 1, Wd, Co), float("nan"), device="cuda")
    oa = ra_zeros(B)
    ra = row_amax(e, x, B)
    native.check(L.egr_conv_h1(p(x), p(w2), p(b), p(None), p(None), p(y), B, 1, Wd, Ci, 1, Wd, Co, 1, k, 1, dil, 0, pad, 0, 0, 0.0, 1, 1, 0, 0,
                               1, Wd, 1, 0, 0, 0, ws, p(ra), B, p(oa), e._st()), "conv_h1")
    desc = dict(x=x.data_ptr(), y=y.data_ptr(), w3=w2.data_ptr(), bias=b.data_ptr(), B=B, W=Wd, OW=Wd, Cin=Ci, Cout=Co, KW=k, dil=dil, pad_l=pad,
                sch=2, w_scale=ws, row_amax=ra.data_ptr(), batch_rows=B, out_amax=oa.data_ptr())
    name = launched_name_ok(native, desc)
    assert name.startswith("k_conv1d_s3<")
    for i in range(B):
        check_bars(f"{case} {name} row {i}", y[i], ref_hat[i], ref[i], A[i])
    assert torch.equal(oa[::RA], y.abs().amax(dim=(1, 2, 3)))


@pytest.mark.parametrize("case", [(36, 700, 128, 128, 7), (16, 500, 64, 128, 5)], ids=lambda c: "x".join(str(v) for v in c))
def test_h1_z_stacked_gemms_equal_the_rounded_operand_model(eng, case):
    """nz problems [P][Cin] x [Cin][Cout] in one launch; P is not a multiple of the 128-row tile and the batch rows sit at levels 1 .. 1e-4."""
    from egregora_amd import native
    e, L = eng, eng.L
    nz, P, Ci, Co, rows = case
    g = torch.Generator().manual_seed(180)
    x = torch.randn(nz, P, Ci, generator=g)
    lv = 10.0 ** torch.linspace(0, -4, rows)
    x = (x.view(nz, rows, P // rows, Ci) * lv.view(1, rows, 1, 1)).reshape(nz, P, Ci).cuda()
    w = (torch.randn(nz, Ci, Co, generator=g) / math.sqrt(Ci)).cuda()
    wp = torch.stack([e.pack_matrix(w[z].cpu()) for z in range(nz)]).cuda().contiguous()       # [nz][ns][Co][16]
    ns = wp.shape[1]
    w2, ws = h2_pack(e, wp.view(nz * ns, Co, 16), Co)
    zf = ns * Co * 16
    ra = row_amax(e, x, rows, nz, P * Ci)
    # the model: a batch row is the same P / rows tiles of every z problem, its maximum is taken over all of them
    xr = x.view(nz, rows, P // rows, Ci).permute(1, 0, 2, 3).contiguous()
    x_hat = round_x(xr, rows).permute(1, 0, 2, 3).reshape(nz, P, Ci)
    w_hat = plane0(w2, nz * ns, Co, ws).view(nz, ns, Co, 16).permute(0, 1, 3, 2).reshape(nz, ns * 16, Co)[:, :Ci]
    ref = torch.einsum("zpc,zcn->zpn", x.double(), w.double())
    ref_hat = torch.einsum("zpc,zcn->zpn", x_hat, w_hat)
    A = torch.einsum("zpc,zcn->zpn", x.double().abs(), w.double().abs())
    y = torch.full((nz, P, Co), float("nan"), device="cuda")
    native.check(L.egr_conv_h1(p(x), p(w2), p(None), p(None), p(None), p(y), P, 1, 1, Ci, 1, 1, Co, 1, 1, 1, 1, 0, 0, 0, 0, 0.0, 1, 1, 0, 0, 1, 1,
                               nz, P * Ci, zf * 2 // 8, P * Co, ws, p(ra), rows, p(None), e._st()), "conv_h1")
    desc = dict(x=x.data_ptr(), y=y.data_ptr(), w3=w2.data_ptr(), B=P, Cin=Ci, Cout=Co, nz=nz, zx=P * Ci, zw=zf * 2 // 8, zy=P * Co, sch=2, w_scale=ws,
                row_amax=ra.data_ptr(), batch_rows=rows)
    name = launched_name_ok(native, desc)
    per = P // rows
    for r in range(rows):                            # every batch row at its own level: the bars hold per row
        sl = slice(r * per, (r + 1) * per)
        check_bars(f"{case} row {r} {name}", y[:, sl], ref_hat[:, sl], ref[:, sl], A[:, sl])


def test_h1_streamed_z_stack_equals_the_per_problem_launches(eng):
    """The z-streamed instantiation (k_conv_s3<128, 128, 1, true, 2>: several z problems per workgroup) is picked from 4096 / nz row
    tiles per problem on: 36 problems of 14592 rows (two per workgroup), three of them against the model and, bit for bit, against
    one launch per problem."""
    from egregora_amd import native
    e, L = eng, eng.L
    nz, P, Ci, Co, rows = 36, 14592, 16, 128, 2
    g = torch.Generator().manual_seed(181)
    lv = torch.tensor([1.0, 1e-4])
    x = (torch.randn(nz, rows, P // rows, Ci, generator=g) * lv.view(1, rows, 1, 1)).reshape(nz, P, Ci).cuda()
    w = (torch.randn(nz, Ci, Co, generator=g) / math.sqrt(Ci)).cuda()
    wp = torch.stack([e.pack_matrix(w[z].cpu()) for z in range(nz)]).cuda().contiguous()
    ns = wp.shape[1]
    w2, ws = h2_pack(e, wp.view(nz * ns, Co, 16), Co)
    zf = ns * Co * 16
    ra = row_amax(e, x, rows, nz, P * Ci)
    y = torch.full((nz, P, Co), float("nan"), device="cuda")
    native.check(L.egr_conv_h1(p(x), p(w2), p(None), p(None), p(None), p(y), P, 1, 1, Ci, 1, 1, Co, 1, 1, 1, 1, 0, 0, 0, 0, 0.0, 1, 1, 0, 0, 1, 1,
                               nz, P * Ci, zf * 2 // 8, P * Co, ws, p(ra), rows, p(None), e._st()), "conv_h1")
    name = native.last_conv_kernel()
    assert name == "k_conv_s3<128, 128, 1, true, 2>", name
    assert bool(torch.isfinite(y).all())
    xr = x.view(nz, rows, P // rows, Ci).permute(1, 0, 2, 3).contiguous()
    x_hat = round_x(xr, rows).permute(1, 0, 2, 3).reshape(nz, P, Ci)
    w_hat = plane0(w2, nz * ns, Co, ws).view(nz, ns, Co, 16).permute(0, 1, 3, 2).reshape(nz, ns * 16, Co)[:, :Ci]
    per = P // rows
    y1 = torch.full((P, Co), float("nan"), device="cuda")
    for z in (0, 1, nz - 1):
        ref = x[z].double() @ w[z].double()
        ref_hat = x_hat[z] @ w_hat[z]
        A = x[z].double().abs() @ w[z].double().abs()
        for r in range(rows):
            sl = slice(r * per, (r + 1) * per)
            # K = 16 is too short a sum for the statistical bar above: here the worst-case bound of the format, 2^-11 per operand
            check_bars(f"streamed z {z} row {r}", y[z, sl], ref_hat[sl], ref[sl], A[sl], k_b=2.0 * (1.0 + 2.0 ** -9))
        # the problem alone (nz = 1) with the same row maxima: the same sums in the same order, the same bits
        native.check(L.egr_conv_h1(p(x[z]), p(w2.view(nz, -1)[z]), p(None), p(None), p(None), p(y1), P, 1, 1, Ci, 1, 1, Co, 1, 1, 1, 1, 0, 0, 0, 0, 0.0,
                                   1, 1, 0, 0, 1, 1, 1, 0, 0, 0, ws, p(ra), rows, p(None), e._st()), "conv_h1")
        assert torch.equal(y1, y[z]), z


def test_h1_rows_at_their_own_level(eng):
    from egregora_amd import native
    e, L = eng, eng.L
    g = torch.Generator().manual_seed(5)
    B, H, W, Ci, Co, k = 2, 8, 32, 128, 128, 3
    x = torch.randn(B, H, W, Ci, generator=g)
    x[1] *= 1e-3
    x = x.cuda()
    w = (torch.randn(Co, Ci, k, k, generator=g) / math.sqrt(Ci * k * k)).cuda()
    wp = e.pack_matrix(w.permute(2, 3, 1, 0).reshape(k * k * Ci, Co).contiguous()).cuda()
    ns = wp.shape[0]
    w2, ws = h2_pack(e, wp, Co)
    w_hat = unpack_conv(plane0(w2, ns, Co, ws), k, k, Ci, Co)
    y = torch.empty(B, H, W, Co, device="cuda")

    def run(xx):
        y.fill_(float("nan"))
        native.check(L.egr_conv_h1(p(xx), p(w2), p(None), p(None), p(None), p(y), B, H, W, Ci, H, W, Co, k, k, 1, 1, 1, 1, 0, 0, 0.0, 1, 1, 0, 0, H, W,
                                   1, 0, 0, 0, ws, p(row_amax(e, xx, B)), B, p(None), e._st()), "conv_h1")
        return y.clone()

    def bar_a_per_row(xx, yy, tag):
        ref_hat = conv64(round_x(xx, B), w_hat, 1)
        for b in range(B):
            a = float((yy[b].double() - ref_hat[b]).abs().max() / ref_hat[b].abs().max())
            print(f"{tag}, row {b}: bar A {a:.2e} (< 2e-6)")
            assert a < 2e-6, (tag, b, a)

    y_first = run(x)
    bar_a_per_row(x, y_first, "row 1 at 1e-3 of row 0")
    x[1] *= 1e-2
    y_second = run(x)
    bar_a_per_row(x, y_second, "row 1 at 1e-5 of row 0")
    assert torch.equal(y_second[0], y_first[0]), "row 0 does not see what row 1 holds"
    x[1] = 0.0
    y_silent = run(x)
    assert float(y_silent[1].abs().max()) == 0.0 and torch.equal(y_silent[0], y_first[0])
    x2 = torch.randn(B, H, W, Ci, generator=g)
    x2[0] *= 1e30
    x2[1] *= 1e-30
    y_range = run(x2.cuda())
    assert bool(torch.isfinite(y_range).all())
    bar_a_per_row(x2.cuda(), y_range, "1e30 next to 1e-30")


def test_h1_input_stationary_3x3_with_fused_groupnorm(eng):
    """egr_conv_h1_gn (k_conv3x3_isp<BN, 32, GN, SILU, 2>): images at different levels with a 5 sigma mean, as the scheme-1 test builds them."""
    from egregora_amd import native
    e, L = eng, eng.L
    g = torch.Generator().manual_seed(51)
    for (B, H, W, Ci, Co, silu, res_on) in [(3, 128, 256, 64, 128, 1, True), (5, 64, 256, 32, 128, 1, False)]:
        lvl = (10.0 ** -torch.arange(B).float())
        x = torch.randn(B, H, W, Ci, generator=g)
        x = x * lvl.view(B, 1, 1, 1) + 5.0 * lvl.view(B, 1, 1, 1)
        sc = (1.0 + 0.2 * torch.randn(B, Ci, generator=g)) / lvl.view(B, 1)
        sh = 0.3 * torch.randn(B, Ci, generator=g) - 5.0 * sc * lvl.view(B, 1)
        w = torch.randn(Co, Ci, 3, 3, generator=g) / math.sqrt(Ci * 9)
        b = 0.1 * torch.randn(Co, generator=g)
        r = 0.1 * torch.randn(B, H, W, Co, generator=g) if res_on else None
        x, sc, sh, w, b = x.cuda(), sc.cuda().contiguous(), sh.cuda().contiguous(), w.cuda(), b.cuda()
        r = r.cuda() if res_on else None
        xn = x.double() * sc.double().view(B, 1, 1, Ci) + sh.double().view(B, 1, 1, Ci)
        if silu:
            xn = xn * torch.sigmoid(xn)
        ref = conv64(xn, w.double(), 1) + b.double() + (r.double() if res_on else 0.0)
        A = conv64(xn.abs(), w.double().abs(), 1)
        wp = e.pack_matrix(w.permute(2, 3, 1, 0).reshape(9 * Ci, Co).contiguous()).cuda()
        ns = wp.shape[0]
        w2, ws = h2_pack(e, wp, Co)
        bound, oa = ra_zeros(B), ra_zeros(B)
        native.check(L.egr_gn_operand_bound(p(sc), p(sh), B, Ci, p(row_amax(e, x, B)), p(bound), e._st()), "bound")
        y = torch.full((B, H, W, Co), float("nan"), device="cuda")
        part = torch.zeros(B * H * W // 32, Co // 4, 2, device="cuda")
        native.check(L.egr_conv_h1_gn(p(x), p(sc), p(sh), silu, p(w2), p(b), p(r), p(y), B, H, W, Ci, Co, 0, ws, p(bound), p(oa), p(part), e._st()), "conv_h1_gn")
        name = native.last_conv_kernel()
        assert name == f"k_conv3x3_isp<128, 32, true, {'true' if silu else 'false'}, 2>", name
        # the model here: the float64 normalised tensor rounded under the scale the kernel derives from the BOUND of the row
        bits = bound[::RA].contiguous().view(torch.int32)
        ee = ((bits >> 23) & 0xff).clamp(15, 254)
        s = torch.pow(torch.tensor(2.0, dtype=torch.float64, device="cuda"), (141 - ee).double()).view(B, 1, 1, 1)
        xn_hat = (xn * s).float().half().double() / s
        ref_hat = conv64(xn_hat, unpack_conv(plane0(w2, ns, Co, ws), 3, 3, Ci, Co), 1) + b.double() + (r.double() if res_on else 0.0)
        for i in range(B):
            check_bars(f"fused GroupNorm {(B, H, W, Ci, Co)} image {i}", y[i], ref_hat[i], ref[i], A[i], k_b=1.0 + 2.0 ** -8, bar_a=False)
        assert torch.equal(oa[::RA], y.abs().amax(dim=(1, 2, 3)))
        yq = y.double().view(B * H * W // 32, 32, Co // 4, 4)
        assert float((part[..., 0].double() - yq.sum(dim=(1, 3))).abs().max()) <= 1e-4 * float(yq.abs().sum(dim=(1, 3)).max())
        assert float((part[..., 1].double() - (yq * yq).sum(dim=(1, 3))).abs().max()) <= 1e-4 * float((yq * yq).sum(dim=(1, 3)).max())
    # a shape that does not qualify is refused with nothing launched
    before = native.last_conv_kernel()
    x = torch.randn(1, 8, 48, 32, generator=g).cuda()
    y = torch.empty(1, 8, 48, 128, device="cuda")
    rc = L.egr_conv_h1_gn(p(x), p(sc), p(sh), 1, p(w2), p(None), p(None), p(y), 1, 8, 48, 32, 128, 0, ws, p(bound), p(None), p(None), e._st())
    assert rc == 3 and "qualify" in native.last_error()
    assert native.last_conv_kernel() == before
