"""The one-term fp16 operand scheme (scheme 2, the opt-in fast mode of FlashSR) as far as the host alone can see it: the launcher's
host-only query names a one-term instantiation for every shape family the scheme serves, and the choices of schemes 0 and 1 (names,
split-K factors, z problems per workgroup) are the ones recorded from the commit before the scheme existed, written out below; the
creation flag has the same value in the header and in the binding, and FlashSREngine.SPLIT maps to it.

One of the shapes comes out differently from what its size suggests: (9, 128, 128, 32, 128, 3) has 147456 GEMM rows, but with one
batch row per image scheme 1 runs it on the input-stationary 3x3 kernel (k_conv3x3_isp), not on a k_conv_s3 tile -- so scheme 2 names
that kernel's one-term form, k_conv3x3_isp<128, 32, false, false, 2>."""
import importlib.util
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
PTR = 4096                      # stands for a 16-byte aligned device pointer: the query dereferences nothing


def _native():
    spec = importlib.util.spec_from_file_location("egr_native_alone", ROOT / "comfyui-egregora-audio-super-resolution_amd" / "native.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def conv(B, H, W, Ci, Co, k):
    return dict(B=B, H=H, W=W, OH=H, OW=W, Cin=Ci, Cout=Co, KH=k, KW=k, pad_t=k // 2, pad_l=k // 2, bias=PTR)


# shape -> (description, batch rows, {scheme: (name, ksplit, zs_nzb)}); schemes 0 and 1 as the parent commit answered
SHAPES = {
    "c128": (conv(2, 16, 12, 128, 128, 3), 2, {0: ("k_conv_s3<128, 128, 1, false, 0>", 9, 0), 1: ("k_conv_s3<128, 128, 1, false, 1>", 9, 0),
                                                2: ("k_conv_s3<128, 128, 1, false, 2>", 9, 0)}),
    "big": (conv(9, 128, 128, 32, 128, 3), 9, {0: ("k_conv_s3<128, 128, 1, false, 0>", 1, 0), 1: ("k_conv3x3_isp<128, 32, false, false>", 1, 0),
                                               2: ("k_conv3x3_isp<128, 32, false, false, 2>", 1, 0)}),
    "splitk": (conv(2, 8, 4, 640, 640, 3), 2, {0: ("k_conv_s3<128, 128, 1, false, 0>", 45, 0), 1: ("k_conv_s3<128, 128, 1, false, 1>", 45, 0),
                                               2: ("k_conv_s3<128, 128, 1, false, 2>", 45, 0)}),
    "bn256": (conv(1, 24, 16, 64, 512, 3), 1, {0: ("k_conv_s3<128, 256, 1, false, 0>", 4, 0), 1: ("k_conv_s3<128, 256, 1, false, 1>", 4, 0),
                                               2: ("k_conv_s3<128, 256, 1, false, 2>", 4, 0)}),
    "c30": (conv(2, 6, 6, 32, 30, 3), 2, {0: ("k_conv_s3<128, 32, 1, false, 0>", 1, 0), 1: ("k_conv_s3<128, 32, 1, false, 1>", 1, 0),
                                          2: ("k_conv_s3<128, 32, 1, false, 2>", 1, 0)}),
    "c1d": (dict(B=3, W=512, OW=512, Cin=64, Cout=64, KW=7, dil=3, pad_l=9, bias=PTR), 3,
            {0: ("k_conv1d_s3<64, 32, 0>", 1, 0), 1: ("k_conv1d_s3<64, 32, 1>", 1, 0), 2: ("k_conv1d_s3<64, 32, 2>", 1, 0)}),
    # z-stacked GEMM, nz 36, P 700, 128 -> 128: six row tiles leave one z per workgroup (nothing to stream)
    "zstack": (dict(nz=36, B=700, Cin=128, Cout=128, zx=700 * 128, zy=700 * 128), 7,
               {0: ("k_conv_s3<128, 128, 1, false, 0>", 1, 0), 1: ("k_conv_s3<128, 128, 1, false, 1>", 1, 0), 2: ("k_conv_s3<128, 128, 1, false, 2>", 1, 0)}),
    # the same stack with 14592 rows: 114 row tiles, two z per workgroup -- the streamed instantiation
    "zstream": (dict(nz=36, B=14592, Cin=128, Cout=128, zx=14592 * 128, zy=14592 * 128), 2,
                {0: ("k_conv_s3<128, 128, 1, true, 0>", 1, 2), 1: ("k_conv_s3<128, 128, 1, true, 1>", 1, 2), 2: ("k_conv_s3<128, 128, 1, true, 2>", 1, 2)}),
}


def describe(key, sch):
    d, rows, _ = SHAPES[key]
    d = dict(d, x=PTR, y=PTR, w3=PTR)
    if sch:
        d.update(sch=sch, row_amax=PTR, batch_rows=rows)
    if "nz" in d:
        d["zw"] = d["Cin"] // 16 * d["Cout"] * (4 if sch else 6)        # dense stack: 16-byte units per z of the two- / three-plane pack
    return d


@pytest.mark.parametrize("key", sorted(SHAPES))
def test_scheme_2_names_a_one_term_instantiation_and_the_other_schemes_did_not_move(key):
    native = _native()
    want = SHAPES[key][2]
    for sch in (0, 1, 2):
        assert tuple(native.conv_kernel_name(**describe(key, sch))) == want[sch], (key, sch)
    name = want[2][0]
    assert name.endswith(", 2>")
    if key in ("c128", "splitk", "bn256", "c30", "zstack", "zstream"):
        assert name.startswith("k_conv_s3<")
    if key == "c1d":
        assert name.startswith("k_conv1d_s3<")
    assert native.last_conv_kernel() == ""                            # a query launches nothing


def test_scheme_3_is_refused():
    native = _native()
    for key in sorted(SHAPES):
        with pytest.raises(RuntimeError, match="bad operand scheme"):
            native.conv_kernel_name(**describe(key, 3))
    with pytest.raises(RuntimeError, match="bad operand scheme"):
        native.conv_kernel_name(**dict(describe("c128", 1), sch=-1))


def test_scheme_2_has_the_preconditions_of_scheme_1():
    native = _native()
    d = describe("c128", 2)
    with pytest.raises(RuntimeError, match="bad operand scheme"):       # no row maxima
        native.conv_kernel_name(**dict(d, row_amax=0))
    with pytest.raises(RuntimeError, match="bad operand scheme"):       # batch rows that do not divide the GEMM rows
        native.conv_kernel_name(**dict(d, batch_rows=5))
    gn = dict(describe("big", 2), gn_scale=PTR, gn_shift=PTR, gn_silu=1)
    assert native.conv_kernel_name(**gn)[0] == "k_conv3x3_isp<128, 32, true, true, 2>"
    with pytest.raises(RuntimeError, match="does not qualify"):         # fused GroupNorm, shape outside the input-stationary kernel
        native.conv_kernel_name(**dict(gn, B=1, H=8, W=48, OH=8, OW=48, batch_rows=1))


def test_flag_value_in_the_header_equals_the_binding():
    native = _native()
    txt = (ROOT / "include" / "egregora_amd.h").read_text()
    m = re.search(r"#define\s+EGR_FSR_FAST_F16\s+0x([0-9a-fA-F]+)u", txt)
    assert m and int(m.group(1), 16) == native.FSR_FAST_F16 == 0x80
    others = [native.FSR_F32_MFMA, native.FSR_NO_WINOGRAD, native.FSR_NO_WINO_F4, native.FSR_NO_GN_PARTIALS, native.FSR_NO_THIN_ENDS,
              native.FSR_NO_FUSE_GN, native.FSR_SPLIT_BF16X3]
    assert all(native.FSR_FAST_F16 & o == 0 for o in others)
    for sym in ("egr_conv_h1", "egr_conv_h1_gn", "egr_flashsr_split_scheme"):
        assert sym in native.SIGNATURES and re.search(r"\b%s\(" % sym, txt), sym
    assert native.SIGNATURES["egr_conv_h1"] == native.SIGNATURES["egr_conv_h2"]
    assert native.SIGNATURES["egr_conv_h1_gn"] == native.SIGNATURES["egr_conv_h2_gn"]


def test_split_value_maps_to_the_flag(pack):
    from egregora_amd import flashsr_engine as E, native
    flags = {}
    for split in ("f16x1", "f16x2", "bf16x3"):
        eng = object.__new__(E.FlashSREngine)       # no engine is built: handle_flags reads the switches only
        eng.SPLIT = split
        flags[split] = eng.handle_flags()
    assert flags["f16x1"] & native.FSR_FAST_F16
    assert not flags["f16x2"] & native.FSR_FAST_F16 and not flags["bf16x3"] & native.FSR_FAST_F16
    assert not flags["f16x1"] & native.FSR_SPLIT_BF16X3 and flags["bf16x3"] & native.FSR_SPLIT_BF16X3
