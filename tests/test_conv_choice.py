"""The launcher's kernel selection, asked through the host-only query egr_conv_kernel_name (no GPU): every name below is written
out as rocprofv3 prints the instantiation and was derived by hand from the selection rules -- the column tile from Cout (32 / 64 /
128; 256 for the split kernels when Cout % 256 == 0), the short-K narrowing (K < 512: halve the tile down to 64 while 128-row tiles x
column tiles < 256), the 256-row tile (bf16 terms, 128 columns, >= 1024 tiles of 256 x 128), z-streaming (ceil(nz / min(nz,
ceil(2048 / tiles))) >= 2 problems per workgroup), split-K (nz == 1, < 192 tiles, >= 32 slabs of 16), and the conditions of the
input-stationary 1-D and 3x3 kernels.  tests/test_gpu_conv_choice.py holds the launches themselves to the same answers."""
import importlib.util
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
PTR = 4096                      # stands for a 16-byte aligned device pointer: the query dereferences nothing

# description -> (name, ksplit, zs_nzb); every case runs with the default switches here and is the base of CASES_SWITCHED
CASES = {
    # fp32 MFMA kernel: column tile by Cout, vector loader with Cin % 16 == 0 and an aligned x, GroupNorm loader
    "igemm_c32": (dict(w=PTR, B=1, H=8, W=8, OH=8, OW=8, Cin=16, Cout=32), ("k_conv_igemm<32, true, false>", 1, 0)),
    "igemm_c33": (dict(w=PTR, B=1, H=8, W=8, OH=8, OW=8, Cin=16, Cout=33), ("k_conv_igemm<64, true, false>", 1, 0)),
    "igemm_c64": (dict(w=PTR, B=1, H=8, W=8, OH=8, OW=8, Cin=16, Cout=64), ("k_conv_igemm<64, true, false>", 1, 0)),
    "igemm_c128": (dict(w=PTR, B=1, H=8, W=8, OH=8, OW=8, Cin=16, Cout=128), ("k_conv_igemm<128, true, false>", 1, 0)),
    "igemm_cin3": (dict(w=PTR, B=1, H=8, W=8, OH=8, OW=8, Cin=3, Cout=32, KH=3, KW=3, pad_t=1, pad_l=1), ("k_conv_igemm<32, false, false>", 1, 0)),
    "igemm_unaligned_x": (dict(x=PTR + 4, w=PTR, B=1, H=8, W=8, OH=8, OW=8, Cin=16, Cout=32), ("k_conv_igemm<32, false, false>", 1, 0)),
    "igemm_gn": (dict(w=PTR, gn_scale=PTR, gn_shift=PTR, gn_silu=1, B=1, H=8, W=8, OH=8, OW=8, Cin=16, Cout=64, KH=3, KW=3, pad_t=1, pad_l=1),
                 ("k_conv_igemm<64, true, true>", 1, 0)),
    "igemm_splitk": (dict(w=PTR, B=128, Cin=512, Cout=32), ("k_conv_igemm<32, true, false>", 4, 0)),
    # split kernels: 256 columns at Cout % 256 == 0 (65536 rows, K = 512: 512 tiles, no narrowing)
    "s3_bn256": (dict(w3=PTR, B=65536, Cin=512, Cout=256), ("k_conv_s3<128, 256, 1, false, 0>", 1, 0)),
    "h2_bn256": (dict(w3=PTR, sch=1, row_amax=PTR, batch_rows=2, B=65536, Cin=512, Cout=256), ("k_conv_s3<128, 256, 1, false, 1>", 1, 0)),
    "s3_bn256_3x3": (dict(w3=PTR, B=1, H=160, W=160, OH=160, OW=160, Cin=64, Cout=256, KH=3, KW=3, pad_t=1, pad_l=1),
                     ("k_conv_s3<128, 256, 1, false, 0>", 1, 0)),            # 200 tiles, 36 slabs: neither narrowed nor split
    "h2_bn256_3x3": (dict(w3=PTR, sch=1, row_amax=PTR, batch_rows=1, B=1, H=160, W=160, OH=160, OW=160, Cin=64, Cout=256, KH=3, KW=3, pad_t=1, pad_l=1),
                     ("k_conv_s3<128, 256, 1, false, 1>", 1, 0)),            # (40 x 5 = 200 < 512 tiles of 4 x 32: not the 3x3 kernel's)
    # K = 256 < 512: 4096 rows = 32 row tiles -> 32, 64, (128 at 64 columns: the loop ends at 64); 16384 rows -> 128 x 2 = 256 at 128
    "s3_narrow_64": (dict(w3=PTR, B=4096, Cin=256, Cout=256), ("k_conv_s3<128, 64, 1, false, 0>", 1, 0)),
    "s3_narrow_128": (dict(w3=PTR, B=16384, Cin=256, Cout=256), ("k_conv_s3<128, 128, 1, false, 0>", 1, 0)),
    "s3_not_narrow": (dict(w3=PTR, B=32768, Cin=256, Cout=256), ("k_conv_s3<128, 256, 1, false, 0>", 1, 0)),
    # 262144 rows x 128 outputs = 1024 tiles of 256 x 128: the bf16 scheme takes them, the fp16 scheme never does
    "s3_bm256": (dict(w3=PTR, B=262144, Cin=64, Cout=128), ("k_conv_s3<256, 128, 1, false, 0>", 1, 0)),
    "s3_bm128": (dict(w3=PTR, B=261888, Cin=64, Cout=128), ("k_conv_s3<128, 128, 1, false, 0>", 1, 0)),
    "h2_never_bm256": (dict(w3=PTR, sch=1, row_amax=PTR, batch_rows=2, B=262144, Cin=64, Cout=128), ("k_conv_s3<128, 128, 1, false, 1>", 1, 0)),
    # z stacks (dense zw: K / 16 * Cout * 6 sixteen-byte units of bf16 terms, * 4 of fp16 terms).  128 rows are ONE tile: 36 groups of
    # one z each, nothing to stream; 114 row tiles -> ceil(2048 / 114) = 18 groups of 2
    "s3_stack_one_tile": (dict(w3=PTR, nz=36, B=128, Cin=16, Cout=128, zx=128 * 16, zw=768, zy=128 * 128), ("k_conv_s3<128, 128, 1, false, 0>", 1, 0)),
    "s3_stack_bias": (dict(w3=PTR, bias=PTR, nz=36, B=128, Cin=16, Cout=128, zx=128 * 16, zw=768, zy=128 * 128), ("k_conv_s3<128, 128, 1, false, 0>", 1, 0)),
    "s3_stack_streamed": (dict(w3=PTR, nz=36, B=14592, Cin=16, Cout=128, zx=14592 * 16, zw=768, zy=14592 * 128), ("k_conv_s3<128, 128, 1, true, 0>", 1, 2)),
    "h2_stack_streamed": (dict(w3=PTR, sch=1, row_amax=PTR, batch_rows=2, nz=36, B=14592, Cin=16, Cout=128, zx=14592 * 16, zw=512, zy=14592 * 128),
                          ("k_conv_s3<128, 128, 1, true, 1>", 1, 2)),
    "s3_stack_streamed_bias": (dict(w3=PTR, bias=PTR, nz=36, B=14592, Cin=16, Cout=128, zx=14592 * 16, zw=768, zy=14592 * 128),
                               ("k_conv_s3<128, 128, 1, false, 0>", 1, 0)),
    "s3_stack_sparse_zw": (dict(w3=PTR, nz=36, B=14592, Cin=16, Cout=128, zx=14592 * 16, zw=1024, zy=14592 * 128), ("k_conv_s3<128, 128, 1, false, 0>", 1, 0)),
    # one tile, 32 slabs: S = min(768, 32 / 8) = 4 parts of 8 slabs
    "s3_splitk": (dict(w3=PTR, B=128, Cin=512, Cout=32), ("k_conv_s3<128, 32, 1, false, 0>", 4, 0)),
    # input-stationary 1-D kernel
    "c1d": (dict(w3=PTR, B=1, W=128, OW=128, Cin=16, Cout=32, KW=3, pad_l=1), ("k_conv1d_s3<32, 16, 0>", 1, 0)),
    "c1d_cin32_h2": (dict(w3=PTR, sch=1, row_amax=PTR, batch_rows=1, B=1, W=128, OW=128, Cin=32, Cout=64, KW=3, pad_l=1), ("k_conv1d_s3<64, 32, 1>", 1, 0)),
    "c1d_w64": (dict(w3=PTR, B=1, W=64, OW=64, Cin=16, Cout=32, KW=3, pad_l=1), ("k_conv_s3<128, 32, 1, false, 0>", 1, 0)),
    "c1d_pad": (dict(w3=PTR, B=1, W=128, OW=128, Cin=16, Cout=32, KW=3, pad_l=2), ("k_conv_s3<128, 32, 1, false, 0>", 1, 0)),
    "c1d_h2_rows64": (dict(w3=PTR, sch=1, row_amax=PTR, batch_rows=4, B=2, W=128, OW=128, Cin=16, Cout=32, KW=3, pad_l=1),
                      ("k_conv_s3<128, 32, 1, false, 1>", 1, 0)),
    # input-stationary 3x3 kernel: fp16 scheme only, 16 x 32 = 512 tiles of 4 x 32 pixels
    "c3": (dict(w3=PTR, sch=1, row_amax=PTR, batch_rows=1, B=1, H=64, W=1024, OH=64, OW=1024, Cin=32, Cout=64, KH=3, KW=3, pad_t=1, pad_l=1),
           ("k_conv3x3_isp<64, 32, false, false>", 1, 0)),
    "c3_gn_silu": (dict(w3=PTR, sch=1, row_amax=PTR, batch_rows=1, gn_scale=PTR, gn_shift=PTR, gn_silu=1, B=1, H=64, W=1024, OH=64, OW=1024, Cin=32,
                        Cout=64, KH=3, KW=3, pad_t=1, pad_l=1), ("k_conv3x3_isp<64, 32, true, true>", 1, 0)),
    "c3_gn": (dict(w3=PTR, sch=1, row_amax=PTR, batch_rows=1, gn_scale=PTR, gn_shift=PTR, B=1, H=64, W=1024, OH=64, OW=1024, Cin=32, Cout=128, KH=3,
                   KW=3, pad_t=1, pad_l=1), ("k_conv3x3_isp<128, 32, true, false>", 1, 0)),
    "c3_bf16": (dict(w3=PTR, B=1, H=64, W=1024, OH=64, OW=1024, Cin=32, Cout=64, KH=3, KW=3, pad_t=1, pad_l=1), ("k_conv_s3<128, 64, 1, false, 0>", 1, 0)),
    "c3_h62": (dict(w3=PTR, sch=1, row_amax=PTR, batch_rows=1, B=1, H=62, W=1024, OH=62, OW=1024, Cin=32, Cout=64, KH=3, KW=3, pad_t=1, pad_l=1),
               ("k_conv_s3<128, 64, 1, false, 1>", 1, 0)),
}
# switch set to 0 (EGR_S3_PF: to 2) -> the cases whose answer changes; every other case must come out as above
CASES_SWITCHED = {
    "EGR_S3_BN256": {"s3_bn256": ("k_conv_s3<128, 128, 1, false, 0>", 1, 0), "h2_bn256": ("k_conv_s3<128, 128, 1, false, 1>", 1, 0),
                     "s3_bn256_3x3": ("k_conv_s3<128, 128, 1, false, 0>", 1, 0), "h2_bn256_3x3": ("k_conv_s3<128, 128, 1, false, 1>", 1, 0),
                     "s3_not_narrow": ("k_conv_s3<128, 128, 1, false, 0>", 1, 0)},
    "EGR_S3_NARROW": {"s3_narrow_64": ("k_conv_s3<128, 256, 1, false, 0>", 1, 0), "s3_narrow_128": ("k_conv_s3<128, 256, 1, false, 0>", 1, 0)},
    "EGR_S3_ZS": {"s3_stack_streamed": ("k_conv_s3<128, 128, 1, false, 0>", 1, 0), "h2_stack_streamed": ("k_conv_s3<128, 128, 1, false, 1>", 1, 0)},
    "EGR_S3_CONV1D": {"c1d": ("k_conv_s3<128, 32, 1, false, 0>", 1, 0), "c1d_cin32_h2": ("k_conv_s3<128, 64, 1, false, 1>", 1, 0)},
    "EGR_S3_CONV3X3": {"c3": ("k_conv_s3<128, 64, 1, false, 1>", 1, 0), "c3_gn_silu": None, "c3_gn": None},
    # prefetch depth 2 exists for the bf16-term 128-row kernels with up to 128 columns, streamed ones excepted
    "EGR_S3_PF": {k: (v[1][0].replace(", 1, false, 0>", ", 2, false, 0>"),) + v[1][1:] for k, v in CASES.items()
                  if v[1][0].startswith("k_conv_s3<128, ") and v[1][0].endswith(", 1, false, 0>") and "<128, 256" not in v[1][0]},
}


def _native():
    spec = importlib.util.spec_from_file_location("egr_native_alone", ROOT / "comfyui-egregora-audio-super-resolution_amd" / "native.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def answers():
    """{case: [name, ksplit, zs_nzb] or None when the query refuses} under this process's switches."""
    native, out = _native(), {}
    for key, (desc, _) in CASES.items():
        try:
            out[key] = list(native.conv_kernel_name(**dict(dict(x=PTR, y=PTR), **desc)))
        except RuntimeError:
            out[key] = None
    return out


def test_default_choices_equal_the_names_written_out():
    got = answers()
    for key, (_, want) in CASES.items():
        assert got[key] == list(want), key
    assert len({v[1][0] for v in CASES.values()}) >= 20            # the cases reach that many different instantiations


@pytest.mark.parametrize("switch", sorted(CASES_SWITCHED))
def test_each_switch_changes_exactly_its_cases(switch):
    """The switches are read once per process: a child process with the switch set answers every case."""
    env = dict(os.environ, **{switch: "2" if switch == "EGR_S3_PF" else "0"})
    r = subprocess.run([sys.executable, __file__], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout)
    for key, (_, want) in CASES.items():
        want = CASES_SWITCHED[switch].get(key, want)
        assert got[key] == (None if want is None else list(want)), (switch, key)


def test_query_refuses_what_the_launch_refuses():
    native = _native()
    c3 = dict(CASES["c3_gn_silu"][0], x=PTR, y=PTR)
    with pytest.raises(RuntimeError, match="does not qualify"):       # GroupNorm loader, fp16 terms, H % 4 != 0: no kernel serves it
        native.conv_kernel_name(**dict(c3, H=62, OH=62))
    with pytest.raises(RuntimeError, match="null x/w/y"):
        native.conv_kernel_name(B=1, Cin=16, Cout=32)
    with pytest.raises(RuntimeError, match="Cin %% 16 == 0|Cin % 16 == 0"):
        native.conv_kernel_name(x=PTR, y=PTR, w3=PTR, B=128, Cin=24, Cout=32)
    with pytest.raises(RuntimeError, match="bad output placement"):
        native.conv_kernel_name(x=PTR, y=PTR, w=PTR, B=1, H=8, W=8, OH=8, OW=8, OHF=4, OWF=8, Cin=16, Cout=32)
    assert native.last_conv_kernel() == ""                            # nothing was launched by any of this


if __name__ == "__main__":
    print(json.dumps(answers()))
