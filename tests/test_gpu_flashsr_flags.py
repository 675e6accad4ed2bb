"""Every creation flag and creation-time switch of the FlashSR handle (egr_flashsr_create, csrc/egr_flashsr.cpp) held to the FLOAT64
run of the same graph, at a toy size at which the flags have something to select.

The reach config.  flashsr_arch.tiny_config() has 32 .. 128 channels against the Winograd threshold of 128 and a 128 x 32 mel image,
so at default flags its handle reaches no Winograd kernel, no GroupNorm partials, no fused GroupNorm and never the input-stationary
3x3.  Two things are changed, nothing else:
  * the Winograd threshold is lowered to 32 (FlashSREngine.WINO_MIN_CH for the Python driver, EGREGORA_FLASHSR_WINOGRAD_MIN_CH for the
    handle, both set before the engine is built): every 3x3 of a res-block then takes F(4x4,3x3) -- all image sizes are multiples of
    4 and Cout / gn_groups is 4, 8 or 16 -- with GroupNorm partials out of its output transform and the next norm fused into the
    next input transform;
  * n_mels = 128 instead of 32 (dataclasses.replace): the input-stationary 3x3 with the GroupNorm in its loader wants W % 32 == 0 and
    at least 512 tiles of 4 x 32 pixels in a forward; four rows of 128 x 128 are exactly 512, so the four-row passes below run the
    VAE's 32-channel level on it (egr_flashsr_infer only: the kernel belongs to the fp16 operand scheme).  The chunk stays 3840.
The 16-channel vocoder stage (640 samples) takes the fused AMP unit, conv_in (one input channel) and the decoder's conv_out (one output
channel) the thin-end kernels; the float64 run of four rows takes a second or two.

What a variant ran is read from the handle's own profile (FlashSREngine.c_profile(fn, ops=True), egr_flashsr_set_profiling level 2):
contraction kernels under the launcher's instantiation names, every other operator launch under the name of the library entry point
the walker called.  Every operator name used below is checked to be an export of the library; the name of the input-stationary 3x3
comes from egr_conv_kernel_name; the kernel families (k_conv_s3, k_conv_igemm, k_amp_unit) are prefixes of what the profile reports.
egr_flashsr_forward walks the graph on the three-term bf16 kernels ("fwd" below), egr_flashsr_infer on the two-term fp16 scheme
("inf") where the handle has it.

Bars (those of tests/test_gpu_flashsr.py::test_engine_matches_torch_reference_stage_by_stage and of
tests/test_gpu_flashsr_capi.py, unchanged): stages mel / z_cond / v / z0 / mel_hat within 2e-4 relative L2 of float64, the waveform
within 1e-3 and 0.05 dB LSD (256 / 64); egr_flashsr_infer within 2e-5 relative norm of the same handle's three-term forward; the walker
equal to the Python driver bit for bit.  Measured values: profiles/flashsr_flags.md.
"""
import contextlib
import dataclasses
import math
from types import SimpleNamespace

import pytest
import torch

from test_gpu_flashsr import f64_forward_on_gpu, nchw, rel_l2

pytestmark = pytest.mark.gpu

STAGES = ("mel", "z_cond", "v", "z0", "mel_hat", "y")
WINO_MIN = 32
ROWS = 4
SEED = 11
ENV = ("EGREGORA_FLASHSR_WINOGRAD_MIN_CH", "EGREGORA_FLASHSR_DIRECT3X3_MAX_COUT", "EGREGORA_FLASHSR_FUSED_AMP", "EGREGORA_FLASHSR_OUT_AMAX",
       "EGREGORA_FLASHSR_SPLIT", "EGREGORA_FLASHSR_STREAMS", "EGREGORA_FLASHSR_ROWS", "EGREGORA_FLASHSR_ARENA_GB")
IS3X3 = "<input-stationary 3x3>"       # stands for the name egr_conv_kernel_name gives (is3x3_name)


def V(attrs=None, env=None, flags=(), h2=True, delta=()):
    return SimpleNamespace(attrs=attrs or {}, env=env or {}, flags=flags, h2=h2, delta=delta)


# name -> class switches of the Python driver (which handle_flags turns into creation flags), environment read by egr_flashsr_create,
# the creation flags the handle must carry, whether egr_flashsr_infer runs the fp16 scheme, and the delta of the launch counts against
# the default handle: (walk, name or prefix*, relation).  absent: launched by the default, not here; new: here only; fewer / more:
# launched by both; same: equal counts.
VARIANTS = {
    "NO_WINO_F4": V(dict(WINO_F4=False), flags=("FSR_NO_WINO_F4",), delta=(
        ("fwd", "egr_winograd4_input", "absent"), ("fwd", "egr_winograd4_output_ra", "absent"), ("fwd", "egr_winograd_input", "new"),
        ("fwd", "egr_winograd_output", "new"), ("inf", "egr_winograd4_input_ra", "absent"), ("inf", "egr_winograd_input", "new"),
        ("inf", "egr_winograd_output", "new"), ("inf", "egr_absmax_rows", "more"))),          # V and the F(2x2) outputs are measured by their readers
    "NO_GN_PARTIALS": V(dict(GN_PARTIALS=False), flags=("FSR_NO_GN_PARTIALS",), delta=(
        ("fwd", "egr_groupnorm_stats_from_partials", "absent"), ("fwd", "egr_groupnorm_coeff_from_stats", "absent"),
        ("fwd", "egr_groupnorm_coeff", "more"), ("fwd", "egr_winograd4_output_ra", "same"),
        ("inf", "egr_groupnorm_stats_from_partials", "absent"), ("inf", "egr_groupnorm_coeff", "more"), ("inf", IS3X3, "same"))),
    "NO_FUSE_GN": V(dict(FUSE_GN="0"), flags=("FSR_NO_FUSE_GN",), delta=(
        ("fwd", "egr_groupnorm_coeff*", "absent"), ("fwd", "egr_groupnorm_stats_from_partials", "absent"),
        ("fwd", "egr_groupnorm_nhwc_ra", "more"), ("fwd", "egr_winograd4_input", "same"), ("inf", "egr_groupnorm_nhwc_ra", "more"))),
    "NO_THIN_ENDS": V(dict(THIN_ENDS=False), flags=("FSR_NO_THIN_ENDS",), delta=(
        ("fwd", "egr_conv_cin1", "absent"), ("fwd", "egr_tap_gather", "absent"), ("inf", "egr_conv_cin1", "absent"),
        ("inf", "egr_tap_gather", "absent"))),
    "NO_WINOGRAD": V(dict(WINO_MIN_CH=1 << 30), flags=("FSR_NO_WINOGRAD",), delta=(      # the handle's threshold stays 32: the flag does the work
        ("fwd", "egr_winograd*", "absent"), ("fwd", "egr_groupnorm_coeff*", "absent"), ("fwd", "egr_groupnorm_nhwc_ra", "more"),
        ("inf", "egr_winograd*", "absent"), ("inf", IS3X3, "same"))),
    "F32_MFMA": V(dict(MFMA_MODE="f32"), flags=("FSR_F32_MFMA",), h2=False, delta=(
        ("fwd", "k_conv_s3*", "absent"), ("fwd", "k_conv_igemm*", "more"), ("fwd", "egr_winograd4_input", "same"),
        ("inf", "k_amp_unit*", "absent"), ("inf", IS3X3, "absent"), ("inf", "k_conv_s3*", "absent"), ("inf", "egr_absmax_rows", "absent"))),
    "SPLIT_BF16X3": V(dict(SPLIT="bf16x3"), flags=("FSR_SPLIT_BF16X3",), h2=False, delta=(
        ("inf", "k_amp_unit*", "absent"), ("inf", IS3X3, "absent"), ("inf", "egr_absmax_rows", "absent"),
        ("inf", "egr_winograd4_input_ra", "absent"), ("inf", "egr_winograd4_input", "new"), ("inf", "egr_eltwise_ra", "absent"))),
    "DIRECT3X3_MAX_COUT=0": V(env={"EGREGORA_FLASHSR_DIRECT3X3_MAX_COUT": "0"}, delta=(
        ("inf", IS3X3, "absent"), ("inf", "egr_gn_operand_bound", "absent"), ("inf", "egr_winograd4_input_ra", "more"))),
    "FUSED_AMP=0": V(env={"EGREGORA_FLASHSR_FUSED_AMP": "0"}, delta=(
        ("inf", "k_amp_unit*", "absent"), ("inf", "egr_snake_aa_ra", "more"))),
    "OUT_AMAX=0": V(env={"EGREGORA_FLASHSR_OUT_AMAX": "0"}, delta=(
        ("inf", "egr_eltwise_ra", "absent"), ("inf", "egr_layernorm_rows_ra", "absent"), ("inf", "egr_concat_channels_ra", "absent"),
        ("inf", "egr_geglu_ra", "absent"), ("inf", "egr_layernorm_rows", "new"), ("inf", "egr_geglu", "new"),
        ("inf", "egr_concat_channels", "new"), ("inf", "egr_absmax_rows", "more"))),
    "WINOGRAD_MIN_CH=64": V(dict(WINO_MIN_CH=64), env={"EGREGORA_FLASHSR_WINOGRAD_MIN_CH": "64"}, delta=(      # 64-channel layers only
        ("fwd", "egr_winograd4_input", "fewer"), ("fwd", "egr_winograd4_output_ra", "fewer"), ("fwd", "egr_groupnorm_nhwc_ra", "more"),
        ("inf", "egr_winograd4_input_ra", "fewer"))),
    # pairs that interact
    # partials exist only with F(4x4): with them requested and F(4x4) off the statistics of every Winograd output fall back to the
    # pass over the tensor; in the fp16 walk the input-stationary 3x3 is then the only producer of partials left
    "NO_WINO_F4+GN_PARTIALS": V(dict(WINO_F4=False, GN_PARTIALS=True), flags=("FSR_NO_WINO_F4",), delta=(
        ("fwd", "egr_groupnorm_stats_from_partials", "absent"), ("fwd", "egr_groupnorm_coeff_from_stats", "absent"),
        ("fwd", "egr_groupnorm_coeff", "more"), ("inf", "egr_groupnorm_stats_from_partials", "fewer"), ("inf", "egr_groupnorm_coeff", "more"))),
    # the input-stationary 3x3 carries its GroupNorm in the loader whatever NO_FUSE_GN says (gn_conv3 tries it first): what the
    # handle does today; every other norm is applied as a pass
    "NO_FUSE_GN+DIRECT3X3": V(dict(FUSE_GN="0"), env={"EGREGORA_FLASHSR_DIRECT3X3_MAX_COUT": "128"}, flags=("FSR_NO_FUSE_GN",), delta=(
        ("inf", IS3X3, "same"), ("inf", "egr_gn_operand_bound", "same"), ("inf", "egr_groupnorm_coeff_from_stats", "fewer"),
        ("inf", "egr_groupnorm_nhwc_ra", "more"))),
    "NO_GN_PARTIALS+NO_FUSE_GN": V(dict(GN_PARTIALS=False, FUSE_GN="0"), flags=("FSR_NO_GN_PARTIALS", "FSR_NO_FUSE_GN"), delta=(
        ("fwd", "egr_groupnorm_coeff*", "absent"), ("fwd", "egr_groupnorm_stats_from_partials", "absent"),
        ("fwd", "egr_groupnorm_nhwc_ra", "more"), ("inf", "egr_groupnorm_stats_from_partials", "absent"),
        ("inf", "egr_groupnorm_coeff_from_stats", "absent"), ("inf", IS3X3, "same"))),
}


def reach_config():
    from egregora_amd import flashsr_arch as A
    return dataclasses.replace(A.tiny_config(), n_mels=128)


@contextlib.contextmanager
def built(cfg, P, v):
    """A fresh Python-driver engine and its handle under the variant's switches (class switches are frozen per engine at construction,
    the environment is read by egr_flashsr_create); closed on exit."""
    from egregora_amd import flashsr_engine as E
    from tools.flashsr_pydriver import PyDriverEngine
    attrs = dict(WINO_MIN_CH=WINO_MIN, WINO_F4=True, GN_PARTIALS=True, THIN_ENDS=True, FUSE_GN="1", MFMA_MODE="bf16x3", SPLIT="f16x2")
    attrs.update(v.attrs)
    env = {"EGREGORA_FLASHSR_WINOGRAD_MIN_CH": str(WINO_MIN)}
    env.update(v.env)
    with pytest.MonkeyPatch.context() as mp:
        for k in ENV:
            mp.delenv(k, raising=False)
        for k, val in env.items():
            mp.setenv(k, val)
        for k, val in attrs.items():
            mp.setattr(E.FlashSREngine, k, val)
        e = PyDriverEngine(cfg, P)
        e.handle
    try:
        yield e
    finally:
        e.close()


def counts(prof):
    return {k: v[0] for k, v in prof.items()}


def launches(cnt, name):
    if name.endswith("*"):
        return sum(n for k, n in cnt.items() if k.startswith(name[:-1]))
    return cnt.get(name, 0)


def profiles(e, d):
    """Launch counts of one egr_flashsr_forward and one egr_flashsr_infer (the second call of each: the scratch exists)."""
    e.c_forward(d.x, d.nz)
    e.c_infer(d.x, d.ids, SEED)
    return (counts(e.c_profile(lambda: e.c_forward(d.x, d.nz), ops=True)), counts(e.c_profile(lambda: e.c_infer(d.x, d.ids, SEED), ops=True)))


def is3x3_name(cfg):
    """What the launcher calls the kernel it picks for the VAE's first-level 3x3 with a fused GroupNorm + SiLU in the fp16 scheme."""
    from egregora_amd import native
    c = cfg.vae_ch * cfg.vae_mult[0]
    ptr = 4096                               # stands for an aligned device pointer: the query dereferences nothing
    return native.conv_kernel_name(x=ptr, w3=ptr, y=ptr, sch=1, row_amax=ptr, batch_rows=ROWS, gn_scale=ptr, gn_shift=ptr, gn_silu=1, B=ROWS,
                                   H=cfg.n_frames, W=cfg.n_mels, OH=cfg.n_frames, OW=cfg.n_mels, Cin=c, Cout=c, KH=3, KW=3, pad_t=1, pad_l=1)[0]


def lsd_256(want, got):
    from oracle import metrics as om
    return float(om.lsd_audio(want.double().numpy().reshape(-1), got.double().numpy().reshape(-1), 256, 64)[0])


def stage_nchw(t):
    return t.permute(0, 3, 1, 2) if t.dim() == 4 else t


@pytest.fixture(scope="module")
def ref(pack):
    """Inputs, noise and weights shared by every variant, the float64 run of both passes (once), and the default handle's launches."""
    from egregora_amd import flashsr_arch as A
    cfg = reach_config()
    P = A.init_params(cfg, 0)
    g = torch.Generator().manual_seed(31)
    d = SimpleNamespace(cfg=cfg, P=P)
    d.x = (0.3 * torch.randn(ROWS, cfg.chunk, generator=g)).cuda()
    t = torch.arange(cfg.chunk) / cfg.sr
    base = sum(torch.sin(2 * math.pi * f * t + i) / (i + 1) for i, f in enumerate((110.0, 440.0, 1234.0, 5000.0, 9000.0)))
    base = 0.5 * base / base.abs().max() + 0.02 * torch.randn(cfg.chunk, generator=g)
    d.x_lev = torch.stack([base, 1e-2 * base, 1e-4 * base, torch.zeros_like(base)]).float().cuda()      # 0 dB, -40 dB, -80 dB, silence
    d.x_lev2 = d.x_lev.clone()
    d.x_lev2[1:] = (0.3 * torch.randn(ROWS - 1, cfg.chunk, generator=g)).cuda()
    d.ids = torch.tensor([3, 4, 5, 6], dtype=torch.int64, device="cuda")
    with built(cfg, P, V()) as e:
        d.nz = e.noise(ROWS, d.ids, SEED)
        d.fwd, d.inf = profiles(e, d)
        d.flags = e.handle_flags()
        d.y_fwd = e.c_forward(d.x, d.nz).cpu()
    d.is3x3 = is3x3_name(cfg)
    d.f64 = {}
    d.y64 = f64_forward_on_gpu(d.x.cpu(), nchw(d.nz.cpu()), P, cfg, d.f64)
    d.f64 = {k: d.f64[k].cpu() for k in STAGES[:-1]}
    d.y64_lev = f64_forward_on_gpu(d.x_lev.cpu(), nchw(d.nz.cpu()), P, cfg)
    return d


def test_default_handle_on_the_reach_config_runs_every_path_the_flags_select(ref):
    from egregora_amd import native
    print("\ndefault handle, egr_flashsr_forward:", sorted(ref.fwd.items()))
    print("default handle, egr_flashsr_infer:", sorted(ref.inf.items()))
    assert ref.flags == 0
    for cnt in (ref.fwd, ref.inf):
        ops = [k for k in cnt if not k.startswith("k_")]
        assert ops and all(k in native.SIGNATURES for k in ops), ops          # operator launches go by the library's entry points
    # F(4x4,3x3) input and output transforms (the input transform leaves the row maxima of V in the fp16 scheme)
    assert ref.fwd.get("egr_winograd4_input", 0) > 0 and ref.fwd.get("egr_winograd4_output_ra", 0) > 0
    assert ref.inf.get("egr_winograd4_input_ra", 0) > 0 and ref.inf.get("egr_winograd4_output_ra", 0) > 0
    assert launches(ref.fwd, "egr_winograd_*") == 0 and launches(ref.inf, "egr_winograd_*") == 0      # no F(2x2): every image is a multiple of 4
    # GroupNorm statistics out of the partials the output transform left
    assert ref.fwd.get("egr_groupnorm_stats_from_partials", 0) > 0 and ref.inf.get("egr_groupnorm_stats_from_partials", 0) > 0
    # a fused GroupNorm consumer: coefficients only (gn_coeff), applied by the next input transform; every res-block norm goes this way, so
    # more norms are fused than applied as a pass
    fused = launches(ref.fwd, "egr_groupnorm_coeff") + ref.fwd.get("egr_groupnorm_coeff_from_stats", 0)
    assert fused > ref.fwd.get("egr_groupnorm_nhwc_ra", 0) > 0
    # the input-stationary 3x3 with the GroupNorm in its loader, under the launcher's own name; fp16 scheme only
    assert ref.is3x3.startswith("k_conv3x3_is") and ref.inf.get(ref.is3x3, 0) > 0 and ref.is3x3 not in ref.fwd
    assert ref.inf.get("egr_gn_operand_bound", 0) == ref.inf[ref.is3x3]
    # the fused AMP unit (fp16 scheme only) and both thin-end kernels
    assert launches(ref.inf, "k_amp_unit*") > 0 and launches(ref.fwd, "k_amp_unit*") == 0
    for cnt in (ref.fwd, ref.inf):
        assert cnt.get("egr_conv_cin1", 0) > 0 and cnt.get("egr_tap_gather", 0) > 0


def check_delta(name, v, fwd, inf, ref):
    """(a) the variant's launches differ from the default's in the stated way."""
    assert (fwd, inf) != (ref.fwd, ref.inf), f"{name}: the handle launched exactly what the default handle launches"
    for walk, cnt, base in (("fwd", fwd, ref.fwd), ("inf", inf, ref.inf)):
        diff = {k: (base.get(k, 0), cnt.get(k, 0)) for k in sorted(set(base) | set(cnt)) if base.get(k, 0) != cnt.get(k, 0)}
        print(f"  {name} {walk}: launches (default, variant) that differ: {diff}")
    from egregora_amd import native
    for walk, key, rel in v.delta:
        key = ref.is3x3 if key == IS3X3 else key
        if not key.startswith("k_"):              # an operator launch: the name is an entry point (or a prefix of some) of the library
            assert any(s.startswith(key[:-1]) for s in native.SIGNATURES) if key.endswith("*") else key in native.SIGNATURES, key
        got, was = launches(inf if walk == "inf" else fwd, key), launches(ref.inf if walk == "inf" else ref.fwd, key)
        ok = {"absent": was > 0 and got == 0, "new": was == 0 and got > 0, "fewer": 0 < got < was, "more": got > was > 0,
              "same": got == was > 0}[rel]
        assert ok, f"{name}: {walk} {key} should be {rel}: default {was}, variant {got}"


@pytest.mark.parametrize("name", list(VARIANTS))
def test_variant_walk_vs_driver_float64_and_product_call(ref, name):
    from egregora_amd import native
    v, cfg = VARIANTS[name], ref.cfg
    with built(cfg, ref.P, v) as e:
        want_flags = 0
        for f in v.flags:
            want_flags |= getattr(native, f)
        assert e.handle_flags() == want_flags, (e.handle_flags(), want_flags)
        assert e.split_info()["enabled"] == v.h2
        # (b) the walker equals the Python driver on every tapped stage, and again on the reused arena
        sa, sb = {}, {}
        ya = e.forward_rows(ref.x, ref.nz, stages=sa)
        yb = e.c_forward(ref.x, ref.nz, stages=sb)
        torch.cuda.synchronize()
        for k in STAGES:
            assert torch.equal(sa[k].reshape(-1), sb[k].reshape(-1)), (name, k)
        assert torch.equal(ya, yb) and bool(torch.isfinite(yb).all())
        assert torch.equal(e.c_forward(ref.x, ref.nz), yb)
        # (a) what the flag selected
        fwd, inf = profiles(e, ref)
        print(f"\n{name}:")
        check_delta(name, v, fwd, inf, ref)
        # (c) the three-term walk against float64
        errs = {k: rel_l2(stage_nchw(sb[k]), ref.f64[k]) for k in STAGES[:-1]}
        yb = yb.cpu()
        e_y, lsd_y = rel_l2(yb, ref.y64), lsd_256(ref.y64, yb)
        print(f"  {name} forward vs float64: " + " ".join(f"{k} {x:.2e}" for k, x in errs.items()) + f" y {e_y:.2e} LSD {lsd_y:.2e} dB")
        for k, x in errs.items():
            assert x <= 2e-4, (name, k, x)
        assert e_y <= 1e-3 and lsd_y <= 0.05, (name, e_y, lsd_y)
        # (d) the product call: fp16 scheme within 2e-5 of the same handle's three-term forward (the same bits where the handle has no
        # fp16 terms), and inside the float64 bars itself
        yi = e.c_infer(ref.x, ref.ids, SEED).cpu()
        dist = float((yi - yb).double().norm() / yb.double().norm())
        e_i, lsd_i = rel_l2(yi, ref.y64), lsd_256(ref.y64, yi)
        print(f"  {name} infer: distance to forward {dist:.2e}, vs float64 y {e_i:.2e} LSD {lsd_i:.2e} dB")
        assert (0.0 < dist <= 2e-5) if v.h2 else torch.equal(yi, yb), (name, dist)
        assert e_i <= 1e-3 and lsd_i <= 0.05, (name, e_i, lsd_i)
        # (e) rows at 0 dB, -40 dB, -80 dB and silence in one pass: each row against its own float64 row, whatever produced its maxima
        yl = e.c_infer(ref.x_lev, ref.ids, SEED).cpu()
        assert bool(torch.isfinite(yl).all()), name
        rows = [rel_l2(yl[r], ref.y64_lev[r]) for r in range(ROWS - 1)]
        print(f"  {name} rows at 0 / -40 / -80 dB vs float64: " + " ".join(f"{x:.2e}" for x in rows))
        for r, x in enumerate(rows):
            assert x <= 1e-3, (name, r, x)
        y2 = e.c_infer(ref.x_lev2, ref.ids, SEED).cpu()
        assert torch.equal(y2[0], yl[0]), f"{name}: row 0 saw the other rows"


def test_fuse_gn_all_is_fuse_gn_1_on_the_handle(ref):
    """handle_flags maps only FUSE_GN = "0" to a creation flag: a handle built under "all" is the default handle."""
    with built(ref.cfg, ref.P, V(dict(FUSE_GN="all"))) as e:
        assert e.FUSE_GN == "all" and e.handle_flags() == 0
        y = e.c_forward(ref.x, ref.nz).cpu()
        fwd, inf = profiles(e, ref)
    assert torch.equal(y, ref.y_fwd)
    assert (fwd, inf) == (ref.fwd, ref.inf)
