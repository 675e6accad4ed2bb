"""The FlashSR handle's opt-in fast mode (EGR_FSR_FAST_F16 / EGREGORA_FLASHSR_SPLIT=f16x1 / egr_flashsr_set_split 3 and 4: one fp16
term per operand where the default runs two), on the reach configuration of tests/test_gpu_flashsr_flags.py -- tiny_config() with
n_mels = 128, Winograd threshold 32, four rows, chunk 3840 -- whose helpers are imported, not copied.

What ran is read from the handle's own profile (level 2): every `..., 1>` contraction launch of the default handle has a `..., 2>`
twin with the same count (but for the one instantiation whose one-term form measured no faster, KEPT_ON_TWO_TERMS: the mode keeps it
on two terms), the input-stationary 3x3 shows as k_conv3x3_isp<..., 2>, and everything else -- the fused AMP unit, the
thin-end operators, every other operator launch -- has the same name and count.  Switching 1 -> 3 -> 1 on a live handle needs no
repacking and leaves no trace; the mode is as pure a function of (weights, row, seed, row id) as the default.

Accuracy against the float64 run of the same graph is MEASURED, per stage (egr_flashsr_forward under set_split 4) and on the waveform,
for noise seeds 11, 12 and 13; each bar below is three times the largest of the three measurements (profiles/flashsr_fast.md holds
them next to the default handle's): the error is rounding noise whose seed-to-seed spread is small, a scale or plane mistake is
orders above.  The waveform error of the mode must also come out ABOVE the default handle's, which shows the assertion is looking
at the mode and not at scheme 1.  The mel stage comes from kernels the mode does not touch: the default handle's bits."""
import math
from types import SimpleNamespace

import pytest
import torch

from test_gpu_flashsr import f64_forward_on_gpu, nchw, rel_l2
from test_gpu_flashsr_flags import ROWS, SEED, STAGES, V, built, counts, lsd_256, reach_config, stage_nchw

pytestmark = pytest.mark.gpu

SEEDS = (11, 12, 13)
FAST = V(dict(SPLIT="f16x1"), flags=("FSR_FAST_F16",))
FAST_ENV = V(env={"EGREGORA_FLASHSR_SPLIT": "f16x1"})
# 3 x the largest of the three measured values (relative L2 against float64; LSD 256 / 64 in dB): see profiles/flashsr_fast.md
MEASURED = {"z_cond": 4.77e-4, "v": 9.71e-4, "z0": 9.71e-4, "mel_hat": 1.55e-3, "y": 1.80e-3, "lsd": 5.66e-2}
BARS = {k: 3 * v for k, v in MEASURED.items()}


# measured no faster on one term than on two (profiles/flashsr_fast.md, egr::h1_pays): the mode keeps these launches on scheme 1
KEPT_ON_TWO_TERMS = ("k_conv_s3<128, 64, 1, false, 1>",)


# egr_flashsr_infer launches of the DEFAULT handle on the reach configuration, as the commit before the mode made them (recorded there
# with the same call sequence): the default walk did not move
PARENT_DEFAULT_PROFILE = {
    "egr_absmax_rows": 3, "egr_concat_channels_ra": 5, "egr_conv_cin1": 1, "egr_eltwise": 1, "egr_eltwise_ra": 3, "egr_geglu_ra": 4,
    "egr_gn_operand_bound": 6, "egr_groupnorm_coeff": 14, "egr_groupnorm_coeff_from_stats": 22, "egr_groupnorm_nhwc_ra": 9,
    "egr_groupnorm_stats_from_partials": 22, "egr_layernorm_rows_ra": 12, "egr_snake_aa_ra": 17, "egr_tap_gather": 1,
    "egr_winograd4_input_ra": 30, "egr_winograd4_output_ra": 30, "k_amp_unit<16, 240>": 4, "k_conv3x3_isp<64, 32, true, true>": 6,
    "k_conv_igemm<32, false, false>": 23, "k_conv_igemm<64, false, false>": 1, "k_conv_s3<128, 32, 1, false, 1>": 16,
    "k_conv_s3<128, 64, 1, false, 0>": 1, "k_conv_s3<128, 64, 1, false, 1>": 94}


def one_term(name):
    """The one-term twin of a contraction instantiation of the default profile (None: the mode leaves the kernel alone)."""
    if name in KEPT_ON_TWO_TERMS:
        return None
    if name.startswith(("k_conv_s3<", "k_conv1d_s3<")) and name.endswith(", 1>"):
        return name[:-2] + "2>"
    if name.startswith("k_conv3x3_isp<"):
        return name[:-1] + ", 2>"
    return None


def infer_profile(e, d):
    e.c_infer(d.x, d.ids, SEED)                   # (the second call: the scratch exists)
    return counts(e.c_profile(lambda: e.c_infer(d.x, d.ids, SEED), ops=True))


@pytest.fixture(scope="module")
def data(pack):
    from egregora_amd import flashsr_arch as A
    cfg = reach_config()
    d = SimpleNamespace(cfg=cfg, P=A.init_params(cfg, 0))
    g = torch.Generator().manual_seed(31)
    d.x = (0.3 * torch.randn(ROWS, cfg.chunk, generator=g)).cuda()
    d.ids = torch.tensor([3, 4, 5, 6], dtype=torch.int64, device="cuda")
    with built(cfg, d.P, V()) as e:
        d.default_prof = infer_profile(e, d)
        d.default_y = e.c_infer(d.x, d.ids, SEED).clone()
        d.default_info = e.split_info()
    with built(cfg, d.P, FAST) as e:
        d.fast_info, d.fast_flags = e.split_info(), e.handle_flags()
        d.fast_prof = infer_profile(e, d)
        d.fast_y = e.c_infer(d.x, d.ids, SEED).clone()
    return d


def test_mode_swaps_the_contraction_kernels_and_nothing_else(data):
    from egregora_amd import native
    d = data
    assert d.default_info["scheme"] == 1 and d.default_info["enabled"]
    twins = {k: one_term(k) for k in d.default_prof}
    print("\ndefault handle:", sorted(d.default_prof.items()))
    assert d.default_prof == PARENT_DEFAULT_PROFILE
    # the default walk does reach the kernels the mode swaps: implicit-GEMM tiles and the input-stationary 3x3
    assert sum(1 for t in twins.values() if t) >= 2, twins
    assert any(k.startswith("k_conv3x3_isp<") for k in d.default_prof) and any(k.startswith("k_conv_s3<") and k.endswith(", 1>") for k in d.default_prof)
    want = {(twins[k] or k): n for k, n in d.default_prof.items()}
    assert d.fast_flags == native.FSR_FAST_F16
    with built(d.cfg, d.P, FAST_ENV) as e:              # the environment value at creation means the same as the flag
        env_info, env_prof = e.split_info(), infer_profile(e, d)
        env_y = e.c_infer(d.x, d.ids, SEED).clone()
    for by, info, got, y in (("flag", d.fast_info, d.fast_prof, d.fast_y), ("environment", env_info, env_prof, env_y)):
        assert info["scheme"] == 3 and info["enabled"], (by, info)
        print(f"\nfast mode by {by}:", sorted(got.items()))
        assert got == want, (by, {k: (want.get(k), got.get(k)) for k in sorted(set(want) | set(got)) if want.get(k) != got.get(k)})
        assert not any(k.endswith(", 1>") and k not in KEPT_ON_TWO_TERMS for k in got if k.startswith(("k_conv_s3<", "k_conv1d_s3<")))
        assert sum(n for k, n in got.items() if k.startswith("k_amp_unit")) == sum(n for k, n in d.default_prof.items() if k.startswith("k_amp_unit")) > 0
        for op in ("egr_conv_cin1", "egr_tap_gather"):                           # the thin ends
            assert got.get(op, 0) == d.default_prof.get(op, 0) > 0, op
        assert [k for k in sorted(got) if not k.startswith("k_")] == [k for k in sorted(d.default_prof) if not k.startswith("k_")]
        assert bool(torch.isfinite(y).all()) and not torch.equal(y, d.default_y)
    assert torch.equal(env_y, d.fast_y), "flag and environment value build the same handle"


def test_flag_is_refused_next_to_the_flags_that_keep_no_fp16_terms(data):
    from egregora_amd import native
    d = data
    for other in (dict(MFMA_MODE="f32"), ):
        with pytest.raises(RuntimeError, match="EGR_FSR_FAST_F16"):
            with built(d.cfg, d.P, V(dict(SPLIT="f16x1", **other))):
                pass
    # EGR_FSR_SPLIT_BF16X3 | EGR_FSR_FAST_F16 cannot be spelled through SPLIT (one value): through the flags directly
    from egregora_amd import flashsr_engine as E
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(E.FlashSREngine, "handle_flags", lambda self: native.FSR_SPLIT_BF16X3 | native.FSR_FAST_F16)
        with pytest.raises(RuntimeError, match="EGR_FSR_FAST_F16"):
            with built(d.cfg, d.P, V()):
                pass


def test_a_live_handle_switches_between_the_schemes_without_repacking(data):
    import ctypes as C
    d = data
    with built(d.cfg, d.P, V()) as e:
        nw = e.split_info()["weights"]
        e.set_split("f16x2")
        y1 = e.c_infer(d.x, d.ids, SEED).clone()
        e.set_split("f16x1")
        assert e.split_info()["scheme"] == 3 and e.split_info()["weights"] == nw
        y3 = e.c_infer(d.x, d.ids, SEED).clone()
        e.set_split("f16x2")
        assert e.split_info()["scheme"] == 1
        y1b = e.c_infer(d.x, d.ids, SEED).clone()
        assert torch.equal(y1, y1b) and torch.equal(y1, d.default_y)
        assert torch.equal(y3, d.fast_y), "the switched handle equals the handle created with the flag, bit for bit"
        e.set_split("f16x1+forward")
        assert e.split_info()["scheme"] == 4
        e.set_split("bf16x3")
        assert e.split_info()["scheme"] == 0
        e.set_split("f16x2")
        assert e.L.egr_flashsr_set_split(C.c_void_p(e.handle), 5) == 1            # EGR_ERR_ARG
        assert e.split_info()["scheme"] == 1
    with built(d.cfg, d.P, V(dict(SPLIT="bf16x3"), flags=("FSR_SPLIT_BF16X3",))) as e:
        assert e.L.egr_flashsr_set_split(C.c_void_p(e.handle), 3) == 3            # EGR_ERR_UNSUPPORTED: no fp16 terms to run on
        assert e.split_info()["scheme"] == 0


def infer_passes(e, x, ids, rows_per_pass):
    """egr_flashsr_infer over x in passes of `rows_per_pass` rows (FlashSREngine.c_infer always asks for the engine's default)."""
    import ctypes as C
    from egregora_amd import native
    x, ids = x.contiguous(), ids.contiguous()
    y = torch.empty_like(x)
    h = C.c_void_p(e.handle)
    native.check(e.L.egr_flashsr_set_rows_per_pass(h, rows_per_pass), "egr_flashsr_set_rows_per_pass")
    native.check(e.L.egr_flashsr_infer(h, C.c_void_p(x.data_ptr()), x.shape[0], 0, SEED, C.c_void_p(ids.data_ptr()), C.c_void_p(y.data_ptr()), e._st()),
                 "egr_flashsr_infer")
    return y


def test_mode_is_a_pure_function_of_its_rows(data):
    """A row's bits depend on (weights, that row, seed, row id): not on the other rows of the call, on pass boundaries, on row groups
    running concurrently, or on the handle's history.  As in the default mode, the launcher's choices follow the row count of a FORWARD
    (four rows of the reach configuration are the 512 tiles the input-stationary 3x3 wants, one or two rows take the Winograd path
    instead), so the calls compared here run forwards of equal size: the four rows in ONE call in passes of one row against each row
    alone, and in passes of two rows against two calls of two rows."""
    import ctypes as C
    from egregora_amd import native
    d = data
    with built(d.cfg, d.P, FAST) as e:
        y = e.c_infer(d.x, d.ids, SEED).clone()
        assert torch.equal(y, d.fast_y)                                           # another handle, the same bits
        assert torch.equal(e.c_infer(d.x, d.ids, SEED), y)                        # a repeat
        x2 = d.x.clone()                                                          # the other rows of the call do not matter
        x2[1] *= 1e-4
        x2[2] = 0.0
        x2[3] *= 50.0
        y2 = e.c_infer(x2, d.ids, SEED)
        assert torch.equal(y2[0], y[0]) and not torch.equal(y2[1], y[1]) and bool(torch.isfinite(y2).all())
        y_by1 = infer_passes(e, d.x, d.ids, 1)                                    # rows a, b, c, d in one call ...
        for r in range(ROWS):                                                     # ... against each row alone
            assert torch.equal(infer_passes(e, d.x[r:r + 1], d.ids[r:r + 1], ROWS)[0], y_by1[r]), r
        y_by2 = infer_passes(e, d.x, d.ids, 2)
        for lo in (0, 2):                                                         # ... and against two calls of two rows
            assert torch.equal(infer_passes(e, d.x[lo:lo + 2], d.ids[lo:lo + 2], ROWS), y_by2[lo:lo + 2]), lo
        print("\nfour-row forward against four one-row forwards, relative distance per row (kernel choices follow a forward's row count):",
              [f"{float((y[r] - y_by1[r]).norm() / y[r].norm()):.1e}" for r in range(ROWS)])
        # history: a loud call, silence and another seed in between change nothing
        e.c_infer(300.0 * d.x, d.ids, SEED)
        e.c_infer(torch.zeros_like(d.x), d.ids, SEED + 1)
        assert torch.equal(e.c_infer(d.x, d.ids, SEED), y)
        # two concurrent row groups of two rows (side streams) against the same two forwards one after the other
        native.check(e.L.egr_flashsr_set_streams(C.c_void_p(e.handle), 2, 2), "egr_flashsr_set_streams")
        y_groups = infer_passes(e, d.x, d.ids, ROWS)
        native.check(e.L.egr_flashsr_set_streams(C.c_void_p(e.handle), 1, 2), "egr_flashsr_set_streams")
        assert torch.equal(y_groups, y_by2)
        assert torch.equal(infer_passes(e, d.x, d.ids, ROWS), y)


def test_mode_accuracy_against_float64_stage_by_stage(data):
    d = data
    cfg = d.cfg
    worst = {k: 0.0 for k in BARS}
    worst_default = {k: 0.0 for k in BARS}
    with built(cfg, d.P, V()) as e:
        for seed in SEEDS:
            nz = e.noise(ROWS, d.ids, seed)
            f64 = {}
            y64 = f64_forward_on_gpu(d.x.cpu(), nchw(nz.cpu()), d.P, cfg, f64)
            out = {}
            for mode in ("f16x2+forward", "f16x1+forward"):
                e.set_split(mode)
                st = {}
                y = e.c_forward(d.x, nz, stages=st).cpu()
                errs = {k: rel_l2(stage_nchw(st[k]), f64[k].cpu()) for k in STAGES[1:-1]}
                errs["y"], errs["lsd"] = rel_l2(y, y64), lsd_256(y64, y)
                out[mode] = (errs, st["mel"].clone(), y)
            e2, e1 = out["f16x2+forward"][0], out["f16x1+forward"][0]
            print(f"\nseed {seed} vs float64 (default | fast mode | bar): " +
                  "  ".join(f"{k} {e2[k]:.2e} | {e1[k]:.2e} | {BARS[k] or float('nan'):.2e}" for k in BARS))
            assert torch.equal(out["f16x2+forward"][1], out["f16x1+forward"][1]), "the mel stage is not the mode's: the default handle's bits"
            assert e1["y"] > e2["y"] and e1["lsd"] > e2["lsd"], (seed, "the assertion is looking at scheme 1, not at the mode", e1, e2)
            for k in BARS:
                worst[k], worst_default[k] = max(worst[k], e1[k]), max(worst_default[k], e2[k])
    print("largest of the three seeds, fast mode:", {k: f"{v:.2e}" for k, v in worst.items()})
    print("largest of the three seeds, default  :", {k: f"{v:.2e}" for k, v in worst_default.items()})
    for k in BARS:
        assert BARS[k] is not None and worst[k] <= BARS[k], (k, worst[k], BARS[k])
