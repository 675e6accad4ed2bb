"""The segment plan of the segmented Descript Audio Codec (egr_dacseg_plan, dac_engine.segment_plan), the
exactness in float64 of a walk cut by that plan (tests/dac_torch.py on the plan's windows against one pass), and the choice between
one pass and segments (dac_engine.choose_path).  Host only: the library loads without a GPU."""
import functools

import pytest
import torch

import dac_check as K
import dac_torch as R

CONFIGS = ("S", "O", "G", "W", "T", "C")
EXACT = 1e-12                                # of the one-pass rms; the cut is exact, the figure seen was 0.0


def hop_of(cfg, kind):
    h = 1
    for s in cfg["encoder_rates" if kind == 0 else "decoder_rates"]:
        h *= s
    return h


def plan_lengths(cfg):
    h = R.hop(cfg)
    return sorted({1, h - 1, h, h + 1, 1003, 2051})


def seg_lengths(F):
    return sorted({s for s in (1, 3, 16, 64, F - 1, F, F + 5) if s >= 1})


@functools.lru_cache(maxsize=None)
def own_margins(name, kind):
    """The test's own backward walk, on index sets, not on a hull: the input positions that the outputs of one frame far from both
    ends depend on, layer by layer from the output back.  Returns the frames needed (left, right) of that frame."""
    cfg = R.config(name)
    per, base = hop_of(cfg, kind), 1000
    rates = cfg["encoder_rates"] if kind == 0 else cfg["decoder_rates"]
    unit = [("c", 7, 1, d, 3 * d) for d in R.DILATIONS]
    if kind == 0:
        layers = [("c", 7, 1, 1, 3)]
        for s in rates:
            layers += [u for u in unit] + [("c", 2 * s, s, 1, -(-s // 2))]          # (the k = 1 convolutions reach nowhere)
        layers += [("c", 3, 1, 1, 1)]
        need = {base}
    else:
        layers = [("c", 7, 1, 1, 3)]
        for s in rates:
            layers += [("t", 2 * s, s, 1, -(-s // 2))] + [u for u in unit]
        layers += [("c", 7, 1, 1, 3)]
        need = set(range(base * per, (base + 1) * per))
    for typ, k, s, d, p in reversed(layers):
        nxt = set()
        for o in need:
            for t in range(k):
                if typ == "c":
                    nxt.add(o * s - p + t * d)
                elif (o + p - t) % s == 0:                  # j = i s - p + t
                    nxt.add((o + p - t) // s)
        need = nxt
    if kind == 0:                                           # samples -> frames: frame f owns samples [f per, (f + 1) per)
        return base - min(need) // per, max(need) // per - base
    return base - min(need), max(need) - base


def partitions(segs, kind, end):
    at = 0
    for s in segs:
        lo, hi = getattr(s, kind + "_lo"), getattr(s, kind + "_hi")
        if lo != at or hi < lo:
            return False
        at = hi
    return at == end


@pytest.mark.parametrize("name", CONFIGS)
def test_own_margins_are_the_issue_s_figures_and_the_engine_s(pack, name):
    from egregora_amd import dac_engine as E
    known = {"S": (17, 19), "O": (14, 16), "G": (22, 24), "W": (8, 10)}
    enc, dec = own_margins(name, 0), own_margins(name, 1)
    assert enc[0] == enc[1] and dec[0] == dec[1]
    if name in known:
        assert (enc[0], dec[0]) == known[name]
    cfg = R.config(name)
    for kind, own in ((E.ENCODE, enc), (E.DECODE, dec)):
        got = E.segment_margins(cfg, kind)
        assert got[0] >= own[0] and got[1] >= own[1], (name, kind, got, own)


@pytest.mark.parametrize("name", CONFIGS)
def test_plan_ranges(pack, name):
    from egregora_amd import dac_engine as E
    cfg = R.config(name)
    for n in plan_lengths(cfg):
        n_pad, F, n_dec = E.lengths(cfg, n)
        for kind, length in ((E.ENCODE, n), (E.DECODE, F)):
            ml, mr = own_margins(name, kind)
            per = hop_of(cfg, kind)
            for S in seg_lengths(F):
                what = (name, n, kind, S)
                count = E.segment_count(cfg, kind, length, S)
                assert count == -(-F // S), what
                segs = [E.segment_plan(cfg, kind, length, S, i) for i in range(count)]
                for i, s in enumerate(segs):
                    got, cnt = E.segment_plan_c(cfg, kind, length, S, i)
                    assert cnt == count and got == s, (what, i, got, s)
                    assert (s.keep_lo, s.keep_hi) == (i * S, min(F, (i + 1) * S)), (what, i)
                    assert 0 <= s.win_lo <= s.keep_lo < s.keep_hi <= s.win_hi <= F, (what, i)
                    assert s.win_lo <= max(0, s.keep_lo - ml) and s.win_hi >= min(F, s.keep_hi + mr), (what, i)
                    assert s.win_hi - s.win_lo <= (S + 2 * max(E.segment_margins(cfg, kind)) + E.SEGMENT_ALIGN - 1) // E.SEGMENT_ALIGN * E.SEGMENT_ALIGN
                    if s.win_lo > 0 and s.win_hi < F:
                        assert (s.win_hi - s.win_lo) % E.SEGMENT_ALIGN == 0, (what, i)
                    if kind == E.ENCODE:
                        assert (s.in_lo, s.in_hi) == (s.win_lo * per, min(n, s.win_hi * per)) and (s.out_lo, s.out_hi) == (s.keep_lo, s.keep_hi), (what, i)
                    else:
                        assert (s.in_lo, s.in_hi) == (s.win_lo, s.win_hi), (what, i)
                        assert s.out_lo == s.keep_lo * per and s.out_hi == (n_dec if i == count - 1 else s.keep_hi * per), (what, i)
                        # the window's own decoded length holds what it stores
                        assert s.out_hi - s.win_lo * per <= E.decoded_length(cfg, s.win_hi - s.win_lo), (what, i)
                assert partitions(segs, "keep", F), what
                assert partitions(segs, "out", F if kind == E.ENCODE else n_dec), what


def test_plan_refuses_bad_arguments(pack):
    import ctypes as C
    from egregora_amd import dac_engine as E, native
    cfg = R.config("S")
    cc, sc, cnt = E.config_c(cfg), E.SegmentC(), C.c_int64()
    lib = native.lib()
    assert lib.egr_dacseg_plan(C.byref(cc), E.ENCODE, 2051, 64, 0, None, C.byref(cnt)) == 0 and cnt.value == 5
    assert lib.egr_dacseg_plan(C.byref(cc), E.ENCODE, 2051, 0, 0, C.byref(sc), None) != 0          # seg_frames < 1
    assert lib.egr_dacseg_plan(C.byref(cc), E.ENCODE, 2051, 64, 5, C.byref(sc), None) != 0         # no such segment
    assert lib.egr_dacseg_plan(C.byref(cc), 2, 2051, 64, 0, C.byref(sc), None) != 0                # no such kind
    assert lib.egr_dacseg_plan(C.byref(cc), E.DECODE, 0, 64, 0, C.byref(sc), None) != 0            # no frames
    for bad in (dict(seg_frames=0), dict(index=5), dict(kind=2), dict(length=0)):
        kw = dict(cfg=cfg, kind=E.ENCODE, length=2051, seg_frames=64, index=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            E.segment_plan(**kw)


@pytest.mark.parametrize("n", [1003, 2051])
@pytest.mark.parametrize("name", ["S", "O", "G"])
def test_a_float64_walk_cut_by_the_plan_is_one_pass(pack, name, n):
    from egregora_amd import dac_engine as E
    cfg, sd, n64, _ = K.model(name)
    f = K.forward(name, n)
    x = f["x"].double()
    ze_one, z_in, y_one = f["enc64"][-1], f["zin"].double(), f["y64"]
    n_pad, F, n_dec = E.lengths(cfg, n)
    H = hop_of(cfg, 1)
    assert ze_one.shape[-1] == F and y_one.shape[-1] == n_dec
    with torch.no_grad():
        for S in seg_lengths(F):
            ze = torch.full_like(ze_one, float("nan"))
            y = torch.full_like(y_one, float("nan"))
            for i in range(E.segment_count(cfg, E.ENCODE, n, S)):
                s = E.segment_plan(cfg, E.ENCODE, n, S, i)
                w = n64.encode_stages(x[:, s.in_lo:s.in_hi])[-1]
                assert w.shape[-1] == s.win_hi - s.win_lo
                ze[:, :, s.out_lo:s.out_hi] = w[:, :, s.keep_lo - s.win_lo:s.keep_hi - s.win_lo]
                d = E.segment_plan(cfg, E.DECODE, F, S, i)
                yw = n64.decode_stages(z_in[:, :, d.in_lo:d.in_hi])[1]
                y[:, d.out_lo:d.out_hi] = yw[:, d.out_lo - d.win_lo * H:d.out_hi - d.win_lo * H]
            e_enc = float((ze - ze_one).norm() / ze_one.norm())
            e_dec = float((y - y_one).norm() / y_one.norm())
            print(f"  {name} n {n} seg_frames {S}: encoder {e_enc:.1e}  decoder {e_dec:.1e}")
            assert e_enc <= EXACT and e_dec <= EXACT, (name, n, S, e_enc, e_dec)


def test_choose_path(pack, monkeypatch):
    from egregora_amd import dac_engine as E
    step, per_frame = E.SEGMENT_STEP, 1000

    def bytes_for(s):
        return 5000 + per_frame * s

    frames = 10 * step + 7
    one = bytes_for(frames) * 3
    # within the budget: one pass, whatever segments would cost
    assert E.choose_path(frames, one, one, bytes_for) is None and E.choose_path(frames, one, 2 * one, bytes_for) is None
    # above it: the largest multiple of the step that fits, at most the first that covers the frames
    for budget in (one - 1, bytes_for(step), bytes_for(step) + 1, bytes_for(2 * step) - 1, bytes_for(7 * step) + 3):
        s = E.choose_path(frames, one, budget, bytes_for)
        assert s is not None and s >= step and s % step == 0 and bytes_for(s) <= budget, (budget, s)
        assert s == 11 * step or budget < bytes_for(s + step), (budget, s)
    assert E.choose_path(frames, one, one - 1, bytes_for) == 11 * step
    assert E.choose_path(3, 10 ** 9, bytes_for(step), bytes_for) == step
    # not even one step fits: the error names the variable and its value, in the format of the one-pass refusal
    monkeypatch.setenv(E.WORKSPACE_GB_ENV, "1e-6")
    with pytest.raises(RuntimeError, match=r"EGREGORA_DAC_WORKSPACE_GB = 1e-06"):
        E.choose_path(frames, one, bytes_for(step) - 1, bytes_for)


def test_workspace_budget_comes_from_the_environment(pack, monkeypatch):
    from egregora_amd import dac_engine as E
    monkeypatch.delenv(E.WORKSPACE_GB_ENV, raising=False)
    assert E.workspace_budget_bytes() == 64 * 2 ** 30
    monkeypatch.setenv(E.WORKSPACE_GB_ENV, "0.5")
    assert E.workspace_budget_bytes() == 2 ** 29


def test_new_symbols_have_signatures(pack):
    from egregora_amd import native
    for name in ("egr_dacseg_plan", "egr_dacseg_encode", "egr_dacseg_decode", "egr_dacseg_workspace_bytes",
                 "egr_dacseg_workspace_held", "egr_dacseg_from_codes"):
        assert name in native.SIGNATURES and hasattr(native.lib(), name), name
    assert native.lib().egr_abi_version() == 5
