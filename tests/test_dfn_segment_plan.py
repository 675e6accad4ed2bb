"""The segment plan of the segmented DeepFilterNet pass (egr_dfn_segment_plan, dfn_engine.segment_plan) and the choice
between one pass and segments (dfn_engine.choose_path).  Host only: the library loads without a GPU."""
import itertools

import pytest

FFT_HOP = ((960, 480), (960, 240), (4096, 2048), (1024, 256))
LOOKAHEADS = (0, 2, 4)
ORDER_LOOK = ((1, 0), (3, 2), (5, 2), (7, 3))


def lengths(hop):
    return (17, 3 * hop + 17, 48000, 480001)


def seg_lengths(nF):
    return sorted({s for s in (1, 2, 7, 64, nF - 1, nF, nF + 5) if s >= 1})


def partitions(segs, kind, end):
    """The non-empty `kind` ranges follow each other from 0 to `end`; an empty one (hi <= lo) starts where the next goes on."""
    at = 0
    for s in segs:
        lo, hi = getattr(s, kind + "_lo"), getattr(s, kind + "_hi")
        if lo != at:
            return False
        at = max(at, hi)
    return at == end


@pytest.mark.parametrize("fft,hop", FFT_HOP)
@pytest.mark.parametrize("la", LOOKAHEADS)
def test_ranges_partition_their_axes_and_cover_what_a_segment_reads(pack, fft, hop, la):
    from egregora_amd import dfn_engine as E
    ov = fft // hop
    for (order, look), n in itertools.product(ORDER_LOOK, lengths(hop)):
        nF = (n + fft) // hop
        for S in seg_lengths(nF):
            count = E.segment_count(fft, hop, n, S)
            segs = [E.segment_plan(fft, hop, la, order, look, n, S, i) for i in range(count)]
            what = (fft, hop, la, order, look, n, S)
            assert partitions(segs, "net", nF) and partitions(segs, "scan", nF) and partitions(segs, "asm", nF), what
            assert partitions(segs, "out", n), what
            assert all(s.net_hi - s.net_lo == S for s in segs[:-1]) and 1 <= segs[-1].net_hi - segs[-1].net_lo <= S, what
            for j, s in enumerate(segs):
                last = j == len(segs) - 1
                if not last:
                    assert s.asm_hi + look <= s.net_hi, (what, j)
                    assert s.out_hi <= max(0, s.asm_hi - ov + 1) * hop, (what, j)
                assert s.spec_lo <= max(0, s.asm_lo - (order - 1 - look)), (what, j)
                assert s.spec_hi >= max(s.scan_hi, min(nF, s.asm_hi + look)), (what, j)
                assert 0 <= s.spec_lo < s.spec_hi <= nF, (what, j)
                # what the workspace of a segment is sized for
                assert s.spec_hi - s.spec_lo <= S + la + order - 1 and s.asm_hi - s.asm_lo <= S + look, (what, j)
                assert s.net_lo <= s.net_hi and s.scan_lo <= s.scan_hi and s.out_lo <= s.out_hi, (what, j)   # only asm may run backwards
                # the carried rows reach back far enough: mask order - 1 rows, coefficients `look` rows, frames ov - 1
                assert s.asm_lo - (order - 1 - look) >= s.net_lo - (order - 1) and s.asm_lo >= s.net_lo - look, (what, j)
                if s.out_hi > s.out_lo:
                    assert (s.out_lo + fft - hop) // hop - (ov - 1) >= s.asm_lo - (ov - 1), (what, j)
                    assert min(nF - 1, (s.out_hi - 1 + fft - hop) // hop) < s.asm_hi, (what, j)


@pytest.mark.parametrize("fft,hop", FFT_HOP)
def test_python_plan_equals_the_exported_plan(pack, fft, hop):
    from egregora_amd import dfn_engine as E
    for la, (order, look), n in itertools.product(LOOKAHEADS, ORDER_LOOK, lengths(hop)):
        nF = (n + fft) // hop
        for S in seg_lengths(nF):
            count = E.segment_count(fft, hop, n, S)
            for i in sorted({0, 1, 2, count // 2, count - 3, count - 2, count - 1} & set(range(count))):
                got, cnt = E.segment_plan_c(fft, hop, la, order, look, n, S, i)
                assert cnt == count and got == E.segment_plan(fft, hop, la, order, look, n, S, i), (fft, hop, la, order, look, n, S, i)


def test_plan_refuses_bad_arguments(pack):
    import ctypes as C
    from egregora_amd import dfn_engine as E, native
    lib = native.lib()
    cnt = C.c_int64()
    sc = E.SegmentC()
    assert lib.egr_dfn_segment_plan(960, 480, 2, 5, 2, 48000, 64, 0, None, C.byref(cnt)) == 0 and cnt.value == 2
    assert lib.egr_dfn_segment_plan(960, 480, 2, 5, 2, 48000, 0, 0, C.byref(sc), None) != 0          # seg_frames < 1
    assert lib.egr_dfn_segment_plan(960, 480, 2, 5, 2, 48000, 64, 2, C.byref(sc), None) != 0         # no such segment
    assert lib.egr_dfn_segment_plan(960, 480, 2, 5, 5, 48000, 64, 0, C.byref(sc), None) != 0         # lookahead >= order
    for bad in (dict(seg_frames=0), dict(index=2), dict(df_lookahead=5)):
        kw = dict(fft_size=960, hop_size=480, conv_lookahead=2, df_order=5, df_lookahead=2, n=48000, seg_frames=64, index=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            E.segment_plan(**kw)


def test_choose_path(pack):
    from egregora_amd import dfn_engine as E
    per_frame = 1000

    def bytes_for(s):
        return 5000 + per_frame * s

    # under budget: one pass
    assert E.choose_path(1000, bytes_for(1000), 2 * bytes_for(1000), bytes_for) is None
    assert E.choose_path(1000, bytes_for(1000), bytes_for(1000), bytes_for) is None
    # over budget: the largest multiple of 64 frames that fits
    for budget in (bytes_for(1000) - 1, bytes_for(64), bytes_for(64) + 1, bytes_for(128) - 1, 400000, 777777):
        s = E.choose_path(1000, bytes_for(1000), budget, bytes_for)
        assert s is not None and s >= 64 and s % 64 == 0 and bytes_for(s) <= budget < bytes_for(s + 64), (budget, s)
    # more frames than one pass takes: segments, whatever the budget
    long_nF = E.ONE_PASS_MAX_FRAMES + 1
    s = E.choose_path(long_nF, 0, 10 ** 18, bytes_for)
    assert s is not None and s % 64 == 0 and 64 <= s <= E.ONE_PASS_MAX_FRAMES
    s = E.choose_path(long_nF, 0, 300000, bytes_for)
    assert s == 256 and bytes_for(s) <= 300000 < bytes_for(s + 64)
    assert E.choose_path(E.ONE_PASS_MAX_FRAMES, 10, 10 ** 18, bytes_for) is None
    # not even 64 frames fit
    with pytest.raises(RuntimeError, match="EGREGORA_DFN_WORKSPACE_GB"):
        E.choose_path(1000, bytes_for(1000), bytes_for(64) - 1, bytes_for)


def test_workspace_budget_comes_from_the_environment(pack, monkeypatch):
    from egregora_amd import dfn_engine as E
    monkeypatch.delenv(E.WORKSPACE_GB_ENV, raising=False)
    assert E.workspace_budget_bytes() == 64 * 2 ** 30
    monkeypatch.setenv(E.WORKSPACE_GB_ENV, "0.5")
    assert E.workspace_budget_bytes() == 2 ** 29


def test_new_symbols_have_signatures(pack):
    from egregora_amd import native
    for name in ("egr_dfn_segment_plan",
                 "egr_dfn3_enhance_segmented", "egr_dfn3_segment_workspace_bytes", "egr_dfn3_workspace_held",
                 "egr_dfn2_enhance_segmented", "egr_dfn2_segment_workspace_bytes", "egr_dfn2_workspace_held"):
        assert name in native.SIGNATURES and hasattr(native.lib(), name), name
    assert native.lib().egr_abi_version() == 5
