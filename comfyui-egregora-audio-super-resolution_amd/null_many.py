"""Many (reference, processed) pairs through the null-test suite at once.

Per pair delays_many / align_many / gain_match_many / null_test_many / full_many are what `Audio Align (XCorr)`, `Audio Gain Match`,
`Audio Null Test` and `Null Test (Full)` compute (egregora_null_test_suite.py), but a WAVE of pairs is a handful of library calls
whose number depends on how many transform lengths and (sample rate, channels) groups the wave holds, never on the number of pairs:

    egr_nullmany_delays     one per transform length: pack (with the mono downmix), the GCC-PHAT passes over all rows, one peak search
    egr_nullmany_shift_fir  one: every (pair, channel) row's shift + fractional FIR
    egr_loudness_tracks     one per (rate, channels) group: the K-weighted 400 ms block energies (LUFS levels; once more for the nulls)
    egr_nullmany_mix        gain, null mix and all sums in one pass (once more before it for a least-squares k or RMS levels)
    egr_metrics_pairs       one: the log-spectral distance

The host blocks once per stage for a wave's lags, levels, sums and LSD values and finishes every number with the single path's own
expressions (device_ops.xcorr_refine / lufs_gate / lsd_finish, egregora_null_test_suite.delay_rule / corr_finish).  Host tensors go up
one by one, tensors already on the device are addressed where they lie (eval_many).  compute_hf_residual needs a transform at each
null's own length and a processed side at another rate a resample of its own: both stay one single-path call per pair and are counted
in stats["per_pair_calls"].
"""
import ctypes as C
import math
from collections import OrderedDict
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import device_ops, eval_many, loudness, native
from .egregora_null_test_suite import corr_finish, delay_rule

TILE, MAX_GROUP_ROWS = 256, 65535          # NULL_TILE, NULL_MAX_GROUP_ROWS (csrc/egr_null_index.h)
_PLANS: "OrderedDict[tuple, int]" = OrderedDict()         # (n, device) -> a one-channel plan for 2 n samples; the rows live in the call's workspace
_MAX_PLANS = 8                                            # the many-path's own cache: a corpus run never evicts fatllama_engine._PLANS
STAT_KEYS = ("waves", "library_calls", "launches", "host_reads", "transform_groups", "level_groups", "per_pair_calls")


def _stats(stats: Optional[dict]):
    if stats is not None:
        stats.update({k: 0 for k in STAT_KEYS})


def _bump(stats: Optional[dict], **kw):
    if stats is not None:
        for k, v in kw.items():
            stats[k] = stats.get(k, 0) + int(v)


def _tab(rows):
    flat = [int(v) for r in rows for v in r]
    return (C.c_int64 * len(flat))(*flat)


def _refused(what: str):
    return RuntimeError(f"{what} refused: {native.last_error()}")


def _ws(need: int, device) -> torch.Tensor:
    return torch.empty((max(int(need), 16),), dtype=torch.uint8, device=device)


def transform_length(n_common: int) -> int:
    """The single path's rule with both sides cut to the common length: a total that IS a power of two stays at that length."""
    return device_ops.xcorr_transform_length(int(n_common), int(n_common))


def transform_groups(common_lengths: Sequence[int]) -> "OrderedDict[int, List[int]]":
    """transform length -> the pairs that share it, in input order.  Host only."""
    groups: "OrderedDict[int, List[int]]" = OrderedDict()
    for i, nc in enumerate(common_lengths):
        groups.setdefault(transform_length(nc), []).append(i)
    return groups


def level_groups(keys: Sequence[tuple]) -> "OrderedDict[tuple, List[int]]":
    """(sample rate, channels) -> the clips that share it, in input order.  Host only."""
    groups: "OrderedDict[tuple, List[int]]" = OrderedDict()
    for i, k in enumerate(keys):
        groups.setdefault((int(k[0]), int(k[1])), []).append(i)
    return groups


def max_shift_samples(sr: int, max_shift_ms) -> int:
    return int(sr * (max_shift_ms / 1000.0))


def _plan(n: int, device: int) -> int:
    key = (int(n), int(device))
    h = _PLANS.get(key)
    if h is not None:
        _PLANS.move_to_end(key)
        return h
    out = C.c_void_p()
    native.check(native.lib().egr_fatllama_plan_create(C.byref(out), 2 * int(n), 1, 1, 0, 0), "egr_fatllama_plan_create")
    _PLANS[key] = out.value
    while len(_PLANS) > _MAX_PLANS:
        _, old = _PLANS.popitem(last=False)
        native.lib().egr_fatllama_plan_destroy(C.c_void_p(old))
    return out.value


def release_plans():
    while _PLANS:
        _, old = _PLANS.popitem(last=False)
        native.lib().egr_fatllama_plan_destroy(C.c_void_p(old))


def pair_bytes(ca: int, ta: int, cb: int, tb: int, n_fft: int = 2048, hop: int = 512) -> int:
    """Device bytes one pair needs by itself, an upper bound: both sides, the aligned / matched / null / scaled outputs, its rows of the
    transform group (z, the correlation and the passes' state: 24 n bytes, egr_nullmany_delays_workspace_bytes), the K-weighted mono
    signals of the loudness calls and the metrics workspace."""
    nc = min(ta, tb)
    n = transform_length(nc)
    ws = int(native.lib().egr_nullmany_delays_workspace_bytes(_tab([(0, ca, ta, 0, cb, tb, nc, 0)]), 1, n))
    if ws == 0:
        raise _refused("egr_nullmany_delays")
    return 4 * (ca * ta + cb * tb) + 4 * 4 * cb * ta + ws + 3 * 4 * ta + eval_many.pair_bytes(ca, ta, cb, ta, n_fft, hop, device_ops.METRICS_LSD)


def pair_work(ta: int, tb: int, n_fft: int = 2048, hop: int = 512) -> int:
    """The most workgroups one pair adds to any grid of a wave: pack tiles of its transform row, or the metrics call's frames."""
    return max(transform_length(min(ta, tb)) // TILE, eval_many.pair_work(ta, ta, n_fft, hop))


# ------------------------------------------------------------------------------------------------ the stages on device tensors
def _delays(xr: List[torch.Tensor], xp: List[torch.Tensor], max_shifts: Sequence[int], stats=None, raw: Optional[list] = None) -> List[float]:
    """Lags of xp[i] against xr[i] ([C,T] float32 CUDA tensors, common length = the shorter side) -> samples, quirk Q8 included.
    raw, when given, receives every pair's four floats of egr_gcc_phat (host tensors)."""
    P = len(xr)
    dev = xr[0].device
    base, offs = loudness.flat_offsets(list(xr) + list(xp))
    nc = [min(a.shape[1], b.shape[1]) for a, b in zip(xr, xp)]
    out4 = torch.empty((P, 4), dtype=torch.float32, device=dev)
    L = native.lib()
    slot, where = 0, [0] * P
    hold = []
    for n, idx in transform_groups(nc).items():
        plan = _plan(n, dev.index or 0)
        for s in range(0, len(idx), MAX_GROUP_ROWS):
            part = idx[s:s + MAX_GROUP_ROWS]
            rows = [(offs[i], xr[i].shape[0], xr[i].shape[1], offs[P + i], xp[i].shape[0], xp[i].shape[1], nc[i], int(max_shifts[i])) for i in part]
            tab = _tab(rows)
            need = int(L.egr_nullmany_delays_workspace_bytes(tab, len(part), n))
            if need == 0:
                raise _refused("egr_nullmany_delays")
            ws = _ws(need, dev)
            hold.append(ws)
            launches = C.c_int(0)
            native.check(L.egr_nullmany_delays(C.c_void_p(plan), C.c_void_p(base), C.c_void_p(base), tab, len(part),
                                               C.c_void_p(out4.data_ptr() + 16 * slot), native.ptr(ws), need, C.byref(launches),
                                               native.stream_ptr()), "egr_nullmany_delays")
            for j, i in enumerate(part):
                where[i] = slot + j
            slot += len(part)
            _bump(stats, library_calls=1, launches=launches.value, transform_groups=1)
    host = out4.cpu()
    _bump(stats, host_reads=1)
    if raw is not None:
        raw.extend(host[where[i]].clone() for i in range(P))
    return [device_ops.xcorr_refine(host[where[i]], transform_length(nc[i])) for i in range(P)]


def _shift_fir(xs: List[torch.Tensor], delays: Sequence[float], taps: int, n_outs: Sequence[int], stats=None):
    """apply_delay for many [C,N] CUDA tensors in one launch -> [C, n_out] tensors (views of one buffer)."""
    dev = xs[0].device
    base, offs = loudness.flat_offsets(xs)
    rule = [delay_rule(float(d), taps, x.shape[1]) for x, d in zip(xs, delays)]
    with_taps = [i for i, (_, hh) in enumerate(rule) if hh is not None]
    m = rule[with_taps[0]][1].size if with_taps else 0
    tap_row = {i: r for r, i in enumerate(with_taps)}
    taps_dev = torch.from_numpy(np.stack([rule[i][1] for i in with_taps])).to(dev) if with_taps else None
    out_off, pos = [], 0
    for x, n_out in zip(xs, n_outs):
        out_off.append(pos)
        pos += x.shape[0] * int(n_out)
    y = torch.empty((pos,), dtype=torch.float32, device=dev)
    rows = []
    for i, x in enumerate(xs):
        for c in range(x.shape[0]):
            rows.append((offs[i] + c * x.shape[1], x.shape[1], rule[i][0], tap_row.get(i, -1), out_off[i] + c * int(n_outs[i]), int(n_outs[i])))
    tab = _tab(rows)
    L = native.lib()
    need = int(L.egr_nullmany_shift_fir_workspace_bytes(tab, len(rows), len(with_taps), m))
    if need == 0:
        raise _refused("egr_nullmany_shift_fir")
    ws = _ws(need, dev)
    launches = C.c_int(0)
    native.check(L.egr_nullmany_shift_fir(C.c_void_p(base), tab, len(rows), native.ptr(taps_dev) if taps_dev is not None else None,
                                          len(with_taps), m, native.ptr(y), native.ptr(ws), need, C.byref(launches),
                                          native.stream_ptr()), "egr_nullmany_shift_fir")
    _bump(stats, library_calls=1, launches=launches.value)
    return [y[o:o + x.shape[0] * int(n)].view(x.shape[0], int(n)) for x, o, n in zip(xs, out_off, n_outs)]


def _mix(A: List[torch.Tensor], B: List[torch.Tensor], ns: Sequence[int], params, store: bool, stats=None):
    """egr_nullmany_mix over pairs (A[i], B[i]) on their first ns[i] samples; params[i] = (g, k, sign, use_k).
    -> (out8 host array [P, 8], matched, null, scaled: lists of [C, n] tensors or None)."""
    P = len(A)
    dev = A[0].device
    for i, (a, b) in enumerate(zip(A, B)):
        if a.shape[0] != b.shape[0]:
            raise ValueError(f"pair {i}: operands could not be broadcast together with shapes {(a.shape[0], int(ns[i]))} {(b.shape[0], int(ns[i]))}")
    base, offs = loudness.flat_offsets(list(A) + list(B))
    out_off, pos = [], 0
    for a, n in zip(A, ns):
        out_off.append(pos)
        pos += a.shape[0] * int(n)
    rows = [(offs[i], A[i].shape[0], A[i].shape[1], offs[P + i], B[i].shape[0], B[i].shape[1], int(ns[i]), out_off[i]) for i in range(P)]
    tab = _tab(rows)
    L = native.lib()
    need = int(L.egr_nullmany_mix_workspace_bytes(tab, P))
    if need == 0:
        raise _refused("egr_nullmany_mix")
    prm = (C.c_float * (4 * P))(*[float(np.float32(v)) for q in params for v in q])
    use_k = any(q[3] for q in params)
    outs = [torch.empty((pos,), dtype=torch.float32, device=dev) if on else None for on in (store, store, store and use_k)]
    out8 = torch.empty((P, 8), dtype=torch.float64, device=dev)
    ws = _ws(need, dev)
    launches = C.c_int(0)
    native.check(L.egr_nullmany_mix(C.c_void_p(base), C.c_void_p(base), tab, prm, P, *[native.ptr(o) if o is not None else None for o in outs],
                                    native.ptr(out8), native.ptr(ws), need, C.byref(launches), native.stream_ptr()), "egr_nullmany_mix")
    host = out8.cpu().numpy()
    _bump(stats, library_calls=1, launches=launches.value, host_reads=1)
    views = [None if o is None else [o[f:f + a.shape[0] * int(n)].view(a.shape[0], int(n)) for a, f, n in zip(A, out_off, ns)] for o in outs]
    return (host, *views)


def _lufs(xs: List[torch.Tensor], srs: Sequence[int], stats=None) -> List[float]:
    """The suite's integrated loudness of every clip: one egr_loudness_tracks call (blk_b = 0, up = 0) and one read per (rate, channels)."""
    res = [0.0] * len(xs)
    for (sr, _), idx in level_groups([(sr, x.shape[0]) for x, sr in zip(xs, srs)]).items():
        st = {}
        for i, (ms, _, _) in zip(idx, loudness.engine_many([xs[i] for i in idx], sr, False, 0, stats=st)):
            res[i] = device_ops.lufs_gate(ms)
        _bump(stats, library_calls=st["library_calls"], launches=st["launches"], host_reads=1, level_groups=1)
    return res


def _rms_db(xs: List[torch.Tensor], stats=None) -> List[float]:
    """10 log10(mean(mono^2) + 1e-20) of every clip from the sums of one egr_nullmany_mix call (each clip against itself)."""
    out8, _, _, _ = _mix(xs, xs, [x.shape[1] for x in xs], [(1.0, 0.0, -1.0, 0)] * len(xs), False, stats)
    return [10.0 * math.log10(float(out8[i][5]) / x.shape[1] + 1e-20) for i, x in enumerate(xs)]


def _levels(xs, srs, mode, stats=None):
    return _lufs(xs, srs, stats) if str(mode).upper().startswith("LUFS") else _rms_db(xs, stats)


def _gains(ref_levels, in_levels, max_gain_db):
    return [float(np.clip(r - i, -abs(max_gain_db), abs(max_gain_db))) for r, i in zip(ref_levels, in_levels)]


def _null(A, B, srs, invert_b, least_squares_scale, compute_corr, compute_null_rms, compute_null_lufs, compute_lsd, compute_hf_residual,
          n_fft, hop, hf_band_hz, gains=None, stats=None):
    """null_stage for many pairs, with the gain of gain_stage folded in (gains: linear factors, None = 1).
    -> (matched, null, metrics) lists."""
    P = len(A)
    ns = [min(a.shape[1], b.shape[1]) for a, b in zip(A, B)]
    g = [1.0] * P if gains is None else [float(np.float32(v)) for v in gains]
    sgn = -1.0 if invert_b else 1.0
    ks = [None] * P
    if least_squares_scale:
        s8, _, _, _ = _mix(A, B, ns, [(g[i], 0.0, sgn, 0) for i in range(P)], False, stats)
        ks = [float(s8[i][4] / float(s8[i][6] + 1e-20)) for i in range(P)]
    out8, matched, nulls, scaled = _mix(A, B, ns, [(g[i], ks[i] if ks[i] is not None else 1.0, sgn, int(ks[i] is not None)) for i in range(P)],
                                        True, stats)
    lufs = _lufs(nulls, srs, stats) if compute_null_lufs else None
    lsd = None
    if compute_lsd:
        side_b = scaled if least_squares_scale else matched
        base, offs = loudness.flat_offsets(list(A) + list(side_b))
        rows = [(offs[i], A[i].shape[0], A[i].shape[1], offs[P + i], side_b[i].shape[0], ns[i], ns[i]) for i in range(P)]
        lsd, _, launches = device_ops.metrics_pairs(base, base, rows, int(n_fft), int(hop), device_ops.METRICS_LSD, device=A[0].device)
        _bump(stats, library_calls=1, launches=launches, host_reads=1)
    metrics = []
    for i in range(P):
        sq, overs, sa, sb, ab, aa, bb = (float(v) for v in out8[i][:7])
        m = {}
        if compute_corr:
            m["corr_coef"] = corr_finish(sa, sb, ab, aa, bb, ns[i], invert_b)
        if compute_null_rms:
            m["null_rms_dbfs"] = 10.0 * math.log10(sq / ns[i] + 1e-20)
        if compute_null_lufs:
            m["null_lufs"] = lufs[i]
        if compute_lsd:
            m["lsd_mean_db"], m["lsd_p95_db"] = device_ops.lsd_finish(float(lsd[i][0]), float(lsd[i][1]), float(lsd[i][2]), int(lsd[i][3]))
        if compute_hf_residual:
            m["hf_residual_db"] = device_ops.band_energy_hi_db(nulls[i], srs[i], hf_band_hz)
            _bump(stats, per_pair_calls=1)
        m["overshoot_count"] = int(overs)
        m["clipped_pct"] = float(100.0 * overs / nulls[i].numel())
        m["scale_k"] = float(1.0 if ks[i] is None else ks[i])
        metrics.append(m)
    return matched, nulls, metrics


# ------------------------------------------------------------------------------------------------ the public calls
def _rates(srs, n: int, who: str):
    """srs: one rate, or per pair a rate or (reference rate, processed rate) -> [(sr_ref, sr_proc)]."""
    if isinstance(srs, (int, float)):
        srs = [srs] * n
    if len(srs) != n:
        raise ValueError(f"{who}: {n} pairs against {len(srs)} sample rates")
    out = [(int(s[0]), int(s[1])) if isinstance(s, (tuple, list)) else (int(s), int(s)) for s in srs]
    for i, (a, b) in enumerate(out):
        if a < 1 or b < 1:
            raise ValueError(f"{who}: item {i}: sample rate {min(a, b)}")
    return out


def _pairs(pairs, who: str):
    return [(eval_many._side(a, who, i), eval_many._side(b, who, i)) for i, (a, b) in enumerate(pairs)]


def _waves(pairs, n_fft=2048, hop=512, max_bytes=None):
    need = [pair_bytes(a.shape[0], a.shape[1], b.shape[0], b.shape[1], n_fft, hop) for a, b in pairs]
    work = [pair_work(a.shape[1], b.shape[1], n_fft, hop) for a, b in pairs]
    return eval_many.plan_waves(need, max_bytes, item_work=work)


def _upload(pairs, rates, wave, stats=None):
    """The wave's sides on the device, the processed side brought to the reference's rate as the nodes do (np.interp's rule)."""
    xs = eval_many._on_device([t for i in wave for t in pairs[i]])
    xr, xp = xs[0::2], xs[1::2]
    for j, i in enumerate(wave):
        sr_ref, sr_proc = rates[i]
        if sr_proc != sr_ref:
            xp[j] = device_ops.resample_linear(xp[j], int(round(xp[j].shape[1] * sr_ref / sr_proc)))
            _bump(stats, per_pair_calls=1)
    return xr, xp


def delays_many(pairs, srs, max_shift_ms=200, stats=None, max_bytes=None, raw: Optional[list] = None) -> List[float]:
    """pairs: [(ref, proc)] of [C,T] / [T] float tensors on the host or the device, proc at the reference's rate unless srs gives
    (sr_ref, sr_proc) -> device_ops.xcorr_delay's lag of every pair in samples (true lag minus one, quirk Q8).  raw, an empty list,
    receives the pairs' four floats of egr_gcc_phat in input order (the waves hold consecutive pairs)."""
    pairs = _pairs(pairs, "delays_many")
    _stats(stats)
    rates = _rates(srs, len(pairs), "delays_many")
    res: List = [None] * len(pairs)
    for wave in _waves(pairs, max_bytes=max_bytes):
        xr, xp = _upload(pairs, rates, wave, stats)
        lags = _delays(xr, xp, [max_shift_samples(rates[i][0], max_shift_ms) for i in wave], stats, raw)
        for j, i in enumerate(wave):
            res[i] = lags[j]
        _bump(stats, waves=1)
    return res


def shift_fir_many(xs, delays, taps=64, n_outs=None, stats=None):
    """apply_delay for many clips in one launch: xs [C,N] / [N] float tensors, delays in samples (apply_delay's rule for shift, fraction
    and taps), n_outs the output lengths (default: each clip's own) -> [C, n_out] CUDA tensors with egr_shift_fir's bits."""
    xs = [eval_many._side(x, "shift_fir_many", i) for i, x in enumerate(xs)]
    _stats(stats)
    if not xs:
        return []
    if len(delays) != len(xs) or (n_outs is not None and len(n_outs) != len(xs)):
        raise ValueError("shift_fir_many: one delay and one output length per clip")
    n_outs = [x.shape[1] for x in xs] if n_outs is None else [int(n) for n in n_outs]
    out = _shift_fir(eval_many._on_device(xs), delays, int(taps), n_outs, stats)
    _bump(stats, waves=1)
    return out


def align_many(pairs, srs, max_shift_ms=200, fractional=True, fir_len=64, stats=None, max_bytes=None):
    """align_stage for many pairs -> [(proc aligned to ref's length, lag in samples)]."""
    pairs = _pairs(pairs, "align_many")
    _stats(stats)
    rates = _rates(srs, len(pairs), "align_many")
    res: List = [None] * len(pairs)
    for wave in _waves(pairs, max_bytes=max_bytes):
        xr, xp = _upload(pairs, rates, wave, stats)
        lags = _delays(xr, xp, [max_shift_samples(rates[i][0], max_shift_ms) for i in wave], stats)
        comp = [float(-lag if fractional else -round(lag)) for lag in lags]
        aligned = _shift_fir(xp, comp, int(fir_len), [a.shape[1] for a in xr], stats)
        for j, i in enumerate(wave):
            res[i] = (aligned[j], lags[j])
        _bump(stats, waves=1)
    return res


def gain_match_many(pairs, srs, mode="LUFS-I", max_gain_db=12.0, stats=None, max_bytes=None):
    """gain_stage for many pairs (ref, in) -> [(in * gain, gain_db, ref_level, in_level)]."""
    pairs = _pairs(pairs, "gain_match_many")
    _stats(stats)
    rates = _rates(srs, len(pairs), "gain_match_many")
    res: List = [None] * len(pairs)
    for wave in _waves(pairs, max_bytes=max_bytes):
        xr, xi = _upload(pairs, rates, wave, stats)
        sr = [rates[i][0] for i in wave]
        lv = _levels(xr + xi, sr + sr, mode, stats)
        ref_lv, in_lv = lv[:len(wave)], lv[len(wave):]
        gdb = _gains(ref_lv, in_lv, max_gain_db)
        _, matched, _, _ = _mix(xi, xi, [x.shape[1] for x in xi], [(10 ** (g / 20.0), 1.0, -1.0, 0) for g in gdb], True, stats)
        for j, i in enumerate(wave):
            res[i] = (matched[j], gdb[j], float(ref_lv[j]), float(in_lv[j]))
        _bump(stats, waves=1)
    return res


def null_test_many(pairs, srs, invert_b=True, least_squares_scale=False, compute_corr=True, compute_null_rms=True, compute_null_lufs=True,
                   compute_lsd=True, compute_hf_residual=False, n_fft=2048, hop=512, hf_band_hz=8000, stats=None, max_bytes=None):
    """null_stage for many pairs (A, B) of one rate each -> [(null [C,n] on the device, metrics in the single node's key order)]."""
    pairs = _pairs(pairs, "null_test_many")
    _stats(stats)
    rates = _rates(srs, len(pairs), "null_test_many")
    for i, (a, b) in enumerate(rates):
        if a != b:
            raise ValueError(f"null_test_many: item {i}: Sample rate mismatch after alignment stage")
    res: List = [None] * len(pairs)
    for wave in _waves(pairs, n_fft, hop, max_bytes):
        A, B = _upload(pairs, rates, wave, stats)
        _, nulls, metrics = _null(A, B, [rates[i][0] for i in wave], invert_b, least_squares_scale, compute_corr, compute_null_rms,
                                  compute_null_lufs, compute_lsd, compute_hf_residual, n_fft, hop, hf_band_hz, None, stats)
        for j, i in enumerate(wave):
            res[i] = (nulls[j], metrics[j])
        _bump(stats, waves=1)
    return res


def full_many(pairs, srs, align_max_shift_ms=200, align_method="gcc-phat", fractional=True, fir_len=64, match_mode="LUFS-I",
              least_squares_scale=False, compute_corr=True, compute_null_rms=True, compute_null_lufs=True, compute_lsd=True,
              compute_hf_residual=False, n_fft=2048, hop=512, stats=None, max_bytes=None):
    """`Null Test (Full)` without its plots for many pairs: align_stage -> gain_stage -> null_stage.
    -> [(matched, null, delay_ms, gain_db, metrics)], the two signals [C, n] on the device."""
    pairs = _pairs(pairs, "full_many")
    _stats(stats)
    rates = _rates(srs, len(pairs), "full_many")
    res: List = [None] * len(pairs)
    for wave in _waves(pairs, n_fft, hop, max_bytes):
        xr, xp = _upload(pairs, rates, wave, stats)
        sr = [rates[i][0] for i in wave]
        lags = _delays(xr, xp, [max_shift_samples(s, align_max_shift_ms) for s in sr], stats)
        comp = [float(-lag if fractional else -round(lag)) for lag in lags]
        aligned = _shift_fir(xp, comp, int(fir_len), [a.shape[1] for a in xr], stats)
        lv = _levels(xr + aligned, sr + sr, match_mode, stats)
        gdb = _gains(lv[:len(wave)], lv[len(wave):], 12.0)
        matched, nulls, metrics = _null(xr, aligned, sr, True, least_squares_scale, compute_corr, compute_null_rms, compute_null_lufs,
                                        compute_lsd, compute_hf_residual, n_fft, hop, 8000, [10 ** (g / 20.0) for g in gdb], stats)
        for j, i in enumerate(wave):
            res[i] = (matched[j], nulls[j], float(1000.0 * lags[j] / sr[j]), float(gdb[j]), metrics[j])
        _bump(stats, waves=1)
    return res
