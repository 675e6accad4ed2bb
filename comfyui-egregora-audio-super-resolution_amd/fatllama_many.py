"""Many clips through `Egregora Fat Llama (GPU)` at once: enhance_many.

Per clip this is fatllama_engine.node_run's arithmetic -- the clip's own up-rating factor, the EGREGORA_FATLLAMA_SPEC variants, PCM_16 in,
the node's write patch out -- but clips whose lengths have no packed plan (the paired chirp-z lengths: nearly every real file) share
launches: a WAVE of them runs on one convolution length P, the largest clip's own, as states of the same kernels (egr_flmany_*), with what
depends on a clip's own transform length in a per-state row table.  The largest clip of a wave, and every clip whose own P is the wave's,
gets the single node's bits; the others its result to fp32 round-off (another, equally exact, convolution length).  The clips go up in
one transfer and come down in one.
"""
import ctypes as C
import os
from typing import List, Optional, Sequence, Tuple

import torch

from . import fatllama_engine, native
from .many_common import budget_bytes, check_clips, download, upload

MAX_ROWS = native.FLMANY_MAX_ROWS       # channel rows of a wave (egr_flmany_create's limit)
DEFAULT_WAVE_GB = 16.0                  # EGREGORA_FATLLAMA_WAVE_GB: device bytes a wave may allocate
# EGREGORA_FATLLAMA_WAVE_SLACK: a wave's states may hold (1 + slack) times the points they would hold on their own P.  The menu of
# scheduled column lengths moves in steps of 3 - 9 %, so 0.15 lets a wave span two steps: a design condition, not a measurement.
DEFAULT_WAVE_SLACK = 0.15

REASONS = {1: "packed plan", 2: "three-level chirp-z plan", 3: "mixed chirp-z kinds", 4: "too many channel rows", 5: "no convolution length",
           6: "legacy chirp-z forced"}


def _arrays(specs):
    n = len(specs)
    return ((C.c_int64 * n)(*[int(s[0]) for s in specs]), (C.c_int * n)(*[int(s[1]) for s in specs]),
            (C.c_int64 * n)(*[int(s[2] or 0) for s in specs]), (C.c_int * n)(*[int(s[3]) for s in specs]))


def query(specs: Sequence[Tuple[int, int, int, int]]) -> dict:
    """egr_flmany_query (host only, works without a GPU).  specs: [(n_in, factor, n_out or 0, channels)] ->
    {"wave": the clips form one wave, "kind", "L", "nc", "P", "states", "rows", "bytes", "TC", "levels", "bad_clip", "reason",
     "gpx", "x_floats", "out_floats", "distinct", "clips": [{"kind", "D", "P", "levels", "N", "state0", "states", "row0"}],
     "state_rows": [{"clip", "s", "c0", "iDr", "cDr", "G", "D", "channels"}]}."""
    n = len(specs)
    H, R = native.FLMANY_HEAD, native.FLMANY_REC
    info = (C.c_int64 * (H + R * (n + sum(int(s[3]) for s in specs))))()
    native.check(native.lib().egr_flmany_query(n, *_arrays(specs), info), "egr_flmany_query")
    v = list(info)
    d = dict(zip(("wave", "kind", "L", "nc", "P", "states", "rows", "bytes", "TC", "levels", "bad_clip", "reason", "gpx", "x_floats",
                  "out_floats", "distinct"), v[:H]))
    d["wave"] = bool(d["wave"])
    d["clips"] = [dict(zip(("kind", "D", "P", "levels", "N", "state0", "states", "row0"), v[H + R * i:H + R * (i + 1)])) for i in range(n)]
    d["state_rows"] = [dict(zip(("clip", "s", "c0", "iDr", "cDr", "G", "D", "channels"), v[H + R * (n + j):H + R * (n + j + 1)]))
                       for j in range(d["states"] if d["wave"] else 0)]
    return d


def wave_bytes(P: int, states: int, distinct: int, rows: int) -> int:
    """Device bytes of a wave as egr_flmany_query counts them: the states, one chirp spectrum per distinct D, the two double-precision
    scratch buffers of their build, peaks and row tables."""
    return states * P * 8 + distinct * P * 8 + 2 * P * 16 + 3 * 2 * states * 4 + states * 120 + rows * 48


def _caps(max_rows, max_bytes, slack):
    if max_rows is None:
        max_rows = MAX_ROWS
    max_bytes = budget_bytes("EGREGORA_FATLLAMA_WAVE_GB", DEFAULT_WAVE_GB, max_bytes)
    if slack is None:
        slack = float(os.environ.get("EGREGORA_FATLLAMA_WAVE_SLACK", DEFAULT_WAVE_SLACK))
    return int(max_rows), int(max_bytes), float(slack)


def plan_waves(specs: Sequence[Tuple[int, int, int, int]], *, max_rows: Optional[int] = None, max_bytes: Optional[int] = None,
               slack: Optional[float] = None, single_only: bool = False):
    """Which clips share a wave.  Host only.  specs: [(n_in, factor, n_out or 0, channels)] -> (waves, fallbacks, padding):
    waves = lists of clip indices, the largest clip first (its own P is the wave's), fallbacks = the clips that go through
    enhance_device one by one (ascending), padding[i] = points of wave i's states over the points they would hold on their own P.

    A clip falls back when its length has a packed plan or a three-level chirp-z plan, when single_only is set (EGR_FL_LEGACY_CHIRPZ,
    a variant the wave does not run), or when it would be alone in its wave.  The others are grouped by chirp-z kind and sorted by
    transform length D (a clip's own P grows with D); a wave is seeded with the largest clip left and takes, in that order, every clip
    that keeps it within max_rows channel rows, max_bytes device bytes and sum(P_wave) <= (1 + slack) sum(P_own) over its states."""
    max_rows, max_bytes, slack = _caps(max_rows, max_bytes, slack)
    info = [query([s])["clips"][0] for s in specs]
    fallbacks, waves, padding = [], [], []
    by_kind = {1: [], 2: []}
    for i, c in enumerate(info):
        if single_only or c["kind"] == 0 or c["levels"] != 2 or int(specs[i][3]) > max_rows:
            fallbacks.append(i)
        else:
            by_kind[c["kind"]].append(i)
    nstates = lambda i: int(specs[i][3]) if info[i]["kind"] == 1 else (int(specs[i][3]) + 1) // 2
    for kind in (1, 2):
        left = sorted(by_kind[kind], key=lambda i: (-info[i]["D"], i))
        while left:
            seed, rest = left[0], []
            P = info[seed]["P"]
            wave, rows, states, own, ds = [seed], int(specs[seed][3]), nstates(seed), nstates(seed) * P, {info[seed]["D"]}
            for i in left[1:]:
                r2, s2, o2, d2 = rows + int(specs[i][3]), states + nstates(i), own + nstates(i) * info[i]["P"], ds | {info[i]["D"]}
                if r2 <= max_rows and wave_bytes(P, s2, len(d2), r2) <= max_bytes and s2 * P <= (1.0 + slack) * o2:
                    wave.append(i)
                    rows, states, own, ds = r2, s2, o2, d2
                else:
                    rest.append(i)
            left = rest
            if len(wave) == 1:
                fallbacks.append(seed)
            else:
                waves.append(wave)
                padding.append(states * P / own)
    return waves, sorted(fallbacks), padding


class Wave:
    """egr_flmany_create / _enhance / _destroy for clips [C, T] given as (n_in, factor, n_out or 0, channels)."""

    def __init__(self, specs):
        self.specs = [tuple(int(v or 0) for v in s) for s in specs]
        self.h = C.c_void_p()
        n = len(self.specs)
        native.check(native.lib().egr_flmany_create(C.byref(self.h), n, *_arrays(self.specs)), "egr_flmany_create")
        rows = sum(s[3] for s in self.specs)
        xo, oo, tot = (C.c_int64 * rows)(), (C.c_int64 * rows)(), (C.c_int64 * 2)()
        native.check(native.lib().egr_flmany_layout(self.h, xo, oo, tot), "egr_flmany_layout")
        self.x_off, self.out_off, self.x_floats, self.out_floats = list(xo), list(oo), tot[0], tot[1]

    def enhance(self, xs: Sequence[torch.Tensor], max_iterations: int, threshold: float, flags: int) -> List[torch.Tensor]:
        """xs: the clips, [C, T] float32 on the current device -> [C, n_out] views of one flat result, enqueued on the current stream."""
        for x, s in zip(xs, self.specs):
            if not (x.is_cuda and x.dtype == torch.float32 and tuple(x.shape) == (s[3], s[0])):
                raise RuntimeError("Wave.enhance wants the [C, T] float32 device tensors the wave was made for")
        x_flat = torch.cat([x.reshape(-1) for x in xs])
        out = torch.empty(self.out_floats, dtype=torch.float32, device=x_flat.device)
        native.check(native.lib().egr_flmany_enhance(self.h, native.ptr(x_flat), native.ptr(out), int(max_iterations), float(threshold),
                                                     int(flags), native.stream_ptr()), "egr_flmany_enhance")
        res, row = [], 0
        for s in self.specs:
            N = s[2] or s[0] * s[1]
            Np = N + (N & 1)
            res.append(out[self.out_off[row]:self.out_off[row] + s[3] * Np].view(s[3], Np)[:, :N])
            row += s[3]
        return res

    def close(self):
        if self.h:
            native.lib().egr_flmany_destroy(self.h)      # (waits for the device)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:      # noqa: BLE001 -- interpreter shutdown
            pass


def _request(x, sr, target_bitrate_kbps):
    """-> (factor, n_out or 0, sr_out) by fatllama_engine.node_run's rules."""
    Cn, T = x.shape
    f = fatllama_engine.upscale_factor(int(sr), Cn, int(target_bitrate_kbps))
    n_out, sr_out = 0, int(sr) * f
    if "ratio_then_int" in fatllama_engine.variant_names():
        r = fatllama_engine.upscale_ratio(int(sr), Cn, int(target_bitrate_kbps))
        n_out, sr_out, f = int(T * r), int(int(sr) * r), 1
        if n_out == T:
            n_out = 0
    return f, n_out, sr_out


def enhance_many(clips: Sequence[Tuple[torch.Tensor, int]], max_iterations: int, threshold_value: float, target_bitrate_kbps: int,
                 toggle_normalize: bool, toggle_autoscale: bool, *, stats: Optional[dict] = None) -> List[Tuple[torch.Tensor, int]]:
    """clips: [([C, T] float tensor on the host or the device, sample_rate)] -> [(float32 [C, n_out] host tensor, sr_out)] in input
    order, each what EgregoraFatLlamaGPU returns for the clip alone (module docstring).  Runs on the current device; stats (optional
    dict) receives {"waves", "rows": per wave, "padding": per wave, "fallbacks", "wave_clips": clip indices per wave}."""
    clips = check_clips("enhance_many", clips)
    if stats is not None:
        stats.update({"waves": 0, "rows": [], "padding": [], "fallbacks": 0, "wave_clips": []})
    if not clips:
        return []
    native.require_device()
    dev = torch.device("cuda", torch.cuda.current_device())
    reqs = [_request(x, sr, target_bitrate_kbps) for x, sr in clips]
    specs = [(x.shape[1], f, n_out, x.shape[0]) for (x, _), (f, n_out, _) in zip(clips, reqs)]
    flags = fatllama_engine._flags(bool(toggle_normalize), bool(toggle_autoscale), True, True, None)
    single_only = (int(max_iterations) < 1 or bool(flags & native.FL_THR_RECOMPUTE) or
                   os.environ.get("EGR_FL_LEGACY_CHIRPZ", "0") not in ("", "0"))
    waves, fallbacks, padding = plan_waves(specs, single_only=single_only)
    xs = [x.contiguous() for x in upload([x for x, _ in clips], dev, torch.float32)]
    ys: List = [None] * len(clips)
    for wave, pad in zip(waves, padding):
        w = Wave([specs[i] for i in wave])
        try:
            # (contiguous copies: the wave and its flat result go before the next wave is made)
            for i, y in zip(wave, w.enhance([xs[i] for i in wave], int(max_iterations), float(threshold_value), flags)):
                ys[i] = y.contiguous()
        finally:
            w.close()
        if stats is not None:
            stats["waves"] += 1
            stats["rows"].append(sum(specs[i][3] for i in wave))
            stats["padding"].append(pad)
            stats["wave_clips"].append(list(wave))
    for i in fallbacks:
        f, n_out, _ = reqs[i]
        ys[i] = fatllama_engine.enhance_device(xs[i], f, int(max_iterations), float(threshold_value), bool(toggle_normalize),
                                               bool(toggle_autoscale), pcm_in=True, node_post=True, n_out=n_out or None)
    if stats is not None:
        stats["fallbacks"] = len(fallbacks)
    return [(y, r[2]) for y, r in zip(download(ys), reqs)]
