"""Many clips through the evaluation nodes at once: metrics_many and loudness_many.

Per pair metrics_many is what `Metrics (LSD + SI-SDR)` computes, per clip loudness_many is what `Loudness Meter (BS1770)` computes, but a
WAVE of them is one library call (egr_metrics_pairs: at most six launches; egr_loudness_tracks: at most four) and one device -> host
copy, whatever the number of clips.  Nothing is padded: the kernels find their pair or clip in a table.  The host finishes every
result with the single path's own expressions (device_ops.lsd_finish / si_sdr_finish, loudness.measure_finish).  Host tensors go up
one by one, as the single nodes send them; tensors that are already on the device are addressed where they lie.
"""
from typing import List, Optional, Sequence, Tuple

import torch

from . import device_ops, loudness, native
from .many_common import budget_bytes

DEFAULT_WAVE_GB = 4.0          # EGREGORA_EVAL_WAVE_GB


def wave_budget(max_bytes: Optional[int] = None) -> int:
    return budget_bytes("EGREGORA_EVAL_WAVE_GB", DEFAULT_WAVE_GB, max_bytes)


def plan_waves(item_bytes: Sequence[int], max_bytes: Optional[int] = None, item_work: Optional[Sequence[int]] = None,
               max_work: int = device_ops.MAX_GRID_256, max_items: int = device_ops.MAX_PAIRS) -> List[List[int]]:
    """Which items share a call.  Host only.  item_bytes[i] = what item i alone needs on the device (workspace entry point plus its
    samples); the items fill a wave in input order until the next one would take the sum past max_bytes (default
    EGREGORA_EVAL_WAVE_GB GiB, 4 when unset).  An item that is over the budget by itself is a wave of its own.  The sum bounds the
    wave's need from above: the tables and buffers of a joint call are the items' laid back to back with less padding.
    item_work[i] = the most workgroups item i adds to any one grid of the call (frames or chunks; blocks or peak tiles): a wave also
    closes before its sum passes max_work, what one grid of 256-thread workgroups holds, or its items max_items.  An item over
    max_work by itself still forms a wave, which the library then refuses by name."""
    budget = wave_budget(max_bytes)
    work = [0] * len(item_bytes) if item_work is None else [int(w) for w in item_work]
    waves, cur, cur_bytes, cur_work = [], [], 0, 0
    for i, b in enumerate(item_bytes):
        if cur and (cur_bytes + int(b) > budget or cur_work + work[i] > max_work or len(cur) >= max_items):
            waves.append(cur)
            cur, cur_bytes, cur_work = [], 0, 0
        cur.append(i)
        cur_bytes += int(b)
        cur_work += work[i]
    if cur:
        waves.append(cur)
    return waves


def pair_work(ta: int, tb: int, n_fft: int, hop: int) -> int:
    """The most workgroups one pair adds to a grid of egr_metrics_pairs: its frames or its SI-SDR chunks."""
    n = min(ta, tb)
    frames = int(native.lib().egr_metrics_pairs_frames(device_ops.pairs_table([(0, 1, n, 0, 1, n, n)]), 1, int(n_fft), int(hop)))
    return max(frames, -(-n // device_ops.METRICS_CHUNK))


def clip_work(n: int, sr: int, up: int) -> int:
    """The most workgroups one clip adds to a grid of egr_loudness_tracks: its 400 ms blocks or its 256-sample peak tiles (the thread
    chunks go 64 to a workgroup and number fewer than the samples / 64)."""
    return max(loudness.block_shape(sr, 0.400, 0.100, n)[2], -(-n * int(up) // 256), -(-n // 64 // 64))


def _side(x, who: str, i: int) -> torch.Tensor:
    if not torch.is_tensor(x) or x.dim() not in (1, 2):
        raise ValueError(f"{who}: item {i}: expected a [C, T] or [T] tensor")
    x = x[None, :] if x.dim() == 1 else x
    if x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"{who}: item {i}: empty signal")
    return x


def _stats(stats: Optional[dict]):
    if stats is not None:
        stats.update({"waves": 0, "library_calls": 0, "launches": 0, "wave_items": [], "wave_launches": []})


def _on_device(xs: List[torch.Tensor]) -> List[torch.Tensor]:
    """Contiguous float32 tensors on the current device.  A host tensor goes up by itself, as the single node sends it: gathering the
    wave in one host buffer first costs a second pass over every sample and was measured slower (profiles/eval_batch.md)."""
    native.require_device()
    dev = torch.device("cuda", torch.cuda.current_device())
    return [x.to(dev, torch.float32).contiguous() for x in xs]


def metrics_flags(compute_lsd: bool, compute_si_sdr: bool) -> int:
    return (device_ops.METRICS_LSD if compute_lsd else 0) | (device_ops.METRICS_SI_SDR if compute_si_sdr else 0)


def pair_bytes(ca: int, ta: int, cb: int, tb: int, n_fft: int, hop: int, flags: int) -> int:
    """Device bytes one pair needs by itself: its workspace (egr_metrics_pairs_workspace_bytes) and its samples."""
    ws = device_ops.metrics_pairs_workspace_bytes([(0, ca, ta, ca * ta, cb, tb, min(ta, tb))], n_fft, hop, flags)
    if ws == 0:
        raise RuntimeError(f"egr_metrics_pairs refused: {native.last_error()}")
    return ws + 4 * (ca * ta + cb * tb)


def metrics_finish(row, compute_lsd: bool, compute_si_sdr: bool) -> dict:
    """One row of egr_metrics_pairs' out8 -> the single node's dictionary, keys in its order."""
    out = {}
    if compute_lsd:
        mean, p95 = device_ops.lsd_finish(float(row[0]), float(row[1]), float(row[2]), int(row[3]))
        out["lsd_mean_db"] = float(mean)
        out["lsd_p95_db"] = float(p95)
    if compute_si_sdr:
        out["si_sdr_db"] = float(device_ops.si_sdr_finish(float(row[6]), float(row[7])))
    return out


def metrics_many(pairs, n_fft=2048, hop=512, compute_lsd=True, compute_si_sdr=True, stats=None):
    """pairs: [(ref, proc)] of [C,T] / [T] float tensors on the host or the device (sample rates are ignored, as in the node) -> the
    dictionaries `Metrics (LSD + SI-SDR)` returns, in input order.  Each side is downmixed to mono and the pair cut to the common
    length on the device.  stats, when given, receives {"waves", "library_calls", "launches", "wave_items", "wave_launches"}."""
    pairs = [(_side(a, "metrics_many", i), _side(b, "metrics_many", i)) for i, (a, b) in enumerate(pairs)]
    _stats(stats)
    flags = metrics_flags(bool(compute_lsd), bool(compute_si_sdr))
    if not pairs or not flags:
        return [{} for _ in pairs]
    n_fft, hop = int(n_fft), int(hop)
    need = [pair_bytes(a.shape[0], a.shape[1], b.shape[0], b.shape[1], n_fft, hop, flags) for a, b in pairs]
    work = [pair_work(a.shape[1], b.shape[1], n_fft, hop) for a, b in pairs]
    res: List = [None] * len(pairs)
    for wave in plan_waves(need, item_work=work):
        xs = _on_device([t for i in wave for t in pairs[i]])
        base, offs = loudness.flat_offsets(xs)
        rows = []
        for j in range(len(wave)):
            a, b = xs[2 * j], xs[2 * j + 1]
            rows.append((offs[2 * j], a.shape[0], a.shape[1], offs[2 * j + 1], b.shape[0], b.shape[1], min(a.shape[1], b.shape[1])))
        out8, _, launches = device_ops.metrics_pairs(base, base, rows, n_fft, hop, flags, device=xs[0].device)
        for j, i in enumerate(wave):
            res[i] = metrics_finish(out8[j], bool(compute_lsd), bool(compute_si_sdr))
        if stats is not None:
            stats["waves"] += 1
            stats["library_calls"] += 1
            stats["launches"] += launches
            stats["wave_items"].append(list(wave))
            stats["wave_launches"].append(launches)
    return res


def loudness_many(clips, compute_true_peak=True, oversample=4, stats=None):
    """clips: [([C,T] / [T] float tensor on the host or the device, sample_rate)] -> the dictionaries loudness.measure returns, in
    input order.  The clips are grouped by (sample rate, channels); each wave of a group is one egr_loudness_tracks call."""
    clips = [(_side(x, "loudness_many", i), int(sr)) for i, (x, sr) in enumerate(clips)]
    _stats(stats)
    if not clips:
        return []
    up = int(oversample) if compute_true_peak else 0
    groups = {}
    for i, (x, sr) in enumerate(clips):
        if sr < 1:
            raise ValueError(f"loudness_many: item {i}: sample rate {sr}")
        groups.setdefault((sr, x.shape[0]), []).append(i)
    res: List = [None] * len(clips)
    for (sr, ch), idx in groups.items():
        need = []
        for i in idx:
            n = clips[i][0].shape[1]
            ws = loudness.many_workspace_bytes([n], ch, sr, True, up)
            if ws == 0:
                raise RuntimeError(f"egr_loudness_tracks refused: {native.last_error()}")
            need.append(ws + 4 * ch * n)
        work = [clip_work(clips[i][0].shape[1], sr, up) for i in idx]
        for wave in plan_waves(need, item_work=work, max_items=device_ops.MAX_GRID_256):
            ids = [idx[j] for j in wave]
            xs = _on_device([clips[i][0] for i in ids])
            st = {}
            for i, (ms_a, ms_b, peak) in zip(ids, loudness.engine_many(xs, sr, True, up, stats=st)):
                res[i] = loudness.measure_finish(ms_a, ms_b, peak, bool(compute_true_peak))
            if stats is not None:
                stats["waves"] += 1
                stats["library_calls"] += st["library_calls"]
                stats["launches"] += st["launches"]
                stats["wave_items"].append(ids)
                stats["wave_launches"].append(st["launches"])
    return res
