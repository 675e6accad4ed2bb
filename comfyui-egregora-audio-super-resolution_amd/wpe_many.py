"""Many clips through `Egregora WPE Dereverb` at once: dereverb_many.

Per clip this is what Egregora_WPE_Dereverb.execute does -- the limits, the passthrough of an empty clip or an unsupported framing, stft,
the iterations, istft -- but the clips of one channel count share the launches: a WAVE of them is one egr_wpemany_dereverb call, 2 +
iterations launches whatever the number of clips.  A clip's spectra, weights and filter never touch another clip's, so nothing is padded
(a wave costs the sum of its clips) and every clip gets the bits the single node gives it.  WPE runs at each clip's own sample rate:
rates need no grouping.  The clips go up in one transfer and come down in one.
"""
from typing import List, Optional, Sequence, Tuple

import torch

from . import native, wpe_engine
from .many_common import budget_bytes, check_clips, download, upload

WIDGET_DEFAULTS = dict(taps=10, delay=3, iterations=3, n_fft=1024, hop=256, use_float32=True)
DEFAULT_WAVE_GB = 16.0          # EGREGORA_WPE_WAVE_GB


def _widgets(who: str, widgets: dict) -> dict:
    unknown = set(widgets) - set(WIDGET_DEFAULTS)
    if unknown:
        raise TypeError(f"{who}: unknown widget(s) {sorted(unknown)}")
    w = dict(WIDGET_DEFAULTS, **widgets)
    return {k: (bool(v) if k == "use_float32" else int(v)) for k, v in w.items()}


def plan_waves(specs: Sequence[Tuple[int, int]], max_bytes: Optional[int] = None, *, n_fft: int = 1024, hop: int = 256, taps: int = 10):
    """Which clips share a call.  Host only.  specs: [(channels, samples per channel)] -> (waves, alone, wave_bytes): waves = lists of
    clip indices of one channel count, each ascending and the waves of a channel count in input order; alone = the clips that go
    through the single call one by one (ascending); wave_bytes[i] = egr_wpemany_workspace_bytes of wave i.

    The clips of a channel count fill a wave in input order until the next one would take its workspace past max_bytes; a clip whose
    own wave is over the budget (or that the many-clip call refuses, such as a clip of 2^31 - 4096 frames) goes alone.  max_bytes
    defaults to EGREGORA_WPE_WAVE_GB GiB, 16 when unset: Fat-Llama's choice for its waves, taken over as it is, not a measurement."""
    max_bytes = budget_bytes("EGREGORA_WPE_WAVE_GB", DEFAULT_WAVE_GB, max_bytes)
    groups = {}
    for i, (c, n) in enumerate(specs):
        groups.setdefault(int(c), []).append(i)
    need = lambda c, idx: wpe_engine.many_workspace_bytes([int(specs[i][1]) for i in idx], c, n_fft, hop, taps)
    waves, alone, wave_bytes = [], [], []
    for c, idx in groups.items():
        cur, cur_bytes = [], 0
        for i in idx:
            b = need(c, [i])
            if not 0 < b <= max_bytes:
                alone.append(i)
                continue
            if cur:
                both = need(c, cur + [i])
                if 0 < both <= max_bytes:
                    cur, cur_bytes = cur + [i], both
                    continue
                waves.append(cur)
                wave_bytes.append(cur_bytes)
            cur, cur_bytes = [i], b
        if cur:
            waves.append(cur)
            wave_bytes.append(cur_bytes)
    return waves, sorted(alone), wave_bytes


def dereverb_many(clips: Sequence[Tuple[torch.Tensor, int]], *, stats: Optional[dict] = None, **widgets) -> List[torch.Tensor]:
    """clips: [([C,T] float tensor on the host or the device, sample_rate)]; widgets: the single node's, by name (WIDGET_DEFAULTS).
    -> float32 host tensors in input order, each what the single node returns for that clip: [C, frames hop - (n_fft - hop)], or the
    input itself for an empty clip or an unsupported framing (with the reference's warning).  channels * taps > 64 or a bad n_fft
    raises RuntimeError before anything is launched.  stats, when given, receives {"waves", "alone", "wave_bytes", "wave_clips"}."""
    w = _widgets("dereverb_many", widgets)
    taps, delay, iterations, n_fft, hop = w["taps"], w["delay"], w["iterations"], w["n_fft"], w["hop"]
    clips = check_clips("dereverb_many", clips, allow_empty=True)
    for x, _ in clips:
        wpe_engine.check_limits(x.shape[0], taps, n_fft)
    if stats is not None:
        stats.update({"waves": 0, "alone": 0, "wave_bytes": [], "wave_clips": []})
    ys: List = [None] * len(clips)
    framing = wpe_engine.framing_supported(n_fft, hop)
    run = []
    for i, (x, _) in enumerate(clips):
        if x.shape[1] == 0 or not framing:
            why = "empty input" if x.shape[1] == 0 else f"hop {hop} does not divide n_fft {n_fft} at least twice"
            print(f"Warning: WPE processing failed: {why}")
            ys[i] = x.to(torch.float32).cpu()
        else:
            run.append(i)
    if not run:
        return ys
    native.require_device()
    dev = torch.device("cuda", torch.cuda.current_device())
    waves, alone, wave_bytes = plan_waves([tuple(clips[i][0].shape) for i in run], n_fft=n_fft, hop=hop, taps=taps)
    xs = [x.contiguous() for x in upload([clips[i][0] for i in run], dev, torch.float32)]
    out: List = [None] * len(run)
    for wave in waves:                  # (the waves reuse one workspace in stream order; each has a flat result of its own)
        for j, y in zip(wave, wpe_engine.dereverb_many([xs[j] for j in wave], n_fft, hop, taps, delay, iterations)):
            out[j] = y
    for j in alone:
        out[j] = wpe_engine.dereverb(xs[j], n_fft, hop, taps, delay, iterations)
    for j, y in zip(run, download(out)):
        ys[j] = y
    if stats is not None:
        stats.update({"waves": len(waves), "alone": len(alone), "wave_bytes": list(wave_bytes),
                      "wave_clips": [[run[j] for j in wave] for wave in waves]})
    return ys


def meta_for(meta: Optional[dict] = None, **widgets) -> dict:
    """The meta the single node attaches to a result: the input's meta plus meta["wpe"]."""
    w = _widgets("meta_for", widgets)
    out = dict(meta or {})
    out["wpe"] = {k: w[k] for k in ("taps", "delay", "iterations", "n_fft", "hop")}
    return out
