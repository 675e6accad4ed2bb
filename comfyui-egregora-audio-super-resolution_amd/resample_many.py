"""Many clips through `Resample Audio (HQ)` at once: resample_many.

Per clip it does what Resample_Audio_HQ.execute does for the modes that run a FIR kernel, but the clips share the launches: they are
grouped by source rate, whatever their lengths and channel counts, and each group is one library call -- egr_resample_poly_tracks for
"auto" / "scipy_polyphase" (the bits of resample.resample_hq), egr_resample_sinc_tracks for "torchaudio" (the bits of
resample.resample_sinc at the node's filter: lowpass_filter_width 64, rolloff 0.945, Kaiser window, the widget's beta).  The clips go
up in one transfer (through one pinned buffer) and the results come down in one transfer; a clip already at the target rate passes through untouched.
"torchaudio" here always means the windowed-sinc kernel: the corpus path has no linear fallback to preserve, and "linear" is refused.
"""
from typing import List, Optional, Sequence, Tuple

import torch

from . import native, resample
from .many_common import check_clips, group_by_rate

MODES = ("auto", "scipy_polyphase", "torchaudio")
NODE_FILTER = dict(lowpass_filter_width=64, rolloff=0.945, method="sinc_interp_kaiser")      # the reference's call (:512-515)


def out_len(T: int, src_sr: int, dst_sr: int) -> int:
    up, down = resample.rates(src_sr, dst_sr)                 # up = n, down = o: both kernels give ceil(T n / o) samples
    return (T * up + down - 1) // down


def resample_many(clips: Sequence[Tuple[torch.Tensor, int]], target_sr: int = 48000, mode: str = "auto", kaiser_beta: float = 14.769,
                  *, stats: Optional[dict] = None, to_host: bool = True) -> List[torch.Tensor]:
    """clips: [([C,T] float tensor on the host or the device, sample_rate)] -> [C, T'] float32 tensors at target_sr in input order (on
    the host, or left on the device with to_host=False), each with the bits of the single call.  stats, when given, receives calls
    (library calls made = distinct source rates other than the target) and groups ({source rate: clips}).
    One wave: the clips are staged group after group in one pinned buffer and uploaded in one copy (clips already on the device are
    gathered there), every group writes its stretch of one output buffer, and that buffer comes down in one copy."""
    if mode not in MODES:
        raise ValueError(f"resample_many: mode must be one of {MODES} (got {mode!r})")
    target_sr = int(target_sr)
    clips = check_clips("resample_many", clips)
    groups = group_by_rate([sr for _, sr in clips], target_sr)
    if stats is not None:
        stats["calls"], stats["groups"] = len(groups), {sr: len(idx) for sr, idx in groups.items()}
    out: List[Optional[torch.Tensor]] = [None if sr != target_sr else (x.to(torch.float32).cpu() if to_host else x.to(torch.float32))
                                         for x, sr in clips]
    if not groups:
        return out
    native.require_device()
    dev = torch.device("cuda", torch.cuda.current_device())
    order = [i for idx in groups.values() for i in idx]                      # group after group: a group is one stretch of the buffers
    n_in = sum(clips[i][0].numel() for i in order)
    n_host = sum(clips[i][0].numel() for i in order if not clips[i][0].is_cuda)
    flat = torch.empty(n_in, dtype=torch.float32, device=dev)
    if n_host:
        stage = torch.empty(n_in, dtype=torch.float32, pin_memory=True)      # host clips at their final places, holes for device clips
    pos, runs = 0, []                                                        # runs: stretches of host clips, one copy each
    for i in order:
        x = clips[i][0]
        if x.is_cuda:
            flat[pos:pos + x.numel()].view(x.shape).copy_(x)
        else:
            stage[pos:pos + x.numel()].view(x.shape).copy_(x)
            if runs and runs[-1][1] == pos:
                runs[-1][1] = pos + x.numel()
            else:
                runs.append([pos, pos + x.numel()])
        pos += x.numel()
    for a, b in runs:
        flat[a:b].copy_(stage[a:b], non_blocking=True)
    n_out = sum(clips[i][0].shape[0] * out_len(clips[i][0].shape[1], clips[i][1], target_sr) for i in order)
    y = torch.empty(n_out, dtype=torch.float32, device=dev)
    ipos = opos = 0
    for sr, idx in groups.items():
        shapes = [tuple(clips[i][0].shape) for i in idx]
        n_g = sum(c * T for c, T in shapes)
        o_g = sum(c * out_len(T, sr, target_sr) for c, T in shapes)
        if mode == "torchaudio":
            resample.sinc_group_flat(flat[ipos:ipos + n_g], shapes, sr, target_sr, y[opos:opos + o_g], beta=float(kaiser_beta), **NODE_FILTER)
        else:
            resample.poly_group_flat(flat[ipos:ipos + n_g], shapes, sr, target_sr, y[opos:opos + o_g])
        ipos, opos = ipos + n_g, opos + o_g
    if to_host:
        host = torch.empty(n_out, dtype=torch.float32, pin_memory=True)
        host.copy_(y, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        y = host
    pos = 0
    for i in order:
        c, T = clips[i][0].shape
        n = out_len(T, clips[i][1], target_sr)
        out[i] = y[pos:pos + c * n].view(c, n)
        pos += c * n
    return out
