"""The host layer the many-clip modules (*_many.py) share: the clip check, grouping by rate, the channel-row tables of clips laid back
to back, the one-transfer upload / download and the GiB budgets.  It imports no engine, so every module may import it at the top.
"""
import os
from typing import Dict, List, Optional, Sequence, Tuple

import torch


def check_clips(who: str, clips, allow_empty: bool = False) -> List[Tuple[torch.Tensor, int]]:
    """clips: [(x, sample_rate)] -> [(x, int(sample_rate))], each x a [C, T] tensor with C >= 1, T >= 1 (allow_empty: T >= 0) and a
    rate of at least 1; ValueError naming `who` and the clip otherwise."""
    clips = [(x, int(sr)) for x, sr in clips]
    what = "a [C, T] tensor" if allow_empty else "a non-empty [C, T] tensor"
    for i, (x, sr) in enumerate(clips):
        if not torch.is_tensor(x) or x.dim() != 2 or x.shape[0] < 1 or (x.shape[1] < 1 and not allow_empty) or sr < 1:
            raise ValueError(f"{who}: clip {i}: expected {what} and a positive sample rate")
    return clips


def group_by_rate(srs: Sequence[int], skip: Optional[int]) -> Dict[int, List[int]]:
    """{rate: indices of srs at that rate}, rates in first-seen order and indices ascending, without the rate `skip`."""
    groups: Dict[int, List[int]] = {}
    for i, sr in enumerate(srs):
        if sr != skip:
            groups.setdefault(sr, []).append(i)
    return groups


def track_rows(shapes, base: int = 0):
    """(ins, lens) of clips [C_i][T_i] laid back to back from `base` (shapes = [(C_i, T_i)]): one row per channel, its offset and
    its length."""
    ins, lens, pos = [], [], int(base)
    for c, T in shapes:
        ins += [pos + k * T for k in range(c)]
        lens += [T] * c
        pos += c * T
    return ins, lens


def clip_views(y: torch.Tensor, tab, shapes) -> List[torch.Tensor]:
    """The clips' [C_i, n_out_i] views of the flat result y of a tracks call on track_rows(shapes): tab is the call's table, whose
    columns 2 and 3 hold each row's output offset and length (a clip's rows are adjacent: its first row places it)."""
    out, t = [], 0
    for c, _ in shapes:
        o, n = int(tab[t, 2]), int(tab[t, 3])
        out.append(y[o:o + c * n].view(c, n))
        t += c
    return out


def upload(xs: Sequence[torch.Tensor], dev: torch.device, dtype: torch.dtype) -> List[torch.Tensor]:
    """Host tensors to the device in one transfer (tensors already there are taken as they are)."""
    host = [i for i, x in enumerate(xs) if not x.is_cuda]
    out = [x if x.is_cuda else None for x in xs]
    if host:
        flat = torch.cat([xs[i].to(dtype).reshape(-1) for i in host]).to(dev)
        pos = 0
        for i in host:
            n = xs[i].numel()
            out[i] = flat[pos:pos + n].view(xs[i].shape)
            pos += n
    return [x.to(dev, dtype) for x in out]


def download(xs: Sequence[torch.Tensor]) -> List[torch.Tensor]:
    """Device tensors of one dtype to the host in one transfer."""
    if not xs:
        return []
    flat = torch.cat([x.reshape(-1) for x in xs]).cpu()
    out, pos = [], 0
    for x in xs:
        out.append(flat[pos:pos + x.numel()].view(x.shape))
        pos += x.numel()
    return out


def budget_bytes(env_name: str, default_gb, override: Optional[int] = None) -> int:
    """`override` when given, else the GiB in the environment variable env_name (read now; default_gb when unset) as bytes."""
    if override is not None:
        return int(override)
    return int(float(os.environ.get(env_name, default_gb)) * 2 ** 30)
