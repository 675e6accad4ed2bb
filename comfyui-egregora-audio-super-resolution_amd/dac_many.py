"""Many clips through `Egregora DAC Encode` / `Egregora DAC Decode` at once: encode_many / decode_many.

Per clip they do what the single nodes do -- rate conversion to the model's rate, the codec, rate conversion back -- but the clips
share the launches: one egr_resample_poly_tracks per source rate and direction (the bits of the single call's resample.resample_hq;
with EGREGORA_SINC_RESAMPLE=1 one egr_resample_sinc_tracks, the bits of resample.resample_sinc: resample.codec_resample decides),
and the codec through DacEngine.encode_many / decode_many (one egr_dacmany_encode / _decode per wave, rows of their own lengths
inside tensors of the wave's longest).  The clips go up in one transfer and the results come down in one transfer per tensor kind.
A clip's result equals the single node's to fp32 round-off (the launcher chooses tiles from the padded shape), not bit for bit.
"""
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import dac_engine, dac_weights, native, resample


def engine_for(model_type: str) -> "dac_engine.DacEngine":
    path = dac_weights.discover(model_type)
    if path is None:
        raise RuntimeError(dac_weights.not_found_message(model_type))
    native.require_device()
    return dac_engine.engine(path)


def _to_rate(xs: List[torch.Tensor], srs: Sequence[int], target: Optional[int], back: bool = False) -> List[torch.Tensor]:
    """Every xs[i] from srs[i] to `target` (back: from `target` to srs[i]), one resample call per distinct rate."""
    groups: Dict[int, List[int]] = {}
    for i, sr in enumerate(srs):
        if sr != target:
            groups.setdefault(sr, []).append(i)
    out = list(xs)
    for sr, idx in groups.items():
        a, b = (target, sr) if back else (sr, target)
        for i, y in zip(idx, resample.codec_resample([xs[i] for i in idx], a, b)):
            out[i] = y
    return out


def _upload(xs: Sequence[torch.Tensor], dev: torch.device, dtype: torch.dtype) -> List[torch.Tensor]:
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


def _download(xs: Sequence[torch.Tensor]) -> List[torch.Tensor]:
    """Device tensors of one dtype to the host in one transfer."""
    if not xs:
        return []
    flat = torch.cat([x.reshape(-1) for x in xs]).cpu()
    out, pos = [], 0
    for x in xs:
        out.append(flat[pos:pos + x.numel()].view(x.shape))
        pos += x.numel()
    return out


def encode_many(clips: Sequence[Tuple[torch.Tensor, int]], model_type: str = "44khz", *, stats: Optional[dict] = None) -> List[dict]:
    """clips: [([C, T] float tensor on the host or the device, sample_rate)] -> per clip, in input order, {"z": float32 [C, latent,
    frames], "codes": int64 [C, n_codebooks, frames] (both on the host), "sample_rate", "model_sample_rate", "n_samples"}."""
    clips = [(x, int(sr)) for x, sr in clips]
    for i, (x, sr) in enumerate(clips):
        if not torch.is_tensor(x) or x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1 or sr < 1:
            raise ValueError(f"encode_many: clip {i}: expected a non-empty [C, T] tensor and a positive sample rate")
    if not clips:
        return []
    eng = engine_for(model_type)
    model_sr = int(eng.cfg["sample_rate"])
    dev = torch.device("cuda", eng.device)
    with torch.cuda.device(eng.device):
        xs = _upload([x for x, _ in clips], dev, torch.float32)
        xs = [x.contiguous() for x in _to_rate(xs, [sr for _, sr in clips], model_sr)]
        res = eng.encode_many(xs, stats=stats)
        zs = _download([z for z, _ in res])
        cs = _download([c for _, c in res])
    return [{"z": z, "codes": c.to(torch.int64), "sample_rate": sr, "model_sample_rate": model_sr, "n_samples": int(x.shape[1])}
            for z, c, (x, sr) in zip(zs, cs, clips)]


def decode_many(items: Sequence[dict], model_type: str = "44khz", *, stats: Optional[dict] = None) -> List[torch.Tensor]:
    """items: dicts with "z" (float [C, latent, frames]) or, without it, "codes" (integer [C, n_codebooks, frames]), and optionally
    "sample_rate" (the rate to return at; default the model's) -> float32 host tensors [C, samples] in input order, not trimmed."""
    if not items:
        return []
    eng = engine_for(model_type)
    model_sr = int(eng.cfg["sample_rate"])
    dev = torch.device("cuda", eng.device)
    srs = [int(d.get("sample_rate", model_sr)) for d in items]
    lat = [d.get("z") is not None for d in items]
    for i, d in enumerate(items):
        if not lat[i] and d.get("codes") is None:
            raise ValueError(f"decode_many: item {i} has neither z nor codes")
    with torch.cuda.device(eng.device):
        zi = [i for i in range(len(items)) if lat[i]]
        ci = [i for i in range(len(items)) if not lat[i]]
        ts: List = [None] * len(items)
        for i, t in zip(zi, _upload([items[i]["z"] for i in zi], dev, torch.float32)):
            ts[i] = t
        for i, t in zip(ci, _upload([items[i]["codes"] for i in ci], dev, torch.int32)):
            ts[i] = t
        ys = eng.decode_many(ts, stats=stats)
        ys = _to_rate([y.contiguous() for y in ys], srs, model_sr, back=True)
        return _download(ys)
