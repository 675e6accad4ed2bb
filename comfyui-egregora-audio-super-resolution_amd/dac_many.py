"""Many clips through `Egregora DAC Encode` / `Egregora DAC Decode` at once: encode_many / decode_many.

Per clip they do what the single nodes do -- rate conversion to the model's rate, the codec, rate conversion back -- but the clips
share the launches: one egr_resample_poly_tracks per source rate and direction (the bits of the single call's resample.resample_hq;
with EGREGORA_SINC_RESAMPLE=1 one egr_resample_sinc_tracks, the bits of resample.resample_sinc: resample.codec_resample decides),
and the codec through DacEngine.encode_many / decode_many (one egr_dacmany_encode / _decode per wave, rows of their own lengths
inside tensors of the wave's longest).  The clips go up in one transfer and the results come down in one transfer per tensor kind.
A clip's result equals the single node's to fp32 round-off (the launcher chooses tiles from the padded shape), not bit for bit.
"""
from typing import List, Optional, Sequence, Tuple

import torch

from . import dac_engine, dac_weights, native, resample
from .many_common import check_clips, download, group_by_rate, upload


def engine_for(model_type: str) -> "dac_engine.DacEngine":
    path = dac_weights.discover(model_type)
    if path is None:
        raise RuntimeError(dac_weights.not_found_message(model_type))
    native.require_device()
    return dac_engine.engine(path)


def _to_rate(xs: List[torch.Tensor], srs: Sequence[int], target: Optional[int], back: bool = False) -> List[torch.Tensor]:
    """Every xs[i] from srs[i] to `target` (back: from `target` to srs[i]), one resample call per distinct rate."""
    out = list(xs)
    for sr, idx in group_by_rate(srs, target).items():
        a, b = (target, sr) if back else (sr, target)
        for i, y in zip(idx, resample.codec_resample([xs[i] for i in idx], a, b)):
            out[i] = y
    return out


def encode_many(clips: Sequence[Tuple[torch.Tensor, int]], model_type: str = "44khz", *, stats: Optional[dict] = None) -> List[dict]:
    """clips: [([C, T] float tensor on the host or the device, sample_rate)] -> per clip, in input order, {"z": float32 [C, latent,
    frames], "codes": int64 [C, n_codebooks, frames] (both on the host), "sample_rate", "model_sample_rate", "n_samples"}."""
    clips = check_clips("encode_many", clips)
    if not clips:
        return []
    eng = engine_for(model_type)
    model_sr = int(eng.cfg["sample_rate"])
    dev = torch.device("cuda", eng.device)
    with torch.cuda.device(eng.device):
        xs = upload([x for x, _ in clips], dev, torch.float32)
        xs = [x.contiguous() for x in _to_rate(xs, [sr for _, sr in clips], model_sr)]
        res = eng.encode_many(xs, stats=stats)
        zs = download([z for z, _ in res])
        cs = download([c for _, c in res])
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
        for i, t in zip(zi, upload([items[i]["z"] for i in zi], dev, torch.float32)):
            ts[i] = t
        for i, t in zip(ci, upload([items[i]["codes"] for i in ci], dev, torch.int32)):
            ts[i] = t
        ys = eng.decode_many(ts, stats=stats)
        ys = _to_rate([y.contiguous() for y in ys], srs, model_sr, back=True)
        return download(ys)
