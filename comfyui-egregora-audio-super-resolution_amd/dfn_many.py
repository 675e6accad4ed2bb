"""Many clips through `Egregora DeepFilterNet Denoise` at once: denoise_many.

Per clip it does what Egregora_DeepFilterNet_Denoise.execute does -- optional downmix, rate conversion to 48 kHz, the network, rate
conversion back, pad / crop, VAD gains and mix -- but the clips share the launches wherever a ragged form exists: one
egr_resample_poly_tracks per source rate and direction, and the network through DfnEngine.enhance_many (one egr_dfn*_enhance_tracks
per wave, the clips' channels side by side whatever their lengths).  The VAD gains and the mix stay the single node's per-clip calls
(mix_on_device), enqueued one after another without a host wait; the results are downloaded at the end.  Every clip gets the bits
the single node gives it.

The packed path is taken exactly when the single node would run the native engine: no backend registered with set_enhancer, upstream
`df` not importable, a model directory of the chosen model found.  Otherwise the clips go through the single node one by one.
"""
from typing import List, Optional, Sequence, Tuple

import torch

from . import native, resample
from . import egregora_audio_enhance_extras as extras
from .many_common import check_clips, group_by_rate

WIDGET_DEFAULTS = dict(device="auto", use_postfilter=False, limit_ceiling=True, stereo_mode="per_channel", frame_ms=20, strength=0.65,
                       mix_curve="equal_power", adaptive_vad_source="rms", adaptive_mode="more_on_noise", adaptive_amount=0.45,
                       vad_threshold=0.90, vad_smooth_ms=60, post_gain_db=0.5, ceiling=0.98)


def native_engine(dfn_model: str, device: Optional[int] = None):
    """The native engine the single node would use for dfn_model, or None when it would use another backend (or find none)."""
    if extras._ENHANCER is not None:
        return None
    try:
        from df.enhance import enhance, init_df      # noqa: F401 -- the single node's own test of the upstream package
        return None
    except Exception:      # noqa: BLE001
        pass
    from . import dfn2_engine, dfn2_weights, dfn_engine, dfn_weights
    for weights, eng in ((dfn_weights, dfn_engine), (dfn2_weights, dfn2_engine)):
        model_dir = weights.discover(dfn_model)
        if model_dir is not None:
            return eng.engine(model_dir, device)
    return None


def denoise_many(clips: Sequence[Tuple[torch.Tensor, int]], dfn_model: str = "DeepFilterNet2", *, stats: Optional[dict] = None,
                 **widgets) -> List[torch.Tensor]:
    """clips: [([C,T] float tensor on the host or the device, sample_rate)]; widgets: the single node's, by name (WIDGET_DEFAULTS).
    -> [C', T] float32 host tensors in input order (C' = 1 with stereo_mode "downmix_mono"), each the single node's result for that
    clip.  stats, when given, receives packed (False: another backend ran clip by clip) and enhance_many's waves / alone."""
    unknown = set(widgets) - set(WIDGET_DEFAULTS)
    if unknown:
        raise TypeError(f"denoise_many: unknown widget(s) {sorted(unknown)}")
    w = dict(WIDGET_DEFAULTS, **widgets)
    native.require_device()
    clips = check_clips("denoise_many", clips)
    eng = native_engine(dfn_model, torch.cuda.current_device()) if clips else None
    if stats is not None:
        stats["packed"] = eng is not None
    if eng is None:                                 # the single node's backend order, clip by clip (it raises when there is none)
        node = extras.Egregora_DeepFilterNet_Denoise()
        return [node.execute({"waveform": x[None], "sample_rate": sr}, dfn_model, **w)[0]["waveform"][0] for x, sr in clips]
    srs = [sr for _, sr in clips]
    dry = []
    for x, _ in clips:
        x = x.float()
        if w["stereo_mode"] == "downmix_mono" and x.shape[0] != 1:
            x = x.mean(dim=0, keepdim=True)
        dry.append(x.contiguous().cuda())
    with torch.cuda.device(eng.device):
        dry48: List[torch.Tensor] = list(dry)
        groups = group_by_rate(srs, 48000)
        for sr, idx in groups.items():
            for i, y in zip(idx, resample.resample_poly_group([dry[i] for i in idx], sr, 48000)):
                dry48[i] = y
        wet48 = eng.enhance_many(dry48, stats=stats)
        wet: List[torch.Tensor] = list(wet48)
        for sr, idx in groups.items():
            for i, y in zip(idx, resample.resample_poly_group([wet48[i] for i in idx], 48000, sr)):
                wet[i] = y
        ys = []
        for i, d in enumerate(dry):
            T = d.shape[1]
            v = wet[i]
            if v.shape[1] != T:                     # polyphase lengths can differ by a sample after the round trip
                v = torch.nn.functional.pad(v, (0, max(0, T - v.shape[1])))[:, :T]
            vad_src = dry48[i].contiguous() if w["adaptive_vad_source"] == "rms" else None
            ys.append(extras.mix_on_device(d, v.contiguous(), vad_src, srs[i], w["strength"], w["mix_curve"], w["adaptive_mode"],
                                           w["adaptive_amount"], w["vad_threshold"], w["vad_smooth_ms"], w["post_gain_db"],
                                           w["limit_ceiling"], w["ceiling"]))
        return [y.cpu() for y in ys]


def meta_for(dfn_model: str, meta: Optional[dict] = None, **widgets) -> dict:
    """The meta the single node attaches to a result: the input's meta plus meta["deepfilternet"]."""
    w = dict(WIDGET_DEFAULTS, **widgets)
    node = extras.Egregora_DeepFilterNet_Denoise()
    out = dict(meta or {})
    out["deepfilternet"] = {
        "model": dfn_model, "device": node._pick_device(w["device"]), "use_postfilter": bool(w["use_postfilter"]),
        "stereo_mode": w["stereo_mode"], "frame_ms": w["frame_ms"], "strength": w["strength"], "mix_curve": w["mix_curve"],
        "adaptive_vad_source": w["adaptive_vad_source"], "adaptive_mode": w["adaptive_mode"], "adaptive_amount": w["adaptive_amount"],
        "vad_threshold": w["vad_threshold"], "vad_smooth_ms": w["vad_smooth_ms"], "post_gain_db": w["post_gain_db"],
        "limit_ceiling": bool(w["limit_ceiling"]), "ceiling": w["ceiling"],
    }
    return out
