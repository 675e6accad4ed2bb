"""ComfyUI node "Egregora DeepFilterNet Denoise (batch)": a LIST of AUDIO values through the denoiser in one ragged pass per wave.

Opt-in (registered when EGREGORA_DENOISE_BATCH_NODES is "1" at import, __init__.py); the reference pack has no such node.  Same
widgets as the single node (egregora_audio_enhance_extras.py).  Every list element is coerced like the single node's input; an AUDIO
dict (or tensor) whose waveform is [B,C,T] contributes B clips.  The clips go through dfn_many.denoise_many; each result is packaged
like the single node's (float32, CPU, contiguous [1,C,T], the input's meta plus meta["deepfilternet"]) and has its bits.
"""
from typing import Any, List, Tuple

import torch

from . import dfn_many
from .egregora_audio_enhance_extras import Egregora_DeepFilterNet_Denoise, _coerce_audio, _make_audio
from .egregora_audio_super_resolution_batch import _first


def clips_of(audio: Any) -> List[Tuple[Any, int, dict]]:
    """One list element -> its clips as ([C,T] tensor, sample rate, meta): B of them for a [B,C,T] waveform."""
    wav, sr, meta = _coerce_audio(audio)
    return [(wav[b], sr, meta) for b in range(wav.shape[0])]


class Egregora_DeepFilterNet_DenoiseBatch:
    INPUT_TYPES = Egregora_DeepFilterNet_Denoise.INPUT_TYPES
    INPUT_IS_LIST = True
    OUTPUT_IS_LIST = (True,)
    RETURN_TYPES = Egregora_DeepFilterNet_Denoise.RETURN_TYPES
    FUNCTION = Egregora_DeepFilterNet_Denoise.FUNCTION
    CATEGORY = Egregora_DeepFilterNet_Denoise.CATEGORY

    def execute(self, audio=None, dfn_model="DeepFilterNet2", **widgets):
        from .audio_glue import is_audio_dict
        if audio is None or is_audio_dict(audio) or not isinstance(audio, (list, tuple)):
            audio = [audio]
        clips = [c for a in audio for c in clips_of(a)]
        model = _first(dfn_model, "DeepFilterNet2")
        w = {k: _first(v, dfn_many.WIDGET_DEFAULTS[k]) for k, v in widgets.items() if k in dfn_many.WIDGET_DEFAULTS}
        unknown = set(widgets) - set(dfn_many.WIDGET_DEFAULTS)
        if unknown:
            raise TypeError(f"execute() got unexpected widget(s) {sorted(unknown)}")
        ys = dfn_many.denoise_many([(x, sr) for x, sr, _ in clips], model, **w)
        return ([_make_audio(sr, y.to(torch.float32).cpu().reshape(1, y.shape[0], -1), dfn_many.meta_for(model, meta, **w))
                 for y, (_, sr, meta) in zip(ys, clips)],)


NODE_CLASS_MAPPINGS = {"Egregora_DeepFilterNet_DenoiseBatch": Egregora_DeepFilterNet_DenoiseBatch}
NODE_DISPLAY_NAME_MAPPINGS = {"Egregora_DeepFilterNet_DenoiseBatch": "Egregora DeepFilterNet Denoise (batch)"}
