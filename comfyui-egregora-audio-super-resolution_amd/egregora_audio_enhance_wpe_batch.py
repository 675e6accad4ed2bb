"""ComfyUI node "Egregora WPE Dereverb (batch)": a LIST of AUDIO values through the dereverberation in one ragged pass per wave.

Opt-in (registered when EGREGORA_ENHANCE_BATCH_NODES is "1" at import, __init__.py); the reference pack has no such node.  Same widgets
as the single node (egregora_audio_enhance_wpe.py).  Every list element is coerced like the single node's input; an AUDIO dict (or
tensor) whose waveform is [B,C,T] contributes B clips.  The clips go through wpe_many.dereverb_many; each result is packaged like the
single node's (float32, CPU, contiguous [1,C,T'], the input's meta plus meta["wpe"]) and has its bits.
"""
import torch

from . import wpe_many
from .egregora_audio_enhance_dfn_batch import clips_of
from .egregora_audio_enhance_extras import _make_audio
from .egregora_audio_enhance_wpe import Egregora_WPE_Dereverb
from .egregora_audio_super_resolution_batch import _first


class Egregora_WPE_DereverbBatch:
    INPUT_TYPES = Egregora_WPE_Dereverb.INPUT_TYPES
    INPUT_IS_LIST = True
    OUTPUT_IS_LIST = (True,)
    RETURN_TYPES = Egregora_WPE_Dereverb.RETURN_TYPES
    FUNCTION = Egregora_WPE_Dereverb.FUNCTION
    CATEGORY = Egregora_WPE_Dereverb.CATEGORY

    def execute(self, audio=None, **widgets):
        from .audio_glue import is_audio_dict
        if audio is None or is_audio_dict(audio) or not isinstance(audio, (list, tuple)):
            audio = [audio]
        unknown = set(widgets) - set(wpe_many.WIDGET_DEFAULTS)
        if unknown:
            raise TypeError(f"execute() got unexpected widget(s) {sorted(unknown)}")
        w = {k: _first(v, wpe_many.WIDGET_DEFAULTS[k]) for k, v in widgets.items()}
        clips = [c for a in audio for c in clips_of(a)]
        ys = wpe_many.dereverb_many([(x, sr) for x, sr, _ in clips], **w)
        return ([_make_audio(sr, y.to(torch.float32).cpu().reshape(1, y.shape[0], -1), wpe_many.meta_for(meta, **w))
                 for y, (_, sr, meta) in zip(ys, clips)],)


NODE_CLASS_MAPPINGS = {"Egregora_WPE_DereverbBatch": Egregora_WPE_DereverbBatch}
NODE_DISPLAY_NAME_MAPPINGS = {"Egregora_WPE_DereverbBatch": "Egregora WPE Dereverb (batch)"}
