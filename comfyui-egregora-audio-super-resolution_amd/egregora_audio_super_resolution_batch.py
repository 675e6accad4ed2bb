"""ComfyUI node "Audio Super Resolution (FlashSR, batch)": a LIST of AUDIO values through FlashSR in packed waves.

Opt-in (registered when EGREGORA_BATCH_NODES is "1" at import, __init__.py); the reference pack has no such node.  Same three
widgets as the single node (egregora_audio_super_resolution.py).  Every list element is coerced like the single node's input
(audio_glue.upscaler_input), except that an AUDIO dict whose waveform is [B,C,T] with B > 1 contributes B clips -- the single node
keeps the reference's "batch element 0 only" (quirk Q4).  The clips' rows share the model's batch dimension
(flashsr_engine.upscale_many: the number of library calls follows the number of sample rates, not of clips); each result is
packaged like the single node's (float32, CPU, contiguous [1,C,T]).
"""
from typing import Any, List, Tuple

import torch

from . import audio_glue, flashsr_engine
from .egregora_audio_super_resolution import CATEGORY, FUNCTION, EgregoraAudioSuperResolution


def clips_of(audio: Any) -> List[Tuple[torch.Tensor, int]]:
    """One list element -> its clips: B of them for an AUDIO dict with a [B,C,T] waveform, otherwise upscaler_input's one."""
    if audio_glue.is_audio_dict(audio):
        wf = audio["waveform"]
        if torch.is_tensor(wf) and wf.dim() == 3 and wf.shape[0] > 1:
            return [audio_glue.upscaler_input({"waveform": wf[b], "sample_rate": audio["sample_rate"]}) for b in range(wf.shape[0])]
    return [audio_glue.upscaler_input(audio)]


def _first(v, default):
    """Widgets of an INPUT_IS_LIST node arrive as one-element lists."""
    if isinstance(v, (list, tuple)):
        return v[0] if len(v) else default
    return v


class EgregoraAudioSuperResolutionBatch:
    INPUT_TYPES = EgregoraAudioSuperResolution.INPUT_TYPES
    INPUT_IS_LIST = True
    OUTPUT_IS_LIST = (True,)
    RETURN_TYPES = ("AUDIO",)
    FUNCTION = FUNCTION
    CATEGORY = CATEGORY
    OUTPUT_NODE = False

    def run(self, audio=None, lowpass_input=False, output_sr="48000"):
        if audio is None or audio_glue.is_audio_dict(audio) or not isinstance(audio, (list, tuple)):
            audio = [audio]
        clips = [c for a in audio for c in clips_of(a)]
        tgt = int(_first(output_sr, "48000"))
        ys = flashsr_engine.upscale_many(clips, bool(_first(lowpass_input, False)), tgt)
        return ([audio_glue.package(tgt, y) for y in ys],)


NODE_CLASS_MAPPINGS = {"EgregoraAudioUpscalerBatch": EgregoraAudioSuperResolutionBatch}
NODE_DISPLAY_NAME_MAPPINGS = {"EgregoraAudioUpscalerBatch": "🎧 Audio Super Resolution (FlashSR, batch)"}
