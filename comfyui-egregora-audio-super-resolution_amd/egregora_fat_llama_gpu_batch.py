"""ComfyUI node "Spectral Enhance (Fat Llama - GPU, batch)": a LIST of AUDIO values through the Fat-Llama loop in packed waves
(fatllama_many).

Opt-in (registered when EGREGORA_FATLLAMA_BATCH_NODES is "1" at import, __init__.py); the reference pack has no such node.  Same
widgets as EgregoraFatLlamaGPU.  Every list element is resolved like the single node's input; an AUDIO whose waveform is [B,C,T] counts as
B clips.  Each output AUDIO is shaped like the single node's for that clip ([1,C,T*f] at the clip's own output rate); its samples
are the single node's bit for bit for the largest clip of a wave and for the clips that run one by one, and within one PCM_16 step
of it otherwise (fatllama_many).
"""
import torch

from . import audio_glue, fatllama_many, native
from .egregora_audio_super_resolution_batch import _first
from .egregora_fat_llama_gpu import CATEGORY, FUNCTION, EgregoraFatLlamaGPU, check_format, resolve_input


def _clips(AUDIO):
    """The list input -> [([C,T] tensor, sr)]: a [B,C,T] waveform counts as B clips."""
    if AUDIO is None:
        raise RuntimeError("No AUDIO provided.")
    elems = [AUDIO] if audio_glue.is_audio_dict(AUDIO) or not isinstance(AUDIO, (list, tuple)) else list(AUDIO)
    clips = []
    for a in elems:
        w = a.get("waveform") if audio_glue.is_audio_dict(a) else None
        if torch.is_tensor(w) and w.dim() == 3 and w.shape[0] > 1:
            clips += [(w[b].detach().float(), int(a["sample_rate"])) for b in range(w.shape[0])]
        else:
            clips.append(resolve_input(a))
    return clips


class EgregoraFatLlamaGPUBatch:
    """EgregoraFatLlamaGPU over a list of clips: clips without a packed plan share launches."""

    @classmethod
    def INPUT_TYPES(cls):
        t = EgregoraFatLlamaGPU.INPUT_TYPES()
        return {"required": dict(t["required"]), "optional": {"AUDIO": ("AUDIO",)}}

    INPUT_IS_LIST = True
    OUTPUT_IS_LIST = (True,)
    RETURN_TYPES = EgregoraFatLlamaGPU.RETURN_TYPES
    FUNCTION = FUNCTION
    CATEGORY = CATEGORY
    OUTPUT_NODE = False

    def run(self, target_format, max_iterations, threshold_value, target_bitrate_kbps, toggle_normalize, toggle_autoscale, AUDIO=None):
        native.require_device()
        check_format(_first(target_format, "wav"))
        res = fatllama_many.enhance_many(_clips(AUDIO), int(_first(max_iterations, 300)), float(_first(threshold_value, 0.6)),
                                         int(_first(target_bitrate_kbps, 1411)), bool(_first(toggle_normalize, True)),
                                         bool(_first(toggle_autoscale, True)))
        return ([audio_glue.package(sr, y) for y, sr in res],)


NODE_CLASS_MAPPINGS = {"EgregoraFatLlamaGPUBatch": EgregoraFatLlamaGPUBatch}
NODE_DISPLAY_NAME_MAPPINGS = {"EgregoraFatLlamaGPUBatch": "🎛️ Spectral Enhance (Fat Llama — GPU, batch)"}
