"""ComfyUI node "Resample Audio (HQ) (batch)": a LIST of AUDIO values through `Resample Audio (HQ)` with one library call per source
rate (resample_many.py).

Opt-in (registered when EGREGORA_RESAMPLE_BATCH_NODES is "1" at import, __init__.py); the reference pack has no such node.  Same
widgets as the single node (egregora_audio_eval_pack.py).  Every list element is coerced like the single node's input, except that an
AUDIO dict whose waveform is [B,C,T] contributes B clips where the single node reads element 0.  Modes "auto" and "scipy_polyphase"
give each clip the single node's samples; "torchaudio" runs the windowed-sinc kernel at the reference's filter (64, 0.945, Kaiser,
the widget's beta) whether or not EGREGORA_SINC_RESAMPLE is set; "linear" has no ragged form and goes through the single node clip
by clip.
"""
from . import resample_many as rm
from .audio_glue import eval_package as make_audio
from .egregora_audio_eval_batch import _as_list, _tensor, clips_of
from .egregora_audio_eval_pack import Resample_Audio_HQ
from .egregora_audio_super_resolution_batch import _first


class Resample_Audio_HQ_Batch:
    INPUT_TYPES = Resample_Audio_HQ.INPUT_TYPES
    INPUT_IS_LIST = True
    OUTPUT_IS_LIST = (True,)
    RETURN_TYPES = Resample_Audio_HQ.RETURN_TYPES
    RETURN_NAMES = Resample_Audio_HQ.RETURN_NAMES
    FUNCTION = Resample_Audio_HQ.FUNCTION
    CATEGORY = Resample_Audio_HQ.CATEGORY

    def execute(self, audio, target_sr=48000, mode="auto", kaiser_beta=14.769):
        clips = [c for a in _as_list(audio) for c in clips_of(a)]
        target_sr, mode, beta = int(_first(target_sr, 48000)), _first(mode, "auto"), float(_first(kaiser_beta, 14.769))
        if mode not in rm.MODES:
            single = Resample_Audio_HQ()
            return ([single.execute(c, target_sr, mode, beta)[0] for c in clips],)
        ys = rm.resample_many([(_tensor(c), c["sample_rate"]) for c in clips], target_sr, mode, beta)
        return ([c if int(c["sample_rate"]) == target_sr else make_audio(target_sr, y.numpy(), c.get("meta", {}))
                 for c, y in zip(clips, ys)],)


NODE_CLASS_MAPPINGS = {"Resample Audio (HQ) (batch)": Resample_Audio_HQ_Batch}
NODE_DISPLAY_NAME_MAPPINGS = {"Resample Audio (HQ) (batch)": "Egregora Resample Audio (HQ) (batch)"}
