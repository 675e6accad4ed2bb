"""ComfyUI nodes "Metrics (LSD + SI-SDR) (batch)" and "Loudness Meter (BS1770) (batch)": LISTS of AUDIO values through the two
evaluation nodes in one ragged pass per wave (eval_many.py).

Opt-in (registered when EGREGORA_EVAL_BATCH_NODES is "1" at import, __init__.py); the reference pack has no such nodes.  Same widgets
as the single nodes (egregora_audio_eval_pack.py, egregora_audio_eval_loudness.py).  Every list element is coerced like the single
node's input, except that an AUDIO dict whose waveform is [B,C,T] contributes B clips where the single node reads element 0.  The
metrics node pairs its two lists element by element after that expansion: lists of unequal length are refused.  Each result is the
single node's dictionary.
"""
from typing import Any, Dict, List

import numpy as np
import torch

from . import eval_many
from .audio_glue import eval_audio as to_internal_audio, is_audio_dict
from .egregora_audio_eval_loudness import Loudness_Meter_1770
from .egregora_audio_eval_pack import Metrics_LSD_SISDR
from .egregora_audio_super_resolution_batch import _first


def clips_of(audio: Any) -> List[Dict[str, Any]]:
    """One list element -> its clips as the eval pack's internal dicts: B of them for a [B,C,T] waveform."""
    if is_audio_dict(audio):
        wf = audio["waveform"]
        if hasattr(wf, "ndim") and wf.ndim == 3 and wf.shape[0] > 1:
            return [to_internal_audio(dict(audio, waveform=wf[b:b + 1])) for b in range(wf.shape[0])]
    return [to_internal_audio(audio)]


def _as_list(v) -> list:
    if v is None or isinstance(v, dict) or not isinstance(v, (list, tuple)):
        return [v]
    return list(v)


def _tensor(a: Dict[str, Any]) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a["samples"], dtype=np.float32))


class Metrics_LSD_SISDR_Batch:
    INPUT_TYPES = Metrics_LSD_SISDR.INPUT_TYPES
    INPUT_IS_LIST = True
    OUTPUT_IS_LIST = (True,)
    RETURN_TYPES = Metrics_LSD_SISDR.RETURN_TYPES
    RETURN_NAMES = Metrics_LSD_SISDR.RETURN_NAMES
    FUNCTION = Metrics_LSD_SISDR.FUNCTION
    CATEGORY = Metrics_LSD_SISDR.CATEGORY

    def execute(self, audio_ref, audio_proc, n_fft=2048, hop=512, compute_lsd=True, compute_si_sdr=True):
        refs = [c for a in _as_list(audio_ref) for c in clips_of(a)]
        procs = [c for a in _as_list(audio_proc) for c in clips_of(a)]
        if len(refs) != len(procs):
            raise ValueError(f"Metrics (batch): {len(refs)} reference clips against {len(procs)} processed clips")
        pairs = [(_tensor(r), _tensor(p)) for r, p in zip(refs, procs)]
        return (eval_many.metrics_many(pairs, int(_first(n_fft, 2048)), int(_first(hop, 512)), bool(_first(compute_lsd, True)),
                                       bool(_first(compute_si_sdr, True))),)


class Loudness_Meter_1770_Batch:
    INPUT_TYPES = Loudness_Meter_1770.INPUT_TYPES
    INPUT_IS_LIST = True
    OUTPUT_IS_LIST = (True,)
    RETURN_TYPES = Loudness_Meter_1770.RETURN_TYPES
    RETURN_NAMES = Loudness_Meter_1770.RETURN_NAMES
    FUNCTION = Loudness_Meter_1770.FUNCTION
    CATEGORY = Loudness_Meter_1770.CATEGORY

    def execute(self, audio, compute_true_peak=True, oversample=4):
        clips = [c for a in _as_list(audio) for c in clips_of(a)]
        return (eval_many.loudness_many([(_tensor(c), c["sample_rate"]) for c in clips], bool(_first(compute_true_peak, True)),
                                        int(_first(oversample, 4))),)


NODE_CLASS_MAPPINGS = {
    "Metrics (LSD + SI-SDR) (batch)": Metrics_LSD_SISDR_Batch,
    "Loudness Meter (BS1770) (batch)": Loudness_Meter_1770_Batch,
}

NODE_DISPLAY_NAME_MAPPINGS = {
    "Metrics (LSD + SI-SDR) (batch)": "Egregora Metrics (LSD + SI-SDR) (batch)",
    "Loudness Meter (BS1770) (batch)": "Egregora Loudness Meter (BS1770) (batch)",
}
