"""ComfyUI nodes "Audio Null Test (batch)" and "Null Test (Full) (batch)": LISTS of AUDIO pairs through the null-test suite in ragged
passes per wave (null_many.py).

Opt-in (registered when EGREGORA_NULLTEST_BATCH_NODES is "1" at import, __init__.py); the reference pack has no such nodes.  `Audio Null
Test (batch)` has the single node's widgets; `Null Test (Full) (batch)` has the single node's without the draw_* flags and without the
three IMAGE outputs (the plots are host matplotlib: whoever wants them feeds a result to `Audio Plotter`).  Every list element is
coerced like the single node's input, except that an AUDIO dict whose waveform is [B,C,T] contributes B clips.  The two lists are paired
element by element after that expansion: lists of unequal length are refused.  Each result is what the single node returns for that
pair, metadata carried the same way.
"""
from . import native, null_many
from .audio_glue import eval_package
from .egregora_audio_eval_batch import _as_list, _tensor, clips_of
from .egregora_audio_super_resolution_batch import _first
from .egregora_null_test_suite import Audio_Null_Test, Null_Test_Full


def _paired(audio_ref, audio_proc, who: str):
    refs = [c for a in _as_list(audio_ref) for c in clips_of(a)]
    procs = [c for a in _as_list(audio_proc) for c in clips_of(a)]
    if len(refs) != len(procs):
        raise ValueError(f"{who}: {len(refs)} reference clips against {len(procs)} processed clips")
    return refs, procs


class Audio_Null_Test_Batch:
    INPUT_TYPES = Audio_Null_Test.INPUT_TYPES
    INPUT_IS_LIST = True
    OUTPUT_IS_LIST = (True, True)
    RETURN_TYPES = Audio_Null_Test.RETURN_TYPES
    RETURN_NAMES = Audio_Null_Test.RETURN_NAMES
    FUNCTION = Audio_Null_Test.FUNCTION
    CATEGORY = Audio_Null_Test.CATEGORY

    def execute(self, audio_ref, audio_proc_aligned_matched, invert_b=True, least_squares_scale=False, compute_corr=True,
                compute_null_rms=True, compute_null_lufs=True, compute_lsd=True, compute_hf_residual=False, n_fft=2048, hop=512,
                hf_band_hz=8000):
        refs, procs = _paired(audio_ref, audio_proc_aligned_matched, "Audio Null Test (batch)")
        for r, p in zip(refs, procs):
            if p["sample_rate"] != r["sample_rate"]:
                raise ValueError("Sample rate mismatch after alignment stage")
        if not refs:
            return ([], [])
        native.require_device()
        out = null_many.null_test_many([(_tensor(r), _tensor(p)) for r, p in zip(refs, procs)], [r["sample_rate"] for r in refs],
                                       bool(_first(invert_b, True)), bool(_first(least_squares_scale, False)), bool(_first(compute_corr, True)),
                                       bool(_first(compute_null_rms, True)), bool(_first(compute_null_lufs, True)),
                                       bool(_first(compute_lsd, True)), bool(_first(compute_hf_residual, False)), int(_first(n_fft, 2048)),
                                       int(_first(hop, 512)), int(_first(hf_band_hz, 8000)))
        return ([eval_package(r["sample_rate"], null.cpu().numpy(), {}) for r, (null, _) in zip(refs, out)], [m for _, m in out])


def _full_inputs():
    types = Null_Test_Full.INPUT_TYPES()
    return {"required": dict(types["required"]), "optional": {k: v for k, v in types["optional"].items() if not k.startswith("draw_")}}


class Null_Test_Full_Batch:
    INPUT_IS_LIST = True
    OUTPUT_IS_LIST = (True,) * 5
    RETURN_TYPES = Null_Test_Full.RETURN_TYPES[:5]
    RETURN_NAMES = Null_Test_Full.RETURN_NAMES[:5]
    FUNCTION = Null_Test_Full.FUNCTION
    CATEGORY = Null_Test_Full.CATEGORY

    @classmethod
    def INPUT_TYPES(cls):
        return _full_inputs()

    def execute(self, audio_ref, audio_proc, align_max_shift_ms=200, align_method="gcc-phat", fractional=True, fir_len=64,
                match_mode="LUFS-I", least_squares_scale=False, compute_corr=True, compute_null_rms=True, compute_null_lufs=True,
                compute_lsd=True, compute_hf_residual=False, n_fft=2048, hop=512):
        refs, procs = _paired(audio_ref, audio_proc, "Null Test (Full) (batch)")
        if not refs:
            return ([], [], [], [], [])
        native.require_device()
        out = null_many.full_many([(_tensor(r), _tensor(p)) for r, p in zip(refs, procs)],
                                  [(r["sample_rate"], p["sample_rate"]) for r, p in zip(refs, procs)], int(_first(align_max_shift_ms, 200)),
                                  str(_first(align_method, "gcc-phat")), bool(_first(fractional, True)), int(_first(fir_len, 64)),
                                  str(_first(match_mode, "LUFS-I")), bool(_first(least_squares_scale, False)), bool(_first(compute_corr, True)),
                                  bool(_first(compute_null_rms, True)), bool(_first(compute_null_lufs, True)), bool(_first(compute_lsd, True)),
                                  bool(_first(compute_hf_residual, False)), int(_first(n_fft, 2048)), int(_first(hop, 512)))
        matched = [eval_package(r["sample_rate"], o[0].cpu().numpy(), p.get("meta", {})) for r, p, o in zip(refs, procs, out)]
        nulls = [eval_package(r["sample_rate"], o[1].cpu().numpy(), {}) for r, o in zip(refs, out)]
        return (matched, nulls, [o[2] for o in out], [o[3] for o in out], [o[4] for o in out])


NODE_CLASS_MAPPINGS = {
    "Audio Null Test (batch)": Audio_Null_Test_Batch,
    "Null Test (Full) (batch)": Null_Test_Full_Batch,
}

NODE_DISPLAY_NAME_MAPPINGS = {k: k for k in NODE_CLASS_MAPPINGS}
