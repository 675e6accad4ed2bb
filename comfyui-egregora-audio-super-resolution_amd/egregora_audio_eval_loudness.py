"""The remaining four nodes of the reference's evaluation pack (egregora_audio_eval_pack.py:232-382): `Loudness Meter (BS1770)`,
`Audio Gain Match (1770)`, `ABX Prepare` and `ABX Judge`, with the reference's mapping keys, display names, INPUT_TYPES /
RETURN_TYPES / RETURN_NAMES / FUNCTION / CATEGORY and `execute` signatures (fixture G15).

The two loudness nodes measure on the device (loudness.py: K-weighting, channel mean, block energies and true peak in
libegregora_amd.so; the gate and the percentiles over the block values in the reference's numpy expressions) and have no CPU
fallback: without the library or a gfx950 device `execute` raises.  The ABX nodes slice and pick on the host and need no device.

Registration is opt-in: the package merges this module's mappings only when EGREGORA_EVAL_NODES=1 is set at import.
"""
import random
from typing import Any, Dict

import numpy as np
import torch

from . import device_ops, loudness, native
from .audio_glue import eval_audio as to_internal_audio, eval_package as make_audio


def _rng(default, lo, hi, step):
    return dict(zip(("default", "min", "max", "step"), (default, lo, hi, step)))


def _device_cn(samples: np.ndarray) -> torch.Tensor:
    native.require_device()
    return torch.from_numpy(np.ascontiguousarray(samples, dtype=np.float32)).cuda()


class ABX_Prepare:
    CATEGORY = "Egregora/Listening"
    RETURN_TYPES = ("AUDIO", "AUDIO", "AUDIO", "DICT")
    RETURN_NAMES = ("audio_A", "audio_B", "audio_X", "abx_meta")
    FUNCTION = "execute"

    @classmethod
    def INPUT_TYPES(cls):
        return {"required": {"audio_A": ("AUDIO", {}), "audio_B": ("AUDIO", {})},
                "optional": {"clip_seconds": ("FLOAT", _rng(10.0, 1.0, 60.0, 0.1)),
                             "random_seed": ("INT", _rng(0, 0, 2**31 - 1, 1)),
                             "start_seconds": ("FLOAT", _rng(0.0, 0.0, 10_000.0, 0.1))}}

    def _clip(self, a: Dict[str, Any], start_s: float, dur_s: float) -> Dict[str, Any]:
        # the clip rule of :252-260: a clip that runs past the end is cut there
        sr = a["sample_rate"]
        s = int(round(start_s * sr))
        n = int(round(dur_s * sr))
        x = a["samples"]
        if s + n > x.shape[1]:
            n = max(0, x.shape[1] - s)
        return make_audio(sr, x[:, s:s + n], a.get("meta", {}))

    def execute(self, audio_A, audio_B, clip_seconds=10.0, random_seed=0, start_seconds=0.0):
        A = to_internal_audio(audio_A)
        B = to_internal_audio(audio_B)
        n = min(A["samples"].shape[1], B["samples"].shape[1])
        A["samples"] = A["samples"][:, :n]
        B["samples"] = B["samples"][:, :n]
        A_c = self._clip(A, start_seconds, clip_seconds)
        B_c = self._clip(B, start_seconds, clip_seconds)
        x_is = random.Random(int(random_seed)).choice(["A", "B"])
        X = A_c if x_is == "A" else B_c
        return A_c, B_c, X, {"x_is": x_is, "seed": int(random_seed)}


class ABX_Judge:
    CATEGORY = "Egregora/Listening"
    RETURN_TYPES = ("DICT",)
    RETURN_NAMES = ("abx_result",)
    FUNCTION = "execute"

    @classmethod
    def INPUT_TYPES(cls):
        return {"required": {"abx_meta": ("DICT", {}), "guess": (["A", "B"], {})}}

    def execute(self, abx_meta, guess):
        x_is = str(abx_meta.get("x_is", "?")).upper()
        return ({"x_is": x_is, "guess": guess.upper(), "correct": bool(guess.upper() == x_is)},)


class Loudness_Meter_1770:
    CATEGORY = "Egregora/Analysis"
    RETURN_TYPES = ("DICT",)
    RETURN_NAMES = ("metrics",)
    FUNCTION = "execute"

    @classmethod
    def INPUT_TYPES(cls):
        return {"required": {"audio": ("AUDIO", {})},
                "optional": {"compute_true_peak": ("BOOLEAN", {"default": True}), "oversample": ("INT", _rng(4, 1, 8, 1))}}

    def execute(self, audio, compute_true_peak=True, oversample=4):
        a = to_internal_audio(audio)
        return (loudness.measure(_device_cn(a["samples"]), a["sample_rate"], bool(compute_true_peak), int(oversample)),)


class Audio_Gain_Match_1770:
    CATEGORY = "Egregora/Analysis"
    RETURN_TYPES = ("AUDIO", "FLOAT", "FLOAT", "FLOAT")
    RETURN_NAMES = ("audio_matched", "gain_db", "ref_level", "in_level")
    FUNCTION = "execute"

    @classmethod
    def INPUT_TYPES(cls):
        return {"required": {"audio_ref": ("AUDIO", {}), "audio_in": ("AUDIO", {})},
                "optional": {"mode": (["LUFS-I", "RMS"], {}), "max_gain_db": ("FLOAT", _rng(12.0, -60.0, 60.0, 0.1))}}

    def execute(self, audio_ref, audio_in, mode="LUFS-I", max_gain_db=12.0):
        ref = to_internal_audio(audio_ref)
        inn = to_internal_audio(audio_in)
        sr = ref["sample_rate"]
        r, x = _device_cn(ref["samples"]), _device_cn(inn["samples"])
        if inn["sample_rate"] != sr:
            # the reference's np.interp resampling with its own length rule (:362-370)
            x = device_ops.resample_linear(x, int(round(x.shape[1] * sr / inn["sample_rate"])))
        if str(mode).upper().startswith("LUFS"):
            ref_level, in_level = loudness.integrated(r, sr), loudness.integrated(x, sr)
        else:
            ref_level, in_level = device_ops.rms_db(r), device_ops.rms_db(x)
        gain_db = float(np.clip(ref_level - in_level, -abs(max_gain_db), abs(max_gain_db)))
        y = device_ops.scale(x, 10 ** (gain_db / 20.0))
        return (make_audio(sr, y.cpu().numpy(), inn.get("meta", {})), float(gain_db), float(ref_level), float(in_level))


NODE_CLASS_MAPPINGS = {
    "ABX Prepare": ABX_Prepare,
    "ABX Judge": ABX_Judge,
    "Loudness Meter (BS1770)": Loudness_Meter_1770,
    "Audio Gain Match (1770)": Audio_Gain_Match_1770,
}

NODE_DISPLAY_NAME_MAPPINGS = {
    "ABX Prepare": "Egregora ABX Prepare",
    "ABX Judge": "Egregora ABX Judge",
    "Loudness Meter (BS1770)": "Egregora Loudness Meter (BS1770)",
    "Audio Gain Match (1770)": "Egregora Audio Gain Match (1770)",
}
