"""`Egregora WPE Dereverb` with the reference's plugin surface (egregora_audio_enhance_extras.py:368-443, fixture G16), computed by
this pack's own kernels (wpe_engine.py, csrc/egr_wpe.hip) instead of nara_wpe's numpy on the host.

Registered only when the environment variable EGREGORA_ENHANCE_NODES is "1" at import (__init__.py).

Deliberate, documented differences from the reference (SPEC.md 4d):
  WPE-Q1  the reference hands nara_wpe's wpe() an array shaped (frames, bins, channels) where (bins, channels, frames) is expected,
          so its try block fails and the node returns its input.  Not reproduced: this node runs what the docstring and the
          widgets describe, per-bin multi-channel WPE over frames.
  WPE-P6  `use_float32` selects nothing: spectra are complex64, statistics and solves are double, for both values.
  WPE-P3  a framing the kernels do not support (hop not dividing n_fft, n_fft / hop < 2) and an empty input return the input
          unchanged with the reference's warning, which is what its `except` branch does for them.
  WPE-P7  channels * taps > 64 raises RuntimeError; there is no CPU fallback.
"""
import torch

from . import native, wpe_engine
from .egregora_audio_enhance_extras import _coerce_audio, _make_audio


class Egregora_WPE_Dereverb:
    """
    Weighted Prediction Error dereverberation.
    Works mono or multi-channel. Uses STFT -> WPE -> iSTFT.
    """
    @classmethod
    def INPUT_TYPES(cls):
        return {
            "required": {
                "audio": ("AUDIO",),
                "taps": ("INT", {"default": 10, "min": 3, "max": 32}),
                "delay": ("INT", {"default": 3, "min": 1, "max": 16}),
                "iterations": ("INT", {"default": 3, "min": 1, "max": 10}),
                "n_fft": ("INT", {"default": 1024, "min": 256, "max": 4096, "step": 256}),
                "hop": ("INT", {"default": 256, "min": 64, "max": 1024, "step": 64}),
                "use_float32": ("BOOLEAN", {"default": True}),
            }
        }

    RETURN_TYPES = ("AUDIO",)
    FUNCTION = "execute"
    CATEGORY = "Egregora/Enhance"

    def execute(self, audio, taps=10, delay=3, iterations=3, n_fft=1024, hop=256, use_float32=True):
        wav, sr, meta = _coerce_audio(audio)  # [B,C,T]
        B, C, T = wav.shape
        taps, delay, iterations, n_fft, hop = int(taps), int(delay), int(iterations), int(n_fft), int(hop)
        wpe_engine.check_limits(C, taps, n_fft)
        if T == 0 or not wpe_engine.framing_supported(n_fft, hop):
            why = "empty input" if T == 0 else f"hop {hop} does not divide n_fft {n_fft} at least twice"
            print(f"Warning: WPE processing failed: {why}")
            out = wav
        else:
            native.require_device()
            dev = wav.device if wav.is_cuda else torch.device("cuda", torch.cuda.current_device())
            out = torch.stack([wpe_engine.dereverb(wav[b].to(dev), n_fft, hop, taps, delay, iterations) for b in range(B)]).to(wav.device)
        meta2 = dict(meta)
        meta2["wpe"] = {"taps": taps, "delay": delay, "iterations": iterations, "n_fft": n_fft, "hop": hop}
        return (_make_audio(sr, out, meta2),)


NODE_CLASS_MAPPINGS = {"Egregora_WPE_Dereverb": Egregora_WPE_Dereverb}
NODE_DISPLAY_NAME_MAPPINGS = {"Egregora_WPE_Dereverb": "Egregora WPE Dereverb"}
