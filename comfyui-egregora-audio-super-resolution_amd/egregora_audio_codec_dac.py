"""`Egregora_DAC_Encode` / `Egregora_DAC_Decode` with the reference's plugin surface (egregora_audio_enhance_extras.py:730-857, fixture
G17), computed by this pack's own kernels (dac_engine.py, csrc/egr_dac.hip) instead of the `dac` package.

Registered only when the environment variable EGREGORA_CODEC_NODES is "1" at import (__init__.py).

Deliberate, documented differences from the reference (SPEC.md 4e):
  DAC-Q1  the reference hands `model.encode` a 2-D [C, T] tensor and `model.decode` a Python list, which upstream rejects.  Not
          reproduced: the C channels of a batch element are C mono rows, as upstream's own `compress` treats channels.
  DAC-Q2  rate conversion uses this pack's polyphase kernel (resample.resample_hq), not torchaudio.  With EGREGORA_SINC_RESAMPLE=1
          (read at call time) it uses the windowed-sinc kernel at torchaudio's defaults, as the reference does (resample.codec_resample).
  The checkpoint is never downloaded (dac_weights.discover); `device` is accepted and ignored, there is no CPU path.
  The DICT also carries `codes`: a list over the batch of int64 [C, n_codebooks, frames]; Decode takes a DICT whose `latents` is
  missing or empty from them (dac_engine.from_codes).  Inputs above the workspace budget run in segments (dac_engine.choose_path).
"""
import torch

from . import dac_engine, dac_weights, native, resample
from .egregora_audio_enhance_extras import _coerce_audio, _make_audio


def _engine(model_type: str):
    path = dac_weights.discover(model_type)
    if path is None:
        raise RuntimeError(dac_weights.not_found_message(model_type))
    native.require_device()
    return dac_engine.engine(path)


class Egregora_DAC_Encode:
    """
    Encodes audio with DAC and returns latent 'z' & metadata in a DICT.
    """
    @classmethod
    def INPUT_TYPES(cls):
        return {
            "required": {
                "audio": ("AUDIO",),
                "model_type": (["44khz", "24khz", "16khz"], {"default": "44khz"}),
                "device": (["auto", "cpu", "cuda"], {"default": "auto"}),
            }
        }

    RETURN_TYPES = ("DICT", "STRING")
    RETURN_NAMES = ("codes", "log")
    FUNCTION = "execute"
    CATEGORY = "Egregora/Codecs"

    def execute(self, audio, model_type="44khz", device="auto"):
        wav, sr, meta = _coerce_audio(audio)  # [B,C,T] float
        B, C, T = wav.shape
        eng = _engine(model_type)
        model_sr = int(eng.cfg["sample_rate"])
        dev = torch.device("cuda", eng.device)
        z_all, codes_all = [], []
        for b in range(B):
            x = wav[b].to(dev)  # [C,T]: C mono rows (DAC-Q1)
            if sr != model_sr:
                x = resample.codec_resample(x, sr, model_sr)
            z, codes = eng.encode(x)
            z_all.append([z.cpu()])
            codes_all.append(codes.to(torch.int64).cpu())
        codes_dict = {
            "model_type": model_type,
            "sample_rate": sr,
            "model_sample_rate": model_sr,
            "latents": z_all,  # list over batch of [z], z float32 [C, latent, frames]
            "codes": codes_all,  # list over batch of int64 [C, n_codebooks, frames]
        }
        log = f"DAC encode ok: model={model_type}, B={B}, C={C}, sr={sr}->{model_sr}"
        return (codes_dict, log)


class Egregora_DAC_Decode:
    """
    Decodes DICT produced by Egregora_DAC_Encode back to AUDIO.
    """
    @classmethod
    def INPUT_TYPES(cls):
        return {
            "required": {
                "codes": ("DICT",),
                "device": (["auto", "cpu", "cuda"], {"default": "auto"}),
            }
        }

    RETURN_TYPES = ("AUDIO", "STRING")
    RETURN_NAMES = ("audio", "log")
    FUNCTION = "execute"
    CATEGORY = "Egregora/Codecs"

    def execute(self, codes, device="auto"):
        model_type = codes.get("model_type", "44khz")
        sr = int(codes.get("sample_rate", 48000))
        model_sr = int(codes.get("model_sample_rate", sr))
        latents_b = codes.get("latents", [])
        codes_b = [] if latents_b else codes.get("codes", [])
        if not latents_b and not codes_b:
            raise ValueError("codes.latents empty")
        eng = _engine(model_type)
        dev = torch.device("cuda", eng.device)
        outs = []
        for z_list in latents_b or codes_b:
            z = z_list[0] if isinstance(z_list, (list, tuple)) else z_list
            if latents_b:
                z = z.to(dev).float()
            else:  # no latents: z from the integer codes [C, n_codebooks, frames], as upstream's decompress does
                c = z.to(dev)
                z = eng.from_codes(c.unsqueeze(0) if c.dim() == 2 else c)
            if z.dim() == 2:  # [latent, frames]: one row
                z = z.unsqueeze(0)
            y = eng.decode(z)  # [C,T] at the model's rate
            if model_sr != sr:
                y = resample.codec_resample(y, model_sr, sr)
            outs.append(y.unsqueeze(0).cpu())
        y_cat = torch.cat(outs, dim=0)  # [B,C,T]
        audio = _make_audio(sr=sr, wav=y_cat)
        log = f"DAC decode ok: model={model_type}, B={y_cat.size(0)}, C={y_cat.size(1)}, {model_sr}->{sr}"
        return (audio, log)


NODE_CLASS_MAPPINGS = {"Egregora_DAC_Encode": Egregora_DAC_Encode, "Egregora_DAC_Decode": Egregora_DAC_Decode}
NODE_DISPLAY_NAME_MAPPINGS = {"Egregora_DAC_Encode": "Egregora DAC Encode", "Egregora_DAC_Decode": "Egregora DAC Decode"}
