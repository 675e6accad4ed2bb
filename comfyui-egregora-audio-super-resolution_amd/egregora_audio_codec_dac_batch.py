"""ComfyUI nodes "Egregora DAC Encode (batch)" / "Egregora DAC Decode (batch)": a LIST of AUDIO values (or of codes DICTs) through
the codec in one padded pass per wave (dac_many).

Opt-in (registered when EGREGORA_CODEC_BATCH_NODES is "1" at import, __init__.py); the reference pack has no such nodes.  Same widgets
as the single nodes (egregora_audio_codec_dac.py).  Every list element is coerced like the single node's input; an AUDIO whose waveform
is [B,C,T] counts as B clips.  Each output DICT / AUDIO is shaped exactly like the single node's for that list element; its values
equal the single node's to fp32 round-off.
"""
import torch

from . import dac_many
from .egregora_audio_codec_dac import Egregora_DAC_Decode, Egregora_DAC_Encode
from .egregora_audio_enhance_extras import _coerce_audio, _make_audio
from .egregora_audio_super_resolution_batch import _first


def _as_list(v, is_one):
    return [v] if v is None or is_one(v) or not isinstance(v, (list, tuple)) else list(v)


class Egregora_DAC_EncodeBatch:
    INPUT_TYPES = Egregora_DAC_Encode.INPUT_TYPES
    INPUT_IS_LIST = True
    OUTPUT_IS_LIST = (True, True)
    RETURN_TYPES = Egregora_DAC_Encode.RETURN_TYPES
    RETURN_NAMES = Egregora_DAC_Encode.RETURN_NAMES
    FUNCTION = Egregora_DAC_Encode.FUNCTION
    CATEGORY = Egregora_DAC_Encode.CATEGORY

    def execute(self, audio=None, model_type="44khz", device="auto"):
        from .audio_glue import is_audio_dict
        model_type = _first(model_type, "44khz")
        elems = [_coerce_audio(a) for a in _as_list(audio, is_audio_dict)]           # (wav [B,C,T], sr, meta)
        clips = [(wav[b], sr) for wav, sr, _ in elems for b in range(wav.shape[0])]
        res = dac_many.encode_many(clips, model_type)
        dicts, logs, k = [], [], 0
        for wav, sr, _ in elems:
            B, C, _T = wav.shape
            mine = res[k:k + B]
            k += B
            model_sr = mine[0]["model_sample_rate"] if mine else sr
            dicts.append({"model_type": model_type, "sample_rate": sr, "model_sample_rate": model_sr,
                          "latents": [[r["z"]] for r in mine], "codes": [r["codes"] for r in mine]})
            logs.append(f"DAC encode ok: model={model_type}, B={B}, C={C}, sr={sr}->{model_sr}")
        return (dicts, logs)


class Egregora_DAC_DecodeBatch:
    INPUT_TYPES = Egregora_DAC_Decode.INPUT_TYPES
    INPUT_IS_LIST = True
    OUTPUT_IS_LIST = (True, True)
    RETURN_TYPES = Egregora_DAC_Decode.RETURN_TYPES
    RETURN_NAMES = Egregora_DAC_Decode.RETURN_NAMES
    FUNCTION = Egregora_DAC_Decode.FUNCTION
    CATEGORY = Egregora_DAC_Decode.CATEGORY

    def execute(self, codes=None, device="auto"):
        dicts = _as_list(codes, lambda v: isinstance(v, dict))
        per_model, shape = {}, []
        for d in dicts:
            model_type = d.get("model_type", "44khz")
            sr = int(d.get("sample_rate", 48000))
            latents_b = d.get("latents", [])
            codes_b = [] if latents_b else d.get("codes", [])
            if not latents_b and not codes_b:
                raise ValueError("codes.latents empty")
            items = []
            for z_list in latents_b or codes_b:
                t = z_list[0] if isinstance(z_list, (list, tuple)) else z_list
                t = t.unsqueeze(0) if t.dim() == 2 else t
                items.append({"z": t.float(), "sample_rate": sr} if latents_b else {"codes": t, "sample_rate": sr})
            bucket = per_model.setdefault(model_type, [])
            shape.append((model_type, sr, int(d.get("model_sample_rate", sr)), len(bucket), len(items)))
            bucket += items
        ys = {m: dac_many.decode_many(items, m) for m, items in per_model.items()}
        audios, logs = [], []
        for model_type, sr, model_sr, at, n in shape:
            y_cat = torch.cat([y.unsqueeze(0) for y in ys[model_type][at:at + n]], dim=0)       # [B,C,T]
            audios.append(_make_audio(sr=sr, wav=y_cat))
            logs.append(f"DAC decode ok: model={model_type}, B={y_cat.size(0)}, C={y_cat.size(1)}, {model_sr}->{sr}")
        return (audios, logs)


NODE_CLASS_MAPPINGS = {"Egregora_DAC_EncodeBatch": Egregora_DAC_EncodeBatch, "Egregora_DAC_DecodeBatch": Egregora_DAC_DecodeBatch}
NODE_DISPLAY_NAME_MAPPINGS = {"Egregora_DAC_EncodeBatch": "Egregora DAC Encode (batch)", "Egregora_DAC_DecodeBatch": "Egregora DAC Decode (batch)"}
