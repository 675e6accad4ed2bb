#!/usr/bin/env python3
"""Golden fixture G17: the plugin surface of the reference's `Egregora DAC Encode` / `Egregora DAC Decode` nodes
(egregora_audio_enhance_extras.py:730-857), captured by importing the reference's module.  Data only: widget dicts, their order, return
types and names, the signatures, the display names, and the text of the RuntimeError both nodes raise while `descript-audio-codec` is
absent from the machine (recorded as `absent_error`), plus the ValueError text of a decode call with empty latents made with an empty
stand-in `dac` module (`empty_error`).

`torchaudio` is imported at the reference module's top but not used on these paths: an empty stub satisfies the import, as in the
G16 generator.

  python tests/golden/make_golden_dac.py REFERENCE_DIR      # writes tests/golden/g17_dac_surface.json
"""
import importlib.util
import inspect
import json
import sys
import types
from pathlib import Path

import torch

OUT = Path(__file__).resolve().parent
KEYS = ("Egregora_DAC_Encode", "Egregora_DAC_Decode")


def surf(cls, display):
    it = cls.INPUT_TYPES()
    return {"INPUT_TYPES": it, "widget_order": {k: list(v.keys()) for k, v in it.items()}, "RETURN_TYPES": list(cls.RETURN_TYPES),
            "RETURN_NAMES": list(getattr(cls, "RETURN_NAMES", ())), "FUNCTION": cls.FUNCTION, "CATEGORY": cls.CATEGORY,
            "signature": str(inspect.signature(getattr(cls, cls.FUNCTION))), "display": display, "class_name": cls.__name__}


def main():
    ref = Path(sys.argv[1])
    sys.modules.setdefault("torchaudio", types.ModuleType("torchaudio"))
    spec = importlib.util.spec_from_file_location("ref_extras", ref / "egregora_audio_enhance_extras.py")
    mod = importlib.util.module_from_spec(spec)
    sys.modules["ref_extras"] = mod
    spec.loader.exec_module(mod)
    g = {"surface": {k: surf(mod.NODE_CLASS_MAPPINGS[k], mod.NODE_DISPLAY_NAME_MAPPINGS[k]) for k in KEYS}, "absent_error": {}}
    assert "dac" not in sys.modules
    A = {"waveform": torch.zeros(1, 1, 1000), "sample_rate": 44100}
    calls = {KEYS[0]: lambda c: c().execute(A), KEYS[1]: lambda c: c().execute({"latents": [[torch.zeros(1, 4, 4)]]})}
    for k in KEYS:
        try:
            calls[k](mod.NODE_CLASS_MAPPINGS[k])
            raise SystemExit("descript-audio-codec is installed here: this fixture records the calls without it")
        except RuntimeError as e:
            g["absent_error"][k] = str(e)
    sys.modules["dac"] = types.ModuleType("dac")
    try:
        mod.NODE_CLASS_MAPPINGS[KEYS[1]]().execute({"model_type": "44khz", "latents": []})
        raise SystemExit("decode of empty latents did not raise")
    except ValueError as e:
        g["empty_error"] = str(e)
    (OUT / "g17_dac_surface.json").write_text(json.dumps(g, indent=1, sort_keys=True, ensure_ascii=False) + "\n", encoding="utf-8")
    print("wrote g17_dac_surface.json:", g["absent_error"], g["empty_error"])


if __name__ == "__main__":
    main()
