#!/usr/bin/env python3
"""Golden fixture G16: the plugin surface of the reference's `Egregora WPE Dereverb` node (egregora_audio_enhance_extras.py:368-443)
and the `meta` it writes, captured by importing the reference's module.  Data only: widget dicts, their order, return types, the
signature, and the outcome of two calls made while `nara_wpe` is absent from the machine:

  * the call as it stands raises the reference's RuntimeError("nara-wpe not installed ...") (recorded as `absent_error`);
  * with an empty stand-in `nara_wpe` whose stft() raises, the reference takes its own `except` branch -- the same branch its real
    run ends in (SPEC.md WPE-Q1) -- returns the input and writes meta["wpe"]: the meta keys, the "wpe" entry, shape and sample rate
    of that call are recorded as `passthrough`.

`torchaudio` is imported at the reference module's top but not used on this path: an empty stub satisfies the import, as in the
G11 generator.

  python tests/golden/make_golden_wpe.py REFERENCE_DIR      # writes tests/golden/g16_wpe_surface.json
"""
import importlib.util
import inspect
import json
import sys
import types
from pathlib import Path

import numpy as np
import torch

OUT = Path(__file__).resolve().parent
KEY = "Egregora_WPE_Dereverb"


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
    cls = mod.NODE_CLASS_MAPPINGS[KEY]
    g = {"surface": {KEY: surf(cls, mod.NODE_DISPLAY_NAME_MAPPINGS[KEY])}}

    rng = np.random.Generator(np.random.PCG64(16))
    x = (0.1 * rng.standard_normal((2, 2, 4000))).astype(np.float32)
    A = {"waveform": torch.from_numpy(x), "sample_rate": 16000, "meta": {"k": 1}}
    kw = dict(taps=5, delay=2, iterations=2, n_fft=512, hop=128, use_float32=True)
    assert "nara_wpe" not in sys.modules
    try:
        cls().execute(A, **kw)
        raise SystemExit("nara_wpe is installed here: this fixture records the call without it")
    except RuntimeError as e:
        g["absent_error"] = str(e)

    def _absent(*a, **k):
        raise ImportError("nara_wpe is absent")
    nw, nwu = types.ModuleType("nara_wpe"), types.ModuleType("nara_wpe.utils")
    nw.wpe, nw.utils = types.SimpleNamespace(wpe=_absent), nwu
    nwu.stft = nwu.istft = _absent
    sys.modules.update({"nara_wpe": nw, "nara_wpe.utils": nwu})
    (out,) = cls().execute(A, **kw)
    y = out["waveform"].numpy()
    g["passthrough"] = {"kwargs": kw, "in_shape": list(x.shape), "shape": list(y.shape), "sr": out["sample_rate"],
                        "keys": sorted(out.keys()), "meta_keys": sorted(out["meta"].keys()), "wpe_meta": out["meta"]["wpe"],
                        "equals_input": bool(np.array_equal(y, x)), "dtype": str(out["waveform"].dtype)}
    (OUT / "g16_wpe_surface.json").write_text(json.dumps(g, indent=1, sort_keys=True, ensure_ascii=False) + "\n", encoding="utf-8")
    print("wrote g16_wpe_surface.json:", g["absent_error"], g["passthrough"]["meta_keys"])


if __name__ == "__main__":
    main()
