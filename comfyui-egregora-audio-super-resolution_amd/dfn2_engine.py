"""Native DeepFilterNet2 backend of `Egregora DeepFilterNet Denoise` (egr_dfn2_* in libegregora_amd.so, csrc/egr_dfn3.hip): the
engine of dfn_engine.py on a DeepFilterNet2 model directory (dfn2_weights.load)."""
import ctypes as C
from pathlib import Path
from typing import Optional

from . import dfn2_weights, dfn_engine, native


def config_c(m: "dfn2_weights.DFN2Model") -> native.Dfn2ConfigC:
    c = m.cfg
    s = native.Dfn2ConfigC()
    s.struct_bytes = C.sizeof(native.Dfn2ConfigC)
    for f in ("sr", "fft_size", "hop_size", "nb_erb", "nb_df", "df_order", "df_lookahead", "conv_lookahead", "emb_hidden_dim",
              "emb_num_layers", "df_hidden_dim", "df_num_layers", "gru_groups", "lin_groups", "conv_ch"):
        setattr(s, f, int(c[f]))
    s.group_shuffle = int(bool(c["group_shuffle"]))
    s.df_output_layer = 1 if c["df_output_layer"] == "linear" else 0
    dfn_engine.config_common(s, m)
    return s


class Dfn2Engine(dfn_engine.DfnEngine):
    """stage(): "gru0" and "sum0" take the GroupedGRU layer index."""
    prefix, stages, indexed, weights = "egr_dfn2", native.DFN2_STAGE, ("gru0", "sum0"), dfn2_weights
    config_c = staticmethod(config_c)


def engine(model_dir: Optional[Path] = None, device: Optional[int] = None) -> Dfn2Engine:
    """The cached engine of (model directory, device); discovery when model_dir is None."""
    return dfn_engine.cached(Dfn2Engine, model_dir, device)
