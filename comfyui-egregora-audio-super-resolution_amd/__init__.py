"""ComfyUI custom-node pack: MI355X-native (gfx950) backend for Egregora Audio Super Resolution.

Drop-in for the reference pack's three core nodes (reference __init__.py:33-43): same mapping keys, same
display names, same INPUT_TYPES / RETURN_TYPES / FUNCTION surface -- plus the evaluation-pack nodes and the DeepFilterNet
stage that run on this pack's kernels (merged the way the reference merges its ENHANCE_MAP / EVAL_MAP, __init__.py:9-23,47-53).  Compute runs in libegregora_amd.so
(hand-written HIP, C ABI in include/egregora_amd.h); importing this package needs neither the library
nor a GPU -- the nodes raise at run() time when either is missing.

The evaluation pack's loudness meter, 1770 gain match and ABX nodes (egregora_audio_eval_loudness.py) are registered only when the
environment variable EGREGORA_EVAL_NODES is "1" at import; the WPE dereverberation node (egregora_audio_enhance_wpe.py) only when
EGREGORA_ENHANCE_NODES is "1", the Descript Audio Codec encode / decode nodes (egregora_audio_codec_dac.py) only when
EGREGORA_CODEC_NODES is "1", the FlashSR batch node (egregora_audio_super_resolution_batch.py: a list of clips in packed waves) only
when EGREGORA_BATCH_NODES is "1", the DeepFilterNet batch node (egregora_audio_enhance_dfn_batch.py: a list of clips in ragged passes)
only when EGREGORA_DENOISE_BATCH_NODES is "1", the codec's batch nodes (egregora_audio_codec_dac_batch.py: a list of clips in padded
passes) only when EGREGORA_CODEC_BATCH_NODES is "1", the Fat-Llama batch node (egregora_fat_llama_gpu_batch.py: a list of clips in
waves that share one chirp-z convolution length) only when EGREGORA_FATLLAMA_BATCH_NODES is "1", the WPE batch node
(egregora_audio_enhance_wpe_batch.py: a list of clips in one ragged pass per wave) only when EGREGORA_ENHANCE_BATCH_NODES is "1", the
evaluation batch nodes (egregora_audio_eval_batch.py: lists of clips scored and metered in one ragged pass per wave) only when
EGREGORA_EVAL_BATCH_NODES is "1", the null-test batch nodes (egregora_null_test_batch.py: lists of pairs aligned, gain-matched and nulled
in ragged passes per wave) only when EGREGORA_NULLTEST_BATCH_NODES is "1", the resampler's batch node
(egregora_audio_resample_batch.py: a list of clips with one library call per source rate) only when EGREGORA_RESAMPLE_BATCH_NODES is "1".
Without them the registered set is the one listed above.
"""
import os

from .egregora_audio_super_resolution import EgregoraAudioSuperResolution
from .egregora_fat_llama_cpu import EgregoraFatLlamaCPU
from .egregora_fat_llama_gpu import EgregoraFatLlamaGPU
from .egregora_audio_eval_pack import (NODE_CLASS_MAPPINGS as EVAL_MAP, NODE_DISPLAY_NAME_MAPPINGS as EVAL_NAMES)
from .egregora_audio_enhance_extras import (NODE_CLASS_MAPPINGS as ENHANCE_MAP, NODE_DISPLAY_NAME_MAPPINGS as ENHANCE_NAMES)
from .egregora_null_test_suite import (NODE_CLASS_MAPPINGS as NULL_MAP, NODE_DISPLAY_NAME_MAPPINGS as NULL_NAMES)

NODE_CLASS_MAPPINGS = {
    "EgregoraAudioUpscaler": EgregoraAudioSuperResolution,
    "EgregoraFatLlamaGPU": EgregoraFatLlamaGPU,
    "EgregoraFatLlamaCPU": EgregoraFatLlamaCPU,
}

NODE_DISPLAY_NAME_MAPPINGS = {
    "EgregoraAudioUpscaler": "🎧 Audio Super Resolution (FlashSR)",
    "EgregoraFatLlamaGPU": "🎛️ Spectral Enhance (Fat Llama — GPU)",
    "EgregoraFatLlamaCPU": "🎛️ Spectral Enhance (Fat Llama — CPU/FFTW)",
}

NODE_CLASS_MAPPINGS.update(ENHANCE_MAP)
NODE_CLASS_MAPPINGS.update(EVAL_MAP)
NODE_CLASS_MAPPINGS.update(NULL_MAP)
NODE_DISPLAY_NAME_MAPPINGS.update(ENHANCE_NAMES)
NODE_DISPLAY_NAME_MAPPINGS.update(EVAL_NAMES)
NODE_DISPLAY_NAME_MAPPINGS.update(NULL_NAMES)

if os.environ.get("EGREGORA_EVAL_NODES") == "1":
    from .egregora_audio_eval_loudness import (NODE_CLASS_MAPPINGS as LOUD_MAP, NODE_DISPLAY_NAME_MAPPINGS as LOUD_NAMES)
    NODE_CLASS_MAPPINGS.update(LOUD_MAP)
    NODE_DISPLAY_NAME_MAPPINGS.update(LOUD_NAMES)

if os.environ.get("EGREGORA_ENHANCE_NODES") == "1":
    from .egregora_audio_enhance_wpe import (NODE_CLASS_MAPPINGS as WPE_MAP, NODE_DISPLAY_NAME_MAPPINGS as WPE_NAMES)
    NODE_CLASS_MAPPINGS.update(WPE_MAP)
    NODE_DISPLAY_NAME_MAPPINGS.update(WPE_NAMES)

if os.environ.get("EGREGORA_CODEC_NODES") == "1":
    from .egregora_audio_codec_dac import (NODE_CLASS_MAPPINGS as DAC_MAP, NODE_DISPLAY_NAME_MAPPINGS as DAC_NAMES)
    NODE_CLASS_MAPPINGS.update(DAC_MAP)
    NODE_DISPLAY_NAME_MAPPINGS.update(DAC_NAMES)

if os.environ.get("EGREGORA_BATCH_NODES") == "1":
    from .egregora_audio_super_resolution_batch import (NODE_CLASS_MAPPINGS as BATCH_MAP, NODE_DISPLAY_NAME_MAPPINGS as BATCH_NAMES)
    NODE_CLASS_MAPPINGS.update(BATCH_MAP)
    NODE_DISPLAY_NAME_MAPPINGS.update(BATCH_NAMES)

if os.environ.get("EGREGORA_DENOISE_BATCH_NODES") == "1":
    from .egregora_audio_enhance_dfn_batch import (NODE_CLASS_MAPPINGS as DFN_BATCH_MAP, NODE_DISPLAY_NAME_MAPPINGS as DFN_BATCH_NAMES)
    NODE_CLASS_MAPPINGS.update(DFN_BATCH_MAP)
    NODE_DISPLAY_NAME_MAPPINGS.update(DFN_BATCH_NAMES)

if os.environ.get("EGREGORA_CODEC_BATCH_NODES") == "1":
    from .egregora_audio_codec_dac_batch import (NODE_CLASS_MAPPINGS as DAC_BATCH_MAP, NODE_DISPLAY_NAME_MAPPINGS as DAC_BATCH_NAMES)
    NODE_CLASS_MAPPINGS.update(DAC_BATCH_MAP)
    NODE_DISPLAY_NAME_MAPPINGS.update(DAC_BATCH_NAMES)

if os.environ.get("EGREGORA_FATLLAMA_BATCH_NODES") == "1":
    from .egregora_fat_llama_gpu_batch import (NODE_CLASS_MAPPINGS as FL_BATCH_MAP, NODE_DISPLAY_NAME_MAPPINGS as FL_BATCH_NAMES)
    NODE_CLASS_MAPPINGS.update(FL_BATCH_MAP)
    NODE_DISPLAY_NAME_MAPPINGS.update(FL_BATCH_NAMES)

if os.environ.get("EGREGORA_ENHANCE_BATCH_NODES") == "1":
    from .egregora_audio_enhance_wpe_batch import (NODE_CLASS_MAPPINGS as WPE_BATCH_MAP, NODE_DISPLAY_NAME_MAPPINGS as WPE_BATCH_NAMES)
    NODE_CLASS_MAPPINGS.update(WPE_BATCH_MAP)
    NODE_DISPLAY_NAME_MAPPINGS.update(WPE_BATCH_NAMES)

if os.environ.get("EGREGORA_EVAL_BATCH_NODES") == "1":
    from .egregora_audio_eval_batch import (NODE_CLASS_MAPPINGS as EVAL_BATCH_MAP, NODE_DISPLAY_NAME_MAPPINGS as EVAL_BATCH_NAMES)
    NODE_CLASS_MAPPINGS.update(EVAL_BATCH_MAP)
    NODE_DISPLAY_NAME_MAPPINGS.update(EVAL_BATCH_NAMES)

if os.environ.get("EGREGORA_NULLTEST_BATCH_NODES") == "1":
    from .egregora_null_test_batch import (NODE_CLASS_MAPPINGS as NULL_BATCH_MAP, NODE_DISPLAY_NAME_MAPPINGS as NULL_BATCH_NAMES)
    NODE_CLASS_MAPPINGS.update(NULL_BATCH_MAP)
    NODE_DISPLAY_NAME_MAPPINGS.update(NULL_BATCH_NAMES)

if os.environ.get("EGREGORA_RESAMPLE_BATCH_NODES") == "1":
    from .egregora_audio_resample_batch import (NODE_CLASS_MAPPINGS as RS_BATCH_MAP, NODE_DISPLAY_NAME_MAPPINGS as RS_BATCH_NAMES)
    NODE_CLASS_MAPPINGS.update(RS_BATCH_MAP)
    NODE_DISPLAY_NAME_MAPPINGS.update(RS_BATCH_NAMES)

__all__ = ["NODE_CLASS_MAPPINGS", "NODE_DISPLAY_NAME_MAPPINGS"]
