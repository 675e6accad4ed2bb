"""FlashSR on the MI355X.  Stands in for the reference's `_FlashSRRunner` (egregora_audio_super_resolution.py:254-369): built
once per process (the reference rebuilds per call, :393), inference on [rows, 245760] where rows = chunks x channels ride the
batch dimension (:366-368).

The model is the C-ABI handle -- `egr_flashsr_create` / `egr_flashsr_infer` (include/egregora_amd.h, csrc/egr_flashsr.cpp): the
graph walk, weight repacking and scratch arena live in the library; this module only hands it the named weight tensors
(`FlashSREngine.handle`, `infer_rows`) and shards chunk blocks -- over the ranks of a torch.distributed process group when one
exists (shard.py: one process per GPU, one all-gather), or, inside ONE process (what a ComfyUI host is), over the devices listed
in EGREGORA_DEVICES: one handle and one host thread per device, contiguous chunk blocks balanced to within one chunk, the gather
as peer copies into device 0's prediction tensor, WOLA on device 0 (`infer_spans_devices`).  A pass of >= 12 rows is split by the library into up
to EGREGORA_FLASHSR_STREAMS (default 2) row groups that run as concurrent forwards on side streams the handle has verified to
sit on other hardware queues; the caller sees one stream.

(The operator-by-operator Python walk of the same graph that the tests use for per-stage taps and ablations is NOT part of the
product: tools/flashsr_pydriver.py, a subclass of this engine, held bit-for-bit equal to the handle by
tests/test_gpu_flashsr_capi.py.)

Activations are channels-last ([B][H][W][C] / [B][L][C]) float32.
PARITY UNPINNED vs upstream (see flashsr_arch.py); checked against oracle/flashsr_torch.py (same table, torch fp32 / fp64).
"""
import ctypes as C
import math
import os
import threading
from typing import Dict, List, Optional, Tuple

import torch

from . import audio_glue, device_ops, flashsr_arch as arch, native, resample, shard
from .many_common import group_by_rate, track_rows

ACT_NONE, ACT_SILU, ACT_TANH, ACT_LEAKY, ACT_LOGCLAMP = 0, 1, 2, 3, 4
EW_ADD, EW_AXPBY, EW_SILU, EW_SCALE, EW_COPY, EW_ADD_SCALE = 0, 1, 2, 3, 4, 5


def _p(t: Optional[torch.Tensor]):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


class FlashSREngine:
    # Switches of the handle (frozen per engine at construction; egr_flashsr_create flags, include/egregora_amd.h):
    # dense contractions run on the bf16 matrix pipe with fp32-grade results ("bf16x3": exact three-way split of both
    # operands, six partial products accumulated in fp32, csrc/egr_nn_gemm_s3.hip) or on v_mfma_f32_32x32x2_f32 ("f32").
    MFMA_MODE = os.environ.get("EGREGORA_FLASHSR_MFMA", "bf16x3")
    # operand scheme of egr_flashsr_infer's split contractions: "f16x2" = two fp16 terms, one power-of-two scale per (tensor, batch
    # row) derived on the device from that row's own maximum (include/egregora_amd.h egr_flashsr_set_split), "bf16x3" = always
    # three bf16 terms.  egr_flashsr_forward / the operator API use the bf16 terms.  "f16x1" = the opt-in fast mode: ONE fp16 term
    # per operand where "f16x2" runs two (EGR_FSR_FAST_F16): reduced precision, outside the pack's accuracy statement (SPEC.md).
    SPLIT = os.environ.get("EGREGORA_FLASHSR_SPLIT", "f16x2")
    # F(2x2,3x3) paid from 256 channels (its transforms move 4x the tensor); F(4x4,3x3) moves 2.25x and pays from 128
    WINO_MIN_CH = int(os.environ.get("EGREGORA_FLASHSR_WINOGRAD_MIN_CH", "128"))
    WINO_F4 = os.environ.get("EGREGORA_FLASHSR_WINOGRAD_F4", "1") != "0"   # F(4x4,3x3) where H and W are multiples of 4
    GN_PARTIALS = os.environ.get("EGREGORA_FLASHSR_GN_PARTIALS", "1") != "0"
    THIN_ENDS = os.environ.get("EGREGORA_FLASHSR_THIN_ENDS", "1") != "0"     # dedicated paths for Cout*kh*kw <= 32 and Cin == 1 convs
    FUSE_GN = os.environ.get("EGREGORA_FLASHSR_FUSE_GN", "1")      # "0" off, "1" Winograd consumers only, "all"
    _KEEP_PARAMS = False        # the test driver (tools/flashsr_pydriver.py) keeps the state dict for its own lazy packs

    def __init__(self, cfg: arch.FlashSRConfig, params: Dict[str, torch.Tensor], device="cuda"):
        native.require_device()
        self.cfg = cfg
        self.dev = torch.device(device)
        if self.dev.index is None:               # pinned to the device that is current now: the handle's memory lives there
            self.dev = torch.device("cuda", torch.cuda.current_device())
        self.L = native.lib()
        # the class-level switches are frozen per engine at construction: the handle flags must see the values this engine was
        # built under, whatever the class holds later
        for name in dir(type(self)):
            if name.isupper() and not name.startswith("_"):
                setattr(self, name, getattr(type(self), name))
        self.mfma = self.MFMA_MODE
        self.thin = self.THIN_ENDS
        self._handle = None
        self._params = {k: v.detach().float().contiguous() for k, v in params.items()}     # torch layouts (host)
        self.window = torch.hann_window(cfg.n_fft, periodic=True, dtype=torch.float32).to(self.dev)
        self.filt = torch.from_numpy(arch.kaiser_sinc_filter(cfg.aa_taps)).to(self.dev)
        self.mel_fb = torch.from_numpy(arch.mel_filterbank(cfg)).contiguous().to(self.dev)       # [n_mels][nb]

    def _st(self):
        return native.stream_ptr()

    # ------------------------------------------------------------------ the C-ABI model handle (product path)
    def time_embedding_input(self) -> torch.Tensor:
        """Sinusoidal embedding of the fixed step t = T-1, [1, unet_ch] float32 (the input of unet.time_embed)."""
        half = self.cfg.unet_ch // 2
        freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32) / half)
        args = float(self.cfg.t_steps - 1) * freqs
        return torch.cat([torch.cos(args), torch.sin(args)])[None].contiguous().to(self.dev)

    def named_tensors(self) -> Dict[str, torch.Tensor]:
        """What egr_flashsr_create takes: the layer table's parameters in torch layouts + the four derived constants."""
        if self._params is None:
            raise RuntimeError("the engine's state dict was released after the handle was built")
        t = {k: v.to(self.dev) for k, v in self._params.items()}
        t["const.window"] = self.window
        t["const.mel_fb"] = self.mel_fb
        t["const.aa_filter"] = self.filt
        t["const.time_emb"] = self.time_embedding_input()
        return t

    def handle_flags(self) -> int:
        f = native.FSR_F32_MFMA if getattr(self, "mfma", self.MFMA_MODE) != "bf16x3" else 0
        f |= native.FSR_NO_WINOGRAD if self.WINO_MIN_CH >= (1 << 20) else 0
        f |= 0 if self.WINO_F4 else native.FSR_NO_WINO_F4
        f |= 0 if self.GN_PARTIALS else native.FSR_NO_GN_PARTIALS
        f |= 0 if getattr(self, "thin", self.THIN_ENDS) else native.FSR_NO_THIN_ENDS
        f |= native.FSR_NO_FUSE_GN if self.FUSE_GN == "0" else 0
        f |= native.FSR_SPLIT_BF16X3 if self.SPLIT == "bf16x3" else 0
        f |= native.FSR_FAST_F16 if self.SPLIT == "f16x1" else 0
        return f

    @property
    def handle(self) -> int:
        """egr_flashsr handle built from this engine's parameters (once)."""
        if self._handle is None:
            with torch.cuda.device(self.dev):      # egr_flashsr_create allocates on the CURRENT device
                named = self.named_tensors()
                descs = (native.TensorDescC * len(named))()
                keep = []
                for d, (k, v) in zip(descs, named.items()):
                    v = v.contiguous()
                    keep.append(v)
                    d.name, d.data, d.ndim = k.encode(), v.data_ptr(), v.dim()
                    for i, n in enumerate(v.shape):
                        d.shape[i] = n
                cc = native.flashsr_config_c(self.cfg)
                out = C.c_void_p()
                native.check(self.L.egr_flashsr_create(C.byref(out), C.byref(cc), descs, len(named), self.handle_flags(), self._st()),
                             "egr_flashsr_create")
                self._handle = out.value
                if not self._KEEP_PARAMS:
                    self._params = None          # the library holds its own packed copy: drop the host-side state dict
                native.check(self.L.egr_flashsr_set_rows_per_pass(C.c_void_p(self._handle), ROWS_PER_PASS), "egr_flashsr_set_rows_per_pass")
        return self._handle

    def close(self):
        if self._handle is not None:
            self.L.egr_flashsr_destroy(C.c_void_p(self._handle))
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:       # noqa: BLE001 -- interpreter shutdown
            pass

    def c_forward(self, x: torch.Tensor, noise: torch.Tensor, stages: Optional[dict] = None, lowpass: bool = False) -> torch.Tensor:
        """egr_flashsr_forward: one pass through the library's graph walk; same arguments and results as forward_rows."""
        x = x.contiguous()
        R = x.shape[0]
        cfg = self.cfg
        y = torch.empty((R, cfg.chunk), dtype=torch.float32, device=self.dev)
        ptrs = None
        if stages is not None:
            h, w = cfg.lat_hw
            bufs = dict(mel=torch.empty((R, cfg.n_frames, cfg.n_mels, 1), dtype=torch.float32, device=self.dev),
                        z_cond=torch.empty((R, h, w, cfg.z_ch), dtype=torch.float32, device=self.dev),
                        v=torch.empty((R, h, w, cfg.z_ch), dtype=torch.float32, device=self.dev),
                        z0=torch.empty((R, h, w, cfg.z_ch), dtype=torch.float32, device=self.dev),
                        mel_hat=torch.empty((R, cfg.n_frames, cfg.n_mels, 1), dtype=torch.float32, device=self.dev),
                        y=torch.empty((R, cfg.n_frames * cfg.hop), dtype=torch.float32, device=self.dev))
            ptrs = (C.c_void_p * 6)(*[bufs[k].data_ptr() for k in ("mel", "z_cond", "v", "z0", "mel_hat", "y")])
            stages.update(bufs)
        native.check(self.L.egr_flashsr_forward(C.c_void_p(self.handle), _p(x), _p(noise.contiguous()), R, 1 if lowpass else 0, _p(y), ptrs,
                                                self._st()), "egr_flashsr_forward")
        return y

    def c_infer(self, x: torch.Tensor, row_ids: Optional[torch.Tensor], seed: int, lowpass: bool = False) -> torch.Tensor:
        """egr_flashsr_infer: [R, chunk] -> [R, chunk], noise keyed by (seed, global row id), rows-per-pass handled in the library."""
        x = x.contiguous()
        y = torch.empty_like(x)
        native.check(self.L.egr_flashsr_set_rows_per_pass(C.c_void_p(self.handle), ROWS_PER_PASS), "egr_flashsr_set_rows_per_pass")
        native.check(self.L.egr_flashsr_infer(C.c_void_p(self.handle), _p(x), x.shape[0], 1 if lowpass else 0, int(seed) & (2 ** 64 - 1),
                                              _p(row_ids.contiguous()) if row_ids is not None else None, _p(y), self._st()),
                     "egr_flashsr_infer")
        return y

    def warmup(self, rows: int = 2):
        """egr_flashsr_warmup: one throw-away pass over `rows` rows of silence (default: one stereo chunk) -- the kernels' code objects
        are loaded and the scratch for that row count exists before the host's first real call.  EGREGORA_FLASHSR_WARMUP=0 skips it."""
        if os.environ.get("EGREGORA_FLASHSR_WARMUP", "1") == "0" or rows < 1:
            return
        with torch.cuda.device(self.dev):
            native.check(self.L.egr_flashsr_warmup(C.c_void_p(self.handle), int(rows), self._st()), "egr_flashsr_warmup")

    def set_split(self, scheme: str):
        """"bf16x3", "f16x2" or "f16x1" for the following c_infer calls (the latter two need an engine built with fp16 weight terms:
        SPLIT = "f16x2" or "f16x1"; one pack serves both, nothing is repacked)."""
        # "+forward": c_forward too runs the fp16 operand terms (tests)
        code = {"bf16x3": 0, "f16x2": 1, "f16x2+forward": 2, "f16x1": 3, "f16x1+forward": 4}[scheme]
        native.check(self.L.egr_flashsr_set_split(C.c_void_p(self.handle), code), "egr_flashsr_set_split")

    def set_arena_cap_gb(self, gb: float):
        """Scratch budget of the handle in GB (0: none; EGREGORA_FLASHSR_ARENA_GB sets it at creation): fewer rows per pass instead of
        an allocation failure next to the host's other models (include/egregora_amd.h egr_flashsr_set_arena_cap)."""
        native.check(self.L.egr_flashsr_set_arena_cap(C.c_void_p(self.handle), float(gb) * 1e9), "egr_flashsr_set_arena_cap")

    def split_info(self) -> dict:
        """enabled: c_infer runs two fp16 terms per operand with per-row scales derived on the device; weights: contraction weights that
        hold fp16 terms; calls: c_infer calls made on the scheme; scheme: the egr_flashsr_set_split value in force (3 / 4: the one-term
        fast mode) (include/egregora_amd.h egr_flashsr_set_split)."""
        en, nw, calls, sch = C.c_int(), C.c_int(), C.c_int64(), C.c_int()
        native.check(self.L.egr_flashsr_split_scheme(C.c_void_p(self.handle), C.byref(sch)), "egr_flashsr_split_scheme")
        native.check(self.L.egr_flashsr_split_info(C.c_void_p(self.handle), C.byref(en), C.byref(nw), C.byref(calls)), "egr_flashsr_split_info")
        return dict(enabled=bool(en.value), weights=nw.value, calls=calls.value, scheme=sch.value)

    def c_profile(self, fn, ops: bool = False) -> dict:
        """{kernel instantiation: (launches, flops, ms)} of the MFMA contraction launches the handle made while fn() ran; ops=True adds
        the graph's other operator launches under the names of their entry points (egr_flashsr_set_profiling level 2)."""
        h = C.c_void_p(self.handle)
        native.check(self.L.egr_flashsr_set_profiling(h, 2 if ops else 1), "egr_flashsr_set_profiling")
        fn()
        n = C.c_int()
        native.check(self.L.egr_flashsr_profile(h, 0, None, 0, None, None, None, C.byref(n)), "egr_flashsr_profile")
        out = {}
        for i in range(n.value):
            buf, la, fl, ms = C.create_string_buffer(128), C.c_int64(), C.c_double(), C.c_double()
            native.check(self.L.egr_flashsr_profile(h, i, buf, 128, C.byref(la), C.byref(fl), C.byref(ms), None), "egr_flashsr_profile")
            out[buf.value.decode()] = (la.value, fl.value, ms.value)
        native.check(self.L.egr_flashsr_set_profiling(h, 0), "egr_flashsr_set_profiling")
        return out

    def noise(self, rows: int, row_ids: Optional[torch.Tensor], seed: int) -> torch.Tensor:
        """The library's Philox noise [rows, h, w, z] keyed by (seed, global row id): what egr_flashsr_infer draws internally."""
        h, w = self.cfg.lat_hw
        out = torch.empty((rows, h, w, self.cfg.z_ch), dtype=torch.float32, device=self.dev)
        native.check(self.L.egr_randn(_p(out), h * w * self.cfg.z_ch, rows, int(seed) & (2 ** 64 - 1), _p(row_ids),
                                      self._st()), "egr_randn")
        return out

    def flop_count(self, rows: int = 1) -> float:
        """Dense-contraction flops of one forward over `rows` rows, counted by the library's graph walk."""
        fl = C.c_double()
        native.check(self.L.egr_flashsr_flop_count(C.c_void_p(self.handle), rows, C.byref(fl), None), "egr_flashsr_flop_count")
        return fl.value


# ---------------------------------------------------------------------------------------------------- module state
# _ENGINES: device index -> engine (one C handle per device), plus ("slot", i) -> engine for position i of EGREGORA_DEVICES when a
# device index repeats there ("0,0": two handles on one GPU -- a handle serves one host thread at a time).  Every read-modify-write
# of the two globals happens under _LOCK; worker threads never build engines (infer_spans_devices resolves them on the caller's
# thread before it starts the workers), so the checkpoints are read ONCE per process whatever the device count.
_ENGINES: Dict[object, FlashSREngine] = {}
_SOURCE: Optional[Tuple[arch.FlashSRConfig, Dict[str, torch.Tensor]]] = None    # host state dict, kept only while more devices may need a copy
_LOCK = threading.RLock()
ROWS_PER_PASS = int(os.environ.get("EGREGORA_FLASHSR_ROWS", "32"))
SEED = int(os.environ.get("EGREGORA_FLASHSR_SEED", "0"))
# rows of the throw-away pass an engine runs when it is built (FlashSREngine.warmup): one stereo chunk loads every kernel the graph
# launches at small row counts; EGREGORA_FLASHSR_WARMUP_ROWS=26 also sizes the arenas of a 60 s stereo file, 0 skips the pass
WARMUP_ROWS = int(os.environ.get("EGREGORA_FLASHSR_WARMUP_ROWS", "2"))


def devices() -> List[int]:
    """Devices the node shards its chunks over inside THIS process: EGREGORA_DEVICES = "0,1,2,..." or "all" (default: the current
    device only).  The first entry stitches (WOLA).  An index may repeat ("0,0": two handles and two host threads on one GPU --
    the single-GPU test of the multi-device path)."""
    spec = os.environ.get("EGREGORA_DEVICES", "").strip()
    if not spec:
        return [torch.cuda.current_device()]
    if spec.lower() == "all":
        return list(range(torch.cuda.device_count()))
    try:
        devs = [int(t) for t in spec.split(",") if t.strip() != ""]
    except ValueError:
        raise RuntimeError(f"EGREGORA_DEVICES={spec!r}: expected a comma-separated list of device indices or 'all'")
    n = torch.cuda.device_count()
    bad = [d for d in devs if not 0 <= d < n]
    if bad or not devs:
        raise RuntimeError(f"EGREGORA_DEVICES={spec!r}: device(s) {bad} not among the {n} visible")
    return devs


def _load_source():
    from . import flashsr_weights
    path = os.environ.get("EGREGORA_FLASHSR_WEIGHTS", "")
    if path:
        if not os.path.exists(path):
            raise RuntimeError(f"EGREGORA_FLASHSR_WEIGHTS={path} (missing).")
        params = torch.load(path, map_location="cpu", weights_only=True)
        return arch.config_from_params(params), params
    params, cfg, where = flashsr_weights.load()
    print(f"[FlashSR] checkpoints from {where}: {len(params)} tensors, layer table {cfg}")
    return cfg, params


def _build_engine(cfg, params, dev: int) -> "FlashSREngine":
    """One engine on `dev` from the host state dict (a separate function so that the tests can count / slow down builds)."""
    eng = FlashSREngine(cfg, params, device=f"cuda:{dev}")
    eng.handle                                               # egr_flashsr_create now, on this thread: nothing is left for a worker to build
    eng.warmup(WARMUP_ROWS)
    return eng


def _slot_keys(devs: List[int]) -> List[object]:
    """Registry key of every position of a device list: the device index the first time it appears, ("slot", i) for a repeat --
    "0,0" is two handles (a handle serves one host thread at a time), "0,1,2" is one per device."""
    seen, keys = set(), []
    for i, d in enumerate(devs):
        keys.append(d if d not in seen else ("slot", i))
        seen.add(d)
    return keys


def _ensure(keys_devs: List[Tuple[object, int]]) -> List["FlashSREngine"]:
    """Engines for (registry key, device) pairs, built serially under the module lock from ONE load of the checkpoints."""
    global _SOURCE
    with _LOCK:
        missing = [(k, d) for k, d in keys_devs if k not in _ENGINES]
        if missing:
            native.require_device()
            if _SOURCE is None:
                _SOURCE = _load_source()
            cfg, params = _SOURCE
            for k, d in missing:
                if k not in _ENGINES:                        # a key may repeat in the request
                    _ENGINES[k] = _build_engine(cfg, params, d)
            if all(k in _ENGINES for k in _slot_keys(devices())):
                _SOURCE = None                               # every handle that will be used holds its packed copy: drop the host state dict
        return [_ENGINES[k] for k, _ in keys_devs]


def ensure_ready(device: Optional[int] = None) -> FlashSREngine:
    """Build the engine of `device` (default: the current one) once per process (the reference rebuilds the model on every run(),
    :393).  Weight sources, in order:
      1. EGREGORA_FLASHSR_WEIGHTS -- a torch state dict already in this pack's layer-table names (flashsr_arch.py);
      2. the three upstream checkpoints student_ldm.pth / sr_vocoder.pth / vae.pth discovered in models/audio/flashsr
         (flashsr_weights.discover: both places the reference can mean, or EGREGORA_FLASHSR_CKPT_DIR), mapped through
         flashsr_keymap.json and validated tensor by tensor;
      3. otherwise the reference's "weights missing" error (:314-317).
    The layer table always comes from the checkpoint's own tensor shapes (flashsr_arch.config_from_params).  Seeded synthetic
    weights are for benches and tests only and are never picked up here: those callers build a FlashSREngine themselves and
    install it with set_engine().  Thread-safe: concurrent callers serialise on the module lock and the checkpoints are read once."""
    dev = torch.cuda.current_device() if device is None and torch.cuda.is_available() else (device or 0)
    eng = _ENGINES.get(dev)                                  # (a plain dict read: safe next to a locked writer under the GIL)
    return eng if eng is not None else _ensure([(dev, dev)])[0]


def engines_for(devs: List[int]) -> List[FlashSREngine]:
    """One engine per POSITION of `devs` (a repeated device index gets its own handle), resolved or built on the calling thread."""
    return _ensure(list(zip(_slot_keys(devs), devs)))


def set_engine(engine: Optional[FlashSREngine]):
    """Install a prebuilt engine for its device (benches, tests); None forgets every engine."""
    global _SOURCE
    with _LOCK:
        if engine is None:
            _ENGINES.clear()
            _SOURCE = None
        else:
            _ENGINES[engine.dev.index] = engine


def set_engines(engines: List[FlashSREngine], devs: Optional[List[int]] = None):
    """Install one prebuilt engine per entry of `devs` (default: each engine's own device), keyed as engines_for() looks them up."""
    devs = [e.dev.index for e in engines] if devs is None else list(devs)
    with _LOCK:
        _ENGINES.clear()
        for k, e in zip(_slot_keys(devs), engines):
            _ENGINES[k] = e


def infer_rows(eng: FlashSREngine, rows_x: torch.Tensor, row_ids: torch.Tensor, seed: int,
               lowpass: bool = False) -> torch.Tensor:
    """rows_x [R, chunk] -> [R, chunk] through the C-ABI handle (egr_flashsr_infer: ROWS_PER_PASS rows at a time on the caller's
    stream, noise keyed by global row id; concurrent row groups inside the call, see the module docstring)."""
    return eng.c_infer(rows_x, row_ids, seed, lowpass)


def balanced_bounds(n: int, k: int) -> List[Tuple[int, int]]:
    """n chunks over k workers as contiguous blocks whose sizes differ by at most one (130 over 8: 17, 17, 16, 16, 16, 16, 16, 16)."""
    base, extra = divmod(n, k) if k > 0 else (0, 0)
    out, lo = [], 0
    for i in range(k):
        hi = lo + base + (1 if i < extra else 0)
        out.append((lo, hi))
        lo = hi
    return out


def infer_spans(x_ct: torch.Tensor, n_chunks: int, win: int, hop: int, lowpass: bool) -> torch.Tensor:
    """[C,T] @48 kHz on the GPU -> predictions [n_chunks, C, win].  Chunks are sharded over the ranks of the default process
    group when one exists (contiguous blocks, one all-gather; shard.py); otherwise over the devices of EGREGORA_DEVICES inside
    this process (infer_spans_devices); otherwise they all run here."""
    Cn = x_ct.shape[0]
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        return shard.sharded_chunks(lambda lo, hi: infer_block(x_ct, lo, hi, win, hop, lowpass), n_chunks, (Cn, win), x_ct.device)
    devs = devices() if x_ct.is_cuda else []
    if len(devs) > 1 and n_chunks > 1:
        return infer_spans_devices(x_ct, n_chunks, win, hop, lowpass, devs)
    return infer_block(x_ct, 0, n_chunks, win, hop, lowpass)


def infer_spans_devices(x_ct: torch.Tensor, n_chunks: int, win: int, hop: int, lowpass: bool, devs: List[int]) -> torch.Tensor:
    """The reference's chunk loop (egregora_audio_super_resolution.py:407-420) spread over several GPUs of ONE process: worker i
    (a host thread bound to devs[i], with that device's own handle) takes the contiguous block balanced_bounds(n)[i], reads the
    input through a peer copy, runs its rows batched, and writes its predictions straight into its slice of the [n, C, win]
    tensor on x_ct's device (peer copy = the gather); the caller stitches there.  Noise is keyed by the GLOBAL row id and every
    row's result depends on that row alone, so the outcome does not depend on the device count beyond fp32 round-off from tile
    choices (they follow the row count of a forward).  UNMEASURED on more than one physical GPU in this repository's test
    pool: the one-GPU box exercises it as EGREGORA_DEVICES=0,0."""
    Cn = x_ct.shape[0]
    home = x_ct.device
    out = torch.empty((n_chunks, Cn, win), dtype=torch.float32, device=home)
    torch.cuda.current_stream(home).synchronize()            # x_ct is complete before another device's stream reads it
    engs = engines_for(devs)                                 # built here, serially, from one load of the checkpoints: the workers only run
    jobs = [(engs[i], d, lo, hi) for i, (d, (lo, hi)) in enumerate(zip(devs, balanced_bounds(n_chunks, len(devs)))) if hi > lo]
    errors: List[BaseException] = []

    def work(eng: FlashSREngine, d: int, lo: int, hi: int):
        try:
            with torch.cuda.device(d):
                xd = x_ct if torch.device("cuda", d) == home else x_ct.to(torch.device("cuda", d), non_blocking=True)
                preds = infer_block(xd, lo, hi, win, hop, lowpass, eng)
                out[lo:hi].copy_(preds, non_blocking=True)   # the gather: a peer copy into the stitching device's tensor
                torch.cuda.current_stream().synchronize()
        except BaseException as ex:      # noqa: BLE001 -- re-raised in the caller's thread
            errors.append(ex)

    threads = [threading.Thread(target=work, args=j, name=f"flashsr-dev{j[1]}") for j in jobs[1:]]
    for t in threads:
        t.start()
    work(*jobs[0])                                           # the first block runs on the caller's thread
    for t in threads:
        t.join()
    if errors:
        raise errors[0]
    return out


def infer_block(x_ct: torch.Tensor, lo: int, hi: int, win: int, hop: int, lowpass: bool, eng: Optional[FlashSREngine] = None) -> torch.Tensor:
    """Predictions [hi - lo, C, win] of the chunks lo .. hi-1 of x_ct (one rank's or device's share; noise keyed by the GLOBAL row id)."""
    eng = eng or ensure_ready(x_ct.device.index)
    Cn = x_ct.shape[0]
    if win != eng.cfg.chunk:
        raise RuntimeError(f"chunk length {win} != model chunk {eng.cfg.chunk}")
    chunks = device_ops.chunk_gather(x_ct, win, hop, lo, hi - lo)                 # [n, C, win]
    ids = (torch.arange(lo, hi, device=x_ct.device, dtype=torch.int64)[:, None] * Cn +
           torch.arange(Cn, device=x_ct.device, dtype=torch.int64)[None, :]).reshape(-1)
    y = infer_rows(eng, chunks.view(-1, win), ids, SEED, lowpass=bool(lowpass))
    return y.view(hi - lo, Cn, win)


# ---------------------------------------------------------------------------------------------------- many clips in packed waves
# A TRACK is one channel of one clip.  Rows of different clips share one egr_flashsr_infer call (a row's result is a function of
# (weights, row, seed, row id) alone); the ragged glue around that call reads small int64 device tables built here (DESIGN.md
# section 4.6, include/egregora_amd.h egr_resample_poly_tracks / egr_chunk_gather_tracks / egr_wola_tracks).
DEFAULT_BATCH_ROWS = 1024          # about 1 GB of rows in and 1 GB out at the model's 245760-sample chunk


def n_chunks_for(total: int, win: int, hop: int) -> int:
    """len(audio_glue.spans(total, win, hop)) without the list."""
    if total <= 0:
        return 0
    return 1 if total <= win else 1 + -(-(total - win) // hop)


def resampled_len(n: int, src_sr: int, dst_sr: int) -> int:
    """Length resample.resample_hq gives n samples: ceil(n * up / down)."""
    if int(src_sr) == int(dst_sr):
        return int(n)
    up, down = resample.rates(src_sr, dst_sr)
    return (int(n) * up + down - 1) // down


def clip_rows(channels: int, n: int, sr: int, win: int, hop: int) -> int:
    """Rows (chunks x channels) a [channels, n] clip at rate sr puts on the model's batch dimension."""
    return int(channels) * n_chunks_for(resampled_len(n, sr, audio_glue.REQ_SR), win, hop)


def wave_budget(max_rows: Optional[int] = None) -> int:
    """Row budget of a wave: max_rows, else EGREGORA_FLASHSR_BATCH_ROWS, else 1024, rounded DOWN to a multiple of ROWS_PER_PASS (so only
    the last pass of a wave is partial), never below one pass."""
    if max_rows is None:
        max_rows = int(os.environ.get("EGREGORA_FLASHSR_BATCH_ROWS", str(DEFAULT_BATCH_ROWS)))
    rpp = max(1, ROWS_PER_PASS)
    return max(rpp, (int(max_rows) // rpp) * rpp)


def plan_waves(row_counts: List[int], max_rows: Optional[int] = None) -> List[List[int]]:
    """Clip indices per wave, in input order.  A wave closes before the clip that would take it past the budget (wave_budget); a clip
    is never split, so one with more rows than the budget is a wave of its own; clips of zero rows are in no wave."""
    budget = wave_budget(max_rows)
    waves: List[List[int]] = []
    cur: List[int] = []
    used = 0
    for i, r in enumerate(row_counts):
        if r <= 0:
            continue
        if cur and used + r > budget:
            waves.append(cur)
            cur, used = [], 0
        cur.append(i)
        used += r
    if cur:
        waves.append(cur)
    return waves


def wave_tables(shapes: List[Tuple[int, int]], offsets: List[int], win: int, hop: int) -> dict:
    """Tables of one wave at 48 kHz.  shapes[i] = (C, T) of clip i, offsets[i] = where its channel 0 starts in the flat input
    (channel c at offsets[i] + c * T).  Rows inside a clip are chunk-major then channel -- the order the single-clip path views as
    [n, C, win] -- and carry the ids the clip would have alone (k * C + c).
      rows   int64 [R,3]: (track offset, track length, chunk index k)            -> egr_chunk_gather_tracks
      ids    int64 [R]:   k * C + c                                               -> egr_flashsr_infer row_ids
      tracks int64 [T,5]: (first row, row stride C, n_chunks, total, out offset)  -> egr_wola_tracks
      clip_out [(out offset, C, T)] per clip (a clip's [C,T] result is contiguous), total_out."""
    import numpy as np
    rows, ids, tracks, clip_out = [], [], [], []
    row0, out = 0, 0
    for (Cn, T), off in zip(shapes, offsets):
        n = n_chunks_for(T, win, hop)
        k = np.repeat(np.arange(n, dtype=np.int64), Cn)
        c = np.tile(np.arange(Cn, dtype=np.int64), n)
        rows.append(np.stack([off + c * T, np.full_like(k, T), k], axis=1))
        ids.append(k * Cn + c)
        cc = np.arange(Cn, dtype=np.int64)
        tracks.append(np.stack([row0 + cc, np.full_like(cc, Cn), np.full_like(cc, n), np.full_like(cc, T), out + cc * T], axis=1))
        clip_out.append((out, Cn, T))
        row0 += n * Cn
        out += Cn * T
    cat = lambda parts, cols: np.ascontiguousarray(np.concatenate(parts, axis=0)) if parts else np.zeros((0,) + cols, dtype=np.int64)
    return dict(rows=cat(rows, (3,)), ids=cat(ids, ()), tracks=cat(tracks, (5,)), clip_out=clip_out, total_out=out, n_rows=row0)


def _upscale_single(x: torch.Tensor, sr: int, lowpass: bool, output_sr: int, win: int, hop: int, eng: FlashSREngine) -> torch.Tensor:
    """The single-clip flow of the node (egregora_audio_super_resolution.py run / upscale_48k) for a clip the packed path leaves out:
    its result, or its error."""
    x = x.to(eng.dev, torch.float32).contiguous()
    if sr != audio_glue.REQ_SR:
        x = resample.resample_hq(x, sr, audio_glue.REQ_SR)
    total = x.shape[1]
    n = n_chunks_for(total, win, hop)
    if n == 0:
        y = torch.zeros((1, max(1, total)), dtype=torch.float32, device=x.device)      # upscale_48k's answer (reference :234-235)
    else:
        y = device_ops.wola_stitch(infer_block(x, 0, n, win, hop, lowpass, eng), total, win, hop)
    if output_sr != audio_glue.REQ_SR:
        y = resample.resample_hq(y, audio_glue.REQ_SR, output_sr)
    return y.cpu()


class _Wave:
    """One enqueued wave: the pinned result, the event behind its download, and where each clip's [C,T] lies in it."""
    __slots__ = ("host", "event", "clip_out", "clips", "rows", "calls")


def _enqueue_wave(eng: FlashSREngine, clips, idx: List[int], lowpass: bool, output_sr: int, win: int, hop: int) -> _Wave:
    import numpy as np
    dev = eng.dev
    REQ = audio_glue.REQ_SR
    # raw samples: host clips first (one pinned upload), device clips behind them (device copies)
    order = sorted(idx, key=lambda i: clips[i][0].is_cuda)
    raw_off, pos = {}, 0
    for i in order:
        raw_off[i] = pos
        pos += clips[i][0].numel()
    n_raw = pos
    n_host = sum(clips[i][0].numel() for i in order if not clips[i][0].is_cuda)
    # 48 kHz layout: a 48 kHz clip stays where it was uploaded; every other rate is one group resampled into a region behind the raw
    # samples, the group's tracks back to back
    groups = {sr: [idx[j] for j in js] for sr, js in group_by_rate([int(clips[i][1]) for i in idx], REQ).items()}
    off48, shapes48, group_tabs = {}, {}, []
    pos = n_raw
    for sr in sorted(groups):
        up, down = resample.rates(sr, REQ)
        ins, lens = [], []
        for i in groups[sr]:                    # (a clip's channels lie back to back from raw_off[i]; the clips of a group need not)
            rows = track_rows([tuple(clips[i][0].shape)], raw_off[i])
            ins += rows[0]
            lens += rows[1]
        tab, total = resample.poly_track_table(ins, lens, up, down)
        t = 0
        for i in groups[sr]:
            Cn = clips[i][0].shape[0]
            off48[i] = pos + int(tab[t, 2])
            shapes48[i] = (Cn, int(tab[t, 3]))
            t += Cn
        group_tabs.append((up, down, pos, total, tab))
        pos += total
    n_buf = pos
    for i in idx:
        if i not in off48:
            off48[i], shapes48[i] = raw_off[i], tuple(clips[i][0].shape)
    wt = wave_tables([shapes48[i] for i in idx], [off48[i] for i in idx], win, hop)
    clip_out, total_out = wt["clip_out"], wt["total_out"]
    out_tab = None
    if output_sr != REQ:
        up_o, down_o = resample.rates(REQ, output_sr)
        out_tab, total_res = resample.poly_track_table(wt["tracks"][:, 4], wt["tracks"][:, 3], up_o, down_o)
        t, clip_out = 0, []
        for i in idx:
            Cn = shapes48[i][0]
            clip_out.append((int(out_tab[t, 2]), Cn, int(out_tab[t, 3])))
            t += Cn
    # every table of the wave in one pinned buffer, one copy
    parts = [g[4].reshape(-1) for g in group_tabs] + [wt["rows"].reshape(-1), wt["ids"], wt["tracks"].reshape(-1)]
    if out_tab is not None:
        parts.append(out_tab.reshape(-1))
    flat = np.concatenate(parts)
    tab_host = torch.empty(flat.size, dtype=torch.int64, pin_memory=True)
    tab_host.numpy()[:] = flat
    tab_dev = tab_host.to(dev, non_blocking=True)
    cuts = np.cumsum([0] + [p.size for p in parts])
    dev_part = lambda j, cols: tab_dev[int(cuts[j]):int(cuts[j + 1])].view(-1, cols) if cols else tab_dev[int(cuts[j]):int(cuts[j + 1])]
    # samples
    buf = torch.empty(n_buf, dtype=torch.float32, device=dev)
    if n_host:
        stage = torch.empty(n_host, dtype=torch.float32, pin_memory=True)
        for i in order:
            x = clips[i][0]
            if not x.is_cuda:
                stage[raw_off[i]:raw_off[i] + x.numel()].view(x.shape).copy_(x)
        buf[:n_host].copy_(stage, non_blocking=True)
    for i in order:
        x = clips[i][0]
        if x.is_cuda:
            buf[raw_off[i]:raw_off[i] + x.numel()].view(x.shape).copy_(x)
    calls = 0
    for j, (up, down, base, total, _) in enumerate(group_tabs):
        h, half = resample.filter_for(up, down, dev)
        device_ops.resample_poly_tracks(buf, dev_part(j, 4), total, up, down, h, half, buf[base:base + total])
        calls += 1
    g = len(group_tabs)
    rows = device_ops.chunk_gather_tracks(buf, dev_part(g, 3), win, hop)
    preds = infer_rows(eng, rows, dev_part(g + 1, 0), SEED, lowpass=bool(lowpass))
    y = device_ops.wola_tracks(preds, dev_part(g + 2, 5), total_out, win, hop)
    calls += 3
    if out_tab is not None:
        h, half = resample.filter_for(up_o, down_o, dev)
        y = device_ops.resample_poly_tracks(y, dev_part(g + 3, 4), total_res, up_o, down_o, h, half,
                                            torch.empty(total_res, dtype=torch.float32, device=dev))
        calls += 1
    w = _Wave()
    w.host = torch.empty(y.numel(), dtype=torch.float32, pin_memory=True)
    w.host.copy_(y, non_blocking=True)
    w.event = torch.cuda.Event()
    w.event.record()
    w.clip_out, w.clips, w.rows, w.calls = clip_out, list(idx), wt["n_rows"], calls
    return w


def upscale_many(clips, lowpass, output_sr: int = 48000, *, win: int = audio_glue.CHUNK_SAMPLES, hop: int = audio_glue.HOP_SAMPLES,
                 max_rows: Optional[int] = None, eng: Optional[FlashSREngine] = None, stats: Optional[dict] = None) -> List[torch.Tensor]:
    """Many clips through FlashSR in packed waves.  clips: [([C,T] float32 tensor on the host or the device, sr)], channel counts,
    lengths and rates free; -> [C, T_out] float32 host tensors in input order, each what the node's flow gives the clip alone up to
    fp32 round-off from tile choices (they follow a forward's row count; one clip alone in its wave: the same bits).

    Per wave (plan_waves): one pinned upload of the samples and one of the tables, one egr_resample_poly_tracks per source rate other
    than 48 kHz, one egr_chunk_gather_tracks, one egr_flashsr_infer over all rows (ids k * C + c counted from 0 in each clip, seed SEED),
    one egr_wola_tracks, one egr_resample_poly_tracks when output_sr != 48000, one download: the number of library calls follows the
    number of rates, not of clips.  Wave n + 1 is enqueued before the host waits for wave n's download (one stream, one event per
    wave).  A clip without samples, or of a shape the single-clip flow rejects, goes through that flow and gets its result or its
    error (the error names the clip's index).  stats, when given, receives waves (clip indices per wave), rows and library_calls
    (one entry per wave)."""
    win, hop, output_sr = int(win), int(hop), int(output_sr)
    native.require_device()
    eng = eng or ensure_ready()
    if win != eng.cfg.chunk:
        raise RuntimeError(f"chunk length {win} != model chunk {eng.cfg.chunk}")
    clips = [(x, int(sr)) for x, sr in clips]
    packed = [torch.is_tensor(x) and x.dim() == 2 and x.shape[0] >= 1 and x.shape[1] >= 1 and x.is_floating_point() and sr >= 1
              for x, sr in clips]
    row_counts = [clip_rows(x.shape[0], x.shape[1], sr, win, hop) if ok else 0 for (x, sr), ok in zip(clips, packed)]
    waves = plan_waves(row_counts, max_rows)
    results: List[Optional[torch.Tensor]] = [None] * len(clips)
    done: List[Tuple[List[int], int, int]] = []               # (clip indices, rows, library calls) per finished wave

    def finish(w: _Wave):
        w.event.synchronize()
        for i, (off, Cn, T) in zip(w.clips, w.clip_out):
            results[i] = w.host[off:off + Cn * T].view(Cn, T).clone()
        w.host = None                                           # the pinned buffer goes back before the next wave asks for one
        done.append((w.clips, w.rows, w.calls))

    with torch.cuda.device(eng.dev):
        for i, ((x, sr), ok) in enumerate(zip(clips, packed)):
            if not ok:
                try:
                    results[i] = _upscale_single(torch.as_tensor(x), sr, bool(lowpass), output_sr, win, hop, eng)
                except Exception as ex:      # noqa: BLE001 -- the single-clip flow's own error, with the clip's place in the list
                    raise RuntimeError(f"clip {i}: {ex}") from ex
        pending = None
        for idx in waves:
            cur = _enqueue_wave(eng, clips, idx, bool(lowpass), output_sr, win, hop)
            if pending is not None:
                finish(pending)
            pending = cur
        if pending is not None:
            finish(pending)
    if stats is not None:
        stats["waves"] = [w[0] for w in done]
        stats["rows"] = [w[1] for w in done]
        stats["library_calls"] = [w[2] for w in done]
    return results
