"""What the directory front ends (dac_batch.py, dfn_batch.py, eval_batch.py, fatllama_batch.py, flashsr_batch.py, null_batch.py,
wpe_batch.py; flashsr_min.py takes load_pack) share: loading the pack when run as a script, finding and reading the files, grouping
them into batches under a budget, and writing a result as <out-dir>/<relative path>.wav with its report line.
"""
import sys
from pathlib import Path

AUDIO_SUFFIXES = (".wav", ".flac")


def load_pack():
    """The pack as the module egregora_amd, loaded from the directory of this file (a front end run as a script has no package)."""
    import importlib.util
    here = Path(__file__).resolve().parent
    spec = importlib.util.spec_from_file_location("egregora_amd", here / "__init__.py", submodule_search_locations=[str(here)])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["egregora_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def discover(in_dir: Path, suffixes=AUDIO_SUFFIXES):
    """Relative paths of the files under in_dir with one of the suffixes, sorted."""
    return sorted(p.relative_to(in_dir) for p in in_dir.rglob("*") if p.is_file() and p.suffix.lower() in suffixes)


def read_clip(path: Path):
    """-> ([C, T] float32 tensor, sample rate)."""
    from egregora_amd import audio_glue, audio_io
    return audio_glue.upscaler_input(audio_io.read_audio(str(path)))


def read_all(in_dir: Path, files, reader, skipped):
    """(relative path, reader(file)) of every file that reads; one that does not is reported, added to `skipped` and left out."""
    for rel in files:
        try:
            yield rel, reader(in_dir / rel)
        except Exception as ex:      # noqa: BLE001 -- any reader error skips the file
            skipped.append(rel)
            print(f"SKIP {rel}: {ex}")


def batches(items, cost_of, budget: float):
    """items grouped in order; a batch closes before the item that would take it past the budget."""
    cur, used = [], 0.0
    for it in items:
        s = cost_of(it)
        if cur and used + s > budget:
            yield cur
            cur, used = [], 0.0
        cur.append(it)
        used += s
    if cur:
        yield cur


def write_wav(out_dir: Path, rel: Path, y, sr: int) -> str:
    """y [C, T] (host tensor) to <out_dir>/<rel>.wav (rel's suffix replaced) as PCM_16 at sr -> the front ends' line for the file."""
    from egregora_amd import wavio
    dst = (out_dir / rel).with_suffix(".wav")
    dst.parent.mkdir(parents=True, exist_ok=True)
    wavio.write_wav_pcm16(str(dst), y.numpy().T, sr)
    return f"{rel} -> {dst} [{y.shape[0]} ch, {y.shape[1]} samples @ {sr} Hz]"
