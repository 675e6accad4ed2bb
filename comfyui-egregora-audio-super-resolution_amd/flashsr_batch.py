"""Directory-level front end of FlashSR: every clip of a folder through flashsr_engine.upscale_many in packed waves.

    python flashsr_batch.py --ckpt-dir DIR --in-dir D --out-dir O [--target-sr 48000|44100|96000] [--lowpass-input] [--max-rows N]

Reads every *.wav and *.flac under --in-dir (sorted, recursive) through audio_io, writes <out-dir>/<relative path>.wav (the input's
suffix replaced) as PCM_16 with wavio.write_wav_pcm16, prints one line per file and OK at the end.  A file that cannot be read is
reported and skipped; the exit status is then 1.  Decoding runs on min(16, os.cpu_count()) host threads one wave ahead of the GPU:
while the GPU works on one wave's clips the next wave is decoded and waits, and the WAV files are written by the same threads.
`--ckpt-dir` as in flashsr_min.py.  EGREGORA_FLASHSR_SPLIT=f16x1 selects the fast mode (README) for previews and batch jobs.
"""
import argparse
import os
import queue
import sys
import threading
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

try:
    from .batch_cli import discover, load_pack, read_clip, write_wav
except ImportError:          # run as a script, or loaded by path: batch_cli.py lies next to this file
    sys.path.append(str(Path(__file__).resolve().parent))
    from batch_cli import discover, load_pack, read_clip, write_wav


def _batches(in_dir: Path, files, pool, workers: int, budget: int, win: int, hop: int, skipped):
    """Decoded clips grouped into waves by upscale_many's own rule (a wave closes before the clip that would take it past the
    budget): yields [(relative path, [C,T] tensor, sr)].  At most two pool-widths of files are decoded ahead of the consumer."""
    from egregora_amd import flashsr_engine
    ahead = 2 * workers
    futs = [(rel, pool.submit(read_clip, in_dir / rel)) for rel in files[:ahead]]
    nxt, cur, used = len(futs), [], 0
    while futs:
        rel, f = futs.pop(0)
        if nxt < len(files):
            futs.append((files[nxt], pool.submit(read_clip, in_dir / files[nxt])))
            nxt += 1
        try:
            x, sr = f.result()
        except Exception as ex:      # noqa: BLE001 -- any decoder error skips the file
            skipped.append(rel)
            print(f"SKIP {rel}: {ex}")
            continue
        rows = flashsr_engine.clip_rows(x.shape[0], x.shape[1], sr, win, hop)
        if cur and used + rows > budget:
            yield cur
            cur, used = [], 0
        cur.append((rel, x, sr))
        used += rows
    if cur:
        yield cur


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--ckpt-dir", required=True)
    ap.add_argument("--in-dir", required=True)
    ap.add_argument("--out-dir", required=True)
    ap.add_argument("--target-sr", type=int, default=48000)
    ap.add_argument("--lowpass-input", action="store_true")
    ap.add_argument("--max-rows", type=int, default=None)
    args = ap.parse_args(argv)
    if args.target_sr not in (48000, 44100, 96000):
        raise SystemExit("--target-sr must be 48000, 44100 or 96000 (the node's output_sr choices)")
    in_dir, out_dir = Path(args.in_dir), Path(args.out_dir)
    if not in_dir.is_dir():
        raise SystemExit(f"--in-dir {in_dir} is not a directory")
    ck = Path(args.ckpt_dir) / "flashsr_amd_state_dict.pt"
    if ck.exists():
        os.environ.setdefault("EGREGORA_FLASHSR_WEIGHTS", str(ck))
    else:
        os.environ.setdefault("EGREGORA_FLASHSR_CKPT_DIR", str(args.ckpt_dir))
    if "egregora_amd" not in sys.modules:
        load_pack()
    from egregora_amd import audio_glue, flashsr_engine
    files = discover(in_dir)
    budget = flashsr_engine.wave_budget(args.max_rows)
    win, hop = audio_glue.CHUNK_SAMPLES, audio_glue.HOP_SAMPLES
    skipped, writes = [], []
    ready: "queue.Queue" = queue.Queue(maxsize=1)           # one decoded wave waits while the GPU works on the one before it

    workers = min(16, os.cpu_count() or 1)
    with ThreadPoolExecutor(max_workers=workers) as pool:
        def produce():
            try:
                for b in _batches(in_dir, files, pool, workers, budget, win, hop, skipped):
                    ready.put(b)
                ready.put(None)
            except BaseException as ex:      # noqa: BLE001 -- re-raised on the main thread
                ready.put(ex)

        threading.Thread(target=produce, name="flashsr-batch-decode", daemon=True).start()
        while True:
            b = ready.get()
            if b is None:
                break
            if isinstance(b, BaseException):
                raise b
            ys = flashsr_engine.upscale_many([(x, sr) for _, x, sr in b], bool(args.lowpass_input), args.target_sr, max_rows=budget)
            writes += [pool.submit(write_wav, out_dir, rel, y, args.target_sr) for (rel, _, _), y in zip(b, ys)]
        for w in writes:
            print(w.result())
    print("OK")
    return 1 if skipped else 0


if __name__ == "__main__":
    sys.exit(main())
