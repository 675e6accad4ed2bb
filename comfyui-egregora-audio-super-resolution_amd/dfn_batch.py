"""Directory-level front end of the DeepFilterNet stage: every clip of a folder through dfn_many.denoise_many in ragged passes.

    python dfn_batch.py --model {DeepFilterNet2,DeepFilterNet3} [--model-dir DIR] --in-dir D --out-dir O [--max-frames N] [widget options]

Reads every *.wav and *.flac under --in-dir (sorted, recursive) through audio_io, writes <out-dir>/<relative path>.wav (the input's
suffix replaced) at the input's rate as PCM_16 with wavio.write_wav_pcm16, prints one line per file and OK at the end.  A file that
cannot be read is reported and skipped; the exit status is then 1.  Decoding runs on min(16, os.cpu_count()) host threads one batch
ahead of the GPU, and the WAV files are written by the same threads.  A batch closes before the clip that would take it past
--max-frames network frames (channels x frames at 48 kHz, default MAX_BATCH_FRAMES); inside a batch DfnEngine.enhance_many plans the
waves under the workspace budget EGREGORA_DFN_WORKSPACE_GB.  --model-dir names the model directory (EGREGORA_DFN_MODEL_DIR); without
it the node's discovery applies.  Nothing is downloaded.  The widget options are the node's widgets with their defaults.
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
MAX_BATCH_FRAMES = 131072        # about 18 GB of workspace at 139 KB per frame and row
FFT, HOP = 960, 480              # both models' framing at 48 kHz; only the batch rule counts with it


def clip_frames(channels: int, n: int, sr: int) -> int:
    """Network frames (channels x frames) a [channels, n] clip at rate sr brings: its 48 kHz length framed as the models frame it."""
    n48 = n if sr == 48000 else -(-n * 48000 // sr)
    return int(channels) * ((n48 + FFT) // HOP)


def _batches(in_dir: Path, files, pool, workers: int, budget: int, skipped):
    """Decoded clips grouped into batches (a batch closes before the clip that would take it past the budget): yields
    [(relative path, [C,T] tensor, sr)].  At most two pool-widths of files are decoded ahead of the consumer."""
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
            if x.shape[1] < 1:
                raise ValueError("no samples")
        except Exception as ex:      # noqa: BLE001 -- any decoder error skips the file
            skipped.append(rel)
            print(f"SKIP {rel}: {ex}")
            continue
        rows = clip_frames(x.shape[0], x.shape[1], sr)
        if cur and used + rows > budget:
            yield cur
            cur, used = [], 0
        cur.append((rel, x, sr))
        used += rows
    if cur:
        yield cur


def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", required=True, choices=["DeepFilterNet2", "DeepFilterNet3"])
    ap.add_argument("--model-dir", default=None)
    ap.add_argument("--in-dir", required=True)
    ap.add_argument("--out-dir", required=True)
    ap.add_argument("--max-frames", type=int, default=MAX_BATCH_FRAMES)
    ap.add_argument("--stereo-mode", choices=["per_channel", "downmix_mono"], default="per_channel")
    ap.add_argument("--strength", type=float, default=0.65)
    ap.add_argument("--mix-curve", choices=["equal_power", "linear"], default="equal_power")
    ap.add_argument("--adaptive-vad-source", choices=["rms", "rnnoise", "none"], default="rms")
    ap.add_argument("--adaptive-mode", choices=["off", "more_on_noise", "more_on_speech", "gate_on_noise"], default="more_on_noise")
    ap.add_argument("--adaptive-amount", type=float, default=0.45)
    ap.add_argument("--vad-threshold", type=float, default=0.90)
    ap.add_argument("--vad-smooth-ms", type=int, default=60)
    ap.add_argument("--post-gain-db", type=float, default=0.5)
    ap.add_argument("--ceiling", type=float, default=0.98)
    ap.add_argument("--no-limit-ceiling", dest="limit_ceiling", action="store_false")
    return ap


def widgets_of(args) -> dict:
    return dict(stereo_mode=args.stereo_mode, strength=args.strength, mix_curve=args.mix_curve, adaptive_vad_source=args.adaptive_vad_source,
                adaptive_mode=args.adaptive_mode, adaptive_amount=args.adaptive_amount, vad_threshold=args.vad_threshold,
                vad_smooth_ms=args.vad_smooth_ms, post_gain_db=args.post_gain_db, ceiling=args.ceiling, limit_ceiling=args.limit_ceiling)


def main(argv=None) -> int:
    args = parser().parse_args(argv)
    in_dir, out_dir = Path(args.in_dir), Path(args.out_dir)
    if not in_dir.is_dir():
        raise SystemExit(f"--in-dir {in_dir} is not a directory")
    if args.max_frames < 1:
        raise SystemExit("--max-frames must be at least 1")
    if args.model_dir:
        os.environ["EGREGORA_DFN_MODEL_DIR"] = str(args.model_dir)
    if "egregora_amd" not in sys.modules:
        load_pack()
    from egregora_amd import dfn_many
    files = discover(in_dir)
    widgets = widgets_of(args)
    skipped, writes = [], []
    ready: "queue.Queue" = queue.Queue(maxsize=1)           # one decoded batch waits while the GPU works on the one before it

    workers = min(16, os.cpu_count() or 1)
    with ThreadPoolExecutor(max_workers=workers) as pool:
        def produce():
            try:
                for b in _batches(in_dir, files, pool, workers, args.max_frames, skipped):
                    ready.put(b)
                ready.put(None)
            except BaseException as ex:      # noqa: BLE001 -- re-raised on the main thread
                ready.put(ex)

        threading.Thread(target=produce, name="dfn-batch-decode", daemon=True).start()
        while True:
            b = ready.get()
            if b is None:
                break
            if isinstance(b, BaseException):
                raise b
            ys = dfn_many.denoise_many([(x, sr) for _, x, sr in b], args.model, **widgets)
            writes += [pool.submit(write_wav, out_dir, rel, y, sr) for (rel, _, sr), y in zip(b, ys)]
        for w in writes:
            print(w.result())
    print("OK")
    return 1 if skipped else 0


if __name__ == "__main__":
    sys.exit(main())
