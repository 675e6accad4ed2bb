"""Directory-level front end of the Fat-Llama spectral enhancer: every clip of a folder through fatllama_many in packed waves.

    python fatllama_batch.py --in-dir D --out-dir O [--max-iterations N] [--threshold T] [--bitrate KBPS] [--no-normalize]
                             [--no-autoscale] [--max-seconds S]

Reads every *.wav and *.flac under --in-dir (sorted, recursive) through audio_io and writes <out-dir>/<relative path>.wav: PCM_16 at the
clip's output rate (its own rate times its own up-rating factor), the samples of `Egregora Fat Llama (GPU)` for that file.  The
defaults are the node's widgets.  One line per file and OK at the end; a file that cannot be read is reported and skipped, the exit
status is then 1.  A batch closes before the clip that would take it past --max-seconds of audio (channels x seconds); inside a batch
fatllama_many.plan_waves forms the waves under EGREGORA_FATLLAMA_WAVE_GB and EGREGORA_FATLLAMA_WAVE_SLACK.
"""
import argparse
import sys
from pathlib import Path

try:
    from .batch_cli import AUDIO_SUFFIXES, batches, discover, load_pack, read_all, write_wav
except ImportError:          # run as a script, or loaded by path: batch_cli.py lies next to this file
    sys.path.append(str(Path(__file__).resolve().parent))
    from batch_cli import AUDIO_SUFFIXES, batches, discover, load_pack, read_all, write_wav

MAX_BATCH_SECONDS = 2400.0        # channel-seconds a batch holds on the device (about 0.5 GB of samples in, as much out at factor 1)


def read_clip(path: Path):
    """-> ([C, T] float32 tensor, sample rate), as the node resolves an audio_path."""
    from egregora_amd import egregora_fat_llama_gpu
    return egregora_fat_llama_gpu.resolve_input(audio_path=str(path))


def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    ap.add_argument("--in-dir", required=True)
    ap.add_argument("--out-dir", required=True)
    ap.add_argument("--max-iterations", type=int, default=300)
    ap.add_argument("--threshold", type=float, default=0.6)
    ap.add_argument("--bitrate", type=int, default=1411)
    ap.add_argument("--no-normalize", action="store_true")
    ap.add_argument("--no-autoscale", action="store_true")
    ap.add_argument("--max-seconds", type=float, default=MAX_BATCH_SECONDS)
    return ap


def main(argv=None) -> int:
    args = parser().parse_args(argv)
    in_dir, out_dir = Path(args.in_dir), Path(args.out_dir)
    if not in_dir.is_dir():
        raise SystemExit(f"--in-dir {in_dir} is not a directory")
    if not args.max_seconds > 0 or args.max_iterations < 1:
        raise SystemExit("--max-seconds must be positive and --max-iterations at least 1")
    if "egregora_amd" not in sys.modules:
        load_pack()
    from egregora_amd import fatllama_many
    skipped = []
    clips = read_all(in_dir, discover(in_dir, AUDIO_SUFFIXES), read_clip, skipped)
    for b in batches(clips, lambda it: it[1][0].shape[0] * it[1][0].shape[1] / it[1][1], args.max_seconds):
        stats = {}
        res = fatllama_many.enhance_many([c for _, c in b], args.max_iterations, args.threshold, args.bitrate, not args.no_normalize,
                                         not args.no_autoscale, stats=stats)
        for (rel, (x, sr)), (y, sr_out) in zip(b, res):
            print(write_wav(out_dir, rel, y, sr_out))
        print(f"batch of {len(b)}: {stats['waves']} waves, {stats['fallbacks']} one by one")
    print("OK")
    return 1 if skipped else 0


if __name__ == "__main__":
    sys.exit(main())
