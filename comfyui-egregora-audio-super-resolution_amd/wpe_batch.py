"""Directory-level front end of the WPE dereverberation: every clip of a folder through wpe_many.dereverb_many in ragged passes.

    python wpe_batch.py --in-dir D --out-dir O [--taps N] [--delay N] [--iterations N] [--n-fft N] [--hop N] [--max-seconds S]

Reads every *.wav and *.flac under --in-dir (sorted, recursive) through audio_io and writes <out-dir>/<relative path>.wav (the input's
suffix replaced) at the input's rate as PCM_16 with wavio.write_wav_pcm16: the samples of `Egregora WPE Dereverb` for that file.  The
defaults are the node's widgets.  One line per file and OK at the end; a file that cannot be read is reported and skipped, the exit
status is then 1.  A batch closes before the clip that would take it past --max-seconds of audio (channels x seconds); inside a batch
wpe_many.plan_waves forms the waves under EGREGORA_WPE_WAVE_GB.
"""
import argparse
import sys
from pathlib import Path

try:
    from .batch_cli import AUDIO_SUFFIXES, batches, discover, load_pack, read_all, read_clip, write_wav
except ImportError:          # run as a script, or loaded by path: batch_cli.py lies next to this file
    sys.path.append(str(Path(__file__).resolve().parent))
    from batch_cli import AUDIO_SUFFIXES, batches, discover, load_pack, read_all, read_clip, write_wav

MAX_BATCH_SECONDS = 2400.0        # channel-seconds a batch holds on the device (about 0.5 GB of samples in, as much out)


def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    ap.add_argument("--in-dir", required=True)
    ap.add_argument("--out-dir", required=True)
    ap.add_argument("--taps", type=int, default=10)
    ap.add_argument("--delay", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--n-fft", type=int, default=1024)
    ap.add_argument("--hop", type=int, default=256)
    ap.add_argument("--max-seconds", type=float, default=MAX_BATCH_SECONDS)
    return ap


def main(argv=None) -> int:
    args = parser().parse_args(argv)
    in_dir, out_dir = Path(args.in_dir), Path(args.out_dir)
    if not in_dir.is_dir():
        raise SystemExit(f"--in-dir {in_dir} is not a directory")
    if not args.max_seconds > 0 or min(args.taps, args.delay, args.iterations) < 1:
        raise SystemExit("--max-seconds must be positive, --taps, --delay and --iterations at least 1")
    if "egregora_amd" not in sys.modules:
        load_pack()
    from egregora_amd import wpe_many
    widgets = dict(taps=args.taps, delay=args.delay, iterations=args.iterations, n_fft=args.n_fft, hop=args.hop)
    skipped = []
    clips = read_all(in_dir, discover(in_dir, AUDIO_SUFFIXES), read_clip, skipped)
    for b in batches(clips, lambda it: it[1][0].shape[0] * it[1][0].shape[1] / it[1][1], args.max_seconds):
        stats = {}
        res = wpe_many.dereverb_many([c for _, c in b], stats=stats, **widgets)
        for (rel, (x, sr)), y in zip(b, res):
            print(write_wav(out_dir, rel, y, sr))
        print(f"batch of {len(b)}: {stats.get('waves', 0)} waves, {stats.get('alone', 0)} one by one")
    print("OK")
    return 1 if skipped else 0


if __name__ == "__main__":
    sys.exit(main())
