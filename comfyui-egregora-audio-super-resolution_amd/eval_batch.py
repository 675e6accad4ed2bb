"""Directory-level front end of the evaluation: every (reference, processed) pair of two folders through eval_many in ragged passes.

    python eval_batch.py --ref-dir R --proc-dir P [--out scores.jsonl] [--loudness] [--n-fft N] [--hop N] [--max-seconds S]

Reads every *.wav and *.flac under --ref-dir and --proc-dir (sorted, recursive) through audio_io; a pair is a reference and a processed
file with the same relative path (suffix aside).  Writes one JSON line per pair -- {"file", the keys of `Metrics (LSD + SI-SDR)`, and
with --loudness "ref_loudness" / "proc_loudness": the dictionaries of `Loudness Meter (BS1770)`} -- and a last line {"pairs", "mean":
{the corpus means of the three metrics}} to --out, or to the standard output without it.  The defaults are the node's widgets.  A
file that cannot be read, or that has no partner in the other folder, is reported on the standard error and makes the exit status 1;
the other pairs are still scored.  A batch closes before the pair that would take it past --max-seconds of audio (channels x
seconds, both sides); inside a batch eval_many plans the waves under EGREGORA_EVAL_WAVE_GB.
"""
import argparse
import json
import sys
from pathlib import Path

try:
    from .batch_cli import batches, discover, load_pack, read_clip
except ImportError:          # run as a script, or loaded by path: batch_cli.py lies next to this file
    sys.path.append(str(Path(__file__).resolve().parent))
    from batch_cli import batches, discover, load_pack, read_clip

MAX_BATCH_SECONDS = 2400.0        # channel-seconds a batch holds on the device (about 0.5 GB of samples)


def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-dir", required=True)
    ap.add_argument("--proc-dir", required=True)
    ap.add_argument("--out", default=None)
    ap.add_argument("--loudness", action="store_true")
    ap.add_argument("--n-fft", type=int, default=2048)
    ap.add_argument("--hop", type=int, default=512)
    ap.add_argument("--max-seconds", type=float, default=MAX_BATCH_SECONDS)
    return ap


def pair_up(ref_dir: Path, proc_dir: Path):
    """-> ([(key, reference path, processed path)], [unpaired relative paths]); key = the relative path without its suffix."""
    refs = {p.with_suffix("").as_posix(): p for p in discover(ref_dir)}
    procs = {p.with_suffix("").as_posix(): p for p in discover(proc_dir)}
    both = sorted(set(refs) & set(procs))
    alone = sorted([f"{ref_dir / refs[k]}" for k in set(refs) - set(procs)] + [f"{proc_dir / procs[k]}" for k in set(procs) - set(refs)])
    return [(k, ref_dir / refs[k], proc_dir / procs[k]) for k in both], alone


def main(argv=None) -> int:
    args = parser().parse_args(argv)
    ref_dir, proc_dir = Path(args.ref_dir), Path(args.proc_dir)
    for d in (ref_dir, proc_dir):
        if not d.is_dir():
            raise SystemExit(f"{d} is not a directory")
    if not args.max_seconds > 0:
        raise SystemExit("--max-seconds must be positive")
    if "egregora_amd" not in sys.modules:
        load_pack()
    from egregora_amd import eval_many
    pairs, alone = pair_up(ref_dir, proc_dir)
    bad = len(alone)
    for p in alone:
        print(f"UNPAIRED {p}", file=sys.stderr)

    def read_all():
        nonlocal bad
        for key, rp, pp in pairs:
            try:
                yield key, read_clip(rp), read_clip(pp)
            except Exception as ex:      # noqa: BLE001 -- any reader error skips the pair
                bad += 1
                print(f"SKIP {key}: {ex}", file=sys.stderr)

    out = open(args.out, "w") if args.out else sys.stdout
    sums, count = {}, 0
    try:
        seconds = lambda it: sum(x.shape[0] * x.shape[1] / sr for x, sr in it[1:])
        for b in batches(read_all(), seconds, args.max_seconds):
            scores = eval_many.metrics_many([(r[0], p[0]) for _, r, p in b], args.n_fft, args.hop)
            if args.loudness:
                loud = eval_many.loudness_many([c for _, r, p in b for c in (r, p)])
            for j, ((key, _, _), s) in enumerate(zip(b, scores)):
                line = dict(file=key, **s)
                if args.loudness:
                    line["ref_loudness"], line["proc_loudness"] = loud[2 * j], loud[2 * j + 1]
                out.write(json.dumps(line) + "\n")
                for k, v in s.items():
                    sums[k] = sums.get(k, 0.0) + v
                count += 1
        out.write(json.dumps({"pairs": count, "mean": {k: v / count for k, v in sums.items()}}) + "\n")
    finally:
        if args.out:
            out.close()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
