"""Directory-level front end of the null test: every (reference, processed) pair of two folders through null_many.full_many.

    python null_batch.py --ref-dir R --proc-dir P [--out scores.jsonl] [--write-null DIR] [--write-matched DIR]
                         [--align-max-shift-ms N] [--no-fractional] [--fir-len N] [--match-mode LUFS-I|RMS] [--least-squares-scale]
                         [--no-compute-corr] [--no-compute-null-rms] [--no-compute-null-lufs] [--no-compute-lsd] [--compute-hf-residual]
                         [--n-fft N] [--hop N] [--max-seconds S]

Reads every *.wav and *.flac under --ref-dir and --proc-dir (sorted, recursive) through audio_io; a pair is a reference and a processed
file with the same relative path (suffix aside), as in eval_batch.py.  Writes one JSON line per pair -- {"file", "delay_ms", "gain_db",
and the metrics of `Null Test (Full)`} -- and a last line {"pairs", "mean": {the corpus means of every number}} to --out, or to the
standard output without it.  --write-null / --write-matched store the null and the aligned, gain-matched signal of every pair under the
given folder at the pair's relative path as PCM_16 at the reference's rate.  The defaults are the node's widgets.  A file that cannot
be read, or that has no partner, is reported on the standard error and makes the exit status 1; the other pairs are still processed.
A batch closes before the pair that would take it past --max-seconds of audio (channels x seconds, both sides); inside a batch
null_many plans the waves under EGREGORA_EVAL_WAVE_GB.
"""
import argparse
import json
import sys
from pathlib import Path

try:
    from .batch_cli import batches, load_pack, read_clip
    from .eval_batch import MAX_BATCH_SECONDS, pair_up
except ImportError:          # run as a script, or loaded by path: batch_cli.py lies next to this file
    sys.path.append(str(Path(__file__).resolve().parent))
    from batch_cli import batches, load_pack, read_clip
    from eval_batch import MAX_BATCH_SECONDS, pair_up

_ON = ("fractional", "compute_corr", "compute_null_rms", "compute_null_lufs", "compute_lsd")
_OFF = ("least_squares_scale", "compute_hf_residual")


def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-dir", required=True)
    ap.add_argument("--proc-dir", required=True)
    ap.add_argument("--out", default=None)
    ap.add_argument("--write-null", default=None)
    ap.add_argument("--write-matched", default=None)
    ap.add_argument("--align-max-shift-ms", type=int, default=200)
    ap.add_argument("--fir-len", type=int, default=64)
    ap.add_argument("--match-mode", choices=["LUFS-I", "RMS"], default="LUFS-I")
    for name in _ON:
        ap.add_argument("--no-" + name.replace("_", "-"), dest=name, action="store_false", default=True)
    for name in _OFF:
        ap.add_argument("--" + name.replace("_", "-"), dest=name, action="store_true", default=False)
    ap.add_argument("--n-fft", type=int, default=2048)
    ap.add_argument("--hop", type=int, default=512)
    ap.add_argument("--max-seconds", type=float, default=MAX_BATCH_SECONDS)
    return ap


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
    from egregora_amd import null_many, wavio
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

    def store(folder, key, y, sr):
        dst = Path(folder) / (key + ".wav")
        dst.parent.mkdir(parents=True, exist_ok=True)
        wavio.write_wav_pcm16(str(dst), y.cpu().numpy().T, sr)

    out = open(args.out, "w") if args.out else sys.stdout
    sums, count = {}, 0
    try:
        seconds = lambda it: sum(x.shape[0] * x.shape[1] / sr for x, sr in it[1:])
        for b in batches(read_all(), seconds, args.max_seconds):
            res = null_many.full_many([(r[0], p[0]) for _, r, p in b], [(r[1], p[1]) for _, r, p in b], args.align_max_shift_ms, "gcc-phat",
                                      args.fractional, args.fir_len, args.match_mode, args.least_squares_scale, args.compute_corr,
                                      args.compute_null_rms, args.compute_null_lufs, args.compute_lsd, args.compute_hf_residual,
                                      args.n_fft, args.hop)
            for (key, r, _), (matched, null, delay_ms, gain_db, metrics) in zip(b, res):
                line = dict(file=key, delay_ms=delay_ms, gain_db=gain_db, **metrics)
                out.write(json.dumps(line) + "\n")
                for k, v in line.items():
                    if k != "file":
                        sums[k] = sums.get(k, 0.0) + v
                count += 1
                if args.write_null:
                    store(args.write_null, key, null, r[1])
                if args.write_matched:
                    store(args.write_matched, key, matched, r[1])
        out.write(json.dumps({"pairs": count, "mean": {k: v / count for k, v in sums.items()}}) + "\n")
    finally:
        if args.out:
            out.close()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
