"""Directory-level front end of the Descript Audio Codec: every clip of a folder through dac_many in padded passes.

    python dac_batch.py --model-type {44khz,24khz,16khz} [--model-dir DIR] --in-dir D --out-dir O [--decode] [--max-seconds S]

Encode reads every *.wav and *.flac under --in-dir (sorted, recursive) through audio_io and writes <out-dir>/<relative path>.npz (the
input's suffix replaced): codes int32 [C, n_codebooks, frames], sample_rate (the file's), model_sample_rate, model_type, n_samples
(the file's length at its own rate).  --decode reads every *.npz under --in-dir and writes <out-dir>/<relative path>.wav: PCM_16 at
sample_rate, trimmed to n_samples.  One line per file and OK at the end; a file that cannot be read is reported and skipped, the exit
status is then 1.  A batch closes before the clip that would take it past --max-seconds of audio (channels x seconds, default
MAX_BATCH_SECONDS); inside a batch DacEngine.encode_many / decode_many plan the waves under EGREGORA_DAC_WORKSPACE_GB.  --model-dir names
the checkpoint directory (EGREGORA_DAC_MODEL_DIR); without it the node's discovery applies.  Nothing is downloaded.
"""
import argparse
import os
import sys
from pathlib import Path

import numpy as np

try:
    from .batch_cli import AUDIO_SUFFIXES, batches, discover, load_pack, read_all, read_clip, write_wav
except ImportError:          # run as a script, or loaded by path: batch_cli.py lies next to this file
    sys.path.append(str(Path(__file__).resolve().parent))
    from batch_cli import AUDIO_SUFFIXES, batches, discover, load_pack, read_all, read_clip, write_wav

MAX_BATCH_SECONDS = 1200.0        # channel-seconds a batch holds on the device before it is encoded (about 0.2 GB of samples)


def read_codes(path: Path) -> dict:
    import torch
    with np.load(str(path)) as f:
        d = {"codes": torch.from_numpy(f["codes"].astype(np.int32)), "sample_rate": int(f["sample_rate"]),
             "model_sample_rate": int(f["model_sample_rate"]), "model_type": str(f["model_type"]), "n_samples": int(f["n_samples"])}
    if d["codes"].dim() != 3 or 0 in d["codes"].shape:
        raise ValueError(f"codes of shape {tuple(d['codes'].shape)}")
    return d


def write_codes(path: Path, r: dict, model_type: str):
    path.parent.mkdir(parents=True, exist_ok=True)
    np.savez(str(path), codes=r["codes"].numpy().astype(np.int32), sample_rate=np.int64(r["sample_rate"]),
             model_sample_rate=np.int64(r["model_sample_rate"]), model_type=np.str_(model_type), n_samples=np.int64(r["n_samples"]))


def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    ap.add_argument("--model-type", required=True, choices=["44khz", "24khz", "16khz"])
    ap.add_argument("--model-dir", default=None)
    ap.add_argument("--in-dir", required=True)
    ap.add_argument("--out-dir", required=True)
    ap.add_argument("--decode", action="store_true")
    ap.add_argument("--max-seconds", type=float, default=MAX_BATCH_SECONDS)
    return ap


def main(argv=None) -> int:
    args = parser().parse_args(argv)
    in_dir, out_dir = Path(args.in_dir), Path(args.out_dir)
    if not in_dir.is_dir():
        raise SystemExit(f"--in-dir {in_dir} is not a directory")
    if not args.max_seconds > 0:
        raise SystemExit("--max-seconds must be positive")
    if args.model_dir:
        os.environ["EGREGORA_DAC_MODEL_DIR"] = str(args.model_dir)
    if "egregora_amd" not in sys.modules:
        load_pack()
    from egregora_amd import dac_many
    skipped = []
    if not args.decode:
        clips = read_all(in_dir, discover(in_dir, AUDIO_SUFFIXES), read_clip, skipped)
        for b in batches(clips, lambda it: it[1][0].shape[0] * it[1][0].shape[1] / it[1][1], args.max_seconds):
            for (rel, (x, sr)), r in zip(b, dac_many.encode_many([c for _, c in b], args.model_type)):
                dst = (out_dir / rel).with_suffix(".npz")
                write_codes(dst, r, args.model_type)
                print(f"{rel} -> {dst} [{r['codes'].shape[0]} ch, {r['codes'].shape[2]} frames, {r['n_samples']} samples @ {sr} Hz]")
    else:
        items = read_all(in_dir, discover(in_dir, (".npz",)), read_codes, skipped)
        for b in batches(items, lambda it: it[1]["codes"].shape[0] * it[1]["n_samples"] / it[1]["sample_rate"], args.max_seconds):
            for rel, d in b:
                if d["model_type"] != args.model_type:
                    raise SystemExit(f"{rel}: encoded with model type {d['model_type']}, --model-type is {args.model_type}")
            for (rel, d), y in zip(b, dac_many.decode_many([d for _, d in b], args.model_type)):
                n = d["n_samples"]
                if y.shape[1] < n:
                    import torch
                    y = torch.nn.functional.pad(y, (0, n - y.shape[1]))
                y = y[:, :n]
                print(write_wav(out_dir, rel, y, d["sample_rate"]))
    print("OK")
    return 1 if skipped else 0


if __name__ == "__main__":
    sys.exit(main())
