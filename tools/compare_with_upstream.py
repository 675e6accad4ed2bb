#!/usr/bin/env python3
"""Opt-in external check (never run by the tests or the bench): compare this pack's Fat-Llama node arithmetic with the
UPSTREAM packages the reference delegates to, on a machine that has them installed.

  pip install fat-llama-fftw soundfile pydub        # (and ffmpeg on PATH), on a box with an MI355X + this pack built
  python tools/compare_with_upstream.py [--seconds 10] [--sr 16000] [--iters 50] [--kbps 1411]

It writes a seeded WAV, runs `fat_llama_fftw.audio_fattener.feed.upscale(...)` with exactly the 7 kwargs the
reference's CPU node passes (reference egregora_fat_llama_cpu.py:126-134), runs the device engine through the node
(`EgregoraFatLlamaGPU`), and prints the reference's own LSD / SI-SDR metric between the two results plus the
fraction of PCM_16 samples that differ.  Until someone runs this, parity with upstream is UNPINNED (see oracle/fatllama.py, SPEC.md):
every disagreement maps to one named field of oracle.fatllama.FatLlamaSpec (factor rounding, interpolation kernel, threshold
reference / kind, autoscale / normalise definitions, PCM scales); `--variants` sweeps the device-side readings of SPEC.md
section 3.  `--flashsr CKPT_DIR` does the same for FlashSR through the node's own checkpoint loader (flashsr_weights.load).
`--dfn3 MODEL_DIR` runs upstream `df.enhance.enhance` and the native DeepFilterNet3 forward pass (dfn_engine, dfn_weights.load) on
the same seeded input and prints the relative error per channel (SPEC.md section 4b; parity unpinned until this has been run).
`--dfn2 MODEL_DIR` does the same for DeepFilterNet2 (dfn2_engine, dfn2_weights.load; SPEC.md section 4c).
`--wpe` runs nara_wpe's documented call -- stft, wpe() on (bins, channels, frames), istft, in float64 -- and this pack's
egr_wpe_dereverb on the same seeded reverberant input and prints the relative error (SPEC.md section 4d; parity unpinned until run).
`--dac MODEL_TYPE` loads the checkpoint dac_weights.discover finds with upstream's `dac.DAC.load`, runs `preprocess` / `encode` /
`decode` per mono row in float64, and the native codec (dac_engine) on the same seeded input: share of equal codes, relative error of
z on the frames whose codes agree, and of the decoded signal (SPEC.md section 4e; parity unpinned until run).
"""
import argparse
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--sr", type=int, default=16000)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--thr", type=float, default=0.6)
    ap.add_argument("--kbps", type=int, default=1411)
    ap.add_argument("--variants", action="store_true", help="sweep the threshold / interpolation readings of SPEC.md section 3")
    ap.add_argument("--flashsr", default="", metavar="CKPT_DIR",
                    help="instead: compare FlashSR_Inference (importable) with this pack on one seeded chunk; CKPT_DIR holds "
                         "student_ldm.pth / sr_vocoder.pth / vae.pth and is read through flashsr_weights.load (the node's loader)")
    ap.add_argument("--dfn3", default="", metavar="MODEL_DIR",
                    help="instead: compare upstream df.enhance.enhance (importable) with the native DeepFilterNet3 on MODEL_DIR "
                         "(config.ini + checkpoints/*.ckpt.best)")
    ap.add_argument("--dfn2", default="", metavar="MODEL_DIR",
                    help="instead: the same for the native DeepFilterNet2 on MODEL_DIR ([train] model = deepfilternet2)")
    ap.add_argument("--wpe", action="store_true", help="instead: compare nara_wpe (importable) with egr_wpe_dereverb (SPEC.md 4d)")
    ap.add_argument("--dac", default="", metavar="MODEL_TYPE",
                    help="instead: compare descript-audio-codec (importable) with the native codec on the discovered checkpoint "
                         "of MODEL_TYPE (44khz / 24khz / 16khz; SPEC.md 4e)")
    args = ap.parse_args()
    if args.dac:
        return compare_dac(args.dac, args.seconds)
    if args.wpe:
        return compare_wpe(args.seconds)
    if args.flashsr:
        return compare_flashsr(args.flashsr)
    if args.dfn3:
        return compare_dfn3(args.dfn3, args.seconds)
    if args.dfn2:
        return compare_dfn3(args.dfn2, args.seconds, dfn2=True)
    try:
        import soundfile as sf
        from fat_llama_fftw.audio_fattener import feed
    except Exception as e:
        sys.exit(f"upstream packages not importable here ({e}); this tool is opt-in")
    import torch
    from packload import load_pack
    from oracle import metrics as om
    pack = load_pack()

    n = int(args.seconds * args.sr)
    rng = np.random.Generator(np.random.PCG64(101))
    t = np.arange(n) / args.sr
    x = sum(np.sin(2 * np.pi * f * t) / (k + 1) for k, f in enumerate(np.geomspace(80, 6000, 8))) + 0.01 * rng.standard_normal(n)
    x = (0.5 * x / np.max(np.abs(x))).astype(np.float32)
    tmp = Path(tempfile.mkdtemp())
    sf.write(str(tmp / "in.wav"), x, args.sr)
    feed.upscale(input_file_path=str(tmp / "in.wav"), output_file_path=str(tmp / "up.wav"), source_format="wav",
                 target_format="wav", max_iterations=args.iters, threshold_value=args.thr, target_bitrate_kbps=args.kbps)
    up, sr_up = sf.read(str(tmp / "up.wav"), dtype="float32", always_2d=False)

    import itertools
    import os
    node = pack.NODE_CLASS_MAPPINGS["EgregoraFatLlamaCPU"]()          # same 7-kwarg contract, device engine
    combos = [""]
    if args.variants:
        names = ("relative", "soft", "no_init_thr")
        thr = [",".join(c) for r in range(len(names) + 1) for c in itertools.combinations(names, r)]
        # x every up-rating rule: linear by the integer factor (survey recall), zero insertion, numpy.interp on the endpoint-inclusive
        # linspace grid by the integer factor, and the same with the ratio applied before int() (judge recall, SPEC.md section 3)
        combos = [",".join(t for t in (a, b) if t) for a in thr for b in ("", "zero_stuff", "linspace", "linspace,ratio_then_int")]
    for combo in combos:
        os.environ["EGREGORA_FATLLAMA_SPEC"] = combo
        (res,) = node.run("wav", args.iters, args.thr, args.kbps, AUDIO={"waveform": torch.from_numpy(x)[None, None], "sample_rate": args.sr})
        mine = res["waveform"][0, 0].numpy()
        m = min(len(up), len(mine))
        lsd = om.lsd_audio(up[:m], mine[:m])
        print(f"[{combo or 'default'}] upstream {up.shape} @ {sr_up} Hz vs this pack {mine.shape} @ {res['sample_rate']} Hz: "
              f"LSD mean/p95 = {lsd[0]:.4g} / {lsd[1]:.4g} dB   SI-SDR = {om.si_sdr(up[:m], mine[:m]):.2f} dB   "
              f"PCM_16 samples differing = {np.mean(np.abs(up[:m] - mine[:m]) * 32768 > 0.5):.4f}")


def compare_wpe(seconds, n_fft=1024, hop=256, taps=10, delay=3, iterations=3):
    """nara_wpe (float64, statistics mode "full") vs egr_wpe_dereverb at the node's default widgets, 16 kHz stereo."""
    import torch
    try:
        from nara_wpe import wpe as np_wpe
        from nara_wpe.utils import istft, stft
    except Exception as e:
        sys.exit(f"nara_wpe not importable here ({e}); this tool is opt-in")
    from packload import load_pack
    load_pack()
    from egregora_amd import wpe_engine
    sys.path.insert(0, str(ROOT / "tests"))
    import wpe_cases
    x = wpe_cases.signal(2, int(seconds * wpe_cases.SR), 4242)
    Y = stft(x.astype(np.float64), size=n_fft, shift=hop)                      # [C, frames, bins] (SPEC WPE-Q1)
    Z = np_wpe.wpe(Y.transpose(2, 0, 1), taps=taps, delay=delay, iterations=iterations, statistics_mode="full")
    up = istft(Z.transpose(1, 2, 0), size=n_fft, shift=hop)
    ours = wpe_engine.dereverb(torch.from_numpy(x).cuda(), n_fft, hop, taps, delay, iterations).cpu().numpy()
    m = min(up.shape[-1], ours.shape[-1])
    print(f"upstream {up.shape} vs this pack {ours.shape}")
    for c in range(2):
        e = float(np.linalg.norm(ours[c, :m] - up[c, :m]) / max(np.linalg.norm(up[c, :m]), 1e-30))
        print(f"channel {c}: relative rms error egr_wpe_dereverb vs nara_wpe {e:.3e}; change against the input "
              f"{float(np.linalg.norm(up[c, :x.shape[1]] - x[c]) / np.linalg.norm(x[c])):.3f}")


def compare_dac(model_type, seconds):
    """Upstream DAC (float64, one mono row at a time) vs egr_dac_encode / egr_dac_decode on the same checkpoint file."""
    import torch
    try:
        import dac
    except Exception as e:
        sys.exit(f"descript-audio-codec not importable here ({e}); this tool is opt-in")
    from packload import load_pack
    load_pack()
    from egregora_amd import dac_engine, dac_weights
    path = dac_weights.discover(model_type)
    if path is None:
        sys.exit(dac_weights.not_found_message(model_type))
    eng = dac_engine.engine(path, 0)
    up = dac.DAC.load(str(path)).double().eval()
    sr = int(eng.cfg["sample_rate"])
    n = int(seconds * sr)
    rng = np.random.Generator(np.random.PCG64(4343))
    t = np.arange(n) / sr
    x = np.stack([sum(np.sin(2 * np.pi * f * (1 + 0.01 * c) * t) / (k + 1) for k, f in enumerate(np.geomspace(80, 6000, 8))) for c in range(2)])
    x = (0.3 * x / np.abs(x).max() + 0.01 * rng.standard_normal(x.shape)).astype(np.float32)
    xt = torch.from_numpy(x)
    with torch.no_grad():
        xp = up.preprocess(xt.double()[:, None], sr)
        z_up, codes_up = up.encode(xp)[:2]
        y_up = up.decode(z_up)[:, 0]
    z, codes = eng.encode(xt.cuda())
    y = eng.decode(z).cpu()
    same = (codes.cpu().long() == codes_up).all(dim=1)
    rel = lambda a, b: float((a.double() - b).norm() / max(float(b.norm()), 1e-30))
    print(f"codes {tuple(codes.shape)}: frames with all codes equal {float(same.double().mean()):.4%}")
    if same.any():
        print(f"z on those frames: relative rms error {rel(z.cpu().transpose(1, 2)[same], z_up.transpose(1, 2)[same]):.3e}")
    m = min(y.shape[-1], y_up.shape[-1])
    print(f"decoded {tuple(y.shape)} vs upstream {tuple(y_up.shape)}: relative rms error {rel(y[:, :m], y_up[:, :m]):.3e}")


def compare_dfn3(model_dir, seconds, dfn2=False):
    """Upstream DeepFilterNet3 (DeepFilterNet2 with dfn2) -- df.enhance with the checkpoint in MODEL_DIR -- vs the native forward pass,
    48 kHz stereo."""
    import torch
    try:
        from df.enhance import enhance, init_df
    except Exception as e:
        sys.exit(f"df (DeepFilterNet) not importable here ({e}); this tool is opt-in")
    from packload import load_pack
    load_pack()
    if dfn2:
        from egregora_amd import dfn2_engine as dfn_engine, dfn2_weights as dfn_weights
    else:
        from egregora_amd import dfn_engine, dfn_weights
    rng = np.random.Generator(np.random.PCG64(1234))
    n = int(seconds * 48000)
    t = np.arange(n) / 48000.0
    x = np.stack([0.3 * np.sin(2 * np.pi * (220 + 30 * c) * t) * (0.5 + 0.5 * np.sin(2 * np.pi * 1.7 * t)) + 0.05 * rng.standard_normal(n)
                  for c in range(2)]).astype(np.float32)
    model, df_state, _ = init_df(model_dir, config_allow_defaults=False)
    model = model.eval()
    with torch.no_grad():
        up = torch.cat([enhance(model, df_state, torch.from_numpy(x[c:c + 1])) for c in range(2)], 0).numpy()
    make = dfn_engine.Dfn2Engine if dfn2 else dfn_engine.Dfn3Engine
    eng = make(dfn_weights.load(Path(model_dir)), torch.cuda.current_device())
    ours = eng.enhance(torch.from_numpy(x).cuda()).cpu().numpy()
    for c in range(2):
        e = float(np.linalg.norm(ours[c] - up[c]) / max(np.linalg.norm(up[c]), 1e-30))
        print(f"channel {c}: relative rms error native vs df {e:.3e} (max abs {float(np.abs(ours[c] - up[c]).max()):.3e})")


def compare_flashsr(ckpt_dir):
    """Upstream FlashSR vs this pack on one 5.12 s chunk with the SAME injected noise (upstream draws its own, so its sampler is
    patched to return ours); prints per-stage shapes that differ and the LSD of the waveforms."""
    import torch
    try:
        from FlashSR.FlashSR import FlashSR
    except Exception as e:
        sys.exit(f"FlashSR_Inference not importable here ({e}); this tool is opt-in")
    from packload import load_pack
    load_pack()
    from egregora_amd import flashsr_engine as E, flashsr_weights as W
    from oracle import metrics as om
    d = Path(ckpt_dir)
    for f in W.FILES:
        print(f"# {f}: {len(W.read_state_dict(d / f))} tensors")
    params, cfg, _ = W.load(d)                      # raises with the list of unmapped / mismatched tensors: fix flashsr_keymap.json
    eng = E.FlashSREngine(cfg, params)
    g = torch.Generator().manual_seed(7)
    x = (0.3 * torch.randn(1, cfg.chunk, generator=g)).cuda()
    nz = eng.noise(1, None, 7)
    mine = eng.c_forward(x, nz).cpu().numpy()
    model = FlashSR(str(d / "student_ldm.pth"), str(d / "sr_vocoder.pth"), str(d / "vae.pth")).eval().cuda()
    real_randn = torch.randn
    torch.randn = lambda *a, **k: nz.permute(0, 3, 1, 2).contiguous() if tuple(a[:1]) and list(a[0] if isinstance(a[0], (tuple, list)) else a) == list(nz.permute(0, 3, 1, 2).shape) else real_randn(*a, **k)
    try:
        with torch.inference_mode():
            up = model(x, lowpass_input=False).float().cpu().numpy()
    finally:
        torch.randn = real_randn
    m = min(up.shape[-1], mine.shape[-1])
    lsd = om.lsd_audio(up[..., :m], mine[..., :m])
    print(f"FlashSR upstream vs this pack: LSD mean/p95 = {lsd[0]:.4g} / {lsd[1]:.4g} dB, SI-SDR {om.si_sdr(up[0, :m], mine[0, :m]):.2f} dB")


if __name__ == "__main__":
    main()
