"""WPE on the device (csrc/egr_wpe.hip) at the shapes tests/test_gpu_wpe.py does not reach, against tests/wpe_numpy.py and with that
file's bars unchanged:

  transforms   framings with n_fft / hop = 2 and 16 (k_wpe_istft sums n_fft / hop + WPE_SEG - 1 frames per run of WPE_SEG segments),
               the radices 5, 7, 11 and 13, an input shorter than one frame and the smallest n_fft; n_fft = 34 (17 divides its
               half) is refused.
  solve        cases F, G, H, L of tests/wpe_cases.py (32 to 64 channels, all "well": tests/test_wpe_host.py pins it).  F and G
               have more than 256 blocks of 4 x 4 statistics (k_wpe_iter<2, *>, 64 x 64 Cholesky), G, H and L more than 32
               channels (the 32-frame tile), L needs 163 584 of the 163 840 bytes of LDS.  Backward error of every iteration,
               forward error of the chain, egr_wpe_dereverb against the staged calls bit for bit.
  refusal      64 channels at delay 128 pass every limit but the LDS one; nothing may be enqueued, and the next call is correct.
  node         one Egregora_WPE_Dereverb call on the 32 channels of case F.

The file runs in order of rising novelty: transforms (kernels every test uses), then H (one block per thread), F, G, L.
"""
import numpy as np
import pytest
import torch

import wpe_cases
import wpe_numpy as wn
from test_gpu_wpe import chain128, dev, enhance_pack, spectra          # noqa: F401 (enhance_pack is a fixture)

pytestmark = pytest.mark.gpu

# (n_fft, hop, n): ratio 2; ratio 16 (two WPE_SEG groups per frame); radices 5 x 7; radices 11 x 13; n < n_fft; the smallest n_fft
FRAMINGS = [(64, 32, 900), (128, 8, 900), (70, 35, 1000), (286, 143, 3000), (256, 64, 100), (4, 2, 50)]


@pytest.mark.parametrize("n_fft,hop,n", FRAMINGS)
def test_transforms(pack, n_fft, hop, n):
    from egregora_amd import wpe_engine
    y = wpe_cases.signal(2, n, 1000 + n_fft)
    ref = wn.analysis(y, n_fft, hop)
    bar = 4 * wn.rel_rms(wn.analysis(y, n_fft, hop, np.float32), ref)
    Yd = wpe_engine.stft(dev(y), n_fft, hop)
    assert tuple(Yd.shape) == ref.shape == (n_fft // 2 + 1, 2, wn.frame_count(n, n_fft, hop))
    err = wn.rel_rms(Yd.cpu().numpy(), ref)
    print(f"stft ({n_fft}, {hop}, {n}): device {err:.2e}, bar {bar:.2e} (4 x float32 numpy), ratio {err / bar:.2f}")
    assert err <= bar, (err, bar)
    z1 = wpe_engine.istft(Yd, n_fft, hop)
    z2 = wpe_engine.istft(wpe_engine.stft(dev(y), n_fft, hop), n_fft, hop)
    assert tuple(z1.shape) == (2, wn.out_length(n, n_fft, hop)) and torch.equal(z1, z2)
    z = z1.cpu().numpy()
    peak = float(np.abs(y).max())
    rt = float(np.abs(z[:, :n] - y).max()) / peak
    print(f"round trip ({n_fft}, {hop}, {n}): {rt:.2e} of the peak (bar 2e-6)")
    assert rt <= 2e-6 and float(np.abs(z[:, n:]).max(initial=0.0)) <= 2e-6 * peak


def test_prime_factor_above_13_is_refused(pack):
    from egregora_amd import wpe_engine
    y = dev(wpe_cases.signal(1, 500, 5))
    with pytest.raises(RuntimeError, match="prime factor above 13"):
        wpe_engine.stft(y, 34, 17)
    with pytest.raises(RuntimeError, match="prime factor above 13"):
        wpe_engine.dereverb(y, 34, 17, 2, 1, 1)


def solve_and_forward(name):
    """Backward error of every iteration on the restatement's own weights, forward error of the device's chain, and the one-call
    chain against the staged calls.  The compensated numpy filter costs K x channels x frames two-sums a bin: at 64 channels it is
    evaluated on every second bin (0, 2, .. 32); G and the flags of every bin are checked, and so is every bin's X by the forward
    error."""
    from egregora_amd import wpe_engine
    c = wpe_cases.CASES[name]
    Y = spectra(name)
    Y128 = Y.astype(np.complex128)
    X128, col = chain128(name)
    Yd = dev(Y)
    nf = lambda a: np.linalg.norm(a, axis=(1, 2))
    sel = slice(None, None, 2 if c["channels"] >= 64 else 1)
    for it, (inv, R, P, _, ok) in enumerate(col):
        assert ok.all()
        out = wpe_engine.iterate(Yd, dev(inv), c["taps"], c["delay"], want_x=True, want_g=True, want_inv=True)
        flags = out["flags"].cpu().numpy()
        assert flags.sum() == 0, f"guard fired in {int(flags.sum())} of {len(flags)} bins"
        G = out["G"].cpu().numpy()
        res = nf(R @ G - P) / (nf(R) * nf(G) + nf(P))
        Xn = wn.apply_filter_compensated(Y128[sel], G[sel], c["taps"], c["delay"])
        xe = wn.rel_rms(out["X"].cpu().numpy()[sel], Xn)
        inv_n = wn.psd_inverse(Xn)
        ie = float(np.max(np.abs(out["inv"].cpu().numpy()[sel] - inv_n) / inv_n))
        print(f"case {name} iteration {it}: backward error max {res.max():.2e} (bar 1e-11), X {xe:.2e} (bar 2e-7), "
              f"next weights {ie:.2e} (bar 1e-12)")
        assert res.max() <= 1e-11, res.max()
        assert xe <= 2e-7, xe
        assert ie <= 1e-12, ie
    forward_error(name)
    xd = dev(wpe_cases.case_signal(name))
    args = (c["n_fft"], c["hop"], c["taps"], c["delay"], c["iterations"])
    Ys, inv, Xs = wpe_engine.stft(xd, c["n_fft"], c["hop"]), None, None
    for it in range(c["iterations"]):
        last = it == c["iterations"] - 1
        out = wpe_engine.iterate(Ys, inv, c["taps"], c["delay"], want_x=last, want_g=False, want_inv=not last)
        inv, Xs = out.get("inv"), out.get("X")
    staged = wpe_engine.istft(Xs, c["n_fft"], c["hop"])
    whole = wpe_engine.dereverb(xd, *args)
    assert torch.equal(staged, whole) and torch.equal(whole, wpe_engine.dereverb(xd, *args))


def forward_error(name):
    """The device's own chain of iterations against the complex128 restatement."""
    from egregora_amd import wpe_engine
    c = wpe_cases.CASES[name]
    Y = spectra(name)
    X128, _ = chain128(name)
    Yd = dev(Y)
    bar = max(2e-7, wn.rel_rms(wn.wpe(Y, c["taps"], c["delay"], c["iterations"]), X128))
    inv, X = None, None
    for it in range(c["iterations"]):
        last = it == c["iterations"] - 1
        out = wpe_engine.iterate(Yd, inv, c["taps"], c["delay"], want_x=last, want_g=False, want_inv=not last)
        assert int(out["flags"].sum()) == 0
        inv, X = out.get("inv"), out.get("X")
    err = wn.rel_rms(X.cpu().numpy(), X128)
    print(f"case {name}: forward error {err:.2e}, bar {bar:.2e}, ratio {err / bar:.2f}")
    assert err <= bar, (err, bar)


@pytest.mark.parametrize("name", ["H", "F", "G", "L"])
def test_solve_and_forward_error_wide(pack, name):
    solve_and_forward(name)


def test_lds_refusal_enqueues_nothing(pack):
    """64 channels, one tap, delay 128: delay + taps - 1 = 128 is inside WPE_MAX_HIST, the tile of 64 x 160 frames is not inside LDS."""
    from egregora_amd import native, wpe_engine
    x = dev(wpe_cases.signal(64, 2000, 9))
    Yd = wpe_engine.stft(x, 64, 16)
    wpe_engine.iterate(Yd, None, 1, 122, want_x=True)                      # (the same shapes one step inside the limit)
    with pytest.raises(RuntimeError, match=r"bytes of LDS needed \(limit 163840\)"):
        wpe_engine.iterate(Yd, None, 1, 128, want_x=True)
    # the one-call chain: its workspace keeps the pattern written here, so not even the analysis was enqueued
    nbytes = int(native.lib().egr_wpe_workspace_bytes(64, 2000, 64, 16, 1))
    ws = wpe_engine.workspace(x.device, nbytes)
    ws.fill_(0xA5)
    with pytest.raises(RuntimeError, match=r"bytes of LDS needed \(limit 163840\)"):
        wpe_engine.dereverb(x, 64, 16, 1, 128, 1)
    torch.cuda.synchronize()
    assert wpe_engine.workspace(x.device, nbytes) is ws and bool((ws == 0xA5).all())
    forward_error("H")


def test_node_32_channels(enhance_pack):
    c = wpe_cases.CASES["F"]
    node = enhance_pack.NODE_CLASS_MAPPINGS["Egregora_WPE_Dereverb"]()
    x = wpe_cases.case_signal("F")
    T = c["n"]
    args = (c["taps"], c["delay"], c["iterations"], c["n_fft"], c["hop"])
    (out,) = node.execute({"waveform": torch.from_numpy(x)[None], "sample_rate": wpe_cases.SR}, *args, True)
    y = out["waveform"]
    assert tuple(y.shape) == (1, 32, wn.out_length(T, c["n_fft"], c["hop"])) and y.dtype == torch.float32 and not y.is_cuda
    assert out["meta"]["wpe"] == dict(zip(("taps", "delay", "iterations", "n_fft", "hop"), args))
    y = y.numpy()[0]
    ref = wn.dereverb(x, c["n_fft"], c["hop"], c["taps"], c["delay"], c["iterations"])
    bar = max(1e-6, 4 * wn.rel_rms(wn.dereverb(x, c["n_fft"], c["hop"], c["taps"], c["delay"], c["iterations"], np.float32), ref))
    err = wn.rel_rms(y, ref)
    change = wn.rel_rms(y[:, :T], x)
    print(f"node F: device {err:.2e}, bar {bar:.2e}, ratio {err / bar:.2f}, change against the input {change:.3f}")
    assert err <= bar, (err, bar)
    assert change > 0.1, change
