"""WPE dereverberation on the device (SPEC.md 4d; csrc/egr_wpe.hip) against the float64 restatement tests/wpe_numpy.py, on the inputs
of tests/wpe_cases.py whose conditioning tests/test_wpe_host.py pins.

Bars, and where they come from:
  transforms   relative rms of egr_wpe_stft against the float64 analysis <= 4 x the error of a float32 numpy.fft analysis of the same
               input (margin 4: another radix order); egr_wpe_istft(egr_wpe_stft(y)) = y within 2e-6 of the peak, same bits twice.
  solve        cases C, D, E (cond(R) up to 1e10): BACKWARD error only.  With R, P rebuilt in float64 from the very inputs the device
               gets, ||R G - P||_F <= 1e-11 (||R||_F ||G||_F + ||P||_F) in every bin; X against Y - G^H Ytilde evaluated in numpy
               from the device's own G within 2e-7 relative rms (complex64 rounding is 6e-8 per part); the next weights against
               WPE-P4 applied to that X within 1e-12 relative, element by element.  Where the prediction cancels the observation
               the terms of the sum are up to 1e4 times |X|, so a plain double evaluation of Y - G^H Ytilde is itself off by 1e-12
               to 1e-11 in 1 / |X|^2 (matmul against long double on C, D, E) and cannot referee a 1e-12 bar: the numpy side is
               wpe_numpy.apply_filter_compensated (exact products, two-sum; 4e-16 to 4e-15 against long double), and the kernel
               sums the same way (wpe_filter_sum).
  forward      cases A, B (cond(R) <= 1e4): relative rms of X against the complex128 restatement <= max(2e-7, the complex64
               restatement's own error): the device does strictly more in double than that path, so it gets no margin over it.
  node         samples against the float64 pipeline within max(1e-6, 4 x the float32 / complex64 numpy pipeline's error).
"""
import numpy as np
import pytest
import torch

import wpe_cases
import wpe_numpy as wn
from conftest import gjson

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_SPEC = {}


def spectra(name):
    """complex64 analysis of a case, computed once: the same bytes go to the device and to the restatement."""
    if name not in _SPEC:
        c = wpe_cases.CASES[name]
        _SPEC[name] = wn.analysis(wpe_cases.case_signal(name), c["n_fft"], c["hop"]).astype(np.complex64)
    return _SPEC[name]


_CHAIN = {}


def chain128(name):
    """The complex128 restatement on those bytes: final X and (inv, R, P, G, ok) per iteration."""
    if name not in _CHAIN:
        c = wpe_cases.CASES[name]
        col = []
        X = wn.wpe(spectra(name).astype(np.complex128), c["taps"], c["delay"], c["iterations"], col)
        _CHAIN[name] = (X, col)
    return _CHAIN[name]


def transform_inputs(name):
    if name == "big":
        return wpe_cases.signal(2, 20000, 77), 4096, 1024
    c = wpe_cases.CASES[name]
    return wpe_cases.case_signal(name), c["n_fft"], c["hop"]


@pytest.mark.parametrize("name", ["A", "E", "big"])
def test_transforms(pack, name):
    from egregora_amd import wpe_engine
    y, n_fft, hop = transform_inputs(name)
    T = y.shape[1]
    ref = wn.analysis(y, n_fft, hop)
    bar = 4 * wn.rel_rms(wn.analysis(y, n_fft, hop, np.float32), ref)
    Yd = wpe_engine.stft(dev(y), n_fft, hop)
    assert tuple(Yd.shape) == ref.shape
    err = wn.rel_rms(Yd.cpu().numpy(), ref)
    print(f"stft {name}: device {err:.2e}, bar {bar:.2e} (4 x float32 numpy)")
    assert err <= bar, (err, bar)
    z1 = wpe_engine.istft(Yd, n_fft, hop)
    z2 = wpe_engine.istft(wpe_engine.stft(dev(y), n_fft, hop), n_fft, hop)
    assert tuple(z1.shape) == (y.shape[0], wn.out_length(T, n_fft, hop)) and torch.equal(z1, z2)
    z = z1.cpu().numpy()
    peak = float(np.abs(y).max())
    rt = float(np.abs(z[:, :T] - y).max()) / peak
    print(f"round trip {name}: {rt:.2e} of the peak")
    assert rt <= 2e-6 and float(np.abs(z[:, T:]).max(initial=0.0)) <= 2e-6 * peak      # (the tail is empty where n_out = T)


@pytest.mark.parametrize("name", ["C", "D", "E"])
def test_solve_backward_error(pack, name):
    from egregora_amd import wpe_engine
    c = wpe_cases.CASES[name]
    Y = spectra(name)
    Y128 = Y.astype(np.complex128)
    Yd = dev(Y)
    nf = lambda a: np.linalg.norm(a, axis=(1, 2))
    for it, (inv, R, P, _, ok) in enumerate(chain128(name)[1]):
        assert ok.all()
        out = wpe_engine.iterate(Yd, dev(inv), c["taps"], c["delay"], want_x=True, want_g=True, want_inv=True)
        flags = out["flags"].cpu().numpy()
        assert flags.sum() == 0, f"guard fired in {int(flags.sum())} of {len(flags)} bins"
        G = out["G"].cpu().numpy()
        res = nf(R @ G - P) / (nf(R) * nf(G) + nf(P))
        Xn = wn.apply_filter_compensated(Y128, G, c["taps"], c["delay"])
        xe = wn.rel_rms(out["X"].cpu().numpy(), Xn)
        inv_n = wn.psd_inverse(Xn)
        ie = float(np.max(np.abs(out["inv"].cpu().numpy() - inv_n) / inv_n))
        print(f"case {name} iteration {it}: backward error max {res.max():.2e}, X {xe:.2e}, next weights {ie:.2e}")
        assert res.max() <= 1e-11, res.max()
        assert xe <= 2e-7, xe
        assert ie <= 1e-12, ie


@pytest.mark.parametrize("name", ["A", "B"])
def test_forward_error_well_conditioned(pack, name):
    from egregora_amd import wpe_engine
    c = wpe_cases.CASES[name]
    Y = spectra(name)
    X128, _ = chain128(name)
    bar = max(2e-7, wn.rel_rms(wn.wpe(Y, c["taps"], c["delay"], c["iterations"]), X128))
    Yd, inv, X = dev(Y), None, None
    for it in range(c["iterations"]):
        last = it == c["iterations"] - 1
        out = wpe_engine.iterate(Yd, inv, c["taps"], c["delay"], want_x=last, want_g=False, want_inv=not last)
        assert int(out["flags"].sum()) == 0
        inv, X = out.get("inv"), out.get("X")
    err = wn.rel_rms(X.cpu().numpy(), X128)
    print(f"case {name}: device {err:.2e}, bar {bar:.2e}")
    assert err <= bar, (err, bar)


def test_guard(pack):
    from egregora_amd import wpe_engine
    c = wpe_cases.CASES["A"]
    Y = spectra("A").copy()
    Y[7] = 0
    out = wpe_engine.iterate(dev(Y), None, c["taps"], c["delay"], want_x=True, want_g=True, want_inv=True)
    flags = out["flags"].cpu().numpy()
    X = out["X"].cpu().numpy()
    assert flags[7] == 1 and flags.sum() == 1
    assert X[7].tobytes() == Y[7].tobytes() and np.all(np.isfinite(X.view(np.float32))) and not np.any(out["G"].cpu().numpy()[7])
    assert wn.rel_rms(X[:7], Y[:7]) > 0.05                                # the other bins are filtered
    y = wpe_cases.signal(1, 300, 9)
    Ys = wpe_engine.stft(dev(y), 256, 64)
    assert Ys.shape[2] < 10
    out = wpe_engine.iterate(Ys, None, 10, 3, want_x=True, want_g=False, want_inv=True)
    assert int(out["flags"].sum()) == Ys.shape[0]
    assert out["X"].cpu().numpy().tobytes() == Ys.cpu().numpy().tobytes()
    z = wpe_engine.dereverb(dev(y), 256, 64, 10, 3, 3).cpu().numpy()
    assert np.all(np.isfinite(z)) and float(np.abs(z[:, :300] - y).max()) <= 2e-6 * float(np.abs(y).max())


@pytest.fixture(scope="module")
def enhance_pack(pack):
    """The package imported with EGREGORA_ENHANCE_NODES=1 (under a second alias: the session's `pack` was imported without it)."""
    import os
    from packload import load_pack
    old = os.environ.get("EGREGORA_ENHANCE_NODES")
    os.environ["EGREGORA_ENHANCE_NODES"] = "1"
    try:
        return load_pack("egregora_amd_enhance")
    finally:
        if old is None:
            del os.environ["EGREGORA_ENHANCE_NODES"]
        else:
            os.environ["EGREGORA_ENHANCE_NODES"] = old


@pytest.mark.parametrize("name", ["A", "B"])
def test_node_end_to_end(enhance_pack, name):
    c = wpe_cases.CASES[name]
    node = enhance_pack.NODE_CLASS_MAPPINGS["Egregora_WPE_Dereverb"]()
    x = np.stack([wpe_cases.case_signal(name), wpe_cases.signal(c["channels"], c["n"], c["seed"] + 50)])
    T = c["n"]
    args = (c["taps"], c["delay"], c["iterations"], c["n_fft"], c["hop"])
    audio = {"waveform": torch.from_numpy(x), "sample_rate": wpe_cases.SR, "meta": {"k": 1}}
    (out,) = node.execute(audio, *args, True)
    y = out["waveform"]
    assert tuple(y.shape) == (2, c["channels"], wn.out_length(T, c["n_fft"], c["hop"])) and y.dtype == torch.float32 and not y.is_cuda
    g = gjson("g16_wpe_surface")["passthrough"]
    assert out["sample_rate"] == wpe_cases.SR and sorted(out.keys()) == g["keys"] and sorted(out["meta"].keys()) == g["meta_keys"]
    assert out["meta"]["wpe"] == dict(zip(("taps", "delay", "iterations", "n_fft", "hop"), args))
    assert sorted(out["meta"]["wpe"]) == sorted(g["wpe_meta"])
    y = y.numpy()
    for b in range(2):
        ref = wn.dereverb(x[b], c["n_fft"], c["hop"], c["taps"], c["delay"], c["iterations"])
        bar = max(1e-6, 4 * wn.rel_rms(wn.dereverb(x[b], c["n_fft"], c["hop"], c["taps"], c["delay"], c["iterations"], np.float32), ref))
        err = wn.rel_rms(y[b], ref)
        change = wn.rel_rms(y[b][:, :T], x[b])
        print(f"node {name}[{b}]: device {err:.2e}, bar {bar:.2e}, change against the input {change:.3f}")
        assert err <= bar, (err, bar)
        assert change > 0.1, change
    (out64,) = node.execute(audio, *args, False)
    assert out64["waveform"].numpy().tobytes() == y.tobytes()
    (same,) = node.execute(audio, c["taps"], c["delay"], c["iterations"], 1024, 192, True)
    assert same["waveform"].numpy().tobytes() == x.tobytes()


def test_dereverb_equals_staged_calls(pack):
    from egregora_amd import wpe_engine
    c = wpe_cases.CASES["B"]
    xd = dev(wpe_cases.case_signal("B"))
    Yd, inv, X = wpe_engine.stft(xd, c["n_fft"], c["hop"]), None, None
    for it in range(c["iterations"]):
        last = it == c["iterations"] - 1
        out = wpe_engine.iterate(Yd, inv, c["taps"], c["delay"], want_x=last, want_g=False, want_inv=not last)
        inv, X = out.get("inv"), out.get("X")
    staged = wpe_engine.istft(X, c["n_fft"], c["hop"])
    whole = wpe_engine.dereverb(xd, c["n_fft"], c["hop"], c["taps"], c["delay"], c["iterations"])
    assert torch.equal(staged, whole) and torch.equal(whole, wpe_engine.dereverb(xd, c["n_fft"], c["hop"], c["taps"], c["delay"], c["iterations"]))
