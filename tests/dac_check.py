"""Gates and quantiser statistics of the native Descript Audio Codec (csrc/egr_dac.hip) against tests/dac_torch.py, shared by
tests/test_dac_host.py and tests/test_gpu_dac.py.

Continuous quantities: relative rms against float64 <= 1.5 x the torch-fp32 restatement's + 3e-7 and <= 1e-4;
max-abs (over the reference's rms, as dfn3_check.maxrel) <= 3 x torch-fp32's + 3e-7.

Codes: a discrete choice cannot be gated on a norm.  tau = 4 x the largest |similarity(torch-fp32) - similarity(float64)| over the
same queries is measured from the restatement alone (the factor 4 covers another accumulation order); a device code must be within
tau of the best in float64, and must EQUAL float64's on every frame whose float64 margins (best minus second best) all exceed 2 tau.
"""
import functools

import torch

import dac_torch as R

FLOOR, CAP, RMS_X, MAX_X = 3e-7, 1e-4, 1.5, 3.0
TAU_X, MARGIN_CAP, MAX_EXCLUDED = 4.0, 1e-4, 0.05
VQ_ROWS, VQ_FRAMES = 2, 1000                # 2 000 frames for the quantiser-alone tests
SEED = 17


def rel(a, ref):
    a, ref = a.double().cpu().reshape(-1), ref.double().cpu().reshape(-1)
    return float((a - ref).norm() / max(float(ref.norm()), 1e-300))


def maxrel(a, ref):
    a, ref = a.double().cpu().reshape(-1), ref.double().cpu().reshape(-1)
    rms = float(ref.norm()) / max(ref.numel(), 1) ** 0.5
    return float((a - ref).abs().max()) / max(rms, 1e-300)


def gate(name, got, r64, r32):
    """Prints the four figures, then asserts both gates."""
    got = got.reshape(r64.shape)
    e, e32, m, m32 = rel(got, r64), rel(r32, r64), maxrel(got, r64), maxrel(r32, r64)
    print(f"  {name}: rms {e:.2e} (fp32 {e32:.2e})  max {m:.2e} (fp32 {m32:.2e})")
    assert e <= RMS_X * e32 + FLOOR and e <= CAP, (name, "rms", e, e32)
    assert m <= MAX_X * m32 + FLOOR, (name, "max", m, m32)
    return e, e32, m, m32


@functools.lru_cache(maxsize=None)
def model(name):
    """(cfg, state dict, float64 net, float32 net) of config `name`."""
    cfg = R.config(name)
    sd = R.synthetic_state_dict(cfg, SEED)
    return cfg, sd, R.Net(sd, cfg, torch.float64), R.Net(sd, cfg, torch.float32)


@functools.lru_cache(maxsize=None)
def forward(name):
    """The whole restatement of config `name` on its test signal, float64 and float32, computed once."""
    cfg, sd, n64, n32 = model(name)
    x = R.test_signal(R.ROWS, R.LENGTHS[name], 3)
    out = {"x": x}
    with torch.no_grad():
        for tag, net in (("64", n64), ("32", n32)):
            enc = net.encode_stages(x)
            z, codes, ins, sims = net.quantize(enc[-1])
            out["enc" + tag], out["z" + tag], out["codes" + tag], out["ins" + tag], out["sims" + tag] = enc, z, codes, ins, sims
        # the decoder is judged from one input: the float64 z rounded to fp32
        zin = out["z64"].float()
        out["zin"] = zin
        for tag, net in (("64", n64), ("32", n32)):
            out["dec" + tag], out["y" + tag] = net.decode_stages(zin)
    return out


@functools.lru_cache(maxsize=None)
def vq_case(name):
    """The quantiser alone on 2 000 synthetic frames: float64 codes, stage inputs, margins, and tau."""
    cfg, sd, n64, n32 = model(name)
    ze = R.quantiser_input(cfg, VQ_ROWS, VQ_FRAMES, 5)
    with torch.no_grad():
        z64, codes64, ins64, sims64 = n64.quantize(ze)
        tau = 0.0
        for q in range(cfg["n_codebooks"]):
            r = ins64[q].float()                                # the same queries for both precisions
            tau = max(tau, float((n32.similarities(r, q).double() - n64.similarities(r.double(), q)).abs().max()))
    return {"ze": ze, "z64": z64, "codes64": codes64, "margins": margins(sims64), "tau": TAU_X * tau}


def margins(sims):
    """[rows, n_codebooks, F]: best minus second-best similarity per stage and frame."""
    out = []
    for s in sims:
        top = s.topk(2, dim=-1).values
        out.append(top[..., 0] - top[..., 1])
    return torch.stack(out, dim=1)


def safe_frames(marg, thr):
    """[rows, F] bool: every stage's margin exceeds thr."""
    return (marg > thr).all(dim=1)


def e2e_tau(name):
    """tau of the end-to-end encode: as vq_case's, with each precision on its own encoder output and residuals, over the frames whose
    two code paths still agree when the stage begins."""
    f = forward(name)
    agree = torch.ones_like(f["codes64"][:, 0], dtype=torch.bool)
    tau = 0.0
    for q in range(f["codes64"].shape[1]):
        d = (f["sims32"][q].double() - f["sims64"][q]).abs().amax(dim=-1)
        if agree.any():
            tau = max(tau, float(d[agree].max()))
        agree &= f["codes32"][:, q] == f["codes64"][:, q]
    return TAU_X * tau


def cl(t):
    """[rows, C, L] -> channels-last [rows, L, C] (the device's stage layout)."""
    return t.transpose(1, 2)
