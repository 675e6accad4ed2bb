"""Gates and quantiser statistics of the native Descript Audio Codec (csrc/egr_dac.hip) against tests/dac_torch.py, shared by
tests/test_dac_host.py, tests/test_gpu_dac.py and tests/test_gpu_dac_configs.py.

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
VQ_RAGGED = (3, 667)                        # 2 001 frames: one more than a multiple of the quantiser's 4 and 8 frames a workgroup
SEED = 17
LEVELS = (1.0, 2.0 ** -10)                  # tests/test_gpu_dac_configs.py: a row at the usual level and one 60 dB below it
LEVELS_CASE = ("S", 1003, 2, 3, LEVELS)     # forward's arguments
REUSE_LENGTHS = (4099, 9)
TIE_PAIRS = ((3, 17), (0, 19))              # (kept, duplicate) codebook rows of tie_case


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


def forward(name, n=None, rows=None, seed=3, levels=None):
    """The whole restatement of config `name` on its test signal, float64 and float32, computed once per argument tuple.  n, rows:
    the signal's length and row count (default: the config's own of dac_torch); levels: a factor per row, applied to the signal and
    again to the decoder's input."""
    return _forward(name, R.LENGTHS[name] if n is None else int(n), R.ROWS if rows is None else int(rows), int(seed),
                    None if levels is None else tuple(float(v) for v in levels))


@functools.lru_cache(maxsize=None)
def _forward(name, n, rows, seed, levels):
    cfg, sd, n64, n32 = model(name)
    x = R.test_signal(rows, n, seed)
    lv = None if levels is None else torch.tensor(levels, dtype=torch.float32)          # (powers of two in the tests: exact)
    if lv is not None:
        x = x * lv[:, None]
    out = {"x": x}
    with torch.no_grad():
        for tag, net in (("64", n64), ("32", n32)):
            enc = net.encode_stages(x)
            z, codes, ins, sims = net.quantize(enc[-1])
            out["enc" + tag], out["z" + tag], out["codes" + tag], out["ins" + tag], out["sims" + tag] = enc, z, codes, ins, sims
        # the decoder is judged from one input: the float64 z rounded to fp32
        zin = out["z64"].float()
        if lv is not None:
            zin = zin * lv[:, None, None]
        out["zin"] = zin
        for tag, net in (("64", n64), ("32", n32)):
            out["dec" + tag], out["y" + tag] = net.decode_stages(zin)
    return out


def vq_case(name, rows=VQ_ROWS, frames=VQ_FRAMES, seed=5):
    """The quantiser alone on rows x frames synthetic frames (2 000 by default): float64 codes, stage inputs, margins, and tau."""
    return _vq_case(name, int(rows), int(frames), int(seed))


def vq_tau(n64, n32, ins64):
    """4 x the largest |similarity(torch-fp32) - similarity(float64)| over the float64 path's stage inputs, rounded to fp32."""
    tau = 0.0
    for q, r64 in enumerate(ins64):
        r = r64.float()                                         # the same queries for both precisions
        tau = max(tau, float((n32.similarities(r, q).double() - n64.similarities(r.double(), q)).abs().max()))
    return TAU_X * tau


@functools.lru_cache(maxsize=None)
def _vq_case(name, rows, frames, seed):
    cfg, sd, n64, n32 = model(name)
    ze = R.quantiser_input(cfg, rows, frames, seed)
    with torch.no_grad():
        z64, codes64, ins64, sims64 = n64.quantize(ze)
        tau = vq_tau(n64, n32, ins64)
    return {"ze": ze, "z64": z64, "codes64": codes64, "margins": margins(sims64), "tau": tau}


def edge_cases():
    """(config, n, rows, signal seed) of the length and row edges: one sample, hop - 1, hop, hop + 1 at 1 and 3 rows, and S at 1024
    samples (its levels are then 1024, 512 and 128 long: multiples of 128).  Below 20 frames the 5 % cap leaves no frame out, so
    the seed is one at which every float64 margin exceeds 2 tau (tests/test_dac_host.py asserts it); 3 serves for all of them."""
    out = []
    for name in ("S", "O", "G"):
        h = R.hop(R.config(name))
        out += [(name, n, rows, 3) for n in (1, h - 1, h, h + 1) for rows in (1, 3)]
    return out + [("S", 1024, 2, 3)]


@functools.lru_cache(maxsize=None)
def tie_case():
    """Config C with exact ties: in every codebook row 17 is a copy of row 3 and row 19 of row 0.  The float64 path is the lowest-
    index rule itself (the duplicates are masked out of its search, so that no rounding of a matrix product can prefer one), its
    margins are those between DIFFERENT rows."""
    cfg, sd, _, _ = model("C")
    sd = dict(sd)
    for q in range(cfg["n_codebooks"]):
        k = f"quantizer.quantizers.{q}.codebook.weight"
        cb = sd[k].clone()
        for keep, dup in TIE_PAIRS:
            cb[dup] = cb[keep]
        sd[k] = cb
    n64, n32 = R.Net(sd, cfg, torch.float64), R.Net(sd, cfg, torch.float32)
    ze = R.quantiser_input(cfg, VQ_ROWS, VQ_FRAMES, 5)
    dups = [d for _, d in TIE_PAIRS]
    with torch.no_grad():
        r = ze.double()
        codes, ins, sims = [], [], []
        for q in range(cfg["n_codebooks"]):
            ins.append(r)
            s = n64.similarities(r, q)
            s[..., dups] = -float("inf")
            sims.append(s)
            codes.append(torch.argmax(s, dim=-1))
            r = r - n64.dequantize_stage(codes[-1], q)
        tau = vq_tau(n64, n32, ins)
    zero = dict(sd)
    zero["quantizer.quantizers.0.in_proj.bias"] = torch.zeros_like(sd["quantizer.quantizers.0.in_proj.bias"])
    return {"cfg": cfg, "sd": sd, "sd_zero_bias": zero, "ze": ze, "codes64": torch.stack(codes, dim=1), "margins": margins(sims), "tau": tau}


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


def e2e_tau(name, *args, **kw):
    """tau of the end-to-end encode: as vq_case's, with each precision on its own encoder output and residuals, over the frames whose
    two code paths still agree when the stage begins.  The arguments are forward's."""
    f = forward(name, *args, **kw)
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
