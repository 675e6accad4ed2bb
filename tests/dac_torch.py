"""Plain-PyTorch restatement of the Descript Audio Codec forward pass (SPEC.md 4e, UPSTREAM-RECALL) in float32 or float64: weight-norm
fold, snake, residual units, encoder, residual vector quantiser, decoder, with every block output kept as a stage.

It is written in upstream's own [rows, C, L] shapes (not the device's channels-last layout) and is the yardstick of
tests/test_gpu_dac.py.  It also builds the synthetic checkpoints the tests use (the real ones are not in the test images): a seeded
random state dict in the UPSTREAM key layout (weight_g / weight_v / bias per conv, alpha [1, C, 1] per snake, codebook.weight), scaled
so that every stage's rms stays in [0.1, 10] in float64 (tests/test_dac_host.py asserts it), snake alpha uniform in [0.5, 2].
"""
from pathlib import Path

import torch
import torch.nn.functional as F

DEFAULT = dict(encoder_dim=64, encoder_rates=[2, 4, 8, 8], latent_dim=None, decoder_dim=1536, decoder_rates=[8, 8, 4, 2], n_codebooks=9,
               codebook_size=1024, codebook_dim=8, sample_rate=44100)
_SMALL = dict(encoder_dim=16, latent_dim=64, decoder_dim=64, n_codebooks=3, codebook_size=64, codebook_dim=8, sample_rate=44100)
# the smallest shapes at which each code path can still go wrong: S pads (1003 is no multiple of the hop 8), O has odd strides
# (a transposed conv gives L s - 1), W runs the 44 kHz widths (up to 1536 channels) on 8 frames, G takes the general paths: no Cin
# is a multiple of 16 (fp32 MFMA contractions, K tails), widths 6 / 10 / 5 are no multiple of 4 (the snake's scalar branch) and
# codebook_dim is 5 (the quantiser's generic instantiation).  T and C are the quantiser's limits: T's codebook (1024 x 16 floats) plus
# eight frames of its 2048-wide latent is 197 KiB, so the quantiser takes four frames a workgroup (131.6 KiB), and codebook_dim 16
# is two passes of its projection loop; C has fewer codes (20) than the 32 lanes of a frame, a ragged second projection pass
# (codebook_dim 12), a latent narrower than 32 and no Cin that is a multiple of 16 but the decoder's first
CONFIGS = {"S": dict(_SMALL, encoder_rates=[2, 4], decoder_rates=[4, 2]), "O": dict(_SMALL, encoder_rates=[2, 5], decoder_rates=[5, 2]),
           "W": dict(DEFAULT),
           "G": dict(encoder_dim=6, encoder_rates=[2, 3], latent_dim=20, decoder_dim=20, decoder_rates=[3, 2], n_codebooks=2, codebook_size=48,
                     codebook_dim=5, sample_rate=44100),
           "T": dict(encoder_dim=4, encoder_rates=[2], latent_dim=2048, decoder_dim=8, decoder_rates=[2], n_codebooks=2, codebook_size=1024,
                     codebook_dim=16, sample_rate=44100),
           "C": dict(encoder_dim=8, encoder_rates=[2, 2], latent_dim=24, decoder_dim=16, decoder_rates=[2, 2], n_codebooks=3, codebook_size=20,
                     codebook_dim=12, sample_rate=44100)}
LENGTHS = {"S": 1003, "O": 1003, "W": 4091, "G": 601, "T": 301, "C": 515}
ROWS = 2
DILATIONS = (1, 3, 9)
UNIT_GAIN = 0.3          # row norm of a residual unit's k = 1 conv and of the quantiser's out_proj: keeps the sums from growing


def config(name: str) -> dict:
    c = dict(CONFIGS[name])
    if c["latent_dim"] is None:
        c["latent_dim"] = c["encoder_dim"] * 2 ** len(c["encoder_rates"])
    return c


def hop(cfg) -> int:
    h = 1
    for s in cfg["encoder_rates"]:
        h *= s
    return h


# ------------------------------------------------------------------------------------------------ synthetic checkpoints
def synthetic_state_dict(cfg: dict, seed: int) -> dict:
    """Upstream key layout (DAC-P5 / P6 / P8).  weight_g is the row norm of the folded weight, chosen per layer class for a gain near 1."""
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def conv(name, co, ci, k, gain=1.0):
        sd[name + ".weight_v"] = torch.randn(co, ci, k, generator=g)
        sd[name + ".weight_g"] = gain * (0.8 + 0.4 * torch.rand(co, 1, 1, generator=g))
        sd[name + ".bias"] = 0.05 * torch.randn(co, generator=g)

    def convtr(name, ci, co, k, gain):
        sd[name + ".weight_v"] = torch.randn(ci, co, k, generator=g)
        sd[name + ".weight_g"] = gain * (0.8 + 0.4 * torch.rand(ci, 1, 1, generator=g))
        sd[name + ".bias"] = 0.05 * torch.randn(co, generator=g)

    def alpha(name, c):
        sd[name] = 0.5 + 1.5 * torch.rand(1, c, 1, generator=g)

    def unit(prefix, c):
        alpha(prefix + ".block.0.alpha", c)
        conv(prefix + ".block.1", c, c, 7, 0.7)
        alpha(prefix + ".block.2.alpha", c)
        conv(prefix + ".block.3", c, c, 1, UNIT_GAIN)

    ne, nd = len(cfg["encoder_rates"]), len(cfg["decoder_rates"])
    c = cfg["encoder_dim"]
    conv("encoder.block.0", c, 1, 7, 3.0)
    for i, s in enumerate(cfg["encoder_rates"], start=1):
        for j in range(3):
            unit(f"encoder.block.{i}.block.{j}", c)
        alpha(f"encoder.block.{i}.block.3.alpha", c)
        conv(f"encoder.block.{i}.block.4", 2 * c, c, 2 * s, 0.8)
        c *= 2
    alpha(f"encoder.block.{ne + 1}.alpha", c)
    conv(f"encoder.block.{ne + 2}", cfg["latent_dim"], c, 3, 1.0)
    for q in range(cfg["n_codebooks"]):
        p = f"quantizer.quantizers.{q}"
        conv(p + ".in_proj", cfg["codebook_dim"], cfg["latent_dim"], 1)
        sd[p + ".codebook.weight"] = torch.randn(cfg["codebook_size"], cfg["codebook_dim"], generator=g)
        conv(p + ".out_proj", cfg["latent_dim"], cfg["codebook_dim"], 1, UNIT_GAIN / cfg["codebook_dim"] ** 0.5)
    c = cfg["decoder_dim"]
    conv("decoder.model.0", c, cfg["latent_dim"], 7, 1.0)
    for i, s in enumerate(cfg["decoder_rates"], start=1):
        alpha(f"decoder.model.{i}.block.0.alpha", c)
        convtr(f"decoder.model.{i}.block.1", c, c // 2, 2 * s, 0.8 * (s / 2.0) ** 0.5)
        c //= 2
        for j in range(3):
            unit(f"decoder.model.{i}.block.{j + 2}", c)
    alpha(f"decoder.model.{nd + 1}.alpha", c)
    conv(f"decoder.model.{nd + 2}", 1, c, 7, 2.0)
    return sd


def write_checkpoint(path: Path, cfg: dict, sd: dict):
    """One torch.save file as upstream writes it (DAC-P1): state_dict + metadata.kwargs."""
    kwargs = {k: cfg[k] for k in DEFAULT}
    torch.save({"state_dict": sd, "metadata": {"kwargs": kwargs}}, str(path))


# ------------------------------------------------------------------------------------------------ forward
def fold(sd, name):
    """DAC-P2 in float64, rounded to fp32 once (the values the device holds)."""
    v, g = sd[name + ".weight_v"].double(), sd[name + ".weight_g"].double()
    nrm = v.flatten(1).norm(dim=1).reshape(-1, 1, 1)
    return (g * v / nrm).float()


class Net:
    """The folded weights at one dtype."""

    def __init__(self, sd: dict, cfg: dict, dtype):
        self.cfg, self.dtype = cfg, dtype
        self.t = {}
        for k in sd:
            if k.endswith(".weight_v"):
                n = k[:-len(".weight_v")]
                self.t[n + ".w"] = fold(sd, n).to(dtype)
                self.t[n + ".b"] = sd[n + ".bias"].float().to(dtype)
            elif k.endswith(".alpha") or k.endswith("codebook.weight"):
                self.t[k] = sd[k].float().to(dtype)

    def conv(self, x, name, stride=1, dil=1, pad=0):
        return F.conv1d(x, self.t[name + ".w"], self.t[name + ".b"], stride=stride, dilation=dil, padding=pad)

    def snake(self, x, name):
        a = self.t[name]
        return x + (a + 1e-9).reciprocal() * torch.sin(a * x).pow(2)

    def unit(self, x, prefix, d):
        y = self.conv(self.snake(x, prefix + ".block.0.alpha"), prefix + ".block.1", dil=d, pad=3 * d)
        y = self.conv(self.snake(y, prefix + ".block.2.alpha"), prefix + ".block.3")
        assert y.shape[-1] == x.shape[-1]                    # DAC-P4: upstream's centre crop never fires
        return x + y

    def encode_stages(self, x):
        """x [rows, n] -> [input conv, block 1 .. n_enc, ze], each [rows, C, L]."""
        cfg = self.cfg
        h = hop(cfg)
        n = x.shape[-1]
        x = F.pad(x.to(self.dtype), (0, -(-n // h) * h - n)).unsqueeze(1)
        out = [self.conv(x, "encoder.block.0", pad=3)]
        for i, s in enumerate(cfg["encoder_rates"], start=1):
            y = out[-1]
            for j, d in enumerate(DILATIONS):
                y = self.unit(y, f"encoder.block.{i}.block.{j}", d)
            y = self.snake(y, f"encoder.block.{i}.block.3.alpha")
            out.append(self.conv(y, f"encoder.block.{i}.block.4", stride=s, pad=-(-s // 2)))
        ne = len(cfg["encoder_rates"])
        out.append(self.conv(self.snake(out[-1], f"encoder.block.{ne + 1}.alpha"), f"encoder.block.{ne + 2}", pad=1))
        return out

    def similarities(self, r, q):
        """r [rows, latent, F] -> cosine similarities [rows, F, K] of quantiser stage q (DAC-P8)."""
        p = f"quantizer.quantizers.{q}"
        e = self.conv(r, p + ".in_proj").transpose(1, 2)                       # [rows, F, cd]
        cb = self.t[p + ".codebook.weight"]
        eh = e / e.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        ch = cb / cb.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        return eh @ ch.t()

    def dequantize_stage(self, codes_q, q):
        """codes_q [rows, F] -> out_proj(codebook row) [rows, latent, F]."""
        p = f"quantizer.quantizers.{q}"
        c = self.t[p + ".codebook.weight"][codes_q].transpose(1, 2)            # [rows, cd, F]
        return self.conv(c, p + ".out_proj")

    def quantize(self, ze, codes=None):
        """ze [rows, latent, F] -> (z, codes [rows, n_codebooks, F], stage inputs, similarities per stage).  With `codes` given the
        search is skipped and z is the arithmetic of those codes.  torch.argmax returns the first maximum: the lowest index wins ties."""
        r = ze.to(self.dtype)
        z = torch.zeros_like(r)
        out_codes, ins, sims = [], [], []
        for q in range(self.cfg["n_codebooks"]):
            ins.append(r)
            s = self.similarities(r, q)
            sims.append(s)
            cq = codes[:, q] if codes is not None else torch.argmax(s, dim=-1)
            out_codes.append(cq)
            zq = self.dequantize_stage(cq, q)
            z = z + zq
            r = r - zq
        return z, torch.stack(out_codes, dim=1), ins, sims

    def decode_stages(self, z):
        """z [rows, latent, F] -> ([input conv, block 1 .. n_dec], y [rows, n_decoded])."""
        cfg = self.cfg
        out = [self.conv(z.to(self.dtype), "decoder.model.0", pad=3)]
        for i, s in enumerate(cfg["decoder_rates"], start=1):
            y = self.snake(out[-1], f"decoder.model.{i}.block.0.alpha")
            n = f"decoder.model.{i}.block.1"
            y = F.conv_transpose1d(y, self.t[n + ".w"], self.t[n + ".b"], stride=s, padding=-(-s // 2))
            for j, d in enumerate(DILATIONS):
                y = self.unit(y, f"decoder.model.{i}.block.{j + 2}", d)
            out.append(y)
        nd = len(cfg["decoder_rates"])
        y = torch.tanh(self.conv(self.snake(out[-1], f"decoder.model.{nd + 1}.alpha"), f"decoder.model.{nd + 2}", pad=3))
        return out, y.squeeze(1)


def test_signal(rows: int, n: int, seed: int) -> torch.Tensor:
    """A few tones plus noise at about -12 dBFS, float32 [rows, n]."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64) / 44100.0
    x = torch.stack([0.2 * torch.sin(2 * torch.pi * (220.0 * (r + 1)) * t) + 0.1 * torch.sin(2 * torch.pi * 3100.0 * t + r) for r in range(rows)])
    return (x + 0.1 * torch.randn(rows, n, generator=g, dtype=torch.float64)).float()


def quantiser_input(cfg: dict, rows: int, frames: int, seed: int) -> torch.Tensor:
    """A synthetic encoder output for the quantiser-alone tests (the encoder of 2 000 frames would take the CPU restatement minutes):
    unit-rms noise with a slow envelope, float64 rounded to fp32, [rows, latent, frames]."""
    g = torch.Generator().manual_seed(seed)
    ze = torch.randn(rows, cfg["latent_dim"], frames, generator=g, dtype=torch.float64)
    env = 0.5 + torch.rand(rows, 1, frames, generator=g, dtype=torch.float64)
    return (ze * env).float()


def rms(t) -> float:
    return float(t.double().pow(2).mean().sqrt())
