"""Descript Audio Codec (SPEC.md 4e), everything that needs no device: opt-in registration and the node surface against fixture G17
(captured from the reference by tests/golden/make_golden_dac.py), the exported symbols, the length rules (egr_dac_lengths, its Python
twin and the restatement's shapes), the checkpoint loader (weight-norm fold, layer table from shapes, refusals), discovery order, the
level of the synthetic models, and the tie statistics the GPU tests' code comparisons rest on: for every input of
tests/test_gpu_dac.py and tests/test_gpu_dac_configs.py, float64 alone stays inside the caps those tests apply."""
import ctypes
import json
import os
import re
import subprocess
import sys
from pathlib import Path

import pytest
import torch

import dac_check as K
import dac_torch as R
from conftest import gjson

ROOT = Path(__file__).resolve().parent.parent
KEYS = ["Egregora_DAC_Decode", "Egregora_DAC_Encode"]
SYMBOLS = ["egr_dac_create", "egr_dac_decode", "egr_dac_destroy", "egr_dac_encode", "egr_dac_lengths", "egr_dac_quantize", "egr_dac_set_stages",
           "egr_dac_stage", "egr_dac_workspace_bytes"]

_DUMP = """
import inspect, json, sys
sys.path.insert(0, %r)
from packload import load_pack
p = load_pack()
out = {"keys": sorted(p.NODE_CLASS_MAPPINGS), "display_keys": sorted(p.NODE_DISPLAY_NAME_MAPPINGS), "surface": {}}
for k in %r:
    if k in p.NODE_CLASS_MAPPINGS:
        c = p.NODE_CLASS_MAPPINGS[k]
        it = c.INPUT_TYPES()
        out["surface"][k] = {"INPUT_TYPES": it, "widget_order": {a: list(v.keys()) for a, v in it.items()},
                             "RETURN_TYPES": list(c.RETURN_TYPES), "RETURN_NAMES": list(getattr(c, "RETURN_NAMES", ())), "FUNCTION": c.FUNCTION,
                             "CATEGORY": c.CATEGORY, "signature": str(inspect.signature(getattr(c, c.FUNCTION))),
                             "display": p.NODE_DISPLAY_NAME_MAPPINGS[k], "class_name": c.__name__}
print("DUMP" + json.dumps(out))
"""


def _import_in_child(flag):
    env = {k: v for k, v in os.environ.items() if k not in ("EGREGORA_ENHANCE_NODES", "EGREGORA_EVAL_NODES", "EGREGORA_CODEC_NODES")}
    if flag is not None:
        env["EGREGORA_CODEC_NODES"] = flag
    args = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", _DUMP % (str(ROOT), KEYS)]
    r = subprocess.run(args, env=env, cwd=str(ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("DUMP")][-1]
    return json.loads(line[4:])


def test_registration_is_opt_in_and_surface_equals_reference():
    g = gjson("g17_dac_surface")
    base = _import_in_child(None)
    assert not set(KEYS) & set(base["keys"]) and not set(KEYS) & set(base["display_keys"])
    assert _import_in_child("0")["keys"] == base["keys"]                  # only "1" switches the nodes on
    on = _import_in_child("1")
    assert sorted(set(on["keys"]) - set(base["keys"])) == KEYS and on["keys"] == on["display_keys"]
    for k in KEYS:
        assert on["surface"][k] == json.loads(json.dumps(g["surface"][k])), k


def test_symbols_are_declared_exported_and_bound(pack):
    from egregora_amd import native
    txt = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "egregora_amd.h").read_text(), flags=re.S)
    declared = sorted(s for s in set(re.findall(r"\b(egr_[a-z0-9_]+)\s*\(", txt)) if s.startswith("egr_dac_"))
    assert declared == SYMBOLS
    lib = ctypes.CDLL(str(native.LIB_PATH))
    for s in SYMBOLS:
        assert hasattr(lib, s) and s in native.SIGNATURES, s
    assert native.lib().egr_abi_version() == native.ABI_VERSION == 5
    assert ctypes.sizeof(native.DacConfigC) == 4 * (4 + 8 + 2 + 8 + 4)


@pytest.mark.parametrize("name", ["S", "O", "W", "G", "T", "C"])
def test_lengths_agree(pack, name):
    """DAC-P7: egr_dac_lengths == dac_engine.lengths == the restatement's shapes, at the hop's edges and at the test length."""
    from egregora_amd import dac_engine
    cfg, sd, n64, n32 = K.model(name)
    h = R.hop(cfg)
    odd = any(s % 2 for s in cfg["decoder_rates"])
    for n in (1, h - 1, h, h + 1, R.LENGTHS[name]):
        got = dac_engine.lengths(cfg, n)
        assert got == dac_engine.lengths_c(cfg, n), n
        n_pad, frames, n_dec = got
        assert n_pad == -(-n // h) * h and frames == n_pad // h
        with torch.no_grad():
            enc = n32.encode_stages(torch.zeros(1, n))
            dec, y = n32.decode_stages(torch.zeros(1, cfg["latent_dim"], frames))
        assert enc[0].shape[-1] == n_pad and enc[-1].shape == (1, cfg["latent_dim"], frames) and y.shape == (1, n_dec), n
        assert (n_dec < n_pad) == odd                                     # an odd stride makes a transposed conv give L s - 1


def test_weight_norm_fold_equals_torch(pack):
    """DAC-P2 for both conv kinds: axis 0 is the output channel of a Conv1d and the INPUT channel of a ConvTranspose1d."""
    from egregora_amd import dac_weights
    g = torch.Generator().manual_seed(2)
    for shape in ((12, 5, 7), (6, 9, 4)):                                 # Conv1d [out, in, k]; ConvTranspose1d [in, out, k]
        v, gg = torch.randn(*shape, generator=g), 0.5 + torch.rand(shape[0], 1, 1, generator=g)
        want = torch._weight_norm(v.double(), gg.double(), 0)
        got = dac_weights.fold_weight_norm(gg, v)
        assert got.dtype == torch.float32 and torch.equal(got, want.float())
        assert torch.allclose(got.double().flatten(1).norm(dim=1), gg.double().flatten(), rtol=1e-6)
        assert torch.equal(got, R.fold({"a.weight_v": v, "a.weight_g": gg}, "a"))


@pytest.mark.parametrize("name", ["S", "O", "W", "G", "T", "C"])
def test_layer_table_from_shapes_and_pack(pack, tmp_path, name):
    from egregora_amd import dac_weights
    cfg, sd, n64, n32 = K.model(name)
    lt = dac_weights.layer_table(sd)
    assert lt == {k: cfg[k] for k in lt} and set(lt) == set(R.DEFAULT) - {"sample_rate"}
    path = tmp_path / f"weights_{name}_test.pth"
    R.write_checkpoint(path, R.CONFIGS[name], sd)
    m = dac_weights.load(path)
    assert m.cfg == cfg                                                   # latent_dim None -> encoder_dim * 2^len(rates) for W
    blob = m.packed()
    want = sum(v.numel() for k, v in sd.items() if not k.endswith(("weight_g", "weight_v")))
    want += sum(v.numel() for k, v in sd.items() if k.endswith("weight_v"))
    assert blob.dtype.name == "float32" and blob.size == want
    # the blob opens with the folded input convolution and its bias
    w0 = R.fold(sd, "encoder.block.0").reshape(-1)
    assert torch.equal(torch.from_numpy(blob[:w0.numel()]), w0)
    assert torch.equal(torch.from_numpy(blob[w0.numel():w0.numel() + cfg["encoder_dim"]]), sd["encoder.block.0.bias"])


def test_loader_refusals(pack, tmp_path):
    from egregora_amd import dac_weights
    cfg, sd, n64, n32 = K.model("S")

    def load_with(mut, kwargs=None):
        d = dict(sd)
        mut(d)
        p = tmp_path / "weights_x_test.pth"
        R.write_checkpoint(p, dict(R.CONFIGS["S"], **(kwargs or {})), d)
        return dac_weights.load(p)

    with pytest.raises(RuntimeError, match=r"missing tensor encoder\.block\.1\.block\.0\.block\.1\.bias"):
        load_with(lambda d: d.pop("encoder.block.1.block.0.block.1.bias"))
    with pytest.raises(RuntimeError, match=r"unmapped tensor decoder\.model\.9\.extra"):
        load_with(lambda d: d.update({"decoder.model.9.extra": torch.zeros(3)}))
    with pytest.raises(RuntimeError, match=r"shape of quantizer\.quantizers\.1\.codebook\.weight: \(64, 4\), expected \(64, 8\)"):
        load_with(lambda d: d.update({"quantizer.quantizers.1.codebook.weight": torch.zeros(64, 4)}))
    with pytest.raises(RuntimeError, match=r"decoder_dim: the tensor shapes imply 64, metadata\.kwargs says 128"):
        load_with(lambda d: None, {"decoder_dim": 128})
    with pytest.raises(RuntimeError, match=r"n_codebooks 33 above 32(.|\n)*codebook_size \* codebook_dim = 32768 above 16384"):
        dac_weights.check_supported(dict(cfg, n_codebooks=33, codebook_size=4096))
    with pytest.raises(RuntimeError, match=r"decoder rate 17 outside 1 \.\. 16"):
        dac_weights.check_supported(dict(cfg, decoder_rates=[17, 2]))
    with pytest.raises(RuntimeError, match=r"latent width 4096 above 2048"):
        dac_weights.check_supported(dict(cfg, latent_dim=4096))
    dac_weights.check_supported(K.model("W")[0])


def test_create_refuses_what_check_supported_refuses(pack):
    """DAC-P9: the host-only entry point runs the library's config check; it refuses the same configs."""
    from egregora_amd import dac_engine, dac_weights
    cfg = K.model("S")[0]
    for bad in (dict(cfg, n_codebooks=33), dict(cfg, codebook_size=4096), dict(cfg, decoder_rates=[17, 2]), dict(cfg, latent_dim=4096),
                dict(cfg, decoder_dim=66), dict(cfg, codebook_dim=128, codebook_size=2)):
        with pytest.raises(RuntimeError):
            dac_weights.check_supported(bad)
        with pytest.raises(RuntimeError, match="egr_dac_lengths failed"):
            dac_engine.lengths_c(bad, 100)


def test_discover_order(pack, tmp_path, monkeypatch):
    from egregora_amd import dac_weights
    env_dir, home = tmp_path / "env", tmp_path / "home"
    cache = home / ".cache" / "descript" / "dac"
    env_dir.mkdir()
    cache.mkdir(parents=True)
    monkeypatch.setenv("HOME", str(home))
    monkeypatch.delenv("EGREGORA_DAC_MODEL_DIR", raising=False)
    dirs = dac_weights.candidate_dirs()
    assert dirs[-1] == cache and all(d.parts[-3:] == ("models", "audio", "dac") for d in dirs[:-1])
    assert dac_weights.discover("44khz") is None
    msg = dac_weights.not_found_message("44khz")
    assert all(s in msg for s in ("EGREGORA_DAC_MODEL_DIR", "models/audio/dac/", "~/.cache/descript/dac/", "weights_44khz_"))
    (cache / "weights_44khz_8kbps_0.0.1.pth").write_bytes(b"")
    assert dac_weights.discover("44khz") == cache / "weights_44khz_8kbps_0.0.1.pth" and dac_weights.discover("24khz") is None
    monkeypatch.setenv("EGREGORA_DAC_MODEL_DIR", str(env_dir))
    assert dac_weights.candidate_dirs()[0] == env_dir
    assert dac_weights.discover("44khz") == cache / "weights_44khz_8kbps_0.0.1.pth"      # the env dir holds none: the search goes on
    (env_dir / "weights_44khz_x.pth").write_bytes(b"")
    assert dac_weights.discover("44khz") == env_dir / "weights_44khz_x.pth"


@pytest.mark.parametrize("name", ["S", "O", "W", "G", "T", "C"])
def test_synthetic_models_keep_their_level(name):
    """Every stage's rms stays in [0.1, 10] in float64, so the relative gates of the GPU tests mean something; alpha in [0.5, 2]."""
    cfg, sd, n64, n32 = K.model(name)
    f = K.forward(name)
    stages = {f"enc{i}": t for i, t in enumerate(f["enc64"])}
    stages.update({f"vq_in{i}": t for i, t in enumerate(f["ins64"])})
    stages.update({f"dec{i}": t for i, t in enumerate(f["dec64"])})
    stages.update(z=f["z64"], y=f["y64"])
    levels = {k: R.rms(v) for k, v in stages.items()}
    print(name, {k: round(v, 3) for k, v in levels.items()})
    assert all(0.1 <= v <= 10 for v in levels.values()), levels
    al = torch.cat([v.flatten() for k, v in sd.items() if k.endswith(".alpha")])
    assert 0.5 <= float(al.min()) and float(al.max()) <= 2.0
    v = K.vq_case(name) if name != "O" else None
    if v is not None:
        assert 0.1 <= R.rms(v["ze"]) <= 10 and 0.1 <= R.rms(v["z64"]) <= 10


@pytest.mark.parametrize("name", ["S", "W", "G", "T", "C"])
def test_tie_statistics(name):
    """What the GPU test's code comparison rests on: in float64 alone at most 5 % of the 2 000 frames have a stage whose best and
    second-best similarities lie within 1e-4, and tau (4 x the fp32 restatement's similarity error) is far below that."""
    v = K.vq_case(name)
    excluded = 1.0 - float(K.safe_frames(v["margins"], K.MARGIN_CAP).double().mean())
    per_stage = float((v["margins"] <= K.MARGIN_CAP).double().mean())
    print(f"{name}: tau {v['tau']:.2e}, queries under 1e-4: {per_stage:.4%}, frames left out at 1e-4: {excluded:.3%}")
    assert v["margins"].shape == (K.VQ_ROWS, K.model(name)[0]["n_codebooks"], K.VQ_FRAMES)
    assert excluded <= K.MAX_EXCLUDED
    assert 0 < 2 * v["tau"] <= K.MARGIN_CAP
    # lowest index wins ties: argmax of a row with two equal maxima
    s = torch.tensor([[0.1, 0.7, 0.7, 0.2]], dtype=torch.float64)
    assert int(torch.argmax(s, dim=-1)) == 1


def _print_and_check_caps(label, marg, tau):
    """tau and the share of frames left out at 2 tau, per row; the caps of the GPU tests (dac_check)."""
    excluded = 1.0 - K.safe_frames(marg, 2 * tau).double().mean(dim=1)
    print(f"{label}: tau {tau:.2e}, frames left out at 2 tau per row: {[f'{float(e):.3%}' for e in excluded]}, smallest margin {float(marg.min()):.2e}")
    assert 0 < 2 * tau <= K.MARGIN_CAP
    assert float(excluded.max()) <= K.MAX_EXCLUDED
    return excluded


@pytest.mark.parametrize("name", ["T", "S"])
def test_tie_statistics_ragged_frame_count(name):
    """The quantiser alone at 3 rows x 667 frames (2 001: the last workgroup has idle frames, a frame group straddles a row)."""
    rows, frames = K.VQ_RAGGED
    v = K.vq_case(name, rows, frames)
    assert v["margins"].shape == (rows, K.model(name)[0]["n_codebooks"], frames)
    _print_and_check_caps(f"{name} {rows} x {frames}", v["margins"], v["tau"])
    excluded = 1.0 - float(K.safe_frames(v["margins"], K.MARGIN_CAP).double().mean())
    print(f"  frames left out at 1e-4: {excluded:.3%}")
    assert excluded <= K.MAX_EXCLUDED


@pytest.mark.parametrize("name,n,rows,seed", K.edge_cases())
def test_edge_lengths_have_no_near_tie(name, n, rows, seed):
    """Below 20 frames the 5 % cap means no frame may be left out: at the chosen seed every float64 margin exceeds 2 tau, and the
    fp32 restatement chooses float64's codes (so that its z is a yardstick on every frame).  A seed that fails is changed, not the cap."""
    f = K.forward(name, n, rows, seed)
    tau = K.e2e_tau(name, n, rows, seed)
    marg = K.margins(f["sims64"])
    excluded = _print_and_check_caps(f"{name} n={n} rows={rows} seed={seed} ({marg.shape[-1]} frames)", marg, tau)
    assert marg.shape[-1] == -(-n // R.hop(K.model(name)[0]))
    if marg.shape[-1] < 20:
        assert float(excluded.max()) == 0.0 and bool((marg > 2 * tau).all())
    assert float((f["codes32"] == f["codes64"]).all(dim=1).double().mean()) >= 1 - K.MAX_EXCLUDED


def test_rows_at_two_levels():
    """tests/test_gpu_dac_configs.py runs config S with row 1 at 2^-10 of row 0 and gates every row against its own float64 rms.
    This pins, from the restatement alone, that each row stays inside the code caps, and what that test can see of a row maximum
    taken from the other row.  The device brings each row of a two-fp16-term contraction into [2^14, 2^15) by a power of two from
    the row's own maximum (egr_conv.h, h2_row_scale):
      * the LOUD row split at the QUIET row's scale overflows fp16, and its dec0 fails the gate: that exchange is visible;
      * the QUIET row split at the LOUD row's scale (hi = fp16(x / s), lo = fp16(x / s - hi), x' = (hi + lo) s) is off by at most
        2^-25 s per element whatever the row's level, since fp16's subnormals reach 2^-24.  Through the float64 dec_in convolution
        that is 1.9e-10 of dec0's rms at 2^-10 (fp32 itself: 5.3e-8), and it only falls relative to the bias that carries a quiet
        row's dec0 as the level drops (9.9e-12 at 2^-16, 8.8e-12 at 2^-24): it passes `gate` at every level, so no level makes
        that exchange visible, and none makes it matter.  The level stays at 2^-10."""
    import math
    name, n, rows, seed, levels = K.LEVELS_CASE
    cfg, sd, n64, n32 = K.model(name)
    f = K.forward(*K.LEVELS_CASE)
    tau = K.e2e_tau(*K.LEVELS_CASE)
    _print_and_check_caps(f"{name} rows at {levels}", K.margins(f["sims64"]), tau)
    agree = (f["codes32"] == f["codes64"]).all(dim=1).double().mean(dim=1)
    assert float(agree.min()) >= 1 - K.MAX_EXCLUDED
    zin = f["zin"].double()
    scale = lambda row: 2.0 ** (math.floor(math.log2(float(zin[row].abs().max()))) - 14)       # the row's maximum lands in [2^14, 2^15)

    def dec0_with(row, s):
        v = zin[row] / s
        hi = v.half().double()
        lo = (v - hi).half().double()
        z2 = zin.clone()
        z2[row] = (hi + lo) * s
        with torch.no_grad():
            return n64.conv(z2, "decoder.model.0", pad=3)[row]

    r64, r32 = f["dec64"][0], f["dec32"][0]
    loud = dec0_with(0, scale(1))
    assert not bool(torch.isfinite(loud).all())
    with pytest.raises(AssertionError):
        K.gate("dec0 of the loud row split at the quiet row's scale", loud, r64[0], r32[0])
    quiet = dec0_with(1, scale(0))
    e, e32 = K.rel(quiet, r64[1]), K.rel(r32[1], r64[1])
    print(f"  dec0 of the quiet row split at the loud row's scale: rms {e:.2e} (fp32 {e32:.2e})")
    assert e <= 2.0 ** -25 * scale(0) * 7 * cfg["latent_dim"] / R.rms(r64[1])      # at most 2^-25 s an element, |w| <= 1, 7 x latent terms


def test_tie_case_has_exact_ties_off_the_near_ties():
    """The ties test of tests/test_gpu_dac_configs.py: with rows 17 = 3 and 19 = 0 in every codebook, float64 (lowest index) returns
    3 or 0 on many frames that are no near-tie between different rows, and the caps hold."""
    t = K.tie_case()
    _print_and_check_caps("C with duplicated rows", t["margins"], t["tau"])
    safe = K.safe_frames(t["margins"], 2 * t["tau"])
    kept = [k for k, _ in K.TIE_PAIRS]
    hit = torch.isin(t["codes64"], torch.tensor(kept)).any(dim=1) & safe
    print(f"  frames off the near-ties on which float64 returns one of {kept}: {int(hit.sum())} of {hit.numel()}")
    assert int(hit.sum()) >= 100 and not bool(torch.isin(t["codes64"], torch.tensor([d for _, d in K.TIE_PAIRS])).any())
    for q in range(t["cfg"]["n_codebooks"]):
        cb = t["sd"][f"quantizer.quantizers.{q}.codebook.weight"]
        assert all(torch.equal(cb[k], cb[d]) for k, d in K.TIE_PAIRS)


def test_reuse_lengths_are_distinct_workloads(pack):
    from egregora_amd import dac_engine
    cfg = K.model("S")[0]
    long, short = (dac_engine.lengths(cfg, n) for n in K.REUSE_LENGTHS)
    assert long[1] > 500 and short == (16, 2, 16)
