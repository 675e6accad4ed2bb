"""Native Descript Audio Codec (csrc/egr_dac.hip) at the configs, lengths and row counts tests/test_gpu_dac.py does not reach, against
the float64 restatement tests/dac_torch.py with the gates of tests/dac_check.py unchanged.  tests/test_dac_host.py shows from the
restatement alone that every input here stays inside the caps on frames left out.

  levels       rows at different levels (row 1 at 2^-10 of row 0), every gate per row: a row maximum is per row
  reuse        one handle long, short, long: workspace reuse, the stage list, the zeroed maxima pool
  lengths      one frame (n = 1, hop - 1, hop), two (hop + 1), 1 and 3 rows; S at 1024 samples (levels of 1024, 512, 128: the
               input-stationary 1-D kernel at 16, 32 and 64 channels)
  ragged       the quantiser alone on 3 x 667 frames: idle frames in the last workgroup, a frame group across two rows
  C            fewer codes (20) than lanes, codebook_dim 12 (a ragged second projection pass), latent 24
  ties         C with duplicated codebook rows: the lowest index wins in the kernel; an all-zero query gives code 0
  T            four frames a workgroup (a 64 KiB codebook beside a 2048-wide latent), codebook_dim 16

The file runs in order of rising novelty: S on kernels every DAC test runs first, the quantiser's never-launched shapes last.
"""
import pytest
import torch

import dac_check as K
import dac_torch as R
from test_gpu_dac import check_codes, engine

pytestmark = pytest.mark.gpu


def rows_of(per_row, n):
    """Row selections a check is evaluated on: each row by itself, or all rows at once."""
    return [slice(r, r + 1) for r in range(n)] if per_row else [slice(0, n)]


def encode_checks(eng, f, tau, label, per_row=False):
    """Every encoder stage, the codes off the near-ties and z on the frames whose codes all agree (tests/test_gpu_dac.py's
    test_encoder_stages, on any forward() and optionally row by row)."""
    cfg = eng.cfg
    rows, n = f["x"].shape
    z, codes = eng.encode(f["x"].cuda())
    torch.cuda.synchronize()
    n_pad, frames, _ = eng.lengths(n)
    assert tuple(z.shape) == (rows, cfg["latent_dim"], frames) == tuple(f["z64"].shape)
    assert tuple(codes.shape) == (rows, cfg["n_codebooks"], frames) and codes.dtype == torch.int32
    assert int(codes.min()) >= 0 and int(codes.max()) < cfg["codebook_size"]
    print(f"{label}: encoder")
    marg = K.margins(f["sims64"])
    codes = codes.cpu().long()
    for sel in rows_of(per_row, rows):
        tag = f"[row {sel.start}]" if per_row else ""
        for i, (r64, r32) in enumerate(zip(f["enc64"], f["enc32"])):
            got = eng.stage("enc", i).cpu().reshape(K.cl(r64).shape)
            K.gate(f"enc{i}{tag}", got[sel], K.cl(r64)[sel], K.cl(r32)[sel])
        ok = check_codes(f"{label}{tag} end to end", codes[sel], f["codes64"][sel], marg[sel], tau)
        ok &= (f["codes32"][sel] == f["codes64"][sel]).all(dim=1)      # z32 is a yardstick only where the fp32 path chose the same codes
        assert float(ok.double().mean()) >= 1 - K.MAX_EXCLUDED
        pick = lambda t: t[sel].double().cpu().transpose(1, 2)[ok]      # [frames kept, latent]
        K.gate(f"z{tag}", pick(z), pick(f["z64"]), pick(f["z32"]))
    return z, codes


def decode_checks(eng, f, label, per_row=False):
    """Every decoder stage and y from the float64 z (test_decoder_stages, on any forward() and optionally row by row)."""
    rows = f["zin"].shape[0]
    y = eng.decode(f["zin"].cuda())
    torch.cuda.synchronize()
    assert tuple(y.shape) == (rows, eng.lengths(f["x"].shape[1])[2]) == tuple(f["y64"].shape)
    print(f"{label}: decoder")
    for sel in rows_of(per_row, rows):
        tag = f"[row {sel.start}]" if per_row else ""
        for i, (r64, r32) in enumerate(zip(f["dec64"], f["dec32"])):
            got = eng.stage("dec", i).cpu().reshape(K.cl(r64).shape)
            K.gate(f"dec{i}{tag}", got[sel], K.cl(r64)[sel], K.cl(r32)[sel])
        K.gate(f"y{tag}", y.cpu()[sel], f["y64"][sel], f["y32"][sel])
    return y


def quantiser_checks(eng, n64, n32, v, label):
    """test_quantiser_alone's parts (a), (b), (c) on any vq_case()."""
    cfg = eng.cfg
    rows, _, frames = v["ze"].shape
    z, codes = eng.quantize(v["ze"].cuda())
    torch.cuda.synchronize()
    codes = codes.cpu().long()
    tau = v["tau"]
    print(f"{label}: quantiser alone on {rows} x {frames} frames, tau {tau:.2e}")
    assert 2 * tau <= K.MARGIN_CAP
    assert int(codes.min()) >= 0 and int(codes.max()) < cfg["codebook_size"]
    worst = 0.0
    with torch.no_grad():
        for q in range(cfg["n_codebooks"]):
            r = eng.stage("vq_in", q).cpu().double().reshape(rows, frames, cfg["latent_dim"]).transpose(1, 2)
            s = n64.similarities(r, q)
            gap = s.max(dim=-1).values - s.gather(-1, codes[:, q].unsqueeze(-1)).squeeze(-1)
            worst = max(worst, float(gap.max()))
            if q == 0:
                assert torch.equal(r.float(), v["ze"])            # the first stage's input is ze itself
        print(f"  (a) largest similarity gap of a chosen code: {worst:.2e} (tau {tau:.2e}, ratio {worst / tau:.2f})")
        assert worst <= tau, (worst, tau)
        z64 = n64.quantize(v["ze"], codes=codes)[0]
        z32 = n32.quantize(v["ze"], codes=codes)[0]
    K.gate("(b) z from the device's codes", z.cpu(), z64, z32)
    check_codes(f"(c) {label}", codes, v["codes64"], v["margins"], tau)
    return codes


# ---------------------------------------------------------------------------------------------- S on the kernels every test runs
def test_rows_at_different_levels(pack):
    """Row 1 is row 0's generator at 2^-10, and its z is scaled by 2^-10 again for the decoder; every gate per row, against the
    row's own float64 rms.  A loud row scaled by the quiet row's maximum overflows fp16 (tests/test_dac_host.py
    test_rows_at_two_levels), and a maximum written to or read from row 0's slot by every row leaves row 1 with none."""
    f = K.forward(*K.LEVELS_CASE)
    assert R.rms(f["x"][1]) < 2.0 ** -9 * R.rms(f["x"][0]) and R.rms(f["zin"][1]) < 2.0 ** -9 * R.rms(f["zin"][0])
    eng = engine(pack, "S")
    encode_checks(eng, f, K.e2e_tau(*K.LEVELS_CASE), "S at two levels", per_row=True)
    decode_checks(eng, f, "S at two levels", per_row=True)


def test_handle_reuse_long_short_long(pack):
    from egregora_amd import dac_engine, dac_weights
    cfg, sd, _, _ = K.model("S")

    def fresh():
        e = dac_engine.DacEngine(dac_weights.DacModel(cfg, sd), torch.cuda.current_device())
        e.keep_stages(True)
        return e

    def call(e, x):
        z, codes = e.encode(x)
        y = e.decode(z)
        torch.cuda.synchronize()
        return z.clone(), codes.clone(), y.clone()

    n_long, n_short = K.REUSE_LENGTHS
    xl, xs = R.test_signal(2, n_long, 3).cuda(), R.test_signal(2, n_short, 4).cuda()
    eng = fresh()
    first = call(eng, xl)
    second = call(eng, xs)
    # stage() after the short call: the short call's shapes (decode was the last call, so the encoder's stages have left)
    n_pad, frames, n_dec = eng.lengths(n_short)
    assert eng.stage("dec", 0).numel() == 2 * frames * cfg["decoder_dim"]
    assert eng.stage("dec", len(cfg["decoder_rates"])).numel() == 2 * n_dec * (cfg["decoder_dim"] >> len(cfg["decoder_rates"]))
    eng.encode(xs)
    assert eng.stage("enc", 0).numel() == 2 * n_pad * cfg["encoder_dim"]
    assert eng.stage("enc", len(cfg["encoder_rates"]) + 1).numel() == 2 * frames * cfg["latent_dim"]
    assert eng.stage("vq_in", cfg["n_codebooks"] - 1).numel() == 2 * frames * cfg["latent_dim"]
    third = call(eng, xl)
    other = call(fresh(), xs)
    for a, b in zip(first, third):
        assert a.shape == b.shape and torch.equal(a, b)
    for a, b in zip(second, other):
        assert a.shape == b.shape and torch.equal(a, b)
    assert tuple(second[2].shape) == (2, n_dec) and tuple(first[2].shape) == (2, eng.lengths(n_long)[2])


@pytest.mark.parametrize("name,n,rows,seed", K.edge_cases())
def test_lengths_and_rows(pack, name, n, rows, seed):
    f = K.forward(name, n, rows, seed)
    eng = engine(pack, name)
    label = f"{name} n={n} rows={rows}"
    encode_checks(eng, f, K.e2e_tau(name, n, rows, seed), label)
    decode_checks(eng, f, label)


# ---------------------------------------------------------------------------------------------- the quantiser's other shapes
def test_quantiser_ragged_frame_count_S(pack):
    cfg, sd, n64, n32 = K.model("S")
    quantiser_checks(engine(pack, "S"), n64, n32, K.vq_case("S", *K.VQ_RAGGED), "S")


def test_config_C(pack):
    cfg, sd, n64, n32 = K.model("C")
    eng = engine(pack, "C")
    quantiser_checks(eng, n64, n32, K.vq_case("C"), "C")
    encode_checks(eng, K.forward("C"), K.e2e_tau("C"), "C")
    decode_checks(eng, K.forward("C"), "C")


def test_ties_go_to_the_lowest_index_and_a_zero_query_to_code_0(pack):
    from egregora_amd import dac_engine, dac_weights
    t = K.tie_case()
    cfg = t["cfg"]
    eng = dac_engine.DacEngine(dac_weights.DacModel(cfg, t["sd"]), torch.cuda.current_device())
    z, codes = eng.quantize(t["ze"].cuda())
    torch.cuda.synchronize()
    codes = codes.cpu().long()
    dups = torch.tensor([d for _, d in K.TIE_PAIRS])
    kept = torch.tensor([k for k, _ in K.TIE_PAIRS])
    n_dup = int(torch.isin(codes, dups).sum())
    print(f"C with duplicated rows: device codes equal to a duplicate {n_dup}, to a kept row {int(torch.isin(codes, kept).sum())}")
    assert n_dup == 0
    ok = check_codes("C with duplicated rows", codes, t["codes64"], t["margins"], t["tau"])
    hit = torch.isin(t["codes64"], kept) & K.safe_frames(t["margins"], 2 * t["tau"]).unsqueeze(1)
    assert int(hit.sum()) >= 100 and bool((codes[hit] == t["codes64"][hit]).all()) and bool(ok.any())
    # an all-zero query against a zero bias: every similarity of stage 0 is exactly 0
    eng0 = dac_engine.DacEngine(dac_weights.DacModel(cfg, t["sd_zero_bias"]), torch.cuda.current_device())
    z0, codes0 = eng0.quantize(torch.zeros(2, cfg["latent_dim"], 37, device="cuda"))
    torch.cuda.synchronize()
    assert bool((codes0[:, 0] == 0).all()) and bool(torch.isfinite(z0).all())


def test_config_T(pack):
    cfg, sd, n64, n32 = K.model("T")
    eng = engine(pack, "T")
    quantiser_checks(eng, n64, n32, K.vq_case("T"), "T")
    quantiser_checks(eng, n64, n32, K.vq_case("T", *K.VQ_RAGGED), "T")
    encode_checks(eng, K.forward("T"), K.e2e_tau("T"), "T")
    decode_checks(eng, K.forward("T"), "T")
