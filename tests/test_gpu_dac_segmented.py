"""The segmented Descript Audio Codec on the device (egr_dacseg_encode / egr_dacseg_decode / egr_dacseg_from_codes,
DESIGN.md 7.6.1) against the float64 restatement tests/dac_torch.py with the gates of tests/dac_check.py: segments of several lengths
(one frame, an interior cut, one frame short of the file, more than the file) on the configs whose strides, paddings and kernel paths
differ, one window against one pass bit for bit, rows at two levels, the workspace and the path the engine chooses above its budget,
z from integer codes, and the length and row edges."""
import pytest
import torch

import dac_check as K
import dac_torch as R

pytestmark = pytest.mark.gpu
_ENGINES = {}
CASES = (("S", 2051), ("O", 2051), ("G", 1205))        # 257 frames; 206 frames, an odd stride; 201 frames, the general paths
W_CASE = ("W", 20483, 8)                               # 41 frames of the 44 kHz widths, margins of 8: five cuts


def new_engine(name):
    from egregora_amd import dac_engine, dac_weights
    cfg, sd, _, _ = K.model(name)
    return dac_engine.DacEngine(dac_weights.DacModel(cfg, sd), torch.cuda.current_device())


def engine(name):
    if name not in _ENGINES:
        _ENGINES[name] = new_engine(name)
    return _ENGINES[name]


def frames_of(name, n):
    """ceil(n / hop): what the encoder makes of n samples when every stride is at least 2 (the tests assert the shapes)."""
    return -(-n // R.hop(R.config(name)))


def seg_cases(extra=()):
    out = []
    for name, n in CASES:
        F = frames_of(name, n)
        out += [(name, n, s) for s in (1, 32, F - 1) + tuple(F + e for e in extra)]
    return out + [W_CASE]


def check_codes(label, codes_dev, codes64, marg, tau):
    """Equality with float64's codes on the frames whose float64 margins all exceed 2 tau; returns that frame mask [rows, F]."""
    safe = K.safe_frames(marg, 2 * tau)
    excluded = 1.0 - float(safe.double().mean())
    same = (codes_dev == codes64).all(dim=1)
    print(f"  {label}: tau {tau:.2e}, frames left out at 2 tau: {excluded:.3%}, frames with equal codes: {float(same.double().mean()):.3%}")
    assert 2 * tau <= K.MARGIN_CAP, tau
    assert excluded <= K.MAX_EXCLUDED, excluded
    assert bool(same[safe].all()), (label, int((~same[safe]).sum()))
    return safe & same


def check_encode(label, f, tau, z, codes, ze):
    """ze through the gate, the codes off the near-ties, z on the frames whose codes all agree."""
    K.gate(f"{label} ze", ze.cpu(), f["enc64"][-1], f["enc32"][-1])
    ok = check_codes(label, codes.cpu().long(), f["codes64"], K.margins(f["sims64"]), tau)
    ok &= (f["codes32"] == f["codes64"]).all(dim=1)
    assert float(ok.double().mean()) >= 1 - K.MAX_EXCLUDED
    pick = lambda t: t.double().cpu().transpose(1, 2)[ok]
    K.gate(f"{label} z", pick(z), pick(f["z64"]), pick(f["z32"]))


# ---- 1
@pytest.mark.parametrize("name,n,seg", seg_cases())
def test_encode_in_segments_against_float64(pack, name, n, seg):
    cfg = R.config(name)
    f = K.forward(name, n)
    eng = engine(name)
    z, codes, ze = eng.encode(f["x"].cuda(), seg_frames=seg, return_ze=True)
    torch.cuda.synchronize()
    F = frames_of(name, n)
    assert tuple(z.shape) == tuple(ze.shape) == (R.ROWS, cfg["latent_dim"], F) and tuple(codes.shape) == (R.ROWS, cfg["n_codebooks"], F)
    assert codes.dtype == torch.int32 and int(codes.min()) >= 0 and int(codes.max()) < cfg["codebook_size"]
    print(f"{name} n {n}: encode in segments of {seg} of {F} frames")
    check_encode(f"{name}/{seg}", f, K.e2e_tau(name, n), z, codes, ze)


# ---- 2
@pytest.mark.parametrize("name,n,seg", seg_cases(extra=(5,)))
def test_decode_in_segments_against_float64(pack, name, n, seg):
    f = K.forward(name, n)
    eng = engine(name)
    y = eng.decode(f["zin"].cuda(), seg_frames=seg)
    torch.cuda.synchronize()
    assert tuple(y.shape) == tuple(f["y64"].shape) == (R.ROWS, eng.lengths(n)[2])
    print(f"{name} n {n}: decode in segments of {seg} of {frames_of(name, n)} frames")
    K.gate("y", y.cpu(), f["y64"], f["y32"])                   # over the whole n_decoded: a crop off by one at an odd stride shows


# ---- 3
@pytest.mark.parametrize("name,n", CASES)
def test_one_window_is_one_pass_bit_for_bit(pack, name, n):
    f = K.forward(name, n)
    eng = engine(name)
    F = frames_of(name, n)
    x, zin = f["x"].cuda(), f["zin"].cuda()
    z1, c1 = eng.encode(x)
    y1 = eng.decode(zin)
    for seg in (F, F + 5):
        z2, c2, _ = eng.encode(x, seg_frames=seg, return_ze=True)
        y2 = eng.decode(zin, seg_frames=seg)
        torch.cuda.synchronize()
        assert torch.equal(z1, z2) and torch.equal(c1, c2) and torch.equal(y1, y2), (name, seg)


# ---- 4
def test_rows_at_two_levels_in_segments(pack):
    """A window's operand scales come from its own row maxima, row by row: the row 60 dB down passes the same gates."""
    name, n, rows, seed, levels = K.LEVELS_CASE
    f = K.forward(*K.LEVELS_CASE)
    eng = engine(name)
    z, codes, ze = eng.encode(f["x"].cuda(), seg_frames=32, return_ze=True)
    y = eng.decode(f["zin"].cuda(), seg_frames=32)
    torch.cuda.synchronize()
    print(f"{name}: rows at levels {levels}, segments of 32 frames")
    for r in range(rows):
        K.gate(f"ze row {r}", ze[r].cpu(), f["enc64"][-1][r], f["enc32"][-1][r])
        K.gate(f"y row {r}", y[r].cpu(), f["y64"][r], f["y32"][r])


# ---- 5
def test_workspace_grows_with_the_length_by_whole_length_buffers_only(pack):
    from egregora_amd import dac_engine as E
    eng = engine("S")
    cfg = eng.cfg
    h, lat, rows = R.hop(cfg), cfg["latent_dim"], 2
    n1, more = 2051, 1000
    n2 = n1 + more * h
    for kind in (E.ENCODE, E.DECODE):
        for seg in (1, 32, 64):
            a, b = eng.segment_workspace_bytes(rows, seg, n1, kind), eng.segment_workspace_bytes(rows, seg, n2, kind)
            print(f"  kind {kind} seg_frames {seg}: {a} -> {b} bytes for {more} more frames")
            assert 0 < a < b and b - a <= 3 * lat * 4 * more * rows, (kind, seg, a, b)
        assert eng.segment_workspace_bytes(rows, 32, n1, kind) < eng.segment_workspace_bytes(rows, 64, n1, kind)


def test_a_segmented_call_holds_less_than_one_pass(pack):
    from egregora_amd import dac_engine as E
    f = K.forward("S", 2051)
    eng = new_engine("S")                                      # a handle that has held nothing yet
    assert eng.workspace_held() == 0
    x = f["x"].cuda()
    z, codes = eng.encode(x, seg_frames=32)
    held = eng.workspace_held()
    assert 0 < held <= eng.segment_workspace_bytes(2, 32, 2051, E.ENCODE) < eng.workspace_bytes(2, 2051)
    y = eng.decode(z, seg_frames=32)
    held = eng.workspace_held()
    assert held <= max(eng.segment_workspace_bytes(2, 32, 2051, k) for k in (E.ENCODE, E.DECODE)) < eng.workspace_bytes(2, 2051)
    # long, short, long: nothing is kept from call to call
    eng.encode(R.test_signal(2, 9, 5).cuda(), seg_frames=32)
    z3, codes3 = eng.encode(x, seg_frames=32)
    y3 = eng.decode(z, seg_frames=32)
    torch.cuda.synchronize()
    assert torch.equal(z, z3) and torch.equal(codes, codes3) and torch.equal(y, y3)
    assert eng.workspace_held() == held


def test_nodes_take_segments_above_the_budget(pack, tmp_path, monkeypatch):
    """The call the engine refused before segments: a budget between a segment's workspace and one pass's."""
    from egregora_amd import dac_engine as E, egregora_audio_codec_dac as nodes
    cfg, sd, n64, n32 = K.model("S")
    R.write_checkpoint(tmp_path / "weights_44khz_test.pth", R.CONFIGS["S"], sd)
    monkeypatch.setenv("EGREGORA_DAC_MODEL_DIR", str(tmp_path))
    f = K.forward("S", 2051)
    x = torch.stack([f["x"], f["x"].flip(0)])                  # [2, 2, 2051]: the second batch element is the first with its rows swapped
    eng = E.engine(tmp_path / "weights_44khz_test.pth")
    # the product's step (2 048 frames, chosen for the 44 kHz model) is longer than this file: the path choice is exercised at a step
    # that cuts 257 frames several times
    monkeypatch.setattr(E, "SEGMENT_STEP", 64)
    seg = max(eng.segment_workspace_bytes(2, E.SEGMENT_STEP, 2051, k) for k in (E.ENCODE, E.DECODE))
    one = eng.workspace_bytes(2, 2051)
    print(f"  workspace: {E.SEGMENT_STEP}-frame segments {seg} bytes, one pass {one} bytes")
    assert seg < one
    monkeypatch.setenv(E.WORKSPACE_GB_ENV, repr((seg + one) / 2 / 2 ** 30))
    budget = E.workspace_budget_bytes()
    assert seg <= budget < one

    def took_segments(kind):
        s = eng.last_seg_frames                                 # the largest multiple of the step whose workspace fits
        return s is not None and s % E.SEGMENT_STEP == 0 and eng.segment_workspace_bytes(2, s, 2051, kind) <= budget

    d, log = nodes.Egregora_DAC_Encode().execute({"waveform": x, "sample_rate": 44100}, "44khz")
    assert took_segments(E.ENCODE), eng.last_seg_frames
    eng.last_seg_frames = None
    (audio, log2) = nodes.Egregora_DAC_Decode().execute(d)
    assert took_segments(E.DECODE), eng.last_seg_frames
    y = audio["waveform"]
    n_dec = E.lengths(cfg, 2051)[2]
    assert tuple(y.shape) == (2, 2, n_dec) and audio["sample_rate"] == 44100
    print("S: node round trip in segments")
    for b in range(2):
        want = (lambda t: t) if b == 0 else (lambda t: t.flip(0))
        agree = (d["codes"][b] == want(f["codes64"])).all(dim=1) & (f["codes32"] == f["codes64"]).all(dim=1)
        assert bool(agree.all())                               # y depends on every frame within the receptive field
        K.gate(f"z[{b}]", d["latents"][b][0], want(f["z64"]), want(f["z32"]))
        K.gate(f"y[{b}]", y[b], want(f["y64"]), want(f["y32"]))
    # a budget no segment fits still refuses, and names the variable
    monkeypatch.setenv(E.WORKSPACE_GB_ENV, "1e-6")
    with pytest.raises(RuntimeError, match=r"EGREGORA_DAC_WORKSPACE_GB = 1e-06"):
        nodes.Egregora_DAC_Encode().execute({"waveform": x, "sample_rate": 44100}, "44khz")
    with pytest.raises(RuntimeError, match=r"EGREGORA_DAC_WORKSPACE_GB = 1e-06"):
        nodes.Egregora_DAC_Decode().execute(d)


# ---- 6
@pytest.mark.parametrize("name", ["S", "W", "G", "T"])
def test_from_codes_has_the_bits_of_the_encode(pack, name):
    cfg, sd, n64, n32 = K.model(name)
    f = K.forward(name)
    eng = engine(name)
    z, codes = eng.encode(f["x"].cuda())
    zc = eng.from_codes(codes)
    torch.cuda.synchronize()
    assert zc.dtype == torch.float32 and torch.equal(zc, z)
    assert torch.equal(eng.from_codes(codes.to(torch.int64)), z)
    ze, c = f["enc64"][-1], codes.cpu().long()
    print(f"{name}: z from codes")
    with torch.no_grad():
        K.gate("z", zc.cpu(), n64.quantize(ze, codes=c)[0], n32.quantize(ze, codes=c)[0])


@pytest.mark.parametrize("name", ["S", "G", "T"])
def test_from_codes_on_a_ragged_frame_count(pack, name):
    cfg, sd, n64, n32 = K.model(name)
    rows, frames = K.VQ_RAGGED
    eng = engine(name)
    ze = R.quantiser_input(cfg, rows, frames, 5)
    z, codes = eng.quantize(ze.cuda())
    assert torch.equal(eng.from_codes(codes), z)
    g = torch.Generator().manual_seed(9)
    c = torch.randint(0, cfg["codebook_size"], (rows, cfg["n_codebooks"], frames), generator=g)
    c[0, :, 0], c[-1, :, -1] = 0, cfg["codebook_size"] - 1
    zc = eng.from_codes(c.cuda())
    torch.cuda.synchronize()
    print(f"{name}: z from {rows} x {frames} random codes")
    with torch.no_grad():
        K.gate("z", zc.cpu(), n64.quantize(ze, codes=c)[0], n32.quantize(ze, codes=c)[0])


def test_from_codes_refuses_codes_outside_the_codebook(pack):
    eng = engine("S")
    cfg = eng.cfg
    good = torch.zeros((1, cfg["n_codebooks"], 5), dtype=torch.int64, device="cuda")
    for bad in (-1, cfg["codebook_size"]):
        c = good.clone()
        c[0, 1, 3] = bad
        with pytest.raises(ValueError, match="from_codes"):
            eng.from_codes(c)
    with pytest.raises(ValueError, match="from_codes"):
        eng.from_codes(good[:, :-1])
    with pytest.raises(ValueError, match="from_codes"):
        eng.from_codes(good.float())
    assert tuple(eng.from_codes(good).shape) == (1, cfg["latent_dim"], 5)


def test_a_codes_only_dict_decodes_to_the_same_audio(pack, tmp_path, monkeypatch):
    from egregora_amd import egregora_audio_codec_dac as nodes
    cfg, sd, _, _ = K.model("S")
    R.write_checkpoint(tmp_path / "weights_44khz_test.pth", R.CONFIGS["S"], sd)
    monkeypatch.setenv("EGREGORA_DAC_MODEL_DIR", str(tmp_path))
    x = torch.stack([R.test_signal(2, 1003, 11), R.test_signal(2, 1003, 12)])
    d, _ = nodes.Egregora_DAC_Encode().execute({"waveform": x, "sample_rate": 44100}, "44khz")
    dec = nodes.Egregora_DAC_Decode()
    (a, log) = dec.execute(d)
    for variant in (dict(d, latents=[]), {k: v for k, v in d.items() if k != "latents"}):
        (b, log2) = dec.execute(variant)
        assert log2 == log and torch.equal(a["waveform"], b["waveform"])
    with pytest.raises(ValueError) as e:
        dec.execute({k: v for k, v in d.items() if k not in ("latents", "codes")})
    assert str(e.value) == "codes.latents empty"


# ---- 7
@pytest.mark.parametrize("name", ["S", "O", "G"])
def test_length_edges_in_segments_of_one_frame(pack, name):
    cfg = R.config(name)
    h = R.hop(cfg)
    eng = engine(name)
    for n in (1, h + 1):
        f = K.forward(name, n, 3, 3)
        z, codes, ze = eng.encode(f["x"].cuda(), seg_frames=1, return_ze=True)
        y = eng.decode(f["zin"].cuda(), seg_frames=1)
        torch.cuda.synchronize()
        print(f"{name} n {n}, three rows, segments of one frame")
        assert tuple(ze.shape) == (3, cfg["latent_dim"], frames_of(name, n)) and tuple(y.shape) == tuple(f["y64"].shape)
        check_encode(f"{name} n {n}", f, K.e2e_tau(name, n, 3, 3), z, codes, ze)
        K.gate("y", y.cpu(), f["y64"], f["y32"])


def test_no_stage_after_a_segmented_call(pack):
    eng = engine("S")
    f = K.forward("S", 2051)
    eng.encode(f["x"].cuda())
    assert eng.stage("enc", 0).numel() > 0                     # one pass leaves its stages
    eng.encode(f["x"].cuda(), seg_frames=32)
    with pytest.raises(RuntimeError, match="egr_dac_stage"):
        eng.stage("enc", 0)
    eng.decode(f["zin"].cuda(), seg_frames=32)
    with pytest.raises(RuntimeError, match="egr_dac_stage"):
        eng.stage("dec", 0)


def test_seg_frames_below_one_is_refused(pack):
    import ctypes as C
    from egregora_amd import native
    eng = engine("S")
    f = K.forward("S", 2051)
    x = f["x"].cuda()
    with pytest.raises(ValueError):
        eng.encode(x, seg_frames=0)
    z = torch.empty((2, eng.cfg["latent_dim"], 257), device="cuda")
    codes = torch.empty((2, eng.cfg["n_codebooks"], 257), dtype=torch.int32, device="cuda")
    rc = native.lib().egr_dacseg_encode(eng.h, native.ptr(x), 2, 2051, native.ptr(z), native.ptr(codes), None, 0, native.stream_ptr())
    assert rc != native.EGR_OK and "seg_frames" in native.last_error()
    y = torch.empty((2, eng.lengths(2051)[2]), device="cuda")
    rc = native.lib().egr_dacseg_decode(eng.h, native.ptr(z), 2, 257, native.ptr(y), 0, native.stream_ptr())
    assert rc != native.EGR_OK and "seg_frames" in native.last_error()
