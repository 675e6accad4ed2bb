"""Many clips in one padded pass of the Descript Audio Codec on the device (egr_dacmany_encode / egr_dacmany_decode)
against the float64 restatement tests/dac_torch.py with the gates of tests/dac_check.py and the code rule of
tests/test_gpu_dac_segmented.py::check_encode: rows of their own lengths in one call at the default and at the tightest padding,
bit-equality with the one-pass calls where the shapes coincide, independence from the neighbouring rows (other signals, NaN, 60 dB up),
rows at two levels, no state carried between call kinds, every refusal, and encode_many / decode_many over several waves.

A padded call equals the single call to fp32 round-off, not bit for bit (the launcher chooses tiles and split-K from the padded shape),
so every clip is held to float64 by the gates the single call is held to."""
import ctypes as C

import pytest
import torch

import dac_check as K
import dac_torch as R
from test_gpu_dac_segmented import check_encode, engine

pytestmark = pytest.mark.gpu
# (n, rows, seed) of K.forward per clip.  Each set was run through the restatement alone: 2 tau <= MARGIN_CAP, no frame left out, fp32
# and float64 codes agree everywhere
CLIPS = {"S": ((2051, 2, 3), (1003, 1, 21), (333, 1, 22), (9, 1, 23), (1, 1, 24), (777, 2, 25), (1024, 1, 26)),
         "O": ((2051, 2, 3), (1003, 1, 21), (11, 1, 22), (333, 2, 23)),
         "G": ((1205, 2, 3), (601, 1, 21), (120, 1, 22)),
         "W": ((4091, 2, 3), (1500, 1, 21))}
GAP = 5                                                    # NaN samples between (and around) the rows of a flat x


def flat_of(rows_x):
    """Rows [n_r] -> (flat x on the device with GAP NaN samples around every row, offsets, lengths)."""
    parts, offs, pos = [torch.full((GAP,), float("nan"))], [], GAP
    for v in rows_x:
        offs.append(pos)
        parts += [v.float(), torch.full((GAP,), float("nan"))]
        pos += v.numel() + GAP
    return torch.cat(parts).cuda(), offs, [int(v.numel()) for v in rows_x]


def wave_of(name):
    """The config's clips as one wave: (forwards, flat x, offsets, lengths, first row of each clip)."""
    fs = [K.forward(name, *c) for c in CLIPS[name]]
    x, offs, lens = flat_of([f["x"][r] for f in fs for r in range(f["x"].shape[0])])
    first, r = [], 0
    for f in fs:
        first.append(r)
        r += f["x"].shape[0]
    return fs, x, offs, lens, first


def padded_z(fs, eng, P, fill):
    """Every clip's zin in front of a row of P frames; the tails hold `fill`."""
    rows = sum(f["zin"].shape[0] for f in fs)
    z = torch.full((rows, eng.cfg["latent_dim"], P), fill, dtype=torch.float32)
    frames, r = [], 0
    for f in fs:
        c, _, F = f["zin"].shape
        z[r:r + c, :, :F] = f["zin"]
        frames += [F] * c
        r += c
    return z.cuda(), frames


# ---- 1
@pytest.mark.parametrize("tight", [False, True])
@pytest.mark.parametrize("name", ["S", "O", "G", "W"])
def test_encode_rows_against_float64(pack, name, tight):
    from egregora_amd import dac_engine as E
    eng = engine(name)
    cfg = eng.cfg
    fs, x, offs, lens, first = wave_of(name)
    longest = max(eng.lengths(n)[1] for n in lens)
    P = longest if tight else E.default_pad_frames(longest)
    z, codes, ze = eng.encode_rows(x, offs, lens, pad_frames=longest if tight else None, return_ze=True)
    torch.cuda.synchronize()
    assert tuple(z.shape) == tuple(ze.shape) == (len(lens), cfg["latent_dim"], P) and tuple(codes.shape) == (len(lens), cfg["n_codebooks"], P)
    assert codes.dtype == torch.int32 and int(codes.min()) >= 0 and int(codes.max()) < cfg["codebook_size"]         # the tails too
    assert bool(torch.isfinite(z).all()) and bool(torch.isfinite(ze).all())
    print(f"{name}: {len(lens)} rows of {lens} samples in {P} frames")
    for f, r0, c in zip(fs, first, CLIPS[name]):
        rows, F = f["x"].shape[0], f["codes64"].shape[-1]
        cut = lambda t: t[r0:r0 + rows, :, :F]
        check_encode(f"{name} n {c[0]}", f, K.e2e_tau(name, *c), cut(z), cut(codes), cut(ze))


# ---- 2
@pytest.mark.parametrize("tight", [False, True])
@pytest.mark.parametrize("name", ["S", "O", "G", "W"])
def test_decode_rows_against_float64(pack, name, tight):
    from egregora_amd import dac_engine as E
    eng = engine(name)
    fs = [K.forward(name, *c) for c in CLIPS[name]]
    longest = max(f["zin"].shape[2] for f in fs)
    P = longest if tight else E.default_pad_frames(longest)
    z, frames = padded_z(fs, eng, P, float("nan"))          # a tail may hold anything
    y = eng.decode_rows(z, frames, pad_frames=longest if tight else None)
    torch.cuda.synchronize()
    assert tuple(y.shape) == (len(frames), E.decoded_length(eng.cfg, P))
    r = 0
    for f, c in zip(fs, CLIPS[name]):
        rows, n_dec = f["y64"].shape
        assert n_dec == eng.lengths(c[0])[2]
        K.gate(f"{name} n {c[0]} y", y[r:r + rows, :n_dec].cpu(), f["y64"], f["y32"])        # the whole n_decoded: a crop off by one shows
        r += rows


# ---- 3
@pytest.mark.parametrize("name", ["S", "O", "G"])
def test_a_wave_of_one_clip_is_one_pass_bit_for_bit(pack, name):
    eng = engine(name)
    f = K.forward(name, *CLIPS[name][0])
    F = f["codes64"].shape[-1]
    x, offs, lens = flat_of(list(f["x"]))
    z1, c1 = eng.encode(f["x"].cuda())
    y1 = eng.decode(f["zin"].cuda())
    z2, c2 = eng.encode_rows(x, offs, lens, pad_frames=F)
    y2 = eng.decode_rows(f["zin"].cuda(), [F] * f["zin"].shape[0], pad_frames=F)
    torch.cuda.synchronize()
    assert torch.equal(z1, z2) and torch.equal(c1, c2) and torch.equal(y1, y2)


@pytest.mark.parametrize("name", ["S", "O", "G"])
def test_clips_of_equal_length_are_the_stacked_one_pass_call(pack, name):
    eng = engine(name)
    n = CLIPS[name][1][0]
    fa, fb = K.forward(name, *CLIPS[name][1]), K.forward(name, n, 2, 3)
    F = fa["codes64"].shape[-1]
    xs, zs = torch.cat([fa["x"], fb["x"]]), torch.cat([fa["zin"], fb["zin"]])
    x, offs, lens = flat_of(list(xs))
    z1, c1 = eng.encode(xs.cuda())
    y1 = eng.decode(zs.cuda())
    z2, c2 = eng.encode_rows(x, offs, lens, pad_frames=F)
    y2 = eng.decode_rows(zs.cuda(), [F] * 3, pad_frames=F)
    torch.cuda.synchronize()
    assert torch.equal(z1, z2) and torch.equal(c1, c2) and torch.equal(y1, y2)


# ---- 4
def test_a_row_does_not_depend_on_its_neighbours(pack):
    """Same lengths and pad_frames, the neighbours replaced: other signals, NaN, the first ones 60 dB up.  The observed clip's bits stay."""
    eng = engine("S")
    f = K.forward("S", 1003, 1, 21)
    F = f["codes64"].shape[-1]
    n_dec = f["y64"].shape[-1]
    got = []
    for kind in ("signals", "nan", "loud"):
        if kind == "nan":
            a, b = torch.full((2051,), float("nan")), torch.full((333,), float("nan"))
        else:
            a, b = R.test_signal(1, 2051, 40)[0], R.test_signal(1, 333, 41)[0]
            if kind == "loud":
                a, b = a * 2.0 ** 10, b * 2.0 ** 10
        x, offs, lens = flat_of([a, f["x"][0], b])
        z, codes, ze = eng.encode_rows(x, offs, lens, return_ze=True)
        P = z.shape[2]
        zin = torch.zeros((3, eng.cfg["latent_dim"], P))
        fill = float("nan") if kind == "nan" else (2.0 ** 10 if kind == "loud" else 1.0)
        zin[0], zin[2] = fill * torch.randn(zin[0].shape, generator=torch.Generator().manual_seed(7)), fill
        zin[1, :, :F] = f["zin"][0]
        y = eng.decode_rows(zin.cuda(), [257, F, 42], pad_frames=P)
        torch.cuda.synchronize()
        got.append((z[1, :, :F].clone(), codes[1, :, :F].clone(), ze[1, :, :F].clone(), y[1, :n_dec].clone()))
    for other in got[1:]:
        assert all(torch.equal(u, v) for u, v in zip(got[0], other))
    assert all(bool(torch.isfinite(t.float()).all()) for t in got[0])
    check_encode("S n 1003 between neighbours", f, K.e2e_tau("S", 1003, 1, 21), got[0][0][None], got[0][1][None], got[0][2][None])
    K.gate("y", got[0][3].cpu(), f["y64"], f["y32"])


# ---- 5
def test_rows_at_two_levels_beside_a_longer_clip(pack):
    """A row's operand scales come from its own valid positions: the row 60 dB down passes the same gates."""
    name, n, rows, seed, levels = K.LEVELS_CASE
    f, g = K.forward(*K.LEVELS_CASE), K.forward(name, 2051, 2, 3)
    eng = engine(name)
    x, offs, lens = flat_of(list(g["x"]) + list(f["x"]))
    z, codes, ze = eng.encode_rows(x, offs, lens, return_ze=True)
    zp, frames = padded_z([g, f], eng, z.shape[2], 1e3)
    y = eng.decode_rows(zp, frames, pad_frames=z.shape[2])
    torch.cuda.synchronize()
    F, n_dec = f["codes64"].shape[-1], f["y64"].shape[-1]
    print(f"{name}: rows at levels {levels} beside two rows of 2051 samples")
    for r in range(rows):
        K.gate(f"ze row {r}", ze[2 + r, :, :F].cpu(), f["enc64"][-1][r], f["enc32"][-1][r])
        K.gate(f"y row {r}", y[2 + r, :n_dec].cpu(), f["y64"][r], f["y32"][r])


# ---- 6
def test_nothing_is_carried_between_call_kinds(pack):
    from test_gpu_dac_segmented import new_engine
    eng = new_engine("S")
    fs, x, offs, lens, first = wave_of("S")
    zp, frames = padded_z(fs, eng, 272, 0.0)
    a = eng.encode_rows(x, offs, lens) + (eng.decode_rows(zp, frames),)
    held = eng.workspace_held()
    assert held > 0
    with pytest.raises(RuntimeError, match="egr_dac_stage"):
        eng.stage("enc", 0)
    long = R.test_signal(2, 4099, 5).cuda()
    z1, _ = eng.encode(long)                                 # one pass on a longer input
    eng.decode(z1)
    assert eng.stage("dec", 0).numel() > 0
    eng.encode(long, seg_frames=32)                          # segments
    eng.decode(z1, seg_frames=32)
    b = eng.encode_rows(x, offs, lens) + (eng.decode_rows(zp, frames),)
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    assert eng.workspace_held() >= held
    with pytest.raises(RuntimeError, match="egr_dac_stage"):
        eng.stage("dec", 0)


# ---- 7
def test_refusals_come_before_anything_is_allocated(pack):
    from egregora_amd import dac_engine as E, native
    from test_gpu_dac_segmented import new_engine
    lib = native.lib()
    eng, big = new_engine("S"), new_engine("W")
    assert eng.workspace_held() == 0 == big.workspace_held()
    buf = torch.zeros(4096, device="cuda")
    ibuf = torch.zeros(4096, dtype=torch.int32, device="cuda")
    st = native.stream_ptr()

    def enc(e, table, rows, P):
        t = (C.c_int64 * max(1, len(table)))(*table)
        return lib.egr_dacmany_encode(e.h, native.ptr(buf), t, rows, P, native.ptr(buf), native.ptr(ibuf), None, st)

    def dec(e, frames, rows, P):
        t = (C.c_int64 * max(1, len(frames)))(*frames)
        return lib.egr_dacmany_decode(e.h, native.ptr(buf), t, rows, P, native.ptr(buf), st)

    def refused(rc, word):
        assert rc in (1, 3) and word in native.last_error(), (rc, native.last_error())        # EGR_ERR_ARG, EGR_ERR_UNSUPPORTED

    for kind, call in ((E.ENCODE, lambda rows, P: enc(eng, [0, 8] * max(rows, 1), rows, P)), (E.DECODE, lambda rows, P: dec(eng, [1] * max(rows, 1), rows, P))):
        refused(call(0, 4), "rows")
        refused(call(-1, 4), "rows")
        refused(call(1, 0), "pad_frames")
        refused(call(1, 2 ** 26 + 1), "quantiser")                                        # rows x pad_frames > 2^26
        refused(call(2, 2 ** 25 + 1), "quantiser")
        for rows, P in ((0, 4), (-1, 4), (1, 0), (1, 2 ** 26 + 1), (2, 2 ** 25 + 1)):
            assert lib.egr_dacmany_workspace_bytes(eng.h, rows, P, kind) == 0
        assert lib.egr_dacmany_workspace_bytes(eng.h, 2, 16, kind) > 0
    assert lib.egr_dacmany_workspace_bytes(eng.h, 2, 16, 2) == 0                          # no such kind
    # rows x padded samples >= 2^31 (the 44 kHz hop, 512: 2^22 frames of one row)
    refused(enc(big, [0, 8], 1, 2 ** 22), "padded samples")
    refused(dec(big, [1], 1, 2 ** 22), "padded samples")
    assert lib.egr_dacmany_workspace_bytes(big.h, 1, 2 ** 22, E.ENCODE) == 0 == lib.egr_dacmany_workspace_bytes(big.h, 1, 2 ** 22, E.DECODE)
    assert lib.egr_dacmany_workspace_bytes(big.h, 1, 2 ** 22 - 1, E.ENCODE) > 0
    # per row
    refused(enc(eng, [0, 8, 0, 0], 2, 4), "n = 0")
    refused(enc(eng, [0, 8, 0, -3], 2, 4), "n = -3")
    refused(enc(eng, [0, 8, -1, 8], 2, 4), "offset")
    refused(enc(eng, [0, 8, 0, 33], 2, 4), "pad_frames")                                  # 33 samples are 5 frames
    assert enc(eng, [0, 8, 0, 32], 2, 4) == native.EGR_OK
    refused(dec(eng, [3, 0], 2, 4), "frames = 0")
    refused(dec(eng, [3, -2], 2, 4), "frames = -2")
    refused(dec(eng, [3, 5], 2, 4), "pad_frames")
    assert dec(eng, [3, 4], 2, 4) == native.EGR_OK
    torch.cuda.synchronize()
    assert big.workspace_held() == 0                                                      # every call on it was refused
    with pytest.raises(ValueError):
        eng.encode_rows(buf, [4090], [8])                                                 # the row leaves x_flat


# ---- 8
def test_encode_many_and_decode_many_over_three_waves(pack, monkeypatch):
    from egregora_amd import dac_engine as E
    from test_gpu_dac_segmented import new_engine
    eng = new_engine("S")
    fs = [K.forward("S", *c) for c in CLIPS["S"]]
    order = (3, 0, 6, 4, 1, 5, 2)                                                         # not sorted by length
    clips = [fs[i]["x"].cuda() for i in order]
    frames = [fs[i]["codes64"].shape[-1] for i in order]
    # 257 x 2, 128, 126, 98 x 2, 42, 2, 1 frames.  A budget of four rows of 272 frames closes the first wave before the rows of 98; a
    # padding share of 0.5 closes the second before the clip of one frame
    monkeypatch.setattr(E, "MAX_PAD_SHARE", 0.5)
    between = lambda kind: repr(sum(eng.many_workspace_bytes(r, 272, kind) for r in (4, 5)) / 2 / 2 ** 30)
    monkeypatch.setenv(E.WORKSPACE_GB_ENV, between(E.ENCODE))
    st = {}
    res = eng.encode_many(clips, stats=st)
    torch.cuda.synchronize()
    waves = st["waves"]
    print("  waves:", waves)
    assert st["alone"] == [] and [w.rows for w in waves] == [4, 4, 1] and [w.pad_frames for w in waves] == [272, 112, 1]
    assert sorted(i for w in waves for i in w.clips) == list(range(len(clips)))
    for (z, codes), x, F in zip(res, clips, frames):
        assert tuple(z.shape) == (x.shape[0], eng.cfg["latent_dim"], F) and tuple(codes.shape) == (x.shape[0], eng.cfg["n_codebooks"], F)
    for w in waves:                                                                       # each clip is its wave's encode_rows call
        offs, lens, pos = [], [], 0
        for i in w.clips:
            c, T = clips[i].shape
            offs += [pos + k * T for k in range(c)]
            lens += [T] * c
            pos += c * T
        z, codes = eng.encode_rows(torch.cat([clips[i].reshape(-1) for i in w.clips]), offs, lens, w.pad_frames)
        r = 0
        for i in w.clips:
            c = clips[i].shape[0]
            assert torch.equal(res[i][0], z[r:r + c, :, :frames[i]]) and torch.equal(res[i][1], codes[r:r + c, :, :frames[i]]), (w, i)
            r += c
    for j, i in enumerate(order):                                                         # input order, and the gates (no ze comes back: the reference's stands in)
        check_encode(f"S clip {i}", fs[i], K.e2e_tau("S", *CLIPS["S"][i]), res[j][0], res[j][1], fs[i]["enc64"][-1].float().cuda())
    sd = {}
    monkeypatch.setenv(E.WORKSPACE_GB_ENV, between(E.DECODE))
    ys = eng.decode_many([z for z, _ in res], stats=sd)
    yc = eng.decode_many([c.long() if j % 2 else c for j, (_, c) in enumerate(res)])
    mixed = eng.decode_many([res[j][0] if j % 2 else res[j][1] for j in range(len(res))])
    torch.cuda.synchronize()
    assert [w.rows for w in sd["waves"]] == [4, 4, 1] and sd["alone"] == []
    for j, (y, F) in enumerate(zip(ys, frames)):
        assert tuple(y.shape) == (clips[j].shape[0], E.decoded_length(eng.cfg, F))
        assert torch.equal(y, yc[j]) and torch.equal(y, mixed[j])                        # codes give the bits of their latents
    for w in sd["waves"]:
        zp = torch.zeros((w.rows, eng.cfg["latent_dim"], w.pad_frames), device="cuda")
        fr, r = [], 0
        for i in w.clips:
            c = clips[i].shape[0]
            zp[r:r + c, :, :frames[i]] = res[i][0]
            fr += [frames[i]] * c
            r += c
        y = eng.decode_rows(zp, fr, w.pad_frames)
        r = 0
        for i in w.clips:
            c = clips[i].shape[0]
            assert torch.equal(ys[i], y[r:r + c, :ys[i].shape[1]]), (w, i)
            r += c
    # a clip above the budget on its own takes the single path
    monkeypatch.setenv(E.WORKSPACE_GB_ENV, repr((eng.many_workspace_bytes(1, 272, E.ENCODE) - 1) / 2 ** 30))
    st2 = {}
    monkeypatch.setattr(E, "SEGMENT_STEP", 32)
    res2 = eng.encode_many([clips[1], clips[3]], stats=st2)                               # 2 x 2051 samples, one sample
    torch.cuda.synchronize()
    assert st2["alone"] == [0] and [w.clips for w in st2["waves"]] == [(1,)]
    check_encode("S alone", fs[0], K.e2e_tau("S", *CLIPS["S"][0]), res2[0][0], res2[0][1], fs[0]["enc64"][-1].float().cuda())
