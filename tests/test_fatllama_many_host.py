"""Host side of the Fat-Llama waves (fatllama_many.plan_waves, egr_flmany_query): no GPU needed."""
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent

# (n_in, factor, n_out or 0, channels)
K1 = [(2 * 7919, 1, 0, 2), (14006, 1, 0, 1), (9002, 1, 0, 3), (4 * 1013, 1, 0, 2), (4801, 2, 0, 2)]
K2 = [(48001, 1, 0, 2), (33333, 1, 0, 3), (7919, 1, 0, 1), (101, 1, 0, 2), (3, 1, 0, 2)]
PACKED = (48000, 1, 0, 2)
THREE_LEVEL = (40000003, 1, 0, 1)          # D = N odd: P >= 8e7 > 1024 x 16384


def test_plan_waves_groups_by_kind_and_honours_the_caps(pack):
    from egregora_amd import fatllama_many as fm
    specs = K1 + [PACKED] + K2 + [THREE_LEVEL]
    info = [fm.query([s])["clips"][0] for s in specs]
    assert info[5]["kind"] == 0 and info[11]["levels"] == 3 and info[11]["kind"] == 2
    waves, fallbacks, padding = fm.plan_waves(specs, slack=100.0)
    assert 5 in fallbacks and 11 in fallbacks                      # a packed length and a three-level length go one by one
    assert sorted([i for w in waves for i in w] + fallbacks) == list(range(len(specs)))          # every clip once
    for w, pad in zip(waves, padding):
        assert len({info[i]["kind"] for i in w}) == 1 and len(w) >= 2           # kinds never mix, nobody is alone
        assert info[w[0]]["D"] == max(info[i]["D"] for i in w)                  # the largest clip leads: its own P is the wave's
        q = fm.query([specs[i] for i in w])
        assert q["wave"] and q["P"] == info[w[0]]["P"]
        own = sum(c["states"] * info[i]["P"] for c, i in zip(q["clips"], w))
        assert abs(pad - q["states"] * q["P"] / own) < 1e-12
        assert q["bytes"] == fm.wave_bytes(q["P"], q["states"], q["distinct"], q["rows"])
    assert sorted(map(sorted, waves)) == [[0, 1, 2, 3, 4], [6, 7, 8, 9, 10]]
    # the padding cap: at the default slack the small clips do not ride on the largest clip's P
    waves, fallbacks, padding = fm.plan_waves(specs)
    assert all(p <= 1.15 + 1e-12 for p in padding) and waves == [[0, 1], [4, 2]] and fallbacks == [3, 5, 6, 7, 8, 9, 10, 11]
    # the rows cap: five channel rows at most -> the stereo / mono / triple clips split up
    waves, _, _ = fm.plan_waves(K1, slack=100.0, max_rows=5)
    assert all(sum(K1[i][3] for i in w) <= 5 for w in waves) and len(waves) == 2
    # the bytes cap: exactly what the two largest clips need lets them share a wave and nobody else join; one byte less does not
    cap = fm.query([K1[0], K1[1]])["bytes"]
    waves, _, _ = fm.plan_waves(K1, slack=100.0, max_bytes=cap)
    assert waves[0] == [0, 1] and all(fm.query([K1[i] for i in w])["bytes"] <= cap for w in waves)
    waves, _, _ = fm.plan_waves(K1, slack=100.0, max_bytes=cap - 1)
    assert all(fm.query([K1[i] for i in w])["bytes"] < cap for w in waves) and not any({0, 1} <= set(w) for w in waves)
    # single_only (a legacy chirp-z run, a variant the wave does not take): everything one by one; a lone clip too
    assert fm.plan_waves(K1, single_only=True) == ([], [0, 1, 2, 3, 4], [])
    assert fm.plan_waves(K1[:1]) == ([], [0], [])


def test_query_geometry_is_the_single_plans(pack):
    from egregora_amd import fatllama_engine as fe, fatllama_many as fm
    for specs in (K1, K2, K1[:1], [(524282, 1, 0, 2), (471860, 1, 0, 2), (314570, 1, 0, 2)]):
        q = fm.query(specs)
        assert q["wave"] and q["levels"] == 2 and q["L"] * q["nc"] == q["P"]
        big = max(range(len(specs)), key=lambda i: q["clips"][i]["D"])
        assert q["P"] == q["clips"][big]["P"]                      # P of the wave = what the largest D gets alone
        TC, nc = q["TC"], q["nc"]
        assert nc % (2 * TC) == 0
        for st in q["state_rows"]:
            c, D = q["clips"][st["clip"]], st["D"]
            assert D == c["D"] and q["P"] >= 2 * D - 1
            assert (D + 2 * st["s"]) % (2 * TC) == (2 * TC - 1 if D % 2 else 0) and 0 <= st["s"] < TC
            Dr = D + 2 * st["s"]
            assert (st["iDr"], st["cDr"]) == divmod(Dr, nc)
            assert st["G"] == nc // (2 * TC) + (0 if D % 2 else 1)
            assert st["c0"] == ((st["cDr"] + 1) // 2 if D % 2 else st["cDr"] // 2) and st["c0"] % TC == 0
            assert st["channels"] == (1 if q["kind"] == 1 else min(2, specs[st["clip"]][3] - 2 * (q["state_rows"].index(st) - c["state0"])))
            if c["P"] == q["P"]:                                   # the plan this clip gets alone is the wave's
                pi = fe.plan_info(specs[st["clip"]][0], specs[st["clip"]][1])
                assert (pi["M"], pi["M1"], pi["M2"], pi["TC"], pi["D"], pi["chirpz_kind"]) == (q["P"], q["L"], nc, TC, D, q["kind"])
        assert q["gpx"] == max(-(-st["G"] // 8) for st in q["state_rows"])
        assert q["rows"] == sum(s[3] for s in specs) and q["x_floats"] == sum(s[0] * s[3] for s in specs)
        assert q["out_floats"] == sum(s[3] * (c["N"] + c["N"] % 2) for s, c in zip(specs, q["clips"]))


def test_query_names_the_clip_that_cannot_join(pack):
    from egregora_amd import fatllama_many as fm
    for specs, bad, why in (([K1[0], PACKED], 1, 1), ([K1[0], K2[0]], 1, 3), ([THREE_LEVEL, K2[0]], 0, 2), ([(4801, 1, 0, 600)] * 2, 1, 4)):
        q = fm.query(specs)
        assert not q["wave"] and (q["bad_clip"], q["reason"]) == (bad, why) and q["state_rows"] == []
    q = fm.query([(4801, 1, 7001, 2), K2[0]])                      # an explicit output length (ratio_then_int)
    assert q["wave"] and q["clips"][0]["N"] == 7001 and q["clips"][0]["kind"] == 2


def test_batch_node_is_registered_only_on_request(pack):
    code = ("import sys; sys.path.insert(0, %r); from packload import load_pack; p = load_pack(); "
            "print('EgregoraFatLlamaGPUBatch' in p.NODE_CLASS_MAPPINGS)" % str(ROOT))
    for val, want in ((None, "False"), ("1", "True")):
        env = {k: v for k, v in os.environ.items() if k != "EGREGORA_FATLLAMA_BATCH_NODES"}
        if val:
            env["EGREGORA_FATLLAMA_BATCH_NODES"] = val
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True).stdout.strip()
        assert out.splitlines()[-1] == want, (val, out)


def test_abi_is_still_5(pack):
    from egregora_amd import native
    assert native.lib().egr_abi_version() == native.ABI_VERSION == 5
    assert {"egr_flmany_query", "egr_flmany_create", "egr_flmany_enhance", "egr_flmany_destroy"} <= set(native.SIGNATURES)
