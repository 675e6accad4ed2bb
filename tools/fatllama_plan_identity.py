"""Device identity record of the Fat-Llama host path (profiles/fatllama_plan.md): run once per library in a fresh process

    python tools/fatllama_plan_identity.py OUT.json                      # the library of this tree
    EGREGORA_AMD_LIB=/path/to/other/libegregora_amd.so python tools/fatllama_plan_identity.py OTHER.json

and compare the two files byte for byte.  Only the public Python API is used, plus egr_fatllama_kernel_times3, egr_band_filter,
egr_spectral_gain and egr_gcc_phat through native.lib().  The file holds the SHA-256 of enhance_device's output for every parameter
tuple of the tests named below, with graph replay on and off (EGR_FL_GRAPH, read when a plan is built) and with EGR_FL_WL and
EGR_FL_SCHED each on and off (one hash per tuple where all eight settings give the same bits); the launch counts of kernel_times3
after a profiled two-level, three-level and chirp-z run; and the hashes of the single-pass outputs on a packed and a chirp-z length.
Nothing in the file names the library it came from."""
import ctypes as C
import hashlib
import json
import os
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from packload import load_pack  # noqa: E402

load_pack()
from egregora_amd import fatllama_engine as fe, native  # noqa: E402
import test_gpu_fatllama as T  # noqa: E402
import test_gpu_fatllama_chirpz as TZ  # noqa: E402

FLAGS = dict(normalize=False, autoscale=False, pcm_in=False, node_post=False)


def sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


def cases(test):
    """The parameter tuples of a test, from its own parametrize marks (two marks: their product, the decorator nearest the function first)."""
    lists = [[v if isinstance(v, tuple) else (v,) for v in m.args[1]] for m in test.pytestmark if m.name == "parametrize"]
    return [a + b for a in lists[0] for b in lists[1]] if len(lists) == 2 else lists[0]


def tuples():
    """(test, id, x, factor, iters, thr, keywords of enhance_device) as the tests build them."""
    for C_, n, f, iters, thr in T.CASES:
        yield "test_loop_matches_oracle", (C_, n, f, iters, thr), T.synth(C_, n, seed=n + f), f, iters, thr, {}
    for C_, n, iters in cases(T.test_graph_replay_equals_plain_launches):
        yield "test_graph_replay_equals_plain_launches", (C_, n, iters), T.synth(C_, n, seed=n + iters), 1, iters, 0.6, {}
    for n, split in cases(T.test_three_level_plan_matches_oracle):
        yield "test_three_level_plan_matches_oracle", (n, split), T.synth(2, n, seed=n), 1, 4, 0.6, {"split": split}
    for C_, n, f, iters, variant, _, thr, scale in cases(T.test_threshold_and_interpolation_variants_match_the_oracle):
        yield ("test_threshold_and_interpolation_variants_match_the_oracle", (variant, thr, scale, C_, n, f, iters),
               T.synth(C_, n, seed=n + f + len(variant), scale=scale), f, iters, thr, {"variant": variant})
    for C_, n, iters in cases(T.test_carried_maximum_at_every_graph_and_ring_boundary):
        yield ("test_carried_maximum_at_every_graph_and_ring_boundary", (C_, n, iters), T.synth(C_, n, seed=n + iters, scale=8000.0), 1, iters,
               0.03, {"variant": "relative,soft"})
    for C_, n, iters in cases(TZ.test_chirpz_graph_replay_equals_plain_launches):
        yield "test_chirpz_graph_replay_equals_plain_launches", (C_, n, iters), T.synth(C_, n, seed=n + iters), 1, iters, 0.6, {}


def single_passes(n):
    """Hashes of egr_band_filter, egr_spectral_gain and egr_gcc_phat on one channel of n samples (or the error code where the plan kind
    does not serve the call: the latter two need a packed-real plan, GCC-PHAT one of 2^k samples)."""
    L = native.lib()
    x = torch.from_numpy(T.synth(1, n, seed=n)).cuda()
    plan = fe._plan(n, 1, 1, 0)
    out = {}
    y = torch.zeros_like(x)
    rc = L.egr_band_filter(C.c_void_p(plan), native.ptr(x), n // 8, native.ptr(y), native.stream_ptr())
    out["egr_band_filter"] = sha(y) if rc == 0 else rc
    gain = torch.linspace(0.0, 1.0, n // 2 + 1, device="cuda").repeat(1, 1).contiguous()
    y = torch.zeros_like(x)
    rc = L.egr_spectral_gain(C.c_void_p(plan), native.ptr(x), native.ptr(gain), native.ptr(y), native.stream_ptr())
    out["egr_spectral_gain"] = sha(y) if rc == 0 else rc
    m = n // 2
    a, b = x[0, :m // 2].contiguous(), torch.roll(x[0, :m // 2], 5).contiguous()
    work = torch.zeros(4 * m, dtype=torch.float32, device="cuda")
    out4 = torch.zeros(4, dtype=torch.float32, device="cuda")
    rc = L.egr_gcc_phat(C.c_void_p(plan), native.ptr(a), a.numel(), native.ptr(b), b.numel(), 16, native.ptr(work), native.ptr(out4), native.stream_ptr())
    out["egr_gcc_phat"] = sha(out4) if rc == 0 else rc
    return out


def main(path):
    native.require_device()
    torch.cuda.set_device(0)
    rec = {"kernel_times3_launches": {}, "single_pass": {}}          # and, per test, enhance_device's output per parameter tuple
    for wl, sched in [("1", "1"), ("0", "1"), ("1", "0"), ("0", "0")]:
        for graph in ("1", "0"):
            os.environ.update({"EGR_FL_WL": wl, "EGR_FL_SCHED": sched, "EGR_FL_GRAPH": graph})
            fe.release_plans()                      # the switches are read when a plan is built
            for test, ident, x, f, iters, thr, kw in tuples():
                y = fe.enhance_device(torch.from_numpy(x).cuda(), f, iters, thr, **FLAGS, **kw)
                rec.setdefault(test, {}).setdefault(json.dumps(ident), {})[f"wl={wl} sched={sched} graph={graph}"] = sha(y)
    for k in ("EGR_FL_WL", "EGR_FL_SCHED", "EGR_FL_GRAPH"):
        os.environ.pop(k)
    runs = 0
    for test, body in rec.items():                      # one hash where all eight settings of the switches agree (most lengths have no
        for k, v in body.items():                       # kernel that the switches select), else the hash per setting
            runs += len(v)
            if len(set(v.values())) == 1:
                body[k] = next(iter(v.values()))
    fe.release_plans()
    for name, n, kw in [("two_level", 9600, {}), ("three_level", 48000, {"split": (20, 24, 50)}), ("chirpz", 4801, {})]:
        x = torch.from_numpy(T.synth(2, n, seed=n)).cuda()
        fe.enhance_device(x, 1, 30, 0.6, **FLAGS, profile=True, **kw)
        plan = fe._plan(n, 2, 1, 0, 0, 0, kw.get("split"), None)
        ms, cnt = (C.c_double * 3)(), (C.c_int64 * 3)()
        native.check(native.lib().egr_fatllama_kernel_times3(C.c_void_p(plan), ms, cnt), "egr_fatllama_kernel_times3")
        rec["kernel_times3_launches"][name] = list(cnt)
    fe.release_plans()
    rec["single_pass"]["packed 65536"] = single_passes(65536)
    rec["single_pass"]["three-level 19200000"] = {k: v for k, v in single_passes(19200000).items() if k != "egr_gcc_phat"}
    rec["single_pass"]["chirpz 4801"] = single_passes(4801)
    fe.release_plans()
    Path(path).parent.mkdir(parents=True, exist_ok=True)
    lines = [f' {json.dumps(sec)}: {{\n' + ",\n".join(f"  {json.dumps(k)}: {json.dumps(v, sort_keys=True)}" for k, v in sorted(body.items())) + "\n }"
             for sec, body in sorted(rec.items())]          # one line per entry
    Path(path).write_text("{\n" + ",\n".join(lines) + "\n}\n")
    print(f"{runs} outputs hashed -> {path}")


if __name__ == "__main__":
    main(sys.argv[1])
