"""Native DeepFilterNet3 over the whole family of configurations dfn_weights.check_supported accepts (dfn3_torch.MATRIX): each
configuration's synthetic model directory is loaded, run on the device at 1 s stereo and at one odd short length (3 hop + 17), and
held to the cumulative gates of tests/test_gpu_dfn3.py on every stage and on y, and to the local per-stage gates of dfn3_check.py
(every stage restated alone from the device's own inputs).  A configuration load() accepts must build an engine and enhance."""
import gc

import pytest
import torch

import dfn3_check as K
import dfn3_torch as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def models(pack, tmp_path_factory):
    from egregora_amd import native
    native.require_device()
    root = tmp_path_factory.mktemp("dfn_cfg")
    made = {}

    def get(name):
        if name not in made:
            d = root / name / "DeepFilterNet3"
            made[name] = (d,) + R.write_model_dir(d, seed=11, cfg_text=R.config_text(**R.MATRIX[name]))
        return made[name]
    return get


@pytest.mark.parametrize("name", sorted(R.MATRIX))
def test_config_matrix_cumulative_and_local_gates(models, name):
    from egregora_amd import dfn_engine, dfn_weights
    d, cfg, sd = models(name)
    eng = dfn_engine.Dfn3Engine(dfn_weights.load(d), torch.cuda.current_device())     # every accepted config builds and runs
    try:
        for what, n in (("1s x2", 48000), ("short x2", 3 * cfg["hop_size"] + 17)):
            x = K.speechy(len(name) + n % 7, n, 2)
            y = eng.enhance(x.cuda())
            torch.cuda.synchronize()
            assert y.shape == x.shape and bool(torch.isfinite(y).all()), (name, what)
            cum, dev, _ = K.cumulative(eng, x, y, cfg, sd)
            loc = K.local(eng, x, y, cfg, sd, dev)
            print(f"\nDFN3 {name} {what} cumulative (device, fp32):", {k: f"{a:.2e}/{b:.2e}" for k, (a, b) in cum.items()})
            print(f"DFN3 {name} {what} local (rms, rms fp32, max, max fp32):", K.fmt(loc))
    finally:
        del eng
        gc.collect()
