"""Native DeepFilterNet2 over the family of configurations dfn2_weights.check_supported accepts (dfn2_torch.MATRIX2): each
configuration's synthetic model directory is loaded, run on the device at 1 s stereo and at one odd short length (3 hop + 17), and
held to the cumulative gates on every stage and on y and to the local per-stage gates of dfn2_check.py.  A configuration load()
accepts must build an engine and enhance."""
import gc

import pytest
import torch

import dfn2_check as K
import dfn2_torch as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def models(pack, tmp_path_factory):
    from egregora_amd import native
    native.require_device()
    root = tmp_path_factory.mktemp("dfn2_cfg")
    made = {}

    def get(name):
        if name not in made:
            d = root / name / "DeepFilterNet2"
            made[name] = (d,) + R.write_model_dir(d, seed=11, cfg_text=R.config_text(**R.MATRIX2[name]))
        return made[name]
    return get


@pytest.mark.parametrize("name", sorted(R.MATRIX2))
def test_config_matrix_cumulative_and_local_gates(models, name):
    from egregora_amd import dfn2_engine, dfn2_weights
    d, cfg, sd = models(name)
    eng = dfn2_engine.Dfn2Engine(dfn2_weights.load(d), torch.cuda.current_device())
    try:
        for what, n in (("1s x2", 48000), ("short x2", 3 * cfg["hop_size"] + 17)):
            x = K.speechy(len(name) + n % 7, n, 2)
            y = eng.enhance(x.cuda())
            torch.cuda.synchronize()
            assert y.shape == x.shape and bool(torch.isfinite(y).all()), (name, what)
            cum, dev, _ = K.cumulative(eng, x, y, cfg, sd)
            loc = K.local(eng, x, y, cfg, sd, dev)
            print(f"\nDFN2 {name} {what} cumulative (device, fp32):", {k: f"{a:.2e}/{b:.2e}" for k, (a, b) in cum.items()})
            print(f"DFN2 {name} {what} local (rms, rms fp32, max, max fp32):", K.fmt(loc))
    finally:
        del eng
        gc.collect()
