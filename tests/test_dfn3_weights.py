"""DeepFilterNet3 model directories on the CPU (dfn_weights.py): config.ini parsing, the layer table the checkpoint's shapes imply,
the key table (dfn3_keymap.json) failing loudly with the full list, the discovery order, and the node's unchanged error when no
backend exists.  The real checkpoint is not in the test images: the directory is synthetic (tests/dfn3_torch.py)."""
import math

import pytest
import torch

import dfn3_torch as R

TODAYS_ERROR = ("DeepFilterNet (python package `df`) is not installed; this pack runs the stage around the model on the GPU but does "
                "not re-implement the upstream network (register one with egregora_audio_enhance_extras.set_enhancer).")


@pytest.fixture()
def model_dir(pack, tmp_path):
    d = tmp_path / "DeepFilterNet3"
    cfg, sd = R.write_model_dir(d, seed=1)
    return d, cfg, sd


def test_config_ini_is_read_in_full(model_dir):
    from egregora_amd import dfn_weights as W
    d, cfg, _ = model_dir
    assert cfg["sr"] == 48000 and cfg["fft_size"] == 960 and cfg["hop_size"] == 480 and cfg["nb_erb"] == 32 and cfg["nb_df"] == 96
    assert cfg["conv_kernel_inp"] == (3, 3) and cfg["conv_kernel"] == (1, 3) and cfg["df_gru_skip"] == "groupedlinear"
    assert cfg["conv_depthwise"] is True and cfg["enc_concat"] is False and cfg["pad_mode"] == "input_specf"
    assert set(cfg) == {k for _, k, _ in W.PARAMS}
    assert W.norm_alpha(cfg) == 0.99                                  # exp(-0.01) rounded to 3 decimals
    widths = W.erb_widths(48000, 960, 32, 2)
    assert sum(widths) == 481 and len(widths) == 32 and min(widths) == 2 and widths[:13] == [2] * 13
    # a config without a key the forward pass reads is refused, listing every absent key
    txt = R.CONFIG_INI.replace("df_order = 5\n", "").replace("lin_groups = 16\n", "")
    (d / "config.ini").write_text(txt)
    with pytest.raises(RuntimeError) as e:
        W.parse_config(d / "config.ini")
    assert "df_order: missing" in str(e.value) and "lin_groups: missing" in str(e.value)


def test_layer_table_from_shapes_equals_the_config(model_dir):
    from egregora_amd import dfn_weights as W
    d, cfg, sd = model_dir
    lt = W.layer_table(sd)
    assert lt["emb_num_layers"] == 3 and lt["df_num_layers"] == 2 and lt["emb_hidden_dim"] == lt["df_hidden_dim"] == 256
    assert all(cfg[k] == v for k, v in lt.items()), {k: (v, cfg[k]) for k, v in lt.items() if cfg[k] != v}
    m = W.load(d)
    assert m.packed().size == sum(int(math.prod(sd[n].shape)) if k == "w" else 2 * sd[n + ".weight"].numel()
                                  for n, k in W.pack_order(cfg))
    # a config that disagrees with the shapes is refused
    (d / "config.ini").write_text(R.CONFIG_INI.replace("df_num_layers = 2", "df_num_layers = 3"))
    with pytest.raises(RuntimeError, match="missing tensors"):
        W.load(d)


def test_bad_checkpoints_raise_with_the_full_list(model_dir):
    from egregora_amd import dfn_weights as W
    d, cfg, sd = model_dir
    bad = dict(sd)
    bad["enc.emb_gru.gru.weight_hh_l7"] = bad.pop("enc.emb_gru.gru.weight_hh_l0")           # renamed
    del bad["erb_dec.convt2.1.weight"]                                                   # missing
    bad["df_dec.df_out.0.weight"] = torch.zeros(16, 16, 59)                              # reshaped
    bad["enc.df_conv0.2.weight"] = torch.zeros(64, 32, 1, 1)                             # reshaped
    with pytest.raises(RuntimeError) as e:
        W.validate(bad, cfg)
    msg = str(e.value)
    for s in ("unmapped tensors (1)", "enc.emb_gru.gru.weight_hh_l7", "missing tensors (2)", "enc.emb_gru.gru.weight_hh_l0",
              "erb_dec.convt2.1.weight", "shape mismatches (2)", "df_dec.df_out.0.weight", "enc.df_conv0.2.weight"):
        assert s in msg, (s, msg)
    torch.save(bad, d / "checkpoints" / "model_120.ckpt.best")
    with pytest.raises(RuntimeError, match="unmapped tensors"):
        W.load(d)
    # an ERB bank that is not the one config.ini implies
    sd2 = dict(sd)
    sd2["erb_fb"] = torch.roll(sd["erb_fb"], 1, 0)
    with pytest.raises(RuntimeError, match="ERB bank"):
        W.validate(sd2, cfg)
    with pytest.raises(RuntimeError, match="not supported"):
        W.check_supported(dict(cfg, enc_concat=True))


def test_discovery_order(pack, tmp_path, monkeypatch):
    from egregora_amd import dfn_weights as W
    root = tmp_path / "ComfyUI" / "custom_nodes" / "pack"
    monkeypatch.setattr(W, "pack_root", lambda: root)
    monkeypatch.setenv("HOME", str(tmp_path / "home"))
    monkeypatch.delenv("EGREGORA_DFN_MODEL_DIR", raising=False)
    q2a = tmp_path / "ComfyUI" / "models" / "audio" / "deepfilternet" / "DeepFilterNet3"
    q2b = tmp_path / "models" / "audio" / "deepfilternet" / "DeepFilterNet3"
    cache = tmp_path / "home" / ".cache" / "DeepFilterNet" / "DeepFilterNet3"
    env = tmp_path / "elsewhere"
    assert W.candidate_dirs() == [q2a, q2b, cache]
    assert W.discover() is None
    R.write_model_dir(cache)
    assert W.discover() == cache
    R.write_model_dir(q2b)
    assert W.discover() == q2b
    R.write_model_dir(q2a)
    assert W.discover() == q2a
    monkeypatch.setenv("EGREGORA_DFN_MODEL_DIR", str(env))
    assert W.candidate_dirs()[0] == env and W.discover() == q2a          # not a model directory yet
    R.write_model_dir(env, epoch=7)
    (env / "checkpoints" / "model_12.ckpt.best").write_bytes((env / "checkpoints" / "model_7.ckpt.best").read_bytes())
    assert W.discover() == env and W.checkpoint_file(env).name == "model_12.ckpt.best"
    assert W.discover("DeepFilterNet2") is None                          # only DeepFilterNet3 is served natively


def test_node_without_any_backend_raises_todays_error(pack, tmp_path, monkeypatch):
    from egregora_amd import dfn_weights as W
    from egregora_amd import egregora_audio_enhance_extras as X
    monkeypatch.setattr(W, "pack_root", lambda: tmp_path / "a" / "b" / "pack")
    monkeypatch.setenv("HOME", str(tmp_path / "home"))
    monkeypatch.delenv("EGREGORA_DFN_MODEL_DIR", raising=False)
    node = pack.NODE_CLASS_MAPPINGS["Egregora_DeepFilterNet_Denoise"]()
    for model in ("DeepFilterNet2", "DeepFilterNet3"):
        with pytest.raises(RuntimeError) as e:
            node._enhance(torch.zeros(1, 960), model, "cpu")
        assert str(e.value) == TODAYS_ERROR
    # a DeepFilterNet3 directory does not serve the DeepFilterNet2 choice
    R.write_model_dir(tmp_path / "m")
    monkeypatch.setenv("EGREGORA_DFN_MODEL_DIR", str(tmp_path / "m"))
    with pytest.raises(RuntimeError) as e:
        node._enhance(torch.zeros(1, 960), "DeepFilterNet2", "cpu")
    assert str(e.value) == TODAYS_ERROR
    assert X._ENHANCER is None


def test_restatement_analysis_synthesis_is_the_identity(pack):
    """libdf's analysis / synthesis with enhance's pad and trim reconstruct the input (the Vorbis window is power-complementary)."""
    import tempfile
    from pathlib import Path
    from egregora_amd import dfn_weights as W
    with tempfile.TemporaryDirectory() as t:
        p = Path(t) / "config.ini"
        p.write_text(R.CONFIG_INI)
        cfg = W.parse_config(p)
    x = torch.randn(2, 4801, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    y = R.synthesis(R.analysis(x, cfg), cfg, x.shape[1])
    assert float((y - x).abs().max()) < 1e-6 * float(x.abs().max())          # w^2 + shifted w^2 = 1 up to the float32 window
