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


def test_config_text_replaces_named_keys_and_refuses_unknown_ones():
    txt = R.config_text(hop_size=240, conv_kernel=(2, 3), pad_mode="none")
    assert "hop_size = 240\n" in txt and "conv_kernel = 2,3\n" in txt and "pad_mode = none\n" in txt
    assert "convt_kernel = 1,3\n" in txt and "conv_kernel_inp = 3,3\n" in txt          # prefixes of a key are other keys
    assert R.config_text() == R.CONFIG_INI
    with pytest.raises(KeyError, match="no_such_key"):
        R.config_text(no_such_key=1)


def _model_dir(tmp_path, overrides, seed=2):
    d = tmp_path / "DeepFilterNet3"
    cfg, sd = R.write_model_dir(d, seed=seed, cfg_text=R.config_text(**overrides))
    return d, cfg, sd


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("overrides", [{}, R.MATRIX["cornerB"], R.MATRIX["conv_kernel_2_3"]], ids=["default", "cornerB", "conv_kernel_2_3"])
def test_restatement_stages_compose_to_enhance_exactly(pack, tmp_path, overrides, dtype):
    """The per-stage functions the local gates call, chained by hand, give enhance()'s stage dict and output bit for bit."""
    d, cfg, sd = _model_dir(tmp_path, overrides)
    x = 0.3 * torch.randn(2, 3 * cfg["hop_size"] + 4801, generator=torch.Generator().manual_seed(4))
    y, st = R.enhance(x, cfg, sd, dtype, stages=True)
    net = R.Net(cfg, sd, dtype)
    spec = R.analysis(x.to(dtype), cfg)
    fe, fs = R.shifted_features(spec, cfg)
    e = [net.e0(fe)]
    for i in (1, 2, 3):
        e.append(net.e_next(i, e[-1]))
    c0 = net.c0(fs)
    grus = [net.gru_enc(e[3], c0)]
    emb = net.emb(grus[0])
    for k in range(cfg["emb_num_layers"] - 1):
        grus.append(net.erb_gru(k, emb if k == 0 else grus[-1]))
    mask = net.mask(grus[-1], *e)
    for k in range(cfg["df_num_layers"]):
        grus.append(net.df_gru(k, emb if k == 0 else grus[-1]))
    coefs = net.coefs(grus[-1], emb, c0)
    spec_e = net.assemble(spec, mask, coefs)
    mine = dict(spec=spec, feat_erb=fe, feat_spec=fs, e0=e[0], e1=e[1], e2=e[2], e3=e[3], c0=c0, emb=emb, mask=mask, coefs=coefs,
                spec_e=spec_e, y=R.synthesis(spec_e, cfg, x.shape[1]))
    assert set(mine) | {"grus"} == set(st)
    for k, v in mine.items():
        assert v.dtype == st[k].dtype and torch.equal(v, st[k]), k
    assert len(grus) == len(st["grus"]) and all(torch.equal(a, b) for a, b in zip(grus, st["grus"]))
    assert torch.equal(mine["y"], y)


def test_lookahead_beyond_the_last_frame_gives_zero_features(pack, tmp_path):
    """DfNet.pad_feat with conv_lookahead >= nF shifts every frame out: all-zero features, as k_dfn_norm_scan writes them."""
    d, cfg, sd = _model_dir(tmp_path, dict(fft_size=4096, hop_size=2048, conv_lookahead=3))
    x = 0.3 * torch.randn(1, 479, generator=torch.Generator().manual_seed(5))
    assert (479 + 4096) // 2048 == 2
    for dt in (torch.float64, torch.float32):
        y, st = R.enhance(x, cfg, sd, dt, stages=True)
        assert not st["feat_erb"].any() and not st["feat_spec"].any() and st["feat_erb"].shape[2] == 2
        assert bool(torch.isfinite(y).all()) and y.shape == x.shape
    fs = torch.arange(2 * 3 * 4 * 5, dtype=torch.float64).reshape(2, 3, 4, 5)
    assert torch.equal(R._shift(fs, 1)[:, :, :3], fs[:, :, 1:]) and not R._shift(fs, 1)[:, :, 3].any()
    assert not R._shift(fs, 4).any() and not R._shift(fs, 9).any() and torch.equal(R._shift(fs, 0), fs)


@pytest.mark.parametrize("name", sorted(R.REJECTED))
def test_unsupported_configs_raise_at_load_with_the_listing_error(pack, tmp_path, name):
    """Everything egr_dfn3_create / its run() / upstream cannot build is refused when the directory is loaded, never later."""
    from egregora_amd import dfn_weights as W
    overrides, fragment = R.REJECTED[name]
    d, cfg, sd = _model_dir(tmp_path, overrides)
    with pytest.raises(RuntimeError, match="not supported by the native forward pass") as e:
        W.load(d)
    assert fragment in str(e.value), (fragment, str(e.value))


def test_convt_weights_take_their_shape_from_convt_kernel(pack, tmp_path):
    """erb_dec.convt2 / convt1 are shaped by convt_kernel (upstream's tconv_layer), not by conv_kernel."""
    from egregora_amd import dfn_weights as W
    d, cfg, sd = _model_dir(tmp_path, dict(conv_kernel="2,3"))
    assert tuple(sd["erb_dec.convt2.0.weight"].shape) == tuple(sd["erb_dec.convt1.0.weight"].shape) == (64, 1, 1, 3)
    assert tuple(sd["erb_dec.convt3.0.weight"].shape) == tuple(sd["enc.erb_conv1.0.weight"].shape) == (64, 1, 2, 3)
    m = W.load(d)
    assert m.packed().size == sum(int(math.prod(sd[n].shape)) if k == "w" else 2 * sd[n + ".weight"].numel()
                                  for n, k in W.pack_order(cfg))
    bad = dict(sd)                                      # the conv_kernel-shaped tensor the old key table asked for is refused
    bad["erb_dec.convt2.0.weight"] = torch.zeros(64, 1, 2, 3)
    with pytest.raises(RuntimeError, match=r"erb_dec.convt2.0.weight: checkpoint \(64, 1, 2, 3\) != table \(64, 1, 1, 3\)"):
        W.validate(bad, cfg)


@pytest.mark.parametrize("name", sorted(R.MATRIX))
def test_every_matrix_config_loads_and_runs_through_the_restatement(pack, tmp_path, name):
    """The configurations tests/test_gpu_dfn3_configs.py runs on the device load, pack to the size egr_dfn3_create derives, and run
    through the restatement in both dtypes at an odd short length (finite, agreeing to float32 precision)."""
    from egregora_amd import dfn_engine, dfn_weights as W
    d, cfg, sd = _model_dir(tmp_path, R.MATRIX[name])
    m = W.load(d)
    c = dfn_engine.config_c(m)
    assert c.convt_kf == 3 and c.kf % 2 == 1 and c.kf_inp % 2 == 1
    assert sum(m.widths) == cfg["fft_size"] // 2 + 1 and len(m.widths) == cfg["nb_erb"]
    x = 0.3 * torch.randn(2, 3 * cfg["hop_size"] + 17, generator=torch.Generator().manual_seed(6))
    y64, s64 = R.enhance(x, cfg, sd, torch.float64, stages=True)
    y32 = R.enhance(x, cfg, sd, torch.float32)
    assert y64.shape == x.shape and bool(torch.isfinite(y64).all()) and bool(torch.isfinite(y32).all())
    assert len(s64["grus"]) == cfg["emb_num_layers"] + cfg["df_num_layers"]
    assert float((y32.double() - y64).norm()) <= 1e-4 * float(y64.norm()) + 1e-12
