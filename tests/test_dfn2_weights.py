"""DeepFilterNet2 model directories on the CPU (dfn2_weights.py): config.ini parsing, the layer table the checkpoint's shapes imply,
the key table (dfn2_keymap.json) failing loudly with the full list, discovery (only `[train] model = deepfilternet2` directories
serve DeepFilterNet2), the supported range, and the restatement tests/dfn2_torch.py itself (GroupedGRU / GroupedLinear semantics,
stages composing to enhance, float32 keeping far inside the GPU gates' cap on every MATRIX2 entry).  The real checkpoint is not in
the test images: the directories are synthetic."""
import math

import pytest
import torch

import dfn2_torch as R
import dfn3_torch as R3
from dfn3_check import CAP, rel, speechy

TODAYS_ERROR = ("DeepFilterNet (python package `df`) is not installed; this pack runs the stage around the model on the GPU but does "
                "not re-implement the upstream network (register one with egregora_audio_enhance_extras.set_enhancer).")


def _model_dir(tmp_path, overrides=None, seed=2, name="DeepFilterNet2"):
    d = tmp_path / name
    cfg, sd = R.write_model_dir(d, seed=seed, cfg_text=R.config_text(**(overrides or {})))
    return d, cfg, sd


def _packed_size(W, sd, cfg):
    return sum(int(math.prod(sd[n].shape)) if k == "w" else 2 * sd[n + ".weight"].numel() for n, k in W.pack_order(cfg))


def test_config_ini_is_read_in_full(pack, tmp_path):
    from egregora_amd import dfn2_weights as W
    d, cfg, _ = _model_dir(tmp_path)
    assert cfg["gru_type"] == "grouped" and cfg["gru_groups"] == 8 and cfg["lin_groups"] == 8 and cfg["group_shuffle"] is False
    assert cfg["df_output_layer"] == "groupedlinear" and cfg["dfop_method"] == "real_unfold" and cfg["df_gru_skip"] == "none"
    assert cfg["conv_lookahead"] == 2 and cfg["emb_hidden_dim"] == cfg["df_hidden_dim"] == 256 and cfg["conv_kernel_inp"] == (3, 3)
    assert set(cfg) == {k for _, k, _ in W.PARAMS} and "pad_mode" not in cfg and "convt_kernel" not in cfg
    txt = R.CONFIG_INI.replace("gru_groups = 8\n", "").replace("dfop_method = real_unfold\n", "").replace("df_order = 5\n", "")
    (d / "config.ini").write_text(txt)
    with pytest.raises(RuntimeError) as e:
        W.parse_config(d / "config.ini")
    for k in ("gru_groups: missing", "dfop_method: missing", "df_order: missing"):
        assert k in str(e.value), (k, str(e.value))


def test_layer_table_from_shapes_equals_the_config(pack, tmp_path):
    from egregora_amd import dfn2_weights as W
    for ov in ({}, R.MATRIX2["cornerA"], R.MATRIX2["cornerB"], R.MATRIX2["df_out_linear"]):
        d, cfg, sd = _model_dir(tmp_path / str(len(ov)), ov)
        lt = W.layer_table(sd)
        for k in ("conv_ch", "conv_kernel", "conv_kernel_inp", "fft_size", "nb_erb", "nb_df", "emb_hidden_dim", "df_hidden_dim",
                  "emb_num_layers", "df_num_layers", "gru_groups", "lin_groups", "df_order", "df_pathway_kernel_size_t", "df_gru_skip",
                  "df_output_layer"):
            assert lt[k] == cfg[k], (ov, k, lt[k], cfg[k])
        m = W.load(d)
        assert m.packed().size == _packed_size(W, sd, cfg)
    d, cfg, sd = _model_dir(tmp_path / "x")
    (d / "config.ini").write_text(R.config_text(gru_groups=4))
    with pytest.raises(RuntimeError, match="gru_groups: shapes say 8, config.ini says 4"):
        W.load(d)


def test_bad_checkpoints_raise_with_the_full_list(pack, tmp_path):
    from egregora_amd import dfn2_weights as W
    d, cfg, sd = _model_dir(tmp_path)
    bad = dict(sd)
    bad["enc.emb_gru.grus.0.layers.9.weight_hh_l0"] = bad.pop("enc.emb_gru.grus.0.layers.3.weight_hh_l0")     # renamed
    del bad["df_dec.df_fc_a.0.bias"]                                                                           # missing
    bad["erb_dec.fc_emb.0.layers.2.weight"] = torch.zeros(64, 31)                                              # reshaped
    with pytest.raises(RuntimeError) as e:
        W.validate(bad, cfg)
    msg = str(e.value)
    for s in ("unmapped tensors (1)", "enc.emb_gru.grus.0.layers.9.weight_hh_l0", "missing tensors (2)",
              "enc.emb_gru.grus.0.layers.3.weight_hh_l0", "df_dec.df_fc_a.0.bias", "shape mismatches (1)",
              "erb_dec.fc_emb.0.layers.2.weight: checkpoint (64, 31) != table (64, 32)"):
        assert s in msg, (s, msg)
    torch.save(bad, d / "checkpoints" / "model_96.ckpt.best")
    with pytest.raises(RuntimeError, match="unmapped tensors"):
        W.load(d)
    sd2 = dict(sd)
    sd2["mask.erb_inv_fb"] = torch.roll(sd["mask.erb_inv_fb"], 1, 1)
    with pytest.raises(RuntimeError, match="ERB bank"):
        W.validate(sd2, cfg)
    # a DeepFilterNet3 state dict is not a DeepFilterNet2 one
    sd3 = R3.synthetic_state_dict(R3.W().parse_config(_write(tmp_path / "c3.ini", R3.CONFIG_INI)))
    with pytest.raises(RuntimeError, match="unmapped tensors"):
        W.validate(sd3, cfg)


def _write(p, txt):
    p.write_text(txt)
    return p


def test_discovery_order_and_model_identity(pack, tmp_path, monkeypatch):
    from egregora_amd import dfn2_weights as W2
    from egregora_amd import dfn_weights as W
    root = tmp_path / "ComfyUI" / "custom_nodes" / "pack"
    monkeypatch.setattr(W, "pack_root", lambda: root)
    monkeypatch.setenv("HOME", str(tmp_path / "home"))
    monkeypatch.delenv("EGREGORA_DFN_MODEL_DIR", raising=False)
    q2a = tmp_path / "ComfyUI" / "models" / "audio" / "deepfilternet" / "DeepFilterNet2"
    q2b = tmp_path / "models" / "audio" / "deepfilternet" / "DeepFilterNet2"
    cache = tmp_path / "home" / ".cache" / "DeepFilterNet" / "DeepFilterNet2"
    env = tmp_path / "elsewhere"
    assert W.candidate_dirs("DeepFilterNet2") == [q2a, q2b, cache]
    assert W2.discover() is None
    R.write_model_dir(cache)
    assert W2.discover() == cache
    R.write_model_dir(q2b)
    assert W2.discover() == q2b
    # a directory in a DeepFilterNet2 place whose config.ini names another model is skipped
    R.write_model_dir(q2a, cfg_text=R.CONFIG_INI.replace("model = deepfilternet2", "model = deepfilternet3"))
    assert W2.discover() == q2b
    with pytest.raises(RuntimeError, match="not 'deepfilternet2'"):
        W2.load(q2a)
    R.write_model_dir(q2a)
    assert W2.discover() == q2a
    # EGREGORA_DFN_MODEL_DIR first, but a DeepFilterNet3 directory there never serves DeepFilterNet2 (and vice versa)
    monkeypatch.setenv("EGREGORA_DFN_MODEL_DIR", str(env))
    R3.write_model_dir(env)
    assert W2.discover() == q2a and W.discover() == env
    R.write_model_dir(env, epoch=7)
    (env / "checkpoints" / "model_120.ckpt.best").unlink()
    assert W2.discover() == env and W2.checkpoint_file(env).name == "model_7.ckpt.best"
    assert W.discover("DeepFilterNet2") is None and W2.discover("DeepFilterNet3") is None
    assert W2.load().dir == env


def test_node_without_a_deepfilternet2_directory_raises_todays_error(pack, tmp_path, monkeypatch):
    from egregora_amd import dfn_weights as W
    monkeypatch.setattr(W, "pack_root", lambda: tmp_path / "a" / "b" / "pack")
    monkeypatch.setenv("HOME", str(tmp_path / "home"))
    R3.write_model_dir(tmp_path / "home" / ".cache" / "DeepFilterNet" / "DeepFilterNet2")       # a DFN3 model under the DFN2 name
    monkeypatch.setenv("EGREGORA_DFN_MODEL_DIR", str(tmp_path / "m3"))
    R3.write_model_dir(tmp_path / "m3")
    node = pack.NODE_CLASS_MAPPINGS["Egregora_DeepFilterNet_Denoise"]()
    with pytest.raises(RuntimeError) as e:
        node._enhance(torch.zeros(1, 960), "DeepFilterNet2", "cpu")
    assert str(e.value) == TODAYS_ERROR


@pytest.mark.parametrize("name", sorted(R.REJECTED2))
def test_unsupported_configs_raise_at_load_with_the_listing_error(pack, tmp_path, name):
    """Everything egr_dfn2_create / its run cannot build is refused when the directory is loaded, never later."""
    from egregora_amd import dfn2_weights as W
    overrides, fragment = R.REJECTED2[name]
    (tmp_path / "checkpoints").mkdir()
    p = _write(tmp_path / "config.ini", R.config_text(**overrides))
    cfg = W.parse_config(p)
    with pytest.raises(RuntimeError, match="not supported by the native forward pass") as e:
        W.check_supported(cfg)
    assert fragment in str(e.value), (fragment, str(e.value))
    torch.save({}, tmp_path / "checkpoints" / "model_1.ckpt.best")
    with pytest.raises(RuntimeError, match="not supported by the native forward pass"):
        W.load(tmp_path)


def test_shuffle_is_the_stated_permutation():
    """SPEC DFN2-P3: output index g h + j takes pre-shuffle index j G + g."""
    for G, h in ((8, 32), (4, 3), (2, 5), (16, 1)):
        x = torch.arange(G * h, dtype=torch.float64).reshape(1, 1, -1)
        y = R.shuffle(x, G)
        for g in range(G):
            for j in range(h):
                assert y[0, 0, g * h + j] == x[0, 0, j * G + g]
        assert sorted(y.reshape(-1).tolist()) == x.reshape(-1).tolist()
    x = torch.randn(3, 4)
    assert torch.equal(R.shuffle(x, 1), x)


def test_grouped_gru_with_one_group_is_stacked_torch_gru(pack, tmp_path):
    """G = 1, no shuffle: layer l's output is layer l of a stacked torch.nn.GRU, and the module output is their sum."""
    d, cfg, sd = _model_dir(tmp_path, dict(gru_groups=1, emb_num_layers=4))
    net = R.Net2(cfg, sd, torch.float64)
    x = torch.randn(2, 37, 256, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    ys, ss = net.ggru(x, "erb_dec.emb_gru", 3)
    ref = torch.nn.GRU(256, 256, num_layers=3, batch_first=True).double()
    with torch.no_grad():
        for l in range(3):
            for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                getattr(ref, f"{n}_l{l}").copy_(sd[f"erb_dec.emb_gru.grus.{l}.layers.0.{n}_l0"])
        y, _ = ref(x)
        outs, h = [], x
        for l in range(3):
            one = torch.nn.GRU(256, 256, batch_first=True).double()
            for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                getattr(one, f"{n}_l0").copy_(getattr(ref, f"{n}_l{l}"))
            h, _ = one(h)
            outs.append(h)
    assert float((ys[-1] - y).abs().max()) <= 1e-12 and all(torch.equal(a, b) for a, b in zip(ys, outs))
    assert torch.equal(ss[-1], (outs[0] + outs[1]) + outs[2])


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("which", ["default", "cornerA", "cornerB"])
def test_restatement_stages_compose_to_enhance_exactly(pack, tmp_path, which, dtype):
    """The per-stage methods the local gates call, chained by hand, give enhance()'s stage dict and output bit for bit."""
    d, cfg, sd = _model_dir(tmp_path, {} if which == "default" else R.MATRIX2[which])
    x = 0.3 * torch.randn(2, 3 * cfg["hop_size"] + 4801, generator=torch.Generator().manual_seed(4))
    y, st = R.enhance(x, cfg, sd, dtype, stages=True)
    net = R.Net2(cfg, sd, dtype)
    spec = R.analysis(x.to(dtype), cfg)
    fe, fs = R.shifted_features(spec, cfg)
    e = [net.e0(fe)]
    for i in (1, 2, 3):
        e.append(net.e_next(i, e[-1]))
    c0 = net.c0(fs)
    grus, sums, acc = [], [], None
    g, acc = net.ggru_step(net.emb_in(e[3], c0), "enc.emb_gru", 0, 1, None)
    grus.append(g), sums.append(acc)
    emb = acc
    for prefix, n in (("erb_dec.emb_gru", cfg["emb_num_layers"] - 1), ("df_dec.df_gru", cfg["df_num_layers"])):
        xin, acc = emb, None
        for l in range(n):
            xin, acc = net.ggru_step(xin, prefix, l, n, acc)
            grus.append(xin), sums.append(acc)
        if prefix == "erb_dec.emb_gru":
            mask = net.mask2(acc, *e)
    c = net.df_c(acc, emb)
    alpha = net.alpha(c)
    coefs = net.coefs2(c, c0)
    spec_e = net.assemble2(spec, mask, coefs, alpha)
    mine = dict(spec=spec, feat_erb=fe, feat_spec=fs, e0=e[0], e1=e[1], e2=e[2], e3=e[3], c0=c0, emb=emb, mask=mask, coefs=coefs,
                alpha=alpha, spec_e=spec_e, y=R.synthesis(spec_e, cfg, x.shape[1]))
    assert set(mine) | {"grus", "sums"} == set(st)
    for k, v in mine.items():
        assert v.dtype == st[k].dtype and torch.equal(v, st[k]), k
    assert len(grus) == len(st["grus"]) == cfg["emb_num_layers"] + cfg["df_num_layers"]
    assert all(torch.equal(a, b) for a, b in zip(grus, st["grus"])) and all(torch.equal(a, b) for a, b in zip(sums, st["sums"]))
    assert torch.equal(mine["y"], y)


def test_mask_then_deep_filter_with_alpha(pack, tmp_path):
    """SPEC DFN2-P7 on hand-made inputs: alpha = 0 gives the masked spectrum everywhere; alpha = 1 and a unit tap at the lookahead-free
    position gives the masked spectrum too; bins >= nb_df are always the masked spectrum."""
    d, cfg, sd = _model_dir(tmp_path)
    net = R.Net2(cfg, sd, torch.float64)
    g = torch.Generator().manual_seed(9)
    T, Fq, E, nb, O = 11, 481, 32, 96, 5
    spec = torch.complex(torch.randn(1, T, Fq, generator=g, dtype=torch.float64), torch.randn(1, T, Fq, generator=g, dtype=torch.float64))
    mask = torch.rand(1, T, E, generator=g, dtype=torch.float64)
    coefs = torch.randn(1, T, nb, 2 * O, generator=g, dtype=torch.float64)
    _, inv = R.W().erb_matrices(R.W().erb_widths(48000, 960, E, 2))
    sm = spec * (mask @ inv.double())
    out0 = net.assemble2(spec, mask, coefs, torch.zeros(1, T, dtype=torch.float64))
    assert torch.allclose(out0, sm, rtol=0, atol=1e-15)
    unit = torch.zeros_like(coefs)
    unit[..., 2 * (O - 1 - cfg["df_lookahead"])] = 1.0                      # tap k = O - 1 - la reads frame t itself
    out1 = net.assemble2(spec, mask, unit, torch.ones(1, T, dtype=torch.float64))
    assert torch.allclose(out1, sm, rtol=0, atol=1e-15)
    a = torch.rand(1, T, generator=g, dtype=torch.float64)
    out = net.assemble2(spec, mask, coefs, a)
    assert torch.equal(out[..., nb:], sm[..., nb:])
    assert not torch.allclose(out[..., :nb], sm[..., :nb])


@pytest.mark.parametrize("name", sorted(R.MATRIX2))
def test_every_matrix_config_loads_and_runs_through_the_restatement(pack, tmp_path, name):
    """The configurations tests/test_gpu_dfn2_configs.py runs on the device load, pack to the size egr_dfn2_create derives, and
    run through the restatement in both dtypes at an odd short length."""
    from egregora_amd import dfn2_engine, dfn2_weights as W
    d, cfg, sd = _model_dir(tmp_path, R.MATRIX2[name])
    m = W.load(d)
    c = dfn2_engine.config_c(m)
    assert c.gru_groups == cfg["gru_groups"] and c.group_shuffle == int(cfg["group_shuffle"]) and c.kf % 2 == 1
    assert m.packed().size == _packed_size(W, sd, cfg)
    x = 0.3 * torch.randn(2, 3 * cfg["hop_size"] + 17, generator=torch.Generator().manual_seed(6))
    y64, s64 = R.enhance(x, cfg, sd, torch.float64, stages=True)
    y32 = R.enhance(x, cfg, sd, torch.float32)
    assert y64.shape == x.shape and bool(torch.isfinite(y64).all()) and bool(torch.isfinite(y32).all())
    assert len(s64["grus"]) == len(s64["sums"]) == cfg["emb_num_layers"] + cfg["df_num_layers"]
    assert float((y32.double() - y64).norm()) <= 1e-4 * float(y64.norm()) + 1e-12


def _stage_list(st):
    out = {k: v for k, v in st.items() if k not in ("grus", "sums")}
    out.update({f"gru{i}": v for i, v in enumerate(st["grus"])})
    out.update({f"sum{i}": v for i, v in enumerate(st["sums"])})
    return out


@pytest.mark.parametrize("name", ["default"] + sorted(R.MATRIX2))
def test_float32_restatement_keeps_far_inside_the_cap(pack, tmp_path, name):
    """The cap condition: with the signal the GPU tests use, the float32 restatement's relative rms error against float64 is at most
    CAP / 10 at every stage, so the GPU gates (<= 1.5x that error + FLOOR, and <= CAP) are decided by the device's precision."""
    d, cfg, sd = _model_dir(tmp_path, {} if name == "default" else R.MATRIX2[name], seed=5)
    x = speechy(3, 48000, 2)
    _, s64 = R.enhance(x, cfg, sd, torch.float64, stages=True)
    _, s32 = R.enhance(x, cfg, sd, torch.float32, stages=True)
    a, b = _stage_list(s64), _stage_list(s32)
    errs = {k: rel(torch.view_as_real(b[k]) if b[k].is_complex() else b[k], torch.view_as_real(a[k]) if a[k].is_complex() else a[k])
            for k in a}
    worst = max(errs, key=errs.get)
    print(f"\n{name}: worst stage {worst} {errs[worst]:.2e}")
    assert errs[worst] <= CAP / 10, errs
