"""The shared host layer of the many-clip paths (many_common.py, resample.poly_track_table, batch_cli.batches): host only."""
import importlib.util

import numpy as np
import pytest
import torch

from conftest import ROOT

CALLERS = ("encode_many", "denoise_many", "enhance_many", "resample_many")


@pytest.mark.parametrize("who", CALLERS)
def test_check_clips_refuses_by_name(pack, who):
    from egregora_amd.many_common import check_clips
    good = torch.zeros(2, 5)
    refused = {"1-D": torch.zeros(5), "3-D": torch.zeros(1, 2, 5), "C = 0": torch.zeros(0, 5), "T = 0": torch.zeros(2, 0),
               "not a tensor": np.zeros((2, 5), np.float32)}
    for what, x in refused.items():
        with pytest.raises(ValueError) as ei:
            check_clips(who, [(good, 48000), (x, 48000)])
        assert str(ei.value) == f"{who}: clip 1: expected a non-empty [C, T] tensor and a positive sample rate", what
    with pytest.raises(ValueError) as ei:
        check_clips(who, [(good, 0)])
    assert str(ei.value) == f"{who}: clip 0: expected a non-empty [C, T] tensor and a positive sample rate"
    out = check_clips(who, [(good, 44100.0), (good[:1], "16000")])
    assert [(x.shape, sr, type(sr)) for x, sr in out] == [((2, 5), 44100, int), ((1, 5), 16000, int)] and out[0][0] is good
    assert check_clips(who, []) == []


def test_check_clips_allow_empty_is_wpes(pack):
    from egregora_amd.many_common import check_clips
    empty, good = torch.zeros(2, 0), torch.zeros(1, 7)
    out = check_clips("dereverb_many", [(good, 16000), (empty, 8000)], allow_empty=True)
    assert out[1][0] is empty and out[1][1] == 8000
    for x, sr in ((torch.zeros(5), 8000), (torch.zeros(1, 2, 5), 8000), (torch.zeros(0, 5), 8000), (good, 0), ([[0.0]], 8000)):
        with pytest.raises(ValueError) as ei:
            check_clips("dereverb_many", [(good, 16000), (empty, 8000), (x, sr)], allow_empty=True)
        assert str(ei.value) == "dereverb_many: clip 2: expected a [C, T] tensor and a positive sample rate"


def test_group_by_rate_keeps_first_seen_order_and_skips_the_target(pack):
    from egregora_amd.many_common import group_by_rate
    g = group_by_rate([44100, 16000, 48000, 44100, 8000, 16000, 48000], 48000)
    assert list(g.items()) == [(44100, [0, 3]), (16000, [1, 5]), (8000, [4])]
    assert group_by_rate([48000, 48000], 48000) == {} and group_by_rate([], 48000) == {}
    assert list(group_by_rate([48000, 16000], None).items()) == [(48000, [0]), (16000, [1])]


def test_track_rows_and_clip_views_against_a_written_table(pack):
    from egregora_amd.many_common import clip_views, track_rows
    shapes = [(1, 1), (2, 3), (3, 1)]
    ins, lens = track_rows(shapes, base=7)
    assert ins == [7, 8, 11, 14, 15, 16] and lens == [1, 3, 3, 1, 1, 1]
    assert track_rows(shapes) == ([0, 1, 4, 7, 8, 9], lens) and track_rows([]) == ([], [])
    # a tracks table as a 2:1 rate change lays it out: (in offset, n_in, out offset, n_out), outputs back to back
    tab = np.array([[7, 1, 0, 2], [8, 3, 2, 6], [11, 3, 8, 6], [14, 1, 14, 2], [15, 1, 16, 2], [16, 1, 18, 2]], dtype=np.int64)
    y = torch.arange(20, dtype=torch.float32)
    views = clip_views(y, tab, shapes)
    assert [tuple(v.shape) for v in views] == [(1, 2), (2, 6), (3, 2)]
    assert views[0].tolist() == [[0, 1]] and views[1].tolist() == [list(range(2, 8)), list(range(8, 14))]
    assert views[2].tolist() == [[14, 15], [16, 17], [18, 19]]
    assert all(v.data_ptr() == y.data_ptr() + 4 * o for v, o in zip(views, (0, 2, 14)))           # views, not copies


def test_poly_track_table_is_the_pinned_table_and_sincs_lengths(pack):
    from egregora_amd import resample
    assert resample.poly_track_table([0], [10], 3, 1)[0].tolist() == [[0, 10, 0, 30]]
    ins, lens = [100, 0, 50], [1, 11, 4001]
    tab, total = resample.poly_track_table(ins, lens, 160, 147)              # 44.1 -> 48 kHz: up = n = 160, down = o = 147
    stab, stotal = resample.sinc_track_table(ins, lens, 147, 160)
    assert tab.dtype == np.int64 and tab.flags["C_CONTIGUOUS"] and np.array_equal(tab, stab) and total == stotal
    assert tab[:, 3].tolist() == [-(-n * 160 // 147) for n in lens] and total == int(tab[:, 3].sum())
    empty, zero = resample.poly_track_table([], [], 160, 147)
    assert empty.shape == (0, 4) and zero == 0


def test_budget_bytes_reads_the_variable_when_called(pack, monkeypatch):
    from egregora_amd.many_common import budget_bytes
    monkeypatch.delenv("EGREGORA_TEST_WAVE_GB", raising=False)
    assert budget_bytes("EGREGORA_TEST_WAVE_GB", 16.0) == 16 * 2 ** 30 and budget_bytes("EGREGORA_TEST_WAVE_GB", "64") == 64 * 2 ** 30
    monkeypatch.setenv("EGREGORA_TEST_WAVE_GB", "2")
    assert budget_bytes("EGREGORA_TEST_WAVE_GB", 16.0) == 2 * 2 ** 30
    monkeypatch.setenv("EGREGORA_TEST_WAVE_GB", "0.75")
    assert budget_bytes("EGREGORA_TEST_WAVE_GB", 16.0) == 3 * 2 ** 28
    assert budget_bytes("EGREGORA_TEST_WAVE_GB", 16.0, override=12345) == 12345 and budget_bytes("EGREGORA_TEST_WAVE_GB", 16.0, 0) == 0
    monkeypatch.setenv("EGREGORA_TEST_WAVE_GB", "1e-9")
    b = budget_bytes("EGREGORA_TEST_WAVE_GB", 16.0)
    assert b == 1 and isinstance(b, int)                                    # truncated like int(): 1.07 bytes


def test_budget_bytes_is_what_the_planners_read(pack, monkeypatch):
    from egregora_amd import dac_engine, dfn_engine, eval_many
    monkeypatch.setenv("EGREGORA_EVAL_WAVE_GB", "0.5")
    monkeypatch.setenv(dac_engine.WORKSPACE_GB_ENV, "1.5")
    monkeypatch.delenv(dfn_engine.WORKSPACE_GB_ENV, raising=False)
    assert eval_many.wave_budget() == 2 ** 29 and eval_many.wave_budget(77) == 77
    assert dac_engine.workspace_budget_bytes() == 3 * 2 ** 29
    assert dfn_engine.workspace_budget_bytes() == int(float(dfn_engine.WORKSPACE_GB_DEFAULT) * 2 ** 30)


def test_batches_close_before_the_item_over_budget(pack):
    spec = importlib.util.spec_from_file_location("batch_cli_alone", ROOT / "comfyui-egregora-audio-super-resolution_amd" / "batch_cli.py")
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    cost = lambda it: it
    assert list(cli.batches([], cost, 10)) == [] and list(cli.batches(iter(()), cost, 10)) == []
    assert list(cli.batches([3, 3, 4, 1, 9, 2], cost, 10)) == [[3, 3, 4], [1, 9], [2]]           # 10 fits: only past the budget closes
    assert list(cli.batches([2, 50, 1, 1], cost, 10)) == [[2], [50], [1, 1]]                     # over budget alone: its own batch
    assert list(cli.batches([50], cost, 10)) == [[50]]
    assert list(cli.batches(iter([("a", 0.6), ("b", 0.5), ("c", 0.5)]), lambda it: it[1], 1.0)) == [[("a", 0.6)], [("b", 0.5), ("c", 0.5)]]
    assert cli.AUDIO_SUFFIXES == (".wav", ".flac")


def test_download_of_host_tensors(pack):
    from egregora_amd.many_common import download
    assert download([]) == []
    xs = [torch.arange(1, dtype=torch.float32).view(1, 1), torch.arange(10, dtype=torch.float32).view(2, 5) + 1,
          torch.arange(12, dtype=torch.float32).view(3, 4).t(), torch.zeros(2, 0)]
    ys = download(xs)
    assert [tuple(y.shape) for y in ys] == [(1, 1), (2, 5), (4, 3), (2, 0)]
    assert all(torch.equal(x, y) and y.is_contiguous() and not y.is_cuda for x, y in zip(xs, ys))
