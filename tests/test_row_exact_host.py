"""CPU: the host side of row-exact ragged batches -- argument checks, the refused experiment knobs, the per-resolution
length bookkeeping and the new C ABI declarations."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lengths_are_checked_against_the_padded_length():
    from megatts2_hierspeechpp_amd import _lib as L
    from megatts2_hierspeechpp_amd import hierspeechpp_speechsynthesizer as HS
    assert HS._row_exact_lengths(False, [3, 9], 10, "cpu") is None
    got = HS._row_exact_lengths(True, [3, 10], 10, "cpu")
    assert got.dtype == torch.int64 and got.tolist() == [3, 10]
    assert HS._row_exact_lengths(True, torch.tensor([4, 7]), 7, "cpu").tolist() == [4, 7]
    for bad in ([3, 11], [0, 5]):
        with pytest.raises(L.HspError):
            HS._row_exact_lengths(True, bad, 10, "cpu")


@pytest.mark.parametrize("knob,value", [("FUSE_ACT_MAX_CHANNELS", 64)])
def test_experiment_knobs_refuse_row_exact(monkeypatch, knob, value):
    from megatts2_hierspeechpp_amd import _lib as L
    from megatts2_hierspeechpp_amd import hierspeechpp_speechsynthesizer as HS
    assert HS.row_exact_refusal() is None
    monkeypatch.setattr(HS, knob, value)
    assert HS.row_exact_refusal() is not None
    with pytest.raises(L.HspError):
        HS._row_exact_lengths(True, [2, 3], 4, "cpu")


def test_row_lengths_per_resolution():
    from megatts2_hierspeechpp_amd import _lib as L
    from megatts2_hierspeechpp_amd import hip_layers
    rows = hip_layers.RowLengths(torch.tensor([5, 12, 1], dtype=torch.int64), 12)
    assert rows.at(12) is rows.frames
    assert rows.at(48).tolist() == [20, 48, 4]
    assert rows.at(3840).tolist() == [1600, 3840, 320]
    assert rows.at(48) is rows.at(48)                          # built once per resolution
    with pytest.raises(L.HspError):
        rows.at(50)                                            # not a whole multiple of the frame count
    with pytest.raises(L.HspError):
        hip_layers.RowLengths(torch.tensor([1.0]), 4)
    assert hip_layers.row_lengths() is None
    with hip_layers.row_exact(rows):
        assert hip_layers.row_lengths() is rows
        inner = hip_layers.RowLengths(torch.tensor([1], dtype=torch.int64), 4)
        with hip_layers.row_exact(inner):
            assert hip_layers.row_lengths() is inner
        assert hip_layers.row_lengths() is rows
    assert hip_layers.row_lengths() is None


def test_row_exact_state_is_per_thread():
    import threading
    from megatts2_hierspeechpp_amd import hip_layers
    seen = []
    with hip_layers.row_exact(hip_layers.RowLengths(torch.tensor([3, 4], dtype=torch.int64), 4)):
        t = threading.Thread(target=lambda: seen.append(hip_layers.row_lengths()))
        t.start()
        t.join()
    assert seen == [None]


def test_header_declares_the_row_exact_abi():
    h = open(os.path.join(ROOT, "include", "hsp.h")).read()
    assert re.search(r"int hsp_act1d_snakebeta_ragged_f32\(const float\* x, float\* y, int32_t B, int32_t C, int32_t L, "
                     r"const int64_t\* lens,", h)
    body = h[h.index("typedef struct hsp_mha_proj_args"):h.index("} hsp_mha_proj_args;")]
    assert body.rstrip().endswith("const int64_t* key_len; /* [B] keys per utterance, or NULL: all Tk */")
    from megatts2_hierspeechpp_amd import _lib as L
    assert L.MhaProjArgs._fields_[-1][0] == "key_len"


def test_vc_batch_files_defaults_to_one_batch_with_row_exact():
    import inspect
    from megatts2_hierspeechpp_amd import inference_vc as IV
    assert inspect.signature(IV.vc_batch).parameters["row_exact"].default is False
    assert inspect.signature(IV.vc_batch_files).parameters["group_by_length"].default is None
