"""CPU: the host side of batched voice conversion (inference_vc.vc_batch / vc_batch_files) -- length arithmetic from
source padding to w2v frames, F0 samples and mel frames, '.hf0.npy' discovery, argument validation, output naming, and
the argument checks of the new entry points (which reject before any HIP call, so they run here on dummy pointers)."""
import os

import numpy as np
import pytest
import torch


def test_length_arithmetic_of_ragged_sources():
    from megatts2_hierspeechpp_amd import inference_vc as IV
    from megatts2_hierspeechpp_amd.extract_w2v import Wav2vec2
    raw = [1, 639, 1279, 1280, 12000, 16000, 63999, 64000, 127361]
    for n in raw:
        lp = IV.padded_length(n)
        assert lp % 1280 == 0 and n < lp <= n + 1280
        assert IV.pad_source(torch.zeros(1, n)).shape == (1, lp)
        T = IV.w2v_frames(lp)
        assert T == lp // 320 == Wav2vec2.frames(lp + 80)
        assert IV.f0_samples(lp) == 4 * T == lp // 80
        assert IV.output_length(T) == 320 * T
        assert IV.output_length(T, 24000) == 480 * T and IV.output_length(T, 48000) == 960 * T
    lens = torch.tensor([IV.padded_length(n) for n in raw])
    assert torch.equal(IV.w2v_frames(lens), lens // 320)            # the same arithmetic on a device-style tensor
    assert [IV.mel_frames(n) for n in (641, 959, 960, 48000, 48319)] == [2, 2, 3, 150, 150]


def test_f0_track_discovery_and_missing_track(tmp_path):
    from megatts2_hierspeechpp_amd import _lib, inference_vc as IV
    wav = tmp_path / "spk1_utt.wav"
    assert IV.f0_path(wav) == str(tmp_path / "spk1_utt.hf0.npy")
    assert IV.f0_path("/a/b.WAV") == "/a/b.hf0.npy"
    assert IV.f0_path("/a/b.flac") == "/a/b.flac.hf0.npy"
    with pytest.raises(_lib.HspError, match="spk1_utt.wav"):
        IV.load_f0(wav)
    track = np.arange(7, dtype=np.float64)
    np.save(tmp_path / "spk1_utt.hf0.npy", track[None])             # extract_f0.py's fallback layout [1, n]
    got = IV.load_f0(wav)
    assert got.dtype == np.float32 and got.shape == (7,) and np.array_equal(got, track)


def test_prompt_grouping_and_count():
    from megatts2_hierspeechpp_amd import _lib, inference_vc as IV
    a, b = torch.zeros(3), torch.zeros(3)
    assert IV.group_prompts(a, 4) == ([a], [0, 0, 0, 0])
    d, idx = IV.group_prompts([a, b, a], 3)
    assert len(d) == 2 and d[0] is a and d[1] is b and idx == [0, 1, 0]
    d, idx = IV.group_prompts([a], 5)
    assert d[0] is a and idx == [0] * 5
    with pytest.raises(_lib.HspError, match="one prompt or one per source"):
        IV.group_prompts([a, b], 3)


def test_check_batch_track_lengths():
    from megatts2_hierspeechpp_amd import _lib, inference_vc as IV
    IV.check_batch([1280, 2560], [16, 33], [48000], [600])               # a YAAPT track may be one frame longer
    with pytest.raises(_lib.HspError, match="source 1: F0 track of 31"):
        IV.check_batch([1280, 2560], [16, 31], [48000], [600])
    with pytest.raises(_lib.HspError, match="pad_source"):
        IV.check_batch([1300], [17], [48000], [600])
    with pytest.raises(_lib.HspError, match="prompt 0: F0 track"):
        IV.check_batch([1280], [16], [48000], [599])
    with pytest.raises(_lib.HspError, match="more than 640"):
        IV.check_batch([1280], [16], [640], [8])
    with pytest.raises(_lib.HspError, match="2 sources but 1"):
        IV.check_batch([1280, 1280], [16], [48000], [600])


def test_length_groups():
    from megatts2_hierspeechpp_amd import inference_vc as IV
    assert IV.length_groups([2560, 1280, 2560, 3840, 1280]) == [[0, 2], [1, 4], [3]]
    assert IV.length_groups([1280]) == [[0]]


def test_output_naming_and_rate():
    from megatts2_hierspeechpp_amd import inference_vc as IV
    assert IV.output_name("/x/src/p225_001.wav", "prompts/p231.wav") == "p225_001_to_p231.wav"
    assert IV.output_name("a.b.wav", "c") == "a.b_to_c.wav"
    assert [IV.output_rate(r) for r in (16000, 24000, 48000, 22050)] == [16000, 24000, 48000, 16000]


def test_new_entry_points_reject_bad_arguments():
    from megatts2_hierspeechpp_amd import _lib
    lib = _lib.lib()
    p = 16                                     # a dummy non-NULL pointer: every call below fails its checks first
    E = _lib.EINVAL
    # reflect pad: pad >= L, Lo > L + 2 pad, y_bs < Lo
    assert lib.hsp_reflect_pad_ragged_f32(p, 100, p, p, 180, 2, 100, 100, 180, None) == E
    assert lib.hsp_reflect_pad_ragged_f32(p, 100, p, p, 200, 2, 100, 40, 181, None) == E
    assert lib.hsp_reflect_pad_ragged_f32(p, 100, p, p, 179, 2, 100, 40, 180, None) == E
    # F0: src stride below n_max, target stride between 0 and nt_max, NULL lengths
    assert lib.hsp_f0_convert_batch_f32(p, 99, p, p, 0, p, 50, p, 100, 2, 100, None) == E
    assert lib.hsp_f0_convert_batch_f32(p, 100, p, p, 20, p, 50, p, 100, 2, 100, None) == E
    assert lib.hsp_f0_convert_batch_f32(p, 100, None, p, 0, p, 50, p, 100, 2, 100, None) == E
    # STFT: T != 1 + L / hop, L <= n_fft / 2, f_ld < T
    assert lib.hsp_stft_frames_ragged_f32(p, 3200, p, p, p, 2, 3200, 1280, 320, 10, 12, None) == E
    assert lib.hsp_stft_frames_ragged_f32(p, 640, p, p, p, 2, 640, 1280, 320, 3, 4, None) == E
    assert lib.hsp_stft_frames_ragged_f32(p, 3200, p, p, p, 2, 3200, 1280, 320, 11, 10, None) == E
    # row reductions: stride below n
    assert lib.hsp_abs_max_rows_f32(p, 10, None, p, 2, 11, None) == E
    assert lib.hsp_peak_int16_gains(p, 11, None, None, p, 11, 2, 11, None) == E
    assert lib.hsp_peak_int16_gains(p, 11, None, p, p, 10, 2, 11, None) == E


def test_vc_models_output_sr_needs_speechsr():
    from megatts2_hierspeechpp_amd import _lib, inference_vc as IV
    with pytest.raises(_lib.HspError, match="speechsr"):
        IV._sr_model(object())
