"""CPU: the host side of the batched prompt denoiser -- the segment-table builder of the packed layout, the sub-batch
split, the refusal of device-only lengths, the argument checks of the packed entry points (which reject before any HIP
call, so they run here on dummy pointers), their declarations and the new vc_batch keywords."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["hsp_norm_factor_rows_f32", "hsp_stft_frames_packed_f32", "hsp_instnorm_prelu_seg_f32", "hsp_zero_gaps_f32",
       "hsp_dwconv_bn_silu_seg_f32", "hsp_istft_ola_seg_f32"]


def _lib_or_build():
    from megatts2_hierspeechpp_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from megatts2_hierspeechpp_amd.build import build
        build()
    return _lib


def test_segment_table_offsets_gaps_and_total():
    from megatts2_hierspeechpp_amd import _lib as L
    from megatts2_hierspeechpp_amd.denoiser import packed
    assert packed.GAP >= 8                       # the dense blocks' largest T shift (dilation 8)
    frames = [4, 10, 81, 145]
    first, t = [], 0
    for n in frames:
        first.append(t)
        t += n + packed.GAP
    assert packed.packed_rows(frames) == t - packed.GAP == sum(frames) + 3 * packed.GAP
    # the host half of a table, without a device: the same arithmetic the Segments constructor runs
    seg = packed.Segments.__new__(packed.Segments)
    with pytest.raises(L.HspError):
        packed.Segments.__init__(seg, frames, torch.device("cpu"), gap=7)
    with pytest.raises(L.HspError):
        packed.Segments.__init__(seg, [4, 0], torch.device("cpu"))
    packed.Segments.__init__(seg, frames, torch.device("cpu"))      # the CPU stands in for the device copy here
    assert seg.first == first and seg.frames == frames and seg.T_tot == t - packed.GAP and seg.B == 4
    assert list(seg.host) == [v for b in range(4) for v in (first[b], frames[b])]
    assert seg.dev.dtype == torch.int32 and seg.dev.tolist() == [[first[b], frames[b]] for b in range(4)]
    assert [(s.start, s.stop) for s in seg.slices()] == [(first[b], first[b] + frames[b]) for b in range(4)]
    for a, b in zip(seg.slices()[:-1], seg.slices()[1:]):
        assert b.start - a.stop == packed.GAP


def test_sub_batch_split_keeps_whole_prompts():
    from megatts2_hierspeechpp_amd import _lib as L
    from megatts2_hierspeechpp_amd.denoiser import packed
    G = packed.GAP
    frames = [4, 10, 81, 145]
    assert packed.split_rows(frames, 10 ** 6) == [[0, 1, 2, 3]]
    assert packed.split_rows(frames, sum(frames) + 3 * G) == [[0, 1, 2, 3]]
    assert packed.split_rows(frames, sum(frames) + 3 * G - 1) == [[0, 1, 2], [3]]
    assert packed.split_rows(frames, 4 + G + 10) == [[0, 1], [2], [3]]
    assert packed.split_rows(frames, 4 + G + 9) == [[0], [1], [2], [3]]
    assert packed.split_rows(frames, 1) == [[0], [1], [2], [3]]      # a row above the cap runs alone
    for cap in (1, 50, 100, 200, 300):
        groups = packed.split_rows(frames, cap)
        assert [b for g in groups for b in g] == [0, 1, 2, 3]
        for g in groups:
            assert len(g) == 1 or packed.packed_rows([frames[b] for b in g]) <= cap
    with pytest.raises(L.HspError):
        packed.split_rows(frames, 0)


def test_lengths_must_live_on_the_host():
    from megatts2_hierspeechpp_amd import _lib as L
    from megatts2_hierspeechpp_amd.denoiser import packed
    import numpy as np
    assert packed.host_ints([3, 4]) == [3, 4] and packed.host_ints(np.array([3, 4])) == [3, 4]
    assert packed.host_ints(torch.tensor([3, 4])) == [3, 4]
    with pytest.raises(L.HspError):
        packed.host_ints([])

    class OnDevice(torch.Tensor):            # a tensor that says it lives on the GPU, for a machine without one
        @property
        def is_cuda(self):
            return True
    with pytest.raises(L.HspError, match="host"):
        packed.host_ints(torch.tensor([3, 4]).as_subclass(OnDevice))
    with pytest.raises(L.HspError, match="host"):
        packed.split_rows(torch.tensor([3, 4]).as_subclass(OnDevice), 100)


def _table(*pairs):
    flat = [v for p in pairs for v in p]
    return (ctypes.c_int32 * len(flat))(*flat)


GOOD = _table((0, 4), (12, 10), (30, 1))
BAD_TABLES = {
    "negative": _table((-1, 4), (12, 10), (30, 1)),
    "empty_segment": _table((0, 4), (12, 0), (30, 1)),
    "overlap": _table((0, 4), (3, 10), (30, 1)),
    "descending": _table((12, 10), (0, 4), (30, 1)),
    "past_T_tot": _table((0, 4), (12, 10), (30, 11)),
}
D = ctypes.c_void_p(0x1000)


def _calls(lib, seg_host, B=3, T_tot=40, seg=D, p=D):
    """Every segment-table entry point on dummy pointers ``p`` with the host table ``seg_host``."""
    h = ctypes.cast(seg_host, ctypes.c_void_p) if seg_host is not None else None
    return {
        "hsp_stft_frames_packed_f32": lib.hsp_stft_frames_packed_f32(p, 14400, p, None, p, p, seg, h, B, 14400, 400, 100,
                                                                     T_tot, T_tot, None),
        "hsp_instnorm_prelu_seg_f32": lib.hsp_instnorm_prelu_seg_f32(p, T_tot * 5, 2, T_tot, 5, seg, h, B, p, p, p, 1e-5,
                                                                     None),
        "hsp_zero_gaps_f32": lib.hsp_zero_gaps_f32(p, T_tot * 5, 2, T_tot, 5, seg, h, B, None),
        "hsp_dwconv_bn_silu_seg_f32": lib.hsp_dwconv_bn_silu_seg_f32(p, p, p, p, p, p, p, 1e-5, p, 2, 3, T_tot, 31, seg, h,
                                                                     B, None),
        "hsp_istft_ola_seg_f32": lib.hsp_istft_ola_seg_f32(p, T_tot, p, None, p, 1000, 1000, 400, 100, seg, h, B, T_tot,
                                                           None),
    }


@pytest.mark.parametrize("name", sorted(BAD_TABLES))
def test_packed_abi_rejects_bad_tables_before_any_hip_call(name):
    _lib = _lib_or_build()
    for fn, rc in _calls(_lib.lib(), BAD_TABLES[name]).items():
        assert rc == _lib.EINVAL, (fn, name, rc)


def test_packed_abi_rejects_bad_counts_and_null_pointers():
    _lib = _lib_or_build()
    lib = _lib.lib()
    E = _lib.EINVAL
    for kw in (dict(B=0), dict(B=-1), dict(T_tot=30), dict(seg=None), dict(p=None)):
        for fn, rc in _calls(lib, GOOD, **kw).items():
            assert rc == E, (fn, kw, rc)
    for fn, rc in _calls(lib, None).items():
        assert rc == E, (fn, "no host table", rc)
    # the per-row norm factor takes no table
    assert lib.hsp_norm_factor_rows_f32(None, 100, D, D, D, 2, 100, None) == E
    assert lib.hsp_norm_factor_rows_f32(D, 100, None, D, D, 2, 100, None) == E
    assert lib.hsp_norm_factor_rows_f32(D, 100, D, None, D, 2, 100, None) == E
    assert lib.hsp_norm_factor_rows_f32(D, 100, D, D, None, 2, 100, None) == E
    assert lib.hsp_norm_factor_rows_f32(D, 100, D, D, D, 0, 100, None) == E
    assert lib.hsp_norm_factor_rows_f32(D, 99, D, D, D, 2, 100, None) == E
    # each null data pointer on its own, with a good table
    h = ctypes.cast(GOOD, ctypes.c_void_p)
    for i in range(4):
        a = [D, D, D, D]
        a[i] = None
        assert lib.hsp_stft_frames_packed_f32(a[0], 14400, a[1], None, a[2], a[3], D, h, 3, 14400, 400, 100, 40, 40,
                                              None) == E, i
        assert lib.hsp_instnorm_prelu_seg_f32(a[0], 200, 2, 40, 5, D, h, 3, a[1], a[2], a[3], 1e-5, None) == E, i
    for i in range(3):
        a = [D, D, D]
        a[i] = None
        assert lib.hsp_istft_ola_seg_f32(a[0], 40, a[1], None, a[2], 1000, 1000, 400, 100, D, h, 3, 40, None) == E, i
    for i in range(8):
        a = [D] * 8
        a[i] = None
        assert lib.hsp_dwconv_bn_silu_seg_f32(*a[:7], 1e-5, a[7], 2, 3, 40, 31, D, h, 3, None) == E, i
    assert lib.hsp_zero_gaps_f32(None, 200, 2, 40, 5, D, h, 3, None) == E
    # shapes: a frame matrix narrower than T_tot, a row with more frames than L samples give (1 + 800 / 100 = 9), an even K, a short output
    assert lib.hsp_stft_frames_packed_f32(D, 14400, D, None, D, D, D, h, 3, 14400, 400, 100, 40, 39, None) == E
    assert lib.hsp_stft_frames_packed_f32(D, 800, D, None, D, D, D, h, 3, 800, 400, 100, 40, 40, None) == E   # T_b = 10 > 9
    assert lib.hsp_dwconv_bn_silu_seg_f32(D, D, D, D, D, D, D, 1e-5, D, 2, 3, 40, 30, D, h, 3, None) == E
    assert lib.hsp_istft_ola_seg_f32(D, 40, D, None, D, 899, 899, 400, 100, D, h, 3, 40, None) == E           # 100 (10 - 1) = 900
    assert lib.hsp_instnorm_prelu_seg_f32(D, 199, 2, 40, 5, D, h, 3, D, D, D, 1e-5, None) == E                # plane pitch


def test_header_declares_the_packed_entry_points():
    from megatts2_hierspeechpp_amd import _lib
    text = open(os.path.join(ROOT, "include", "hsp.h")).read()
    assert "#define HSP_VERSION 104" in text          # 104: the four one-prompt twins of the _seg entry points left
    for gone in ("hsp_sum_sq_f32", "hsp_instnorm_prelu_f32", "hsp_dwconv_bn_silu_f32", "hsp_istft_ola_f32"):
        assert not re.search(r"\bint\s+%s\s*\(" % gone, text) and gone not in _lib.SIGNATURES, gone
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES, name
        if name != "hsp_norm_factor_rows_f32":
            decl = text[text.index("int " + name):]
            decl = decl[:decl.index(";")]
            assert "const int32_t* seg," in decl and "const int32_t* seg_host" in decl, name


def test_vc_batch_keywords_and_defaults():
    from megatts2_hierspeechpp_amd import inference_vc as IV
    from megatts2_hierspeechpp_amd.denoiser import infer
    from megatts2_hierspeechpp_amd.denoiser.generator import MPNet
    p = inspect.signature(IV.vc_batch).parameters
    for name in ("denoiser", "hps_denoiser", "denoised"):
        assert p[name].default is None and p[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    assert p["denoise_ratio"].default == 0.0
    assert list(inspect.signature(IV.denoise_prompts).parameters) == ["prompts", "denoiser", "hps"]
    q = inspect.signature(infer.denoise_batch).parameters
    assert list(q)[:3] == ["wavs", "model", "hps"] and q["lengths"].default is None and q["max_rows"].default > 0
    assert q["return_spectrogram"].default is False
    assert inspect.signature(MPNet.forward).parameters["lengths"].default is None
    assert callable(infer.mag_pha_stft_batch) and callable(infer.mag_pha_istft_batch)


def test_chosen_prompts_leave_most_phases_well_conditioned():
    """The GPU tests compare phases only where the reference magnitude is above 1e-3 of its peak and demand that this
    keeps more than half of the bins: held here, with the oracle, for the input and the denoised spectrogram of all four
    prompts."""
    import helpers as H
    import denoise_batch_inputs as DI
    from oracle import hsp_oracle as O
    meta, _ = H.load_fixture("denoise_l8000")
    meta2, _ = H.load_fixture("denoise_l14400")
    assert meta["seed"] == meta2["seed"] == 7 and meta["shapes"] == meta2["shapes"]     # one state dict for both
    sd = H.oracle_sd(meta)
    for n, wav in zip(DI.LENGTHS, DI.rows()):
        assert wav.shape == (n,) and float(abs(wav).max()) > 0.0                 # never silent
        if n not in DI.FIXTURES:
            assert float(abs(wav).max()) <= 0.5                                   # the synthetic rows
        w = torch.from_numpy(wav)
        y = (w * torch.sqrt(len(w) / torch.sum(w ** 2.0))).unsqueeze(0)
        spec = torch.stft(y, 400, hop_length=100, win_length=400, window=torch.hann_window(400), center=True,
                          pad_mode="reflect", normalized=False, return_complex=True)
        mag_in = (torch.abs(spec) ** 0.3).numpy()
        _, amp_g, _ = O.denoise(sd, meta["prefix"], w)
        assert mag_in.shape == (1, 201, 1 + n // 100)
        assert DI.solid(mag_in).mean() > 0.5 and DI.solid(amp_g.numpy()).mean() > 0.5, n
