"""GPU (-m gpu): the three STFT framing entry points of csrc/hsp_mel.hip (plain, ragged rows, rows packed into one
matrix) and the two reflect-pad entry points of csrc/hsp_pointwise.hip, each called through the C ABI against the float32
restatements of tests/glue_ref.py.  Both operations are exact -- framing is one fp32 multiply per element (two with a
scale, in the order w * (x * scale)), padding is a copy -- so every comparison is on bits, the zeroed pitch, past-the-row
and gap columns included, and the same rows through the plain, ragged and packed forms must agree bit for bit.

Shapes (glue_ref.FRAME_*): n_fft = 320, hop = 5 with L = 347 (70 frames: a second 64-frame tile, part-filled; a second
256-position block) and L = 161 = n_fft / 2 + 1 (the shortest legal row: both edges reflect inside one frame); n_fft =
100, hop = 7 for a part-filled 64-position group; ragged and packed rows of 347, 161 and 200 samples, the row pitch
rounded up to 4 and 3 gap columns between packed segments.  Samples past a row's length are NaN: never read.  Every
output sits between canaries.  tests/test_glue_ref_host.py pins the restatements against torch on a CPU.

    python -m pytest tests/test_gpu_framing_contract.py -q -m gpu
"""
import ctypes

import numpy as np
import pytest
import torch

import glue_ref as R
from test_gpu_glue_kernels import SENT, _bits, _buf, _call, _dev, _flat, _outside_untouched

pytestmark = pytest.mark.gpu

N_FFT, HOP = R.FRAME_N_FFT, R.FRAME_HOP


@pytest.fixture(scope="module")
def lib():
    from megatts2_hierspeechpp_amd import _lib as L
    return L


def _rows(x, device, pitch_extra=0, lengths=None):
    """x [B, L] on the device in rows of pitch L + pitch_extra (the slack filled with 9e9), NaN past lengths[b]."""
    B, L = x.shape
    _, xv = _buf((B, L + pitch_extra), (slice(None), slice(0, L)), device, fill=9.0e9)
    xv.copy_(_dev(x, device))
    for b, n in enumerate(lengths if lengths is not None else ()):
        xv[b, n:] = float("nan")
    return xv


def _plain(lib, device, x, w, hop, T=None, f_ld=None):
    B, L = x.shape
    T = 1 + L // hop if T is None else T
    f_ld = R.frame_ld(T) if f_ld is None else f_ld
    xd, wd = _rows(x, device), _dev(w, device)
    buf, sl, fr = _flat((B, len(w), f_ld), device)
    code = lib.lib().hsp_stft_frames_f32(lib.fptr(xd), lib.fptr(wd), lib.fptr(fr), B, L, len(w), hop, T, f_ld,
                                         lib.stream_ptr())
    return code, buf, sl, fr


def _ragged(lib, device, x, lengths, w, hop, T=None, null_lengths=False, x_bs=None):
    B, L = x.shape
    T = 1 + L // hop if T is None else T
    f_ld = R.frame_ld(T)
    xd, wd = _rows(x, device, 3, lengths), _dev(w, device)
    ld = _dev(np.asarray(lengths, np.int64), device)
    buf, sl, fr = _flat((B, len(w), f_ld), device)
    code = lib.lib().hsp_stft_frames_ragged_f32(lib.fptr(xd), xd.stride(0) if x_bs is None else x_bs,
                                                None if null_lengths else lib.ptr(ld), lib.fptr(wd), lib.fptr(fr), B, L,
                                                len(w), hop, T, f_ld, lib.stream_ptr())
    return code, buf, sl, fr


def _packed(lib, device, x, lengths, w, hop, first, frames, T_tot, scale=None, f_ld=None, L=None):
    B, Lx = x.shape
    f_ld = R.frame_ld(T_tot) if f_ld is None else f_ld
    xd, wd = _rows(x, device, 3, lengths), _dev(w, device)
    ld = _dev(np.asarray(lengths, np.int64), device)
    flat = [v for b in range(B) for v in (first[b], frames[b])]
    host = (ctypes.c_int32 * len(flat))(*flat)
    seg = _dev(np.asarray(flat, np.int32), device)
    sc = _dev(np.asarray(scale, np.float32), device) if scale is not None else None
    buf, sl, fr = _flat((len(w), f_ld), device)
    code = lib.lib().hsp_stft_frames_packed_f32(lib.fptr(xd), xd.stride(0), lib.ptr(ld), lib.fptr(sc), lib.fptr(wd),
                                                lib.fptr(fr), lib.ptr(seg), ctypes.cast(host, ctypes.c_void_p), B,
                                                Lx if L is None else L, len(w), hop, T_tot, f_ld, lib.stream_ptr())
    return code, buf, sl, fr


def _got(code, buf, sl, fr, name):
    _call(code)
    _outside_untouched(buf, sl, name)
    return fr.cpu().numpy()


# ------------------------------------------------------------------------------------------------ framing
@pytest.mark.parametrize("n_fft,hop,L", [(N_FFT, HOP, L) for L in R.FRAME_LS] + [(100, 7, 120)])
def test_one_row_through_plain_ragged_and_packed_forms(n_fft, hop, L, device, lib):
    """Two whole rows: every form against the restatement, and so against each other, bit for bit."""
    x, w = R.frame_rows(2, L, seed=4000 + L), R.frame_window(n_fft)
    T = 1 + L // hop
    want = R.stft_frames_ragged(x, [L, L], w, hop, R.frame_ld(T))
    assert (want[:, 1:, :T] != 0).all() and (want[:, :, T:] == 0).all()       # only w[0] = 0 and the pitch columns
    plain = _got(*_plain(lib, device, x, w, hop), f"stft_frames L={L}")
    _bits(plain, want, f"stft_frames L={L}")
    ragged = _got(*_ragged(lib, device, x, [L, L], w, hop), f"stft_frames_ragged L={L}")
    _bits(ragged, want, f"stft_frames_ragged len = L = {L}")
    for b in range(2):
        for scale in (None, [R.FRAME_SCALE[b]]):
            got = _got(*_packed(lib, device, x[b:b + 1], [L], w, hop, [0], [T], T, scale), f"stft_frames_packed L={L}")
            if scale is None:
                _bits(got, plain[b], f"stft_frames_packed, one segment, L={L} row {b}")
            _bits(got, R.stft_frames_packed(x[b:b + 1], [L], w, hop, [0], R.frame_ld(T), scale),
                  f"stft_frames_packed, one segment, scale {scale}, L={L} row {b}")


def test_ragged_rows(device, lib):
    lens = list(R.FRAME_RAGGED)
    x, w = R.frame_rows(3, max(lens), seed=4100), R.frame_window()
    T = 1 + max(lens) // HOP
    want = R.stft_frames_ragged(x, lens, w, HOP, R.frame_ld(T))
    got = _got(*_ragged(lib, device, x, lens, w, HOP), "stft_frames_ragged")
    _bits(got, want, f"stft_frames_ragged {lens}")
    for b, n in enumerate(lens):                                               # zeros past each row's own frames
        assert not got[b, :, 1 + n // HOP:].any()
        solo = _got(*_plain(lib, device, x[b:b + 1, :n], w, HOP), "stft_frames")
        _bits(got[b, :, :1 + n // HOP], solo[0, :, :1 + n // HOP], f"ragged row {b} against its own plain call")


@pytest.mark.parametrize("scaled", [False, True], ids=["no_scale", "scale"])
def test_packed_rows(scaled, device, lib):
    lens = list(R.FRAME_RAGGED)
    first, frames, T_tot = R.packed_table(lens)
    assert first == [0, 73, 109] and frames == [70, 33, 41] and T_tot == 150 and R.frame_ld(T_tot) == 152
    x, w = R.frame_rows(3, max(lens), seed=4200), R.frame_window()
    scale = R.FRAME_SCALE if scaled else None
    want = R.stft_frames_packed(x, lens, w, HOP, first, R.frame_ld(T_tot), scale)
    got = _got(*_packed(lib, device, x, lens, w, HOP, first, frames, T_tot, scale), "stft_frames_packed")
    _bits(got, want, f"stft_frames_packed {lens} scale {scale}")
    keep = np.zeros(got.shape[1], bool)
    for s, n in zip(first, frames):
        keep[s:s + n] = True
    assert keep.sum() == sum(frames) and not got[:, ~keep].any()               # gap and pitch columns: zeros


def test_framing_launchers_refuse_what_distinguishes_them(device, lib):
    """Each refusal beside a call that differs in that one argument and is accepted; a refused call writes nothing."""
    E = lib.EINVAL
    L = 347
    x, w = R.frame_rows(1, L, seed=4300), R.frame_window()

    def refused(code, buf, sl, fr):
        torch.cuda.synchronize()
        return code == E and bool((buf == SENT).all())

    def accepted(code, buf, sl, fr):
        torch.cuda.synchronize()
        return code == 0

    # plain: any T whose last frame's centre lies inside the signal; ragged: exactly T = 1 + L / hop
    assert accepted(*_plain(lib, device, x, w, HOP, T=70)) and accepted(*_plain(lib, device, x, w, HOP, T=69))
    assert refused(*_plain(lib, device, x, w, HOP, T=71))                      # (T - 1) hop = 350 > 347
    assert refused(*_plain(lib, device, x, w, HOP, T=70, f_ld=69))             # row pitch below T
    assert accepted(*_ragged(lib, device, x, [L], w, HOP, T=70))
    assert refused(*_ragged(lib, device, x, [L], w, HOP, T=69)) and refused(*_ragged(lib, device, x, [L], w, HOP, T=71))
    assert refused(*_ragged(lib, device, x, [L], w, HOP, null_lengths=True))   # the ragged entry point needs lengths
    assert refused(*_ragged(lib, device, x, [L], w, HOP, x_bs=L - 1))         # x_bs < L
    # packed: the segment-table checks, and no row with more frames than 1 + L / hop
    assert accepted(*_packed(lib, device, x, [L], w, HOP, [0], [70], 70))
    assert accepted(*_packed(lib, device, x, [L], w, HOP, [2], [60], 62))
    assert refused(*_packed(lib, device, x, [L], w, HOP, [0], [71], 71))       # 71 frames > 1 + 347 / 5
    assert refused(*_packed(lib, device, x, [L], w, HOP, [3], [70], 70))       # the segment ends past T_tot
    assert refused(*_packed(lib, device, x, [L], w, HOP, [0], [70], 70, f_ld=69))
    assert refused(*_packed(lib, device, x, [L], w, HOP, [0], [33], 33, L=160))   # L <= n_fft / 2
    two = R.frame_rows(2, L, seed=4301)
    assert accepted(*_packed(lib, device, two, [L, L], w, HOP, [0, 73], [70, 70], 143))
    assert refused(*_packed(lib, device, two, [L, L], w, HOP, [0, 69], [70, 70], 139))    # overlapping segments
    assert refused(*_packed(lib, device, two, [L, L], w, HOP, [73, 0], [70, 70], 143))    # not ascending


# ------------------------------------------------------------------------------------------------ reflect padding
@pytest.mark.parametrize("L,pad", R.PAD_SHAPES)
def test_reflect_pad_plain_and_ragged(L, pad, device, lib):
    """Plain on whole rows; ragged with full lengths (equal to plain, bit for bit) and with ragged ones."""
    B = 3
    x = R.frame_rows(B, L, seed=4400 + L)
    Lo = L + 2 * pad
    xv = _rows(x, device, 3)
    ybuf, ysl, y = _flat((B, Lo), device)
    _call(lib.lib().hsp_reflect_pad_f32(lib.fptr(xv), xv.stride(0), lib.fptr(y), B, L, pad, lib.stream_ptr()))
    _outside_untouched(ybuf, ysl, "reflect_pad")
    plain = y.cpu().numpy()
    _bits(plain, R.reflect_pad(x, pad), f"reflect_pad L={L} pad={pad}")
    for lens in ([L] * B, [L, pad + 1, max(pad + 1, (2 * L) // 3)]):
        xr = _rows(x, device, 3, lens)
        ld = _dev(np.asarray(lens, np.int64), device)
        # the output rows as columns [2, 2 + Lo) of a wider canary buffer: y_bs = Lo + 5
        ybuf, y = _buf((B, Lo + 5), (slice(None), slice(2, 2 + Lo)), device)
        _call(lib.lib().hsp_reflect_pad_ragged_f32(lib.fptr(xr), xr.stride(0), lib.ptr(ld), lib.fptr(y), y.stride(0), B, L,
                                                   pad, Lo, lib.stream_ptr()))
        _outside_untouched(ybuf, (slice(None), slice(2, 2 + Lo)), "reflect_pad_ragged")
        got = y.cpu().numpy()
        _bits(got, R.reflect_pad_ragged(x, lens, pad), f"reflect_pad_ragged L={L} pad={pad} lengths {lens}")
        if lens == [L] * B:
            _bits(got, plain, "reflect_pad_ragged with full lengths against reflect_pad")
