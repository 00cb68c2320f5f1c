"""denoiser/infer.py: ``denoise(noisy_wav, model, hps)`` with the reference's signature.  torch.stft / torch.istft
(third party) are restated as the framing kernel of the prompt mel front-end, a DFT product on the MFMA GEMM against a
host-built (float64 -> fp32) basis, and an overlap-add kernel; magnitude compression, phase and the polar
re-composition are pointwise launches.  One host synchronisation: the norm factor ``sqrt(len / sum(x^2))`` is read
back once (prompt pre-processing, outside any timed path).  ``denoise_batch`` is the same call for B prompts in one
packed pass with no read-back at all."""
from __future__ import annotations

import math

import numpy as np
import torch
from torch import nn

from .. import _lib as L
from .. import functional as Fh
from ..hip_layers import Conv1d, finalize as _finalize


class _Stft(nn.Module):
    """Forward and inverse DFT bases of a (n_fft, hop) pair as packed 1 x 1 conv weights, plus the Hann window."""

    def __init__(self, n_fft, hop_size, win_size):
        super().__init__()
        if win_size != n_fft or n_fft % 2:
            raise L.HspError("denoiser STFT: only win_size == n_fft (even) is built")
        self.n_fft, self.hop, self.n_freqs = n_fft, hop_size, n_fft // 2 + 1
        nf = self.n_freqs
        n = np.arange(n_fft, dtype=np.float64)
        f = np.arange(nf, dtype=np.float64)
        ang = 2.0 * np.pi * ((f[:, None] * n[None, :]) % n_fft) / n_fft
        self.dft = Conv1d(n_fft, 2 * nf, 1, bias=False)           # rows: cos | -sin   (torch.stft, onesided)
        self.idft = Conv1d(2 * nf, n_fft, 1, bias=False)          # irfft: DC / Nyquist once, the others twice; their
        wgt = np.full(nf, 2.0)                                    # imaginary parts are ignored as a C2R FFT does
        wgt[0] = wgt[-1] = 1.0
        inv = np.concatenate([np.cos(ang) * wgt[:, None], -np.sin(ang) * wgt[:, None]], 0).T / n_fft   # [n_fft, 2 nf]
        inv[:, nf] = 0.0
        inv[:, 2 * nf - 1] = 0.0
        with torch.no_grad():
            self.dft.weight.copy_(torch.from_numpy(np.concatenate([np.cos(ang), -np.sin(ang)], 0).astype(np.float32))
                                  .reshape(self.dft.weight.shape))
            self.idft.weight.copy_(torch.from_numpy(inv.astype(np.float32)).reshape(self.idft.weight.shape))
        self._window = None

    def finalize(self, device):
        _finalize(self, device)
        self._window = torch.hann_window(self.n_fft, periodic=True, dtype=torch.float32).to(device)
        return self


_STFT = {}


def _stft_for(device, n_fft, hop_size, win_size):
    key = (device.type, device.index, n_fft, hop_size, win_size)
    if key not in _STFT:
        _STFT[key] = _Stft(n_fft, hop_size, win_size).finalize(device)
    return _STFT[key]


def mag_pha_stft(y, n_fft, hop_size, win_size, compress_factor=1.0, center=True):
    """infer.py:12-24: y [1, L] -> (mag [1, F, T], pha [1, F, T], com [1, F, T, 2])."""
    if not center or y.dim() != 2 or y.shape[0] != 1:
        raise L.HspError("mag_pha_stft: one utterance [1, L], center=True")
    if not y.is_cuda or y.dtype != torch.float32:
        raise L.HspError("the denoiser runs on the GPU in float32 only; there is no CPU fallback")
    st = _stft_for(y.device, n_fft, hop_size, win_size)
    y = y.contiguous()
    Ls = y.shape[1]
    if Ls <= n_fft // 2:
        raise L.HspError(f"mag_pha_stft: reflect padding needs more than {n_fft // 2} samples, got {Ls}")
    T = 1 + Ls // hop_size
    f_ld = (T + 3) & ~3
    frames = torch.empty(1, n_fft, f_ld, dtype=torch.float32, device=y.device)
    L.check(L.lib().hsp_stft_frames_f32(L.fptr(y), L.fptr(st._window), L.fptr(frames), 1, Ls, n_fft, hop_size, T, f_ld,
                                        L.stream_ptr()), "hsp_stft_frames_f32")
    spec = st.dft(frames)                                          # [1, 2 F, f_ld]: real | imaginary rows
    nf = st.n_freqs
    mag = torch.empty(1, nf, T, dtype=torch.float32, device=y.device)
    pha = torch.empty(1, nf, T, dtype=torch.float32, device=y.device)
    L.check(L.lib().hsp_mag_pha_f32(L.fptr(spec), spec.stride(1), L.fptr(mag), L.fptr(pha), nf, T, float(compress_factor),
                                    L.stream_ptr()), "hsp_mag_pha_f32")
    return mag, pha, _com(mag, pha)


def _com(mag, pha):
    _, nf, T = mag.shape
    re = torch.empty(nf, T, dtype=torch.float32, device=mag.device)
    im = torch.empty(nf, T, dtype=torch.float32, device=mag.device)
    L.check(L.lib().hsp_polar_f32(L.fptr(mag), L.fptr(pha), 1.0, L.fptr(re), T, L.fptr(im), T, nf, T, L.stream_ptr()),
            "hsp_polar_f32")
    return torch.stack((re, im), dim=-1).unsqueeze(0)


def mag_pha_istft(mag, pha, n_fft, hop_size, win_size, compress_factor=1.0, center=True, scale=1.0):
    """infer.py:26-32: mag, pha [1, F, T] -> wav [1, hop (T - 1)] (times ``scale``)."""
    if not center or mag.dim() != 3 or mag.shape[0] != 1 or mag.shape != pha.shape:
        raise L.HspError("mag_pha_istft: one utterance [1, F, T], center=True")
    st = _stft_for(mag.device, n_fft, hop_size, win_size)
    mag, pha = mag.contiguous(), pha.contiguous()
    _, nf, T = mag.shape
    if nf != st.n_freqs or T < 2:
        raise L.HspError(f"mag_pha_istft: expected {st.n_freqs} bins and at least two frames")
    t_ld = (T + 3) & ~3
    spec = torch.zeros(1, 2 * nf, t_ld, dtype=torch.float32, device=mag.device)
    L.check(L.lib().hsp_polar_f32(L.fptr(mag), L.fptr(pha), 1.0 / float(compress_factor), L.fptr(spec), t_ld,
                                  L.fptr(spec[0, nf:]), t_ld, nf, T, L.stream_ptr()), "hsp_polar_f32")
    frames = st.idft(spec)                                         # [1, n_fft, t_ld]
    wav = torch.empty(1, hop_size * (T - 1), dtype=torch.float32, device=mag.device)
    L.check(L.lib().hsp_istft_ola_f32(L.fptr(frames), frames.stride(1), L.fptr(st._window), L.fptr(wav), n_fft, hop_size, T,
                                      float(scale), L.stream_ptr()), "hsp_istft_ola_f32")
    return wav


@torch.no_grad()
def denoise(noisy_wav, model, hps):
    """infer.py:3-10: noisy_wav [L] on the GPU -> denoised [1, hop (T - 1)]."""
    if noisy_wav.dim() != 1:
        raise L.HspError("denoise takes one 1-D waveform, as the reference")
    if not noisy_wav.is_cuda or noisy_wav.dtype != torch.float32:
        raise L.HspError("the denoiser runs on the GPU in float32 only; there is no CPU fallback")
    x = noisy_wav.contiguous()
    ss = torch.empty(1, dtype=torch.float32, device=x.device)
    L.check(L.lib().hsp_sum_sq_f32(L.fptr(x), x.numel(), L.fptr(ss), L.stream_ptr()), "hsp_sum_sq_f32")
    ssv = float(ss.item())
    if not ssv > 0.0:
        raise L.HspError("denoise(): the prompt is silent (sum of squares 0); the reference's norm factor is inf there "
                         "and its output NaN")
    norm = math.sqrt(x.numel() / ssv)
    y = Fh.axpby(x, x, norm, 0.0).unsqueeze(0)
    amp, pha, _ = mag_pha_stft(y, hps.n_fft, hps.hop_size, hps.win_size, hps.compress_factor)
    amp_g, pha_g, _ = model(amp, pha)
    return mag_pha_istft(amp_g, pha_g, hps.n_fft, hps.hop_size, hps.win_size, hps.compress_factor, scale=1.0 / norm)


# ------------------------------------------------------------------ ragged batches
def _pad_rows(wavs, lengths):
    """A list of 1-D device rows, or padded [B, L_max] + HOST lengths -> (padded fp32 [B, L_max], host lengths)."""
    from .packed import host_ints
    if isinstance(wavs, torch.Tensor):
        if wavs.dim() != 2 or lengths is None:
            raise L.HspError("denoise_batch takes a list of 1-D waveforms, or padded [B, L_max] with host lengths")
        lens = host_ints(lengths, "denoise_batch lengths")
        if len(lens) != wavs.shape[0] or max(lens) > wavs.shape[1]:
            raise L.HspError(f"denoise_batch: lengths {lens} do not fit rows of shape {tuple(wavs.shape)}")
        x = wavs
    else:
        rows = list(wavs)
        if not rows or any(r.dim() != 1 for r in rows):
            raise L.HspError("denoise_batch takes a list of 1-D waveforms, or padded [B, L_max] with host lengths")
        lens = [int(r.shape[0]) for r in rows]
        if lengths is not None and host_ints(lengths, "denoise_batch lengths") != lens:
            raise L.HspError("denoise_batch: lengths differ from the rows' own")
        x = torch.zeros(len(rows), max(lens), dtype=torch.float32, device=rows[0].device)
        for b, r in enumerate(rows):
            if r.dtype != torch.float32:
                raise L.HspError("the denoiser runs on the GPU in float32 only; there is no CPU fallback")
            x[b, :lens[b]].copy_(r)
    if not x.is_cuda or x.dtype != torch.float32:
        raise L.HspError("the denoiser runs on the GPU in float32 only; there is no CPU fallback")
    return x.contiguous(), lens


def _unpack(t, seg, T_max):
    """packed [1, F, T_tot] -> [B, F, T_max], zero past each row's frames (copies, no arithmetic)."""
    out = torch.zeros(seg.B, t.shape[1], T_max, dtype=torch.float32, device=t.device)
    for b, sl in enumerate(seg.slices()):
        out[b, :, :seg.frames[b]].copy_(t[0, :, sl])
    return out


def _stft_packed(y, lens, seg, st, compress_factor, scale=None):
    """y [B, L_max] with host lengths -> packed (mag, pha) [1, F, T_tot] in the layout of ``seg``; ``scale`` (device
    fp32 [B]) multiplies row b inside the framing.  Gap columns come out as magnitude 0, phase 0."""
    B, Lm = y.shape
    n_fft, hop, nf = st.n_fft, st.hop, st.n_freqs
    if min(lens) <= n_fft // 2:
        raise L.HspError(f"mag_pha_stft_batch: reflect padding needs more than {n_fft // 2} samples per row, got {lens}")
    from .packed import device_lengths
    dlen = device_lengths(lens, y.device)
    f_ld = (seg.T_tot + 3) & ~3
    frames = torch.empty(1, n_fft, f_ld, dtype=torch.float32, device=y.device)
    L.check(L.lib().hsp_stft_frames_packed_f32(L.fptr(y), y.stride(0), L.ptr(dlen), L.fptr(scale), L.fptr(st._window),
                                               L.fptr(frames), *seg.args(), Lm, n_fft, hop, seg.T_tot, f_ld,
                                               L.stream_ptr()), "hsp_stft_frames_packed_f32")
    spec = st.dft(frames)                                          # [1, 2 F, f_ld]: column-wise, so it serves unchanged
    mag = torch.empty(1, nf, seg.T_tot, dtype=torch.float32, device=y.device)
    pha = torch.empty(1, nf, seg.T_tot, dtype=torch.float32, device=y.device)
    L.check(L.lib().hsp_mag_pha_f32(L.fptr(spec), spec.stride(1), L.fptr(mag), L.fptr(pha), nf, seg.T_tot,
                                    float(compress_factor), L.stream_ptr()), "hsp_mag_pha_f32")
    return mag, pha


def _istft_packed(mag, pha, seg, st, compress_factor, inv=None):
    """packed mag, pha [1, F, T_tot] -> (wav [B, n_max], host lengths hop (T_b - 1)); row b times inv[b]."""
    n_fft, hop, nf = st.n_fft, st.hop, st.n_freqs
    T = seg.T_tot
    mag, pha = mag.contiguous(), pha.contiguous()
    t_ld = (T + 3) & ~3
    spec = torch.zeros(1, 2 * nf, t_ld, dtype=torch.float32, device=mag.device)
    L.check(L.lib().hsp_polar_f32(L.fptr(mag), L.fptr(pha), 1.0 / float(compress_factor), L.fptr(spec), t_ld,
                                  L.fptr(spec[0, nf:]), t_ld, nf, T, L.stream_ptr()), "hsp_polar_f32")
    frames = st.idft(spec)                                         # [1, n_fft, t_ld]
    out_len = [hop * (n - 1) for n in seg.frames]
    n_max = max(1, max(out_len))
    wav = torch.empty(seg.B, n_max, dtype=torch.float32, device=mag.device)
    L.check(L.lib().hsp_istft_ola_seg_f32(L.fptr(frames), frames.stride(1), L.fptr(st._window), L.fptr(inv), L.fptr(wav),
                                          n_max, n_max, n_fft, hop, *seg.args(), T, L.stream_ptr()),
            "hsp_istft_ola_seg_f32")
    return wav, out_len


def mag_pha_stft_batch(y, lengths, n_fft, hop_size, win_size, compress_factor=1.0, center=True, scale=None):
    """``mag_pha_stft`` on the rows of y [B, L_max] at their own HOST ``lengths`` (samples), in one packed pass: ->
    (mag [B, F, T_max], pha [B, F, T_max], com [B, F, T_max, 2]), T_b = 1 + lengths[b] // hop frames per row, zeros
    after.  ``scale`` (device fp32 [B]): row b is multiplied by scale[b] first."""
    from .packed import host_ints, segments_for
    if not center or y.dim() != 2:
        raise L.HspError("mag_pha_stft_batch: padded rows [B, L_max], center=True")
    if not y.is_cuda or y.dtype != torch.float32:
        raise L.HspError("the denoiser runs on the GPU in float32 only; there is no CPU fallback")
    lens = host_ints(lengths, "mag_pha_stft_batch lengths")
    if len(lens) != y.shape[0] or max(lens) > y.shape[1]:
        raise L.HspError(f"mag_pha_stft_batch: lengths {lens} do not fit rows of shape {tuple(y.shape)}")
    st = _stft_for(y.device, n_fft, hop_size, win_size)
    seg = segments_for([1 + n // hop_size for n in lens], y.device)
    mag, pha = _stft_packed(y.contiguous(), lens, seg, st, compress_factor, scale)
    T_max = max(seg.frames)
    mag, pha = _unpack(mag, seg, T_max), _unpack(pha, seg, T_max)
    B, nf = seg.B, st.n_freqs
    re = torch.empty(B * nf, T_max, dtype=torch.float32, device=y.device)
    im = torch.empty(B * nf, T_max, dtype=torch.float32, device=y.device)
    L.check(L.lib().hsp_polar_f32(L.fptr(mag), L.fptr(pha), 1.0, L.fptr(re), T_max, L.fptr(im), T_max, B * nf, T_max,
                                  L.stream_ptr()), "hsp_polar_f32")
    return mag, pha, torch.stack((re, im), dim=-1).reshape(B, nf, T_max, 2)


def mag_pha_istft_batch(mag, pha, lengths, n_fft, hop_size, win_size, compress_factor=1.0, center=True, scale=None):
    """``mag_pha_istft`` on the rows of mag, pha [B, F, T_max] at their own HOST ``lengths`` (frames, >= 2) -> (wav
    [B, n_max], lengths hop (T_b - 1)); row b is multiplied by scale[b] (device fp32 [B]) and zero past its end."""
    from .packed import host_ints, segments_for
    if not center or mag.dim() != 3 or mag.shape != pha.shape:
        raise L.HspError("mag_pha_istft_batch: mag / pha [B, F, T_max], center=True")
    frames = host_ints(lengths, "mag_pha_istft_batch lengths")
    st = _stft_for(mag.device, n_fft, hop_size, win_size)
    if len(frames) != mag.shape[0] or mag.shape[1] != st.n_freqs or max(frames) > mag.shape[2] or min(frames) < 2:
        raise L.HspError(f"mag_pha_istft_batch: expected {st.n_freqs} bins and 2 .. T_max frames per row, got {frames}")
    seg = segments_for(frames, mag.device)
    pk = [torch.zeros(1, st.n_freqs, seg.T_tot, dtype=torch.float32, device=mag.device) for _ in range(2)]
    for dst, src in zip(pk, (mag, pha)):
        for b, sl in enumerate(seg.slices()):
            dst[0, :, sl].copy_(src[b, :, :frames[b]])
    return _istft_packed(pk[0], pk[1], seg, st, compress_factor, scale)


# a packed row of T holds, in floats: the dense buffers 5 x 64 x F (encoder at F = 201, the two decoders at F' = 100),
# the conformers' 4 x 64 x F' feed-forward and 3 x 64 x F' q/k/v activations and a few [64, F] temporaries
BYTES_PER_ROW = 4 * (5 * 64 * 201 + 2 * 5 * 64 * 100 + 7 * 64 * 100 + 4 * 64 * 201)


@torch.no_grad()
def denoise_batch(wavs, model, hps, lengths=None, max_rows: int = 8192, return_spectrogram: bool = False):
    """``denoise`` for B prompts in one packed pass.

    wavs     a list of B 1-D fp32 device waveforms, or padded fp32 [B, L_max] with HOST ``lengths`` (samples);
    returns  (out fp32 [B, n_max], out_lengths): row b holds ``denoise(wavs[b])`` on ``out_lengths[b] = hop *
             (lengths[b] // hop)`` samples (host ints) and zeros after.  With ``return_spectrogram`` also the
             (mag, pha) [B, F, T_max] the network was given, zero past each row's 1 + lengths[b] // hop frames.

    The call copies nothing to the host and never synchronises -- the norm factor sqrt(len / sum x^2) of every row
    stays on the device (``hsp_norm_factor_rows_f32``) -- so a fixed set of lengths can be captured in a hipGraph.
    One difference from ``denoise``: a silent row cannot raise without a read-back; it comes out as zeros (scale and
    inverse scale 0) and the other rows are untouched.

    Memory: every row of the packed T axis (one STFT frame, 1 / 160 s, plus 8 gap rows between prompts) holds about
    ``BYTES_PER_ROW`` = 0.9 MB of activations at its peak -- the dense buffers alone are 5 x 64 x F floats per row.
    When the packed row count would exceed ``max_rows`` (8192: about 50 s of prompts, 7.4 GB) the batch runs as
    consecutive sub-batches of whole prompts."""
    from .packed import device_lengths, segments_for, split_rows
    x, lens = _pad_rows(wavs, lengths)
    hop = hps.hop_size
    st = _stft_for(x.device, hps.n_fft, hop, hps.win_size)
    if min(lens) <= hps.n_fft // 2:
        raise L.HspError(f"denoise_batch: reflect padding needs more than {hps.n_fft // 2} samples per row, got {lens}")
    B, Lm = x.shape
    frames = [1 + n // hop for n in lens]
    dlen = device_lengths(lens, x.device)
    scale = torch.empty(B, dtype=torch.float32, device=x.device)
    inv = torch.empty(B, dtype=torch.float32, device=x.device)
    L.check(L.lib().hsp_norm_factor_rows_f32(L.fptr(x), x.stride(0), L.ptr(dlen), L.fptr(scale), L.fptr(inv), B, Lm,
                                             L.stream_ptr()), "hsp_norm_factor_rows_f32")
    out_len = [hop * (n - 1) for n in frames]
    n_max, T_max = max(out_len), max(frames)
    groups = split_rows(frames, max_rows)
    out = torch.zeros(B, n_max, dtype=torch.float32, device=x.device) if len(groups) > 1 else None
    spec = [torch.zeros(B, st.n_freqs, T_max, dtype=torch.float32, device=x.device) for _ in range(2)] \
        if return_spectrogram else None
    for rows in groups:
        b0, b1 = rows[0], rows[-1] + 1
        seg = segments_for(frames[b0:b1], x.device)
        amp, pha = _stft_packed(x[b0:b1], lens[b0:b1], seg, st, hps.compress_factor, scale[b0:b1])
        if spec is not None:
            for dst, src in zip(spec, (amp, pha)):
                dst[b0:b1, :, :max(seg.frames)].copy_(_unpack(src, seg, max(seg.frames)))
        amp_g, pha_g, _ = model.forward_packed(amp, pha, seg)
        wav, _ = _istft_packed(amp_g, pha_g, seg, st, hps.compress_factor, inv[b0:b1])
        if out is None:
            out = wav
        else:
            out[b0:b1, :wav.shape[1]].copy_(wav)
    return (out, out_len, tuple(spec)) if return_spectrogram else (out, out_len)
