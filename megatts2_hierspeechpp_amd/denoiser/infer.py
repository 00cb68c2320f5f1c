"""denoiser/infer.py: ``denoise(noisy_wav, model, hps)`` with the reference's signature.  torch.stft / torch.istft
(third party) are restated as a framing kernel, a DFT product on the MFMA GEMM against a host-built (float64 -> fp32)
basis, and an overlap-add kernel; magnitude compression, phase and the polar re-composition are pointwise launches.
``denoise_batch`` runs B prompts in one packed pass with no read-back at all; ``denoise`` is that pass
on a segment table of one row, after its one host synchronisation: the norm factor ``sqrt(len / sum(x^2))`` is read
back once (prompt pre-processing, outside any timed path) so that a silent prompt can raise."""
from __future__ import annotations

import numpy as np
import torch
from torch import nn

from .. import _lib as L
from ..hip_layers import Conv1d, finalize as _finalize
from .packed import device_lengths, host_ints, segments_for, split_rows
from .utils import polar_pair


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
    Ls = y.shape[1]
    if Ls <= n_fft // 2:
        raise L.HspError(f"mag_pha_stft: reflect padding needs more than {n_fft // 2} samples, got {Ls}")
    st = _stft_for(y.device, n_fft, hop_size, win_size)
    mag, pha = _stft_packed(y.contiguous(), [Ls], segments_for([1 + Ls // hop_size], y.device), st, compress_factor)
    return mag, pha, polar_pair(mag, pha)


def mag_pha_istft(mag, pha, n_fft, hop_size, win_size, compress_factor=1.0, center=True, scale=1.0):
    """infer.py:26-32: mag, pha [1, F, T] -> wav [1, hop (T - 1)] (times ``scale``)."""
    if not center or mag.dim() != 3 or mag.shape[0] != 1 or mag.shape != pha.shape:
        raise L.HspError("mag_pha_istft: one utterance [1, F, T], center=True")
    st = _stft_for(mag.device, n_fft, hop_size, win_size)
    _, nf, T = mag.shape
    if nf != st.n_freqs or T < 2:
        raise L.HspError(f"mag_pha_istft: expected {st.n_freqs} bins and at least two frames")
    inv = None if scale == 1.0 else torch.full((1,), float(scale), dtype=torch.float32, device=mag.device)
    return _istft_packed(mag, pha, segments_for([T], mag.device), st, compress_factor, inv)[0]


@torch.no_grad()
def denoise(noisy_wav, model, hps):
    """infer.py:3-10: noisy_wav [L] on the GPU -> denoised [1, hop (T - 1)]."""
    if noisy_wav.dim() != 1:
        raise L.HspError("denoise takes one 1-D waveform, as the reference")
    if not noisy_wav.is_cuda or noisy_wav.dtype != torch.float32:
        raise L.HspError("the denoiser runs on the GPU in float32 only; there is no CPU fallback")
    x, lens = noisy_wav.contiguous().unsqueeze(0), [noisy_wav.shape[0]]
    scale, inv = _norm_factors(x, lens, hps, "denoise")
    if not float(scale[0]) > 0.0:                                   # the one read-back; a silent row has scale 0
        raise L.HspError("denoise(): the prompt is silent (sum of squares 0); the reference's norm factor is inf there "
                         "and its output NaN")
    return _denoise_rows(x, lens, scale, inv, model, hps)[0]


# ------------------------------------------------------------------ ragged batches
def _pad_rows(wavs, lengths):
    """A list of 1-D device rows, or padded [B, L_max] + HOST lengths -> (padded fp32 [B, L_max], host lengths)."""
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


def _stft_packed(y, lens, seg, st, compress_factor, scale=None):
    """y [B, L_max] with host lengths -> packed (mag, pha) [1, F, T_tot] in the layout of ``seg``; ``scale`` (device
    fp32 [B]) multiplies row b inside the framing.  Gap columns come out as magnitude 0, phase 0."""
    B, Lm = y.shape
    n_fft, hop, nf = st.n_fft, st.hop, st.n_freqs
    if min(lens) <= n_fft // 2:
        raise L.HspError(f"mag_pha_stft_batch: reflect padding needs more than {n_fft // 2} samples per row, got {lens}")
    dlen = device_lengths(lens, y.device)
    f_ld = (seg.T_tot + 3) & ~3
    frames = torch.empty(1, n_fft, f_ld, dtype=torch.float32, device=y.device)
    L.call("hsp_stft_frames_packed_f32", L.fptr(y), y.stride(0), L.ptr(dlen), L.fptr(scale), L.fptr(st._window),
           L.fptr(frames), *seg.args(), Lm, n_fft, hop, seg.T_tot, f_ld)
    spec = st.dft(frames)                                          # [1, 2 F, f_ld]: column-wise, so it serves unchanged
    mag = torch.empty(1, nf, seg.T_tot, dtype=torch.float32, device=y.device)
    pha = torch.empty(1, nf, seg.T_tot, dtype=torch.float32, device=y.device)
    L.call("hsp_mag_pha_f32", L.fptr(spec), spec.stride(1), L.fptr(mag), L.fptr(pha), nf, seg.T_tot,
           float(compress_factor))
    return mag, pha


def _istft_packed(mag, pha, seg, st, compress_factor, inv=None):
    """packed mag, pha [1, F, T_tot] -> (wav [B, n_max], host lengths hop (T_b - 1)); row b times inv[b]."""
    n_fft, hop, nf = st.n_fft, st.hop, st.n_freqs
    T = seg.T_tot
    mag, pha = mag.contiguous(), pha.contiguous()
    t_ld = (T + 3) & ~3
    spec = torch.zeros(1, 2 * nf, t_ld, dtype=torch.float32, device=mag.device)
    L.call("hsp_polar_f32", L.fptr(mag), L.fptr(pha), 1.0 / float(compress_factor), L.fptr(spec), t_ld,
           L.fptr(spec[0, nf:]), t_ld, nf, T)
    frames = st.idft(spec)                                         # [1, n_fft, t_ld]
    out_len = [hop * (n - 1) for n in seg.frames]
    n_max = max(1, max(out_len))
    wav = torch.empty(seg.B, n_max, dtype=torch.float32, device=mag.device)
    L.call("hsp_istft_ola_seg_f32", L.fptr(frames), frames.stride(1), L.fptr(st._window), L.fptr(inv), L.fptr(wav),
           n_max, n_max, n_fft, hop, *seg.args(), T)
    return wav, out_len


def mag_pha_stft_batch(y, lengths, n_fft, hop_size, win_size, compress_factor=1.0, center=True, scale=None):
    """``mag_pha_stft`` on the rows of y [B, L_max] at their own HOST ``lengths`` (samples), in one packed pass: ->
    (mag [B, F, T_max], pha [B, F, T_max], com [B, F, T_max, 2]), T_b = 1 + lengths[b] // hop frames per row, zeros
    after.  ``scale`` (device fp32 [B]): row b is multiplied by scale[b] first."""
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
    mag, pha = seg.unpack(mag, T_max), seg.unpack(pha, T_max)
    return mag, pha, polar_pair(mag, pha)


def mag_pha_istft_batch(mag, pha, lengths, n_fft, hop_size, win_size, compress_factor=1.0, center=True, scale=None):
    """``mag_pha_istft`` on the rows of mag, pha [B, F, T_max] at their own HOST ``lengths`` (frames, >= 2) -> (wav
    [B, n_max], lengths hop (T_b - 1)); row b is multiplied by scale[b] (device fp32 [B]) and zero past its end."""
    if not center or mag.dim() != 3 or mag.shape != pha.shape:
        raise L.HspError("mag_pha_istft_batch: mag / pha [B, F, T_max], center=True")
    frames = host_ints(lengths, "mag_pha_istft_batch lengths")
    st = _stft_for(mag.device, n_fft, hop_size, win_size)
    if len(frames) != mag.shape[0] or mag.shape[1] != st.n_freqs or max(frames) > mag.shape[2] or min(frames) < 2:
        raise L.HspError(f"mag_pha_istft_batch: expected {st.n_freqs} bins and 2 .. T_max frames per row, got {frames}")
    seg = segments_for(frames, mag.device)
    return _istft_packed(seg.pack(mag), seg.pack(pha), seg, st, compress_factor, scale)


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
    x, lens = _pad_rows(wavs, lengths)
    scale, inv = _norm_factors(x, lens, hps, "denoise_batch")
    out, spec = _denoise_rows(x, lens, scale, inv, model, hps, max_rows, return_spectrogram)
    out_len = [hps.hop_size * (n // hps.hop_size) for n in lens]
    return (out, out_len, spec) if return_spectrogram else (out, out_len)


def _norm_factors(x, lens, hps, who):
    """x [B, L_max] with host lengths -> the norm factor sqrt(len / sum x^2) of every row and its inverse, device fp32
    [B] each (0 for a silent row); nothing is read back."""
    if min(lens) <= hps.n_fft // 2:
        raise L.HspError(f"{who}: reflect padding needs more than {hps.n_fft // 2} samples per row, got {lens}")
    B, Lm = x.shape
    scale = torch.empty(B, dtype=torch.float32, device=x.device)
    inv = torch.empty(B, dtype=torch.float32, device=x.device)
    L.call("hsp_norm_factor_rows_f32", L.fptr(x), x.stride(0), L.ptr(device_lengths(lens, x.device)), L.fptr(scale),
           L.fptr(inv), B, Lm)
    return scale, inv


def _denoise_rows(x, lens, scale, inv, model, hps, max_rows: int = 8192, want_spec: bool = False):
    """The packed pass on x [B, L_max]: STFT of ``scale[b]`` times row b, the network, inverse STFT times ``inv[b]``, in
    sub-batches of at most ``max_rows`` packed rows -> (out [B, n_max], the (mag, pha) [B, F, T_max] the network was
    given if ``want_spec``, else None)."""
    hop = hps.hop_size
    st = _stft_for(x.device, hps.n_fft, hop, hps.win_size)
    B = x.shape[0]
    frames = [1 + n // hop for n in lens]
    n_max, T_max = hop * (max(frames) - 1), max(frames)
    groups = split_rows(frames, max_rows)
    out = torch.zeros(B, n_max, dtype=torch.float32, device=x.device) if len(groups) > 1 else None
    spec = tuple(torch.zeros(B, st.n_freqs, T_max, dtype=torch.float32, device=x.device) for _ in range(2)) \
        if want_spec else None
    for rows in groups:
        b0, b1 = rows[0], rows[-1] + 1
        seg = segments_for(frames[b0:b1], x.device)
        amp, pha = _stft_packed(x[b0:b1], lens[b0:b1], seg, st, hps.compress_factor, scale[b0:b1])
        if spec is not None:
            for dst, src in zip(spec, (amp, pha)):
                dst[b0:b1, :, :max(seg.frames)].copy_(seg.unpack(src, max(seg.frames)))
        amp_g, pha_g, _ = model.forward_packed(amp, pha, seg)
        wav, _ = _istft_packed(amp_g, pha_g, seg, st, hps.compress_factor, inv[b0:b1])
        if out is None:
            out = wav
        else:
            out[b0:b1, :wav.shape[1]].copy_(wav)
    return out, spec
