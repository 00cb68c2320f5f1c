"""HIP mirror of the tensor core of the reference's inference_plm.py (its ``tts()`` between mel
extraction and wav writing, :156-190, and the model bundle of ``model_load`` :203-263).

The prompt file ingest (:120-126: ``torchaudio.load``, first channel, kaiser-window resampling to 16 kHz) is
``audio.load`` + ``functional.resample`` (``tts_from_prompt_file``; ``tts_from_prompt(prompt_sr=...)``), and
``scale_norm='prompt'`` (:127-128,185-186) is ``tts_from_prompt(scale_norm="prompt")``; the int16 stage of every
harness here is one `output.OutputStage`.  Out of scope here (host plumbing, not the hot path): text cleaning /
phonemisation (``get_text``) -- callers hand over phone ids.  The prompt mel transform is
``Mels_preprocess.MelSpectrogramFixed``, the optional prompt denoiser ``denoiser.generator.MPNet`` +
``denoiser.infer.denoise`` (:142-147)."""
from __future__ import annotations

import math
from typing import Optional

import torch
from torch import nn

from . import _lib as L
from . import functional as Fh
from .hierspeechpp_speechsynthesizer import SynthesizerTrn
from .hip_layers import finalize as _finalize
from .output import SCALE_NORMS, OutputStage, output_rate, pack, prompt_peak  # noqa: F401  (re-exported names)
from .ttv_v1.t2w2v_transformer import Megatts2PLM1
from .ttv_v1.t2w2v_transformer import SynthesizerTrn as Text2W2V

# text/symbols_lmdh.py: len(symbols), len(tone_symbols), len(language_symbols)
N_VOCAB, N_TONE, N_LANGUAGE = 126, 11, 4


class TtsModels(nn.Module):
    """The ``hierspeech`` tuple of inference_plm.py:tts as one module: ``voc`` = net_g (the hierarchical
    synthesizer), ``ttv`` = text2w2v, ``plm`` = the prosody LM, optional ``sr`` = SpeechSR.  One weight
    arena for all of them -> one RCCL broadcast in a multi-GPU job."""

    def __init__(self, voc_cfg: dict, ttv_cfg: dict, speechsr: Optional[nn.Module] = None):
        super().__init__()
        self.voc = SynthesizerTrn(641, 61440 // 320, **voc_cfg)
        self.ttv = Text2W2V(N_VOCAB, N_TONE, N_LANGUAGE, 641, 320, 16000, 60, **ttv_cfg)
        self.plm = Megatts2PLM1()
        if speechsr is not None:
            self.sr = speechsr

    def finalize(self, device, materialize: bool = True):
        self.arena = _finalize(self, device, materialize)
        return self


def zero_below(x, thr: float):
    x = x.contiguous()
    y = torch.empty_like(x)
    L.call("hsp_zero_below_f32", L.fptr(x), float(thr), L.fptr(y), x.numel())
    return y


peak_int16 = Fh.peak_int16   # the int16 stage of the reference's tts() (inference_plm.py:185-188)


# the forms the output stage had before `output.OutputStage`, kept for their callers: thin delegates
def check_limiter(scale_norm: str, limiter: bool, return_stats: bool = False) -> None:
    OutputStage(scale_norm, limiter=limiter, return_stats=return_stats).check()


def int16_rows(audio, n_valid, rate: int, scale_norm: str, gain, target_lufs: float, *limiter_args, **limiter_kw):
    """`OutputStage.int16`; ``limiter_args`` / ``limiter_kw``: the fields of the stage from ``limiter`` on."""
    return OutputStage(scale_norm, target_lufs, *limiter_args, **limiter_kw).int16(audio, n_valid, rate, gain)


def output_gain(scale_norm: str, prompt_audio) -> float:
    return OutputStage(scale_norm).gain(prompt_audio)


def prompt_mels(mel_fn, audio, denoiser=None, hps_denoiser=None):
    """The two prompt mels of inference_plm.py:130-150: ``src_mel_ttv`` from the prompt zero-padded to the next
    multiple of 1600 samples (always at least one sample of padding, :131-134), and ``src_mel`` [2, 80, T] from the
    un-padded prompt stacked with itself (denoise_ratio = 0, :142-143) or with its denoised version cut to the same
    length (``denoiser`` = a finalized denoiser.generator.MPNet, ``hps_denoiser`` its config: :144-150; the denoiser
    sees the PADDED prompt, as in the reference).  ``audio`` [1, n] fp32 on the GPU, or [B, n] for B prompts of one
    length (``src_mel`` is [2B, 80, T] then: the B prompts' mels followed by the B denoised ones, and the denoiser runs
    them as one ``denoise_batch``); ``mel_fn`` a finalized Mels_preprocess.MelSpectrogramFixed."""
    n = audio.shape[-1]
    padded = torch.zeros(audio.shape[0], (n // 1600 + 1) * 1600, dtype=audio.dtype, device=audio.device)
    padded[:, :n].copy_(audio)
    src_mel_ttv = mel_fn(padded)
    if denoiser is None:
        src_mel = mel_fn(audio)
        src_mel = src_mel.repeat(2, 1, 1) if src_mel.shape[0] == 1 else torch.cat([src_mel, src_mel], 0)
        return src_mel_ttv, src_mel
    if audio.shape[0] != 1:
        # B prompts of one length: each padded, denoised and cut as the single prompt below, in one packed pass
        from .denoiser.infer import denoise_batch
        den, _ = denoise_batch(padded, denoiser, hps_denoiser, lengths=[padded.shape[-1]] * audio.shape[0])
        both = torch.cat([padded, den[:, :padded.shape[-1]]], 0)[:, :n]   # [2B, n]: the B prompts, then the B denoised
        return src_mel_ttv, mel_fn(both.contiguous())
    from .denoiser.infer import denoise
    den = denoise(padded[0], denoiser, hps_denoiser)                  # [1, len(padded)] (1600 is a multiple of the hop)
    both = torch.cat([padded, den[:, :padded.shape[-1]]], 0)[:, :n]   # :147,150 (copies, no arithmetic)
    return src_mel_ttv, mel_fn(both.contiguous())


def write_wav(path, sample_rate: int, pcm):
    """scipy.io.wavfile.write(path, rate, int16 array) of inference_plm.py:195-200: 16-bit mono PCM RIFF."""
    import wave
    import numpy as np
    a = pcm.detach().cpu().numpy() if isinstance(pcm, torch.Tensor) else np.asarray(pcm)
    if a.dtype != np.int16 or a.ndim != 1:
        raise ValueError("write_wav takes a 1-D int16 array (one utterance)")
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(int(sample_rate))
        f.writeframes(a.astype("<i2").tobytes())


@torch.no_grad()
def prosody_from_audio(models: TtsModels, mel_fn, audio, sr: int = 16000, lengths=None):
    """Prosody codes of recorded speech: ``audio`` fp32 [B, n] (or [n]) on the GPU at rate ``sr``, ``lengths`` int64 [B]
    samples per row (device tensor; None: every row is n samples) -> (codes int64 [B, T], frames int64 [B]).
    Resampled to 16 kHz when ``sr`` differs (kaiser window, as the prompt ingest), mel by ``mel_fn`` (a finalized
    Mels_preprocess.MelSpectrogramFixed), then ``SynthesizerTrn.prosody_codes``: every code held for 8 frames, zeros
    from frames[b] on.  Nothing is read back to the host."""
    if audio.dim() == 1:
        audio = audio.unsqueeze(0)
    if int(sr) != 16000:
        audio = Fh.resample(audio, sr, 16000, resampling_method="kaiser_window", lengths=lengths)
        if lengths is not None:
            lengths = (lengths.to(torch.int64) * 16000 + int(sr) - 1) // int(sr)
    if lengths is None:
        mel = mel_fn(audio)
        frames = torch.full((audio.shape[0],), mel.shape[2], dtype=torch.int64, device=audio.device)
    else:
        mel, frames = mel_fn(audio, lengths)
    return models.ttv.prosody_codes(mel, frames), frames


def fit_prosody_codes(codes, src_frames, dst_frames, width: Optional[int] = None):
    """Stretch or compress held prosody codes to another frame count by centre-aligned nearest index: row b's target
    frame t < Lt takes its source index ((2 t + 1) Ls) // (2 Lt), Ls = src_frames[b], Lt = dst_frames[b] (the identity
    when Ls == Lt); entries from Lt on are zero.  codes int64 [B, Ts] (or [Ts]); the frame counts are int tensors [B]
    (or ints).  -> int64 [B, width]; ``width`` None: max(dst_frames), which reads it back when it is a device tensor."""
    if codes.dim() == 1:
        codes = codes.unsqueeze(0)
    B, dev = codes.shape[0], codes.device
    as_col = lambda v: torch.as_tensor(v, dtype=torch.int64, device=dev).reshape(-1, 1).expand(B, 1)  # noqa: E731
    ls, lt = as_col(src_frames), as_col(dst_frames)
    if width is None:
        width = int(lt.max().item())
    t = torch.arange(width, dtype=torch.int64, device=dev).unsqueeze(0)
    idx = torch.div((2 * t + 1) * ls, 2 * lt.clamp(min=1), rounding_mode="floor").clamp(max=codes.shape[1] - 1)
    return torch.where(t < lt, torch.gather(codes, 1, idx), torch.zeros_like(idx))


def _check_given_prosody(prosody_codes, prosody_lengths, plm_sampling, plm_prefix, plm_causal, takes: int = 1) -> None:
    """``prosody_codes`` replaces the prosody LM: everything that steers the LM is refused next to it."""
    if prosody_codes is None:
        if prosody_lengths is not None:
            raise L.HspError("prosody_lengths without prosody_codes")
        return
    for name, given in (("plm_sampling", plm_sampling is not None), ("plm_prefix", plm_prefix is not None),
                        ("plm_causal", bool(plm_causal)), ("takes > 1", takes > 1)):
        if given:
            raise L.HspError(f"prosody_codes and {name} exclude each other: given codes skip the prosody LM")


@torch.no_grad()
def tts(models: TtsModels, text, text_length, tone, language, src_mel_ttv, src_mel_ttv_length, src_mel, src_length2,
        noise_scale_vc: float = 0.333, denoise_ratio: float = 0.0, output_sr: int = 16000, dur=None, noise=None,
        return_float: bool = False, gain: float = 0.999, plm_sampling=None, seeds=None, scale_norm: str = "max",
        target_lufs: float = -23.0, plm_causal: bool = False, plm_prefix=None, return_codes: bool = False,
        prosody_codes=None, prosody_lengths=None, limiter: bool = False, ceiling_db: float = -1.0,
        lookahead_ms: float = 1.5, limiter_passes: int = 2, return_stats: bool = False):
    """inference_plm.py:tts :156-190 on tensors.  ``plm_sampling`` (a ttv_v1.t2w2v_transformer.PlmSampling) and
    ``seeds`` make the prosody LM sample its codes (``Megatts2PLM1.infer``); None: greedy, as the reference.
    ``plm_causal``: the prosody LM decodes under the causal mask it is trained with, through a K/V cache
    (``infer(causal=True)``: other codes than the reference's bidirectional loop gives); False: the reference's loop.
    ``plm_prefix`` (int64 [B, P], needs ``plm_causal``): the first P prosody codes of every row are given and only the
    rest is decoded (``infer(prefix_codes=)``) -- durations do not depend on the codes, so the kept beginning of an
    earlier take of the same text and prompt fits frame for frame.  ``return_codes``: the PLM codes int64 [B, T] are
    appended to the result (the codes a later ``plm_prefix`` is cut from).
    ``prosody_codes`` (int64 [B, Ts], e.g. from `prosody_from_audio`; ``prosody_lengths`` [B] their frame counts, None:
    all Ts): the prosody LM is skipped and the given codes, fitted per row to that row's frame count
    (`fit_prosody_codes`), are used instead -- excludes ``plm_sampling``, ``plm_prefix`` and ``plm_causal``;
    ``return_codes`` then returns the fitted codes.
    ``scale_norm`` ... ``return_stats``: the int16 stage, see `output.OutputStage`; ``gain`` is the gain of 'max' /
    'prompt' (the caller's 0.999 or prompt peak).  The stats follow the audio, the codes come last.

    text / tone / language int64 [B, N], text_length [B]; src_mel_ttv [B, 80, Tm'] (prompt mel for the
    front-end) with lengths; src_mel [2B, 80, Tm] = the B prompt mels followed by the B denoised prompt
    mels (the reference's ``torch.cat([audio, denoised])`` at B = 1) with ``src_length2`` [2B].
    Returns int16 audio [B, n] (n = 320 * frames, x3 / x1.5 with SpeechSR), every row converted over its own length.
    B > 1 runs the utterances side by side; rows are independent up to the
    vocoder, whose convolutions see a shorter row's zero padding exactly as the reference's own batched
    ``infer`` does (equal-length batches are exact)."""
    stage = OutputStage(scale_norm, target_lufs, limiter, ceiling_db, lookahead_ms, limiter_passes,
                        return_stats).check()
    if plm_prefix is not None and not plm_causal:
        raise L.HspError("plm_prefix needs plm_causal=True: only the causal decoder can continue from given codes")
    _check_given_prosody(prosody_codes, prosody_lengths, plm_sampling, plm_prefix, plm_causal)
    wav, audio, stats, codes = _tts(models, text, text_length, tone, language, src_mel_ttv, src_mel_ttv_length, src_mel,
                                    src_length2, noise_scale_vc, denoise_ratio, output_sr, dur, noise, stage, gain,
                                    plm_sampling, seeds, plm_causal, plm_prefix, prosody_codes, prosody_lengths)
    return pack(wav, (audio, return_float), (stats, return_stats), (codes, return_codes))


def _tts(models, text, text_length, tone, language, src_mel_ttv, src_mel_ttv_length, src_mel, src_length2,
         noise_scale_vc, denoise_ratio, output_sr, dur, noise, stage: OutputStage, gain, plm_sampling, seeds,
         plm_causal, plm_prefix, prosody_codes, prosody_lengths):
    """`tts` behind its argument checks -> (wav, audio, stats or None, codes)."""
    B = text.shape[0]
    x_frame, g, x_lengths, x_mask = models.ttv.inf_extract_tc_latent(text, text_length, src_mel_ttv, src_mel_ttv_length,
                                                                     tone, language, dur=dur)
    if prosody_codes is None:
        codes = models.plm.infer(x_frame, sampling=plm_sampling, seeds=seeds, causal=plm_causal,
                                 prefix_codes=plm_prefix)
    else:
        if prosody_codes.dim() != 2 or prosody_codes.shape[0] != B:
            raise L.HspError(f"prosody_codes must be int64 [B = {B}, Ts], got {tuple(prosody_codes.shape)}")
        src = prosody_codes.shape[1] if prosody_lengths is None else prosody_lengths
        codes = fit_prosody_codes(prosody_codes.to(x_frame.device), src, torch.ceil(x_lengths).to(torch.int64),
                                  width=x_frame.shape[2])
    return (*_tts_from_codes(models, x_frame, g, codes, x_lengths, x_mask, src_mel, src_length2, noise_scale_vc,
                             denoise_ratio, output_sr, noise, stage, gain), codes)


@torch.no_grad()
def tts_from_codes(models: TtsModels, x_frame, g, codes, x_lengths, x_mask, src_mel, src_length2,
                   noise_scale_vc: float = 0.333, denoise_ratio: float = 0.0, output_sr: int = 16000, noise=None,
                   return_float: bool = False, gain: float = 0.999, scale_norm: str = "max", target_lufs: float = -23.0,
                   limiter: bool = False, ceiling_db: float = -1.0, lookahead_ms: float = 1.5, limiter_passes: int = 2,
                   return_stats: bool = False):
    """`tts` from the prosody codes on (inference_plm.py:161-190): ``x_frame, g, x_lengths, x_mask`` as
    ``inf_extract_tc_latent`` returned them, ``codes`` int64 [B, T] from ``Megatts2PLM1.infer`` in either mode.
    ``scale_norm`` ... ``return_stats``: the int16 stage, see `output.OutputStage`; the stats dict is the last
    result."""
    stage = OutputStage(scale_norm, target_lufs, limiter, ceiling_db, lookahead_ms, limiter_passes,
                        return_stats).check()
    wav, audio, stats = _tts_from_codes(models, x_frame, g, codes, x_lengths, x_mask, src_mel, src_length2,
                                        noise_scale_vc, denoise_ratio, output_sr, noise, stage, gain)
    return pack(wav, (audio, return_float), (stats, return_stats))


def _tts_from_codes(models, x_frame, g, codes, x_lengths, x_mask, src_mel, src_length2, noise_scale_vc, denoise_ratio,
                    output_sr, noise, stage: OutputStage, gain):
    """`tts_from_codes` behind its argument check -> (wav, audio, stats or None)."""
    B = x_frame.shape[0]
    w2v_x, pitch = models.ttv.inf_plm_gen(x_frame, g, codes.unsqueeze(1) if B == 1 else codes, x_lengths, x_mask)
    pitch = zero_below(pitch, math.log(55.0))                                  # :166 pitch clipping
    T2 = w2v_x.shape[2]
    if B == 1:
        src_length = torch.full((1,), T2, dtype=torch.int64, device=w2v_x.device)   # :163 the whole padded length
        audio = models.voc.voice_conversion_noise_control(w2v_x, src_length, src_mel, src_length2, pitch,
                                                          noise_scale=noise_scale_vc, denoise_ratio=denoise_ratio,
                                                          noise=noise)
        n_valid = None
    else:
        frames = torch.ceil(x_lengths).to(torch.int64)
        audio = models.voc.voice_conversion_noise_control(w2v_x, frames, src_mel, src_length2, pitch.unsqueeze(1),
                                                          noise_scale=noise_scale_vc, denoise_ratio=denoise_ratio,
                                                          noise=noise)
        n_valid = frames * 320
    if output_sr in (24000, 48000):
        audio = models.sr(audio)
        if n_valid is not None:
            n_valid = n_valid * output_sr // 16000
    wav, stats = stage.int16(audio, n_valid, output_rate(output_sr), gain)
    return wav, audio, stats


@torch.no_grad()
def tts_from_prompt(models: TtsModels, mel_fn, text, tone, language, prompt_audio, output_path=None,
                    noise_scale_vc: float = 0.333, output_sr: int = 16000, dur=None, noise=None,
                    denoise_ratio: float = 0.0, denoiser=None, hps_denoiser=None, prompt_sr: int = 16000,
                    scale_norm: str = "max", return_float: bool = False, plm_sampling=None, seed: int = 0,
                    takes: int = 1, target_lufs: float = -23.0, plm_causal: bool = False, plm_prefix=None,
                    return_codes: bool = False, prosody_codes=None, prosody_lengths=None, limiter: bool = False,
                    ceiling_db: float = -1.0, lookahead_ms: float = 1.5, limiter_passes: int = 2,
                    return_stats: bool = False):
    """inference_plm.py:tts :126-201 from the prompt WAVEFORM on: resampling to 16 kHz when ``prompt_sr`` differs
    (:124-126, kaiser window), prompt mels (:130-150, `prompt_mels`; with ``denoise_ratio`` > 0 the second prompt mel
    comes from the denoised prompt and the style vectors are mixed by voice_conversion_noise_control), text -> w2v /
    f0 -> waveform (`tts`), int16 (:185-188), optional 16-bit WAV (:195-200).
    text / tone / language int64 [1, N] on the GPU; prompt_audio fp32 [1, n] at ``prompt_sr`` on the GPU;
    ``mel_fn`` a finalized Mels_preprocess.MelSpectrogramFixed.  Returns int16 [n_out] (and the float audio with
    ``return_float``).

    ``plm_sampling`` (a ttv_v1.t2w2v_transformer.PlmSampling): the prosody LM samples its codes with seed ``seed``.
    ``plm_causal``: causal K/V-cached decoding of the prosody LM (see `tts`).
    ``takes`` = N > 1: one call synthesises N takes of the same text and prompt, take k with the PLM seed ``seed + k``
    (each take equals the solo call with that seed: the rows of a batch are independent and have one length, since the
    durations do not depend on the codes); returns int16 [N, n_out] and writes ``<stem>_take<k><ext>``.  An explicit
    ``noise`` with one row is used by every take; None: every take draws its own.
    ``plm_prefix`` (int64 [P] or [1, P], needs ``plm_causal``): the first P prosody codes are given (see `tts`); with
    ``takes`` = N the one prefix is shared by all N takes: N different endings of one beginning.  ``return_codes``
    appends the PLM codes (int64 [T], or [N, T] with takes) to the result.
    ``prosody_codes`` (int64 [Ts] or [1, Ts]; ``prosody_lengths`` their frame count, None: Ts): given prosody codes
    instead of the prosody LM (see `tts`); excludes ``plm_sampling``, ``plm_prefix``, ``plm_causal`` and ``takes`` > 1.
    ``scale_norm`` ... ``return_stats``: the int16 stage, see `output.OutputStage`, every take converted over its own
    length (stats: fp32 [takes] tensors)."""
    stage = OutputStage(scale_norm, target_lufs, limiter, ceiling_db, lookahead_ms, limiter_passes,
                        return_stats).check()
    takes = int(takes)
    if takes < 1:
        raise L.HspError(f"takes must be >= 1, got {takes}")
    _check_given_prosody(prosody_codes, prosody_lengths, plm_sampling, plm_prefix, plm_causal, takes)
    if prosody_codes is not None:
        prosody_codes = prosody_codes.reshape(1, -1)
    if takes > 1 and plm_sampling is None:
        raise L.HspError("takes > 1 needs plm_sampling: greedy decoding gives the same take every time")
    if plm_prefix is not None:
        if not plm_causal:
            raise L.HspError("plm_prefix needs plm_causal=True: only the causal decoder can continue from given codes")
        if not isinstance(plm_prefix, torch.Tensor) or plm_prefix.dim() not in (1, 2) or \
                (plm_prefix.dim() == 2 and plm_prefix.shape[0] != 1):
            raise L.HspError("plm_prefix must be an int64 [P] or [1, P] tensor: one prefix, shared by every take")
        plm_prefix = plm_prefix.reshape(1, -1).expand(takes, -1).contiguous()
    if denoise_ratio != 0 and denoiser is None:
        raise L.HspError("denoise_ratio > 0 needs the denoiser model (denoiser.generator.MPNet), as "
                         "inference_plm.py:144-147")
    if int(prompt_sr) != 16000:
        prompt_audio = Fh.resample(prompt_audio, prompt_sr, 16000, resampling_method="kaiser_window")
    gain = stage.gain(prompt_audio)
    src_mel_ttv, src_mel = prompt_mels(mel_fn, prompt_audio, denoiser if denoise_ratio != 0 else None, hps_denoiser)
    dev = prompt_audio.device
    assert text.shape[0] == 1 and prompt_audio.shape[0] == 1, "the reference harness synthesises one utterance per call"
    B = takes
    if B > 1:
        rep = lambda x: None if x is None else x.expand(B, *x.shape[1:]).contiguous()  # noqa: E731
        text, tone, language, src_mel_ttv, dur = rep(text), rep(tone), rep(language), rep(src_mel_ttv), rep(dur)
        src_mel = torch.cat([rep(src_mel[:1]), rep(src_mel[1:2])])     # the B prompt mels, then the B second mels
        if noise is not None and noise.shape[0] == 1:
            noise = rep(noise)
    text_length = torch.full((B,), text.shape[1], dtype=torch.int64, device=dev)
    ttv_len = torch.full((B,), src_mel_ttv.shape[2], dtype=torch.int64, device=dev)
    src_length2 = torch.full((2 * B,), src_mel.shape[2], dtype=torch.int64, device=dev)
    seeds = int(seed) if plm_sampling is not None else None
    wav, audio, stats, codes = _tts(models, text, text_length, tone, language, src_mel_ttv, ttv_len, src_mel,
                                    src_length2, noise_scale_vc, float(denoise_ratio), output_sr, dur, noise, stage,
                                    gain, plm_sampling, seeds, plm_causal, plm_prefix, prosody_codes, prosody_lengths)
    if B == 1:
        wav, codes = wav[0], codes[0]
        if output_path is not None:
            write_wav(output_path, output_rate(output_sr), wav)
    elif output_path is not None:
        import os
        stem, ext = os.path.splitext(str(output_path))
        for k in range(B):
            write_wav(f"{stem}_take{k}{ext}", output_rate(output_sr), wav[k])
    return pack(wav, (audio, return_float), (stats, return_stats), (codes, return_codes))


def tts_from_prompt_file(models: TtsModels, mel_fn, text, tone, language, prompt_path, output_path=None,
                         plm_sampling=None, seed: int = 0, takes: int = 1, plm_causal: bool = False, plm_prefix=None,
                         return_codes: bool = False, prosody_codes=None, prosody_lengths=None, **kwargs):
    """inference_plm.py:120-201 from the prompt FILE on: ``audio.load`` (torchaudio.load), channel 0 to the GPU of
    ``text``, then `tts_from_prompt` at the file's rate (resampled to 16 kHz there).  ``plm_sampling`` / ``seed`` /
    ``takes`` / ``plm_causal`` / ``plm_prefix`` / ``return_codes`` / ``prosody_codes`` / ``prosody_lengths`` and
    ``kwargs`` (the fields of `output.OutputStage`, ...) go to `tts_from_prompt`."""
    from . import audio as A
    OutputStage.of(kwargs).check()      # before the file is read
    prompt, rate = A.load(prompt_path)
    return tts_from_prompt(models, mel_fn, text, tone, language, prompt[:1].to(text.device), output_path=output_path,
                           prompt_sr=rate, plm_sampling=plm_sampling, seed=seed, takes=takes, plm_causal=plm_causal,
                           plm_prefix=plm_prefix, return_codes=return_codes, prosody_codes=prosody_codes,
                           prosody_lengths=prosody_lengths, **kwargs)
