"""HIP mirror of the tensor core of the reference's inference_plm.py (its ``tts()`` between mel
extraction and wav writing, :156-190, and the model bundle of ``model_load`` :203-263).

The prompt file ingest (:120-126: ``torchaudio.load``, first channel, kaiser-window resampling to 16 kHz) is
``audio.load`` + ``functional.resample`` (``tts_from_prompt_file``; ``tts_from_prompt(prompt_sr=...)``), and
``scale_norm='prompt'`` (:127-128,185-186) is ``tts_from_prompt(scale_norm="prompt")``; the int16 stage of every
harness here is one `output.OutputStage`.  Out of scope here (host plumbing, not the hot path): text cleaning /
phonemisation (``get_text``) -- callers hand over phone ids.  The prompt mel transform is
``Mels_preprocess.MelSpectrogramFixed``, the optional prompt denoiser ``denoiser.generator.MPNet`` +
``denoiser.infer.denoise`` (:142-147).

``tts_batch`` / ``tts_lines`` / ``tts_batch_files`` speak many different lines in ragged batches (the reference speaks
one line per call); row b of a batch is held to ``tts_from_prompt`` on line b alone."""
from __future__ import annotations

import math
from typing import Optional

import torch
from torch import nn

from . import _lib as L
from . import functional as Fh
from . import hip_layers
from . import prosody_controls as PC
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
        lookahead_ms: float = 1.5, limiter_passes: int = 2, return_stats: bool = False, row_exact: bool = False,
        style=None, noise_seeds=None, pitch=None, lf0=None, return_lf0: bool = False, length_scale=1.0,
        phone_scale=None):
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
    ``infer`` does (equal-length batches are exact).  ``row_exact`` (B > 1): the vocoder and SpeechSR run every row as
    at B = 1 too, so row b of a ragged batch equals the call on row b alone; `row_exact_refusal`
    applies.  ``style`` [B, 256, 1]: the vocoder's style vectors, precomputed per prompt at the prompt's own length
    (``voc.style_vector``); ``src_mel`` / ``src_length2`` are not read then.  ``gain`` may be a device fp32 [B] tensor.
    ``noise_seeds`` (an int s: row b draws with s + b; or an int64 [B] tensor; excludes ``noise``): the vocoder's prior
    noise is the seeded stream of include/hsp.h "seeded prior noise", so the waveform is a function of (weights, inputs,
    seeds) alone; None: ``noise``, or a draw from torch's process-wide generator.
    Prosody controls (all off by default, and then no launch is added):
    ``pitch`` (a `prosody_controls.PitchEdit`): the log-F0 track the vocoder is given -- the pitch predictor's, clipped
    below 55 Hz (:166) -- is edited over every row's own 4 * frames (one launch; None or an identity edit: none).
    ``lf0`` (fp32 [B, 4 * T2]): replaces the predicted track; durations do not depend on codes or pitch, so a track
    read from an earlier take of the same text, prompt and scales fits frame for frame; ``pitch`` then edits it.
    ``return_lf0``: the track the vocoder was given, fp32 [B, 4 * T2], is the last result, after the codes.
    ``length_scale`` (a float or a [B] sequence) and ``phone_scale`` (a list of B rows of text_length[b] factors, or
    None; reads ``text_length`` back): the pace of a row and of its phones, each in [0.25, 4]
    (`prosody_controls.check_scales`); given durations ``dur`` are scaled by ``phone_scale`` alone."""
    stage = OutputStage(scale_norm, target_lufs, limiter, ceiling_db, lookahead_ms, limiter_passes,
                        return_stats).check()
    Fh.check_noise_seeds(noise, noise_seeds, None if noise_seeds is None else text.shape[0])
    if plm_prefix is not None and not plm_causal:
        raise L.HspError("plm_prefix needs plm_causal=True: only the causal decoder can continue from given codes")
    _check_given_prosody(prosody_codes, prosody_lengths, plm_sampling, plm_prefix, plm_causal)
    pitch = PC.check_pitch(pitch, text.shape[0])
    length_scale, scale = PC.check_scales(
        length_scale, phone_scale, [text.shape[1]] * text.shape[0] if phone_scale is None else text_length.tolist(),
        dur is not None)
    wav, audio, stats, codes, track = _tts(models, text, text_length, tone, language, src_mel_ttv, src_mel_ttv_length,
                                           src_mel, src_length2, noise_scale_vc, denoise_ratio, output_sr, dur, noise,
                                           stage, gain, plm_sampling, seeds, plm_causal, plm_prefix, prosody_codes,
                                           prosody_lengths, row_exact, style, noise_seeds, pitch, lf0, length_scale,
                                           scale)
    return pack(wav, (audio, return_float), (stats, return_stats), (codes, return_codes), (track, return_lf0))


def _front(models, text, text_length, src_mel_ttv, src_mel_ttv_length, tone, language, dur, length_scale, scale, **kw):
    """``inf_extract_tc_latent`` as the harnesses call it: without pace controls (``length_scale`` 1.0 and no ``scale``,
    the float32 [B, N] numpy array of `prosody_controls.check_scales`) the call there has always been."""
    if scale is not None:
        width = text.shape[1]
        if scale.shape[1] < width:      # a padded batch wider than its longest line
            import numpy as np
            scale = np.pad(scale, ((0, 0), (0, width - scale.shape[1])), constant_values=1.0)
        kw["phone_scale"] = torch.from_numpy(scale[:, :width].copy()).to(text.device)
    if length_scale != 1.0:
        kw["length_scale"] = length_scale
    return models.ttv.inf_extract_tc_latent(text, text_length, src_mel_ttv, src_mel_ttv_length, tone, language, dur=dur,
                                            **kw)


def _tts(models, text, text_length, tone, language, src_mel_ttv, src_mel_ttv_length, src_mel, src_length2,
         noise_scale_vc, denoise_ratio, output_sr, dur, noise, stage: OutputStage, gain, plm_sampling, seeds,
         plm_causal, plm_prefix, prosody_codes, prosody_lengths, row_exact=False, style=None, noise_seeds=None,
         pitch=None, lf0=None, length_scale=1.0, scale=None):
    """`tts` behind its argument checks -> (wav, audio, stats or None, codes, the vocoder's log-F0 track)."""
    B = text.shape[0]
    x_frame, g, x_lengths, x_mask = _front(models, text, text_length, src_mel_ttv, src_mel_ttv_length, tone, language,
                                           dur, length_scale, scale)
    if prosody_codes is None:
        codes = models.plm.infer(x_frame, sampling=plm_sampling, seeds=seeds, causal=plm_causal,
                                 prefix_codes=plm_prefix)
    else:
        if prosody_codes.dim() != 2 or prosody_codes.shape[0] != B:
            raise L.HspError(f"prosody_codes must be int64 [B = {B}, Ts], got {tuple(prosody_codes.shape)}")
        src = prosody_codes.shape[1] if prosody_lengths is None else prosody_lengths
        codes = fit_prosody_codes(prosody_codes.to(x_frame.device), src, torch.ceil(x_lengths).to(torch.int64),
                                  width=x_frame.shape[2])
    wav, audio, stats, track = _tts_from_codes(models, x_frame, g, codes, x_lengths, x_mask, src_mel, src_length2,
                                               noise_scale_vc, denoise_ratio, output_sr, noise, stage, gain, row_exact,
                                               style, noise_seeds, pitch, lf0)
    return wav, audio, stats, codes, track


@torch.no_grad()
def tts_from_codes(models: TtsModels, x_frame, g, codes, x_lengths, x_mask, src_mel, src_length2,
                   noise_scale_vc: float = 0.333, denoise_ratio: float = 0.0, output_sr: int = 16000, noise=None,
                   return_float: bool = False, gain: float = 0.999, scale_norm: str = "max", target_lufs: float = -23.0,
                   limiter: bool = False, ceiling_db: float = -1.0, lookahead_ms: float = 1.5, limiter_passes: int = 2,
                   return_stats: bool = False, row_exact: bool = False, style=None, noise_seeds=None, pitch=None,
                   lf0=None, return_lf0: bool = False):
    """`tts` from the prosody codes on (inference_plm.py:161-190): ``x_frame, g, x_lengths, x_mask`` as
    ``inf_extract_tc_latent`` returned them, ``codes`` int64 [B, T] from ``Megatts2PLM1.infer`` in either mode.
    ``scale_norm`` ... ``return_stats``: the int16 stage, see `output.OutputStage`; the stats dict is the last
    result.  ``row_exact`` / ``style`` / ``noise_seeds`` / ``pitch`` / ``lf0`` / ``return_lf0`` (the track comes
    last): as for `tts`."""
    stage = OutputStage(scale_norm, target_lufs, limiter, ceiling_db, lookahead_ms, limiter_passes,
                        return_stats).check()
    pitch = PC.check_pitch(pitch, x_frame.shape[0])
    Fh.check_noise_seeds(noise, noise_seeds, None if noise_seeds is None else x_frame.shape[0])
    wav, audio, stats, track = _tts_from_codes(models, x_frame, g, codes, x_lengths, x_mask, src_mel, src_length2,
                                               noise_scale_vc, denoise_ratio, output_sr, noise, stage, gain, row_exact,
                                               style, noise_seeds, pitch, lf0)
    return pack(wav, (audio, return_float), (stats, return_stats), (track, return_lf0))


def _tts_from_codes(models, x_frame, g, codes, x_lengths, x_mask, src_mel, src_length2, noise_scale_vc, denoise_ratio,
                    output_sr, noise, stage: OutputStage, gain, row_exact=False, style=None, noise_seeds=None,
                    edit=None, lf0=None):
    """`tts_from_codes` behind its argument check -> (wav, audio, stats or None, the vocoder's log-F0 track [B, 4 T2]).
    ``edit``: a checked `PitchEdit` that is no identity, or None; ``lf0``: a given track instead of the predicted one."""
    B, T2 = x_frame.shape[0], x_frame.shape[2]
    if lf0 is not None:
        lf0 = PC.check_lf0(lf0, B, T2)                                         # before any launch
    w2v_x, pitch = models.ttv.inf_plm_gen(x_frame, g, codes.unsqueeze(1) if B == 1 else codes, x_lengths, x_mask)
    pitch = zero_below(pitch, math.log(55.0))                                  # :166 pitch clipping
    frames = None if B == 1 else torch.ceil(x_lengths).to(torch.int64)
    if lf0 is not None:             # a given track, held to zero past every row's own frames as the predicted one is
        pitch = lf0.to(pitch.device) if B == 1 else \
            Fh.mask_mul(lf0.to(pitch.device).unsqueeze(1), Fh.sequence_mask(4 * frames, 4 * T2)).squeeze(1)
    if edit is not None:
        pitch = edit.apply(pitch, None if B == 1 else 4 * frames)
    if B == 1:
        src_length = torch.full((1,), T2, dtype=torch.int64, device=w2v_x.device)   # :163 the whole padded length
        audio = models.voc.voice_conversion_noise_control(w2v_x, src_length, src_mel, src_length2, pitch,
                                                          noise_scale=noise_scale_vc, denoise_ratio=denoise_ratio,
                                                          noise=noise, style=style, noise_seeds=noise_seeds)
        n_valid = None
    else:
        audio = models.voc.voice_conversion_noise_control(w2v_x, frames, src_mel, src_length2, pitch.unsqueeze(1),
                                                          noise_scale=noise_scale_vc, denoise_ratio=denoise_ratio,
                                                          noise=noise, style=style, row_exact=row_exact,
                                                          noise_seeds=noise_seeds)
        n_valid = frames * 320
    if output_sr in (24000, 48000):
        if row_exact and B > 1:        # SpeechSR on the ragged rows, each as on its own (as inference_vc.vc_batch)
            with hip_layers.row_exact(hip_layers.RowLengths(frames, audio.shape[2] // 320)):
                audio = models.sr(audio)
        else:
            audio = models.sr(audio)
        if n_valid is not None:
            n_valid = n_valid * output_sr // 16000
    if stage is None:                  # `tts_lines(join=True)`: the programme is converted, not its lines
        return None, audio, None, pitch
    wav, stats = stage.int16(audio, n_valid, output_rate(output_sr), gain)
    return wav, audio, stats, pitch


@torch.no_grad()
def tts_from_prompt(models: TtsModels, mel_fn, text, tone, language, prompt_audio, output_path=None,
                    noise_scale_vc: float = 0.333, output_sr: int = 16000, dur=None, noise=None,
                    denoise_ratio: float = 0.0, denoiser=None, hps_denoiser=None, prompt_sr: int = 16000,
                    scale_norm: str = "max", return_float: bool = False, plm_sampling=None, seed: int = 0,
                    takes: int = 1, target_lufs: float = -23.0, plm_causal: bool = False, plm_prefix=None,
                    return_codes: bool = False, prosody_codes=None, prosody_lengths=None, limiter: bool = False,
                    ceiling_db: float = -1.0, lookahead_ms: float = 1.5, limiter_passes: int = 2,
                    return_stats: bool = False, noise_seed: Optional[int] = None, pitch=None, lf0=None,
                    return_lf0: bool = False, length_scale=1.0, phone_scale=None):
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
    ``noise_seed`` (an int; excludes ``noise``): the vocoder's prior noise is the seeded stream of that seed (`tts`),
    take k drawing with ``noise_seed + k`` -- so with ``seed`` and ``noise_seed`` a take is reproducible down to the
    waveform, and take k equals the solo call with ``seed + k`` and ``noise_seed + k``.  None: drawn from torch's
    process-wide generator, another waveform on every call.
    ``plm_prefix`` (int64 [P] or [1, P], needs ``plm_causal``): the first P prosody codes are given (see `tts`); with
    ``takes`` = N the one prefix is shared by all N takes: N different endings of one beginning.  ``return_codes``
    appends the PLM codes (int64 [T], or [N, T] with takes) to the result.
    ``prosody_codes`` (int64 [Ts] or [1, Ts]; ``prosody_lengths`` their frame count, None: Ts): given prosody codes
    instead of the prosody LM (see `tts`); excludes ``plm_sampling``, ``plm_prefix``, ``plm_causal`` and ``takes`` > 1.
    ``scale_norm`` ... ``return_stats``: the int16 stage, see `output.OutputStage`, every take converted over its own
    length (stats: fp32 [takes] tensors).
    ``pitch`` / ``lf0`` / ``return_lf0`` / ``length_scale`` / ``phone_scale``: the prosody controls of `tts`.
    ``pitch`` holds one value per take or one for all; ``lf0`` (fp32 [4 * T2] or [1, 4 * T2]) is shared by the takes;
    ``length_scale`` is one float and ``phone_scale`` one row of N factors (or a list holding it): the takes of a call
    have one length.  ``return_lf0`` appends the vocoder's track, fp32 [4 * T2] ([N, 4 * T2] with takes), last."""
    stage = OutputStage(scale_norm, target_lufs, limiter, ceiling_db, lookahead_ms, limiter_passes,
                        return_stats).check()
    takes = int(takes)
    if takes < 1:
        raise L.HspError(f"takes must be >= 1, got {takes}")
    if isinstance(noise_seed, torch.Tensor):
        raise L.HspError("noise_seed is one int (take k draws with noise_seed + k)")
    Fh.check_noise_seeds(noise, noise_seed, what="noise_seed")
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
    pitch = PC.check_pitch(pitch, takes)
    if phone_scale is not None and not (isinstance(phone_scale, (list, tuple)) and len(phone_scale) == 1
                                        and not isinstance(phone_scale[0], (int, float))):
        phone_scale = [phone_scale]
    if not isinstance(length_scale, (int, float)):
        raise L.HspError("length_scale is one float here: the takes of a call have one length")
    length_scale, scale = PC.check_scales(length_scale, phone_scale, [text.shape[1]], dur is not None)
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
        if scale is not None:
            scale = scale.repeat(B, 0)
        if lf0 is not None:
            lf0 = lf0.reshape(1, -1).expand(B, -1)
    text_length = torch.full((B,), text.shape[1], dtype=torch.int64, device=dev)
    ttv_len = torch.full((B,), src_mel_ttv.shape[2], dtype=torch.int64, device=dev)
    src_length2 = torch.full((2 * B,), src_mel.shape[2], dtype=torch.int64, device=dev)
    seeds = int(seed) if plm_sampling is not None else None
    wav, audio, stats, codes, track = _tts(models, text, text_length, tone, language, src_mel_ttv, ttv_len, src_mel,
                                           src_length2, noise_scale_vc, float(denoise_ratio), output_sr, dur, noise,
                                           stage, gain, plm_sampling, seeds, plm_causal, plm_prefix, prosody_codes,
                                           prosody_lengths, noise_seeds=noise_seed, pitch=pitch, lf0=lf0,
                                           length_scale=length_scale, scale=scale)
    if B == 1:
        wav, codes, track = wav[0], codes[0], track[0]
        if output_path is not None:
            write_wav(output_path, output_rate(output_sr), wav)
    elif output_path is not None:
        import os
        stem, ext = os.path.splitext(str(output_path))
        for k in range(B):
            write_wav(f"{stem}_take{k}{ext}", output_rate(output_sr), wav[k])
    return pack(wav, (audio, return_float), (stats, return_stats), (codes, return_codes), (track, return_lf0))


def tts_from_prompt_file(models: TtsModels, mel_fn, text, tone, language, prompt_path, output_path=None,
                         plm_sampling=None, seed: int = 0, takes: int = 1, plm_causal: bool = False, plm_prefix=None,
                         return_codes: bool = False, prosody_codes=None, prosody_lengths=None, pitch=None, lf0=None,
                         return_lf0: bool = False, length_scale=1.0, phone_scale=None, **kwargs):
    """inference_plm.py:120-201 from the prompt FILE on: ``audio.load`` (torchaudio.load), channel 0 to the GPU of
    ``text``, then `tts_from_prompt` at the file's rate (resampled to 16 kHz there).  ``plm_sampling`` / ``seed`` /
    ``takes`` / ``plm_causal`` / ``plm_prefix`` / ``return_codes`` / ``prosody_codes`` / ``prosody_lengths`` and
    ``pitch`` / ``lf0`` / ``return_lf0`` / ``length_scale`` / ``phone_scale`` and
    ``kwargs`` (the fields of `output.OutputStage`, ``noise`` / ``noise_seed``, ...) go to `tts_from_prompt`."""
    from . import audio as A
    OutputStage.of(kwargs).check()      # before the file is read
    PC.check_pitch(pitch, int(takes))
    Fh.check_noise_seeds(kwargs.get("noise"), kwargs.get("noise_seed"), what="noise_seed")
    prompt, rate = A.load(prompt_path)
    return tts_from_prompt(models, mel_fn, text, tone, language, prompt[:1].to(text.device), output_path=output_path,
                           prompt_sr=rate, plm_sampling=plm_sampling, seed=seed, takes=takes, plm_causal=plm_causal,
                           plm_prefix=plm_prefix, return_codes=return_codes, prosody_codes=prosody_codes,
                           prosody_lengths=prosody_lengths, pitch=pitch, lf0=lf0, return_lf0=return_lf0,
                           length_scale=length_scale, phone_scale=phone_scale, **kwargs)


# ---------------------------------------------------------------- a page of lines: ragged batches
MAX_PHONES = 438    # phones per line: the Gaussian upsampler's bound

STAGE_HOOK = None   # measurement hook (tools/tts_ragged_bench.py): STAGE_HOOK(name) at the start of every tts_batch stage


def _stage(name):
    if STAGE_HOOK is not None:
        STAGE_HOOK(name)


def line_chunks(phone_counts, max_batch: int):
    """The batches of `tts_lines`, from the phone counts alone: the lines sorted by phone count (a stable sort: equal
    counts keep the caller's order) and cut into chunks of at most ``max_batch`` -> a list of index lists.  Every index
    appears once; `chunk_order` of the result restores the caller's order."""
    if int(max_batch) < 1:
        raise L.HspError(f"max_batch must be >= 1, got {max_batch}")
    order = sorted(range(len(phone_counts)), key=lambda i: int(phone_counts[i]))
    return [order[i:i + int(max_batch)] for i in range(0, len(order), int(max_batch))]


def chunk_order(chunks):
    """The inverse permutation of `line_chunks`: ``inv[k]`` is the place of the caller's line k among the chunks' rows
    taken in order, so ``[flat[i] for i in inv]`` is in the caller's order."""
    flat = [k for rows in chunks for k in rows]
    inv = [0] * len(flat)
    for place, k in enumerate(flat):
        inv[k] = place
    return inv


def join_plan(lengths, rate: int, pause_ms: float):
    """Where the lines of a programme start: ``lengths`` output samples per line at ``rate``, ``round(pause_ms * rate /
    1000)`` zero samples between consecutive lines -> (offsets, total samples)."""
    if not pause_ms >= 0:
        raise L.HspError(f"pause_ms must be >= 0, got {pause_ms}")
    pause = round(float(pause_ms) * int(rate) / 1000)
    offsets, pos = [], 0
    for n in lengths:
        offsets.append(pos)
        pos += int(n) + pause
    return offsets, (pos - pause if offsets else 0)


def _row(x):
    return x.reshape(-1)


def _per_line(arg, B: int, what: str):
    """A per-line keyword: None, or a list of B entries."""
    if arg is None:
        return None
    if not isinstance(arg, (list, tuple)) or len(arg) != B:
        got = len(arg) if isinstance(arg, (list, tuple)) else type(arg).__name__
        raise L.HspError(f"{what} must be a list of one entry per line ({B}), got {got}")
    return list(arg)


def check_lines(lines, prompts, dur=None, plm_sampling=None, plm_causal=False, plm_prefixes=None, prosody_codes=None,
                prosody_lengths=None, denoised=None):
    """The argument checks of `tts_batch` / `tts_lines`, from shapes alone (no device work): B triples (ids, tone,
    language) of one length each in [1, MAX_PHONES], one prompt or B, per-line keywords as lists of B, ``plm_prefixes``
    only with ``plm_causal``, ``prosody_codes`` with nothing that steers the prosody LM.  -> the phone counts."""
    if not isinstance(lines, (list, tuple)) or not lines:
        raise L.HspError("lines must be a non-empty list of (ids, tone, language) triples")
    B, counts = len(lines), []
    for b, line in enumerate(lines):
        if not isinstance(line, (list, tuple)) or len(line) != 3:
            raise L.HspError(f"line {b} must be a triple (ids, tone, language)")
        for x in line:
            if not isinstance(x, torch.Tensor) or x.dtype != torch.int64 or x.dim() not in (1, 2) or \
                    (x.dim() == 2 and x.shape[0] != 1):
                raise L.HspError(f"line {b}: ids / tone / language must be int64 [N] or [1, N] tensors")
        n = [x.shape[-1] for x in line]
        if n[0] == 0:
            raise L.HspError(f"line {b} is empty: a line needs at least one phone")
        if n[1] != n[0] or n[2] != n[0]:
            raise L.HspError(f"line {b}: ids, tone and language have different lengths {tuple(n)}")
        if n[0] > MAX_PHONES:
            raise L.HspError(f"line {b} has {n[0]} phones; the Gaussian upsampler takes {MAX_PHONES} at the most")
        counts.append(n[0])
    if isinstance(prompts, (list, tuple)) and len(prompts) not in (1, B):
        raise L.HspError(f"give one prompt or one per line ({B}), got {len(prompts)}")
    if isinstance(denoised, (list, tuple)) and len(denoised) not in (1, B):
        raise L.HspError(f"give one denoised prompt or one per line ({B}), got {len(denoised)}")
    dur = _per_line(dur, B, "dur")
    if dur is not None:
        for b, d in enumerate(dur):
            if d.numel() != counts[b]:
                raise L.HspError(f"line {b}: {d.numel()} durations for {counts[b]} phones")
    plm_prefixes = _per_line(plm_prefixes, B, "plm_prefixes")
    if plm_prefixes is not None and not plm_causal:
        raise L.HspError("plm_prefixes needs plm_causal=True: only the causal decoder can continue from given codes")
    prosody_codes = _per_line(prosody_codes, B, "prosody_codes")
    lengths = _per_line(prosody_lengths, B, "prosody_lengths")
    _check_given_prosody(prosody_codes, lengths, plm_sampling, plm_prefixes, plm_causal)
    return counts


def _check_denoiser(denoise_ratio, denoised, denoiser, hps_denoiser, who: str) -> None:
    """`inference_vc.vc_batch`'s rules for the second prompt mel."""
    if denoised is not None and denoiser is not None:
        raise L.HspError(f"{who}: give the denoised prompts or a denoiser, not both")
    if denoise_ratio != 0 and denoised is None and denoiser is None:
        raise L.HspError(f"{who}: denoise_ratio != 0 needs the denoised prompts (denoised=) or a denoiser "
                         "(denoiser=, hps_denoiser=)")
    if denoiser is not None and hps_denoiser is None:
        raise L.HspError(f"{who}: a denoiser needs its config (hps_denoiser=)")


def _pad_rows(rows, width: int, dtype, device):
    """Zero-padded [len(rows), width] copy of 1-D (or [1, n]) rows."""
    out = torch.zeros(len(rows), width, dtype=dtype, device=device)
    for b, r in enumerate(rows):
        r = _row(r)
        out[b, :r.shape[0]].copy_(r)
    return out


def _encode_prompts(models, mel_fn, prompts, B, prompt_sr, denoise_ratio, denoised, denoiser, hps_denoiser):
    """Every distinct prompt of B lines (`group_prompts`) encoded once and exactly as `tts_from_prompt` encodes it
    (`prompt_mels`): -> (per distinct prompt its ``(src_mel_ttv [1, 80, Tm'], style [1, 256, 1], the 16 kHz waveform
    [1, n])``, line -> index).  With a denoiser all distinct prompts are denoised in one packed pass."""
    from .inference_vc import denoise_prompts, group_prompts
    distinct, index = group_prompts(prompts, B)
    P = len(distinct)
    first = [index.index(p) for p in range(P)]
    dev = distinct[0].device
    rows = []
    for p, a in enumerate(distinct):
        a = _row(a).to(torch.float32).reshape(1, -1)
        if int(prompt_sr) != 16000:
            a = Fh.resample(a, prompt_sr, 16000, resampling_method="kaiser_window")
        if a.shape[-1] <= 640:
            raise L.HspError(f"prompt {p} has {a.shape[-1]} samples at 16 kHz; the mel transform needs more than 640")
        rows.append(a.contiguous())
    seconds = [None] * P
    if denoise_ratio != 0 and denoiser is not None:
        seconds = denoise_prompts(rows, denoiser, hps_denoiser)          # one packed pass over the distinct prompts
    elif denoise_ratio != 0 and denoised is not None:
        given = denoised if isinstance(denoised, (list, tuple)) else [denoised]
        if len(given) == 1 and P != 1:
            raise L.HspError(f"{P} distinct prompts need denoised as a list of one entry per line")
        seconds = [given[first[p]] if len(given) == B and B > 1 else given[0] for p in range(P)]
    encoded = []
    for p, a in enumerate(rows):
        n = a.shape[-1]
        if seconds[p] is None:
            mel_ttv, mel = prompt_mels(mel_fn, a)
        else:
            s = _row(seconds[p])
            if s.shape[0] < n:
                raise L.HspError(f"denoised prompt {p} is shorter than its prompt")
            padded = torch.zeros(1, (n // 1600 + 1) * 1600, dtype=torch.float32, device=dev)
            padded[:, :n].copy_(a)
            mel_ttv = mel_fn(padded)
            mel = mel_fn(torch.cat([a, s[:n].reshape(1, -1).to(torch.float32)], 0).contiguous())
        style = models.voc.style_vector(mel, torch.full((2,), mel.shape[2], dtype=torch.int64, device=dev),
                                        denoise_ratio)
        encoded.append((mel_ttv, style, a))
    return encoded, index


def _prompt_rows(encoded, index, want_peaks):
    """The rows of a batch from its lines' encoded prompts (``index``: line -> entry of ``encoded``): -> (src_mel_ttv
    [B, 80, Tm'] zero-padded, its lengths int64 [B], style [B, 256, 1], prompt peaks fp32 [B] or None)."""
    from .inference_vc import _device_lengths, _stack
    B, dev = len(index), encoded[0][0].device
    widths = [encoded[i][0].shape[2] for i in index]
    src_mel_ttv = torch.zeros(B, 80, max(widths), dtype=torch.float32, device=dev)
    for b, i in enumerate(index):
        src_mel_ttv[b, :, :widths[b]].copy_(encoded[i][0][0])
    style = torch.cat([encoded[i][1] for i in index])
    peaks = None
    if want_peaks:                     # the peak of each row's own prompt, taken on the device
        pm, lens = _stack([encoded[i][2] for i in index], dev)
        peaks = Fh.abs_max_rows(pm, _device_lengths(lens, dev))
    return src_mel_ttv, _device_lengths(widths, dev), style, peaks


def _plm_codes(models, x_frame, frames, plm_sampling, seeds, plm_causal, plm_prefixes, prosody_codes, prosody_lengths):
    """The prosody codes int64 [B, T2] of a ragged batch (``frames``: host frame counts); entries from a row's frame
    count on are not meaningful."""
    B, _, T2 = x_frame.shape
    dev = x_frame.device
    if prosody_codes is not None:
        src = [_row(c).shape[0] for c in prosody_codes] if prosody_lengths is None else [int(n) for n in prosody_lengths]
        given = _pad_rows(prosody_codes, max(_row(c).shape[0] for c in prosody_codes), torch.int64, dev)
        return fit_prosody_codes(given, torch.tensor(src, dtype=torch.int64).to(dev),
                                 torch.tensor(frames, dtype=torch.int64).to(dev), width=T2)
    if plm_prefixes is None:
        return models.plm.infer(x_frame, sampling=plm_sampling, seeds=seeds, causal=plm_causal)
    given = [None if p is None else _row(p) for p in plm_prefixes]
    for b, p in enumerate(given):
        if p is not None and not 1 <= p.shape[0] < frames[b]:
            raise L.HspError(f"line {b}: a prefix needs 1 <= P < {frames[b]} codes (the line's frames), got "
                             f"{p.shape[0]}")
    if all(p is not None and p.shape[0] == given[0].shape[0] for p in given):
        return models.plm.infer(x_frame, sampling=plm_sampling, seeds=seeds, causal=True,
                                prefix_codes=torch.stack(given).to(dev))
    # prefixes of different lengths: every line at its own position, through one decode session
    rows = models.plm.infer_many([x_frame[b, :, :frames[b]] for b in range(B)], slots=B, sampling=plm_sampling,
                                 seeds=seeds, prefixes=given)
    return _pad_rows(rows, T2, torch.int64, dev)


def _tts_batch(models, mel_fn, lines, prompts, stage, *, dur=None, length_scale=1.0, noise=None, noise_scale_vc=0.333,
               denoise_ratio=0.0, denoised=None, denoiser=None, hps_denoiser=None, prompt_sr=16000, output_sr=16000,
               plm_sampling=None, seeds=0, plm_causal=False, plm_prefixes=None, prosody_codes=None,
               prosody_lengths=None, row_exact=True, int16=True, encoded=None, noise_seeds=None, pitch=None, lf0=None,
               phone_scale=None):
    """`tts_batch` behind the check of its output stage -> (wav or None, lengths int64 [B], audio, stats or None,
    codes (a list of B), the frame counts on the host, the vocoder's log-F0 rows (a list of B [4 T_b])).  ``int16`` False: the int16 stage is left to the caller.
    ``encoded``: what `_encode_prompts` made of the lines' prompts (`tts_lines` encodes a page's prompts once)."""
    counts = check_lines(lines, prompts, dur, plm_sampling, plm_causal, plm_prefixes, prosody_codes, prosody_lengths,
                         denoised)
    _check_denoiser(denoise_ratio, denoised, denoiser, hps_denoiser, "tts_batch")
    B, N = len(lines), max(counts)
    pitch = PC.check_pitch(pitch, B)
    length_scale, scale = PC.check_scales(length_scale, phone_scale, counts, dur is not None)
    if lf0 is not None and not isinstance(lf0, torch.Tensor):
        lf0 = _per_line(lf0, B, "lf0")
    if isinstance(seeds, torch.Tensor) and seeds.shape != (B,):
        raise L.HspError(f"seeds must be an int or an int64 [{B}] tensor, got shape {tuple(seeds.shape)}")
    if noise is not None and (noise.dim() != 3 or noise.shape[0] != B or noise.shape[1] != 192):
        raise L.HspError(f"noise must be fp32 [{B}, 192, >= T_max], got {tuple(noise.shape)}")
    Fh.check_noise_seeds(noise, noise_seeds, B)
    if row_exact and B > 1:
        from .hierspeechpp_speechsynthesizer import row_exact_refusal
        why = row_exact_refusal()
        if why is not None:
            raise L.HspError(f"row_exact is not available with {why}")
    if output_sr in (24000, 48000) and getattr(models, "sr", None) is None:
        raise L.HspError("output_sr 24000 / 48000 needs TtsModels(..., speechsr=<SpeechSR model>)")
    from .inference_vc import _device_lengths, output_length
    dev = lines[0][0].device
    _stage("prompts")
    if encoded is None:
        encoded = _encode_prompts(models, mel_fn, prompts, B, prompt_sr, denoise_ratio, denoised, denoiser, hps_denoiser)
    src_mel_ttv, ttv_len, style, peaks = _prompt_rows(*encoded, stage.scale_norm == "prompt")
    _stage("front")
    text, tone, language = (_pad_rows([line[i] for line in lines], N, torch.int64, dev) for i in range(3))
    text_length = _device_lengths(counts, dev)
    durs = None if dur is None else _pad_rows([d.to(torch.float32) for d in dur], N, torch.float32, dev)
    pace = {} if scale is None else dict(phone_scale=torch.from_numpy(scale).to(dev))
    x_frame, g, x_lengths, x_mask, frame_lengths = models.ttv.inf_extract_tc_latent(
        text, text_length, src_mel_ttv, ttv_len, tone, language, length_scale=length_scale, dur=durs, host_lengths=True,
        **pace)
    frames = [int(math.ceil(v)) for v in frame_lengths.tolist()]
    T2 = x_frame.shape[2]
    if isinstance(lf0, list):          # per-line rows, as `return_lf0` hands them back: each its line's 4 * frames
        for b, r in enumerate(lf0):
            if _row(r).shape[0] != 4 * frames[b]:
                raise L.HspError(f"line {b}: lf0 must hold {4 * frames[b]} values (4 per frame of the {frames[b]} "
                                 f"frames these durations give), got {_row(r).shape[0]}")
        lf0 = _pad_rows([r.to(torch.float32) for r in lf0], 4 * T2, torch.float32, dev)
    if noise is not None:
        if noise.shape[2] < T2:
            raise L.HspError(f"noise has {noise.shape[2]} columns; the longest line has {T2} frames")
        noise = noise[:, :, :T2].to(torch.float32).contiguous()
    _stage("plm")
    codes = _plm_codes(models, x_frame, frames, plm_sampling, seeds, plm_causal, plm_prefixes, prosody_codes,
                       prosody_lengths)
    _stage("vocoder")
    wav, audio, stats, track = _tts_from_codes(models, x_frame, g, codes, x_lengths, x_mask, None, None, noise_scale_vc,
                                               float(denoise_ratio), output_sr, noise, stage if int16 else None,
                                               0.999 if peaks is None else peaks, row_exact, style, noise_seeds, pitch,
                                               lf0)
    _stage("end")
    lengths = output_length(torch.ceil(x_lengths).to(torch.int64), output_sr)
    return (wav, lengths, audio, stats, [codes[b, :frames[b]] for b in range(B)], frames,
            [track[b, :4 * frames[b]] for b in range(B)])


@torch.no_grad()
def tts_batch(models: TtsModels, mel_fn, lines, prompts, *, return_float: bool = False, return_codes: bool = False,
              scale_norm: str = "max", target_lufs: float = -23.0, limiter: bool = False, ceiling_db: float = -1.0,
              lookahead_ms: float = 1.5, limiter_passes: int = 2, return_stats: bool = False, pitch=None, lf0=None,
              return_lf0: bool = False, length_scale=1.0, phone_scale=None, **kw):
    """`tts_from_prompt` for B different lines in one ragged batch; row b equals the one-line call on line b (same
    ``dur``, ``noise[b:b+1, :, :T_b]``, prompt and seed) -- DESIGN.md §4.3, INTEGRATION.md "reading a page".

    lines    B triples (ids, tone, language), each an int64 [N_b] or [1, N_b] device tensor, 1 <= N_b <= 438;
    prompts  one waveform (fp32 [n] / [1, n] at ``prompt_sr``, more than 640 samples at 16 kHz) shared by every line,
             or a list of B: lines holding the same tensor object share the prompt, whose mels, denoised form and
             style vector are computed once, as `tts_from_prompt` computes them;
    dur      a list of B [N_b] pinned durations, None: predicted (``length_scale``: the speaking rate, as
             ``inf_extract_tc_latent`` takes it);
    length_scale, phone_scale  the pace: a float for the page or a [B] sequence, one per line; a list of B rows of N_b
             factors, one per phone (None entries: 1), or None.  Each in [0.25, 4]; row b equals the one-line call with
             line b's values (`prosody_controls.check_scales`); pinned durations are scaled by ``phone_scale`` alone;
    pitch    a `prosody_controls.PitchEdit` whose per-row values are per line: the vocoder's log-F0 track of every
             line is edited over the line's own 4 * frames, as the one-line call edits it (one launch; None: none);
    lf0      given tracks instead of the pitch predictor's: a list of B fp32 [4 T_b] rows (what ``return_lf0`` hands
             back), or fp32 [B, 4 T_max]; a wrong width is an error that names the expected one;
    noise    fp32 [B, 192, >= T_max] (columns past the longest line's frames are ignored), None: drawn;
    noise_seeds  an int s (line b draws its prior noise with s + b) or an int64 [B] tensor, instead of ``noise``: the
             seeded stream of `tts`, so row b equals ``tts_from_prompt(noise_seed=s + b)`` and no noise tensor exists;
    denoise_ratio, denoised / denoiser / hps_denoiser  as `inference_vc.vc_batch`: the denoised prompts in the form
             of ``prompts``, or the denoiser that makes them in one packed pass (``denoise_prompts``);
    plm_sampling, seeds  sampled prosody codes; ``seeds`` an int s (line b draws with s + b) or an int64 [B] tensor;
    plm_causal, plm_prefixes  causal decoding; a list of B given beginnings (int64 [P_b], None entries allowed when
             the lengths differ), decoded by ``infer(prefix_codes=)`` when all have one length, else ``infer_many``;
    prosody_codes / prosody_lengths  lists of B: given codes instead of the prosody LM (the exclusions of `tts`);
    row_exact  True (the default): the vocoder and SpeechSR run every row as at B = 1; False: the padded-batch
             semantics of `tts`, exact only for equal frame counts and, as measured, no faster;
    scale_norm ... return_stats  the int16 stage (`output.OutputStage`, validated before anything else): every row
             over its own length, 'prompt' with the peak of the row's own prompt, taken on the device.

    Returns (wav int16 [B, n_max], lengths int64 [B] on the device): row b is wav[b, :lengths[b]], zeros after; then,
    where asked and in this order, the float audio [B, 1, n_max], the stats dict, the codes as a list of B int64
    [T_b], and with ``return_lf0`` the log-F0 tracks the vocoder was given as a list of B fp32 [4 T_b]."""
    stage = OutputStage(scale_norm, target_lufs, limiter, ceiling_db, lookahead_ms, limiter_passes,
                        return_stats).check()
    wav, lengths, audio, stats, codes, _, tracks = _tts_batch(models, mel_fn, lines, prompts, stage, pitch=pitch, lf0=lf0,
                                                              length_scale=length_scale, phone_scale=phone_scale, **kw)
    return pack(wav, (lengths, True), (audio, return_float), (stats, return_stats), (codes, return_codes),
                (tracks, return_lf0))


def _take(arg, rows):
    return None if arg is None else [arg[k] for k in rows]


def _line_seeds(seeds, N: int, what: str):
    """The per-line seeds int64 [N] of a page (``seeds`` / ``noise_seeds`` alike): an int s gives the caller's line k
    the seed s + k; a tensor [N] holds one per line.  `tts_lines` slices them per chunk."""
    if isinstance(seeds, torch.Tensor):
        if seeds.shape != (N,):
            raise L.HspError(f"{what} must be an int or an int64 [{N}] tensor, got shape {tuple(seeds.shape)}")
        return seeds.to(torch.int64)
    return torch.arange(int(seeds), int(seeds) + N, dtype=torch.int64)


@torch.no_grad()
def tts_lines(models: TtsModels, mel_fn, lines, prompts, *, max_batch: int = 16, join: bool = False,
              pause_ms: float = 300.0, return_float: bool = False, return_codes: bool = False, dur=None, noise=None,
              seeds=0, plm_prefixes=None, prosody_codes=None, prosody_lengths=None, denoised=None, noise_seeds=None,
              pitch=None, lf0=None, return_lf0: bool = False, length_scale=1.0, phone_scale=None, **kw):
    """Any number of lines: sorted by phone count, cut into chunks of at most ``max_batch`` (`line_chunks`), one
    `tts_batch` per chunk (the per-line keywords ``dur``, ``noise`` rows, ``seeds``, ``noise_seeds``, ``plm_prefixes``,
    ``prosody_codes`` / ``prosody_lengths``, the rows of ``pitch``, ``lf0`` (a list of N rows), a per-line
    ``length_scale`` and ``phone_scale`` sliced per chunk; an int ``seeds`` / ``noise_seeds`` = s gives the caller's
    line k the seed s + k whatever chunk it lands in), results in the caller's order.  ``return_lf0``: the lines'
    log-F0 tracks (a list of N fp32 [4 T_k]) come last, after the codes.  Every distinct prompt of the
    page is encoded, and with a denoiser denoised, once per call, whatever chunks its lines fall into.  Other keywords
    go to `tts_batch`.

    ``join`` False: a list of N int16 rows [n_k]; then, where asked, the float rows (a list of [n_k]), the stats (a
    dict of [N] tensors) and the codes (a list).  ``join`` True: one programme, int16 [n]: the float rows concatenated
    at the output rate with ``round(pause_ms * rate / 1000)`` zero samples between consecutive lines (`join_plan`) and
    converted by one `OutputStage.int16` call, so scale_norm='lufs' meters the programme, not each line ('prompt' is
    refused: a programme has no single prompt); then the float programme [1, 1, n], the stats and the codes where
    asked.  The lines' lengths come from the front-end's own read-back, so the join is slices and copies."""
    stage = OutputStage.of(kw).check()
    for name in ("scale_norm", "target_lufs", "limiter", "ceiling_db", "lookahead_ms", "limiter_passes", "return_stats"):
        kw.pop(name, None)
    if int(max_batch) < 1:
        raise L.HspError(f"max_batch must be >= 1, got {max_batch}")
    if not pause_ms >= 0:
        raise L.HspError(f"pause_ms must be >= 0, got {pause_ms}")
    if join and stage.scale_norm == "prompt":
        raise L.HspError("join=True takes scale_norm 'max' or 'lufs': a programme has no single prompt")
    counts = check_lines(lines, prompts, dur, kw.get("plm_sampling"), kw.get("plm_causal", False), plm_prefixes,
                         prosody_codes, prosody_lengths, denoised)
    _check_denoiser(kw.get("denoise_ratio", 0.0), denoised, kw.get("denoiser"), kw.get("hps_denoiser"), "tts_lines")
    from .inference_vc import output_length
    N, output_sr = len(lines), kw.get("output_sr", 16000)
    Fh.check_noise_seeds(noise, noise_seeds, N)
    if pitch is not None:
        PC.check_pitch(pitch, N)
    PC.check_scales(length_scale, phone_scale, counts, dur is not None)
    lf0 = _per_line(lf0, N, "lf0")
    per_scale = not isinstance(length_scale, (int, float))
    line_seeds = _line_seeds(seeds, N, "seeds")
    line_noise_seeds = None if noise_seeds is None else _line_seeds(noise_seeds, N, "noise_seeds")
    dev = lines[0][0].device
    chunks = line_chunks(counts, max_batch)
    per_prompt = isinstance(prompts, (list, tuple)) and len(prompts) == N and N > 1
    per_denoised = isinstance(denoised, (list, tuple)) and len(denoised) == N and N > 1
    # every distinct prompt of the page is encoded (and denoised) once, whatever chunks its lines fall into
    encoded, index = _encode_prompts(models, mel_fn, prompts, N, kw.get("prompt_sr", 16000), kw.get("denoise_ratio", 0.0),
                                     denoised, kw.get("denoiser"), kw.get("hps_denoiser"))
    wavs, floats, codes, n_out, part_stats, tracks = [], [], [], [], [], []
    for rows in chunks:
        idx = torch.tensor(rows, dtype=torch.int64)
        wav, _, audio, stats, cds, frames, trk = _tts_batch(
            models, mel_fn, [lines[k] for k in rows], _take(prompts, rows) if per_prompt else prompts,
            stage, dur=_take(dur, rows), noise=None if noise is None else noise[idx.to(noise.device)],
            seeds=line_seeds[idx.to(line_seeds.device)].to(dev),
            noise_seeds=None if line_noise_seeds is None else line_noise_seeds[idx.to(line_noise_seeds.device)].to(dev),
            plm_prefixes=_take(plm_prefixes, rows),
            prosody_codes=_take(prosody_codes, rows), prosody_lengths=_take(prosody_lengths, rows),
            denoised=_take(denoised, rows) if per_denoised else denoised, int16=not join,
            encoded=(encoded, [index[k] for k in rows]), pitch=None if pitch is None else pitch.rows(rows),
            lf0=_take(lf0, rows), length_scale=[float(length_scale[k]) for k in rows] if per_scale else length_scale,
            phone_scale=_take(phone_scale, rows), **kw)
        for i in range(len(rows)):
            n = output_length(frames[i], output_sr)
            n_out.append(n)
            floats.append(audio[i, 0, :n])
            if not join:
                wavs.append(wav[i, :n])
        codes += cds
        tracks += trk
        part_stats.append(stats)
    inv = chunk_order(chunks)
    back = lambda flat: [flat[i] for i in inv]  # noqa: E731
    floats, codes, n_out, tracks = back(floats), back(codes), back(n_out), back(tracks)
    if not join:
        stats = None
        if stage.return_stats:
            order = torch.tensor(inv, device=dev)
            stats = {k: torch.cat([ps[k] for ps in part_stats])[order] for k in part_stats[0]}
        return pack(back(wavs), (floats, return_float), (stats, stage.return_stats), (codes, return_codes),
                    (tracks, return_lf0))
    rate = output_rate(output_sr)
    offsets, total = join_plan(n_out, rate, pause_ms)
    programme = torch.zeros(1, 1, total, dtype=torch.float32, device=dev)
    for off, n, row in zip(offsets, n_out, floats):
        programme[0, 0, off:off + n].copy_(row)
    wav, stats = stage.int16(programme, None, rate, 0.999)
    return pack(wav.reshape(-1), (programme, return_float), (stats, stage.return_stats), (codes, return_codes),
                (tracks, return_lf0))


def tts_batch_files(models: TtsModels, mel_fn, lines, prompt_paths, out_dir=None, names=None, device=None, pitch=None,
                    lf0=None, return_lf0: bool = False, length_scale=1.0, phone_scale=None, **kw):
    """`tts_lines` from prompt FILES: ``prompt_paths`` one WAV file for every line or a list of one per line, at any
    sample rate; every distinct file is loaded once (``audio.load_16k``: channel 0, kaiser-window resampling to
    16 kHz) and shared by the lines that name it.  ``pitch`` / ``lf0`` / ``return_lf0`` / ``length_scale`` /
    ``phone_scale`` and the keywords ``kw`` go to `tts_lines` (``noise`` rows, ``noise_seeds`` and the per-line prosody
    controls are indexed by the caller's line order).  With ``out_dir`` the rows are
    written as ``<out_dir>/<names[k]>.wav`` (``names`` None: ``line_0000.wav``, ...) at the output rate, or as one
    ``programme.wav`` with ``join=True``.  Returns what `tts_lines` returns."""
    import os
    from . import audio as A
    OutputStage.of(kw).check()          # before any file is read
    if not isinstance(lines, (list, tuple)) or not lines:
        raise L.HspError("lines must be a non-empty list of (ids, tone, language) triples")
    N = len(lines)
    Fh.check_noise_seeds(kw.get("noise"), kw.get("noise_seeds"), N)
    PC.check_pitch(pitch, N)
    per_line = isinstance(prompt_paths, (list, tuple))
    paths = [str(p) for p in prompt_paths] if per_line else [str(prompt_paths)]
    if len(paths) not in (1, N):
        raise L.HspError(f"give one prompt file or one per line ({N}), got {len(paths)}")
    if names is not None and len(names) != N:
        raise L.HspError(f"names must hold one name per line ({N}), got {len(names)}")
    if kw.get("prompt_sr", 16000) != 16000:
        raise L.HspError("tts_batch_files reads the rate from each file: prompt_sr is not a keyword here")
    check_lines(lines, paths, kw.get("dur"), kw.get("plm_sampling"), kw.get("plm_causal", False),
                kw.get("plm_prefixes"), kw.get("prosody_codes"), kw.get("prosody_lengths"), kw.get("denoised"))
    if device is None:
        device = lines[0][0].device
    loaded = {p: A.load_16k(p, device) for p in dict.fromkeys(paths)}       # each distinct prompt file loaded once
    out = tts_lines(models, mel_fn, lines, [loaded[p] for p in paths] if len(paths) > 1 else loaded[paths[0]],
                    pitch=pitch, lf0=lf0, return_lf0=return_lf0, length_scale=length_scale, phone_scale=phone_scale, **kw)
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        rate = output_rate(kw.get("output_sr", 16000))
        first = out[0] if isinstance(out, tuple) else out
        if kw.get("join", False):
            write_wav(os.path.join(str(out_dir), "programme.wav"), rate, first)
        else:
            for k, row in enumerate(first):
                write_wav(os.path.join(str(out_dir), f"{names[k] if names is not None else f'line_{k:04d}'}.wav"),
                          rate, row)
    return out
