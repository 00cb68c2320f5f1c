"""HIP mirror of the reference's inference_speechsr.py:SuperResoltuion (:21-50): speech at any rate -> channel 0 ->
16 kHz (kaiser-window resampling, :28-34) -> SpeechSR (speechsr48k / speechsr24k) -> int16 peak-normalised with
gain 0.999 (:37-40; or brought to a target loudness, scale_norm="lufs") -> optional 16-bit WAV at 48 or 24 kHz
(:45-48)."""
from __future__ import annotations

import torch

from . import functional as Fh
from .inference_plm import write_wav
from .output import OutputStage, pack


@torch.no_grad()
def super_resolution(sr_model, audio, sample_rate: int, output_sr: int = 48000, output_path=None,
                     scale_norm: str = "max", target_lufs: float = -23.0, limiter: bool = False,
                     ceiling_db: float = -1.0, lookahead_ms: float = 1.5, limiter_passes: int = 2,
                     return_stats: bool = False):
    """``sr_model`` a finalized SpeechSR (speechsr48k / speechsr24k SynthesizerTrn); ``audio`` fp32 [channels, n] on
    the GPU at ``sample_rate`` (``audio.load(path)`` moved there).  Returns int16 [n_out].  As in the reference, the
    model fixes the upsampling factor and ``output_sr`` only labels the file: 48000, or 24000 for any other value.
    ``scale_norm`` ... ``return_stats``: the int16 stage, see `output.OutputStage` -- 'max' or 'lufs' here (there is no
    prompt), metered at the rate the model produced: 16 kHz times its upsampling factor."""
    stage = OutputStage(scale_norm, target_lufs, limiter, ceiling_db, lookahead_ms, limiter_passes, return_stats)
    stage.check(norms=("max", "lufs"))
    x = audio[:1]
    if int(sample_rate) != 16000:
        x = Fh.resample(x, sample_rate, 16000, resampling_method="kaiser_window")
    y = sr_model(x.unsqueeze(1))                                   # [1, 1, n_out]
    wav, stats = stage.int16(y, None, 16000 * y.shape[-1] // x.shape[-1])
    wav = wav.reshape(-1)
    if output_path is not None:
        write_wav(output_path, 48000 if output_sr == 48000 else 24000, wav)
    return pack(wav, (stats, return_stats))
