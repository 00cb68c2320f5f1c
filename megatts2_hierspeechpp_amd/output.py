"""The output stage of every harness (inference_plm, inference_vc, inference_speechsr), float rows -> int16 rows:
`OutputStage` holds what a call asked for, validates it once and picks the conversion; `output_rate` is the rate rule
and `pack` the order of a harness's results."""
from __future__ import annotations

from dataclasses import dataclass, fields

import numpy as np
import torch

from . import _lib as L
from . import functional as Fh

# the rules of the int16 stage: the reference's two peak rules (inference_plm.py:185-188) and the loudness target
SCALE_NORMS = ("max", "prompt", "lufs")


@torch.no_grad()
def prompt_peak(audio) -> float:
    """``torch.max(audio.abs())`` of scale_norm='prompt' (inference_plm.py:127-128, inference_vc.py:104-105), taken as
    the reference does on the CPU copy of the 16 kHz prompt: a host synchronise, not for use inside a captured graph."""
    return float(np.abs(audio.detach().cpu().numpy()).max())


def output_rate(output_sr: int) -> int:
    """The rate of a harness's rows and of its WAV header (inference_vc.py:164-170): 48000, 24000, else 16000."""
    return output_sr if output_sr in (24000, 48000) else 16000


def pack(first, *optional):
    """The result of a harness: ``first``, then the value of every wanted ``(value, wanted)`` pair in the order given
    -- audio, then stats, then codes.  One result is returned bare, more as a tuple."""
    out = (first, *(value for value, wanted in optional if wanted))
    return out if len(out) > 1 else out[0]


@dataclass(frozen=True)
class OutputStage:
    """What a harness call asked of its int16 stage.
    ``scale_norm`` 'max': every row is scaled by its own peak (over its own length) times 0.999 (inference_plm.py:
      187-188); 'prompt': times the prompt's peak instead (:185-186; `gain` reads it back to the host) -- a prompt whose
      peak is above 1 (full scale) is outside the contract: the reference's astype('int16') wraps such samples around,
      hsp_peak_int16 saturates them; 'lufs': every row is brought to ``target_lufs`` (BS.1770-4, metered at the output
      rate over the row's own length; `functional.lufs_int16`), its peak held at 0.999 of full scale at the most.
    ``limiter`` (needs 'lufs'): a row whose peaks would pass the ceiling is not held under the target but run through
      the look-ahead true-peak limiter (`functional.lufs_limit_int16`: ``ceiling_db`` dBTP, ``lookahead_ms``,
      ``limiter_passes`` meter-and-limit rounds, 1 ... 4).
    ``return_stats`` (needs ``limiter``): the harness returns the limiter's per-row stats -- a dict of fp32 [B] device
      tensors achieved_lufs, true_peak, min_gain -- after the audio and before any codes.
    The gain of 'max' / 'prompt' is data, not policy: an argument of `int16`."""
    scale_norm: str = "max"
    target_lufs: float = -23.0
    limiter: bool = False
    ceiling_db: float = -1.0
    lookahead_ms: float = 1.5
    limiter_passes: int = 2
    return_stats: bool = False

    @classmethod
    def of(cls, kwargs) -> "OutputStage":
        """The stage a ``**kwargs`` harness was asked for: the fields that ``kwargs`` names, defaults for the rest."""
        return cls(**{f.name: kwargs[f.name] for f in fields(cls) if f.name in kwargs})

    def check(self, norms=SCALE_NORMS) -> "OutputStage":
        """The one validation, in one order: an unknown ``scale_norm`` (``norms``: the ones the harness takes), the
        limiter without 'lufs', the stats without the limiter.  -> self"""
        if self.scale_norm not in norms:
            names = (" or " if len(norms) == 2 else ", ").join(map(repr, norms))
            raise L.HspError(f"unknown scale_norm {self.scale_norm!r} ({names})")
        if self.limiter and self.scale_norm != "lufs":
            raise L.HspError(f"limiter=True needs scale_norm='lufs', got {self.scale_norm!r}: the limiter serves the "
                             "loudness target")
        if self.return_stats and not self.limiter:
            raise L.HspError("return_stats=True needs limiter=True: the stats are the limiter's")
        return self

    def gain(self, prompt_audio) -> float:
        """The gain of the int16 conversion: the prompt's peak for 'prompt', else 0.999 -- the gain of 'max' and the
        ceiling of 'lufs', which has no fixed gain (it is metered per row on the device)."""
        if self.scale_norm == "prompt":
            return prompt_peak(prompt_audio)
        self.check()                    # an unknown norm has no gain
        return 0.999

    def int16(self, audio, n_valid, rate: int, gain=0.999):
        """The one dispatch: fp32 [B, 1, n] / [B, n] with ``n_valid`` int64 [B] samples per row (None: all n) at
        ``rate`` -> (int16 [B, n], the limiter's stats or None).  ``gain``: a float or a device fp32 [B]."""
        if self.scale_norm != "lufs":
            return Fh.peak_int16(audio, n_valid, gain), None
        if not self.limiter:
            return Fh.lufs_int16(audio, n_valid, rate, self.target_lufs), None
        return Fh.lufs_limit_int16(audio, n_valid, rate, self.target_lufs, self.ceiling_db, self.lookahead_ms,
                                   self.limiter_passes)
