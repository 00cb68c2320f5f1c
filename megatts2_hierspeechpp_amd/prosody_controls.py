"""Prosody controls of a take (no counterpart in the reference): the pitch edit of the log-F0 track
the vocoder is given (`PitchEdit`, one launch of hsp_f0_edit_rows_f32) and the checks of the pace keywords
(``length_scale`` per line, ``phone_scale`` per phone) of the TTS harnesses.

The track is the one both harnesses hand to ``voice_conversion_noise_control``: l = log(f0 + 1), fp32, 0 = unvoiced,
200 frames a second (4 per vocoder frame)."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from . import functional as Fh

SHIFT_MAX = 48.0               # semitones: four octaves either way
RANGE_MAX = 4.0
F_MIN_FLOOR = 55.0             # the harness's own voicing floor (inference_plm.py:166)
SCALE_MIN, SCALE_MAX = 0.25, 4.0


def _host(v):
    """A float, sequence or tensor as a float64 numpy array (a device tensor is read back: `check` runs once)."""
    if isinstance(v, torch.Tensor):
        return v.detach().to("cpu", torch.float64).numpy()
    return np.asarray(v, dtype=np.float64)


def _per_row(v, B: int, name: str):
    """``v`` (a float or a [B] sequence / tensor) as float64 [B]."""
    a = _host(v)
    if a.ndim == 0:
        return np.full(B, float(a))
    if a.shape != (B,):
        raise L.HspError(f"PitchEdit.{name} must be a float or hold one value per row ({B}), got shape {a.shape}")
    return a


@dataclass(frozen=True, eq=False)
class PitchEdit:
    """What a harness call asked of the pitch of its rows (include/hsp.h "pitch edit of a log-F0 track").

    ``shift``      semitones added to every voiced frame;
    ``range``      the factor on a voiced frame's distance (in ln Hz) from the row's own mean: 0 flattens the row onto
                   its geometric mean, 1 keeps it, 2 doubles every excursion;
    ``target_hz``  the register the row's geometric mean is moved to; None (or 0 for a row): it stays;
    ``offsets``    a drawn contour: semitones per frame, fp32 [B, n] (a tensor or a list of rows; a row shorter than the
                   track is continued with zeros, a longer one is cut);
    ``f_min`` / ``f_max``  the edited track is clamped into them (Hz): 55 is the harness's voicing floor, 1100 the
                   reference's ``f0_max``.
    ``shift`` / ``range`` / ``target_hz`` are a float for every row or a [B] sequence or tensor, one per row.
    Unvoiced frames stay unvoiced.  A row with shift 0, range 1, no target and no ``offsets`` is an identity row and is
    copied bit for bit; an edit of identity rows alone (`is_identity`) makes no launch in the harnesses."""
    shift: object = 0.0
    range: object = 1.0
    target_hz: object = None
    offsets: object = None
    f_min: float = 55.0
    f_max: float = 1100.0

    def check(self, B: Optional[int] = None) -> "PitchEdit":
        """Validate once (shapes against ``B`` rows where the caller knows them); -> self."""
        fmin, fmax = float(self.f_min), float(self.f_max)
        if not (math.isfinite(fmin) and math.isfinite(fmax)):
            raise L.HspError(f"PitchEdit: f_min and f_max must be finite, got {self.f_min} and {self.f_max}")
        if not F_MIN_FLOOR <= fmin < fmax:
            raise L.HspError(f"PitchEdit: needs {F_MIN_FLOOR:g} <= f_min < f_max, got f_min = {fmin:g}, f_max = {fmax:g}")
        rows = B
        for name in ("shift", "range", "target_hz"):
            v = getattr(self, name)
            if v is None:
                if name != "target_hz":
                    raise L.HspError(f"PitchEdit.{name} must be a number or one per row, got None")
                continue
            a = _host(v)
            if a.ndim > 1 or (a.ndim == 1 and rows is not None and a.shape[0] != rows):
                raise L.HspError(f"PitchEdit.{name} must be a float or hold one value per row"
                                 f"{'' if rows is None else f' ({rows})'}, got shape {a.shape}")
            if a.ndim == 1 and rows is None:
                rows = a.shape[0]
            if not np.isfinite(a).all():
                raise L.HspError(f"PitchEdit.{name} must be finite")
            if name == "shift" and (np.abs(a) > SHIFT_MAX).any():
                raise L.HspError(f"PitchEdit.shift must lie in [-{SHIFT_MAX:g}, {SHIFT_MAX:g}] semitones")
            if name == "range" and ((a < 0.0) | (a > RANGE_MAX)).any():
                raise L.HspError(f"PitchEdit.range must lie in [0, {RANGE_MAX:g}]")
            if name == "target_hz" and (a < 0.0).any():
                raise L.HspError("PitchEdit.target_hz must be positive (0: no target for that row)")
        off = self.offsets
        if off is not None:
            if isinstance(off, torch.Tensor):
                if off.dim() != 2 or (rows is not None and off.shape[0] != rows):
                    raise L.HspError(f"PitchEdit.offsets must be [B{'' if rows is None else f' = {rows}'}, n] or a list "
                                     f"of rows, got shape {tuple(off.shape)}")
                seq = [off]
            elif isinstance(off, (list, tuple)):
                if rows is not None and len(off) != rows:
                    raise L.HspError(f"PitchEdit.offsets must be [B = {rows}, n] or a list of {rows} rows, got "
                                     f"{len(off)} rows")
                seq = list(off)
            else:
                raise L.HspError("PitchEdit.offsets must be a [B, n] tensor or a list of rows")
            for r in seq:
                if not np.isfinite(_host(r)).all():
                    raise L.HspError("PitchEdit.offsets must be finite")
        return self

    @property
    def is_identity(self) -> bool:
        """No row changes: no launch is needed."""
        if self.offsets is not None:
            return False
        t = self.target_hz
        return bool((_host(self.shift) == 0.0).all() and (_host(self.range) == 1.0).all()
                    and (t is None or (_host(t) == 0.0).all()))

    def rows(self, index) -> "PitchEdit":
        """The edit of the rows ``index`` (a list of ints) of this one, in that order: what `tts_lines` hands a chunk."""
        def take(v):
            if v is None or (not isinstance(v, (list, tuple, torch.Tensor, np.ndarray))) or \
                    (isinstance(v, (torch.Tensor, np.ndarray)) and v.ndim == 0):
                return v
            return [v[k] for k in index] if isinstance(v, (list, tuple)) else \
                v[torch.as_tensor(index, device=v.device) if isinstance(v, torch.Tensor) else np.asarray(index)]
        return PitchEdit(take(self.shift), take(self.range), take(self.target_hz), take(self.offsets), self.f_min,
                         self.f_max)

    def operands(self, B: int, n: int, device):
        """The launch's operands on ``device``: (shift, range, target_hz, offsets), fp32 [B] / [B, n], None where every
        row has the default (NULL in the launch)."""
        def vec(v, default, name):
            if v is None:
                return None
            if isinstance(v, torch.Tensor) and v.dim() == 1:
                if v.shape[0] != B:
                    raise L.HspError(f"PitchEdit.{name} must be a float or hold one value per row ({B}), got shape "
                                     f"{tuple(v.shape)}")
                return v.to(device=device, dtype=torch.float32).contiguous()
            a = _per_row(v, B, name)
            if (a == default).all():
                return None
            return torch.from_numpy(a.astype(np.float32)).to(device)
        off = self.offsets
        if off is not None:
            seq = list(off) if isinstance(off, (list, tuple)) else [off[b] for b in range(off.shape[0])]
            if len(seq) != B:
                raise L.HspError(f"PitchEdit.offsets must be [B = {B}, n] or a list of {B} rows, got {len(seq)} rows")
            full = torch.zeros(B, n, dtype=torch.float32, device=device)
            for b, r in enumerate(seq):
                r = torch.as_tensor(r, dtype=torch.float32).reshape(-1)[:n]
                full[b, :r.shape[0]].copy_(r)
            off = full
        return vec(self.shift, 0.0, "shift"), vec(self.range, 1.0, "range"), vec(self.target_hz, 0.0, "target_hz"), off

    def apply(self, lf0, lengths=None, return_mean: bool = False, out=None):
        """The edited track of ``lf0`` fp32 [B, n] (or [n]: one row) on the GPU, row b over ``lengths[b]`` frames (int64
        [B], None: all n) -- ONE launch, identity edits included (the harnesses skip those).  ``return_mean``: also
        mean_hz fp32 [B], the rows' geometric mean F0 before the edit.  ``out`` may be ``lf0``."""
        one = lf0.dim() == 1
        x = lf0.reshape(1, -1) if one else lf0
        if x.dim() != 2:
            raise L.HspError(f"PitchEdit.apply takes lf0 as fp32 [B, n] or [n], got {tuple(lf0.shape)}")
        if x.stride(1) != 1:
            x = x.contiguous()
        B, n = x.shape
        self.check(B)
        if lengths is not None:
            lengths = torch.as_tensor(lengths, dtype=torch.int64).to(x.device)
            if lengths.shape != (B,):
                raise L.HspError(f"PitchEdit.apply: lengths must be int64 [{B}], got {tuple(lengths.shape)}")
        shift, rng, target, off = self.operands(B, n, x.device)
        got = Fh.f0_edit(x, lengths, shift, rng, target, off, self.f_min, self.f_max,
                         out=None if out is None else out.reshape(B, n), return_mean=return_mean)
        y, mean = got if return_mean else (got, None)
        y = y.reshape(lf0.shape)
        return (y, mean) if return_mean else y


def check_pitch(pitch, B: Optional[int] = None):
    """The ``pitch=`` keyword of a harness: None or a checked `PitchEdit`; -> None where no launch is needed."""
    if pitch is None:
        return None
    if not isinstance(pitch, PitchEdit):
        raise L.HspError(f"pitch must be a prosody_controls.PitchEdit or None, got {type(pitch).__name__}")
    pitch.check(B)
    return None if pitch.is_identity else pitch


def check_lf0(lf0, B: int, T2: int):
    """The ``lf0=`` keyword of a TTS harness against the front-end's frame count: fp32 [B, 4 * T2]."""
    if not isinstance(lf0, torch.Tensor) or lf0.dim() not in (1, 2) or lf0.reshape(-1, lf0.shape[-1]).shape != (B, 4 * T2):
        got = tuple(lf0.shape) if isinstance(lf0, torch.Tensor) else type(lf0).__name__
        raise L.HspError(f"lf0 must be fp32 [{B}, {4 * T2}] (4 per frame of the {T2} frames these durations give), got "
                         f"{got}")
    return lf0.reshape(B, 4 * T2).to(torch.float32).contiguous()


def _check_scale(a, what: str):
    if not np.isfinite(a).all() or (a < SCALE_MIN).any() or (a > SCALE_MAX).any():
        raise L.HspError(f"{what} must lie in [{SCALE_MIN:g}, {SCALE_MAX:g}]")


def check_scales(length_scale, phone_scale, counts, given_dur: bool = False):
    """The pace keywords of a TTS harness, from shapes and values alone (no device work): ``length_scale`` a float or a
    [B] sequence, ``phone_scale`` None or a list of B rows of ``counts[b]`` factors, all in [0.25, 4].
    -> (the float the duration kernel takes, the scales float32 [B, max(counts)] as a numpy array or None).
    A float ``length_scale`` without ``phone_scale`` goes to hsp_duration_f32 as before (None).  Otherwise the row's
    length_scale is folded into its phone scales -- ONE fp32 product per phone, formed here -- and the kernel runs with
    length_scale 1: ``exp(logw) * 1`` is exact, so a per-row length_scale alone gives the bits of the float form, and
    a row of a batch gets the factors its one-line call gets.  ``given_dur``: the durations are the caller's, which
    ``length_scale`` has never scaled (ttv_v1/t2w2v_transformer.py:955-957 scales the predicted ones): it is checked
    and not folded, and ``phone_scale`` alone scales them."""
    B = len(counts)
    ls = _host(length_scale)
    if ls.ndim > 1 or (ls.ndim == 1 and ls.shape[0] != B):
        raise L.HspError(f"length_scale must be a float or hold one value per line ({B}), got shape {ls.shape}")
    _check_scale(ls, "length_scale")
    if phone_scale is None and (ls.ndim == 0 or given_dur):
        return (float(ls) if ls.ndim == 0 else 1.0), None
    if phone_scale is not None and (not isinstance(phone_scale, (list, tuple)) or len(phone_scale) != B):
        got = len(phone_scale) if isinstance(phone_scale, (list, tuple)) else type(phone_scale).__name__
        raise L.HspError(f"phone_scale must be a list of one row per line ({B}), got {got}")
    per_row = np.ones(B, np.float32) if given_dur else np.broadcast_to(ls, (B,)).astype(np.float32)
    scale = np.ones((B, max(counts)), dtype=np.float32)
    for b in range(B):
        row = np.ones(counts[b], dtype=np.float32)
        if phone_scale is not None and phone_scale[b] is not None:
            given = _host(phone_scale[b]).reshape(-1)
            if given.shape[0] != counts[b]:
                raise L.HspError(f"line {b}: {given.shape[0]} phone scales for {counts[b]} phones")
            _check_scale(given, f"phone_scale of line {b}")
            row = given.astype(np.float32)
        scale[b, :counts[b]] = per_row[b] * row
    return 1.0, scale
