"""Audio file ingest of the reference harnesses: ``torchaudio.load(path)`` (normalize=True) for RIFF WAV, then the
"first channel -> 16 kHz" idiom of inference_plm.py:120-126, inference.py:118-124, inference_vc.py:76-78,98-103 and
inference_speechsr.py:28-34.  Decoding is host plumbing (scipy.io.wavfile, a reference dependency); the resampling
runs on the GPU (functional.resample)."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from . import functional as Fh


def load(path):
    """torchaudio.load(path, normalize=True) for WAV: -> (float32 [channels, n] CPU tensor, sample rate).
    Scaling: int16 / 2^15; int32 and 24-bit (read as the top 24 bits of int32) / 2^31; uint8 (x - 128) / 128;
    float32 as stored (float64 cast to float32)."""
    from scipy.io import wavfile
    rate, data = wavfile.read(str(path))
    if data.dtype == np.int16:
        a = data.astype(np.float32) / np.float32(32768.0)
    elif data.dtype == np.int32:
        a = data.astype(np.float32) / np.float32(2.0 ** 31)
    elif data.dtype == np.uint8:
        a = (data.astype(np.float32) - np.float32(128.0)) / np.float32(128.0)
    elif data.dtype in (np.float32, np.float64):
        a = data.astype(np.float32)
    else:
        raise L.HspError(f"{path}: unsupported WAV sample type {data.dtype}")
    a = a.reshape(a.shape[0], -1).T                  # [n] / [n, ch] -> [ch, n]
    return torch.from_numpy(np.ascontiguousarray(a)), int(rate)


def load_16k(path, device):
    """The reference's three lines after torchaudio.load: keep channel 0, move it to ``device``, and resample to 16 kHz
    with resampling_method="kaiser_window" when the file has another rate.  -> fp32 [1, n16] on ``device``."""
    audio, rate = load(path)
    audio = audio[:1].to(device)
    if rate != 16000:
        audio = Fh.resample(audio, rate, 16000, resampling_method="kaiser_window")
    return audio
