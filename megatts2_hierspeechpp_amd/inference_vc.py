"""The tensor core of the reference's voice-conversion harness (reference: inference_vc.py:70-160): source waveform
-> reflect pad 40 -> wav2vec2 hidden state 7 -> (with the source's and the prompt's F0 tracks) F0 conversion ->
prompt mels -> ``voice_conversion_noise_control`` -> peak-normalised int16.

File ingest (:76-78,98-103: ``torchaudio.load`` + kaiser-window resampling to 16 kHz) is ``load_source`` for the
source and ``audio.load_16k`` for the target prompt; ``scale_norm='prompt'`` (:104-105,157-158) is
``vc(scale_norm="prompt")``.  Outside this module: the YAAPT pitch tracker (third-party ``amfm_decompy``, CPU numpy
code, absent from this image).  The F0 tracks are inputs here, computed by the caller from the 16 kHz audio (the padded
source, the unpadded target) at the tracker's rate of 200 Hz (4 per w2v frame), zeros where unvoiced.

``vc_batch`` / ``vc_batch_files`` convert many sources in one pass (the reference converts one file per process call);
row b of a batch is held to ``vc`` run on row b alone."""
from __future__ import annotations

import os
from typing import Optional

import numpy as np
import torch
from torch import nn

from . import _lib as L
from . import functional as Fh
from . import hip_layers
from . import prosody_controls as PC
from .output import OutputStage, output_rate, pack

SOURCE_HOP = 1280   # pad_source's multiple (inference_vc.py:74-75)
W2V_PAD = 40        # reflect pad before wav2vec2 (:85)
FRAME = 320         # samples per w2v / vocoder frame
F0_HOP = 80         # samples per YAAPT frame (5 ms): 4 per w2v frame

STAGE_HOOK = None   # measurement hook (tools/vc_batch_bench.py): STAGE_HOOK(name) at the start of every vc_batch stage
TAP_HOOK = None     # test hook: TAP_HOOK(name, tensor) with vc_batch's intermediates ('reflect_pad', 'w2v', 'lf0',
                    # 'mel', 'style'; 'mel' once per distinct prompt: its [2, 80, Tm] prompt | denoised mels), no effect
                    # when None


class VcModels(nn.Module):
    """The models the harness loads (inference_vc.py:model_load): the vocoder, the wav2vec2 producer and, optionally,
    SpeechSR (``speechsr``: a speechsr48k / speechsr24k SynthesizerTrn, as in TtsModels) for output_sr 24000 / 48000."""

    def __init__(self, voc_cfg, spec_channels=641, segment_frames=61440 // 320, w2v_layer=7,
                 speechsr: Optional[nn.Module] = None):
        super().__init__()
        from .extract_w2v import Wav2vec2
        from .hierspeechpp_speechsynthesizer import SynthesizerTrn
        self.voc = SynthesizerTrn(spec_channels, segment_frames, **voc_cfg)
        self.w2v = Wav2vec2(layer=w2v_layer)
        if speechsr is not None:
            self.sr = speechsr

    def finalize(self, device, materialize: bool = True):
        from .hip_layers import finalize
        self.arena = finalize(self, device, materialize)
        return self


def pad_source(audio, hop: int = 1280):
    """inference_vc.py:74-75: zero-pad the source to the next multiple of 1280 samples (always at least one sample)."""
    n = audio.shape[-1]
    p = (n // hop + 1) * hop - n
    out = torch.zeros(*audio.shape[:-1], n + p, dtype=torch.float32, device=audio.device)
    out[..., :n] = audio
    return out


def load_source(path, device):
    """inference_vc.py:76-78: the source file at 16 kHz (``audio.load_16k``: channel 0, kaiser-window resampling),
    padded by `pad_source` -> fp32 [1, Ls] on ``device``."""
    from .audio import load_16k
    return pad_source(load_16k(path, device))


@torch.no_grad()
def vc(models: VcModels, mel_fn, source_audio, f0_src, target_audio, f0_trg, noise_scale_vc=0.333, denoise_ratio=0.0,
       denoised_audio=None, noise=None, return_float=False, scale_norm="max", output_sr=16000, target_lufs=-23.0,
       limiter=False, ceiling_db=-1.0, lookahead_ms=1.5, limiter_passes=2, return_stats=False, noise_seed=None,
       pitch=None, return_lf0=False):
    """source_audio [1, Ls] (16 kHz, already padded by pad_source), f0_src [1, Ls / 80] (YAAPT, 0 = unvoiced),
    target_audio [1, Lt], f0_trg [1, Lt / 80] -> int16 waveform [320 T] (and the float audio with return_float).
    ``output_sr`` 24000 / 48000: SpeechSR (``models.sr``) runs after the vocoder (:147-151) -> [480 T] / [960 T].
    ``denoised_audio``: the denoiser's output for the prompt (inference_vc.py:118-121); None = the prompt itself, which
    is what the reference does at denoise_ratio == 0.  ``scale_norm`` ... ``return_stats``: the int16 stage, see
    `output.OutputStage`; the prompt of 'prompt' is ``target_audio`` (inference_vc.py:104-105).
    ``noise_seed`` (an int; excludes ``noise``): the vocoder's prior noise is the seeded stream of include/hsp.h "seeded
    prior noise", so the same call gives the same waveform; None: ``noise``, or torch's process-wide generator.
    ``pitch`` (a `prosody_controls.PitchEdit`): the converted log-F0 track is edited before the vocoder reads it (one
    launch; None or an identity edit: none).  ``return_lf0``: the track the vocoder was given, fp32 [4 T], comes last."""
    stage = OutputStage(scale_norm, target_lufs, limiter, ceiling_db, lookahead_ms, limiter_passes,
                        return_stats).check()
    pitch = PC.check_pitch(pitch, 1)
    if isinstance(noise_seed, torch.Tensor):
        raise L.HspError("noise_seed is one int")
    Fh.check_noise_seeds(noise, noise_seed, what="noise_seed")
    gain = stage.gain(target_audio)
    x_w2v = models.w2v(Fh.reflect_pad(source_audio, 40))                       # :85-86
    T = x_w2v.shape[2]
    x_length = torch.tensor([T], dtype=torch.int64, device=x_w2v.device)
    lf0 = Fh.f0_convert(f0_src, f0_trg)                                        # :80-81,104-105
    second = target_audio if denoised_audio is None else denoised_audio
    both = torch.empty(2, target_audio.shape[-1], dtype=torch.float32, device=target_audio.device)
    both[0].copy_(target_audio.reshape(-1))
    both[1].copy_(second.reshape(-1)[:target_audio.shape[-1]])
    trg_mel = mel_fn(both)                                                     # [2, 80, Tm]  (:113-126)
    trg_len = torch.tensor([trg_mel.shape[2]] * 2, dtype=torch.int64, device=x_w2v.device)
    lf0 = lf0.reshape(1, -1)[:, :4 * T]
    if pitch is not None:
        lf0 = pitch.apply(lf0)
    audio = models.voc.voice_conversion_noise_control(x_w2v, x_length, trg_mel, trg_len, lf0,
                                                      noise_scale=noise_scale_vc, denoise_ratio=denoise_ratio,
                                                      noise=noise, noise_seeds=noise_seed)
    if output_sr in (24000, 48000):
        audio = _sr_model(models)(audio)                                       # :147-151
    wav, stats = stage.int16(audio.reshape(1, -1), None, output_rate(output_sr), gain)
    return pack(wav.reshape(-1), (audio, return_float), (stats, return_stats), (lf0.reshape(-1), return_lf0))


def _sr_model(models):
    sr = getattr(models, "sr", None)
    if sr is None:
        raise L.HspError("output_sr 24000 / 48000 needs VcModels(..., speechsr=<SpeechSR model>)")
    return sr


# ---------------------------------------------------------------- batched conversion: length arithmetic (host side)
def padded_length(n: int) -> int:
    """Samples of a source after pad_source: the next multiple of 1280 above n (at least one sample of padding)."""
    return (n // SOURCE_HOP + 1) * SOURCE_HOP


def w2v_frames(n_padded):
    """wav2vec2 frames of a padded source of ``n_padded`` samples (int or int64 tensor): the feature encoder's output
    length after the reflect pad of 2 x 40 samples; n_padded / 320 for every multiple of 1280."""
    from .extract_w2v import Wav2vec2
    return Wav2vec2.frames(n_padded + 2 * W2V_PAD)


def f0_samples(n_padded):
    """Converted log-F0 samples the vocoder reads for a padded source: 4 per w2v frame (= n_padded / 80)."""
    return 4 * w2v_frames(n_padded)


def mel_frames(n: int) -> int:
    """Valid frames of MelSpectrogramFixed (hop 320, last frame dropped) for a prompt of n samples."""
    return n // FRAME


def output_length(frames, output_sr: int = 16000):
    """Output samples of a row of ``frames`` vocoder frames at ``output_sr`` (SpeechSR: x1.5 / x3)."""
    n = frames * FRAME
    return n * output_sr // 16000 if output_sr in (24000, 48000) else n


def output_name(source_path, target_path) -> str:
    """inference_vc.py:164-166: '<source stem>_to_<target stem>.wav'."""
    stem = lambda p: os.path.splitext(os.path.basename(str(p)))[0]
    return f"{stem(source_path)}_to_{stem(target_path)}.wav"


def f0_path(wav_path) -> str:
    """Where extract_f0.py leaves the YAAPT track of a WAV file: 'x.wav' -> 'x.hf0.npy' (other names: + '.hf0.npy')."""
    root, ext = os.path.splitext(str(wav_path))
    return (root if ext.lower() == ".wav" else str(wav_path)) + ".hf0.npy"


def load_f0(wav_path) -> np.ndarray:
    """The track of ``wav_path`` from its '.hf0.npy' file (extract_f0.py: [n] or [1, n]) -> float32 [n].  A missing
    track is an error: the conversion has no F0 fallback."""
    p = f0_path(wav_path)
    if not os.path.exists(p):
        raise L.HspError(f"no F0 track for {wav_path}: expected {p} (written by the reference's extract_f0.py)")
    return np.asarray(np.load(p), dtype=np.float32).reshape(-1)


def group_prompts(targets, B: int):
    """``targets`` = one prompt (shared by every row) or a list of B prompts -> (distinct prompts, row -> index).
    Rows share a prompt when they hold the same object (``is``); every distinct prompt is encoded once."""
    if not isinstance(targets, (list, tuple)):
        return [targets], [0] * B
    if len(targets) == 1:
        return [targets[0]], [0] * B
    if len(targets) != B:
        raise L.HspError(f"vc_batch: give one prompt or one per source ({B}), got {len(targets)}")
    distinct, index = [], []
    for t in targets:
        for i, d in enumerate(distinct):
            if d is t:
                index.append(i)
                break
        else:
            index.append(len(distinct))
            distinct.append(t)
    return distinct, index


def length_groups(lengths):
    """Row indices grouped by equal padded source length, groups in order of first appearance: the equal-length batches
    of vc_batch_files(group_by_length=True)."""
    groups = {}
    for b, n in enumerate(lengths):
        groups.setdefault(int(n), []).append(b)
    return list(groups.values())


def check_batch(src_lengths, f0_src_lengths, trg_lengths, f0_trg_lengths):
    """Host-side checks of a batch (lengths in samples / track frames; trg_* per distinct prompt): sources padded by
    pad_source, every source track at least Ls / 80 frames long (the vocoder reads that many), every prompt track at
    least Lt / 80 long, every prompt long enough for the mel transform (> 640 samples)."""
    if len(src_lengths) != len(f0_src_lengths):
        raise L.HspError(f"vc_batch: {len(src_lengths)} sources but {len(f0_src_lengths)} source F0 tracks")
    if len(trg_lengths) != len(f0_trg_lengths):
        raise L.HspError(f"vc_batch: {len(trg_lengths)} prompts but {len(f0_trg_lengths)} prompt F0 tracks")
    for b, (n, nf) in enumerate(zip(src_lengths, f0_src_lengths)):
        if n <= 0 or n % SOURCE_HOP:
            raise L.HspError(f"vc_batch: source {b} has {n} samples; pad it with pad_source (a multiple of "
                             f"{SOURCE_HOP})")
        if nf < f0_samples(n):
            raise L.HspError(f"vc_batch: source {b}: F0 track of {nf} frames, needs >= {f0_samples(n)} "
                             f"(= {n} / {F0_HOP})")
    for p, (n, nf) in enumerate(zip(trg_lengths, f0_trg_lengths)):
        if n <= 640:
            raise L.HspError(f"vc_batch: prompt {p} has {n} samples; the mel transform needs more than 640")
        if nf < n // F0_HOP or nf <= 0:
            raise L.HspError(f"vc_batch: prompt {p}: F0 track of {nf} frames, needs >= {n // F0_HOP} "
                             f"(= {n} / {F0_HOP})")


# ---------------------------------------------------------------- batched conversion: device side
def _stage(name):
    if STAGE_HOOK is not None:
        STAGE_HOOK(name)


def _tap(name, t):
    if TAP_HOOK is not None:
        TAP_HOOK(name, t)


def _flat(x):
    return x.reshape(-1)


def _device_lengths(lengths, device):
    """int64 [B] on ``device`` from host ints; fills (no pageable host copy) while a graph is being captured."""
    if torch.cuda.is_current_stream_capturing():
        return torch.cat([torch.full((1,), int(n), dtype=torch.int64, device=device) for n in lengths])
    return torch.tensor([int(n) for n in lengths], dtype=torch.int64).to(device)


def _stack(rows, device, width=None):
    """Zero-padded [len(rows), width] fp32 copy of 1-D (or [1, n]) device rows -> (tensor, host lengths)."""
    lens = [_flat(r).shape[0] for r in rows]
    out = torch.zeros(len(rows), max(lens) if width is None else width, dtype=torch.float32, device=device)
    for i, r in enumerate(rows):
        out[i, :lens[i]].copy_(_flat(r))
    return out, lens


def _rows(arg, device, what):
    """A list of rows, or (padded [B, N] tensor, int64 [B] lengths) -> (padded, device lengths, host lengths or
    None)."""
    if isinstance(arg, tuple):
        x, n = arg
        if x.dim() != 2 or n.shape != (x.shape[0],):
            raise L.HspError(f"vc_batch: {what} as (padded [B, N], lengths [B]), got {tuple(x.shape)} / "
                             f"{tuple(n.shape)}")
        return x.to(torch.float32).contiguous(), n.to(device=device, dtype=torch.int64).contiguous(), None
    x, lens = _stack(list(arg), device)
    return x, _device_lengths(lens, device), lens


@torch.no_grad()
def denoise_prompts(prompts, denoiser, hps):
    """The denoised form of every prompt as inference_vc.py:117-133 makes it, for all of them in one
    ``denoiser.infer.denoise_batch``: zero-pad each prompt to the next multiple of 1600 samples (always at least one
    sample of padding, :117-119), denoise the padded prompts, cut to the padded length (:130) and to the prompt's own
    length (:133).  ``prompts``: 1-D or [1, n] fp32 device tensors; ``denoiser`` a finalized denoiser.generator.MPNet,
    ``hps`` its config.  Returns a list of 1-D tensors, the form ``vc_batch`` takes as ``denoised``."""
    from .denoiser.infer import denoise_batch
    rows = [_flat(p) for p in prompts]
    if not rows:
        raise L.HspError("denoise_prompts: no prompts")
    lens = [r.shape[0] for r in rows]
    padded_lens = [(n // 1600 + 1) * 1600 for n in lens]
    padded, _ = _stack(rows, rows[0].device, max(padded_lens))
    out, out_lens = denoise_batch(padded, denoiser, hps, lengths=padded_lens)
    # 1600 is a multiple of the denoiser's hop, so row b holds all padded_lens[b] samples
    assert all(o >= n for o, n in zip(out_lens, lens))
    return [out[b, :n] for b, n in enumerate(lens)]


@torch.no_grad()
def vc_batch(models: VcModels, mel_fn, sources, f0_srcs, targets, f0_trgs, *, noise=None, noise_scale_vc=0.333,
             denoise_ratio=0.0, denoised=None, output_sr=16000, scale_norm="max", return_float=False,
             row_exact=False, denoiser=None, hps_denoiser=None, target_lufs=-23.0, limiter=False, ceiling_db=-1.0,
             lookahead_ms=1.5, limiter_passes=2, return_stats=False, noise_seeds=None, pitch=None, return_lf0=False):
    """``vc`` for B sources in one pass.

    sources  B 16 kHz rows padded by pad_source ([Ls_b] or [1, Ls_b] device tensors), or (padded fp32 [B, Ls],
             int64 lengths [B]) -- the tensor form with device lengths keeps the call free of host read-backs, so a
             fixed shape can be captured in a hipGraph;
    f0_srcs  the B YAAPT tracks of the padded sources (>= Ls_b / 80 frames each), as a list or (padded, lengths);
    targets  one prompt [Lt] / [1, Lt] shared by every row, or a list of B prompts (rows holding the same tensor object
             share it: its mel and style vector are computed once, at its own length);
    f0_trgs  the prompts' tracks, in the same form as ``targets``;
    denoised the denoiser's output per prompt, in the same form as ``targets`` (None = the prompts themselves);
    denoiser / hps_denoiser  a finalized denoiser.generator.MPNet and its config: with ``denoise_ratio != 0`` and no
             ``denoised``, every distinct prompt is denoised here in one packed pass (``denoise_prompts``).  Giving
             both ``denoised`` and ``denoiser``, or ``denoise_ratio != 0`` with neither, is an error;
    noise    fp32 [B, 192, T_max] (T_max = Ls / 320), None = drawn;
    noise_seeds  an int s (row b draws its prior noise with s + b) or an int64 [B] tensor, instead of ``noise``: the
             seeded stream of ``vc(noise_seed=)``; with ``row_exact`` row b equals ``vc`` on it alone with its seed, and
             no noise tensor is built;
    scale_norm ... return_stats  the int16 stage, see `output.OutputStage`: every row over its own length, 'prompt'
             with the peak of the row's own prompt (taken on the device: no norm reads anything back to the host);
    pitch    a `prosody_controls.PitchEdit` whose per-row values are per source: every row's converted log-F0 track is
             edited over its own 4 T_b frames, as ``vc(pitch=)`` edits it (one launch; None or an identity edit: none);
    return_lf0  the tracks the vocoder was given, fp32 [B, 4 T_max] (row b: its first 4 T_b entries, zeros after), come
             last.

    Returns (wav int16 [B, n_max], lengths int64 [B] on the device): row b's valid samples are wav[b, :lengths[b]]
    (320 T_b at 16 kHz, x1.5 / x3 with SpeechSR), zeros after; with ``return_float`` also the float audio
    [B, 1, n_max].  Row b up to the vocoder equals ``vc`` on row b alone; the vocoder and SpeechSR run the ragged batch
    with per-row frame counts as ``tts`` does at B > 1.  ``row_exact``: the vocoder runs each row as
    at B = 1 too (key-masked flows, ragged activations, zeros past every row's end), so every row equals ``vc`` on it
    alone, at 16, 24 and 48 kHz."""
    stage = OutputStage(scale_norm, target_lufs, limiter, ceiling_db, lookahead_ms, limiter_passes,
                        return_stats).check()
    if noise_seeds is not None:
        Fh.check_noise_seeds(noise, noise_seeds, sources[0].shape[0] if isinstance(sources, tuple) else len(sources))
    pitch = PC.check_pitch(pitch, sources[0].shape[0] if isinstance(sources, tuple) else len(sources))
    voc = models.voc
    if denoised is not None and denoiser is not None:
        raise L.HspError("vc_batch: give the denoised prompts or a denoiser, not both")
    if denoise_ratio != 0 and denoised is None and denoiser is None:
        raise L.HspError("vc_batch: denoise_ratio != 0 needs the denoised prompts (denoised=) or a denoiser "
                         "(denoiser=, hps_denoiser=)")
    if denoiser is not None and hps_denoiser is None:
        raise L.HspError("vc_batch: a denoiser needs its config (hps_denoiser=)")
    dev = sources[0].device
    x, src_len, src_host = _rows(sources, dev, "sources")
    B, Ls = x.shape
    fs, fs_len, fs_host = _rows(f0_srcs, dev, "f0_srcs")
    if fs.shape[0] != B:
        raise L.HspError(f"vc_batch: {B} sources but {fs.shape[0]} source F0 tracks")
    prompts, index = group_prompts(targets, B)
    P = len(prompts)
    first = [index.index(p) for p in range(P)]                                 # a row of every distinct prompt

    def follow(arg, what):          # f0_trgs / denoised: the form of `targets`, one entry per distinct prompt
        if isinstance(arg, (list, tuple)) and len(arg) == B and B > 1:
            return [arg[first[p]] for p in range(P)]
        if isinstance(arg, (list, tuple)):
            if len(arg) != 1:
                raise L.HspError(f"vc_batch: {what} needs one entry or one per source ({B}), got {len(arg)}")
            arg = arg[0]
        if P != 1:
            raise L.HspError(f"vc_batch: {P} distinct prompts need {what} as a list of one entry per source")
        return [arg]

    p_tracks = follow(f0_trgs, "f0_trgs")
    if denoised is None and denoiser is not None and denoise_ratio != 0:
        seconds = denoise_prompts(prompts, denoiser, hps_denoiser)
    else:
        seconds = prompts if denoised is None else follow(denoised, "denoised")
    p_lens = [_flat(p).shape[0] for p in prompts]
    if src_host is not None and fs_host is not None:
        check_batch(src_host, fs_host, p_lens, [_flat(t).shape[0] for t in p_tracks])
    else:
        check_batch([], [], p_lens, [_flat(t).shape[0] for t in p_tracks])
        if Ls % SOURCE_HOP or fs.shape[1] < Ls // F0_HOP:
            raise L.HspError(f"vc_batch: padded sources [B, {Ls}] need Ls % {SOURCE_HOP} == 0 and tracks of >= "
                             f"{Ls // F0_HOP} columns, got {fs.shape[1]}")
    if output_sr in (24000, 48000):
        _sr_model(models)

    _stage("wav2vec2")
    # wav2vec2 hidden state 7 of every row at its own length (:85-86)
    y = Fh.reflect_pad_ragged(x, src_len, W2V_PAD)
    x_w2v = models.w2v(y, src_len + 2 * W2V_PAD)                              # [B, 1024, T_max]
    _tap("reflect_pad", y)
    _tap("w2v", x_w2v)
    T = x_w2v.shape[2]
    frames = w2v_frames(src_len)                                               # int64 [B]
    _stage("f0_mel_style")
    # F0 conversion per row (:80-81,104-105), zero past a row's 4 T_b samples
    if len(p_tracks) == 1:
        ft = _flat(p_tracks[0]).reshape(1, -1).to(torch.float32).contiguous()
        ft_len = torch.full((B,), ft.shape[1], dtype=torch.int64, device=dev)
    else:
        ft, ft_host = _stack([p_tracks[index[b]] for b in range(B)], dev)
        ft_len = _device_lengths(ft_host, dev)
    lf0 = Fh.f0_convert_batch(fs, fs_len, ft, ft_len)[:, :4 * T].reshape(B, 1, 4 * T)
    lf0 = Fh.mask_mul(lf0, Fh.sequence_mask(4 * frames, 4 * T))
    if pitch is not None:
        lf0 = pitch.apply(lf0.reshape(B, 4 * T), 4 * frames).reshape(B, 1, 4 * T)
    _tap("lf0", lf0)
    # one style vector per distinct prompt, at the prompt's own length (:113-126); the ragged mel covers them all
    pm, _ = _stack([r for p in range(P) for r in (prompts[p], seconds[p])], dev)
    pm_len = _device_lengths([n for n in p_lens for _ in range(2)], dev)
    for p in range(P):
        if _flat(seconds[p]).shape[0] < p_lens[p]:
            raise L.HspError(f"vc_batch: denoised prompt {p} is shorter than its prompt")
    mels, _ = mel_fn(pm, pm_len)          # [2P, 80, Tm_max]; a denoised row is read up to its prompt's length only
    styles = []
    for p in range(P):
        tm = mel_frames(p_lens[p])
        mel_p = Fh.copy_strided(mels[2 * p:2 * p + 2, :, :tm])
        _tap("mel", mel_p)
        styles.append(voc.style_vector(mel_p, torch.full((2,), tm, dtype=torch.int64, device=dev), denoise_ratio))
    style = styles[0].expand(B, -1, -1).contiguous() if P == 1 else torch.cat([styles[index[b]] for b in range(B)])
    _tap("style", style)
    _stage("vocoder")
    audio = voc.voice_conversion_noise_control(x_w2v, frames, None, None, lf0, noise_scale=noise_scale_vc,
                                               denoise_ratio=denoise_ratio, noise=noise, style=style,
                                               row_exact=row_exact, noise_seeds=noise_seeds)
    if output_sr in (24000, 48000):
        _stage("speechsr")
        if row_exact:                  # SpeechSR on the ragged rows, each as on its own (lengths at 16 kHz: 320 T_b)
            with hip_layers.row_exact(hip_layers.RowLengths(frames, audio.shape[2] // 320)):
                audio = models.sr(audio)                                       # :147-151
        else:
            audio = models.sr(audio)                                           # :147-151
    _stage("int16")
    n_valid = output_length(frames, output_sr)
    gain = 0.999
    if stage.scale_norm == "prompt":   # (:157-160) the peak of each row's own prompt, as a device fp32 [B]
        peaks = Fh.abs_max_rows(pm[0::2].contiguous(), pm_len[0::2].contiguous())
        gain = peaks.expand(B).contiguous() if P == 1 else torch.cat([peaks[index[b]:index[b] + 1] for b in range(B)])
    wav, stats = stage.int16(audio, n_valid, output_rate(output_sr), gain)
    _stage("end")
    return pack(wav, (n_valid, True), (audio, return_float), (stats, return_stats),
                (lf0.reshape(B, 4 * T), return_lf0))


@torch.no_grad()
def vc_batch_files(models: VcModels, mel_fn, source_paths, target_paths, out_dir=None, f0=None, device=None,
                   group_by_length: Optional[bool] = None, pitch=None, return_lf0=False, **kw):
    """The reference's per-file loop (inference_vc.py:70-170, one process call per file) as batches: every source and
    prompt WAV at any sample rate (``audio.load_16k``; sources padded by pad_source), F0 tracks from ``f0`` (a mapping
    path -> track) or else from the '.hf0.npy' file extract_f0.py writes beside each WAV (a missing track is an error
    naming the file), ``vc_batch`` calls (keywords ``kw``; ``noise`` [B, 192, T_max] and ``noise_seeds`` -- an int s:
    source b draws with s + b; or an int64 [B] tensor -- are indexed by ``source_paths`` and sliced per batch;
    ``denoiser=`` and ``hps_denoiser=`` with ``denoise_ratio != 0`` denoise every distinct prompt file of a batch in one
    packed pass, the reference harness's step :117-133), and with ``out_dir`` one '<src>_to_<trg>.wav' per row at the output rate.
    ``target_paths``: one prompt file for every source, or one per source.

    ``group_by_length`` True: one vc_batch call per padded source length (`length_groups`), so every batch has equal
    rows and each output matches the one-file conversion (contract item 2).  False: ONE ragged batch,
    faster, but every row shorter than the longest differs from its one-file conversion over its whole length (the
    flows' attention sees the batch's padding; contract item 3).  None (the default): True, unless ``row_exact=True``
    is given -- then ONE ragged batch whose rows each match their one-file conversion.
    The fields of `output.OutputStage` go to ``vc_batch`` with ``kw``; ``return_stats=True`` appends the limiter's
    per-row stats (fp32 [B] tensors in the order of ``source_paths``).  ``pitch`` (a `prosody_controls.PitchEdit`,
    per-row values in the order of ``source_paths``) is sliced per batch; ``return_lf0`` appends the vocoder's log-F0
    tracks, fp32 [B, 4 T_max], last.
    Returns (wav int16 [B, n_max], lengths int64 [B] on the device); the files hold wav[b, :lengths[b]]."""
    from .audio import load_16k
    from .inference_plm import write_wav
    return_stats = OutputStage.of(kw).check().return_stats                  # before any file is read
    Fh.check_noise_seeds(kw.get("noise"), kw.get("noise_seeds"), len(source_paths))
    if pitch is not None:
        PC.check_pitch(pitch, len(source_paths))
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    source_paths = [str(p) for p in source_paths]
    B = len(source_paths)
    per_row = isinstance(target_paths, (list, tuple))
    trg_paths = [str(p) for p in target_paths] if per_row else [str(target_paths)] * B
    if len(trg_paths) != B:
        raise L.HspError(f"vc_batch_files: give one prompt file or one per source ({B}), got {len(trg_paths)}")
    if kw.get("return_float"):
        raise L.HspError("vc_batch_files returns int16 rows only (use vc_batch for the float audio)")
    f0 = {} if f0 is None else {str(k): v for k, v in f0.items()}
    if group_by_length is None:
        group_by_length = not kw.get("row_exact", False)

    def track(path):
        t = f0[path] if path in f0 else load_f0(path)
        return torch.as_tensor(np.asarray(t, dtype=np.float32).reshape(-1)).to(device)

    sources = [load_source(p, device) for p in source_paths]
    prompts, tracks = {}, {}
    for p in dict.fromkeys(trg_paths):                                      # each distinct prompt file loaded once
        prompts[p], tracks[p] = load_16k(p, device), track(p)
    f0_srcs = [track(p) for p in source_paths]
    groups = length_groups([s.shape[-1] for s in sources]) if group_by_length else [list(range(B))]
    noise = kw.pop("noise", None)
    seeds = kw.pop("noise_seeds", None)
    if seeds is not None:                                                   # one seed per file, whatever batch it joins
        seeds = Fh.row_seeds(seeds, B, "cpu")
    parts, part_stats, part_lf0 = [], [], []
    for rows in groups:
        T = max(sources[b].shape[-1] for b in rows) // FRAME
        nz = None if noise is None else noise[torch.tensor(rows, device=noise.device), :, :T].contiguous()
        sd = None if seeds is None else seeds[torch.tensor(rows)]
        parts.append(vc_batch(models, mel_fn, [sources[b] for b in rows], [f0_srcs[b] for b in rows],
                              [prompts[trg_paths[b]] for b in rows], [tracks[trg_paths[b]] for b in rows], noise=nz,
                              noise_seeds=sd, pitch=None if pitch is None else pitch.rows(rows), return_lf0=return_lf0,
                              **kw))
        if return_lf0:
            part_lf0.append(parts[-1][-1])
        if return_stats:
            part_stats.append(parts[-1][2])
        parts[-1] = parts[-1][:2]
    stats = None
    if return_stats:
        order = torch.tensor([b for rows in groups for b in rows], device=device).argsort()
        stats = {k: torch.cat([ps[k] for ps in part_stats])[order] for k in part_stats[0]}
    if len(groups) == 1:
        wav, lengths = parts[0]
    else:
        wav = torch.zeros(B, max(w.shape[1] for w, _ in parts), dtype=torch.int16, device=device)
        lengths = torch.zeros(B, dtype=torch.int64, device=device)
        for rows, (w, n) in zip(groups, parts):
            idx = torch.tensor(rows, device=device)
            wav[idx, :w.shape[1]] = w
            lengths[idx] = n
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        rate = output_rate(kw.get("output_sr", 16000))
        n = lengths.cpu().tolist()
        host = wav.cpu()
        for b in range(B):
            write_wav(os.path.join(str(out_dir), output_name(source_paths[b], trg_paths[b])), rate, host[b, :n[b]])
    tracks = None
    if return_lf0:
        tracks = torch.zeros(B, max(t.shape[1] for t in part_lf0), dtype=torch.float32, device=device)
        for rows, t in zip(groups, part_lf0):
            tracks[torch.tensor(rows, device=device), :t.shape[1]] = t
    return pack(wav, (lengths, True), (stats, return_stats), (tracks, return_lf0))
