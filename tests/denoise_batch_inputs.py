"""The four prompts of the batched-denoiser tests (no tests here): two synthetic rows below every T dilation / across
dilation 8, and the ``wav`` of the two denoiser golden fixtures, which share one state dict."""
import numpy as np

import helpers as H

LENGTHS = [300, 900, 8000, 14400]            # T = 1 + L // 100 = 4, 10, 81, 145 frames
FIXTURES = {8000: "denoise_l8000", 14400: "denoise_l14400"}


def tone_row(n, seed):
    """Seeded tones plus noise, peak <= 0.5, never silent."""
    r = np.random.default_rng(seed)
    t = np.arange(n)
    x = 0.2 * np.sin(t * r.uniform(0.03, 0.09)) + 0.15 * np.sin(t * r.uniform(0.2, 0.5) + 1.0) + 0.03 * r.standard_normal(n)
    return np.clip(x, -0.5, 0.5).astype(np.float32)


def row(n):
    return H.load_fixture(FIXTURES[n])[1]["wav"] if n in FIXTURES else tone_row(n, n)


def rows():
    return [row(n) for n in LENGTHS]


def solid(mag):
    """Bins whose phase is well conditioned: magnitude above 1e-3 of the peak."""
    return mag > 1e-3 * mag.max()


def circular(a, b):
    return np.abs(np.angle(np.exp(1j * (a.astype(np.float64) - b.astype(np.float64)))))


# ------------------------------------------------------------------ the voice-conversion side of the wiring tests
def speech(n, seed, sr=16000):
    """Harmonics of a gliding pitch plus a noise floor, |x| < 1."""
    r = np.random.default_rng(seed)
    t = np.arange(n) / sr
    ph = 2 * np.pi * np.cumsum(110.0 + 30.0 * np.sin(2 * np.pi * 0.9 * t + seed)) / sr
    x = sum(np.sin(k * ph) / k for k in range(1, 6)) * (0.4 + 0.6 * np.sin(2 * np.pi * 1.7 * t + seed) ** 2)
    x = 0.3 * x + 0.02 * r.standard_normal(n)
    return (0.9 * x / np.abs(x).max()).astype(np.float32)


def track(n, seed, lo=90.0, hi=300.0):
    """A YAAPT-like F0 track: 30 % unvoiced frames."""
    r = np.random.default_rng(seed)
    return np.where(r.random(n) < 0.3, 0, r.uniform(lo, hi, n)).astype(np.float32)


def vc_models(device):
    """(VcModels with synthetic weights, the 80-bin mel front-end), finalized on ``device``."""
    import torch
    from megatts2_hierspeechpp_amd import inference_vc as IV, synth
    from megatts2_hierspeechpp_amd.Mels_preprocess import MelSpectrogramFixed
    from oracle.hsp_oracle import default_config
    models = IV.VcModels(default_config())
    models.load_state_dict({k: torch.from_numpy(synth.synth_tensor(k, tuple(v.shape), 2))
                            for k, v in models.state_dict().items()})
    models.finalize(device)
    mel_fn = MelSpectrogramFixed(sample_rate=16000, n_fft=1280, win_length=1280, hop_length=320, f_min=0, f_max=8000,
                                 n_mels=80, window_fn=torch.hann_window).finalize(device)
    return models, mel_fn


def vc_case(device, raw, prompt_lens, seed):
    """Padded sources, their tracks, prompts and the prompts' tracks as device tensors."""
    import torch
    from megatts2_hierspeechpp_amd import inference_vc as IV
    d = lambda a: torch.from_numpy(a).to(device)
    srcs = [IV.pad_source(d(speech(n, seed + b)).reshape(1, -1)) for b, n in enumerate(raw)]
    f0s = [d(track(s.shape[-1] // 80 + 1, seed + 50 + b)) for b, s in enumerate(srcs)]
    prompts = [d(speech(n, seed + 80 + i)).reshape(1, -1) for i, n in enumerate(prompt_lens)]
    f0t = [d(track(n // 80, seed + 90 + i, lo=150, hi=350)) for i, n in enumerate(prompt_lens)]
    return srcs, f0s, prompts, f0t
