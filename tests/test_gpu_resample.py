"""GPU (-m gpu): functional.resample (hsp_resample_f32) against a float64 restatement of torchaudio 0.13.1's sinc
resampler, against an analytic band-limited sine, under graph capture, and through the file-in harnesses
(inference_plm.tts_from_prompt_file, inference_speechsr.super_resolution, inference_vc.vc with scale_norm='prompt').

torchaudio is not available here: the restatement below is the formula of _get_sinc_resample_kernel /
_apply_sinc_resample_kernel written out, and the sine test checks that it is a correct resampler."""
import math

import numpy as np
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu

RATE_PAIRS = [(f, 16000) for f in (44100, 48000, 22050, 24000, 32000, 8000, 11025, 96000)] + [(16000, 24000),
                                                                                              (16000, 48000)]
METHODS = ["sinc_interpolation", "kaiser_window"]
_BANKS = {}


def ref_bank(orig, new, method, lpw=6, rolloff=0.99):
    """torchaudio 0.13.1 _get_sinc_resample_kernel in float64 (p / n formed in fp32): (o, n, width, bank [n, K])."""
    key = (orig, new, method)
    if key not in _BANKS:
        g = math.gcd(orig, new)
        o, n = orig // g, new // g
        base = min(o, n) * rolloff
        width = math.ceil(lpw * o / base)
        K = 2 * width + o
        pn = (-np.arange(n).astype(np.float32) / np.float32(n)).astype(np.float64)
        t = np.clip(((np.arange(K)[None, :] - width) / o + pn[:, None]) * base, -lpw, lpw)
        if method == "kaiser_window":
            beta = 14.769656459379492
            w = np.i0(beta * np.sqrt(1 - (t / lpw) ** 2)) / np.i0(beta)
        else:
            w = np.cos(t * math.pi / lpw / 2) ** 2
        with np.errstate(invalid="ignore", divide="ignore"):
            s = np.where(t == 0, 1.0, np.sin(math.pi * t) / (math.pi * t))
        _BANKS[key] = (o, n, width, s * w * base / o)
    return _BANKS[key]


def ref_resample(x, orig, new, method):
    """_apply_sinc_resample_kernel in float64 on one row: pad (width, width + o), strided correlation, cut to
    ceil(n L / o)."""
    o, n, width, bank = ref_bank(orig, new, method)
    K = bank.shape[1]
    Lx = x.shape[0]
    frames = Lx // o + 1
    xp = np.zeros(width + frames * o + K)
    xp[width:width + Lx] = x
    win = np.lib.stride_tricks.sliding_window_view(xp, K)[::o][:frames]
    return (win @ bank.T).reshape(-1)[:math.ceil(n * Lx / o)]


def signal(B, L, sr, seed):
    """Harmonic stack + noise floor (the recipe of the prompt tests of test_gpu_parity.py, at rate sr), |x| < 1."""
    rng = np.random.default_rng(seed)
    t = np.arange(L) / float(sr)
    f0 = rng.uniform(90, 300, (B, 1))
    voiced = sum(np.sin(2 * np.pi * f0 * h * t) / h for h in range(1, 12))
    env = 0.5 + 0.5 * np.sin(2 * np.pi * 2.5 * t)
    return (0.15 * voiced * env + 0.02 * rng.standard_normal((B, L))).astype(np.float32)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("orig,new", RATE_PAIRS)
def test_resample_matches_float64_restatement(orig, new, method, device):
    from megatts2_hierspeechpp_amd import functional as F
    o, n, width, bank = ref_bank(orig, new, method)
    K = bank.shape[1]
    worst = 0.0
    for L in sorted({1, K - 1, 7 * o + 3 if o > 1 else 1001, 10 * orig}):
        for B in (1, 3):
            x = signal(B, L, orig, seed=L + B)
            lens = [L, max(1, L // 2), max(1, L - o - 1)][:B]
            xt = torch.from_numpy(x).to(device)
            y = F.resample(xt, orig, new, resampling_method=method,
                           lengths=torch.tensor(lens, device=device) if B > 1 else None)
            T = math.ceil(n * L / o)
            assert y.shape == (B, T) and y.dtype == torch.float32
            yh = y.cpu().numpy()
            for b in range(B):
                Tb = math.ceil(n * lens[b] / o)
                want = ref_resample(x[b, :lens[b]].astype(np.float64), orig, new, method)
                assert want.shape == (Tb,)
                err = float(np.abs(yh[b, :Tb] - want).max())
                worst = max(worst, err)
                assert err <= 1e-5, (orig, new, method, L, B, b, err)
                assert not yh[b, Tb:].any(), "samples past T_b must be zero"
    print(f"resample {orig}->{new} {method}: max|gpu - float64| = {worst:.2e}")
    x = torch.from_numpy(signal(2, 100, orig, 1)).to(device)
    assert F.resample(x, orig, orig) is x                                     # equal rates: the input itself


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("orig", [44100, 48000])
def test_resample_band_limited_sine(orig, method, device):
    from megatts2_hierspeechpp_amd import functional as F
    L = orig // 2
    x = np.sin(2 * np.pi * 1000.0 * np.arange(L) / orig)
    y = F.resample(torch.from_numpy(x.astype(np.float32)).to(device), orig, 16000, resampling_method=method)
    y = y.cpu().numpy().astype(np.float64)
    ref = ref_resample(x, orig, 16000, method)
    exact = np.sin(2 * np.pi * 1000.0 * np.arange(ref.shape[0]) / 16000)
    w = ref_bank(orig, 16000, method)[2]
    mid = slice(w, ref.shape[0] - w)
    ref_err = float(np.abs(ref[mid] - exact[mid]).max())
    gpu_err = float(np.abs(y[mid] - exact[mid]).max())
    assert ref_err < 5e-3, ref_err                                            # the restatement is a resampler
    assert gpu_err <= ref_err + 1e-5, (gpu_err, ref_err)


def test_resample_graph_capture_replays_bit_identical(device):
    from megatts2_hierspeechpp_amd import functional as F
    x = torch.from_numpy(signal(2, 44100, 44100, 3)).to(device)
    eager = F.resample(x, 44100, 16000, resampling_method="kaiser_window")   # uploads the bank outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = F.resample(x, 44100, 16000, resampling_method="kaiser_window")
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


# ------------------------------------------------------------------ the file-in harnesses
def _write_float_wav(path, rate, x):
    from scipy.io import wavfile
    wavfile.write(path, rate, x.astype(np.float32))                          # float32 WAV: read back exactly


def _tts_setup(device):
    from megatts2_hierspeechpp_amd import inference_plm as IP, synth
    from oracle.hsp_oracle import default_config
    models = IP.TtsModels(default_config(), H.TTV_MODEL)
    models.load_state_dict({k: torch.from_numpy(synth.synth_tensor(k, tuple(v.shape), 7)) for k, v in models.state_dict().items()})
    models.finalize(device)
    return models


def _mel_fn(device):
    from megatts2_hierspeechpp_amd.Mels_preprocess import MelSpectrogramFixed
    return MelSpectrogramFixed(sample_rate=16000, n_fft=1280, win_length=1280, hop_length=320, f_min=0, f_max=8000,
                               n_mels=80, window_fn=torch.hann_window).finalize(device)


def test_tts_from_prompt_file_at_44k(device, tmp_path):
    """A 44.1 kHz prompt file through tts_from_prompt_file equals tts_from_prompt fed with functional.resample of the
    same samples; scale_norm='prompt' keeps the float audio and scales the int16 output by the prompt's peak.  The
    prompt's peak is below 1: a prompt resampled above full scale is outside the contract (the reference's
    astype('int16') wraps there)."""
    from megatts2_hierspeechpp_amd import functional as F, inference_plm as IP
    models, mel_fn = _tts_setup(device), _mel_fn(device)
    r = np.random.default_rng(5)
    N = 7
    ids = torch.from_numpy(r.integers(12, 113, (1, N))).to(device)
    tone = torch.from_numpy(r.integers(0, 11, (1, N))).to(device)
    lang = torch.where(ids < 74, 1, 2)
    dur = torch.full((1, N), 4.0, device=device)
    noise = torch.from_numpy(r.standard_normal((1, 192, N * 2)).astype(np.float32)).to(device)
    x44 = signal(1, 55125, 44100, 11)
    assert np.abs(x44).max() < 1
    path = tmp_path / "prompt44k.wav"
    _write_float_wav(path, 44100, x44[0])
    kw = dict(dur=dur, noise=noise)
    wav = IP.tts_from_prompt_file(models, mel_fn, ids, tone, lang, path, output_path=tmp_path / "out.wav", **kw)
    p16 = F.resample(torch.from_numpy(x44).to(device), 44100, 16000, resampling_method="kaiser_window")
    assert p16.shape == (1, 20000)
    want = IP.tts_from_prompt(models, mel_fn, ids, tone, lang, p16, **kw)
    assert wav.dtype == torch.int16 and wav.shape == (N * 2 * 320,) and torch.equal(wav, want)
    w_max, a_max = IP.tts_from_prompt_file(models, mel_fn, ids, tone, lang, path, return_float=True, **kw)
    w_pr, a_pr = IP.tts_from_prompt_file(models, mel_fn, ids, tone, lang, path, scale_norm="prompt", return_float=True,
                                         **kw)
    assert torch.equal(w_max, wav) and torch.equal(a_pr, a_max)
    peak = float(p16.abs().max())
    assert 0 < peak < 1
    assert torch.equal(w_pr, IP.peak_int16(a_pr.reshape(1, -1), gain=peak).reshape(-1))
    assert not torch.equal(w_pr, w_max)


def test_super_resolution_from_22k_file(device, tmp_path):
    from scipy.io import wavfile
    from megatts2_hierspeechpp_amd import audio, functional as F, synth
    from megatts2_hierspeechpp_amd.hip_layers import finalize
    from megatts2_hierspeechpp_amd.inference_plm import peak_int16
    from megatts2_hierspeechpp_amd.inference_speechsr import super_resolution
    from megatts2_hierspeechpp_amd.speechsr48k.speechsr import SynthesizerTrn as SpeechSR
    sr = SpeechSR(128, 30, "0", [3, 7, 11], [[1, 3, 5]] * 3, [3], 32, [3])
    sr.load_state_dict({k: torch.from_numpy(synth.synth_tensor("sr." + k, tuple(v.shape), 0)) for k, v in sr.state_dict().items()})
    finalize(sr, device)
    x22 = np.concatenate([signal(1, 22050, 22050, 4), signal(1, 22050, 22050, 5)], 0)   # stereo: channel 0 is kept
    path = tmp_path / "in22k.wav"
    _write_float_wav(path, 22050, x22.T)
    a, rate = audio.load(path)
    assert rate == 22050 and a.shape == (2, 22050)
    out = tmp_path / "out48k.wav"
    wav = super_resolution(sr, a.to(device), rate, output_sr=48000, output_path=out)
    p16 = F.resample(torch.from_numpy(x22[:1]).to(device), 22050, 16000, resampling_method="kaiser_window")
    assert p16.shape == (1, 16000)
    want = peak_int16(sr(p16.unsqueeze(1)).reshape(1, -1)).reshape(-1)
    assert wav.dtype == torch.int16 and wav.shape == (48000,) and torch.equal(wav, want)
    rate_out, back = wavfile.read(out)
    assert rate_out == 48000 and np.array_equal(back, wav.cpu().numpy())
    assert torch.equal(audio.load_16k(path, device), p16)


def test_vc_scale_norm_prompt(device):
    from megatts2_hierspeechpp_amd import inference_vc as IV, synth
    from megatts2_hierspeechpp_amd.inference_plm import peak_int16
    from oracle.hsp_oracle import default_config
    models = IV.VcModels(default_config())
    models.load_state_dict({k: torch.from_numpy(synth.synth_tensor(k, tuple(v.shape), 2)) for k, v in models.state_dict().items()})
    models.finalize(device)
    mel_fn = _mel_fn(device)
    src = IV.pad_source(torch.from_numpy(signal(1, 12000, 16000, 5)).to(device))
    trg = torch.from_numpy(signal(1, 9000, 16000, 6)).to(device)
    rng = np.random.default_rng(8)
    f0s = torch.from_numpy(np.where(rng.random((1, 160)) < 0.3, 0, rng.uniform(90, 300, (1, 160))).astype(np.float32)).to(device)
    f0t = torch.from_numpy(np.where(rng.random((1, 112)) < 0.3, 0, rng.uniform(150, 350, (1, 112))).astype(np.float32)).to(device)
    noise = torch.randn(1, 192, 40, device=device)
    w_max, a_max = IV.vc(models, mel_fn, src, f0s, trg, f0t, noise=noise, return_float=True)
    w_pr, a_pr = IV.vc(models, mel_fn, src, f0s, trg, f0t, noise=noise, return_float=True, scale_norm="prompt")
    assert torch.equal(a_pr, a_max)
    peak = float(trg.abs().max())
    assert 0 < peak < 1
    assert torch.equal(w_pr, peak_int16(a_pr.reshape(1, -1), gain=peak).reshape(-1))
    assert torch.equal(w_max, peak_int16(a_max.reshape(1, -1)).reshape(-1))
