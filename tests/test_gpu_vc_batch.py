"""GPU (-m gpu): batched voice conversion.  The per-row-length entry points of include/hsp.h against NumPy / torch
restatements at ragged lengths, the ragged prompt mel and wav2vec2 against per-row calls, and inference_vc.vc_batch /
vc_batch_files against the parity contract of DESIGN.md §4.5 (row b is held to vc() on row b alone)."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

pytestmark = pytest.mark.gpu


def _speech(n, seed, sr=16000):
    """harmonics of a gliding pitch + a noise floor, |x| < 1"""
    r = np.random.default_rng(seed)
    t = np.arange(n) / sr
    ph = 2 * np.pi * np.cumsum(110.0 + 30.0 * np.sin(2 * np.pi * 0.9 * t + seed)) / sr
    x = sum(np.sin(k * ph) / k for k in range(1, 6)) * (0.4 + 0.6 * np.sin(2 * np.pi * 1.7 * t + seed) ** 2)
    x = 0.3 * x + 0.02 * r.standard_normal(n)
    return (0.9 * x / np.abs(x).max()).astype(np.float32)


def _track(n, seed, p_unvoiced=0.3, lo=90.0, hi=300.0):
    r = np.random.default_rng(seed)
    return np.where(r.random(n) < p_unvoiced, 0, r.uniform(lo, hi, n)).astype(np.float32)


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


@pytest.fixture(scope="module")
def vc_setup(device):
    from megatts2_hierspeechpp_amd import inference_vc as IV, synth
    from megatts2_hierspeechpp_amd.Mels_preprocess import MelSpectrogramFixed
    from megatts2_hierspeechpp_amd.speechsr48k.speechsr import SynthesizerTrn as SpeechSR
    from oracle.hsp_oracle import default_config
    models = IV.VcModels(default_config(), speechsr=SpeechSR(128, 30, "0", [3, 7, 11], [[1, 3, 5]] * 3, [3], 32, [3]))
    models.load_state_dict({k: torch.from_numpy(synth.synth_tensor(k, tuple(v.shape), 2))
                            for k, v in models.state_dict().items()})
    models.finalize(device)
    mel_fn = MelSpectrogramFixed(sample_rate=16000, n_fft=1280, win_length=1280, hop_length=320, f_min=0, f_max=8000,
                                 n_mels=80, window_fn=torch.hann_window).finalize(device)
    return models, mel_fn


# ---------------------------------------------------------------------------------------------- entry points
@pytest.mark.parametrize("B", [1, 5, 64])
def test_reflect_pad_ragged_bitwise(device, B):
    from megatts2_hierspeechpp_amd import functional as Fh
    r = np.random.default_rng(B)
    Lmax, pad = 3001, 40
    lens = r.integers(pad + 1, Lmax + 1, B)
    lens[0] = Lmax
    if B > 1:
        lens[1] = pad + 1
        lens[-1] = 1281
    x = torch.from_numpy(r.standard_normal((B, Lmax)).astype(np.float32))
    y = Fh.reflect_pad_ragged(x.to(device), torch.from_numpy(lens).to(device), pad).cpu()
    assert y.shape == (B, Lmax + 2 * pad)
    for b, n in enumerate(lens):
        want = TF.pad(x[b:b + 1, :n], (pad, pad), mode="reflect")[0]
        assert torch.equal(y[b, :n + 2 * pad], want), b
        assert not y[b, n + 2 * pad:].any()


@pytest.mark.parametrize("B,shared", [(9, True), (9, False), (64, False)])
def test_f0_convert_batch_bitwise_per_row(device, B, shared):
    from megatts2_hierspeechpp_amd import functional as Fh
    r = np.random.default_rng(B + shared)
    N = 1601
    n_src = r.integers(1, N + 1, B)
    n_src[0] = N
    src = np.zeros((B, N), np.float32)
    for b in range(B):
        src[b, :n_src[b]] = _track(n_src[b], 100 + b)
    src[1 % B] = 0.0                                          # an all-unvoiced source row
    nt = r.integers(1, 801, 1 if shared else B)
    trg = np.zeros((len(nt), 800), np.float32)
    for i, n in enumerate(nt):
        trg[i, :n] = _track(n, 300 + i, lo=150, hi=350)
    if not shared:
        trg[2] = 0.0                                          # an all-unvoiced prompt track
    s, t = torch.from_numpy(src).to(device), torch.from_numpy(trg).to(device)
    n_trg = np.broadcast_to(nt, (B,)) if shared else nt
    out = Fh.f0_convert_batch(s, torch.from_numpy(n_src).to(device), t, torch.from_numpy(np.array(n_trg)).to(device))
    for b in range(B):
        tb = t[0 if shared else b, :n_trg[b]]
        want = Fh.f0_convert(s[b:b + 1, :n_src[b]], tb.reshape(1, -1))
        assert torch.equal(out[b:b + 1, :n_src[b]], want), b
        assert not out[b, n_src[b]:].any()
    assert not out[1 % B].any()


def test_row_peak_and_per_row_gain_int16(device):
    from megatts2_hierspeechpp_amd import functional as Fh
    from megatts2_hierspeechpp_amd.inference_plm import peak_int16
    r = np.random.default_rng(4)
    B, n = 33, 5000
    x = torch.from_numpy(r.standard_normal((B, n)).astype(np.float32)).to(device)
    lens = torch.from_numpy(r.integers(1, n + 1, B)).to(device)
    lens[0] = n
    peaks = Fh.abs_max_rows(x, lens)
    gains = torch.from_numpy(r.uniform(0.1, 1.0, B).astype(np.float32)).to(device)
    wav = Fh.peak_int16_gains(x, lens, gains)
    for b in range(B):
        nb = int(lens[b])
        assert float(peaks[b]) == float(x[b, :nb].abs().max())
        want = peak_int16(x[b:b + 1], lens[b:b + 1], float(gains[b]))
        assert torch.equal(wav[b:b + 1], want), b
    assert torch.equal(Fh.abs_max_rows(x), x.abs().amax(1))


def test_ragged_prompt_mel_matches_per_row_calls(device, vc_setup):
    _, mel_fn = vc_setup
    lens = [641, 959, 48000, 30001, 12345, 960]
    B, Lmax = len(lens), max(lens)
    x = torch.zeros(B, Lmax, device=device)
    for b, n in enumerate(lens):
        x[b, :n] = torch.from_numpy(_speech(n, 20 + b)).to(device)
    x[1, lens[1]:] = 0.7                                      # garbage past a row's length must not leak in
    mels, mlen = mel_fn(x, torch.tensor(lens, device=device))
    assert mels.shape == (B, 80, Lmax // 320) and mlen.tolist() == [n // 320 for n in lens]
    for b, n in enumerate(lens):
        solo = mel_fn(x[b:b + 1, :n].contiguous())
        assert solo.shape[2] == n // 320
        assert _rel(mels[b:b + 1, :, :n // 320], solo) <= 1e-5, b


def test_wav2vec2_lengths_match_solo_rows(device, vc_setup):
    from megatts2_hierspeechpp_amd import functional as Fh
    models, _ = vc_setup
    frames = [400, 40, 123, 256]
    lens = [320 * T for T in frames]                          # padded-source lengths (123: not a 1280 multiple)
    B, Lmax = len(lens), max(lens)
    x = torch.zeros(B, Lmax, device=device)
    for b, n in enumerate(lens):
        x[b, :n] = torch.from_numpy(_speech(n, 40 + b)).to(device)
    ln = torch.tensor(lens, device=device)
    h = models.w2v(Fh.reflect_pad_ragged(x, ln, 40), ln + 80)
    assert h.shape == (B, 1024, max(frames))
    for b, n in enumerate(lens):
        solo = models.w2v(Fh.reflect_pad(x[b:b + 1, :n].contiguous(), 40))
        assert solo.shape == (1, 1024, frames[b])
        assert _rel(h[b:b + 1, :, :frames[b]], solo) <= 1e-5, (b, _rel(h[b:b + 1, :, :frames[b]], solo))


# ---------------------------------------------------------------------------------------------- vc_batch
def _case(device, raw, prompt_lens, seed):
    from megatts2_hierspeechpp_amd import inference_vc as IV
    srcs = [IV.pad_source(torch.from_numpy(_speech(n, seed + b)).to(device).reshape(1, -1)) for b, n in enumerate(raw)]
    f0s = [torch.from_numpy(_track(s.shape[-1] // 80 + 1, seed + 50 + b)).to(device) for b, s in enumerate(srcs)]
    prompts = [torch.from_numpy(_speech(n, seed + 80 + i)).to(device).reshape(1, -1) for i, n in enumerate(prompt_lens)]
    f0t = [torch.from_numpy(_track(n // 80, seed + 90 + i, lo=150, hi=350)).to(device) for i, n in enumerate(prompt_lens)]
    return srcs, f0s, prompts, f0t


def test_vc_batch_ragged_contract(device, vc_setup):
    """B = 3 ragged sources, two distinct prompts (rows 0 and 2 share one): items 1, 3 and 4 of the contract, item 1 on
    vc_batch's own intermediates (inference_vc.TAP_HOOK)."""
    from megatts2_hierspeechpp_amd import functional as Fh, inference_vc as IV
    from megatts2_hierspeechpp_amd.inference_plm import peak_int16
    models, mel_fn = vc_setup
    srcs, f0s, prompts, f0t = _case(device, [12000, 30000, 5000], [40000, 23456], 7)
    rows_p, rows_t = [prompts[0], prompts[1], prompts[0]], [f0t[0], f0t[1], f0t[0]]
    T = [s.shape[-1] // 320 for s in srcs]
    noise = torch.from_numpy(np.random.default_rng(3).standard_normal((3, 192, max(T))).astype(np.float32)).to(device)
    taps = {}
    IV.TAP_HOOK = lambda name, t: taps.setdefault(name, []).append(t.clone())
    try:
        wav, n_out, audio = IV.vc_batch(models, mel_fn, srcs, f0s, rows_p, rows_t, noise=noise, scale_norm="prompt",
                                        return_float=True)
    finally:
        IV.TAP_HOOK = None
    assert wav.dtype == torch.int16 and wav.shape == (3, 320 * max(T)) and n_out.tolist() == [320 * t for t in T]
    # item 1: every piece before the vocoder, row by row against the solo path (the pieces of vc())
    y, w2v, lf0, style = taps["reflect_pad"][0], taps["w2v"][0], taps["lf0"][0], taps["style"][0]
    assert lf0.shape == (3, 1, 4 * max(T)) and style.shape == (3, 256, 1) and len(taps["mel"]) == 2
    for b in range(3):
        n = srcs[b].shape[-1]
        assert torch.equal(y[b:b + 1, :n + 80], Fh.reflect_pad(srcs[b], 40)) and not y[b, n + 80:].any()
        solo = models.w2v(Fh.reflect_pad(srcs[b], 40))
        assert _rel(w2v[b:b + 1, :, :T[b]], solo) <= 1e-5, b
        want_f0 = Fh.f0_convert(f0s[b].reshape(1, -1), rows_t[b].reshape(1, -1))[:, :4 * T[b]]
        assert torch.equal(lf0[b, :, :4 * T[b]], want_f0) and not lf0[b, :, 4 * T[b]:].any(), b
    solo_style = []
    for p in range(2):
        m = mel_fn(torch.cat([prompts[p], prompts[p]], 0))
        assert taps["mel"][p].shape == m.shape and _rel(taps["mel"][p], m) <= 1e-5, p
        solo_style.append(models.voc.style_vector(m, torch.full((2,), m.shape[2], device=device)))
    for b, p in enumerate([0, 1, 0]):
        assert _rel(style[b:b + 1], solo_style[p]) <= 1e-5, b
    # item 3: the float rows are voice_conversion_noise_control on the stacked inputs
    want = models.voc.voice_conversion_noise_control(w2v, torch.tensor(T, device=device), None, None, lf0,
                                                     noise=noise, style=style)
    assert torch.equal(audio, want)
    # item 4: each int16 row is the per-row-gain conversion of its float row, with its own prompt's peak
    for b in range(3):
        n = 320 * T[b]
        peak = float(rows_p[b].abs().max())
        assert torch.equal(wav[b:b + 1, :n], peak_int16(audio[b:b + 1, :, :n].reshape(1, -1), gain=peak))
        assert not wav[b, n:].any()


def test_vc_batch_equal_length_rows_match_solo_vc(device, vc_setup):
    """B = 8 equal-length sources sharing one prompt: every float row within 1e-4 of its peak of vc() on that row."""
    from megatts2_hierspeechpp_amd import inference_vc as IV
    models, mel_fn = vc_setup
    srcs, f0s, prompts, f0t = _case(device, [15000] * 8, [30000], 11)
    T = srcs[0].shape[-1] // 320
    noise = torch.from_numpy(np.random.default_rng(5).standard_normal((8, 192, T)).astype(np.float32)).to(device)
    wav, n_out, audio = IV.vc_batch(models, mel_fn, srcs, f0s, prompts[0], f0t[0], noise=noise, return_float=True)
    for b in range(8):
        w1, a1 = IV.vc(models, mel_fn, srcs[b], f0s[b].reshape(1, -1), prompts[0], f0t[0].reshape(1, -1),
                       noise=noise[b:b + 1], return_float=True)
        assert _rel(audio[b:b + 1], a1) <= 1e-4, (b, _rel(audio[b:b + 1], a1))
        assert (wav[b].int() - w1.int()).abs().max() <= 4


def test_output_sr_48k_solo_and_batch(device, vc_setup):
    from megatts2_hierspeechpp_amd import inference_vc as IV, synth
    from megatts2_hierspeechpp_amd.hip_layers import finalize
    from megatts2_hierspeechpp_amd.inference_plm import peak_int16
    from megatts2_hierspeechpp_amd.speechsr24k.speechsr import SynthesizerTrn as SR24
    models, mel_fn = vc_setup
    srcs, f0s, prompts, f0t = _case(device, [9000, 9000], [20000], 13)
    T = srcs[0].shape[-1] // 320
    noise = torch.from_numpy(np.random.default_rng(6).standard_normal((2, 192, T)).astype(np.float32)).to(device)
    a = lambda b: (srcs[b], f0s[b].reshape(1, -1), prompts[0], f0t[0].reshape(1, -1))
    w16, a16 = IV.vc(models, mel_fn, *a(0), noise=noise[:1], return_float=True)
    w48, a48 = IV.vc(models, mel_fn, *a(0), noise=noise[:1], return_float=True, output_sr=48000)
    assert w48.shape == (960 * T,) and torch.equal(a48, models.sr(a16))
    assert torch.equal(w48, peak_int16(a48.reshape(1, -1)).reshape(-1))
    assert torch.equal(IV.vc(models, mel_fn, *a(0), noise=noise[:1]), w16)    # output_sr=16000: unchanged
    sr24 = SR24(128, 30, "0", [3, 7, 11], [[1, 3, 5]] * 3, [3], 32, [3])
    sr24.load_state_dict({k: torch.from_numpy(synth.synth_tensor("sr24." + k, tuple(v.shape), 1))
                          for k, v in sr24.state_dict().items()})
    finalize(sr24, device)
    for sr, rate, factor in ((models.sr, 48000, 3), (sr24, 24000, 1.5)):
        m = types.SimpleNamespace(voc=models.voc, w2v=models.w2v, sr=sr)
        wav, n_out, audio = IV.vc_batch(m, mel_fn, srcs, f0s, prompts[0], f0t[0], noise=noise, output_sr=rate,
                                        return_float=True)
        assert n_out.tolist() == [int(320 * T * factor)] * 2 and audio.shape == (2, 1, int(320 * T * factor))
        for b in range(2):
            _, a1 = IV.vc(m, mel_fn, *a(b), noise=noise[b:b + 1], return_float=True, output_sr=rate)
            assert _rel(audio[b:b + 1], a1) <= 1e-4, (rate, b, _rel(audio[b:b + 1], a1))


def test_vc_batch_files_22k_44k(device, vc_setup, tmp_path):
    from scipy.io import wavfile
    from megatts2_hierspeechpp_amd import _lib, audio as A, inference_vc as IV
    models, mel_fn = vc_setup
    files = []
    for i, (rate, n) in enumerate([(22050, 20000), (44100, 70000), (22050, 9000), (22050, 20000)]):
        p = tmp_path / f"src{i}.wav"
        wavfile.write(p, rate, _speech(n, 60 + i, rate))
        files.append(p)
    prompt = tmp_path / "voice.wav"
    wavfile.write(prompt, 44100, _speech(100000, 70, 44100))
    srcs = [IV.load_source(p, device) for p in files]
    trg = A.load_16k(prompt, device)
    for p, s in zip(files, srcs):
        np.save(str(p)[:-4] + ".hf0.npy", _track(s.shape[-1] // 80 + 1, 1)[None])
    with pytest.raises(_lib.HspError, match="voice.wav"):
        IV.vc_batch_files(models, mel_fn, files, prompt)
    np.save(tmp_path / "voice.hf0.npy", _track(trg.shape[-1] // 80, 2))
    assert IV.length_groups([s.shape[-1] for s in srcs]) == [[0, 3], [1], [2]]
    T = max(s.shape[-1] for s in srcs) // 320
    noise = torch.from_numpy(np.random.default_rng(8).standard_normal((4, 192, T)).astype(np.float32)).to(device)
    f0s = [torch.from_numpy(np.load(str(p)[:-4] + ".hf0.npy").reshape(-1)).to(device) for p in files]
    f0t = torch.from_numpy(np.load(tmp_path / "voice.hf0.npy")).to(device)
    # default: one equal-length batch per padded length, each row as its own group's vc_batch gives it
    out = tmp_path / "out"
    wav, n_out = IV.vc_batch_files(models, mel_fn, files, prompt, out_dir=out, noise=noise, output_sr=48000)
    assert wav.shape == (4, 960 * T)
    for rows in ([0, 3], [1], [2]):
        Tg = max(srcs[b].shape[-1] for b in rows) // 320
        w, n = IV.vc_batch(models, mel_fn, [srcs[b] for b in rows], [f0s[b] for b in rows], trg, f0t,
                           noise=noise[rows, :, :Tg].contiguous(), output_sr=48000)
        for i, b in enumerate(rows):
            assert int(n_out[b]) == int(n[i]) and torch.equal(wav[b, :int(n[i])], w[i, :int(n[i])]), b
            assert not wav[b, int(n[i]):].any()
    for b, p in enumerate(files):
        rate, back = wavfile.read(out / f"src{b}_to_voice.wav")
        assert rate == 48000 and np.array_equal(back, wav[b, :int(n_out[b])].cpu().numpy())
    # one ragged batch on request
    wav1, n1 = IV.vc_batch_files(models, mel_fn, files, prompt, noise=noise, output_sr=48000, group_by_length=False)
    want, n_want = IV.vc_batch(models, mel_fn, srcs, f0s, trg, f0t, noise=noise, output_sr=48000)
    assert torch.equal(wav1, want) and torch.equal(n1, n_want) and torch.equal(n1, n_out)


def test_vc_batch_graph_replay_equals_eager(device, vc_setup):
    from megatts2_hierspeechpp_amd import inference_vc as IV
    models, mel_fn = vc_setup
    srcs, f0s, prompts, f0t = _case(device, [9000, 20000, 3000], [24000], 17)
    x, xl = IV._stack(srcs, device)
    fs, fl = IV._stack(f0s, device)
    xl, fl = torch.tensor(xl, device=device), torch.tensor(fl, device=device)
    T = x.shape[1] // 320
    noise = torch.from_numpy(np.random.default_rng(9).standard_normal((3, 192, T)).astype(np.float32)).to(device)
    run = lambda: IV.vc_batch(models, mel_fn, (x, xl), (fs, fl), prompts[0], f0t[0], noise=noise, scale_norm="prompt",
                              return_float=True)
    eager = run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed = run()
    g.replay()
    torch.cuda.synchronize()
    for e, r in zip(eager, graphed):
        assert torch.equal(e, r)
    # the list form gives the same batch
    lw, ln = IV.vc_batch(models, mel_fn, srcs, f0s, prompts[0], f0t[0], noise=noise, scale_norm="prompt")
    assert torch.equal(lw, eager[0]) and torch.equal(ln, eager[1])
