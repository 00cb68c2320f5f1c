"""GPU (-m gpu): the BS.1770-4 meter of csrc/hsp_loudness.hip against the float64 restatement (tests/loudness_ref.py),
ragged batches against solo rows, the gain op, the int16 stage end to end, scale_norm="lufs" of the harnesses, and the
meter -> gains -> int16 chain under graph capture.

Bars.  TOL = 0.1 LU is the meter tolerance of EBU Tech 3341.  Where an int16 row is metered, truncation to int16 moves
every sample by less than 1 / 32767 of full scale; K-weighting amplifies by 10^(4 / 20) at the most (the shelf), and a
block that passes the relative gate is at most 10 LU under the target, so its K-weighted rms is at least
10^((target - 10 + 0.691) / 20): the reading moves by at most 20 log10(1 + 10^(4 / 20) / 32767 / that rms)
(`int16_allowance`; 0.028 LU at -27 LUFS)."""
import numpy as np
import pytest
import torch

import helpers as H
import loudness_ref as R

pytestmark = pytest.mark.gpu

TOL = 0.1
ROWS_16K = ("16k_799", "16k_800", "16k_801", "16k_1599", "16k_6400", "16k_19680", "16k_two_level")


def int16_allowance(target):
    return 20.0 * np.log10(1.0 + 10.0 ** (4.0 / 20.0) / 32767.0 / 10.0 ** ((target - 10.0 + 0.691) / 20.0))


def _solo(name, device):
    from megatts2_hierspeechpp_amd import functional as Fh
    fs, x = R.cases()[name]
    lufs, peak = Fh.loudness(torch.from_numpy(x).reshape(1, -1).to(device), fs)
    return lufs.cpu(), peak.cpu()


def _padded(names, device, extra=37, tail=2):
    """The rows of `names` in one [B, n] view of a [B, n + extra] buffer (x_bs > n), n = the longest + tail, NaN
    everywhere outside the rows."""
    xs = [R.cases()[k][1] for k in names]
    lens = [len(x) for x in xs]
    n = max(lens) + tail
    buf = torch.full((len(xs), n + extra), float("nan"), dtype=torch.float32)
    for b, x in enumerate(xs):
        buf[b, :lens[b]] = torch.from_numpy(x)
    return buf.to(device)[:, :n], torch.tensor(lens, dtype=torch.int64, device=device)


@pytest.mark.parametrize("name", ROWS_16K + ("24k_2s", "48k_2s"))
def test_meter_matches_float64_restatement(name, device):
    want, _, want_peak = R.reference(name)
    lufs, peak = _solo(name, device)
    dev = abs(float(lufs[0]) - want)
    print(f"{name}: gpu {float(lufs[0]):.6f} LUFS, float64 {want:.6f}, |diff| {dev:.2e} LU")
    assert dev <= TOL, (name, float(lufs[0]), want)
    assert float(peak[0]) == want_peak


def test_edge_rows_silent_and_empty(device):
    from megatts2_hierspeechpp_amd import functional as Fh
    x = torch.zeros(3, 16000, device=device)
    x[1, :8000] = torch.from_numpy(R.speech(8000, 2)).to(device)
    lens = torch.tensor([16000, 0, 100], dtype=torch.int64, device=device)     # silent with blocks; empty; silent, short
    lufs, peak = Fh.loudness(x, 16000, lens)
    assert torch.isneginf(lufs).all() and not peak.any()
    quiet = 1e-4 * torch.from_numpy(np.stack([R.speech(48000, 4), R.speech(48000, 5)])).to(device)   # about -94 LUFS
    lufs, peak = Fh.loudness(quiet, 16000, torch.tensor([48000, 6399], device=device))
    assert torch.isneginf(lufs[0])                                             # every block under the absolute gate
    assert abs(float(lufs[1]) - R.lufs(quiet[1, :6399].cpu().numpy(), 16000)) <= TOL       # under 400 ms: ungated
    assert torch.equal(peak, torch.stack([quiet[0].abs().max(), quiet[1, :6399].abs().max()]))


@pytest.mark.parametrize("names", [ROWS_16K, ("24k_2s", "16k_19680"), ("48k_2s", "16k_6400", "16k_801")])
def test_ragged_batch_rows_equal_solo_rows_bitwise(names, device):
    """Padded rows, x_bs > n, NaN past every row's length: each row's (lufs, peak) is bit-identical to the call on that
    row alone, at 16 kHz (2 chunks per hop) and -- the same samples read as 24 / 48 kHz rows -- at 3 and 6."""
    from megatts2_hierspeechpp_amd import functional as Fh
    fs = R.cases()[names[0]][0]
    x, lens = _padded(names, device)
    assert x.stride(0) > x.shape[1] and torch.isnan(x).any()
    lufs, peak = Fh.loudness(x, fs, lens)
    assert torch.isfinite(lufs).all() and torch.isfinite(peak).all()
    for b, n in enumerate(lens.tolist()):
        l1, p1 = Fh.loudness(x[b:b + 1, :n].contiguous(), fs)
        assert torch.equal(lufs[b:b + 1], l1) and torch.equal(peak[b:b + 1], p1), (names[b], float(lufs[b]), float(l1))
    # a different batch around the same rows
    l2, p2 = Fh.loudness(x[1:3], fs, lens[1:3])
    assert torch.equal(l2, lufs[1:3]) and torch.equal(p2, peak[1:3])


def test_gain_op_matches_numpy(device):
    from megatts2_hierspeechpp_amd import functional as Fh
    lufs = np.array([-14.2, -30.0, -23.0, -np.inf, -60.5, -3.0, -np.inf, -49.0], np.float32)
    peak = np.array([0.5, 0.25, 0.9, 0.0, 0.01, 1.0, 0.3, 0.9], np.float32)
    for target, ceiling in ((-23.0, 0.999), (-16.0, 0.5), (-27.0, 1.0)):
        fin = np.isfinite(lufs)
        want = np.full(len(lufs), np.inf)
        want[fin] = 10.0 ** ((np.float64(np.float32(target)) - lufs[fin].astype(np.float64)) / 20.0) * peak[fin]
        lim = want >= np.float64(np.float32(ceiling))
        want = np.where(lim, np.float64(np.float32(ceiling)), want).astype(np.float32)
        gains, limited = Fh.loudness_gains(torch.from_numpy(lufs).to(device), torch.from_numpy(peak).to(device), target,
                                           ceiling)
        assert limited.dtype == torch.int32 and np.array_equal(limited.cpu().numpy(), lim.astype(np.int32)), target
        np.testing.assert_allclose(gains.cpu().numpy(), want, rtol=2.0 ** -23, atol=0)
        assert lim[3] and lim[6] and lim.sum() > 2 and (~lim).sum() >= 2       # -inf rows, a real limit, free rows


def test_int16_rows_read_the_target(device):
    """meter -> gains -> peak_int16_gains on the ragged 16 kHz rows plus a row that cannot reach the target (a spike
    over a quiet floor) and a silent row: every unlimited row reads the target, the limited row peaks at the ceiling,
    the silent row is zeros."""
    from megatts2_hierspeechpp_amd import functional as Fh
    target, ceiling = -23.0, 0.999
    x, lens = _padded(ROWS_16K, device)
    B0, n = x.shape
    spiky = 0.004 * R.speech(8000, 40)
    spiky[4000] = 0.9
    y = torch.full((B0 + 2, n), float("nan"), device=device)
    y[:B0] = x
    y[B0, :8000] = torch.from_numpy(spiky).to(device)
    y[B0 + 1, :5000] = 0.0
    lens = torch.cat([lens, torch.tensor([8000, 5000], device=device)])
    lufs, peak = Fh.loudness(y, 16000, lens)
    gains, limited = Fh.loudness_gains(lufs, peak, target, ceiling)
    wav = Fh.peak_int16_gains(y, lens, gains)
    assert torch.equal(wav, Fh.lufs_int16(y, lens, 16000, target, ceiling))
    assert limited.tolist() == [0] * B0 + [1, 1]
    out = wav.to(torch.float32) / 32767.0
    got, _ = Fh.loudness(out, 16000, lens)
    bar = TOL + int16_allowance(target)
    for b in range(B0):
        nb = int(lens[b])
        ref, margin = R.integrated_loudness(out[b, :nb].cpu().numpy(), 16000)
        assert margin > 0.1, (b, margin)                           # the scaled row is as well conditioned as its source
        print(f"{ROWS_16K[b]}: int16 row reads {float(got[b]):.4f} (gpu) / {ref:.4f} (float64), target {target}")
        assert abs(float(got[b]) - target) <= bar and abs(ref - target) <= bar, (b, float(got[b]), ref)
        assert not wav[b, nb:].any()
    assert abs(int(wav[B0].abs().max()) / 32767.0 - ceiling) <= 1.0 / 32767.0
    assert float(got[B0]) < target - 1.0                           # limited: it stays under the target
    assert not wav[B0 + 1].any()


def test_meter_gains_int16_capture_replays_equal_eager(device):
    """The whole int16 stage issues launches on one stream and nothing else (no read-back, no host copy): it captures
    as one linear chain, and two replays give the eager result."""
    from megatts2_hierspeechpp_amd import functional as Fh
    x, lens = _padded(ROWS_16K, device)

    def run():
        lufs, peak = Fh.loudness(x, 16000, lens)
        gains, limited = Fh.loudness_gains(lufs, peak, -20.0)
        return lufs, peak, gains, limited, Fh.peak_int16_gains(x, lens, gains)

    eager = [t.clone() for t in run()]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed = run()
    for _ in range(2):
        for t in graphed:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        for e, r in zip(eager, graphed):
            assert torch.equal(e, r)


# ---------------------------------------------------------------------------------------------- harnesses
def _mel_fn(device):
    from megatts2_hierspeechpp_amd.Mels_preprocess import MelSpectrogramFixed
    return MelSpectrogramFixed(sample_rate=16000, n_fft=1280, win_length=1280, hop_length=320, f_min=0, f_max=8000,
                               n_mels=80, window_fn=torch.hann_window).finalize(device)


def _track(n, seed, lo=90.0, hi=300.0):
    r = np.random.default_rng(seed)
    return np.where(r.random(n) < 0.3, 0, r.uniform(lo, hi, n)).astype(np.float32)


def _reads_target(wav_row, fs, target, what):
    from megatts2_hierspeechpp_amd import functional as Fh
    out = wav_row.to(torch.float32).reshape(1, -1) / 32767.0
    got = float(Fh.loudness(out, fs)[0][0])
    ref, margin = R.integrated_loudness(out[0].cpu().numpy(), fs)
    print(f"{what}: {got:.4f} LUFS (gpu), {ref:.4f} (float64), gate margin {margin:.2f} LU, target {target}")
    bar = TOL + int16_allowance(target)
    assert abs(got - target) <= bar and abs(ref - target) <= bar, (what, got, ref, target)


def test_vc_batch_scale_norm_lufs(device):
    from megatts2_hierspeechpp_amd import _lib, functional as Fh, inference_vc as IV, synth
    from oracle.hsp_oracle import default_config
    models = IV.VcModels(default_config())
    models.load_state_dict({k: torch.from_numpy(synth.synth_tensor(k, tuple(v.shape), 2))
                            for k, v in models.state_dict().items()})
    models.finalize(device)
    mel_fn = _mel_fn(device)
    srcs = [IV.pad_source(torch.from_numpy(R.speech(n, 50 + b, level=0.9)).to(device).reshape(1, -1))
            for b, n in enumerate((12000, 30000))]
    f0s = [torch.from_numpy(_track(s.shape[-1] // 80 + 1, 60 + b)).to(device) for b, s in enumerate(srcs)]
    prompt = torch.from_numpy(R.speech(24000, 70, level=0.9)).to(device).reshape(1, -1)
    f0t = torch.from_numpy(_track(24000 // 80, 71, 150.0, 350.0)).to(device)
    T = max(s.shape[-1] for s in srcs) // 320
    noise = torch.from_numpy(np.random.default_rng(3).standard_normal((2, 192, T)).astype(np.float32)).to(device)
    w_max, n_max, a_max = IV.vc_batch(models, mel_fn, srcs, f0s, prompt, f0t, noise=noise, return_float=True)
    wav, n_out, audio = IV.vc_batch(models, mel_fn, srcs, f0s, prompt, f0t, noise=noise, return_float=True,
                                    scale_norm="lufs", target_lufs=-27)
    assert torch.equal(audio, a_max) and torch.equal(n_out, n_max) and n_out.tolist() == [12800, 30720]
    for b, n in enumerate(n_out.tolist()):
        _reads_target(wav[b, :n], 16000, -27.0, f"vc_batch row {b}")
        assert not wav[b, n:].any()
    assert torch.equal(wav, Fh.lufs_int16(audio, n_out, 16000, -27.0))         # the stage is that chain on these rows
    # the single-utterance harness takes the same rule
    w1, a1 = IV.vc(models, mel_fn, srcs[1], f0s[1].reshape(1, -1), prompt, f0t.reshape(1, -1), noise=noise[1:2],
                   return_float=True, scale_norm="lufs", target_lufs=-27)
    _reads_target(w1, 16000, -27.0, "vc")
    assert torch.equal(w1, Fh.lufs_int16(a1, None, 16000, -27.0).reshape(-1))
    with pytest.raises(_lib.HspError, match="unknown scale_norm"):
        IV.vc_batch(models, mel_fn, srcs, f0s, prompt, f0t, noise=noise, scale_norm="rms")


def test_tts_from_prompt_scale_norm_lufs(device):
    from megatts2_hierspeechpp_amd import _lib, functional as Fh, inference_plm as IP, synth
    from oracle.hsp_oracle import default_config
    models = IP.TtsModels(default_config(), H.TTV_MODEL)
    models.load_state_dict({k: torch.from_numpy(synth.synth_tensor(k, tuple(v.shape), 7))
                            for k, v in models.state_dict().items()})
    models.finalize(device)
    mel_fn = _mel_fn(device)
    r = np.random.default_rng(5)
    N = 7
    ids = torch.from_numpy(r.integers(12, 113, (1, N))).to(device)
    tone = torch.from_numpy(r.integers(0, 11, (1, N))).to(device)
    lang = torch.where(ids < 74, 1, 2)
    kw = dict(dur=torch.full((1, N), 4.0, device=device), return_float=True,
              noise=torch.from_numpy(r.standard_normal((1, 192, N * 2)).astype(np.float32)).to(device))
    prompt = torch.from_numpy(R.speech(20000, 80, level=0.9)).reshape(1, -1).to(device)
    w_max, a_max = IP.tts_from_prompt(models, mel_fn, ids, tone, lang, prompt, **kw)
    wav, audio = IP.tts_from_prompt(models, mel_fn, ids, tone, lang, prompt, scale_norm="lufs", **kw)
    assert wav.dtype == torch.int16 and wav.shape == w_max.shape and torch.equal(audio, a_max)
    _reads_target(wav, 16000, -23.0, "tts_from_prompt")
    assert torch.equal(wav, Fh.lufs_int16(audio, None, 16000, -23.0).reshape(-1))
    w27, a27 = IP.tts_from_prompt(models, mel_fn, ids, tone, lang, prompt, scale_norm="lufs", target_lufs=-27.0, **kw)
    _reads_target(w27, 16000, -27.0, "tts_from_prompt at -27")
    assert torch.equal(w27, Fh.lufs_int16(a27, None, 16000, -27.0).reshape(-1))
    with pytest.raises(_lib.HspError, match="unknown scale_norm"):
        IP.tts_from_prompt(models, mel_fn, ids, tone, lang, prompt, scale_norm="rms", **kw)


def test_super_resolution_scale_norm_lufs(device):
    from megatts2_hierspeechpp_amd import synth
    from megatts2_hierspeechpp_amd.hip_layers import finalize
    from megatts2_hierspeechpp_amd.inference_plm import peak_int16
    from megatts2_hierspeechpp_amd.inference_speechsr import super_resolution
    from megatts2_hierspeechpp_amd.speechsr48k.speechsr import SynthesizerTrn as SpeechSR
    sr = SpeechSR(128, 30, "0", [3, 7, 11], [[1, 3, 5]] * 3, [3], 32, [3])
    sr.load_state_dict({k: torch.from_numpy(synth.synth_tensor("sr." + k, tuple(v.shape), 0)) for k, v in sr.state_dict().items()})
    finalize(sr, device)
    x = torch.from_numpy(R.speech(16000, 90, level=0.9)).reshape(1, -1).to(device)
    wav = super_resolution(sr, x, 16000, scale_norm="lufs", target_lufs=-30.0)
    assert wav.shape == (48000,)
    _reads_target(wav, 48000, -30.0, "super_resolution")
    assert torch.equal(super_resolution(sr, x, 16000), peak_int16(sr(x.unsqueeze(1)).reshape(1, -1)).reshape(-1))
