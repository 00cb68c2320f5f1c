"""GPU (-m gpu): batched TTS of different lines (inference_plm.tts_batch / tts_lines / tts_batch_files, and
tts / tts_from_codes with row_exact=True).  The yardstick is the one-line harness: row b of a batch against
``tts_from_prompt`` on line b alone with the same durations, the noise ``noise[b:b+1, :, :T_b]``, the same prompt and
the same seed.

Bars: codes equal; float audio within 1e-4 of the one-line row's peak (the bar of tests/test_gpu_row_exact.py,
test_gpu_vc_batch.py and test_tts_takes_equal_solo_calls); int16 rows within 5 LSB (1e-4 x 32767 rounded up to 4, plus 1
for the truncating cast) and zero from lengths[b] on.

The base case: lines of 7 / 12 / 5 phones with pinned durations (all 4; eleven 3s and one 4; all 2) = 14 / 18.5 -> 19 /
5 frames: no frame count is a multiple of 4 (the row-exact decoder pads to 4), one ends in half a frame, the shortest
row is under a third of the longest.  Two distinct prompts of 20000 and 9000 samples; lines 0 and 2 hold the same
tensor object.  Models and synthetic weights as test_tts_takes_equal_solo_calls builds them, SpeechSR as
tests/test_gpu_vc_batch.py.

SEED: the text seed of the base case.  The bidirectional prosody LM's logits differ in the last bits between B = 1 and
B > 1 (its token GEMMs tile by the total column count), so test 2 needs every step's top-2 margin of the one-line logits
to be at least 1e-3 of max |logit| (the bar of tests/plm_prefix_ref.py's searched cases).  The front-end runs on the GPU
only, so the seed was searched there (seeds 0 .. 39); see SEED below for the measured minimum."""
import math
import os

import numpy as np
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu

SEED = 20           # measured on an MI355X: minimum top-2 margin over the 38 steps of the three rows 2.08e-2 of max |logit|
#                     (bidirectional; 1.90e-2 causal), the widest of seeds 0 .. 39 and 20 times the bar; test 2 prints it
PHONES = (7, 12, 5)
FRAMES = (14, 19, 5)
PROMPT_LENS = (20000, 9000)
PROMPT_OF = (0, 1, 0)
NOISE_W = 24        # wider than T_max = 19: the columns past it are ignored
MARGIN = 1e-3


def _durations():
    d1 = np.full(12, 3.0, np.float32)
    d1[4] = 4.0
    return [np.full(7, 4.0, np.float32), d1, np.full(5, 2.0, np.float32)]


def _prompt(n, seed, f0):
    r = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    return (0.3 * np.sin(2 * np.pi * f0 * t) + 0.05 * r.standard_normal(n)).astype(np.float32)


def _lines(device, phones, seed):
    r = np.random.default_rng(seed)
    out = []
    for n in phones:
        ids = torch.from_numpy(r.integers(12, 113, n)).to(device)
        tone = torch.from_numpy(r.integers(0, 11, n)).to(device)
        out.append((ids, tone, torch.where(ids < 74, 1, 2)))
    return out


@pytest.fixture(scope="module")
def setup(device):
    from megatts2_hierspeechpp_amd import inference_plm as IP, synth
    from megatts2_hierspeechpp_amd.Mels_preprocess import MelSpectrogramFixed
    from megatts2_hierspeechpp_amd.speechsr48k.speechsr import SynthesizerTrn as SpeechSR
    from oracle.hsp_oracle import default_config
    mel_fn = MelSpectrogramFixed(sample_rate=16000, n_fft=1280, win_length=1280, hop_length=320, f_min=0, f_max=8000,
                                 n_mels=80, window_fn=torch.hann_window).finalize(device)
    models = IP.TtsModels(default_config(), H.TTV_MODEL,
                          speechsr=SpeechSR(128, 30, "0", [3, 7, 11], [[1, 3, 5]] * 3, [3], 32, [3]))
    models.load_state_dict({k: torch.from_numpy(synth.synth_tensor(k, tuple(v.shape), 7))
                            for k, v in models.state_dict().items()})
    models.finalize(device)
    return models, mel_fn


@pytest.fixture(scope="module")
def base(device):
    """The base case, built once and left unchanged."""
    lines = _lines(device, PHONES, SEED)
    p = [torch.from_numpy(_prompt(n, 20 + i, 140.0 + 60.0 * i)).to(device).reshape(1, -1)
         for i, n in enumerate(PROMPT_LENS)]
    prompts = [p[i] for i in PROMPT_OF]
    assert prompts[0] is prompts[2]
    dur = [torch.from_numpy(d).to(device) for d in _durations()]
    noise = torch.from_numpy(np.random.default_rng(SEED + 1).standard_normal((3, 192, NOISE_W)).astype(np.float32)) \
        .to(device)
    return dict(lines=lines, prompts=prompts, dur=dur, noise=noise)


@pytest.fixture(scope="module")
def solos():
    """The one-line results of this module, keyed by (the name the caller gives the configuration, row)."""
    return {}


def _solo(solos, name, setup, case, b, frames=FRAMES, **kw):
    """`tts_from_prompt` on line b alone -> (wav, audio, codes); computed once per named configuration and row."""
    from megatts2_hierspeechpp_amd import inference_plm as IP
    if (name, b) not in solos:
        models, mel_fn = setup
        ids, tone, lang = (x.reshape(1, -1) for x in case["lines"][b])
        solos[name, b] = IP.tts_from_prompt(
            models, mel_fn, ids, tone, lang, case["prompts"][b], dur=case["dur"][b].reshape(1, -1),
            noise=case["noise"][b:b + 1, :, :frames[b]].contiguous(), return_float=True, return_codes=True, **kw)
    return solos[name, b]


def _check_rows(got, solos, what, setup, case, rate_mul=1, frames=FRAMES, codes_equal=True, tol=None, per_row=None,
                **solo_kw):
    """Rows of a `tts_batch` result (wav, lengths, audio, codes) against the one-line calls (``what`` names the
    configuration in the one-line cache; ``per_row``: keywords of row b's one-line call beside ``solo_kw``).  With
    ``tol`` (a bar on the float audio other than 1e-4 of the peak) the int16 bar scales with it: tol / peak x 32767
    rounded up, plus 1 for the truncating cast."""
    wav, lengths, audio, codes = got
    n = [320 * f * rate_mul for f in frames]
    assert lengths.tolist() == n and wav.dtype == torch.int16
    assert wav.shape == (len(frames), max(n)) and audio.shape == (len(frames), 1, max(n))
    for b in range(len(frames)):
        solo_wav, solo, solo_codes = _solo(solos, what, setup, case, b, frames, **solo_kw,
                                           **(per_row[b] if per_row else {}))
        assert solo_wav.shape == (n[b],) and codes[b].shape == (frames[b],)
        if codes_equal:
            assert torch.equal(codes[b], solo_codes), (what, b)
        peak = solo.abs().max().item()
        err = (audio[b, 0, :n[b]] - solo.reshape(-1)).abs().max().item()
        bar = 1e-4 * peak if tol is None else tol(solo)
        lsb = (wav[b, :n[b]].to(torch.int32) - solo_wav.to(torch.int32)).abs().max().item()
        print(f"{what} row {b}: max |batch - solo| = {err:.3e} (bar {bar:.3e}, peak {peak:.3f}), int16 {lsb} LSB")
        assert err <= bar, (what, b, err, bar)
        assert lsb <= (5 if tol is None else math.ceil(bar / peak * 32767.0) + 1), (what, b, lsb)
        assert not wav[b, n[b]:].any(), (what, b)


# 1
def test_causal_greedy_rows_equal_one_line_calls(setup, base, solos):
    from megatts2_hierspeechpp_amd import inference_plm as IP
    models, mel_fn = setup
    got = IP.tts_batch(models, mel_fn, base["lines"], base["prompts"], dur=base["dur"], noise=base["noise"],
                       plm_causal=True, return_float=True, return_codes=True)
    assert got[1].tolist() == [320 * f for f in FRAMES]
    _check_rows(got, solos, "causal", setup, base, plm_causal=True)
    # B = 1 goes through the same code
    one = IP.tts_batch(models, mel_fn, base["lines"][1:2], base["prompts"][1], dur=base["dur"][1:2],
                       noise=base["noise"][1:2], plm_causal=True, return_float=True, return_codes=True)
    solo_wav, solo, solo_codes = _solo(solos, "causal", setup, base, 1, plm_causal=True)
    assert torch.equal(one[0][0], solo_wav) and torch.equal(one[2].reshape(-1), solo.reshape(-1))
    assert torch.equal(one[3][0], solo_codes) and one[1].tolist() == [320 * 19]
    with pytest.raises(Exception, match="columns"):
        IP.tts_batch(models, mel_fn, base["lines"], base["prompts"], dur=base["dur"], noise=base["noise"][:, :, :18])


# 2
def test_bidirectional_greedy_rows_equal_one_line_calls(setup, base, device, solos):
    """The reference loop.  Condition of the inputs (asserted, never skipped): every step of every row has a top-2
    margin of the one-line logits of at least 1e-3 of max |logit|."""
    from megatts2_hierspeechpp_amd import inference_plm as IP
    models, mel_fn = setup
    worst = math.inf
    for b in range(3):
        ids, tone, lang = (x.reshape(1, -1) for x in base["lines"][b])
        ttv_mel, _ = IP.prompt_mels(mel_fn, base["prompts"][b])
        one = lambda v: torch.full((1,), v, dtype=torch.int64, device=device)  # noqa: E731
        x_frame = models.ttv.inf_extract_tc_latent(ids, one(ids.shape[1]), ttv_mel, one(ttv_mel.shape[2]), tone, lang,
                                                   dur=base["dur"][b].reshape(1, -1))[0]
        codes, logits = models.plm.infer(x_frame, return_logits=True)
        assert logits.shape == (1, FRAMES[b], 1024)
        top2 = logits[0].double().topk(2, dim=1).values
        ratio = ((top2[:, 0] - top2[:, 1]) / logits[0].double().abs().max()).min().item()
        print(f"row {b}: minimum top-2 margin {ratio:.3e} of max |logit| over {FRAMES[b]} steps")
        worst = min(worst, ratio)
        assert torch.equal(codes[0], _solo(solos, "bidirectional", setup, base, b)[2])
    print(f"seed {SEED}: minimum margin {worst:.3e} (bar {MARGIN:.0e})")
    assert worst >= MARGIN, worst
    got = IP.tts_batch(models, mel_fn, base["lines"], base["prompts"], dur=base["dur"], noise=base["noise"],
                       return_float=True, return_codes=True)
    _check_rows(got, solos, "bidirectional", setup, base)


# 3
def test_sampled_rows_equal_one_line_calls_with_their_seeds(setup, base):
    from megatts2_hierspeechpp_amd import inference_plm as IP
    from megatts2_hierspeechpp_amd.ttv_v1.t2w2v_transformer import PlmSampling
    models, mel_fn = setup
    sp = PlmSampling(temperature=1.3, top_p=0.98)
    # the same line and prompt three times: only the seeds tell the rows apart
    case = dict(lines=[base["lines"][0]] * 3, prompts=[base["prompts"][0]] * 3, dur=[base["dur"][0]] * 3,
                noise=base["noise"][:1].expand(3, -1, -1).contiguous())
    got = IP.tts_batch(models, mel_fn, case["lines"], case["prompts"], dur=case["dur"], noise=case["noise"],
                       plm_sampling=sp, seeds=40, plm_causal=True, return_float=True, return_codes=True)
    wav, lengths, audio, codes = got
    assert lengths.tolist() == [320 * 14] * 3
    for b in range(3):
        ids, tone, lang = (x.reshape(1, -1) for x in case["lines"][b])
        solo_wav, solo, solo_codes = IP.tts_from_prompt(
            models, mel_fn, ids, tone, lang, case["prompts"][b], dur=case["dur"][b].reshape(1, -1),
            noise=case["noise"][b:b + 1, :, :14].contiguous(), plm_sampling=sp, seed=40 + b, plm_causal=True,
            return_float=True, return_codes=True)
        assert torch.equal(codes[b], solo_codes), b
        err = (audio[b].reshape(-1) - solo.reshape(-1)).abs().max().item()
        assert err <= 1e-4 * solo.abs().max().item(), (b, err)
        assert (wav[b].to(torch.int32) - solo_wav.to(torch.int32)).abs().max().item() <= 5
    assert not torch.equal(codes[0], codes[1]) and not torch.equal(codes[1], codes[2])
    assert not torch.equal(wav[0], wav[1]) and not torch.equal(wav[1], wav[2]) and not torch.equal(wav[0], wav[2])
    # a seed tensor means the same as the int
    again = IP.tts_batch(models, mel_fn, case["lines"], case["prompts"], dur=case["dur"], noise=case["noise"],
                         plm_sampling=sp, seeds=torch.tensor([40, 41, 42]), plm_causal=True)
    assert torch.equal(again[0], wav)


# 4
def test_48k_rows_equal_one_line_calls(setup, base, solos):
    from megatts2_hierspeechpp_amd import inference_plm as IP
    models, mel_fn = setup
    got = IP.tts_batch(models, mel_fn, base["lines"], base["prompts"], dur=base["dur"], noise=base["noise"],
                       plm_causal=True, output_sr=48000, return_float=True, return_codes=True)
    _check_rows(got, solos, "48 kHz", setup, base, rate_mul=3, plm_causal=True, output_sr=48000)


def _front(setup, base, device):
    """The ragged front-end call of the base case, as `tts` makes it, and the padded prompt mels."""
    from megatts2_hierspeechpp_amd import inference_plm as IP
    models, mel_fn = setup
    pad = lambda rows, dt: torch.stack([torch.cat([r.reshape(-1), r.new_zeros(12 - r.numel())]) for r in rows]).to(dt)  # noqa: E731
    text, tone, lang = (pad([ln[i] for ln in base["lines"]], torch.int64) for i in range(3))
    dur = pad(base["dur"], torch.float32)
    mels = [IP.prompt_mels(mel_fn, p) for p in base["prompts"]]
    wt, wm = max(m[0].shape[2] for m in mels), max(m[1].shape[2] for m in mels)
    ttv = torch.zeros(3, 80, wt, device=device)
    src = torch.zeros(6, 80, wm, device=device)
    for b, (mt, mm) in enumerate(mels):
        ttv[b, :, :mt.shape[2]] = mt[0]
        src[b, :, :mm.shape[2]] = mm[0]
        src[3 + b, :, :mm.shape[2]] = mm[1]
    lens = lambda v: torch.tensor(v, dtype=torch.int64, device=device)  # noqa: E731
    style = torch.cat([models.voc.style_vector(mm, lens([mm.shape[2]] * 2)) for _, mm in mels])
    return dict(text=text, tone=tone, lang=lang, dur=dur, text_len=lens(list(PHONES)), ttv=ttv,
                ttv_len=lens([m[0].shape[2] for m in mels]), src=src, src_len=lens([m[1].shape[2] for m in mels] * 2),
                style=style)


# 5
def test_tts_from_codes_row_exact_given_codes(setup, base, device):
    """The vocoder half on its own: given random codes, every row of the ragged row-exact call against the row alone."""
    from megatts2_hierspeechpp_amd import inference_plm as IP
    models, _ = setup
    f = _front(setup, base, device)
    x_frame, g, x_lengths, x_mask = models.ttv.inf_extract_tc_latent(f["text"], f["text_len"], f["ttv"], f["ttv_len"],
                                                                     f["tone"], f["lang"], dur=f["dur"])
    assert x_lengths.tolist() == [14.0, 18.5, 5.0] and x_frame.shape[2] == 19
    codes = torch.from_numpy(np.random.default_rng(9).integers(0, 1024, (3, 19))).to(device)
    noise = base["noise"][:, :, :19].contiguous()
    wav, audio = IP.tts_from_codes(models, x_frame, g, codes, x_lengths, x_mask, None, None, noise=noise,
                                   return_float=True, row_exact=True, style=f["style"])
    loose = IP.tts_from_codes(models, x_frame, g, codes, x_lengths, x_mask, None, None, noise=noise, style=f["style"])
    assert not torch.equal(loose, wav)                 # the padded-batch semantics are another computation
    for b, T in enumerate(FRAMES):
        w1, a1 = IP.tts_from_codes(models, x_frame[b:b + 1, :, :T].contiguous(), g[b:b + 1], codes[b:b + 1, :T].contiguous(),
                                   x_lengths[b:b + 1], x_mask[b:b + 1, :, :T], None, None,
                                   noise=noise[b:b + 1, :, :T].contiguous(), return_float=True, style=f["style"][b:b + 1])
        peak = a1.abs().max().item()
        err = (audio[b, 0, :320 * T] - a1.reshape(-1)).abs().max().item()
        print(f"given codes row {b}: max |batch - solo| = {err:.3e} (bar {1e-4 * peak:.3e})")
        assert err <= 1e-4 * peak, (b, err)
        assert (wav[b, :320 * T].to(torch.int32) - w1.reshape(-1).to(torch.int32)).abs().max().item() <= 5
        assert not wav[b, 320 * T:].any() and not audio[b, 0, 320 * T:].any()


# 6
def test_tts_row_exact_on_a_hand_padded_batch_equals_tts_batch(setup, base, device):
    from megatts2_hierspeechpp_amd import inference_plm as IP
    models, mel_fn = setup
    f = _front(setup, base, device)
    noise = base["noise"][:, :, :19].contiguous()
    want = IP.tts_batch(models, mel_fn, base["lines"], base["prompts"], dur=base["dur"], noise=base["noise"],
                        plm_causal=True, return_float=True, return_codes=True)
    # the prompts have two mel widths, so the style vectors are given (src_mel wants one width)
    wav, audio, codes = IP.tts(models, f["text"], f["text_len"], f["tone"], f["lang"], f["ttv"], f["ttv_len"], None, None,
                               dur=f["dur"], noise=noise, plm_causal=True, row_exact=True, style=f["style"],
                               return_float=True, return_codes=True)
    for b, T in enumerate(FRAMES):
        assert torch.equal(codes[b, :T], want[3][b])
    assert torch.equal(wav, want[0]) and torch.equal(audio, want[2])


# 7
def test_denoise_ratio_with_a_denoiser(setup, base, device, solos):
    """Two distinct prompts denoised in one packed pass against the one-line calls, each of which denoises its prompt
    alone; the bar is the one tests/test_gpu_denoise_batch.py holds a packed row to against the row alone
    (helpers.tol_for: 1e-4 x max(1, peak))."""
    from megatts2_hierspeechpp_amd import inference_plm as IP
    from megatts2_hierspeechpp_amd.hip_layers import finalize
    models, mel_fn = setup
    meta, _ = H.load_fixture("denoise_l8000")
    net = H.build_module(meta)
    net.load_state_dict(H.synth_sd(meta), strict=True)
    finalize(net, device)
    kw = dict(denoise_ratio=0.8, denoiser=net, hps_denoiser=H.DENOISER_H)
    got = IP.tts_batch(models, mel_fn, base["lines"], base["prompts"], dur=base["dur"], noise=base["noise"],
                       plm_causal=True, return_float=True, return_codes=True, **kw)
    _check_rows(got, solos, "denoised", setup, base, tol=lambda ref: H.tol_for(ref.cpu().numpy()), plm_causal=True,
                **kw)
    plain = IP.tts_batch(models, mel_fn, base["lines"], base["prompts"], dur=base["dur"], noise=base["noise"],
                         plm_causal=True)
    assert not torch.equal(plain[0], got[0])           # the denoised style vector took part
    from megatts2_hierspeechpp_amd.inference_vc import denoise_prompts
    den = denoise_prompts([base["prompts"][0], base["prompts"][1]], net, H.DENOISER_H)
    given = IP.tts_batch(models, mel_fn, base["lines"], base["prompts"], dur=base["dur"], noise=base["noise"],
                         plm_causal=True, denoise_ratio=0.8, denoised=[den[i] for i in PROMPT_OF])
    assert torch.equal(given[0], got[0])


# 8
def test_scale_norm_prompt_uses_each_rows_own_prompt(setup, base, solos):
    from megatts2_hierspeechpp_amd import inference_plm as IP
    models, mel_fn = setup
    got = IP.tts_batch(models, mel_fn, base["lines"], base["prompts"], dur=base["dur"], noise=base["noise"],
                       plm_causal=True, scale_norm="prompt", return_float=True, return_codes=True)
    _check_rows(got, solos, "scale_norm prompt", setup, base, plm_causal=True, scale_norm="prompt")
    wav, lengths, audio, _ = got
    peaks = [base["prompts"][b].abs().max().item() for b in range(3)]
    assert peaks[0] != peaks[1]
    for b, n in enumerate(lengths.tolist()):
        row = audio[b, 0, :n]
        want = (row / row.abs().max() * (32767.0 * peaks[b])).to(torch.int32)
        assert (wav[b, :n].to(torch.int32) - want).abs().max().item() <= 1, b
        assert abs(wav[b, :n].to(torch.int32).abs().max().item() - 32767.0 * peaks[b]) <= 2.0, b


# 9
def test_lufs_limiter_stats_follow_the_one_line_calls(setup, device):
    """Two lines of 30 and 41 frames (the BS.1770 meter needs 400-ms blocks) at a target picked between the two rows'
    thresholds: brought to -6.5 LUFS, row 0 peaks at 0.869 (under the ceiling 0.891: min_gain 1) and row 1 would peak at
    0.915 (limited), so the rows' true_peak and min_gain differ by some 2e-2 and swapped stats cannot pass.

    Against the chain (the bar tests/test_gpu_limiter.py holds a ragged row to against the row alone: bit equality):
    row b's stats and int16 row equal `functional.lufs_limit_int16` on its own float row.

    Against the one-line call, whose float row differs by up to eps = 1e-4 of its peak (asserted): with L0 the one-line
    row's loudness, rms = 10^((L0 + 0.691) / 20) its K-weighted rms, 10^(4/20) the largest gain of the K filter, a meter
    reading moves by at most d = 20 log10(1 + rel), rel = 10^(4/20) eps / rms.  The chain meters once per pass and once
    more at the end, so achieved_lufs moves by (passes + 1) d at the most and the gains by a factor (1 + rel)^passes.
    The true peak is Lambda-Lipschitz in the sup norm (Lambda = limiter_ref.lam): the row scaled by G = 10^((target -
    L0) / 20) moves it by Lambda G eps, the gain error by true_peak ((1 + rel)^passes - 1), rounding by bar_tp.
    min_gain = ceiling / (true peak before limiting), smoothed by 1-Lipschitz steps: Lambda G eps / ceiling plus the
    gain error plus bar_s."""
    import limiter_ref as M
    import loudness_ref as R
    import test_gpu_limiter as TL
    from megatts2_hierspeechpp_amd import inference_plm as IP
    models, mel_fn = setup
    frames = (30, 41)
    lines = _lines(device, (15, 20), 31)
    d1 = np.full(20, 4.0, np.float32)
    d1[:2] = 5.0
    dur = [torch.full((15,), 4.0, device=device), torch.from_numpy(d1).to(device)]
    prompt = torch.from_numpy(R.speech(20000, 80, level=0.9)).reshape(1, -1).to(device)
    noise = torch.from_numpy(np.random.default_rng(32).standard_normal((2, 192, 41)).astype(np.float32)).to(device)
    target, passes, fs = -6.5, 2, 16000
    kw = dict(scale_norm="lufs", target_lufs=target, limiter=True, return_stats=True)
    wav, lengths, audio, stats, codes = IP.tts_batch(models, mel_fn, lines, prompt, dur=dur, noise=noise,
                                                     plm_causal=True, return_float=True, return_codes=True, **kw)
    n = [320 * T for T in frames]
    assert lengths.tolist() == n
    assert set(stats) == {"achieved_lufs", "true_peak", "min_gain"} and all(v.shape == (2,) for v in stats.values())
    TL._stats_equal_the_chain(stats, [wav[b, :n[b]] for b in range(2)], [audio[b, 0, :n[b]] for b in range(2)], fs, target)
    TL._equals_the_chain(wav, stats, audio, lengths, fs, target)
    bars = []
    for b, T in enumerate(frames):
        ids, tone, lang = (x.reshape(1, -1) for x in lines[b])
        w1, a1, s1, c1 = IP.tts_from_prompt(models, mel_fn, ids, tone, lang, prompt, dur=dur[b].reshape(1, -1),
                                            noise=noise[b:b + 1, :, :T].contiguous(), plm_causal=True,
                                            return_float=True, return_codes=True, **kw)
        assert torch.equal(codes[b], c1)
        peak = a1.abs().max().item()
        eps = 1e-4 * peak
        assert (audio[b, 0, :n[b]] - a1.reshape(-1)).abs().max().item() <= eps
        L0 = float(R.lufs(a1.reshape(-1).double().cpu().numpy(), fs))
        rel = 10.0 ** (4.0 / 20.0) * eps / 10.0 ** ((L0 + 0.691) / 20.0)
        G = 10.0 ** ((target - L0) / 20.0)
        gain_err = (1.0 + rel) ** passes - 1.0
        got = {k: float(v[b]) for k, v in stats.items()}
        ref = {k: float(v[0]) for k, v in s1.items()}
        bar = dict(achieved_lufs=(passes + 1) * 20.0 * math.log10(1.0 + rel),
                   true_peak=M.lam(fs) * G * eps + ref["true_peak"] * gain_err + TL.bar_tp(fs, G * peak),
                   min_gain=M.lam(fs) * G * eps / TL.C32 + gain_err + TL.bar_s(fs, 24, G * peak))
        bars.append(bar)
        for k in bar:
            print(f"row {b} {k}: batch {got[k]:.6f}, one-line {ref[k]:.6f}, |diff| {abs(got[k] - ref[k]):.2e} (bar {bar[k]:.2e})")
            assert abs(got[k] - ref[k]) <= bar[k], (b, k, got[k], ref[k], bar[k])
        assert (wav[b, :n[b]].to(torch.int32) - w1.to(torch.int32)).abs().max().item() <= \
            math.ceil((1e-4 + gain_err) * 32767.0) + 1, b
        assert not wav[b, n[b]:].any()
    # the rows tell: the limiter idles on row 0 and works on row 1, and the stats differ by far more than the bars
    assert float(stats["min_gain"][0]) == 1.0 and float(stats["min_gain"][1]) < 1.0
    for k in ("true_peak", "min_gain"):
        assert abs(float(stats[k][0]) - float(stats[k][1])) > 5.0 * max(bars[0][k], bars[1][k]), k


def _five(device):
    phones = (6, 3, 9, 3, 5)
    lines = _lines(device, phones, 77)
    dur = [torch.full((n,), 2.0 + (k % 2), device=device) for k, n in enumerate(phones)]       # 6, 4.5 -> 5, 9, 4.5, 5
    frames = [math.ceil(float(d.sum()) / 2) for d in dur]
    noise = torch.from_numpy(np.random.default_rng(78).standard_normal((5, 192, max(frames))).astype(np.float32)) \
        .to(device)
    p = [torch.from_numpy(_prompt(n, 90 + i, 120.0 + 50.0 * i)).to(device) for i, n in enumerate((8000, 12000))]
    return lines, [p[0], p[1], p[0], p[1], p[1]], dur, noise, frames


# 10
def test_tts_lines_chunking_does_not_change_the_rows(setup, device):
    from megatts2_hierspeechpp_amd import inference_plm as IP
    models, mel_fn = setup
    lines, prompts, dur, noise, frames = _five(device)
    kw = dict(dur=dur, noise=noise, plm_causal=True, return_float=True, return_codes=True)
    w5, a5, c5 = IP.tts_lines(models, mel_fn, lines, prompts, max_batch=5, **kw)
    w2, a2, c2 = IP.tts_lines(models, mel_fn, lines, prompts, max_batch=2, **kw)
    whole = IP.tts_batch(models, mel_fn, lines, prompts, dur=dur, noise=noise, plm_causal=True)
    assert [w.shape[0] for w in w5] == [320 * f for f in frames] == [w.shape[0] for w in w2]
    for k in range(5):
        assert torch.equal(c5[k], c2[k]), k
        peak = a5[k].abs().max().item()
        assert (a5[k] - a2[k]).abs().max().item() <= 1e-4 * peak, k
        assert (w5[k].to(torch.int32) - w2[k].to(torch.int32)).abs().max().item() <= 5, k
        # the caller's order: line k is row k of the un-chunked batch
        assert (w5[k].to(torch.int32) - whole[0][k, :w5[k].shape[0]].to(torch.int32)).abs().max().item() <= 5, k
    # the stats of chunked calls come back in the caller's order too: line k's are the chain's on line k's own float row
    import test_gpu_limiter as TL
    lim = dict(dur=dur, noise=noise, plm_causal=True, return_float=True, scale_norm="lufs", target_lufs=-20.0,
               limiter=True, return_stats=True)
    ws, as_, st = IP.tts_lines(models, mel_fn, lines, prompts, max_batch=2, **lim)
    assert all(v.shape == (5,) for v in st.values())
    TL._stats_equal_the_chain(st, ws, as_, 16000, -20.0)
    assert len({round(float(v), 4) for v in st["true_peak"]}) == 5     # five different rows: an order mix-up would show


# 11
def test_tts_lines_join_is_one_programme(setup, device):
    import test_gpu_loudness as TLo
    from megatts2_hierspeechpp_amd import functional as Fh, inference_plm as IP
    models, mel_fn = setup
    lines, prompts, dur, noise, frames = _five(device)
    kw = dict(dur=dur, noise=noise, plm_causal=True, max_batch=2)
    rows = IP.tts_lines(models, mel_fn, lines, prompts, return_float=True, **kw)[1]
    pause = round(12.5 * 16000 / 1000)
    wav, prog = IP.tts_lines(models, mel_fn, lines, prompts, join=True, pause_ms=12.5, scale_norm="lufs",
                             target_lufs=-27.0, return_float=True, **kw)
    n = [320 * f for f in frames]
    assert wav.dtype == torch.int16 and wav.shape == (sum(n) + 4 * pause,) and prog.shape == (1, 1, wav.shape[0])
    pos = 0
    for k in range(5):
        assert torch.equal(prog[0, 0, pos:pos + n[k]], rows[k]), k
        pos += n[k]
        if k < 4:
            assert not prog[0, 0, pos:pos + pause].any() and not wav[pos:pos + pause].any(), k
            pos += pause
    out = wav.to(torch.float32).reshape(1, -1) / 32767.0
    got = float(Fh.loudness(out, 16000)[0][0])
    bar = TLo.TOL + TLo.int16_allowance(-27.0)         # the bar of test_gpu_loudness._reads_target
    print(f"programme of {wav.shape[0]} samples: {got:.4f} LUFS, target -27 (bar {bar:.3f})")
    assert abs(got - (-27.0)) <= bar
    assert torch.equal(wav, Fh.lufs_int16(prog, None, 16000, -27.0).reshape(-1))   # ONE conversion of the programme


# 12
def test_tts_batch_files_writes_rows_and_loads_a_shared_prompt_once(setup, base, device, tmp_path, monkeypatch):
    from megatts2_hierspeechpp_amd import audio as A, inference_plm as IP
    from scipy.io import wavfile
    models, mel_fn = setup
    paths = []
    for i, n in enumerate(PROMPT_LENS):
        pcm = torch.from_numpy(np.round(_prompt(n, 20 + i, 140.0 + 60.0 * i) * 32767.0).astype(np.int16))
        IP.write_wav(tmp_path / f"p{i}.wav", 16000, pcm)
        paths.append(str(tmp_path / f"p{i}.wav"))
    calls, real = [], A.load

    def counting(path):
        calls.append(str(path))
        return real(path)

    monkeypatch.setattr(A, "load", counting)
    kw = dict(dur=base["dur"], noise=base["noise"], plm_causal=True)
    rows = IP.tts_batch_files(models, mel_fn, base["lines"], [paths[i] for i in PROMPT_OF], out_dir=tmp_path / "out",
                              names=["a", "b", "c"], **kw)
    assert sorted(calls) == sorted(paths)              # three lines, two files, two reads
    assert [r.shape[0] for r in rows] == [320 * f for f in FRAMES]
    for name, row in zip("abc", rows):
        rate, back = wavfile.read(tmp_path / "out" / f"{name}.wav")
        assert rate == 16000 and back.dtype == np.int16 and np.array_equal(back, row.cpu().numpy())
    prompts = [A.load_16k(p, device) for p in paths]
    want = IP.tts_lines(models, mel_fn, base["lines"], [prompts[i] for i in PROMPT_OF], **kw)
    assert all(torch.equal(r, w) for r, w in zip(rows, want))
    del calls[:]
    prog = IP.tts_batch_files(models, mel_fn, base["lines"], paths[0], out_dir=tmp_path / "one", join=True, **kw)
    assert calls == [paths[0]]
    rate, back = wavfile.read(tmp_path / "one" / "programme.wav")
    assert rate == 16000 and np.array_equal(back, prog.cpu().numpy())
    assert os.path.exists(tmp_path / "out" / "a.wav") and not os.path.exists(tmp_path / "one" / "line_0000.wav")
    IP.tts_batch_files(models, mel_fn, base["lines"][:1], paths[1], out_dir=tmp_path / "dflt", dur=base["dur"][:1])
    assert os.path.exists(tmp_path / "dflt" / "line_0000.wav")


def test_given_beginnings_of_one_length_and_of_different_lengths(setup, base, device, solos):
    """``plm_prefixes``: foreign codes in front of every line, against the one-line ``plm_prefix=`` -- of one length
    (``infer(prefix_codes=)``) and of different lengths, one line without any (``infer_many(prefixes=)``)."""
    from megatts2_hierspeechpp_amd import _lib as L, inference_plm as IP
    models, mel_fn = setup
    r = np.random.default_rng(12)
    kw = dict(dur=base["dur"], noise=base["noise"], plm_causal=True, return_float=True, return_codes=True)
    for lens in ((3, 3, 3), (5, 9, None)):
        pre = [None if p is None else torch.from_numpy(r.integers(0, 1024, p)).to(device) for p in lens]
        got = IP.tts_batch(models, mel_fn, base["lines"], base["prompts"], plm_prefixes=pre, **kw)
        for b, p in enumerate(pre):
            assert p is None or torch.equal(got[3][b][:p.numel()], p), (lens, b)
        _check_rows(got, solos, f"prefixes {lens}", setup, base, plm_causal=True,
                    per_row=[{} if p is None else dict(plm_prefix=p) for p in pre])
    with pytest.raises(L.HspError, match="prefix needs"):      # line 2 has 5 frames: a prefix leaves one to decode
        IP.tts_batch(models, mel_fn, base["lines"], base["prompts"],
                     plm_prefixes=[torch.zeros(5, dtype=torch.int64, device=device)] * 3, **kw)


def test_given_prosody_codes_per_line(setup, base, device, solos):
    """``prosody_codes`` as a list of B recordings' codes of different lengths, fitted per row to the row's frames."""
    from megatts2_hierspeechpp_amd import inference_plm as IP
    models, mel_fn = setup
    r = np.random.default_rng(13)
    given = [torch.from_numpy(r.integers(0, 1024, n)).to(device) for n in (20, 11, 8)]
    kw = dict(dur=base["dur"], noise=base["noise"], return_float=True, return_codes=True)
    got = IP.tts_batch(models, mel_fn, base["lines"], base["prompts"], prosody_codes=given, **kw)
    _check_rows(got, solos, "given codes", setup, base, per_row=[dict(prosody_codes=c) for c in given])
    got = IP.tts_batch(models, mel_fn, base["lines"], base["prompts"], prosody_codes=given, prosody_lengths=[16, 11, 3],
                       **kw)
    _check_rows(got, solos, "given codes and lengths", setup, base,
                per_row=[dict(prosody_codes=c, prosody_lengths=n) for c, n in zip(given, (16, 11, 3))])


def test_prompts_at_another_rate(setup, base, device, solos):
    """``prompt_sr``: every distinct prompt is resampled to 16 kHz once, as the one-line call resamples it."""
    from megatts2_hierspeechpp_amd import inference_plm as IP
    models, mel_fn = setup
    p = [torch.from_numpy(_prompt(n, 40 + i, 150.0 + 40.0 * i)).to(device).reshape(1, -1)
         for i, n in enumerate((30000, 13500))]          # 24 kHz: 20000 and 9000 samples at 16 kHz
    case = dict(base, prompts=[p[i] for i in PROMPT_OF])
    got = IP.tts_batch(models, mel_fn, case["lines"], case["prompts"], dur=case["dur"], noise=case["noise"],
                       plm_causal=True, prompt_sr=24000, return_float=True, return_codes=True)
    _check_rows(got, solos, "24 kHz prompts", setup, case, plm_causal=True, prompt_sr=24000)


PRED_TEXT_SEED = 7   # text seed of the predicted-duration batch case (test_predicted_durations_in_tts_batch): measured
#                      minimum distance from an integer 4.9e-2 over both scales, the widest of seeds 0 .. 39
PRED_SCALES = (1.0, 1.3)


def pre_ceil_durations(models, mel_fn, line, prompt, length_scale, device):
    """exp(logw) * length_scale of one line alone with its prompt: the values whose ceil the front-end takes (the first
    steps of ``SynthesizerTrn._tc_latent`` on the un-padded row)."""
    from megatts2_hierspeechpp_amd import functional as Fh, inference_plm as IP
    ttv = models.ttv
    ids, tone, lang = (x.reshape(1, -1) for x in line)
    one = lambda v: torch.full((1,), v, dtype=torch.int64, device=device)  # noqa: E731
    mel, _ = IP.prompt_mels(mel_fn, prompt.reshape(1, -1))
    n, tm = ids.shape[1], mel.shape[2]
    g = ttv.emb_g(mel, Fh.sequence_mask(one(tm), tm), per_utterance=True).unsqueeze(-1)
    h, x_mask = ttv.enc_p(ids, one(n), g, tone, lang)
    mel_out, h_mask = ttv.mel_encoder(mel, one(tm))
    xs = torch.empty(1, ttv.inter_channels, n, dtype=torch.float32, device=device)
    ttv.mha(h, mel_out, mask_q=x_mask, mask_k=h_mask, res=h, cbias=ttv.cond_g(g, force_direct=True), out=xs)
    logw = ttv.duration_predictor(xs, x_mask, g=g, lengths=one(n))
    return torch.exp(logw.double().reshape(-1)[:n]) * length_scale


def test_predicted_durations_in_tts_batch(setup, base, device):
    """``tts_batch(dur=None)``, the call a page reader makes, at ``length_scale`` 1 and 1.3: every row's frame count,
    codes and audio against the line alone.  ceil(exp(logw) * length_scale) is discontinuous, so the text (seed
    PRED_TEXT_SEED, searched on an MI355X over seeds 0 .. 39 with the base case's prompts) keeps every one-line value at
    least 1e-3 from an integer at both scales -- the distance tests/test_gpu_frontend_scale.py asks of its case;
    asserted here from the one-line values, no phone left out.  The one-line call is `tts_from_prompt(dur=None)` at
    scale 1; it has no ``length_scale``, so at 1.3 the line alone goes through the same public steps by hand:
    ``inf_extract_tc_latent(length_scale=)``, ``plm.infer(causal=True)``, `tts_from_codes`."""
    from megatts2_hierspeechpp_amd import inference_plm as IP
    models, mel_fn = setup
    lines = _lines(device, PHONES, PRED_TEXT_SEED)
    prompts = base["prompts"]
    noise = torch.from_numpy(np.random.default_rng(41).standard_normal((3, 192, 160)).astype(np.float32)).to(device)
    one = lambda v: torch.full((1,), v, dtype=torch.int64, device=device)  # noqa: E731
    seen = []
    for ls in PRED_SCALES:
        worst = math.inf
        for b in range(3):
            v = pre_ceil_durations(models, mel_fn, lines[b], prompts[b], ls, device)
            worst = min(worst, float((v - torch.round(v)).abs().min()))
        print(f"length_scale {ls}: minimum distance of exp(logw) * length_scale from an integer {worst:.2e}")
        assert worst >= 1e-3, (ls, worst)
        wav, lengths, audio, codes = IP.tts_batch(models, mel_fn, lines, prompts, noise=noise, plm_causal=True,
                                                  length_scale=ls, return_float=True, return_codes=True)
        frames = [n // 320 for n in lengths.tolist()]
        print(f"length_scale {ls}: frames {frames}")
        seen.append(frames)
        for b in range(3):
            ids, tone, lang = (x.reshape(1, -1) for x in lines[b])
            ttv_mel, src_mel = IP.prompt_mels(mel_fn, prompts[b])
            x_frame, g, x_lengths, x_mask = models.ttv.inf_extract_tc_latent(
                ids, one(ids.shape[1]), ttv_mel, one(ttv_mel.shape[2]), tone, lang, length_scale=ls)
            T = x_frame.shape[2]
            assert T == frames[b], (ls, b, T, frames)                # the row's frame count is the line's own
            nz = noise[b:b + 1, :, :T].contiguous()
            if ls == 1.0:
                w1, a1, c1 = IP.tts_from_prompt(models, mel_fn, ids, tone, lang, prompts[b], noise=nz, plm_causal=True,
                                                return_float=True, return_codes=True)
            else:
                c1 = models.plm.infer(x_frame, causal=True)
                w1, a1 = IP.tts_from_codes(models, x_frame, g, c1, x_lengths, x_mask, src_mel,
                                           torch.full((2,), src_mel.shape[2], dtype=torch.int64, device=device),
                                           noise=nz, return_float=True)
                w1, c1 = w1[0], c1[0]
            assert w1.shape == (320 * T,)
            assert torch.equal(codes[b], c1), (ls, b)
            peak = a1.abs().max().item()
            err = (audio[b, 0, :320 * T] - a1.reshape(-1)).abs().max().item()
            print(f"length_scale {ls} row {b}: {T} frames, max |batch - solo| = {err:.3e} (bar {1e-4 * peak:.3e})")
            assert err <= 1e-4 * peak, (ls, b, err)
            assert (wav[b, :320 * T].to(torch.int32) - w1.to(torch.int32)).abs().max().item() <= 5
            assert not wav[b, 320 * T:].any()
    assert seen[0] != seen[1]                              # the scale took part


# 13
def test_predicted_durations_give_the_one_line_frame_counts(setup, device):
    """Predicted durations: ceil(exp(logw)) is discontinuous, so the inputs are the ones tests/test_gpu_frontend_scale.py
    builds for its predicted-duration case (PRED_SEED with the front-end weights of that file keeps every duration away
    from an integer): those weights are loaded into the front-end here, and the padded prompt mels of that builder go
    through `tts(row_exact=True)`.  Every row's frame count, codes and audio against the call on the row alone."""
    import test_gpu_frontend_scale as FS
    from megatts2_hierspeechpp_amd import inference_plm as IP, synth
    from oracle.hsp_oracle import default_config
    models = IP.TtsModels(default_config(), H.TTV_MODEL)
    sd = {k: torch.from_numpy(synth.synth_tensor(k, tuple(v.shape), 7)) for k, v in models.state_dict().items()}
    sd.update({"ttv." + k: v for k, v in FS.ttv_state_dict()[1].items()})
    models.load_state_dict(sd)
    models.finalize(device)
    ns, tms = FS.NS, FS.TMS                            # the guarantee holds for the builder's own sizes only
    inp = FS.front_inputs(FS.PRED_SEED)
    d = lambda k: torch.from_numpy(inp[k]).to(device)  # noqa: E731
    lens = lambda v: torch.tensor(v, dtype=torch.int64, device=device)  # noqa: E731
    mel = d("mel")
    style = torch.cat([models.voc.style_vector(mel[b:b + 1, :, :tm].repeat(2, 1, 1).contiguous(), lens([tm, tm]))
                       for b, tm in enumerate(tms)])
    fl = models.ttv.inf_extract_tc_latent(d("ids"), d("lengths"), mel, d("mel_lengths"), d("tone"), d("language"))[2]
    frames = [math.ceil(v) for v in fl.tolist()]
    noise = torch.from_numpy(np.random.default_rng(6).standard_normal((3, 192, max(frames))).astype(np.float32)) \
        .to(device)
    wav, audio, codes = IP.tts(models, d("ids"), d("lengths"), d("tone"), d("language"), mel, d("mel_lengths"), None,
                               None, noise=noise, plm_causal=True, row_exact=True, style=style, return_float=True,
                               return_codes=True)
    assert wav.shape == (3, 320 * max(frames))
    print(f"predicted durations: frames {frames}")
    for b, (n, tm) in enumerate(zip(ns, tms)):
        w1, a1, c1 = IP.tts(models, d("ids")[b:b + 1, :n].contiguous(), lens([n]), d("tone")[b:b + 1, :n].contiguous(),
                            d("language")[b:b + 1, :n].contiguous(), mel[b:b + 1, :, :tm].contiguous(), lens([tm]), None,
                            None, noise=noise[b:b + 1, :, :frames[b]].contiguous(), plm_causal=True,
                            style=style[b:b + 1], return_float=True, return_codes=True)
        assert w1.shape == (1, 320 * frames[b]), (b, w1.shape, frames)       # the row's frame count is the one-line call's
        assert torch.equal(codes[b, :frames[b]], c1[0]), b
        peak = a1.abs().max().item()
        err = (audio[b, 0, :320 * frames[b]] - a1.reshape(-1)).abs().max().item()
        print(f"predicted durations row {b}: {frames[b]} frames, max |batch - solo| = {err:.3e} (bar {1e-4 * peak:.3e})")
        assert err <= 1e-4 * peak, (b, err)
        assert wav[b, 320 * frames[b] - 320:320 * frames[b]].any() and not wav[b, 320 * frames[b]:].any()
