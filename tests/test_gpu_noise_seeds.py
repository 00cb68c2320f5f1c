"""GPU (-m gpu): ``noise_seeds`` through the model and the harnesses -- the seeded prior noise of include/hsp.h makes a
row's waveform a function of (weights, inputs, seed) alone, with no noise tensor anywhere.

Model (the vocoder alone, rows of 14 / 19 / 5 frames as tests/test_gpu_tts_batch.py): ``infer`` and
``voice_conversion_noise_control`` with ``noise_seeds`` equal the same call with ``noise=randn_rows(seeds, 192, T)`` bit
for bit, at B = 3 (three FRONT_SPLITS groups, each drawing from its own slice of the seeds) and at B = 1.

Harnesses, with the bars tests/test_gpu_tts_batch.py uses for a row against its one-line call -- codes equal, float
audio within helpers.tol_for of the one-line row, int16 within 5 LSB: `tts_batch` rows against `tts_from_prompt` with
``noise_seed = s + b``; `tts_lines` on five lines cut into chunks of 2 against one chunk of 5; the takes of
`tts_from_prompt` against solo calls with ``seed + k`` / ``noise_seed + k``, the same call twice, and the unseeded call
that still draws anew; `vc_batch` rows against `vc` (inputs of tests/test_gpu_vc_batch.py's ragged case).

Defaults: with ``noise=`` given the prior sample still is `functional.sample_prior(stats, noise, mask, noise_scale)`."""
import numpy as np
import pytest
import torch

import helpers as H
from test_gpu_tts_batch import FRAMES, PHONES, PROMPT_LENS, PROMPT_OF, SEED, _durations, _lines, _prompt
from test_gpu_vc_batch import _case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tts_setup(device):
    from megatts2_hierspeechpp_amd import inference_plm as IP, synth
    from megatts2_hierspeechpp_amd.Mels_preprocess import MelSpectrogramFixed
    from oracle.hsp_oracle import default_config
    mel_fn = MelSpectrogramFixed(sample_rate=16000, n_fft=1280, win_length=1280, hop_length=320, f_min=0, f_max=8000,
                                 n_mels=80, window_fn=torch.hann_window).finalize(device)
    models = IP.TtsModels(default_config(), H.TTV_MODEL)
    models.load_state_dict({k: torch.from_numpy(synth.synth_tensor(k, tuple(v.shape), 7))
                            for k, v in models.state_dict().items()})
    models.finalize(device)
    return models, mel_fn


@pytest.fixture(scope="module")
def base(device):
    """The base case of tests/test_gpu_tts_batch.py without its noise tensor, built once and left unchanged."""
    p = [torch.from_numpy(_prompt(n, 20 + i, 140.0 + 60.0 * i)).to(device).reshape(1, -1)
         for i, n in enumerate(PROMPT_LENS)]
    return dict(lines=_lines(device, PHONES, SEED), prompts=[p[i] for i in PROMPT_OF],
                dur=[torch.from_numpy(d).to(device) for d in _durations()])


@pytest.fixture(scope="module")
def voc_inputs(device):
    """Inputs of the vocoder's entry points for rows of 14 / 19 / 5 frames, built once and left unchanged."""
    r = np.random.default_rng(11)
    T = max(FRAMES)
    g = lambda *s: torch.from_numpy(r.standard_normal(s).astype(np.float32)).to(device)  # noqa: E731
    return dict(mel=g(3, 80, T) - 4.0, w2v=0.3 * g(3, 1024, T), f0=5.0 + 0.3 * g(3, 1, 4 * T),
                trg_mel=g(6, 80, 40) - 4.0,
                length=torch.tensor(FRAMES, dtype=torch.int64, device=device),
                trg_length=torch.tensor([40, 31, 25] * 2, dtype=torch.int64, device=device),
                seeds=torch.tensor([2 ** 40 + 5, -1, 12], dtype=torch.int64, device=device))


def _row_against_solo(what, audio, wav, solo_audio, solo_wav):
    """The bars of a row against its one-line call: helpers.tol_for on the float audio, 5 LSB on int16."""
    a, s = audio.reshape(-1), solo_audio.reshape(-1)
    assert a.shape == s.shape and wav.reshape(-1).shape == solo_wav.reshape(-1).shape, what
    err, bar = (a - s).abs().max().item(), H.tol_for(s.cpu().numpy())
    lsb = (wav.reshape(-1).to(torch.int32) - solo_wav.reshape(-1).to(torch.int32)).abs().max().item()
    print(f"{what}: max |row - solo| = {err:.3e} (bar {bar:.1e}, peak {s.abs().max().item():.3f}), int16 {lsb} LSB")
    assert err <= bar, (what, err, bar)
    assert lsb <= 5, (what, lsb)


# ------------------------------------------------------------------------------------------------ model
def test_infer_with_seeds_equals_infer_with_their_noise(tts_setup, voc_inputs):
    from megatts2_hierspeechpp_amd import _lib as L, functional as Fh
    from megatts2_hierspeechpp_amd import hierspeechpp_speechsynthesizer as HS
    voc, v = tts_setup[0].voc, voc_inputs
    assert min(HS.FRONT_SPLITS, 3) > 1                      # B = 3 is cut into several groups
    noise = Fh.randn_rows(v["seeds"], 192, max(FRAMES))
    args = (v["mel"], v["w2v"], v["length"], v["f0"])
    o, e = voc.infer(*args, noise_seeds=v["seeds"], row_exact=True)
    o_n, e_n = voc.infer(*args, noise=noise, row_exact=True)
    assert torch.equal(o, o_n) and torch.equal(e, e_n)
    assert o.shape == (3, 1, 320 * max(FRAMES)) and bool(torch.isfinite(o).all()) and o.abs().max().item() > 0
    other = voc.infer(*args, noise_seeds=v["seeds"] + 1, row_exact=True)[0]
    assert not torch.equal(other, o)
    for b in (0, 1):                                        # B = 1: the row alone, by seed tensor and by int
        T = FRAMES[b]
        solo = (v["mel"][b:b + 1, :, :T].contiguous(), v["w2v"][b:b + 1, :, :T].contiguous(), v["length"][b:b + 1],
                v["f0"][b:b + 1, :, :4 * T].contiguous())
        o1, e1 = voc.infer(*solo, noise_seeds=v["seeds"][b:b + 1], row_exact=True)
        o1_n, e1_n = voc.infer(*solo, noise=noise[b:b + 1, :, :T].contiguous(), row_exact=True)
        assert torch.equal(o1, o1_n) and torch.equal(e1, e1_n), b
        assert torch.equal(voc.infer(*solo, noise_seeds=int(v["seeds"][b]), row_exact=True)[0], o1), b
    with pytest.raises(L.HspError, match="not both"):
        voc.infer(*args, noise=noise, noise_seeds=v["seeds"])
    with pytest.raises(L.HspError, match="shape"):
        voc.infer(*args, noise_seeds=v["seeds"][:2])


def test_voice_conversion_with_seeds_equals_its_noise(tts_setup, voc_inputs):
    from megatts2_hierspeechpp_amd import functional as Fh
    voc, v = tts_setup[0].voc, voc_inputs
    noise = Fh.randn_rows(v["seeds"], 192, max(FRAMES))
    args = (v["w2v"], v["length"], v["trg_mel"], v["trg_length"], v["f0"])
    for fn in (voc.voice_conversion_noise_control, voc.voice_conversion):
        # the plain form takes one prompt mel per row, the noise-control form the prompt and its denoised twin
        a = args if fn.__name__ == "voice_conversion_noise_control" else (*args[:2], args[2][:3], args[3][:3], args[4])
        got = fn(*a, noise_scale=0.333, noise_seeds=v["seeds"], row_exact=True)
        assert torch.equal(got, fn(*a, noise_scale=0.333, noise=noise, row_exact=True)), fn.__name__
        assert torch.equal(got, fn(*a, noise_scale=0.333, noise_seeds=v["seeds"], row_exact=True)), fn.__name__
    b, T = 2, FRAMES[2]                                     # B = 1
    solo = (v["w2v"][b:b + 1, :, :T].contiguous(), v["length"][b:b + 1], v["trg_mel"][[b, 3 + b]],
            v["trg_length"][[b, 3 + b]], v["f0"][b:b + 1, :, :4 * T].contiguous())
    a1 = voc.voice_conversion_noise_control(*solo, noise_seeds=v["seeds"][b:b + 1], row_exact=True)
    assert torch.equal(a1, voc.voice_conversion_noise_control(*solo, noise=noise[b:b + 1, :, :T].contiguous(),
                                                              row_exact=True))


def test_posterior_encoder_takes_seeds(tts_setup, voc_inputs):
    from megatts2_hierspeechpp_amd import functional as Fh
    voc, v = tts_setup[0].voc, voc_inputs
    mask = Fh.sequence_mask(v["length"], max(FRAMES))
    g = voc.emb_g(v["mel"], mask).unsqueeze(-1)
    z, m, logs = voc.enc_p_l(v["w2v"], v["f0"], mask, g=g, noise_seeds=v["seeds"])
    z_n, _, _ = voc.enc_p_l(v["w2v"], v["f0"], mask, g=g, noise=Fh.randn_rows(v["seeds"], 192, max(FRAMES)))
    assert torch.equal(z, z_n) and m.shape == logs.shape == z.shape


# ------------------------------------------------------------------------------------------------ defaults unchanged
def test_given_noise_still_goes_through_sample_prior(tts_setup, voc_inputs, base, device, monkeypatch):
    """With ``noise=`` every prior sample is `functional.sample_prior(stats, noise, mask, noise_scale)` on the caller's
    rows, seeds unset -- for one `infer` and one `tts_batch` call -- and `infer` is that sample pushed through the flows
    and the decoder."""
    from megatts2_hierspeechpp_amd import commons, functional as Fh, inference_plm as IP
    models, mel_fn = tts_setup
    voc, v = models.voc, voc_inputs
    calls, plain = [], Fh.sample_prior

    def recording(stats, noise, mask, noise_scale, seeds=None):
        z = plain(stats, noise, mask, noise_scale, seeds=seeds)
        calls.append((stats, noise, mask, noise_scale, seeds, z.clone()))      # the flows update z in place
        return z

    monkeypatch.setattr(Fh, "sample_prior", recording)
    T = FRAMES[1]
    mel, w2v, length, f0 = v["mel"][1:2], v["w2v"][1:2], v["length"][1:2], v["f0"][1:2]
    noise = torch.from_numpy(np.random.default_rng(3).standard_normal((3, 192, 24)).astype(np.float32)).to(device)
    o, e_ = voc.infer(mel, w2v, length, f0, noise=noise[1:2, :, :T].contiguous())
    assert len(calls) == 1 and calls[0][4] is None and torch.equal(calls[0][1], noise[1:2, :, :T])
    x_mask = commons.sequence_mask(length, T)
    g = voc.emb_g(mel, x_mask).unsqueeze(-1)
    z = plain(voc.enc_p_l.stats(w2v, f0, x_mask, g), noise[1:2, :, :T].contiguous(), x_mask, 1.0)
    assert torch.equal(z, calls[0][5])
    z = voc.flow(voc.flow_l(z, x_mask, g=g, reverse=True, owned=True), x_mask, g=g, reverse=True, owned=True)
    o_want, e_want = voc._decode(z, g)
    assert torch.equal(o, o_want) and torch.equal(e_, e_want)

    calls.clear()
    wav, lengths = IP.tts_batch(models, mel_fn, base["lines"], base["prompts"], dur=base["dur"], noise=noise,
                                plm_causal=True)
    assert lengths.tolist() == [320 * f for f in FRAMES]
    assert len(calls) == 3                                  # one prior launch per FRONT_SPLITS group
    for b, (stats, nz, mask, ns, seeds, z) in enumerate(calls):
        assert seeds is None and ns == 0.333 and torch.equal(nz, noise[b:b + 1, :, :max(FRAMES)])
        assert torch.equal(z, plain(stats, nz, mask, ns))
    again = IP.tts_batch(models, mel_fn, base["lines"], base["prompts"], dur=base["dur"], noise=noise, plm_causal=True)
    assert torch.equal(again[0], wav)


# ------------------------------------------------------------------------------------------------ harnesses
def test_tts_batch_rows_equal_one_line_calls_with_their_noise_seeds(tts_setup, base):
    from megatts2_hierspeechpp_amd import inference_plm as IP
    models, mel_fn = tts_setup
    wav, lengths, audio, codes = IP.tts_batch(models, mel_fn, base["lines"], base["prompts"], dur=base["dur"],
                                              noise_seeds=7, plm_causal=True, return_float=True, return_codes=True)
    assert lengths.tolist() == [320 * f for f in FRAMES]
    for b, T in enumerate(FRAMES):
        ids, tone, lang = (x.reshape(1, -1) for x in base["lines"][b])
        solo_wav, solo, solo_codes = IP.tts_from_prompt(models, mel_fn, ids, tone, lang, base["prompts"][b],
                                                        dur=base["dur"][b].reshape(1, -1), noise_seed=7 + b,
                                                        plm_causal=True, return_float=True, return_codes=True)
        assert torch.equal(codes[b], solo_codes), b
        _row_against_solo(f"tts_batch(noise_seeds=7) row {b}", audio[b, 0, :320 * T], wav[b, :320 * T], solo, solo_wav)
        assert not wav[b, 320 * T:].any()
    # a seed tensor means the same as the int, on the host or on the device
    for seeds in (torch.tensor([7, 8, 9]), torch.tensor([7, 8, 9], device=wav.device)):
        assert torch.equal(IP.tts_batch(models, mel_fn, base["lines"], base["prompts"], dur=base["dur"],
                                        noise_seeds=seeds, plm_causal=True)[0], wav)
    other = IP.tts_batch(models, mel_fn, base["lines"], base["prompts"], dur=base["dur"], noise_seeds=8,
                         plm_causal=True)
    assert not torch.equal(other[0], wav)


def test_tts_lines_rows_do_not_depend_on_the_chunking(tts_setup, base, device):
    """Five lines, chunks of 2 against one chunk of 5: the caller's line k draws with 7 + k wherever it lands."""
    from megatts2_hierspeechpp_amd import inference_plm as IP
    models, mel_fn = tts_setup
    phones = (7, 12, 5, 9, 6)
    lines = _lines(device, phones, SEED + 3)
    dur = [torch.full((n,), 2.0, device=device) for n in phones]         # one frame per phone
    assert IP.line_chunks(phones, 2) == [[2, 4], [0, 3], [1]]            # every line changes its row and its chunk
    kw = dict(dur=dur, noise_seeds=7, plm_causal=True, return_float=True, return_codes=True)
    run = lambda mb: IP.tts_lines(models, mel_fn, lines, base["prompts"][0], max_batch=mb, **kw)  # noqa: E731
    (w2, a2, c2), (w5, a5, c5) = run(2), run(5)
    for k, n in enumerate(phones):
        assert w2[k].shape == (320 * n,) and torch.equal(c2[k], c5[k]), k
        _row_against_solo(f"tts_lines line {k}: max_batch 2 against 5", a2[k], w2[k], a5[k], w5[k])
    k = 3                                                                # ... and it is the one-line call with 7 + k
    ids, tone, lang = (x.reshape(1, -1) for x in lines[k])
    solo_wav, solo, solo_codes = IP.tts_from_prompt(models, mel_fn, ids, tone, lang, base["prompts"][0],
                                                    dur=dur[k].reshape(1, -1), noise_seed=7 + k, plm_causal=True,
                                                    return_float=True, return_codes=True)
    assert torch.equal(c2[k], solo_codes)
    _row_against_solo(f"tts_lines line {k} against tts_from_prompt(noise_seed={7 + k})", a2[k], w2[k], solo, solo_wav)
    # a tensor holds one seed per line
    w_t = IP.tts_lines(models, mel_fn, lines, base["prompts"][0], max_batch=2, dur=dur, plm_causal=True,
                       noise_seeds=torch.arange(7, 12))
    assert all(torch.equal(a, b) for a, b in zip(w_t, w2))


def test_takes_are_reproducible_down_to_the_waveform(tts_setup, device):
    """tts_from_prompt(takes=3, seed=s, noise_seed=11): take k against the solo call with seed s + k and noise_seed
    11 + k; the same call twice gives the same bits; the takes differ; without noise_seed two calls differ (the draw
    from torch's generator, as before)."""
    from megatts2_hierspeechpp_amd import inference_plm as IP
    from megatts2_hierspeechpp_amd.ttv_v1.t2w2v_transformer import PlmSampling
    models, mel_fn = tts_setup
    r = np.random.default_rng(5)                             # the inputs of test_tts_takes_equal_solo_calls
    N = 7
    ids = torch.from_numpy(r.integers(12, 113, (1, N))).to(device)
    tone = torch.from_numpy(r.integers(0, 11, (1, N))).to(device)
    lang = torch.where(ids < 74, 1, 2)
    t = np.arange(20000) / 16000.0
    prompt = torch.from_numpy((0.3 * np.sin(2 * np.pi * 140 * t) + 0.05 * r.standard_normal(20000))
                              .astype(np.float32)[None]).to(device)
    kw = dict(dur=torch.full((1, N), 4.0, device=device), plm_sampling=PlmSampling(temperature=1.3, top_p=0.98),
              return_float=True, return_codes=True)
    call = lambda **k: IP.tts_from_prompt(models, mel_fn, ids, tone, lang, prompt, **kw, **k)  # noqa: E731
    wav, audio, codes = call(seed=40, takes=3, noise_seed=11)
    assert wav.shape == (3, N * 2 * 320) and wav.dtype == torch.int16
    for k in range(3):
        solo_wav, solo, solo_codes = call(seed=40 + k, noise_seed=11 + k)
        assert torch.equal(codes[k], solo_codes), k
        _row_against_solo(f"take {k} against seed {40 + k}, noise_seed {11 + k}", audio[k], wav[k], solo, solo_wav)
    again = call(seed=40, takes=3, noise_seed=11)
    assert torch.equal(again[0], wav) and torch.equal(again[1], audio) and torch.equal(again[2], codes)
    assert not torch.equal(wav[0], wav[1]) and not torch.equal(wav[1], wav[2]) and not torch.equal(wav[0], wav[2])
    # the noise seed alone tells two takes of the same codes apart
    same_codes = call(seed=40, noise_seed=12)
    assert torch.equal(same_codes[2], codes[0]) and not torch.equal(same_codes[0], wav[0])
    # today's behaviour, kept: no noise_seed, no noise -> another draw on every call
    first, second = call(seed=40, takes=3), call(seed=40, takes=3)
    assert torch.equal(first[2], second[2]) and not torch.equal(first[0], second[0])


def test_vc_batch_rows_equal_vc_with_their_noise_seeds(device):
    from megatts2_hierspeechpp_amd import inference_vc as IV, synth
    from megatts2_hierspeechpp_amd.Mels_preprocess import MelSpectrogramFixed
    from oracle.hsp_oracle import default_config
    models = IV.VcModels(default_config())
    models.load_state_dict({k: torch.from_numpy(synth.synth_tensor(k, tuple(v.shape), 2))
                            for k, v in models.state_dict().items()})
    models.finalize(device)
    mel_fn = MelSpectrogramFixed(sample_rate=16000, n_fft=1280, win_length=1280, hop_length=320, f_min=0, f_max=8000,
                                 n_mels=80, window_fn=torch.hann_window).finalize(device)
    srcs, f0s, prompts, f0t = _case(device, [12000, 30000, 5000], [40000, 23456], 7)       # the ragged contract case
    rows_p, rows_t = [prompts[0], prompts[1], prompts[0]], [f0t[0], f0t[1], f0t[0]]
    seeds = torch.tensor([2 ** 40 + 5, -1, 3], dtype=torch.int64)
    wav, n_out, audio = IV.vc_batch(models, mel_fn, srcs, f0s, rows_p, rows_t, noise_seeds=seeds, return_float=True,
                                    row_exact=True)
    for b in range(3):
        n = 320 * (srcs[b].shape[-1] // 320)
        assert int(n_out[b]) == n
        w1, a1 = IV.vc(models, mel_fn, srcs[b], f0s[b].reshape(1, -1), rows_p[b], rows_t[b].reshape(1, -1),
                       noise_seed=int(seeds[b]), return_float=True)
        _row_against_solo(f"vc_batch(noise_seeds) row {b}", audio[b, 0, :n], wav[b, :n], a1, w1)
        assert not wav[b, n:].any()
    # an int s gives row b the seed s + b
    by_int = IV.vc_batch(models, mel_fn, srcs, f0s, rows_p, rows_t, noise_seeds=3, row_exact=True)
    by_tensor = IV.vc_batch(models, mel_fn, srcs, f0s, rows_p, rows_t, noise_seeds=torch.tensor([3, 4, 5]),
                            row_exact=True)
    assert torch.equal(by_int[0], by_tensor[0])
