"""GPU (-m gpu): the prosody controls at model level -- ``pitch=`` / ``lf0=`` / ``return_lf0=`` / per-line
``length_scale`` / ``phone_scale=`` of the TTS harnesses, ``pitch=`` / ``return_lf0=`` of the VC harnesses (DESIGN.md
§4.3.1).  Random-weight models and small lines as tests/test_gpu_tts_batch.py, whose helpers are imported; the vocoder's
prior noise is seeded (``noise_seeds``), so a take is a function of its inputs and everything that is one computation is
compared bit for bit (torch.equal).

Where a row of a batch stands against the one-line call the comparison is the one `_check_rows` of
tests/test_gpu_tts_batch.py applies (`_rows_equal` below restates it for seeded noise and predicted durations): codes
equal, float audio within 1e-4 of the one-line row's peak, int16 within 5 LSB, zeros from the row's length on -- and the
edited log-F0 rows, whose inputs are given and equal, bit for bit.  VC rows under ``row_exact=True``: the bars of
tests/test_gpu_row_exact.py (1e-4 of the peak, 8 LSB).

The pitch predictor of a random-weight model need not voice a single frame, so the edits that must be heard act on a
given synthetic track (``lf0=``, tests/f0_edit_ref.track); its voiced count is asserted."""
import math

import numpy as np
import pytest
import torch

import f0_edit_ref as R
import helpers as H
import test_gpu_tts_batch as TB
from test_gpu_vc_batch import _case as vc_case, _rel

pytestmark = pytest.mark.gpu

NOISE_SEED = 50
SHIFT = (2.0, 0.0, -3.0)          # row 1 is an identity row in a mixed batch
RANGE = (1.0, 1.0, 0.6)
LENGTH_SCALE = (1.0, 1.3, 1.0)    # the scales TB.PRED_TEXT_SEED was searched at


@pytest.fixture(scope="module")
def setup(device):
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
def case(device):
    """Three lines of 7 / 12 / 5 phones, two prompts (lines 0 and 2 share one), pinned durations for the tests that
    want fixed frame counts (14 / 19 / 5 frames).  Built once and left unchanged."""
    lines = TB._lines(device, TB.PHONES, TB.PRED_TEXT_SEED)
    p = [torch.from_numpy(TB._prompt(n, 20 + i, 140.0 + 60.0 * i)).to(device).reshape(1, -1)
         for i, n in enumerate(TB.PROMPT_LENS)]
    return dict(lines=lines, prompts=[p[i] for i in TB.PROMPT_OF],
                dur=[torch.from_numpy(d).to(device) for d in TB._durations()])


def _given_track(n, seed, device):
    l = R.track(n, seed, voiced=0.8)
    assert (l > 0).sum() >= n // 3
    return torch.from_numpy(l).to(device)


def _one(case, b):
    return tuple(x.reshape(1, -1) for x in case["lines"][b])


def _rows_equal(got, solos, frames):
    """`_check_rows` of tests/test_gpu_tts_batch.py on (wav, lengths, audio, codes[, tracks]) against the one-line
    results (wav, audio, codes[, track]) -- the same bars -- and the log-F0 rows bit for bit."""
    wav, lengths, audio, codes = got[:4]
    n = [320 * f for f in frames]
    assert lengths.tolist() == n and wav.dtype == torch.int16
    assert wav.shape == (len(frames), max(n)) and audio.shape == (len(frames), 1, max(n))
    for b in range(len(frames)):
        solo_wav, solo, solo_codes = solos[b][:3]
        assert solo_wav.shape == (n[b],) and codes[b].shape == (frames[b],)
        assert torch.equal(codes[b], solo_codes), b
        peak = solo.abs().max().item()
        err = (audio[b, 0, :n[b]] - solo.reshape(-1)).abs().max().item()
        lsb = (wav[b, :n[b]].to(torch.int32) - solo_wav.to(torch.int32)).abs().max().item()
        print(f"row {b}: max |batch - solo| = {err:.3e} (bar {1e-4 * peak:.3e}, peak {peak:.3f}), int16 {lsb} LSB")
        assert err <= 1e-4 * peak, (b, err)
        assert lsb <= 5, (b, lsb)
        assert not wav[b, n[b]:].any(), b
        if len(got) > 4:
            assert got[4][b].shape == (4 * frames[b],) and torch.equal(got[4][b], solos[b][3]), b


def _record_calls(monkeypatch):
    from megatts2_hierspeechpp_amd import _lib as L
    seen, real = [], L.call

    def recording(name, *a):
        seen.append(name)
        return real(name, *a)

    monkeypatch.setattr(L, "call", recording)
    return seen


def test_no_edit_is_the_take_as_it_was(setup, case, device, monkeypatch):
    """``pitch=None``, an identity `PitchEdit` and the call without the keyword: the same int16 rows in `tts` and
    `tts_batch`, and neither new launch is made."""
    from megatts2_hierspeechpp_amd import inference_plm as IP
    from megatts2_hierspeechpp_amd.prosody_controls import PitchEdit
    models, mel_fn = setup
    seen = _record_calls(monkeypatch)
    ids, tone, lang = _one(case, 0)
    ttv_mel, src_mel = IP.prompt_mels(mel_fn, case["prompts"][0])
    one = lambda v, k=1: torch.full((k,), v, dtype=torch.int64, device=device)  # noqa: E731
    run = lambda **kw: IP.tts(models, ids, one(ids.shape[1]), tone, lang, ttv_mel, one(ttv_mel.shape[2]), src_mel,  # noqa: E731
                              one(src_mel.shape[2], 2), dur=case["dur"][0].reshape(1, -1), plm_causal=True,
                              noise_seeds=NOISE_SEED, **kw)
    plain = run()
    assert plain.shape == (1, 320 * 14) and plain.any()
    for kw in (dict(pitch=None), dict(pitch=PitchEdit()), dict(pitch=PitchEdit(shift=[0.0], range=[1.0]), lf0=None,
                                                               length_scale=1.0, phone_scale=None)):
        assert torch.equal(run(**kw), plain), kw
    batch = lambda **kw: IP.tts_batch(models, mel_fn, case["lines"], case["prompts"], dur=case["dur"], plm_causal=True,  # noqa: E731
                                      noise_seeds=NOISE_SEED, **kw)
    wav, lengths = batch()
    assert lengths.tolist() == [320 * f for f in TB.FRAMES]
    for kw in (dict(pitch=None), dict(pitch=PitchEdit()), dict(pitch=PitchEdit(shift=[0.0] * 3, target_hz=[0.0] * 3))):
        assert torch.equal(batch(**kw)[0], wav), kw
    assert "hsp_f0_edit_rows_f32" not in seen and "hsp_duration_scaled_f32" not in seen
    assert seen.count("hsp_duration_f32") == 8


def test_return_lf0_is_the_clipped_predictor_track_and_feeds_back(setup, case, device):
    from megatts2_hierspeechpp_amd import _lib as L, inference_plm as IP
    from megatts2_hierspeechpp_amd.prosody_controls import PitchEdit
    models, mel_fn = setup
    ids, tone, lang = _one(case, 1)
    T = TB.FRAMES[1]
    kw = dict(dur=case["dur"][1].reshape(1, -1), noise_seed=NOISE_SEED)
    wav, codes, track = IP.tts_from_prompt(models, mel_fn, ids, tone, lang, case["prompts"][1], plm_causal=True,
                                           return_codes=True, return_lf0=True, **kw)
    assert wav.shape == (320 * T,) and codes.shape == (T,) and track.shape == (4 * T,) and track.dtype == torch.float32
    # the track by hand: the pitch predictor's output, clipped below 55 Hz (inference_plm.py:166)
    ttv_mel, _ = IP.prompt_mels(mel_fn, case["prompts"][1])
    one = lambda v: torch.full((1,), v, dtype=torch.int64, device=device)  # noqa: E731
    x_frame, g, x_lengths, x_mask = models.ttv.inf_extract_tc_latent(ids, one(ids.shape[1]), ttv_mel, one(ttv_mel.shape[2]),
                                                                     tone, lang, dur=kw["dur"])
    _, lf0 = models.ttv.inf_plm_gen(x_frame, g, codes.reshape(1, 1, -1), x_lengths, x_mask)
    assert torch.equal(track, IP.zero_below(lf0, math.log(55.0)).reshape(-1))
    print(f"predicted track: {int((track > 0).sum())} of {4 * T} frames voiced")
    # the editing loop: the same codes and seeds with the track fed back give the take again
    again, track2 = IP.tts_from_prompt(models, mel_fn, ids, tone, lang, case["prompts"][1], prosody_codes=codes, lf0=track,
                                       return_lf0=True, **kw)
    assert torch.equal(again, wav) and torch.equal(track2, track)
    # an edit of the predicted track: the returned track is PitchEdit.apply on the unedited one
    e = PitchEdit(shift=-2.0, range=1.4)
    _, track3 = IP.tts_from_prompt(models, mel_fn, ids, tone, lang, case["prompts"][1], prosody_codes=codes, pitch=e,
                                   return_lf0=True, **kw)
    assert torch.equal(track3, e.apply(track))
    with pytest.raises(L.HspError, match=rf"lf0 must be fp32 \[1, {4 * T}\] \(4 per frame of the {T} frames"):
        IP.tts_from_prompt(models, mel_fn, ids, tone, lang, case["prompts"][1], prosody_codes=codes, lf0=track[:-4], **kw)


def test_an_edit_moves_the_pitch_and_nothing_else(setup, case, device):
    """A given track, then the same take with an edit: the vocoder's track is `PitchEdit.apply` on the given one bit
    for bit, the codes are the take's, and the waveform differs."""
    from megatts2_hierspeechpp_amd import inference_plm as IP
    from megatts2_hierspeechpp_amd.prosody_controls import PitchEdit
    models, mel_fn = setup
    ids, tone, lang = _one(case, 0)
    T = TB.FRAMES[0]
    given = _given_track(4 * T, 1, device)
    kw = dict(dur=case["dur"][0].reshape(1, -1), noise_seed=NOISE_SEED, plm_causal=True, lf0=given, return_codes=True,
              return_lf0=True)
    wav, codes, track = IP.tts_from_prompt(models, mel_fn, ids, tone, lang, case["prompts"][0], **kw)
    assert torch.equal(track, given)
    off = torch.from_numpy(np.linspace(-2.0, 2.0, 4 * T).astype(np.float32))
    seen = []
    for e in (PitchEdit(shift=3.0), PitchEdit(range=0.0), PitchEdit(target_hz=240.0), PitchEdit(offsets=[off]),
              PitchEdit(shift=-1.0, range=1.5, target_hz=120.0, offsets=off.reshape(1, -1), f_min=80.0, f_max=400.0)):
        w, c, t = IP.tts_from_prompt(models, mel_fn, ids, tone, lang, case["prompts"][0], pitch=e, **kw)
        want, mean = e.apply(given, return_mean=True)
        assert torch.equal(t, want) and torch.equal(c, codes)
        assert not torch.equal(t, given) and not torch.equal(w, wav)
        assert w.shape == wav.shape and all(not torch.equal(w, s) for s in seen)
        seen.append(w)
    flat = PitchEdit(range=0.0).apply(given)
    hz = torch.expm1(flat[given > 0].double())
    assert float((hz / float(mean[0]) - 1).abs().max()) <= 1e-6           # every voiced frame at the geometric mean


def _scales_away_from_integers(exp_logw, ls, seed):
    """Phone scales for one line: drawn in [0.5, 2], each stepped by 1 % until its duration -- exp(logw) times the
    folded fp32 factor fl(ls * s), in float64 -- lies at least 1e-2 from an integer.  -> (scales, pre-ceil durations)."""
    r = np.random.default_rng(seed)
    s = r.uniform(0.5, 2.0, exp_logw.shape[0]).astype(np.float32)
    for _ in range(100):
        p = exp_logw * (np.float32(ls) * s).astype(np.float64)
        near = np.abs(p - np.round(p)) < 1e-2
        if not near.any():
            break
        s[near] *= np.float32(1.01)
    return s, p


def test_batch_rows_with_their_own_pitch_and_pace_equal_the_one_line_calls(setup, case, device):
    """Predicted durations, a ``length_scale`` per line and a ``phone_scale`` per phone, a shift and a range per line on
    given tracks.  Condition of the inputs (asserted): every one-line pre-ceil duration, read the way
    `pre_ceil_durations` of tests/test_gpu_tts_batch.py reads it, lies at least 1e-3 from an integer.  Then every row's
    frame count is the sum of the reference ceil of those durations, and row b equals the one-line call with row b's
    values."""
    from megatts2_hierspeechpp_amd import inference_plm as IP
    from megatts2_hierspeechpp_amd.prosody_controls import PitchEdit
    models, mel_fn = setup
    lines, prompts = case["lines"], case["prompts"]
    scales, frames = [], []
    for b in range(3):
        v = TB.pre_ceil_durations(models, mel_fn, lines[b], prompts[b], 1.0, device).cpu().numpy()
        s, p = _scales_away_from_integers(v, LENGTH_SCALE[b], 60 + b)
        dist = float(np.abs(p - np.round(p)).min())
        print(f"line {b}: length_scale {LENGTH_SCALE[b]}, phone scales {np.round(s, 3).tolist()}, minimum distance of a "
              f"pre-ceil duration from an integer {dist:.2e}")
        assert dist >= 1e-3 and s.min() >= 0.25 and s.max() <= 4.0, (b, dist)
        scales.append(s.tolist())
        frames.append(math.ceil(float(np.ceil(p).sum()) / 2))
    assert len(set(frames)) > 1                                            # a ragged batch
    given = [_given_track(4 * f, 10 + b, device) for b, f in enumerate(frames)]
    got = IP.tts_batch(models, mel_fn, lines, prompts, plm_causal=True, noise_seeds=NOISE_SEED, length_scale=LENGTH_SCALE,
                       phone_scale=scales, pitch=PitchEdit(shift=SHIFT, range=RANGE), lf0=given, return_float=True,
                       return_codes=True, return_lf0=True)
    print(f"frames {frames}")
    assert [n // 320 for n in got[1].tolist()] == frames                   # the reference ceil of the pre-ceil durations
    solos = []
    for b in range(3):
        ids, tone, lang = _one(case, b)
        solos.append(IP.tts_from_prompt(models, mel_fn, ids, tone, lang, prompts[b], plm_causal=True,
                                        noise_seed=NOISE_SEED + b, length_scale=LENGTH_SCALE[b], phone_scale=scales[b],
                                        pitch=PitchEdit(shift=SHIFT[b], range=RANGE[b]), lf0=given[b], return_float=True,
                                        return_codes=True, return_lf0=True))
    _rows_equal(got, solos, frames)
    assert torch.equal(got[4][1], given[1])                                # the identity row of the mixed batch
    for b in (0, 2):
        assert torch.equal(got[4][b], PitchEdit(shift=SHIFT[b], range=RANGE[b]).apply(given[b]))
    # the pace took part: the page at scale 1 has other frame counts
    plain = IP.tts_batch(models, mel_fn, lines, prompts, plm_causal=True, noise_seeds=NOISE_SEED)
    assert [n // 320 for n in plain[1].tolist()] != frames
    # a per-line length_scale alone is the float form of every line, frame for frame
    for ls in (1.3,):
        a = IP.tts_batch(models, mel_fn, lines, prompts, plm_causal=True, noise_seeds=NOISE_SEED, length_scale=ls)
        b = IP.tts_batch(models, mel_fn, lines, prompts, plm_causal=True, noise_seeds=NOISE_SEED, length_scale=[ls] * 3)
        assert torch.equal(a[1], b[1]) and torch.equal(a[0], b[0])


def test_tts_lines_chunking_does_not_change_the_rows(setup, device):
    """Five lines at ``max_batch=2`` against ``max_batch=16``: ``pitch`` rows, ``lf0``, ``length_scale`` and
    ``phone_scale`` are sliced per chunk as ``seeds`` are.  Pinned durations (which ``length_scale`` does not scale:
    its slicing is checked, its effect is not) scaled per phone: ceil(dur * scale) is exact, so the frame counts are
    known here."""
    from megatts2_hierspeechpp_amd import inference_plm as IP
    from megatts2_hierspeechpp_amd.prosody_controls import PitchEdit
    models, mel_fn = setup
    lines, prompts, dur, _, _ = TB._five(device)
    r = np.random.default_rng(8)
    scales = [r.choice(np.array([0.5, 1.0, 1.5, 2.0], np.float32), d.numel()).tolist() for d in dur]
    frames = [math.ceil(float(np.ceil(d.cpu().numpy() * np.array(s, np.float32)).sum()) / 2) for d, s in zip(dur, scales)]
    given = [_given_track(4 * f, 40 + k, device) for k, f in enumerate(frames)]
    edit = PitchEdit(shift=[1.0, -2.0, 0.0, 3.0, -1.0], range=torch.tensor([1.0, 0.5, 1.0, 2.0, 1.2]),
                     offsets=[torch.full((4 * f,), 0.25 * k) for k, f in enumerate(frames)])
    kw = dict(dur=dur, plm_causal=True, noise_seeds=NOISE_SEED, pitch=edit, lf0=given, phone_scale=scales,
              length_scale=[1.0, 1.3, 0.8, 2.0, 1.0], return_float=True, return_codes=True, return_lf0=True)
    w16, a16, c16, t16 = IP.tts_lines(models, mel_fn, lines, prompts, max_batch=16, **kw)
    w2, a2, c2, t2 = IP.tts_lines(models, mel_fn, lines, prompts, max_batch=2, **kw)
    assert [w.shape[0] for w in w16] == [320 * f for f in frames] == [w.shape[0] for w in w2]
    for k in range(5):
        assert torch.equal(c16[k], c2[k]) and torch.equal(t16[k], t2[k]), k
        assert torch.equal(t16[k], edit.rows([k]).apply(given[k])), k      # line k's own edit, whatever chunk it is in
        peak = a16[k].abs().max().item()
        assert (a16[k] - a2[k]).abs().max().item() <= 1e-4 * peak, k
        assert (w16[k].to(torch.int32) - w2[k].to(torch.int32)).abs().max().item() <= 5, k
    assert len({t.shape[0] for t in t16}) > 1


def test_vc_rows_with_their_own_edits_equal_vc(device):
    """``vc``: no keyword, None and an identity edit are one waveform.  ``vc_batch(row_exact=True)`` with a shift, a
    range and a target per row: every row's track is bit for bit the track of ``vc`` on the row alone with its values
    and `PitchEdit.apply` on the unedited track; the audio within the bars of tests/test_gpu_row_exact.py."""
    from megatts2_hierspeechpp_amd import inference_vc as IV, synth
    from megatts2_hierspeechpp_amd.Mels_preprocess import MelSpectrogramFixed
    from megatts2_hierspeechpp_amd.prosody_controls import PitchEdit
    from oracle.hsp_oracle import default_config
    models = IV.VcModels(default_config())
    models.load_state_dict({k: torch.from_numpy(synth.synth_tensor(k, tuple(v.shape), 2))
                            for k, v in models.state_dict().items()})
    models.finalize(device)
    mel_fn = MelSpectrogramFixed(sample_rate=16000, n_fft=1280, win_length=1280, hop_length=320, f_min=0, f_max=8000,
                                 n_mels=80, window_fn=torch.hann_window).finalize(device)
    srcs, f0s, prompts, f0t = vc_case(device, [5000, 12000, 8000], [16000], 51)
    solo = lambda b, **kw: IV.vc(models, mel_fn, srcs[b], f0s[b].reshape(1, -1), prompts[0], f0t[0].reshape(1, -1),  # noqa: E731
                                 noise_seed=NOISE_SEED + b, **kw)
    plain = solo(0)
    assert torch.equal(solo(0, pitch=None), plain) and torch.equal(solo(0, pitch=PitchEdit()), plain)
    shift, rng, target = [2.0, 0.0, -4.0], [1.0, 1.0, 0.5], [0.0, 0.0, 150.0]
    edit = PitchEdit(shift=shift, range=rng, target_hz=target)
    T = [s.shape[-1] // 320 for s in srcs]
    kw = dict(noise_seeds=NOISE_SEED, row_exact=True, return_float=True, return_lf0=True)
    _, _, _, before = IV.vc_batch(models, mel_fn, srcs, f0s, prompts[0], f0t[0], **kw)
    wav, n_out, audio, tracks = IV.vc_batch(models, mel_fn, srcs, f0s, prompts[0], f0t[0], pitch=edit, **kw)
    assert tracks.shape == (3, 4 * max(T)) and n_out.tolist() == [320 * t for t in T]
    assert torch.equal(tracks, edit.apply(before, 4 * torch.tensor(T)))
    for b in range(3):
        w1, a1, t1 = solo(b, pitch=PitchEdit(shift=shift[b], range=rng[b], target_hz=target[b] or None),
                          return_float=True, return_lf0=True)
        n = 320 * T[b]
        assert t1.shape == (4 * T[b],) and torch.equal(tracks[b, :4 * T[b]], t1) and not tracks[b, 4 * T[b]:].any(), b
        assert int((t1 > 0).sum()) > T[b]                                  # a voiced row: the edit is heard
        err = _rel(audio[b:b + 1, :, :n], a1)
        print(f"vc row {b}: {T[b]} frames, max |batch - solo| / peak = {err:.3e} (bar 1e-4)")
        assert err <= 1e-4, (b, err)
        assert not audio[b, :, n:].any(), b
        assert (wav[b, :n].int() - w1.reshape(-1).int()).abs().max() <= 8, b
    assert torch.equal(tracks[1], before[1]) and not torch.equal(tracks[0], before[0])
    assert not torch.equal(solo(0, pitch=PitchEdit(shift=2.0)), plain)
