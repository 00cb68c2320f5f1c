"""GPU (-m gpu): prosody codes from recorded speech.

1. hsp_prosody_encode_f32 through the C ABI against the float64 restatement of tests/prosody_ref.py: codes exactly
   equal (every compared pooled frame has a float64 margin >= 1e-3, asserted on a CPU by tests/test_prosody_ref_host.py
   for these same inputs), nothing written outside either output.
2. The model layer: SynthesizerTrn.prosody_codes / extract_tc_latent_code against the reference fixtures of
   tests/golden/prosody/ and against the legacy infer().
3. The harness: tts(prosody_codes=), prosody_from_audio, a captured graph.

    python -m pytest tests/test_gpu_prosody.py -q -m gpu
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import helpers as H
import prosody_ref as R

pytestmark = pytest.mark.gpu

ISENT = -7             # canary of the integer outputs
D, POOL = R.D, R.POOL


@pytest.fixture(scope="module")
def L():
    from megatts2_hierspeechpp_amd import _lib
    return _lib


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _device_weights(w, device, ld=D, bias=True):
    out = {}
    for tag, c in zip(("1a", "1b", "2a", "2b"), R.CONVS):
        out["w" + tag] = _dev(R.pack_taps(w[c + ".weight"], ld).reshape(-1), device)
        out["b" + tag] = _dev(np.asarray(w[c + ".bias"], np.float32), device) if bias else None
    out["embed"] = _dev(np.asarray(w[R.EMBED], np.float32), device)
    return out


def _guarded(B, n, device):
    """An int64 output [B, n] inside a canary-filled buffer: two rows above and below, 8 columns left and right."""
    buf = torch.full((B + 4, n + 16), ISENT, dtype=torch.int64, device=device)
    return buf, buf[2:B + 2, 8:8 + n]


def _untouched(buf, B, n, name):
    c = buf.clone()
    c[2:B + 2, 8:8 + n] = ISENT
    assert bool((c == ISENT).all()), f"{name}: memory outside the output region was written"


def _run(L, device, x, lengths, dw, codes=True, pooled=True, ld=D):
    """x: a device view [B, D, T] with unit time stride -> (codes [B, T] or None, pooled [B, Tp] or None) as numpy."""
    B, Dx, T = x.shape
    Tp = -(-T // POOL)
    lens = _dev(np.asarray(lengths, np.int64), device)
    a = L.ProsodyArgs()
    a.x, a.x_bs, a.x_cs, a.lengths = L.fptr(x), x.stride(0), x.stride(1), L.ptr(lens)
    a.B, a.D, a.T, a.k, a.w_ld, a.bins = B, Dx, T, R.K, ld, dw["embed"].shape[0]
    for tag in ("1a", "1b", "2a", "2b"):
        setattr(a, "w" + tag, L.fptr(dw["w" + tag]))
        setattr(a, "b" + tag, L.fptr(dw["b" + tag]))
    a.embed = L.fptr(dw["embed"])
    cbuf = pbuf = None
    if codes:
        cbuf, cv = _guarded(B, T, device)
        a.codes, a.c_bs = L.ptr(cv), cv.stride(0)
    if pooled:
        pbuf, pv = _guarded(B, Tp, device)
        a.pooled, a.p_bs = L.ptr(pv), pv.stride(0)
    L.check(L.lib().hsp_prosody_encode_f32(ctypes.byref(a), L.stream_ptr()), "hsp_prosody_encode_f32")
    torch.cuda.synchronize()
    out = []
    for buf, n, name in ((cbuf, T, "codes"), (pbuf, Tp, "pooled")):
        if buf is None:
            out.append(None)
            continue
        _untouched(buf, B, n, name)
        out.append(buf[2:B + 2, 8:8 + n].cpu().numpy())
    return out


def _check(L, device, mel, lengths, w, name, **kw):
    want = R.encode(mel[:, :D], lengths, w)
    x = _dev(mel, device)[:, :D]                                       # the strided [:, :20] view of the 80-bin mel
    codes, pooled = _run(L, device, x, lengths, _device_weights(w, device), **kw)
    bad = int((pooled != want["pooled"]).sum())
    print(f"{name}: {want['pooled'].size} pooled frames, {bad} differ; min float64 margin "
          f"{np.nanmin(want['margin']) if np.isfinite(want['margin']).any() else float('nan'):.4f}")
    assert (pooled == want["pooled"]).all(), (name, np.argwhere(pooled != want["pooled"])[:5])
    assert (codes == want["codes"]).all(), name
    return codes, pooled


# ------------------------------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("name", ["ragged", "tile_edge", "t43", "len0"])
def test_kernel_equals_float64_restatement(device, L, name):
    mel, lengths = R.cases()[name]
    codes, pooled = _check(L, device, mel, lengths, R.weights(), name)
    if name == "len0":
        assert (codes[0] == 0).all() and (pooled[0] == 0).all()        # a row of length 0: zeros only
    if name == "ragged":
        assert (codes[4, 0] == pooled[4, 0]) and (codes[4, 1:] == 0).all()   # the one-frame row


def test_kernel_strided_view_equals_contiguous_copy_and_either_output_alone(device, L):
    mel, lengths = R.cases()["t43"]
    w = R.weights()
    dw = _device_weights(w, device)
    full = _dev(mel, device)
    view, copy = full[:, :D], full[:, :D].contiguous()
    assert view.stride(0) == 80 * 43 and copy.stride(0) == D * 43
    cv, pv = _run(L, device, view, lengths, dw)
    cc, pc = _run(L, device, copy, lengths, dw)
    assert (cv == cc).all() and (pv == pc).all()
    c_only, none = _run(L, device, view, lengths, dw, pooled=False)
    assert none is None and (c_only == cv).all()
    none, p_only = _run(L, device, view, lengths, dw, codes=False)
    assert none is None and (p_only == pv).all()
    # packed taps with a leading dimension above D (rows past Cout are padding), and no biases at all
    wide = _device_weights(w, device, ld=24)
    cw, pw = _run(L, device, view, lengths, wide, ld=24)
    assert (cw == cv).all() and (pw == pv).all()
    # a codebook that is not 16-byte aligned takes the kernel with the channel count at run time: same codes
    shifted = dict(dw)
    shifted["embed"] = torch.cat([torch.zeros(1, device=device), dw["embed"].reshape(-1)])[1:].view(R.BINS, D)
    assert shifted["embed"].data_ptr() % 16 == 4
    cs, ps = _run(L, device, view, lengths, shifted)
    assert (cs == cv).all() and (ps == pv).all()
    w0 = {k: v for k, v in w.items() if not k.endswith(".bias")}
    want = R.encode(mel[:, :D], lengths, w0)
    nb = dict(_device_weights(w, device, bias=False))
    m = R.compared_margin(want["margin"], lengths)
    assert m.min() >= R.MIN_MARGIN, m.min()
    c0, p0 = _run(L, device, view, lengths, nb)
    assert (c0 == want["codes"]).all() and (p0 == want["pooled"]).all()


def test_kernel_tie_takes_the_lowest_index(device, L):
    mel, lengths, w2, win, lo, hi = R.tie_case()
    first = lo if lo is not None else win
    _, pooled = _check(L, device, mel, lengths, w2, "tie")
    assert pooled[0, 0] == first and hi not in pooled and (lo is None or win not in pooled)


def test_kernel_pools_the_padding_zero_of_a_straddling_window(device, L):
    mel, lengths, w = R.negative_tail_case()
    _check(L, device, mel, lengths, w, "negative_tail")


def test_kernel_agrees_with_the_unfused_search_bit_for_bit(device, L):
    """hsp_vq_nearest_f32 and the fused kernel share one distance function: with identity taps (1 at the centre tap, no
    bias) q is exactly the max-pooled input, so both kernels search the same q and must return the same codes."""
    r = np.random.default_rng(3)
    w = R.weights()
    eye = np.zeros((D, D, R.K), np.float32)
    eye[np.arange(D), np.arange(D), 2] = 1.0
    for c in R.CONVS:
        w[c + ".weight"], w[c + ".bias"] = eye, np.zeros(D, np.float32)
    x = r.standard_normal((2, D, 48)).astype(np.float32)
    lengths = np.array((48, 48), np.int64)
    xd = _dev(x, device)
    codes, pooled = _run(L, device, xd, lengths, _device_weights(w, device))
    q = xd.reshape(2, D, 6, POOL).amax(-1).contiguous()
    out = torch.empty(2, 6, dtype=torch.int64, device=device)
    L.check(L.lib().hsp_vq_nearest_f32(L.fptr(q), q.stride(0), q.stride(1), L.fptr(_dev(w[R.EMBED], device)), L.ptr(out),
                                       out.stride(0), 2, D, 6, R.BINS, 1, 6, L.stream_ptr()), "hsp_vq_nearest_f32")
    assert (out.cpu().numpy() == pooled).all()


# --------------------------------------------------------------------------------------------- 2. the model layer
@pytest.fixture(scope="module")
def ttv(device):
    from megatts2_hierspeechpp_amd import synth
    from megatts2_hierspeechpp_amd.hip_layers import finalize
    from megatts2_hierspeechpp_amd.ttv_v1.t2w2v_transformer import SynthesizerTrn
    mod = SynthesizerTrn(126, 11, 4, 641, 320, 16000, 60, **H.TTV_MODEL)
    mod.load_state_dict({k: torch.from_numpy(synth.synth_tensor(k, tuple(v.shape), 7)) for k, v in mod.state_dict().items()})
    finalize(mod, device)
    return mod


def test_prosody_codes_ragged_batch_equals_rows_alone(device, ttv):
    mel, lengths = R.cases()["ragged"]
    want = R.encode(mel[:, :D], lengths, R.weights())
    md, ld = _dev(mel, device), _dev(lengths, device)
    codes, pooled = ttv.prosody_codes(md, ld), ttv.prosody_codes(md, ld, pooled=True)
    assert codes.dtype == torch.int64 and codes.shape == (7, 200) and pooled.shape == (7, 25)
    assert (codes.cpu().numpy() == want["codes"]).all() and (pooled.cpu().numpy() == want["pooled"]).all()
    for b, n in enumerate(lengths):
        alone = ttv.prosody_codes(md[b:b + 1, :, :n].contiguous(), ld[b:b + 1])
        assert torch.equal(alone[0], codes[b, :n]), b
    from megatts2_hierspeechpp_amd._lib import HspError
    for bad_mel, bad_len in ((md[:, :10], ld), (md, ld[:3]), (md[:, :, :0], ld)):   # refused before the launch
        with pytest.raises(HspError):
            ttv.prosody_codes(bad_mel, bad_len)


@pytest.mark.parametrize("name", ["ttv_infer_n8", "ttv_infer_n12"])
def test_prosody_codes_equal_the_legacy_infer_codes(device, ttv, name):
    meta, arrays = H.load_fixture(name)
    assert meta["seed"] == 7 and meta["prefix"] == ""
    d = lambda k: _dev(arrays[k], device)
    n, tm = arrays["ids"].shape[1], arrays["mel"].shape[2]
    dl = lambda v: torch.tensor(v, dtype=torch.int64, device=device)
    w2v, lf0, codes = ttv.infer(d("ids"), dl([n]), d("mel"), dl([tm]), d("tone"), d("language"), dur=d("dur"), return_codes=True)
    mine = ttv.prosody_codes(d("mel"), dl([tm]))
    want = R.encode(arrays["mel"][:, :D], [tm], R.weights())
    assert R.compared_margin(want["margin"], [tm]).min() >= R.MIN_MARGIN
    assert torch.equal(codes, mine) and (mine.cpu().numpy() == want["codes"]).all()
    ref = H.outputs(arrays)
    assert np.abs(w2v.cpu().numpy() - ref[0]).max() <= H.tol_for(ref[0])


def _fixture(name):
    z = np.load(os.path.join(R.GOLDEN, name + ".npz"))
    return json.loads(bytes(z["meta"]).decode()), {k: z[k] for k in z.files if k != "meta"}


def _extract(ttv, a, device, rows=slice(None)):
    d = lambda k: _dev(a[k][rows], device)
    return ttv.extract_tc_latent_code(d("ids"), d("lengths"), d("mel_spk"), d("mel_spk_lengths"), d("tone"), d("language"),
                                      d("dur"), d("mrte_mel"), d("mrte_mel_lengths"))


@pytest.mark.parametrize("name", ["tc_code_t40", "tc_code_t64", "tc_code_b3", "tc_code_b2"])
def test_extract_tc_latent_code_against_the_reference(device, ttv, name):
    meta, a = _fixture(name)
    assert meta["seed"] == 7 and np.nanmin(a["margin"]) >= R.MIN_MARGIN
    x_frame, lr_codes = _extract(ttv, a, device)
    assert lr_codes.dtype == torch.int64 and (lr_codes.cpu().numpy() == a["lr_codes"]).all()
    got, ref = x_frame.cpu().numpy(), a["x_frame"]
    err, tol = float(np.abs(got - ref).max()), H.tol_for(ref)
    print(f"{name}: x_frame max|hip - reference| = {err:.3e} (bar {tol:.1e})")
    assert got.shape == ref.shape and err <= tol
    B = a["ids"].shape[0]
    for b in range(B if B > 1 else 0):                                 # a ragged call, row by row against B = 1 calls
        n, tm, tr, f = (int(a[k][b]) for k in ("lengths", "mel_spk_lengths", "mrte_mel_lengths", "frames"))
        one = {k: v[b:b + 1] for k, v in a.items()}
        one.update(ids=one["ids"][:, :n], tone=one["tone"][:, :n], language=one["language"][:, :n], dur=one["dur"][:, :n],
                   mel_spk=one["mel_spk"][:, :, :tm], mrte_mel=one["mrte_mel"][:, :, :tr])
        xf1, c1 = _extract(ttv, one, device)
        assert torch.equal(c1[0], lr_codes[b, :tm]), (name, b)
        e = float((xf1[0] - x_frame[b, :, :f]).abs().max())
        assert xf1.shape[2] == f and e <= H.tol_for(ref[b]), (name, b, e)
        assert float(x_frame[b, :, f:].abs().max()) == 0.0 if f < x_frame.shape[2] else True


def test_score_runs_on_the_mirror_outputs(device, ttv):
    from megatts2_hierspeechpp_amd import synth
    from megatts2_hierspeechpp_amd.hip_layers import finalize
    from megatts2_hierspeechpp_amd.ttv_v1.t2w2v_transformer import Megatts2PLM1
    plm = Megatts2PLM1()
    plm.load_state_dict({k: torch.from_numpy(synth.synth_tensor("plm." + k, tuple(v.shape), 7)) for k, v in plm.state_dict().items()})
    finalize(plm, device)
    _, a = _fixture("tc_code_t64")
    x_frame, lr_codes = _extract(ttv, a, device)
    assert x_frame.shape[2] == lr_codes.shape[1] == 64
    lg = plm.score(x_frame, lr_codes, torch.tensor([64], dtype=torch.int64))
    assert lg.shape == (1, 64, 1024) and bool(torch.isfinite(lg).all())


def test_prosody_codes_under_a_captured_graph(device, ttv):
    mel, lengths = R.cases()["tile_edge"]
    md, ld = _dev(mel, device), _dev(lengths, device)
    eager = ttv.prosody_codes(md, ld)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ttv.prosody_codes(md, ld)
    out.fill_(ISENT)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    other, _ = R.cases()["ragged"]
    md.copy_(_dev(other[:4, :, :md.shape[2]], device))                 # a replay reads the new mel, no host step between
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ttv.prosody_codes(md, ld)) and not torch.equal(out, eager)


# -------------------------------------------------------------------------------------------------- 3. the harness
@pytest.fixture(scope="module")
def tts_setup(device):
    from megatts2_hierspeechpp_amd import inference_plm as IP, synth
    from megatts2_hierspeechpp_amd.Mels_preprocess import MelSpectrogramFixed
    from oracle.hsp_oracle import default_config
    models = IP.TtsModels(default_config(), H.TTV_MODEL)
    models.load_state_dict({k: torch.from_numpy(synth.synth_tensor(k, tuple(v.shape), 7)) for k, v in models.state_dict().items()})
    models.finalize(device)
    mel_fn = MelSpectrogramFixed(sample_rate=16000, n_fft=1280, win_length=1280, hop_length=320, f_min=0, f_max=8000,
                                 n_mels=80, window_fn=torch.hann_window).finalize(device)
    r = np.random.default_rng(12)
    N, Tm = 9, 64
    ids = _dev(r.integers(12, 113, (1, N)), device)
    tone = _dev(r.integers(0, 11, (1, N)), device)
    lang = torch.where(ids < 74, 1, 2)
    tl = torch.full((1,), N, dtype=torch.int64, device=device)
    mel = _dev(synth.synth_inputs(1, Tm, seed=4)["mel"], device)
    ml = torch.full((1,), Tm, dtype=torch.int64, device=device)
    dur = torch.full((1, N), 4.0, device=device)
    noise = _dev(r.standard_normal((1, 192, N * 2)).astype(np.float32), device)
    args = (ids, tl, tone, lang, mel, ml, torch.cat([mel, mel]), torch.cat([ml, ml]))
    return IP, models, mel_fn, args, dict(dur=dur, noise=noise)


def test_tts_with_given_prosody_codes(device, tts_setup):
    IP, models, mel_fn, args, kw = tts_setup
    ids, tl, tone, lang, mel, ml, mel2, ml2 = args
    given = models.ttv.prosody_codes(mel, ml)                          # 64 frames of codes for an 18-frame utterance
    wav, audio, codes = IP.tts(models, *args, prosody_codes=given, return_codes=True, return_float=True, **kw)
    x_frame, g, x_lengths, x_mask = models.ttv.inf_extract_tc_latent(ids, tl, mel, ml, tone, lang, dur=kw["dur"])
    T2 = x_frame.shape[2]
    fitted = IP.fit_prosody_codes(given, 64, T2)
    assert T2 == 18 and torch.equal(codes, fitted)
    assert (fitted.cpu().numpy() == R.fit_codes(given.cpu().numpy(), [64], [T2], T2)).all()
    wav_h, audio_h = IP.tts_from_codes(models, x_frame, g, fitted, x_lengths, x_mask, mel2, ml2, noise=kw["noise"],
                                       return_float=True)
    assert torch.equal(wav, wav_h) and torch.equal(audio, audio_h)
    # prosody_lengths: only the first 40 frames of the given codes count
    part = IP.tts(models, *args, prosody_codes=given, prosody_lengths=torch.tensor([40], device=device), return_codes=True,
                  **kw)[1]
    assert torch.equal(part, IP.fit_prosody_codes(given[:, :40], 40, T2))
    # round trip: the PLM's own codes, handed back, reproduce the same int16 audio with the same noise
    wav_p, codes_p = IP.tts(models, *args, return_codes=True, **kw)
    wav_r, codes_r = IP.tts(models, *args, prosody_codes=codes_p, return_codes=True, **kw)
    assert wav_p.dtype == torch.int16 and torch.equal(codes_r, codes_p) and torch.equal(wav_r, wav_p)
    assert not torch.equal(wav, wav_p)                                  # other codes, other audio


def test_prosody_from_audio(device, tts_setup):
    IP, models, mel_fn, args, kw = tts_setup
    r = np.random.default_rng(13)
    t = np.arange(24000) / 16000.0
    audio = _dev(np.stack([0.3 * np.sin(2 * np.pi * f * t) + 0.05 * r.standard_normal(24000) for f in (140.0, 210.0)])
                 .astype(np.float32), device)
    codes, frames = IP.prosody_from_audio(models, mel_fn, audio)
    mel = mel_fn(audio)
    assert codes.shape == (2, mel.shape[2]) and frames.tolist() == [75, 75] and frames.dtype == torch.int64
    assert torch.equal(codes, models.ttv.prosody_codes(mel, frames))
    lens = torch.tensor([24000, 16000], dtype=torch.int64, device=device)
    codes_r, frames_r = IP.prosody_from_audio(models, mel_fn, audio, lengths=lens)
    assert frames_r.tolist() == [75, 50] and torch.equal(codes_r[0], codes[0]) and bool((codes_r[1, 50:] == 0).all())
    one = IP.prosody_from_audio(models, mel_fn, audio[1, :16000].contiguous())[0]
    assert torch.equal(one[0], codes_r[1, :50])
    # another rate: resampled to 16 kHz first
    c8, f8 = IP.prosody_from_audio(models, mel_fn, audio[:, ::2].contiguous(), sr=8000)
    assert c8.shape == (2, 75) and f8.tolist() == [75, 75]
