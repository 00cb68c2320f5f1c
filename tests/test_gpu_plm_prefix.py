"""GPU checks of prosody-LM decoding behind a given code prefix: hsp_plm_prefill_attn_f32 against its header contract in
float64, the caches PlmDecodeSession.admit(prefix_codes=) leaves, Megatts2PLM1.infer(prefix_codes=) and infer_many(prefixes=)
against the float64 forced-prefix decode (tests/plm_prefix_ref.py) and against each other, sampling, slot reuse, the TTS
harness and the refusals.  Every float comparison: at most 1e-4 of the reference's range; codes are compared exactly."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import plm_causal_ref as R  # noqa: E402
import plm_prefix_ref as PR  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-4


@pytest.fixture(scope="module")
def plm(device):
    from megatts2_hierspeechpp_amd import synth
    from megatts2_hierspeechpp_amd.ttv_v1.t2w2v_transformer import Megatts2PLM1
    m = Megatts2PLM1()
    m.load_state_dict({k: torch.from_numpy(synth.synth_tensor("plm." + k, tuple(v.shape), 7))
                       for k, v in m.state_dict().items()})
    m.finalize(device)
    return m


def _close(got, want, what=""):
    want = np.asarray(want)
    err, rng = np.abs(np.asarray(got, np.float64) - want).max(), np.abs(want).max()
    print(f"{what}: max err {err:.3e}, range {rng:.3e}, ratio {err / rng:.2e}")
    assert err <= TOL * rng, (what, err, rng)


def _bytes(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


def _i64(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(device)


# ------------------------------------------------------------------------------------------- 1. kernel contract
CANARY = 7.0


def _prefill_call(L, qkv, out, kc, vc, n, D, H):
    a = L.PlmPrefillAttnArgs()
    a.qkv, a.q_rs = L.fptr(qkv), qkv.stride(0)
    a.out, a.o_rs = (L.fptr(out), out.stride(0)) if out is not None else (None, 0)
    a.k_cache, a.v_cache, a.cs = L.fptr(kc), L.fptr(vc), kc.stride(0)
    a.n, a.D, a.H, a.debug = n, D, H, 0
    L.check(L.lib().hsp_plm_prefill_attn_f32(ctypes.byref(a), L.stream_ptr()), "hsp_plm_prefill_attn_f32")
    torch.cuda.synchronize()


def _contract(device, D, H, n):
    from megatts2_hierspeechpp_amd import _lib as L
    assert L.lib().hsp_plm_prefill_attn_supported(D, H) == 1
    r = np.random.default_rng(1000 * H + n)
    q_rs, o_rs, Tp, S = n + 5, n + 3, n + 6, 3                       # pitches above n; the row is slot 1 of 3 in the caches
    qkv_np = r.standard_normal((3 * D, q_rs)).astype(np.float32)
    qkv_np[:D] *= 2.0                                                 # scores of a few units: a softmax that is not flat
    qkv_np[:, n:] = np.nan                                            # columns >= n are never read
    kc_np = r.standard_normal((D, S, Tp)).astype(np.float32)          # the other slots and columns < n: must be kept / overwritten
    vc_np = r.standard_normal((D, S, Tp)).astype(np.float32)
    kc_np[:, :, n:] = np.nan
    vc_np[:, :, n:] = np.nan
    dev = lambda a: torch.from_numpy(a).to(device)
    qkv = dev(qkv_np)
    obuf = torch.full((D + 2, o_rs), CANARY, device=device)           # out between canaries: a row above, one below, columns >= n
    out = obuf[1:D + 1]
    kc, vc = dev(kc_np), dev(vc_np)
    _prefill_call(L, qkv, out, kc[:, 1], vc[:, 1], n, D, H)
    want = PR.prefill_attn(qkv_np, n, D, H)
    got, got_k, got_v = obuf.cpu().numpy(), kc.cpu().numpy(), vc.cpu().numpy()
    assert np.isfinite(got[1:D + 1, :n]).all()
    _close(got[1:D + 1, :n], want, f"out D={D} H={H} n={n}")
    _close(got_k[:, 1, :n], qkv_np[D:2 * D, :n].astype(np.float64), f"k D={D} H={H} n={n}")
    _close(got_v[:, 1, :n], qkv_np[2 * D:, :n].astype(np.float64), f"v D={D} H={H} n={n}")
    # nothing outside was written, bit for bit (NaN columns included); qkv is unchanged
    assert (got[0] == CANARY).all() and (got[D + 1] == CANARY).all() and (got[1:D + 1, n:] == CANARY).all()
    for g, w in ((got_k, kc_np), (got_v, vc_np)):
        assert g[:, [0, 2]].tobytes() == w[:, [0, 2]].tobytes()
        assert g[:, 1, n:].tobytes() == w[:, 1, n:].tobytes()
    assert _bytes(qkv) == qkv_np.tobytes()
    # out = NULL: the caches alone, with the same bits
    k2, v2 = dev(kc_np), dev(vc_np)
    _prefill_call(L, qkv, None, k2[:, 1], v2[:, 1], n, D, H)
    assert _bytes(k2) == got_k.tobytes() and _bytes(v2) == got_v.tobytes()
    assert _bytes(qkv) == qkv_np.tobytes()


@pytest.mark.parametrize("n", [1, 3, 4, 5, 16, 17, 63, 64, 65, 130, 256, 257])
def test_prefill_attn_contract(device, n):
    """The sizes where a 16-query tile, a 64-key block or a wave boundary starts or ends."""
    _contract(device, 276, 4, n)


@pytest.mark.parametrize("n", [1, 7, 64, 131])
def test_prefill_attn_contract_second_geometry(device, n):
    """8 heads of 8 channels: fewer head channels than channel groups of the p V step."""
    _contract(device, 64, 8, n)


def test_prefill_attn_column_does_not_depend_on_n(device):
    """include/hsp.h: column i of out depends on columns 0 .. i alone -- the call for n = 40 gives the first 40 columns
    of the call for n = 130, bit for bit."""
    from megatts2_hierspeechpp_amd import _lib as L
    D, H = 276, 4
    r = np.random.default_rng(5)
    qkv = torch.from_numpy(r.standard_normal((3 * D, 132)).astype(np.float32)).to(device)
    outs = []
    for n in (130, 40):
        out, kc, vc = (torch.zeros(D, 132, device=device) for _ in range(3))
        _prefill_call(L, qkv, out, kc, vc, n, D, H)
        outs.append(out)
    assert _bytes(outs[0][:, :40]) == _bytes(outs[1][:, :40])


# ------------------------------------------------------------------------------ 2. caches after admit(prefix_codes=)
def test_admit_prefills_the_slots_caches(device, plm):
    case = (17, 24, 9119)
    P, T, _ = case
    tc_np, prefix, _, _, _, kv64 = PR.foreign(case)
    ses = plm.decode_session(3, T)
    for kc, vc in ses.kv:
        kc.fill_(float("nan"))
        vc.fill_(float("nan"))
    ses.admit(1, torch.from_numpy(tc_np[0]).to(device), prefix_codes=_i64(prefix, device))
    torch.cuda.synchronize()
    assert ses.pos.cpu().tolist() == [-1, P, -1] and ses.len.cpu().tolist()[1] == T and ses._left == [0, T - P, 0]
    assert ses.codes[1, :P + 1].cpu().tolist() == [plm.GO_ID] + prefix.tolist()
    for l, ((kc, vc), (k64, v64)) in enumerate(zip(ses.kv, kv64)):
        for name, got, want in (("k", kc, k64), ("v", vc, v64)):
            g = got.cpu().numpy()
            _close(g[:, 1, :P], want[0, :, :P], f"layer {l} {name} cache")
            assert np.isnan(g[:, [0, 2]]).all() and np.isnan(g[:, 1, P:]).all()   # untouched: still the NaN fill


# ------------------------------------------------------------------------------------------- 3. foreign prefixes
@pytest.mark.parametrize("case", PR.FOREIGN_CASES, ids=lambda c: f"P{c[0]}-T{c[1]}")
def test_infer_behind_a_foreign_prefix_equals_float64(device, plm, case):
    P, T, _ = case
    tc_np, prefix, want_codes, want_logits, _, _ = PR.foreign(case)
    tc, pre = torch.from_numpy(tc_np).to(device), _i64(prefix[None], device)
    codes, logits = plm.infer(tc, return_logits=True, causal=True, prefix_codes=pre)
    assert codes.shape == (1, T) and codes.dtype == torch.int64 and logits.shape == (1, T - P, 1024)
    _close(logits.cpu().numpy(), want_logits[:, P:], f"logits behind the prefix {case}")
    assert np.array_equal(codes.cpu().numpy(), want_codes)
    assert torch.equal(codes[:, :P], pre)
    assert torch.equal(plm.infer(tc, causal=True, prefix_codes=pre), codes)


# ------------------------------------------------------------------------------------------------ 4. own prefixes
def _many(plm, reqs, **kw):
    """infer_many, and the session it made."""
    made, orig = [], plm.decode_session
    plm.decode_session = lambda *a, **k: (made.append(orig(*a, **k)), made[-1])[1]
    try:
        out = plm.infer_many(reqs, **kw)
    finally:
        del plm.decode_session
    torch.cuda.synchronize()
    assert len(made) == 1
    return out, made[0]


def _own(device, shape):
    tc_np, want_codes, _, _ = R.decoded(shape)
    Ps = PR.OWN_CASES[shape]
    reqs = [torch.from_numpy(tc_np[i].copy()).to(device) for i in range(shape[0])]
    pres = [_i64(want_codes[i, :p], device) for i, p in enumerate(Ps)]
    return reqs, pres, want_codes, Ps


@pytest.fixture(scope="module")
def solo13(device, plm):
    reqs, pres, want, _ = _own(device, (5, 13))
    solo = [plm.infer(q[None], causal=True, prefix_codes=p[None])[0] for q, p in zip(reqs, pres)]
    for s, w in zip(solo, want):
        assert np.array_equal(s.cpu().numpy(), w)
    return solo


@pytest.mark.parametrize("capture", [True, False], ids=["captured", "eager"])
@pytest.mark.parametrize("slots", [2, 8])
def test_session_behind_own_prefixes(device, plm, solo13, slots, capture):
    from megatts2_hierspeechpp_amd.ttv_v1.t2w2v_transformer import session_plan
    reqs, pres, want, Ps = _own(device, (5, 13))
    out, ses = _many(plm, reqs, slots=slots, capture=capture, prefixes=pres)
    for i, (o, s) in enumerate(zip(out, solo13)):
        assert o.dtype == torch.int64 and o.shape == (13,)
        assert np.array_equal(o.cpu().numpy(), want[i]), i
        assert torch.equal(o, s), i
    steps = session_plan([13 - p for p in Ps], slots)[1]
    assert steps == {2: 18, 8: 12}[slots] and ses.steps == steps
    assert (ses.captures, ses.replays) == ((1, steps) if capture else (0, 0))
    assert ses.pos.cpu().tolist() == [-1] * slots
    # a list mixing None and prefixes
    mixed = [pres[0], None, pres[2], None, pres[4]]
    out2, ses2 = _many(plm, reqs, slots=slots, capture=capture, prefixes=mixed)
    for i, o in enumerate(out2):
        assert np.array_equal(o.cpu().numpy(), want[i]), i
    assert ses2.steps == session_plan([13 - (p.shape[0] if p is not None else 0) for p in mixed], slots)[1]


def test_session_behind_long_own_prefixes(device, plm):
    """P = 256 (four whole key blocks, sixteen query tiles) and P = 64 of 260: the decode crosses the 256-key mark of the
    decode kernel right behind the prefill."""
    from megatts2_hierspeechpp_amd.ttv_v1.t2w2v_transformer import session_plan
    reqs, pres, want, Ps = _own(device, (2, 260))
    out, ses = _many(plm, reqs, slots=2, prefixes=pres)
    for i, o in enumerate(out):
        assert np.array_equal(o.cpu().numpy(), want[i]), i
        assert torch.equal(o, plm.infer(reqs[i][None], causal=True, prefix_codes=pres[i][None])[0]), i
    assert ses.steps == session_plan([260 - p for p in Ps], 2)[1] == 196


# ---------------------------------------------------------------------------------------------------- 5. sampling
def test_sampled_session_behind_prefixes_equals_solo_runs(device, plm):
    from megatts2_hierspeechpp_amd.ttv_v1.t2w2v_transformer import PlmSampling
    sp = PlmSampling(temperature=1.1, top_k=40, top_p=0.95, repetition_penalty=1.2)
    tc_np = R.case_tc((3, 20), [71, 72, 73])
    lengths, seeds, Ps = [20, 7, 12], [5, 2 ** 40 + 3, -9], [9, 3, None]
    reqs = [torch.from_numpy(tc_np[i, :, :n].copy()).to(device) for i, n in enumerate(lengths)]
    pres = [None if p is None else _i64(PR.foreign_prefix(p), device) for p in Ps]
    out, _ = _many(plm, reqs, slots=2, sampling=sp, seeds=seeds, prefixes=pres)
    for i, q in enumerate(reqs):
        sd = torch.tensor([seeds[i]], dtype=torch.int64, device=device)
        solo = plm.infer(q[None], sampling=sp, seeds=sd, causal=True, prefix_codes=None if pres[i] is None else pres[i][None])[0]
        assert torch.equal(out[i], solo), i
        if pres[i] is not None:
            assert torch.equal(out[i][:Ps[i]], pres[i])
    other, _ = _many(plm, reqs, slots=2, sampling=sp, seeds=[s + 1000 for s in seeds], prefixes=pres)
    assert torch.equal(other[0][:9], out[0][:9]) and not torch.equal(other[0][9:], out[0][9:])   # other seeds, other tails


# -------------------------------------------------------------------------------------------------- 6. slot reuse
def test_a_reused_slot_admits_a_prefix_cleanly(device, plm, solo13):
    """One slot: the first request (latent scaled by 1e3, and longer) poisons the slot's caches and codes; the second is
    admitted with a prefix and must equal its solo run."""
    reqs, pres, _, Ps = _own(device, (5, 13))
    second, pre = reqs[3][:, :10].contiguous(), pres[3]                         # 10 frames, its own first 4 codes given
    alone = plm.infer(second[None], causal=True, prefix_codes=pre[None])[0]
    assert torch.equal(alone, solo13[3][:10])                                   # causal: a row cut in time keeps its codes
    out, ses = _many(plm, [reqs[0] * 1e3, second], slots=1, prefixes=[None, pre])
    assert ses.steps == 13 + (10 - 4)
    assert torch.equal(out[1], alone) and torch.equal(out[1][:4], pre)
    assert not torch.equal(out[0][:10], alone)


# ----------------------------------------------------------------------------------------------------- 7. harness
def test_tts_with_a_prefix_equals_hand_composition(device):
    from megatts2_hierspeechpp_amd import inference_plm as IP, synth
    from megatts2_hierspeechpp_amd.ttv_v1.t2w2v_transformer import PlmSampling
    from oracle.hsp_oracle import default_config
    import helpers as Hh
    models = IP.TtsModels(default_config(), Hh.TTV_MODEL)
    models.load_state_dict({k: torch.from_numpy(synth.synth_tensor(k, tuple(v.shape), 7)) for k, v in models.state_dict().items()})
    models.finalize(device)
    r = np.random.default_rng(11)
    B, N, Tm = 2, 9, 40
    ids = torch.from_numpy(r.integers(12, 113, (B, N))).to(device)
    tone = torch.from_numpy(r.integers(0, 11, (B, N))).to(device)
    lang = torch.where(ids < 74, 1, 2)
    tl = torch.full((B,), N, dtype=torch.int64, device=device)
    mel = torch.from_numpy(synth.synth_inputs(B, Tm, seed=3)["mel"]).to(device)
    ml = torch.full((B,), Tm, dtype=torch.int64, device=device)
    dur = torch.full((B, N), 4.0, device=device)
    noise = torch.from_numpy(r.standard_normal((B, 192, N * 2)).astype(np.float32)).to(device)
    mel2, ml2 = torch.cat([mel, mel]), torch.cat([ml, ml])
    kw = dict(dur=dur, noise=noise, return_float=True)
    p = _i64(r.integers(0, 1024, (B, 7)), device)
    wav, audio, codes = IP.tts(models, ids, tl, tone, lang, mel, ml, mel2, ml2, plm_causal=True, plm_prefix=p,
                               return_codes=True, **kw)
    x_frame, g, x_lengths, x_mask = models.ttv.inf_extract_tc_latent(ids, tl, mel, ml, tone, lang, dur=dur)
    codes_h = models.plm.infer(x_frame, causal=True, prefix_codes=p)
    wav_h, audio_h = IP.tts_from_codes(models, x_frame, g, codes_h, x_lengths, x_mask, mel2, ml2, noise=noise, return_float=True)
    assert torch.equal(codes, codes_h) and torch.equal(wav, wav_h) and torch.equal(audio, audio_h)
    assert codes.shape == (B, x_frame.shape[2]) and torch.equal(codes[:, :7], p)
    # return_codes without a prefix and without return_float: (wav, codes); the codes are those of the plain call
    wav_c, codes_c = IP.tts(models, ids, tl, tone, lang, mel, ml, mel2, ml2, plm_causal=True, return_codes=True, dur=dur,
                            noise=noise)
    assert torch.equal(codes_c, models.plm.infer(x_frame, causal=True))
    assert torch.equal(wav_c, IP.tts(models, ids, tl, tone, lang, mel, ml, mel2, ml2, plm_causal=True, dur=dur, noise=noise))
    # takes = 3 with one prefix: three rows that all start with it
    from megatts2_hierspeechpp_amd.Mels_preprocess import MelSpectrogramFixed
    mel_fn = MelSpectrogramFixed(sample_rate=16000, n_fft=1280, win_length=1280, hop_length=320, f_min=0, f_max=8000,
                                 n_mels=80, window_fn=torch.hann_window).finalize(device)
    t = np.arange(20000) / 16000.0
    prompt = torch.from_numpy((0.3 * np.sin(2 * np.pi * 140 * t) + 0.05 * r.standard_normal(20000))
                              .astype(np.float32)[None]).to(device)
    sp = PlmSampling(temperature=1.0, top_k=50)
    one = p[0, :5]
    wavs, codes3 = IP.tts_from_prompt(models, mel_fn, ids[:1], tone[:1], lang[:1], prompt, dur=dur[:1], noise=noise[:1], plm_sampling=sp, seed=3,
                                      takes=3, plm_causal=True, plm_prefix=one, return_codes=True)
    assert wavs.shape[0] == 3 and codes3.shape[0] == 3 and codes3.dtype == torch.int64
    assert all(torch.equal(codes3[k, :5], one) for k in range(3))


# ------------------------------------------------------------------------------------------------------- 8. time
def test_prefill_of_150_positions_is_below_150_steps_of_the_loop(device, plm):
    """the loop without this feature takes 155.4 us per step at 1 x 200 (the parent commit's
    tools/plm_causal_bench.py), so stepping through a 150-frame prefix is 23.31 ms before the first new code; the prefill
    of the same prefix was measured at 0.35 ms.  Asserted against the measured 23.31 ms, not against a ratio."""
    T, P = 200, 150
    tc = torch.randn(256, T, generator=torch.Generator().manual_seed(1)).to(device)
    pre = _i64(PR.foreign_prefix(P), device)
    Tp = (T + 3) & ~3
    rows = [(torch.empty(plm.d_model, Tp, device=device), torch.empty(plm.d_model, Tp, device=device)) for _ in plm.plm.layers]
    times = []
    for rep in range(8):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        plm.prefill(tc, pre, rows)
        e1.record()
        torch.cuda.synchronize()
        if rep >= 3:
            times.append(e0.elapsed_time(e1))
    med = sorted(times)[len(times) // 2]
    print(f"prefill({P}) median of 5: {med:.3f} ms (all: {[round(t, 3) for t in times]}); 150 steps of the loop: 23.31 ms")
    assert med < 23.31


# ---------------------------------------------------------------------------------------------------- 9. refusals
def test_prefix_refusals(device, plm):
    from megatts2_hierspeechpp_amd import inference_plm as IP
    from megatts2_hierspeechpp_amd._lib import HspError
    T = 8
    tc = torch.from_numpy(R.case_tc((2, T), [1, 2])).to(device)
    ok = torch.zeros(2, 3, dtype=torch.int64, device=device)
    bad = [ok[:, :0],                                                       # P = 0 columns
           torch.zeros(2, T, dtype=torch.int64, device=device),             # P >= T
           torch.zeros(2, T + 1, dtype=torch.int64, device=device),
           ok.to(torch.int32), ok.to(torch.float32),                        # wrong dtype
           ok + 1024, ok - 1,                                               # a code out of range (the go id included)
           ok[0], ok[:1]]                                                   # not [B, P]
    for p in bad:
        with pytest.raises(HspError):
            plm.infer(tc, causal=True, prefix_codes=p)
    with pytest.raises(HspError):
        plm.infer(tc, causal=False, prefix_codes=ok)                         # the bidirectional loop keeps nothing
    with pytest.raises(HspError):
        plm.infer(tc, prefix_codes=ok)
    with pytest.raises(HspError):                                            # plm_prefix without plm_causal: refused first
        IP.tts(None, None, None, None, None, None, None, None, None, plm_prefix=ok)
    ses = plm.decode_session(2, T)
    for p in (ok[0, :0], torch.zeros(T, dtype=torch.int64, device=device), ok[0].to(torch.int32), ok[0] + 1024, ok):
        with pytest.raises(HspError):
            ses.admit(0, tc[0], prefix_codes=p)
        assert not ses.busy(0)                                               # a refused admission leaves the slot free
    ses.admit(0, tc[0], prefix_codes=ok[0])
    with pytest.raises(HspError):
        ses.admit(0, tc[0], prefix_codes=ok[0])                              # a busy slot
    with pytest.raises(HspError):
        plm.infer_many([tc[0], tc[1]], slots=2, prefixes=[ok[0]])            # one prefix entry per request
    with pytest.raises(HspError):
        plm.infer_many([tc[0], tc[1]], slots=2, prefixes=[ok[0], torch.zeros(T, dtype=torch.int64, device=device)])
    torch.cuda.synchronize()
