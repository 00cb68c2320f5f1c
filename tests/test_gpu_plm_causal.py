"""GPU checks of causal prosody-LM decoding: hsp_plm_decode_layer_f32 against its header contract, Megatts2PLM1.score and
infer(causal=True) against the float64 restatement (tests/plm_causal_ref.py), sampling, graph capture and the TTS harness.
Every float comparison: at most 1e-4 of the reference's range."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import plm_causal_ref as R  # noqa: E402
import plm_sampling_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-4
D, H, F = 276, 4, 1104


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


# ------------------------------------------------------------------------------------------- 1. kernel contract
class _Layer:
    """Random weights of one layer: float64 masters (rounded to float32 first) + the device operands of the kernel."""

    def __init__(self, device, seed=1, D=D, H=H, F=F):
        self.D, self.H, self.F = D, H, F
        r = np.random.default_rng(seed)
        f = lambda *s, scale=1.0: (r.standard_normal(s) * scale).astype(np.float32)
        w = dict(g1=1 + f(D, scale=0.2), b1=f(D, scale=0.2), g2=1 + f(D, scale=0.2), b2=f(D, scale=0.2),
                 wq=f(D, D, scale=D ** -0.5), bq=f(D, scale=0.1), wk=f(D, D, scale=D ** -0.5), bk=f(D, scale=0.1),
                 wv=f(D, D, scale=D ** -0.5), bv=f(D, scale=0.1), wo=f(D, D, scale=D ** -0.5), bo=f(D, scale=0.1),
                 w1=f(F, D, scale=D ** -0.5), c1=f(F, scale=0.1), w2=f(D, F, scale=F ** -0.5), c2=f(D, scale=0.1))
        self.w64 = {k: v.astype(np.float64) for k, v in w.items()}
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        self.dev = dict(g1=dev(w["g1"]), b1=dev(w["b1"]), g2=dev(w["g2"]), b2=dev(w["b2"]),
                        wqkv_t=dev(np.concatenate([w["wq"], w["wk"], w["wv"]], 0).T),
                        bqkv=dev(np.concatenate([w["bq"], w["bk"], w["bv"]])), wo_t=dev(w["wo"].T), bo=dev(w["bo"]),
                        w1_t=dev(w["w1"].T), c1=dev(w["c1"]), w2_t=dev(w["w2"].T), c2=dev(w["c2"]))


@pytest.fixture(scope="module")
def layer(device):
    return _Layer(device)


def _args(L, lay, x, y, kc, vc, t, B):
    """x / y [D, B] views, kc / vc [D, B, Tp] contiguous."""
    a = L.PlmDecodeArgs()
    a.x, a.x_bs, a.x_cs = L.fptr(x), x.stride(1), x.stride(0)
    a.y, a.y_bs, a.y_cs = L.fptr(y), y.stride(1), y.stride(0)
    a.k_cache, a.v_cache, a.bs, a.cs = L.fptr(kc), L.fptr(vc), kc.stride(1), kc.stride(0)
    a.t, a.B, a.D, a.H, a.F, a.eps = t, B, lay.D, lay.H, lay.F, 1e-5
    for k, v in lay.dev.items():
        setattr(a, k, L.fptr(v))
    need = L.lib().hsp_plm_decode_workspace_bytes(B, lay.D)
    assert need == 4 * B * lay.D * 13
    ws = torch.full((need // 4,), float("nan"), device=x.device)            # scratch carries nothing between calls
    a.workspace, a.workspace_bytes = L.fptr(ws), need
    a._keep = ws
    return a


def _contract(device, layer, B, ts):
    from megatts2_hierspeechpp_amd import _lib as L
    D = layer.D
    assert L.lib().hsp_plm_decode_supported(D, layer.H, layer.F) == 1
    r = np.random.default_rng(100 + B)
    for t in ts:
        Tp = t + 1 + (3 if t % 2 else 6)                                   # cache pitch > t + 1
        x_np = r.standard_normal((D, B)).astype(np.float32)
        kc_np = r.standard_normal((D, B, Tp)).astype(np.float32)
        vc_np = r.standard_normal((D, B, Tp)).astype(np.float32)
        kc_np[:, :, t:] = np.nan                                            # columns >= t: never read (t is overwritten)
        vc_np[:, :, t:] = np.nan
        # x and y as strided [1, D, B] views: every other column of a [D, 2 B] buffer, and a [D, B + 3] buffer
        xbuf = torch.zeros(D, 2 * B, device=device)
        x = xbuf[:, ::2]
        x.copy_(torch.from_numpy(x_np))
        ybuf = torch.full((D, B + 3), 7.0, device=device)
        y = ybuf[:, 1:B + 1]
        kc, vc = torch.from_numpy(kc_np).to(device), torch.from_numpy(vc_np).to(device)
        a = _args(L, layer, x, y, kc, vc, t, B)
        L.check(L.lib().hsp_plm_decode_layer_f32(ctypes.byref(a), L.stream_ptr()), "hsp_plm_decode_layer_f32")
        torch.cuda.synchronize()
        k64, v64 = kc_np.transpose(1, 0, 2).astype(np.float64), vc_np.transpose(1, 0, 2).astype(np.float64)   # [B, D, Tp]
        want = R.decode_layer(layer.w64, x_np.T.astype(np.float64), k64, v64, t, H=layer.H)                              # [B, D]
        got_y, got_k, got_v = y.cpu().numpy(), kc.cpu().numpy(), vc.cpu().numpy()
        assert np.isfinite(got_y).all()
        _close(got_y.T, want, f"y B={B} t={t}")
        _close(got_k[:, :, t].T, k64[:, :, t], f"k B={B} t={t}")
        _close(got_v[:, :, t].T, v64[:, :, t], f"v B={B} t={t}")
        other = np.arange(Tp) != t
        assert got_k[:, :, other].tobytes() == kc_np[:, :, other].tobytes()       # bit-identical, NaN columns included
        assert got_v[:, :, other].tobytes() == vc_np[:, :, other].tobytes()
        assert (ybuf[:, 0] == 7).all() and (ybuf[:, B + 1:] == 7).all() and torch.equal(x.cpu(), torch.from_numpy(x_np))


@pytest.mark.parametrize("B", [1, 3, 16])
def test_decode_layer_kernel_contract(device, layer, B):
    _contract(device, layer, B, (0, 1, 3, 4, 63, 64, 65, 255, 256))


def test_decode_layer_kernel_contract_second_geometry(device):
    """hsp_plm_decode_supported accepts a family of geometries; one far from the PLM's: 8 heads of 8 channels (fewer
    head channels than waves, input slices past the end), 8 hidden units per feed-forward slice."""
    _contract(device, _Layer(device, seed=2, D=64, H=8, F=96), 3, (0, 5, 64, 130))


def test_decode_layer_row_is_bit_identical_alone_and_in_a_batch(device, layer):
    """include/hsp.h: row b of a batch equals the call on that row alone bit for bit (y and column t of both caches)."""
    from megatts2_hierspeechpp_amd import _lib as L
    B, r = 16, np.random.default_rng(7)
    run = lambda a: (L.check(L.lib().hsp_plm_decode_layer_f32(ctypes.byref(a), L.stream_ptr()), "decode"),
                     torch.cuda.synchronize())
    for t in (0, 5, 70, 256):
        Tp = t + 3
        x = torch.from_numpy(r.standard_normal((D, B)).astype(np.float32)).to(device)
        kc = torch.from_numpy(r.standard_normal((D, B, Tp)).astype(np.float32)).to(device)
        vc = torch.from_numpy(r.standard_normal((D, B, Tp)).astype(np.float32)).to(device)
        y = torch.zeros(D, B, device=device)
        kb, vb = kc.clone(), vc.clone()
        run(_args(L, layer, x, y, kb, vb, t, B))
        for b in (0, 7, 15):
            x1, y1 = x[:, b:b + 1].contiguous(), torch.zeros(D, 1, device=device)
            k1, v1 = kc[:, b:b + 1].contiguous(), vc[:, b:b + 1].contiguous()
            run(_args(L, layer, x1, y1, k1, v1, t, 1))
            same = lambda u, w: u.cpu().numpy().tobytes() == w.cpu().numpy().tobytes()
            assert same(y1[:, 0], y[:, b]), (t, b)
            assert same(k1[:, 0, t], kb[:, b, t]) and same(v1[:, 0, t], vb[:, b, t]), (t, b)


def test_decode_layer_refusals(device, layer):
    from megatts2_hierspeechpp_amd import _lib as L
    B, t, Tp = 2, 3, 8
    x, y = torch.zeros(D, B, device=device), torch.full((D, B), 5.0, device=device)
    kc, vc = torch.zeros(D, B, Tp, device=device), torch.zeros(D, B, Tp, device=device)
    call = lambda a: L.lib().hsp_plm_decode_layer_f32(ctypes.byref(a), L.stream_ptr())
    assert L.lib().hsp_plm_decode_layer_f32(None, L.stream_ptr()) == L.EINVAL
    ptrs = ["workspace", "x", "y", "k_cache", "v_cache", "g1", "b1", "wqkv_t", "bqkv", "wo_t", "bo", "g2", "b2", "w1_t", "c1", "w2_t", "c2"]
    for name in ptrs:
        a = _args(L, layer, x, y, kc, vc, t, B)
        setattr(a, name, None)
        assert call(a) == L.EINVAL, name
    for field, value in [("t", -1), ("t", B * Tp), ("t", 2 ** 31 - 1), ("debug", 1), ("B", 0), ("D", 277), ("H", 5),
                         ("F", 1102), ("D", 0), ("F", 8192 * 12), ("workspace_bytes", 4 * B * D * 13 - 4), ("workspace_bytes", 0),
                         ("B", 70000)]:
        a = _args(L, layer, x, y, kc, vc, t, B)
        setattr(a, field, value)
        assert call(a) == L.EINVAL, (field, value)
    a = _args(L, layer, x, y, kc, vc, t, B)
    a.wo_t = L.fptr(layer.dev["wo_t"].reshape(-1)[1:])                       # a weight matrix off its 16-byte alignment
    assert call(a) == L.EINVAL
    torch.cuda.synchronize()
    assert (y == 5).all() and (kc == 0).all() and (vc == 0).all()           # nothing was launched
    assert L.lib().hsp_plm_decode_supported(276, 4, 1104) == 1 and L.lib().hsp_plm_decode_supported(277, 4, 1104) == 0
    a = _args(L, layer, x, y, kc, vc, t, B)
    assert call(a) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------ 2. score
def test_score_matches_reference_golden(device, plm):
    g = np.load(os.path.join(HERE, "golden", "causal", "plm_causal_b2_t24.npz"))
    dev = lambda a: torch.from_numpy(a).to(device)
    lg = plm.score(dev(g["tc"]), dev(g["p_codes"]), dev(g["lens"])).cpu().numpy()
    assert lg.shape == (2, 24, 1024)
    rng = np.abs(g["logits"]).max()
    for b, n in enumerate(g["lens"]):
        err = np.abs(lg[b, :n] - g["logits"][b, :n]).max()
        print(f"golden row {b}: err {err:.3e} of range {rng:.3f}")
        assert err <= TOL * rng


def test_score_matches_float64_ragged(device, plm):
    r = np.random.default_rng(21)
    lens = np.array([33, 20, 29])
    tc = r.standard_normal((3, 256, 33)).astype(np.float32)
    codes = r.integers(0, 1024, (3, 33)).astype(np.int64)
    for b, n in enumerate(lens):
        codes[b, n:] = 1025
    want = R.forward_logits(R.synth_state(), tc, codes, lens)
    got = plm.score(torch.from_numpy(tc).to(device), torch.from_numpy(codes).to(device), torch.from_numpy(lens)).cpu().numpy()
    for b, n in enumerate(lens):
        _close(got[b, :n], want[b, :n], f"score row {b}")
    from megatts2_hierspeechpp_amd._lib import HspError
    with pytest.raises(HspError):                                            # the reference's assertion: max(lens) == T
        plm.score(torch.from_numpy(tc).to(device), torch.from_numpy(codes).to(device), torch.tensor([20, 20, 29]))


# ------------------------------------------------------------------------------------------------------ 3. infer
@pytest.mark.parametrize("shape", sorted(R.DECODE_CASES))
def test_causal_infer_equals_float64_decode(device, plm, shape):
    B, T = shape
    tc_np, want_codes, want_logits, _ = R.decoded(shape)
    tc = torch.from_numpy(tc_np).to(device)
    codes, logits = plm.infer(tc, return_logits=True, causal=True)
    assert codes.shape == (B, T) and logits.shape == (B, T, 1024)
    _close(logits.cpu().numpy(), want_logits, f"loop logits {shape}")
    assert np.array_equal(codes.cpu().numpy(), want_codes)                                  # no exceptions
    assert torch.equal(plm.infer(tc, causal=True), codes)
    # the identity the mode rests on: the loop's logits are the teacher-forced logits of its own codes
    sc = plm.score(tc, codes, torch.full((B,), T, dtype=torch.int64))
    _close(sc.cpu().numpy(), logits.cpu().numpy().astype(np.float64), f"score vs loop {shape}")
    # each row of the batch equals the row decoded alone
    for b in range(B):
        solo_c, solo_l = plm.infer(tc[b:b + 1].contiguous(), return_logits=True, causal=True)
        assert torch.equal(solo_c[0], codes[b]), b
        # the decode kernel is bit-invariant to the batch (hsp.h); the predict layer's GEMM picks its tile by the
        # column count, so the logits agree to rounding, not to the bit
        _close(solo_l[0].cpu().numpy(), logits[b].cpu().numpy().astype(np.float64), f"solo row {b} {shape}")


def test_causal_differs_from_bidirectional_and_default_is_unchanged(device, plm):
    tc = torch.from_numpy(R.decoded((3, 9))[0]).to(device)
    c0, l0 = plm.infer(tc, return_logits=True)
    c1, l1 = plm.infer(tc, return_logits=True, causal=False)
    assert torch.equal(c0, c1) and torch.equal(l0, l1)
    _, l2 = plm.infer(tc, return_logits=True, causal=True)
    assert torch.equal(l0[:, 0], l2[:, 0]) or (l0[:, 0] - l2[:, 0]).abs().max() <= TOL * l0.abs().max()   # one position: same model
    assert not torch.allclose(l0[:, 1:], l2[:, 1:], atol=1e-2)


# --------------------------------------------------------------------------------------------------- 4. sampling
def test_causal_sampling_follows_the_reference_sampler(device, plm):
    from megatts2_hierspeechpp_amd.ttv_v1.t2w2v_transformer import PlmSampling
    sp = PlmSampling(temperature=1.1, top_k=40, top_p=0.95, repetition_penalty=1.2)
    B, T = 3, 20
    tc = torch.from_numpy(R.case_tc((B, T), [71, 72, 73])).to(device)
    seeds = [5, 2 ** 40 + 3, -9]
    sd = torch.tensor(seeds, dtype=torch.int64, device=device)
    codes, logits = plm.infer(tc, return_logits=True, sampling=sp, seeds=sd, causal=True)
    codes_np, lg = codes.cpu().numpy(), logits.cpu().numpy()
    for b in range(B):
        for t in range(T):
            want, _ = S.decide(lg[b, t], [int(c) for c in codes_np[b, :t]], seeds[b], t + 1, temperature=sp.temperature,
                               top_k=sp.top_k, top_p=sp.top_p, repetition_penalty=sp.repetition_penalty)
            assert int(codes_np[b, t]) == want, (b, t)
    again = plm.infer(tc, sampling=sp, seeds=sd, causal=True)
    assert torch.equal(again, codes)
    assert not torch.equal(plm.infer(tc, sampling=sp, seeds=sd + 1000, causal=True), codes)
    # row b of the batch == the solo run with its seed
    assert torch.equal(plm.infer(tc[1:2].contiguous(), sampling=sp, seeds=sd[1:2].contiguous(), causal=True)[0], codes[1])


# ---------------------------------------------------------------------------------------------- 5. graph capture
def test_causal_loop_graph_capture_equals_eager(device, plm):
    shape, seeds = R.GRAPH_CASE
    tc = torch.from_numpy(R.case_tc(shape, seeds)).to(device)
    eager_c, eager_l = plm.infer(tc, return_logits=True, causal=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_c, out_l = plm.infer(tc, return_logits=True, causal=True)
    out_c.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_c, eager_c) and torch.equal(out_l, eager_l)
    tc.copy_(torch.from_numpy(R.case_tc(shape, [s + 100 for s in seeds])).to(device))      # a replay reads new inputs
    graph.replay()
    torch.cuda.synchronize()
    c2, l2 = plm.infer(tc, return_logits=True, causal=True)
    assert torch.equal(out_c, c2) and torch.equal(out_l, l2) and not torch.equal(c2, eager_c)


# ----------------------------------------------------------------------------------------------------- 6. harness
def test_tts_plm_causal_equals_hand_composition(device):
    from megatts2_hierspeechpp_amd import inference_plm as IP, synth
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
    # which loop ran: this synthetic TTS model is degenerate enough that both modes pick the same codes, so the waveform
    # cannot tell; count the entries into the K/V-cached loop instead
    calls, cached_loop = [], models.plm._infer_causal
    models.plm._infer_causal = lambda *a, **k: (calls.append(1), cached_loop(*a, **k))[1]
    wav_c, audio_c = IP.tts(models, ids, tl, tone, lang, mel, ml, mel2, ml2, plm_causal=True, **kw)
    assert len(calls) == 1
    x_frame, g, x_lengths, x_mask = models.ttv.inf_extract_tc_latent(ids, tl, mel, ml, tone, lang, dur=dur)
    codes = models.plm.infer(x_frame, causal=True)
    wav_h, audio_h = IP.tts_from_codes(models, x_frame, g, codes, x_lengths, x_mask, mel2, ml2, noise=noise, return_float=True)
    assert torch.equal(wav_c, wav_h) and torch.equal(audio_c, audio_h)
    wav_d, audio_d = IP.tts(models, ids, tl, tone, lang, mel, ml, mel2, ml2, **kw)
    wav_f, audio_f = IP.tts(models, ids, tl, tone, lang, mel, ml, mel2, ml2, plm_causal=False, **kw)
    assert torch.equal(wav_d, wav_f) and torch.equal(audio_d, audio_f)
    assert len(calls) == 2                                                  # the hand composition's one; none by default
