"""GPU checks of the sampled PLM decoding (hsp_sample_f32, hsp_plm_embed_sample_f32, Megatts2PLM1.infer(sampling=...))
against the reference sampler's fixtures and against the greedy path."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import plm_sampling_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(HERE, "golden", "sampling")


def _plm(device, seed=7):
    from megatts2_hierspeechpp_amd import synth
    from megatts2_hierspeechpp_amd.ttv_v1.t2w2v_transformer import Megatts2PLM1
    m = Megatts2PLM1()
    m.load_state_dict({k: torch.from_numpy(synth.synth_tensor("plm." + k, tuple(v.shape), seed))
                       for k, v in m.state_dict().items()})
    m.finalize(device)
    return m


def test_sample_kernel_matches_reference_fixture(device):
    from megatts2_hierspeechpp_amd import _lib as L
    from megatts2_hierspeechpp_amd.ttv_v1.t2w2v_transformer import PlmSampling
    d = np.load(os.path.join(GOLD, "plm_sample_cases.npz"))
    meta = json.loads(bytes(d["meta"]).decode())
    for c, m in enumerate(meta):
        prev = [int(t) for t in d["prev"][c][:m["n_prev"]]]
        j = int(d["j"][c])
        sp = PlmSampling(**{k: m[k] for k in ("temperature", "top_k", "top_p", "repetition_penalty")})
        codes = torch.tensor([[1024] + prev + [-1]], dtype=torch.int64, device=device)
        logits = torch.from_numpy(d["logits"][c]).reshape(1, 1024, 1).to(device)   # the loop's [1, V, B] layout
        seeds = torch.tensor([int(d["seed"][c])], dtype=torch.int64, device=device)
        probs = torch.full((1, 1024), -1.0, device=device)
        a = sp.c_args(seeds, probs)
        L.check(L.lib().hsp_sample_f32(L.fptr(logits), 1, 1, 1, 1024, L.ptr(codes[:, j:]), codes.stride(0), j,
                                       ctypes.byref(a), L.stream_ptr()), "hsp_sample_f32")
        torch.cuda.synchronize()
        assert (probs.cpu()[0] - torch.from_numpy(d["probs"][c])).abs().max().item() <= 1e-6, (c, m)
        assert int(codes[0, j]) == int(d["token"][c]), (c, m)
        assert codes[0, :j].cpu().tolist() == [1024] + prev


def test_embed_sample_equals_sample_then_embed(device):
    from megatts2_hierspeechpp_amd import _lib as L
    from megatts2_hierspeechpp_amd.ttv_v1.t2w2v_transformer import PlmSampling
    m = _plm(device)
    sp = PlmSampling(temperature=0.9, top_k=30, top_p=0.95, repetition_penalty=1.2)
    g = torch.Generator().manual_seed(8)
    m.infer(torch.zeros(1, 256, 2, device=device))
    for B, n in [(16, 2), (5, 37), (32, 200)]:
        tc = torch.randn(B, 256, 200, generator=g).to(device)
        codes = torch.randint(0, 40, (B, 201), generator=g).to(device)     # few distinct tokens: the penalty bites
        codes[:, 0] = m.GO_ID
        logits = (torch.randn(1, 1024, B, generator=g) * 2).to(device)
        seeds = torch.randint(-2 ** 62, 2 ** 62, (B,), generator=g).to(device)
        a = sp.c_args(seeds)
        c1, c2 = codes.clone(), codes.clone()
        L.check(L.lib().hsp_sample_f32(L.fptr(logits), 1, B, B, 1024, L.ptr(c1[:, n - 1:]), c1.stride(0), n - 1,
                                       ctypes.byref(a), L.stream_ptr()), "hsp_sample_f32")
        x1 = m._embed(tc, c1, n)
        x2 = m._embed(tc, c2, n, prev_logits=logits, sample=a)
        assert torch.equal(c1, c2) and torch.equal(x1, x2)
        assert not torch.equal(c2[:, n - 1], codes[:, n - 1])
    # the n == 1 one-position form of the layer-0 cache at position t
    import types
    B, t, Tp = 8, 9, 12
    tc = torch.randn(B, 256, Tp, generator=g).to(device)
    codes = torch.randint(0, 40, (B, Tp + 1), generator=g).to(device)
    codes[:, 0] = m.GO_ID
    logits = (torch.randn(1, 1024, B, generator=g) * 2).to(device)
    seeds = torch.arange(B, dtype=torch.int64, device=device) * 977
    a = sp.c_args(seeds)
    c1, c2 = codes.clone(), codes.clone()
    L.check(L.lib().hsp_sample_f32(L.fptr(logits), 1, B, B, 1024, L.ptr(c1[:, t:]), c1.stride(0), t, ctypes.byref(a),
                                   L.stream_ptr()), "hsp_sample_f32")
    cache = types.SimpleNamespace(emb=torch.zeros(m.d_model, B, Tp, device=device))
    m._embed_one(tc, c2, t, cache, logits, a)
    torch.cuda.synchronize()
    assert torch.equal(c1, c2)
    x1 = m._embed(tc, c1, t + 1)
    want = x1[0, :, :B * (t + 1)].reshape(m.d_model, B, t + 1)[:, :, t]
    assert torch.equal(cache.emb[:, :, t], want)


@pytest.mark.parametrize("cache_l0", [True, False])
def test_sampled_infer_reproduces_reference_loop(device, monkeypatch, cache_l0):
    from megatts2_hierspeechpp_amd.ttv_v1 import t2w2v_transformer as T2
    d = np.load(os.path.join(GOLD, "plm_sample_loop.npz"))
    meta = json.loads(bytes(d["meta"]).decode())
    m = _plm(device, meta["weight_seed"])
    monkeypatch.setattr(T2, "PLM_CACHE_L0", cache_l0)
    codes = m.infer(torch.from_numpy(d["tc"]).to(device), sampling=T2.PlmSampling(**meta["params"]),
                    seeds=torch.from_numpy(d["seeds"]).to(device)).cpu().numpy()
    assert (codes == d["codes"]).all(), (codes, d["codes"])


def test_top_k_1_is_greedy_and_seeds(device):
    from megatts2_hierspeechpp_amd.ttv_v1.t2w2v_transformer import PlmSampling
    m = _plm(device)
    g = torch.Generator().manual_seed(3)
    tc = torch.randn(4, 256, 18, generator=g).to(device)
    greedy = m.infer(tc)
    assert torch.equal(m.infer(tc, sampling=PlmSampling(top_k=1, temperature=0.5), seeds=11), greedy)
    # row b of a batch == the solo call with that row's seed; different seeds differ
    sp = PlmSampling(temperature=1.3, top_p=0.98, repetition_penalty=1.1)
    tc5 = torch.randn(5, 256, 18, generator=g).to(device)
    batch = m.infer(tc5, sampling=sp, seeds=100)
    for b in range(5):
        assert torch.equal(batch[b], m.infer(tc5[b:b + 1].contiguous(), sampling=sp, seeds=100 + b)[0])
    assert not torch.equal(m.infer(tc5, sampling=sp, seeds=100), m.infer(tc5, sampling=sp, seeds=7000))


def test_graph_replays_with_new_seeds(device):
    from megatts2_hierspeechpp_amd.ttv_v1.t2w2v_transformer import PlmSampling
    m = _plm(device)
    sp = PlmSampling(temperature=1.2, top_k=50, top_p=0.97, repetition_penalty=1.2)
    g = torch.Generator().manual_seed(4)
    tc = torch.randn(4, 256, 16, generator=g).to(device)
    A = torch.tensor([1, 2, 3, 4], dtype=torch.int64, device=device)
    Bs = torch.tensor([-5, 99, 2 ** 40, 7], dtype=torch.int64, device=device)
    eager_a = m.infer(tc, sampling=sp, seeds=A.clone())
    eager_b = m.infer(tc, sampling=sp, seeds=Bs.clone())
    seeds = A.clone()
    m.infer(tc, sampling=sp, seeds=seeds)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = m.infer(tc, sampling=sp, seeds=seeds)
    seeds.copy_(A)
    graph.replay()
    torch.cuda.synchronize()
    got_a = out.clone()
    seeds.copy_(Bs)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(got_a, eager_a) and torch.equal(out, eager_b) and not torch.equal(eager_a, eager_b)


def test_greedy_default_unchanged(device):
    m = _plm(device)
    tc = torch.randn(3, 256, 21, generator=torch.Generator().manual_seed(5)).to(device)
    c1, l1 = m.infer(tc, return_logits=True)
    c2, l2 = m.infer(tc, return_logits=True, sampling=None)
    assert torch.equal(c1, c2) and torch.equal(l1, l2)


def _sample(logits, codes, j, a):
    from megatts2_hierspeechpp_amd import _lib as L
    B = codes.shape[0]
    L.check(L.lib().hsp_sample_f32(L.fptr(logits), 1, B, B, logits.shape[1], L.ptr(codes[:, j:]), codes.stride(0), j,
                                   ctypes.byref(a), L.stream_ptr()), "hsp_sample_f32")
    torch.cuda.synchronize()
    return codes[:, j].cpu().tolist()


def test_device_stream_is_the_philox_stream(device):
    """Equal logits, no filter: the token is the index of the largest u, i.e. of the largest w >> 8 of the row's Philox
    words -- the device stream, word by word order, against the numpy Philox at 64 seeds and three columns."""
    from megatts2_hierspeechpp_amd.ttv_v1.t2w2v_transformer import PlmSampling
    B = 64
    seeds = torch.randint(-2 ** 63, 2 ** 63 - 1, (B,), generator=torch.Generator().manual_seed(2), dtype=torch.int64)
    logits = torch.zeros(1, 1024, B, device=device)
    seeds_dev = seeds.to(device)                     # the struct holds its pointer: keep the tensor alive
    a = PlmSampling().c_args(seeds_dev)
    for j in (1, 5, 300):
        codes = torch.full((B, j + 1), 1024, dtype=torch.int64, device=device)
        got = _sample(logits, codes, j, a)
        want = [int(np.argmin(R.exp_draws(int(s), j))) for s in seeds.tolist()]
        assert got == want, j


def test_top_word_draw_is_not_infinite(device):
    """Seed 725543 draws w >> 8 = 0xFFFFFF for token 11 at column 1: u = 1 - 2^-25, q = 3e-8, not 0.  Token 11 with a
    logit 30 below the rest must lose (a q of 0 would make its race score infinite); the token is the numpy one."""
    from megatts2_hierspeechpp_amd.ttv_v1.t2w2v_transformer import PlmSampling
    seed, j, i = 725543, 1, 11
    w = R.philox4x32_10(np.array([i >> 2, j, 0, 0], np.uint64), np.array([seed, 0], np.uint64))[i & 3]
    assert int(w) >> 8 == 0xFFFFFF
    lg = np.zeros(1024, np.float32)
    lg[i] = -30.0
    want, _ = R.decide(lg, [], seed, j)
    seeds_dev = torch.tensor([seed], dtype=torch.int64, device=device)
    a = PlmSampling().c_args(seeds_dev)
    codes = torch.full((1, 2), 1024, dtype=torch.int64, device=device)
    got = _sample(torch.from_numpy(lg).reshape(1, 1024, 1).to(device), codes, j, a)
    assert got == [want] and want != i


def test_tts_takes_equal_solo_calls(device, tmp_path):
    """tts_from_prompt(takes=3, seed=s): take k == the solo call with seed s + k (same explicit noise), the takes
    differ, and the files <stem>_take<k><ext> hold them."""
    from megatts2_hierspeechpp_amd import inference_plm as IP, synth
    from megatts2_hierspeechpp_amd.Mels_preprocess import MelSpectrogramFixed
    from megatts2_hierspeechpp_amd.ttv_v1.t2w2v_transformer import PlmSampling
    from oracle.hsp_oracle import default_config
    import helpers as H
    from scipy.io import wavfile
    mel_fn = MelSpectrogramFixed(sample_rate=16000, n_fft=1280, win_length=1280, hop_length=320, f_min=0, f_max=8000,
                                 n_mels=80, window_fn=torch.hann_window).finalize(device)
    models = IP.TtsModels(default_config(), H.TTV_MODEL)
    models.load_state_dict({k: torch.from_numpy(synth.synth_tensor(k, tuple(v.shape), 7))
                            for k, v in models.state_dict().items()})
    models.finalize(device)
    r = np.random.default_rng(5)
    N = 7
    ids = torch.from_numpy(r.integers(12, 113, (1, N))).to(device)
    tone = torch.from_numpy(r.integers(0, 11, (1, N))).to(device)
    lang = torch.where(ids < 74, 1, 2)
    t = np.arange(20000) / 16000.0
    prompt = torch.from_numpy((0.3 * np.sin(2 * np.pi * 140 * t) + 0.05 * r.standard_normal(20000))
                              .astype(np.float32)[None]).to(device)
    dur = torch.full((1, N), 4.0, device=device)
    noise = torch.from_numpy(r.standard_normal((1, 192, N * 2)).astype(np.float32)).to(device)
    sp = PlmSampling(temperature=1.3, top_p=0.98)
    kw = dict(dur=dur, noise=noise, plm_sampling=sp, return_float=True)
    wav, audio = IP.tts_from_prompt(models, mel_fn, ids, tone, lang, prompt, output_path=tmp_path / "x.wav", seed=40,
                                    takes=3, **kw)
    assert wav.shape == (3, N * 2 * 320) and wav.dtype == torch.int16
    for k in range(3):
        solo_wav, solo = IP.tts_from_prompt(models, mel_fn, ids, tone, lang, prompt, seed=40 + k, **kw)
        peak = solo.abs().max().item()
        assert (audio[k].reshape(-1) - solo.reshape(-1)).abs().max().item() <= 1e-4 * peak, k
        rate, back = wavfile.read(tmp_path / f"x_take{k}.wav")
        assert rate == 16000 and np.array_equal(back, wav[k].cpu().numpy())
    assert not torch.equal(wav[0], wav[1]) and not torch.equal(wav[1], wav[2]) and not torch.equal(wav[0], wav[2])
