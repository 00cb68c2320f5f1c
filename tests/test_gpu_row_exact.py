"""GPU (-m gpu): row-exact ragged batches.  The per-row key lengths of hsp_mha_proj_f32 against a
float64 restatement, the ragged Activation1d against solo launches on each row, and vc_batch(row_exact=True) against
vc() on every row alone (eager and as a hipGraph replay)."""
import numpy as np
import pytest
import torch

from test_gpu_vc_batch import _case, _rel, vc_setup  # noqa: F401  (module fixture)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------ key-masked mha_proj
def _mha_proj_ref(q, k, v, H, scale, wt, bias, mask, cscale, res, key_len):
    """float64: per-row masked softmax over keys < key_len[b], projection, * mask * cscale + res."""
    q, k, v, wt, bias, mask, cscale, res = (t.double().cpu() for t in (q, k, v, wt, bias, mask, cscale, res))
    B, C, Tq = q.shape
    D = C // H
    y = torch.empty(B, wt.shape[0], Tq, dtype=torch.float64)
    for b in range(B):
        n = int(key_len[b])
        o = torch.empty(C, Tq, dtype=torch.float64)
        for h in range(H):
            qs, ks, vs = q[b, h * D:(h + 1) * D], k[b, h * D:(h + 1) * D, :n], v[b, h * D:(h + 1) * D, :n]
            p = torch.softmax(scale * qs.t() @ ks, dim=1)                  # [Tq, n]
            o[h * D:(h + 1) * D] = vs @ p.t()
        y[b] = ((wt @ o + bias[:, None]) * mask[b, 0][None, :]) * cscale[b][:, None] + res[b]
    return y


@pytest.mark.parametrize("H,D", [(2, 96), (4, 69)])
@pytest.mark.parametrize("Tk", [4, 37, 256, 257, 1000])
def test_mha_proj_key_len_against_float64(device, H, D, Tk):
    from megatts2_hierspeechpp_amd import functional as Fh
    r = np.random.default_rng(Tk + H)
    B, C = 5, H * D
    g = lambda *s: torch.from_numpy(r.standard_normal(s).astype(np.float32)).to(device)
    q, k, v = g(B, C, Tk), g(B, C, Tk), g(B, C, Tk)
    wt, bias, cscale, res = g(C, C) * C ** -0.5, g(C), g(B, C), g(B, C, Tk)
    lens = np.array([1, Tk, r.integers(1, Tk + 1), r.integers(1, Tk + 1), max(1, Tk - 1)], np.int64)
    mask = torch.from_numpy((np.arange(Tk)[None, None, :] < lens[:, None, None]).astype(np.float32)).to(device)
    kl = torch.from_numpy(lens).to(device)
    y = Fh.mha_proj(q, k, v, H, D ** -0.5, wt, bias=bias, mask=mask, cscale=cscale, res=res, key_len=kl)
    want = _mha_proj_ref(q, k, v, H, D ** -0.5, wt, bias, mask, cscale, res, lens)
    err = (y.double().cpu() - want).abs().max() / want.abs().max()
    assert err <= 2e-6, (lens.tolist(), float(err))
    # every row at its full length: the maskless launch, bit for bit
    full = torch.full((B,), Tk, dtype=torch.int64, device=device)
    a = Fh.mha_proj(q, k, v, H, D ** -0.5, wt, bias=bias, mask=mask, cscale=cscale, res=res, key_len=full)
    b = Fh.mha_proj(q, k, v, H, D ** -0.5, wt, bias=bias, mask=mask, cscale=cscale, res=res)
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------ ragged Activation1d
def test_ragged_activation_matches_solo_rows(device):
    from megatts2_hierspeechpp_amd import functional as Fh
    from megatts2_hierspeechpp_amd.synth import kaiser_sinc_filter12
    r = np.random.default_rng(3)
    B, C, L = 9, 24, 1600
    lens = np.array([L, 1, 5, 496, 497, 498, 994, 993, 1203], np.int64)   # ends on and just past the 496-sample segments
    x = torch.from_numpy(r.standard_normal((B, C, L)).astype(np.float32)).to(device)
    ea = torch.from_numpy(r.uniform(0.5, 2.0, C).astype(np.float32)).to(device)
    binv = torch.from_numpy(r.uniform(0.3, 1.5, C).astype(np.float32)).to(device)
    f = torch.from_numpy(kaiser_sinc_filter12().astype(np.float32).reshape(-1))
    filt = torch.cat([f, f]).to(device)
    y = Fh.act1d(x, ea, binv, filt, lens=torch.from_numpy(lens).to(device)).cpu()
    plain = Fh.act1d(x, ea, binv, filt).cpu()
    assert torch.equal(y[0], plain[0])                       # a full row is the plain launch
    for b, n in enumerate(lens):
        solo = Fh.act1d(x[b:b + 1, :, :n].contiguous(), ea, binv, filt).cpu()[0]
        if n % 4 == 0:    # the solo launch takes the same (wave-per-segment) kernel
            assert torch.equal(y[b, :, :n], solo), b
        else:             # ... else the workgroup-tile kernel, another summation order
            assert _rel(y[b, :, :n], solo) <= 1e-6, (b, _rel(y[b, :, :n], solo))
        assert not y[b, :, n:].any(), b


# ------------------------------------------------------------------------------------------ end to end
def _solo_check(IV, models, mel_fn, srcs, f0s, prompts, f0t, noise, audio, wav, n_out):
    for b in range(len(srcs)):
        T = srcs[b].shape[-1] // 320
        w1, a1 = IV.vc(models, mel_fn, srcs[b], f0s[b].reshape(1, -1), prompts[b], f0t[b].reshape(1, -1),
                       noise=noise[b:b + 1, :, :T].contiguous(), return_float=True)
        n = 320 * T
        assert int(n_out[b]) == n
        err = _rel(audio[b:b + 1, :, :n], a1)
        assert err <= 1e-4, (b, T, err)
        assert not audio[b, :, n:].any(), b
        assert (wav[b, :n].int() - w1.reshape(-1).int()).abs().max() <= 8, b


@pytest.mark.parametrize("forced_fft", [False, True])
def test_vc_batch_row_exact_shared_prompt(device, vc_setup, forced_fft):
    from megatts2_hierspeechpp_amd import hierspeechpp_speechsynthesizer as HS, inference_vc as IV
    models, mel_fn = vc_setup
    raw = [8000, 64000, 20000, 41000, 12345, 30000, 52000, 16000]      # 0.5-4 s
    srcs, f0s, prompts, f0t = _case(device, raw, [48000], 21)
    Tm = max(s.shape[-1] for s in srcs) // 320
    noise = torch.from_numpy(np.random.default_rng(2).standard_normal((8, 192, Tm)).astype(np.float32)).to(device)
    old = HS.FFT_MIN_COLS
    HS.FFT_MIN_COLS = 0 if forced_fft else old
    try:
        wav, n_out, audio = IV.vc_batch(models, mel_fn, srcs, f0s, prompts[0], f0t[0], noise=noise, return_float=True,
                                        row_exact=True)
        _solo_check(IV, models, mel_fn, srcs, f0s, [prompts[0]] * 8, [f0t[0]] * 8, noise, audio, wav, n_out)
    finally:
        HS.FFT_MIN_COLS = old


def test_vc_batch_row_exact_per_row_prompts(device, vc_setup):
    from megatts2_hierspeechpp_amd import inference_vc as IV
    models, mel_fn = vc_setup
    srcs, f0s, prompts, f0t = _case(device, [30000, 9000, 50000, 17777], [40000, 23456, 31000, 16000], 31)
    Tm = max(s.shape[-1] for s in srcs) // 320
    noise = torch.from_numpy(np.random.default_rng(4).standard_normal((4, 192, Tm)).astype(np.float32)).to(device)
    wav, n_out, audio = IV.vc_batch(models, mel_fn, srcs, f0s, prompts, f0t, noise=noise, return_float=True,
                                    row_exact=True)
    _solo_check(IV, models, mel_fn, srcs, f0s, prompts, f0t, noise, audio, wav, n_out)


def test_vc_batch_row_exact_graph_replay_equals_eager(device, vc_setup):
    from megatts2_hierspeechpp_amd import inference_vc as IV
    models, mel_fn = vc_setup
    srcs, f0s, prompts, f0t = _case(device, [9000, 20000, 3000], [24000], 17)
    x, xl = IV._stack(srcs, device)
    fs, fl = IV._stack(f0s, device)
    xl, fl = torch.tensor(xl, device=device), torch.tensor(fl, device=device)
    T = x.shape[1] // 320
    noise = torch.from_numpy(np.random.default_rng(9).standard_normal((3, 192, T)).astype(np.float32)).to(device)
    run = lambda: IV.vc_batch(models, mel_fn, (x, xl), (fs, fl), prompts[0], f0t[0], noise=noise, return_float=True,
                              row_exact=True)
    eager = run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed = run()
    g.replay()
    torch.cuda.synchronize()
    for e, r in zip(eager, graphed):
        assert torch.equal(e, r)


# ------------------------------------------------------------------------------- ragged activation inside the transforms
def _fft_convs(models):
    """an AMP block whose two first convs both take the frequency-domain form and pair up"""
    from megatts2_hierspeechpp_amd import hierspeechpp_speechsynthesizer as HS
    for blk in models.voc.dec.resblocks:
        c1, c2 = blk.convs1[0], blk.convs2[0]
        if c1.__dict__.get("_fft") and c2.__dict__.get("_fft"):
            return blk, c1, c2
    pytest.skip("no frequency-domain AMP conv in this config")


@pytest.mark.parametrize("placement", ["forward", "pair"])
def test_ragged_activation_in_the_transforms_matches_solo_rows(device, vc_setup, placement):
    from megatts2_hierspeechpp_amd import hip_layers
    models, _ = vc_setup
    blk, c1, c2 = _fft_convs(models)
    a1, a2 = blk.activations[0], blk.activations[1]
    r = np.random.default_rng(12)
    L = 1600
    lens = np.array([L, 4, 241, 480, 482, 963, 1203], np.int64)   # ends on and just past the 240-sample segments
    B = len(lens)
    x = torch.from_numpy(r.standard_normal((B, c1.cin, L)).astype(np.float32) * 0.5).to(device)
    if placement == "pair" and not c1.fft_pair_ok(c2, x):
        pytest.skip("no pair launch for this geometry")
    run = (lambda t: c1.forward_fft(t, act1d=a1)) if placement == "forward" else \
        (lambda t: c1.forward_fft_pair(c2, t, act_first=a1, act_second=a2))
    with hip_layers.row_exact(hip_layers.RowLengths(torch.from_numpy(lens).to(device), L)):
        y = run(x)
    for b, n in enumerate(lens):
        xs = x[b:b + 1, :, :n].contiguous()
        # the solo reference: the same fused launch where the row length allows it, else the stand-alone activation
        if n % 4 == 0:
            want = run(xs)
        elif placement == "forward":
            want = c1.forward_fft(a1(xs))
        else:
            want = c2.forward_fft(a2(c1.forward_fft(a1(xs))))
        assert _rel(y[b:b + 1, :, :n], want) <= 1e-5, (placement, b, int(n), _rel(y[b:b + 1, :, :n], want))


# ------------------------------------------------------------------------------- DiT block: fused and two-launch forms
def test_dit_block_key_mask_fused_and_fallback_match_solo(device, vc_setup, monkeypatch):
    from megatts2_hierspeechpp_amd import functional as Fh
    models, _ = vc_setup
    blk = models.voc.flow.flows[0].enc_block[0]
    C = blk.hidden_size
    r = np.random.default_rng(5)
    lens = np.array([70, 23, 41], np.int64)
    B, T = len(lens), int(lens.max())
    mask = torch.from_numpy((np.arange(T)[None, None] < lens[:, None, None]).astype(np.float32)).to(device)
    x = torch.from_numpy(r.standard_normal((B, C, T)).astype(np.float32)).to(device) * mask
    mod = torch.from_numpy(0.3 * r.standard_normal((B, 6 * C, 1)).astype(np.float32)).to(device)
    kl = torch.from_numpy(lens).to(device)
    fused = blk(x, None, mask, mod=mod, key_len=kl)
    monkeypatch.setattr(Fh, "FUSE_MHA_PROJ", False)        # the two-launch form: hsp_mha_f32 with mask_k
    fallback = blk(x, None, mask, mod=mod, key_len=kl)
    assert _rel(fallback, fused) <= 1e-5
    for b, n in enumerate(lens):
        solo = blk(x[b:b + 1, :, :n].contiguous(), None, mask[b:b + 1, :, :n].contiguous(), mod=mod[b:b + 1].contiguous())
        for y in (fused, fallback):
            assert _rel(y[b:b + 1, :, :n], solo) <= 1e-5, b
            assert not y[b, :, n:].any(), b


# ------------------------------------------------------------------------------- 24 / 48 kHz and the files entry point
@pytest.mark.parametrize("output_sr", [24000, 48000])
def test_vc_batch_row_exact_speechsr(device, vc_setup, output_sr, monkeypatch):
    from megatts2_hierspeechpp_amd import inference_vc as IV, synth
    from megatts2_hierspeechpp_amd.speechsr24k.speechsr import SynthesizerTrn as SpeechSR24
    models, mel_fn = vc_setup
    if output_sr == 24000:
        sr = SpeechSR24(128, 30, "0", [3, 7, 11], [[1, 3, 5]] * 3, [3], 32, [3])
        sr.load_state_dict({k: torch.from_numpy(synth.synth_tensor(k, tuple(v.shape), 3))
                            for k, v in sr.state_dict().items()})
        sr.finalize(device)
        monkeypatch.setattr(models, "sr", sr)
    srcs, f0s, prompts, f0t = _case(device, [8000, 40000, 17000, 26000], [30000], 41)
    Tm = max(s.shape[-1] for s in srcs) // 320
    noise = torch.from_numpy(np.random.default_rng(6).standard_normal((4, 192, Tm)).astype(np.float32)).to(device)
    wav, n_out, audio = IV.vc_batch(models, mel_fn, srcs, f0s, prompts[0], f0t[0], noise=noise, return_float=True,
                                    row_exact=True, output_sr=output_sr)
    per_frame = output_sr // 50
    for b in range(4):
        T = srcs[b].shape[-1] // 320
        w1, a1 = IV.vc(models, mel_fn, srcs[b], f0s[b].reshape(1, -1), prompts[0], f0t[0].reshape(1, -1),
                       noise=noise[b:b + 1, :, :T].contiguous(), return_float=True, output_sr=output_sr)
        n = per_frame * T
        assert int(n_out[b]) == n and a1.shape[-1] == n
        assert _rel(audio[b:b + 1, :, :n], a1) <= 1e-4, (b, _rel(audio[b:b + 1, :, :n], a1))
        assert not audio[b, :, n:].any()
        assert (wav[b, :n].int() - w1.reshape(-1).int()).abs().max() <= 8, b


def test_vc_batch_files_row_exact_is_one_batch(device, vc_setup, tmp_path):
    from scipy.io import wavfile
    from megatts2_hierspeechpp_amd import audio as A, inference_vc as IV
    from test_gpu_vc_batch import _speech, _track
    models, mel_fn = vc_setup
    files = []
    for i, n in enumerate([20000, 70000, 9000, 33000]):
        p = tmp_path / f"src{i}.wav"
        wavfile.write(p, 16000, _speech(n, 90 + i))
        files.append(p)
    prompt = tmp_path / "voice.wav"
    wavfile.write(prompt, 16000, _speech(48000, 99))
    for p in files:
        s = IV.load_source(p, device)
        np.save(str(p)[:-4] + ".hf0.npy", _track(s.shape[-1] // 80 + 1, 3)[None])
    np.save(tmp_path / "voice.hf0.npy", _track(A.load_16k(prompt, device).shape[-1] // 80, 4))
    Tm = max(IV.load_source(p, device).shape[-1] for p in files) // 320
    noise = torch.from_numpy(np.random.default_rng(7).standard_normal((4, 192, Tm)).astype(np.float32)).to(device)
    calls = []
    IV.STAGE_HOOK = lambda name: calls.append(name) if name == "wav2vec2" else None
    try:
        wav, n_out = IV.vc_batch_files(models, mel_fn, files, prompt, out_dir=tmp_path / "out", row_exact=True,
                                       noise=noise)
    finally:
        IV.STAGE_HOOK = None
    assert len(calls) == 1
    for b, p in enumerate(files):
        w1, n1 = IV.vc_batch_files(models, mel_fn, [p], prompt, noise=noise[b:b + 1])
        rate, back = wavfile.read(tmp_path / "out" / f"src{b}_to_voice.wav")
        assert rate == 16000 and back.shape[0] == int(n1[0]) == int(n_out[b])
        assert np.abs(back.astype(np.int32) - w1[0, :int(n1[0])].cpu().numpy().astype(np.int32)).max() <= 8, b
