"""GPU (-m gpu): row-exact ragged batches held to the reference.  The inputs of the goldens infer_config1,
vc_noise_control and vc_plain become the short row of a batch with longer random rows (padding filled with junk, not
zeros); with row_exact=True that row meets the golden outputs, with the frequency-domain form as chosen and forced."""
import numpy as np
import pytest
import torch

import helpers as H
from megatts2_hierspeechpp_amd import synth

pytestmark = pytest.mark.gpu


def _model(meta, device):
    from megatts2_hierspeechpp_amd.hip_layers import finalize
    mod = H.build_module(meta)
    sd = H.synth_sd(meta)
    pre = meta["prefix"] + "." if meta["prefix"] else ""
    for k, v in mod.state_dict().items():
        if k not in sd:
            sd[k] = torch.from_numpy(synth.synth_tensor(pre + k, tuple(v.shape), meta["seed"]))
    mod.load_state_dict(sd, strict=True)
    finalize(mod, device)
    return mod


def _ragged(gold, T_rows, row, r, scale=1.0):
    """[B, ..., max T] with the golden array (last axis T_g) at `row`, random rows elsewhere, junk past every row's end"""
    shape = gold.shape[1:-1]
    per = gold.shape[-1] // T_rows[row]           # columns per frame (4 for F0)
    Tm = max(T_rows) * per
    out = (scale * r.standard_normal((len(T_rows),) + shape + (Tm,))).astype(np.float32)
    out[row, ..., :gold.shape[-1]] = gold[0]
    return out


def _check(out, ref, n, what):
    ref = np.asarray(ref)
    got = out.detach().cpu().numpy()
    assert np.abs(got[..., :n] - ref[..., :n]).max() <= H.tol_for(ref), what
    assert not np.any(got[..., n:]), what


@pytest.fixture(params=[False, True], ids=["fft-policy", "fft-forced"])
def fft_forced(request, monkeypatch):
    from megatts2_hierspeechpp_amd import hierspeechpp_speechsynthesizer as HS
    if request.param:
        monkeypatch.setattr(HS, "FFT_MIN_COLS", 0)
    return request.param


def test_infer_config1_as_a_short_row(device, fft_forced):
    meta, a = H.load_fixture("infer_config1")
    mod = _model(meta, device)
    Tg = a["w2v"].shape[2]
    T_rows, row = [80, Tg, 123], 1
    r = np.random.default_rng(1)
    d = lambda v: torch.from_numpy(v).to(device)
    mel = d(_ragged(a["mel"], T_rows, row, r))
    w2v = d(_ragged(a["w2v"], T_rows, row, r))
    f0 = d(_ragged(a["f0"], T_rows, row, r, scale=0.5))
    noise = d(_ragged(a["noise"], T_rows, row, r))
    o, e_ = mod.infer(mel, w2v, torch.tensor(T_rows, device=device), f0, noise=noise, row_exact=True)
    _check(o[row], a["out0"][0], 320 * Tg, "o")
    _check(e_[row], a["out1"][0], 4 * Tg, "e_")


def test_vc_noise_control_as_a_short_row(device, fft_forced):
    meta, a = H.load_fixture("vc_noise_control")
    mod = _model(meta, device)
    Tg = a["w2v"].shape[2]
    T_rows, row = [Tg, 80, 123], 0
    r = np.random.default_rng(2)
    d = lambda v: torch.from_numpy(v).to(device)
    w2v = d(_ragged(a["w2v"], T_rows, row, r))
    f0 = d(_ragged(a["f0"][:, None], T_rows, row, r, scale=0.5))
    noise = d(_ragged(a["noise"], T_rows, row, r))
    B = len(T_rows)
    mel = d(np.concatenate([np.repeat(a["mel"][:1], B, 0), np.repeat(a["mel"][1:], B, 0)]))   # B prompts, B denoised
    trg_len = torch.tensor([int(a["trg_length"][0])] * B + [int(a["trg_length"][1])] * B, device=device)
    o = mod.voice_conversion_noise_control(w2v, torch.tensor(T_rows, device=device), mel, trg_len, f0,
                                           noise_scale=meta["noise_scale"], denoise_ratio=meta["denoise_ratio"],
                                           noise=noise, row_exact=True)
    _check(o[row], a["out0"][0], 320 * Tg, "vc_noise_control")


def test_vc_plain_as_a_short_row(device, fft_forced):
    meta, a = H.load_fixture("vc_plain")
    mod = _model(meta, device)
    Tg, Tm = a["w2v"].shape[2], a["mel"].shape[2]
    T_rows, row = [80, 123, Tg], 2
    r = np.random.default_rng(3)
    d = lambda v: torch.from_numpy(v).to(device)
    w2v = d(_ragged(a["w2v"], T_rows, row, r))
    f0 = d(_ragged(a["f0"][:, None], T_rows, row, r, scale=0.5))
    noise = d(_ragged(a["noise"], T_rows, row, r))
    # every row its own prompt; the golden row's prompt (Tm frames) padded with junk to the longest one
    p_lens = [60, 31, int(a["trg_length"][0])]
    mel = r.standard_normal((3, 80, max(p_lens + [Tm]))).astype(np.float32)
    mel[row, :, :Tm] = a["mel"][0]
    o = mod.voice_conversion(w2v, torch.tensor(T_rows, device=device), d(mel), torch.tensor(p_lens, device=device), f0,
                             noise_scale=meta["noise_scale"], noise=noise, uncond=bool(meta.get("uncond", False)),
                             row_exact=True)
    _check(o[row], a["out0"][0], 320 * Tg, "vc_plain")
