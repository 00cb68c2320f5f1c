"""Host checks of the prosody-code path (no GPU): the float64 restatement of hsp_prosody_encode_f32 (tests/prosody_ref.py)
against the oracle, torch and the reference fixtures; the conditions the exact-code GPU comparisons rely on; the harness's
index rule and argument rules; the entry point's ABI and refusals."""
from __future__ import annotations

import ctypes
import glob
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import prosody_ref as R
from oracle import hsp_oracle as O
import helpers

ROOT = R.ROOT
POOL, D = R.POOL, R.D


def _sd(w):
    return {k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in w.items()}


def _oracle_row(x, n, w):
    """The reference's own composition on one row whose length T is a multiple of 8: oracle PLMConv, F.max_pool1d,
    oracle PLMConv and nearest code, in float64."""
    sd = _sd(w)
    T = x.shape[1]
    xt = torch.from_numpy(np.asarray(x, np.float64))[None]
    m = (torch.arange(T) < n).double()[None, None]
    mp = (torch.arange(T // POOL) < -(-n // POOL)).double()[None, None]
    h = O.plm_conv(sd, "plm_conv1", xt, m)
    q = O.plm_conv(sd, "plm_conv2", F.max_pool1d(h, POOL, POOL), mp)
    return O.vq_nearest(sd[R.EMBED], q)[0].numpy(), q[0].numpy(), h[0].numpy()


def test_restatement_matches_oracle_and_torch():
    w = R.weights()
    for T, lengths in ((64, (64, 41, 9, 1)), (136, (136, 130)), (40, (40,))):
        mel = R.mel_case(lengths, T, 8100 + T)[:, :D]
        for b, n in enumerate(lengths):
            code, _, q, h = R.encode_row(mel[b], n, w)
            ocode, oq, oh = _oracle_row(mel[b], n, w)
            npool = -(-n // POOL)
            assert np.abs(h - oh).max() < 1e-12 and np.abs(q - oq).max() < 1e-12
            assert (code[:npool] == ocode[:npool]).all(), (T, n)


def test_restatement_zero_pads_a_length_that_is_no_multiple_of_eight():
    """T = 43 equals the same rows in a T = 48 batch (frames >= T count as zeros), for both outputs."""
    w = R.weights()
    mel, lengths = R.cases()["t43"]
    x = mel[:, :D]
    a = R.encode(x, lengths, w)
    b = R.encode(np.pad(x, ((0, 0), (0, 0), (0, 5)), constant_values=3.0), lengths, w)
    assert (a["codes"] == b["codes"][:, :43]).all() and (a["pooled"] == b["pooled"]).all()
    assert a["pooled"].shape == (2, 6) and (a["codes"][1, 30:] == 0).all() and (a["pooled"][1, 4:] == 0).all()
    # the strided [:, :20] view of the 80-bin mel and a contiguous copy are the same numbers
    c = R.encode(np.ascontiguousarray(x), lengths, w)
    assert (a["codes"] == c["codes"]).all()
    # a row does not depend on its neighbours nor on the padding after its length
    alone = R.encode(x[1:2, :, :30], lengths[1:], w)
    assert (alone["pooled"][0] == a["pooled"][1, :4]).all()


def _fixtures():
    return sorted(glob.glob(os.path.join(R.GOLDEN, "*.npz")))


def test_reference_fixtures_match_the_restatement_with_margin():
    files = _fixtures()
    assert [os.path.basename(f) for f in files] == ["tc_code_b2.npz", "tc_code_b3.npz", "tc_code_t40.npz", "tc_code_t64.npz"]
    for f in files:
        z = np.load(f)
        meta = json.loads(bytes(z["meta"]).decode())
        w = R.weights(meta["seed"])
        lengths = z["mel_spk_lengths"]
        out = R.encode(z["mel_spk"][:, :D], lengths, w)
        # the condition: EVERY compared pooled frame is at least MIN_MARGIN from a different answer, none left out
        for margin in (z["margin"], out["margin"]):
            m = R.compared_margin(margin, lengths)
            assert m.size == sum(-(-int(n) // POOL) for n in lengths) and np.isfinite(m).all()
            assert m.min() >= R.MIN_MARGIN, (f, m.min())
        # the reference's margins come from its float32 q: they agree with the float64 ones to float32 rounding
        assert np.nanmax(np.abs(z["margin"] - out["margin"])) < 1e-3
        assert (out["codes"] == z["lr_codes"]).all(), f
        assert abs(meta["min_margin"] - np.nanmin(z["margin"])) < 1e-12


def test_gpu_case_inputs_have_margin():
    """The exact-code comparisons of tests/test_gpu_prosody.py rest on this: measured minimum margins are printed."""
    w = R.weights()
    for name, (mel, lengths) in R.cases().items():
        out = R.encode(mel[:, :D], lengths, w)
        m = R.compared_margin(out["margin"], np.minimum(lengths, mel.shape[2]))
        assert m.size == sum(-(-int(n) // POOL) for n in lengths)
        print(name, "min margin", m.min() if m.size else None)
        assert m.size == 0 or m.min() >= R.MIN_MARGIN, (name, m.min())
    mel, lengths, w2 = R.negative_tail_case()
    m = R.compared_margin(R.encode(mel[:, :D], lengths, w2)["margin"], lengths)
    assert m.size == 2 + 3 + 3 and m.min() >= R.MIN_MARGIN, m.min()


def test_tie_case_pins_the_lowest_index():
    mel, lengths, w2, win, lo, hi = R.tie_case()
    base = R.encode(mel[:, :D], lengths, R.weights())
    tied = R.encode(mel[:, :D], lengths, w2)
    first = lo if lo is not None else win
    assert hi > win and (lo is None or lo < win)
    want = np.where(base["pooled"] == win, first, base["pooled"])
    want[1, 4:] = 0
    assert (tied["pooled"] == want).all() and tied["pooled"][0, 0] == first
    assert (base["pooled"] == win).sum() >= 1
    # every frame that did not choose the duplicated code keeps its margin: only the tie itself is decided by the rule
    keep = (base["pooled"] != win) & np.isfinite(base["margin"])
    assert np.nanmin(tied["margin"][keep]) >= R.MIN_MARGIN


def test_negative_tail_case_takes_the_padding_zero():
    mel, lengths, w = R.negative_tail_case()
    bias = np.asarray(w["plm_conv1.conv2.bias"], np.float64)
    assert (bias < 0).all()
    skipped = 0
    for b, n in enumerate(lengths):
        code, _, q, h = R.encode_row(mel[b, :D], int(n), w)
        assert (h[:, :n] == bias[:, None]).all() and (h[:, n:] == 0).all()
        hp = h.reshape(D, -1, POOL).max(-1)
        last = -(-int(n) // POOL) - 1
        if n % POOL:
            assert (hp[:, last] == 0).all()                      # the straddling window: the padding zero in all 20 channels
            # a pool that skips the masked frames takes the bias there instead and ends on another code
            p2 = hp.copy()
            p2[:, last] = bias
            mp = (np.arange(hp.shape[1]) <= last).astype(np.float64)[None]
            q2 = R.plm_conv(p2, mp, w, "plm_conv2")
            e = np.asarray(w[R.EMBED], np.float64)
            code2 = ((q2.T[:, None, :] - e[None]) ** 2).sum(-1).argmin(-1)
            skipped += int((code2[:last + 1] != code[:last + 1]).sum())
        assert (hp[:, :last + (0 if n % POOL else 1)] == bias[:, None]).all()
    assert skipped >= 1


def test_fit_prosody_codes_against_a_loop():
    from megatts2_hierspeechpp_amd.inference_plm import fit_prosody_codes
    r = np.random.default_rng(5)
    codes = r.integers(0, 1024, (6, 300))
    ls = np.array([300, 1, 300, 7, 123, 64])
    lt = np.array([300, 200, 1, 7, 61, 128])          # identity, the largest stretch, the largest squeeze, identity, ...
    for width in (300, 128):
        got = fit_prosody_codes(torch.from_numpy(codes), torch.from_numpy(ls), torch.from_numpy(lt), width=width).numpy()
        assert got.dtype == np.int64 and (got == R.fit_codes(codes, ls, lt, width)).all()
    got = fit_prosody_codes(torch.from_numpy(codes), torch.from_numpy(ls), torch.from_numpy(lt))
    assert got.shape == (6, 300)
    assert (got[0].numpy() == codes[0]).all() and (got[3, :7].numpy() == codes[3, :7]).all() and (got[3, 7:] == 0).all()
    assert got[2, 0] == codes[2, 150] and (got[1, :200] == codes[1, 0]).all()
    one = fit_prosody_codes(torch.from_numpy(codes[0]), 300, 150)                    # 1-D codes, plain ints
    assert one.shape == (1, 150) and (one[0].numpy() == codes[0, 1::2]).all()


def test_harness_argument_rules():
    from megatts2_hierspeechpp_amd import inference_plm as IP
    from megatts2_hierspeechpp_amd._lib import HspError
    from megatts2_hierspeechpp_amd.ttv_v1.t2w2v_transformer import PlmSampling
    import inspect
    c = torch.zeros(1, 16, dtype=torch.int64)
    none = (None,) * 8
    for kw in (dict(plm_sampling=PlmSampling()), dict(plm_causal=True), dict(plm_causal=True, plm_prefix=c[:, :4])):
        with pytest.raises(HspError, match="exclude each other"):
            IP.tts(None, *none, prosody_codes=c, **kw)
        with pytest.raises(HspError, match="exclude each other"):
            IP.tts_from_prompt(None, None, None, None, None, None, prosody_codes=c, **kw)
    with pytest.raises(HspError, match="prosody_codes and takes > 1"):
        IP.tts_from_prompt(None, None, None, None, None, None, prosody_codes=c, takes=2)
    with pytest.raises(HspError, match="without prosody_codes"):
        IP.tts(None, *none, prosody_lengths=torch.tensor([16]))
    for fn in (IP.tts, IP.tts_from_prompt, IP.tts_from_prompt_file):
        p = inspect.signature(fn).parameters
        assert p["prosody_codes"].default is None and p["prosody_lengths"].default is None
    assert list(inspect.signature(IP.prosody_from_audio).parameters) == ["models", "mel_fn", "audio", "sr", "lengths"]
    assert list(inspect.signature(IP.fit_prosody_codes).parameters)[:3] == ["codes", "src_frames", "dst_frames"]
    from megatts2_hierspeechpp_amd.ttv_v1.t2w2v_transformer import SynthesizerTrn
    assert list(inspect.signature(SynthesizerTrn.extract_tc_latent_code).parameters) == [
        "self", "x", "x_lengths", "mel_spk", "mel_spk_lengths", "tone", "language", "dur", "mrte_mel", "mrte_mel_lengths"]
    assert list(inspect.signature(SynthesizerTrn.prosody_codes).parameters) == ["self", "mel", "mel_lengths", "pooled"]


# ------------------------------------------------------------------------------------------------------------ ABI
def _args(L, **kw):
    a = L.ProsodyArgs()
    a.x, a.lengths, a.embed, a.codes, a.pooled = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000   # never dereferenced: all refused
    a.w1a, a.w1b, a.w2a, a.w2b, a.b1a, a.b1b, a.b2a, a.b2b = (0x6000 + 0x100 * i for i in range(8))
    a.x_bs, a.x_cs, a.c_bs, a.p_bs = 80 * 64, 64, 64, 8
    a.B, a.D, a.T, a.k, a.w_ld, a.bins = 2, 20, 64, 5, 20, 1024
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_refusals_are_decided_on_the_host():
    from megatts2_hierspeechpp_amd import _lib as L
    lib = L.lib()
    call = lambda a: lib.hsp_prosody_encode_f32(ctypes.byref(a), None)          # NULL stream: nothing may be launched
    assert lib.hsp_prosody_encode_f32(None, None) == L.EINVAL
    refused = [dict(x=None), dict(lengths=None), dict(embed=None), dict(codes=None, pooled=None), dict(w1a=None),
               dict(w1b=None), dict(w2a=None), dict(w2b=None), dict(D=33), dict(D=0), dict(D=-20), dict(bins=1025),
               dict(bins=0), dict(bins=-1), dict(k=3), dict(k=7), dict(k=0), dict(B=0), dict(B=-1), dict(B=65536),
               dict(T=0), dict(T=-8), dict(w_ld=19), dict(w_ld=0)]
    for kw in refused:
        assert call(_args(L, **kw)) == L.EINVAL, kw


def test_names_agree_across_header_ctypes_map_and_library(tmp_path):
    from megatts2_hierspeechpp_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "hsp.h")).read()
    declared = set(re.findall(r"\b(hsp_[a-z0-9_]+)\s*\(", hdr))
    lib = L.lib()
    nm = "hsp_prosody_encode_f32"
    assert nm in declared and nm in L.SIGNATURES and getattr(lib, nm) is not None
    assert L.SIGNATURES[nm][1][0] is ctypes.POINTER(L.ProsodyArgs)
    assert lib.hsp_version() == 104 and int(re.search(r"#define HSP_VERSION (\d+)", hdr).group(1)) == 104
    vmap = open(os.path.join(ROOT, "megatts2_hierspeechpp_amd", "csrc", "hsp.map")).read()
    assert "global: hsp_*;" in vmap and "prosody" not in vmap
    helpers.assert_struct_layouts(tmp_path, {"hsp_prosody_args": L.ProsodyArgs})


def test_the_distance_is_stated_once():
    """vq_nearest_kernel and prosody_encode_kernel call one device function for the distance arithmetic."""
    csrc = os.path.join(ROOT, "megatts2_hierspeechpp_amd", "csrc")
    dev = open(os.path.join(csrc, "hsp_device.h")).read()
    assert dev.count("float hsp_vq_dist(") == 1 and dev.count("float hsp_vq_sq(") == 1
    for f in ("hsp_frontend.hip", "hsp_prosody.hip"):
        s = open(os.path.join(csrc, f)).read()
        assert "hsp_vq_dist(" in s and "hsp_vq_sq(" in s and "2.0f *" not in s, f
    assert R.tile_frames() >= 1
