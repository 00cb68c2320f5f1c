"""GPU (-m gpu): the text -> wav2vec stages against the CPU oracle at sentence size -- ragged batches of three rows
through ``inf_extract_tc_latent`` (120 / 73 / 9 phones, prompts of 300 / 211 / 150 mel frames; pinned and predicted
durations, length_scale 1 and 1.3), ``inf_plm_gen`` (250 / 167 / 31 frames, one length ending in .5) and the legacy
``infer`` (60 phones, a 304-frame prompt).  The oracle runs every row alone on the un-padded row, as the reference
does; the product runs the padded batch once.  Synthetic weights (synth.synth_tensor), helpers.TTV_MODEL.

Tolerance: helpers.tol_for (1e-4 x max(1, peak of the oracle's output)); lengths, masks and codes are exact; frames
past a row's length must be exactly zero.

Oracle CPU time: the whole file, oracle and product calls together, took 1.3 s of test calls (5 s with the weight
upload) on the GPU machine with 16 threads, so no size had to shrink.

    python -m pytest tests/test_gpu_frontend_scale.py -q -m gpu
"""
import math

import numpy as np
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu

W_SEED = 7                      # weight seed of the golden fixtures
NS, TMS = (120, 73, 9), (300, 211, 150)
PRED_SEED = 3                   # text / prompt seed of the predicted-duration case (see front_inputs)
DUR_MIN_DIST = 1e-3


def _close(got, ref, name):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert np.isfinite(got).all(), name
    err, tol = float(np.abs(got.astype(np.float64) - ref).max()), H.tol_for(ref)
    print(f"{name}: max|hip - oracle| = {err:.3e} (bar {tol:.1e})")
    assert err <= tol, f"{name}: max|hip - oracle| = {err:.3e} > {tol:.1e}"


def front_inputs(seed, ns=NS, tms=TMS):
    """Padded batch of text ids / tones / languages (the id -> language rule of tools/make_golden.py) and prompt mels.
    Importable without a GPU: tools and the seed search for the predicted-duration case build the same arrays."""
    from megatts2_hierspeechpp_amd import synth
    r = np.random.default_rng(seed)
    B, Nm, Tm = len(ns), max(ns), max(tms)
    ids, tone, lang = (np.zeros((B, Nm), np.int64) for _ in range(3))
    mel = np.zeros((B, 80, Tm), np.float32)
    for b, (n, tm) in enumerate(zip(ns, tms)):
        ids[b, :n] = r.integers(1, 126, n)
        tone[b, :n] = r.integers(0, 11, n)
        lang[b, :n] = np.where(ids[b, :n] < 74, 1, np.where(ids[b, :n] < 113, 2, 0))
        mel[b, :, :tm] = synth.synth_inputs(1, tm, seed=1000 * seed + 10 * b + 1)["mel"][0]
    dur = np.zeros((B, Nm), np.float32)
    for b, n in enumerate(ns):
        dur[b, :n] = r.integers(1, 21, n)
    return dict(ids=ids, tone=tone, language=lang, mel=mel, dur=dur, lengths=np.array(ns, np.int64),
                mel_lengths=np.array(tms, np.int64))


def oracle_pre_ceil(sd, ids, mel, tone, language, length_scale=1.0):
    """exp(logw) * length_scale of one un-padded row: the value the oracle's torch.ceil sees
    (oracle.ttv_extract_tc_latent_one's own first lines)."""
    from oracle import hsp_oracle as O
    g = O.style_encoder(sd, "emb_g", mel, torch.ones(1, 1, mel.shape[2])).unsqueeze(-1)
    x = O.text_encoder(sd, "enc_p", ids, tone, language)
    h = O.mel_encoder(sd, "mel_encoder", mel)
    x = x + O.mha_plain(sd, "mha", x, h, torch.ones(1, 1, x.shape[2], h.shape[2]), 4) + O.conv1d(sd, "cond_g", g)
    return (torch.exp(O.duration_predictor(sd, "duration_predictor", x, g)) * length_scale).flatten()


def ttv_state_dict():
    from megatts2_hierspeechpp_amd import synth
    mod = H.build_module({"kind": "ttv_front", "shapes": []})
    return mod, {k: torch.from_numpy(synth.synth_tensor(k, tuple(v.shape), W_SEED)) for k, v in mod.state_dict().items()}


@pytest.fixture(scope="module")
def ttv(device):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    mod, sd = ttv_state_dict()
    mod.load_state_dict(sd, strict=True)
    mod.finalize(device)
    return mod, sd


def _front_oracle(sd, inp, length_scale, pinned):
    from oracle import hsp_oracle as O
    t = lambda a: torch.from_numpy(a)
    rows = []
    with torch.no_grad():
        for b, (n, tm) in enumerate(zip(inp["lengths"], inp["mel_lengths"])):
            a = (t(inp["ids"][b:b + 1, :n]), t(inp["mel"][b:b + 1, :, :tm]), t(inp["tone"][b:b + 1, :n]),
                 t(inp["language"][b:b + 1, :n]))
            override = t(inp["dur"][b:b + 1, :n]).unsqueeze(1) if pinned else None
            rows.append(O.ttv_extract_tc_latent_one(sd, *a, length_scale=length_scale, dur_override=override))
    return rows


def _check_front(mod, sd, device, inp, length_scale, pinned, name):
    d = lambda k: torch.from_numpy(inp[k]).to(device)
    rows = _front_oracle(sd, inp, length_scale, pinned)
    with torch.no_grad():
        xf, g, fl, mask = mod.inf_extract_tc_latent(d("ids"), d("lengths"), d("mel"), d("mel_lengths"), d("tone"),
                                                    d("language"), length_scale=length_scale,
                                                    dur=d("dur") if pinned else None)
    torch.cuda.synchronize()
    xf, g, fl, mask = xf.cpu().numpy(), g.cpu().numpy(), fl.cpu().numpy(), mask.cpu().numpy()
    want_fl = np.array([r[2] for r in rows], np.float64)
    assert np.array_equal(fl.astype(np.float64), want_fl), (name, fl, want_fl)
    T2 = max(r[0].shape[2] for r in rows)
    assert xf.shape == (len(rows), 256, T2) and mask.shape == (len(rows), 1, T2) and mask.dtype == np.bool_
    for b, (oxf, og, ofl, _) in enumerate(rows):
        n2 = oxf.shape[2]
        assert n2 == math.ceil(ofl)
        _close(xf[b, :, :n2], oxf[0].numpy(), f"{name} x_frame row {b} ({inp['lengths'][b]} phones, {n2} frames)")
        _close(g[b], og[0].numpy(), f"{name} g row {b}")
        assert (xf[b, :, n2:] == 0).all(), f"{name} row {b}: frames past the row's length must be exactly zero"
        assert mask[b, 0, :n2].all() and not mask[b, 0, n2:].any()


def test_front_pinned_durations(ttv, device):
    mod, sd = ttv
    _check_front(mod, sd, device, front_inputs(1), 1.0, True, "front pinned")


def test_front_pinned_durations_length_scale(ttv, device):
    """With caller-supplied durations the reference ignores length_scale (t2w2v_transformer.py:955-957 only scales the
    predicted ones); the call must still meet the oracle."""
    mod, sd = ttv
    _check_front(mod, sd, device, front_inputs(1), 1.3, True, "front pinned, length_scale 1.3")


def test_front_predicted_durations(ttv, device):
    """Predicted durations: ceil(exp(logw)) is discontinuous, so the inputs (seed PRED_SEED, picked on a CPU) keep the
    oracle's exp(logw) at least 1e-3 from an integer for every phone; asserted here from the oracle's own values, no
    phone left out."""
    mod, sd = ttv
    inp = front_inputs(PRED_SEED)
    t = lambda a: torch.from_numpy(a)
    with torch.no_grad():
        for b, (n, tm) in enumerate(zip(inp["lengths"], inp["mel_lengths"])):
            v = oracle_pre_ceil(sd, t(inp["ids"][b:b + 1, :n]), t(inp["mel"][b:b + 1, :, :tm]), t(inp["tone"][b:b + 1, :n]),
                                t(inp["language"][b:b + 1, :n])).double().numpy()
            dist = np.abs(v - np.rint(v))
            print(f"row {b}: exp(logw) in [{v.min():.3f}, {v.max():.3f}], min distance from an integer {dist.min():.2e}")
            assert int((dist < DUR_MIN_DIST).sum()) == 0, f"row {b}: {int((dist < DUR_MIN_DIST).sum())} phones within 1e-3"
    _check_front(mod, sd, device, inp, 1.0, False, "front predicted")


def test_plm_gen_sentence_size(ttv, device):
    """inf_plm_gen at T2 = 250 / 167 / 31 (the middle length ends in .5), random codes, per row against the oracle."""
    from oracle import hsp_oracle as O
    mod, sd = ttv
    t2s = (250, 167, 31)
    flen = np.array([250.0, 166.5, 31.0], np.float32)
    r = np.random.default_rng(83)
    B, T2 = len(t2s), max(t2s)
    xf = r.standard_normal((B, 256, T2)).astype(np.float32)
    g = r.standard_normal((B, 256, 1)).astype(np.float32)
    codes = r.integers(0, 1024, (B, T2))
    for b, n in enumerate(t2s):
        xf[b, :, n:] = 0
    d = lambda a: torch.from_numpy(a).to(device)
    with torch.no_grad():
        w2v, lf0 = mod.inf_plm_gen(d(xf), d(g), d(codes), d(flen), None)
    torch.cuda.synchronize()
    w2v, lf0 = w2v.cpu().numpy(), lf0.cpu().numpy()
    assert w2v.shape == (B, 1024, T2) and lf0.shape == (B, 4 * T2)
    t = lambda a: torch.from_numpy(a)
    for b, n in enumerate(t2s):
        with torch.no_grad():
            ow, ol = O.ttv_plm_gen_one(sd, t(xf[b:b + 1, :, :n]), t(g[b:b + 1]), t(codes[b:b + 1, :n]), float(flen[b]))
        _close(w2v[b, :, :n], ow[0].numpy(), f"plm_gen w2v row {b} (T2 = {n})")
        _close(lf0[b, :4 * n], ol[0].numpy(), f"plm_gen lf0 row {b}")
        assert (w2v[b, :, n:] == 0).all() and (lf0[b, 4 * n:] == 0).all(), f"row {b}: not zero past its length"


def test_legacy_infer_sentence_size(ttv, device):
    """The non-PLM ``infer`` with 60 phones and a prompt of 8 x 38 = 304 frames (durations summing to 608): w2v, lf0 and
    the prompt's prosody codes against oracle.ttv_infer_one."""
    from megatts2_hierspeechpp_amd import synth
    from oracle import hsp_oracle as O
    mod, sd = ttv
    n, tm = 60, 8 * 38
    inp = front_inputs(5, ns=(n,), tms=(tm,))
    r = np.random.default_rng(84)
    dur = r.integers(1, 20, (1, n)).astype(np.float32)
    while dur.sum() != 2 * tm:
        j = int(r.integers(0, n))
        dur[0, j] = min(20.0, dur[0, j] + 1) if dur.sum() < 2 * tm else max(1.0, dur[0, j] - 1)
    t = lambda a: torch.from_numpy(a)
    with torch.no_grad():
        ow, ol, ocodes = O.ttv_infer_one(sd, t(inp["ids"]), t(inp["mel"]), t(inp["tone"]), t(inp["language"]), t(dur))
    d = lambda a: torch.from_numpy(a).to(device)
    dl = lambda v: torch.tensor(v, dtype=torch.int64, device=device)
    with torch.no_grad():
        w2v, lf0, codes = mod.infer(d(inp["ids"]), dl([n]), d(inp["mel"]), dl([tm]), d(inp["tone"]), d(inp["language"]),
                                    dur=d(dur), return_codes=True)
    torch.cuda.synchronize()
    assert ocodes.shape == (1, tm // 8) and codes.shape == (1, tm)
    want = ocodes.repeat_interleave(8, dim=1).numpy()
    got = codes.cpu().numpy()
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {got.size} prompt codes differ from the oracle's"
    _close(w2v.cpu().numpy(), ow.numpy(), "legacy infer w2v")
    _close(lf0.cpu().numpy(), ol.numpy(), "legacy infer lf0")
