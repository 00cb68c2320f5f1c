"""GPU (-m gpu): hsp_duration_scaled_f32 (csrc/hsp_frontend.hip) against include/hsp.h.

Bit equality throughout: at scale 1 against hsp_duration_f32 (``dur`` and ``frames``), for other scales against
``numpy.ceil`` on the fp32 products formed in the stated order (tests/f0_edit_ref.scaled_durations).  The products are
IEEE fp32 products on both sides; what may differ by an ulp is expf itself, so the log-durations of the predicted case
are nudged until every product (formed in float64) lies at least 1e-3 from an integer, asserted -- over a hundred fp32
ulps of the largest product (below 128: 7.6e-6), so the ceil cannot depend on it.

B = 4 rows at N in {1, 255, 256, 257, 1003}: lengths N, N / 2, 0 and 1, padded row strides, poisoned padding."""
import numpy as np
import pytest
import torch

import f0_edit_ref as R
from test_prosody_controls_host import einval_cases

pytestmark = pytest.mark.gpu

NS = (1, 255, 256, 257, 1003)
PAD = 5
LS = 1.3


def _strided(a, device):
    buf = torch.full((a.shape[0], a.shape[1] + PAD), float("nan"), dtype=torch.float32, device=device)
    buf[:, :a.shape[1]] = torch.from_numpy(a).to(device)
    return buf, buf[:, :a.shape[1]]


def _launch(device, lengths, N, logw=None, dur=None, scale=None, length_scale=1.0):
    """One launch of either entry point -> (dur [4, N], frames [4]); the padding of ``dur`` must stay untouched."""
    from megatts2_hierspeechpp_amd import _lib as L
    lens = torch.from_numpy(lengths).to(device)
    dbuf, d = _strided(np.zeros((4, N), np.float32) if dur is None else dur, device)
    if dur is None:
        d.fill_(float("nan"))
    lw = None if logw is None else _strided(logw, device)[1]
    frames = torch.full((4,), float("nan"), dtype=torch.float32, device=device)
    args = [L.fptr(lw), 0 if lw is None else lw.stride(0), L.ptr(lens), float(length_scale), L.fptr(d), d.stride(0),
            L.fptr(frames), 4, N]
    if scale is None:
        L.call("hsp_duration_f32", *args)
    else:
        sc = _strided(scale, device)[1]
        L.call("hsp_duration_scaled_f32", *args, L.fptr(sc), sc.stride(0))
    torch.cuda.synchronize()
    assert torch.isnan(dbuf[:, N:]).all()
    return d.clone(), frames


def _case(N):
    r = np.random.default_rng(100 + N)
    lengths = np.array([N, N // 2, 0, 1], np.int64)
    scale = r.uniform(0.25, 4.0, (4, N)).astype(np.float32)
    logw = r.uniform(-1.0, 2.5, (4, N)).astype(np.float32)
    for _ in range(200):
        p = np.exp(logw.astype(np.float64)) * np.float64(np.float32(LS)) * scale
        near = np.abs(p - np.round(p)) < 1e-3
        if not near.any():
            break
        logw[near] += np.float32(0.01)
    assert np.abs(p - np.round(p)).min() >= 1e-3 and p.max() < 128.0
    whole = np.ceil(np.exp(logw)).astype(np.float32)           # caller-supplied durations are whole frame counts
    return lengths, scale, logw, whole


@pytest.mark.parametrize("N", NS)
def test_scale_1_is_bit_identical_to_the_unscaled_launch(device, N):
    lengths, _, logw, whole = _case(N)
    ones = np.ones((4, N), np.float32)
    for ls in (1.0, LS):
        a = _launch(device, lengths, N, logw=logw, length_scale=ls)
        b = _launch(device, lengths, N, logw=logw, length_scale=ls, scale=ones)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), ls
    a = _launch(device, lengths, N, dur=whole)
    b = _launch(device, lengths, N, dur=whole, scale=ones)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert a[1].tolist() == [float(whole[k, :lengths[k]].sum()) for k in range(4)]


@pytest.mark.parametrize("N", NS)
def test_other_scales_against_numpy_ceil(device, N):
    lengths, scale, logw, whole = _case(N)
    got, frames = _launch(device, lengths, N, logw=logw, length_scale=LS, scale=scale)
    want, want_frames = R.scaled_durations(np.exp(logw), lengths, scale, LS)
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(frames.cpu().numpy(), want_frames)
    assert want[0].min() >= 1.0 and not want[2].any() and not want[3, 1:].any()
    got, frames = _launch(device, lengths, N, dur=whole, scale=scale)
    want, want_frames = R.scaled_durations(whole, lengths, scale)
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(frames.cpu().numpy(), want_frames)
    # a row does not depend on the others: the batch against the same rows in another order
    perm = np.array([2, 0, 3, 1])
    again, f2 = _launch(device, lengths[perm], N, logw=logw[perm], length_scale=LS, scale=scale[perm])
    first, f1 = _launch(device, lengths, N, logw=logw, length_scale=LS, scale=scale)
    assert torch.equal(again, first[torch.from_numpy(perm).to(device)]) and torch.equal(f2, f1[torch.from_numpy(perm).to(device)])


def test_the_front_end_takes_the_scaled_launch_only_when_a_scale_is_given(device, monkeypatch):
    """``_tc_latent`` through a recording `_lib.call`: hsp_duration_f32 without a scale, as it always has, and
    hsp_duration_scaled_f32 with one; scales of 1 give the frames and the x_frame of the unscaled call bit for bit."""
    import helpers as H
    from megatts2_hierspeechpp_amd import _lib as L, synth
    from megatts2_hierspeechpp_amd.inference_plm import N_LANGUAGE, N_TONE, N_VOCAB
    from megatts2_hierspeechpp_amd.ttv_v1.t2w2v_transformer import SynthesizerTrn
    ttv = SynthesizerTrn(N_VOCAB, N_TONE, N_LANGUAGE, 641, 320, 16000, 60, **H.TTV_MODEL)
    ttv.load_state_dict({k: torch.from_numpy(synth.synth_tensor("ttv." + k, tuple(v.shape), 7))
                         for k, v in ttv.state_dict().items()})
    ttv.finalize(device)
    r = np.random.default_rng(3)
    ids = torch.from_numpy(r.integers(12, 113, (2, 6))).to(device)
    tone = torch.from_numpy(r.integers(0, 11, (2, 6))).to(device)
    lang = torch.where(ids < 74, 1, 2)
    mel = torch.from_numpy(r.standard_normal((2, 80, 30)).astype(np.float32)).to(device)
    lens = lambda v: torch.tensor(v, dtype=torch.int64, device=device)  # noqa: E731
    seen, real = [], L.call

    def recording(name, *a):
        seen.append(name)
        return real(name, *a)

    monkeypatch.setattr(L, "call", recording)
    plain = ttv.inf_extract_tc_latent(ids, lens([6, 4]), mel, lens([30, 22]), tone, lang)
    assert seen.count("hsp_duration_f32") == 1 and "hsp_duration_scaled_f32" not in seen
    del seen[:]
    ones = ttv.inf_extract_tc_latent(ids, lens([6, 4]), mel, lens([30, 22]), tone, lang,
                                     phone_scale=torch.ones(2, 6, device=device))
    assert seen.count("hsp_duration_scaled_f32") == 1 and "hsp_duration_f32" not in seen
    assert torch.equal(ones[2], plain[2]) and torch.equal(ones[0], plain[0])
    slow = ttv.inf_extract_tc_latent(ids, lens([6, 4]), mel, lens([30, 22]), tone, lang,
                                     phone_scale=torch.full((2, 6), 2.0, device=device))
    print(f"frames / 2 at scale 1: {plain[2].tolist()}, at scale 2: {slow[2].tolist()}")
    assert (slow[2] >= plain[2]).all() and (slow[2] <= 2 * plain[2]).all()     # ceil(x) <= ceil(2 x) <= 2 ceil(x)


def test_bad_arguments_are_refused_before_any_launch():
    assert einval_cases() == 30
