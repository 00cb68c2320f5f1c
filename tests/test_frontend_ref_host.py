"""CPU: the float64 restatements of tests/frontend_ref.py against what the project already trusts (the oracle, torch),
and the input conditions the GPU kernel tests rely on, for the exact seeds those tests use:

  * every duration target is at least 1e-3 from an integer after logw is rounded to fp32,
  * every nearest-code column has a float64 margin of at least 1e-4 (zero columns may be left out),
  * the fp32 oracle's Gaussian upsampling is within a tenth of the project bar of float64, so the bar leaves room
    for a kernel that sums in another order.

    python -m pytest tests/test_frontend_ref_host.py -q
"""
import math

import numpy as np
import pytest
import torch

import frontend_ref as R
import helpers as H
from oracle import hsp_oracle as O


@pytest.fixture(autouse=True)
def _threads():
    torch.set_num_threads(min(16, torch.get_num_threads()))


def _oracle_gauss_rows(case):
    """oracle.gaussian_upsampling row by row on the un-padded row (fp32), padded with zeros to the batch's T."""
    x = case["xbuf"][:, :case["C"]]
    out = np.zeros((case["B"], case["C"], case["T"]), np.float32)
    for b in range(case["B"]):
        n = int(case["lens"][b])
        d = torch.from_numpy(case["dur"][b:b + 1, :n])
        v = torch.maximum(torch.minimum(torch.from_numpy(case["rng"][b:b + 1, :n]), d * 2), torch.tensor(1e-5))
        y = O.gaussian_upsampling(torch.from_numpy(np.ascontiguousarray(x[b:b + 1, :, :n])), d, v)
        out[b, :, :y.shape[2]] = y[0].numpy()
    return out


@pytest.mark.parametrize("case", R.GAUSS_CASES, ids=lambda c: f"n{c['N']}_c{c['C']}_t{c['T']}")
def test_gaussian_restatement_and_headroom(case):
    c = R.gauss_case(**case)
    if case["T"] is not None:
        assert c["T"] == case["T"]
    assert c["N"] <= R.GAUSS_N_LIMIT and (c["frames"] == c["dur"].sum(1)).all()
    # the inputs cover what the case list promises
    valid = np.arange(c["N"])[None] < c["lens"][:, None]
    assert (c["dur"][~valid] == 0).all() and (c["frames"] >= 1).all()
    if c["N"] >= 33:
        assert (c["dur"][valid] == 0).any(), "no zero duration"
        assert (c["rng"][valid] > 2 * c["dur"][valid]).any() and (c["rng"][valid] < 2 * c["dur"][valid]).any()
    ref = R.gaussian_upsample(c["xbuf"][:, :c["C"]], c["dur"], c["rng"], c["lens"], c["frames"], c["T"])
    got = _oracle_gauss_rows(c)
    err = float(np.abs(got - ref).max())
    print(f"gauss N={c['N']} C={c['C']} T={c['T']}: max|oracle fp32 - float64| = {err:.2e}, bar {H.tol_for(ref):.1e}")
    assert err <= 0.1 * H.tol_for(ref), (err, H.tol_for(ref))
    for b in range(c["B"]):          # the tail is zero
        assert (ref[b, :, int(c["frames"][b]):] == 0).all()


def test_gaussian_restatement_masks_padding_phones():
    """Values parked in the padding (phones >= len, frames >= frames[b]) do not reach the restatement's output."""
    c = R.gauss_case(seed=31, N=9, C=8)
    x = c["xbuf"][:, :8].copy()
    base = R.gaussian_upsample(x, c["dur"], c["rng"], c["lens"], c["frames"], c["T"])
    for b in range(c["B"]):
        x[b, :, c["lens"][b]:] = 1e6
    dur = c["dur"].copy()
    dur[1, c["lens"][1]:] = 7.0
    assert np.array_equal(base, R.gaussian_upsample(x, dur, c["rng"], c["lens"], c["frames"], c["T"]))


@pytest.mark.parametrize("N", R.DUR_NS)
@pytest.mark.parametrize("scale", R.DUR_SCALES)
def test_duration_targets_stay_clear_of_integers(N, scale):
    logw, lens = R.duration_case(100 + N, N, scale)
    dur, frames, val = R.duration_exact(logw, lens, scale)
    dist = np.abs(val - np.rint(val))
    assert float(dist.min()) >= R.DUR_MIN_DIST, dist.min()
    assert float(val.max()) < 64.0
    # torch's fp32 expression agrees with the float64 one on these inputs
    want = torch.ceil(torch.exp(torch.from_numpy(logw)) * scale).numpy()
    valid = np.arange(N)[None] < np.clip(lens, 0, N)[:, None]
    assert np.array_equal(np.where(valid, want, 0.0), dur)
    assert (frames == dur.sum(1)).all() and frames[0] == 0 and float(frames.max()) < 2 ** 24
    assert lens[0] == 0 and lens[-1] > N and lens[2] == N


def test_duration_exact_points():
    for scale, want in ((1.0, 1.0), (2.0, 2.0)):
        dur, frames, _ = R.duration_exact(np.zeros((1, 5), np.float32), [3], scale)
        assert dur.tolist() == [[want] * 3 + [0.0] * 2] and frames.tolist() == [3 * int(want)]
    kept, s = R.duration_keep(np.array([[3, 0, 7, 9]], np.float32), [3])
    assert kept.tolist() == [[3, 0, 7, 0]] and s.tolist() == [10.0]


def test_pointwise_restatements_match_torch():
    r = np.random.default_rng(41)
    tabs = [r.standard_normal((n, 6)).astype(np.float32) for n in (13, 5, 3)]
    ids = [r.integers(0, t.shape[0], (2, 7)) for t in tabs]
    sc = math.sqrt(6)
    tt = lambda a: torch.from_numpy(a)
    emb = torch.nn.functional.embedding
    for k in (1, 2, 3):
        want = emb(tt(ids[0]), tt(tabs[0])) * sc
        if k == 2:
            want = want + emb(tt(ids[1]), tt(tabs[1])) * sc
        if k == 3:   # TextEncoder.forward's own expression (t2w2v_transformer.py:127-131)
            want = want + emb(tt(ids[1]), tt(tabs[1])) * sc + emb(tt(ids[2]), tt(tabs[2])) * sc
        assert np.array_equal(R.embedding_sum(ids[:k], tabs[:k], sc), want.transpose(1, 2).numpy())
    x = r.standard_normal((2, 5, 11)).astype(np.float32)
    cb = r.standard_normal((2, 5)).astype(np.float32)
    assert np.array_equal(R.add_cbias(x, cb), (tt(x) + tt(cb).unsqueeze(-1)).numpy())
    thr = math.log(55.0)
    x[0, 0, :4] = [np.float32(thr), -np.inf, np.nan, np.inf]
    y = tt(x.copy())
    y[y < thr] = 0
    assert np.array_equal(R.zero_below(x, thr), y.numpy(), equal_nan=True)
    z = R.zero_below(x, thr)[0, 0]
    assert z[0] == np.float32(thr) and z[1] == 0 and np.isnan(z[2]) and z[3] == np.inf
    for L, k in ((11, 8), (11, 3), (16, 8), (5, 5)):
        xx = r.standard_normal((2, 3, L)).astype(np.float32)
        assert np.array_equal(R.maxpool1d(xx, k), torch.nn.functional.max_pool1d(tt(xx), k, k).numpy())


@pytest.mark.parametrize("case", R.VQ_CASES, ids=lambda c: f"b{c['B']}_t{c['T']}_r{c['rep']}")
def test_vq_restatement_and_margins(case):
    xbuf, embed = R.vq_case(**case)
    x = xbuf[:, 1:21, :case["T"]]
    codes, margin = R.vq_nearest(x, embed)
    print(f"vq seed {case['seed']}: min float64 margin {margin.min():.2e} over {margin.size} columns")
    assert float(margin.min()) >= R.VQ_MIN_MARGIN, "a column of this seed would have to be left out: pick another seed"
    want = O.vq_nearest(torch.from_numpy(embed), torch.from_numpy(np.ascontiguousarray(x)))
    assert np.array_equal(codes, want.numpy())
    Tout = case["rep"] * case["T"] - case["cut"]
    held, _ = R.vq_nearest(x, embed, case["rep"], Tout)
    assert held.shape == (case["B"], Tout)
    assert np.array_equal(held, np.repeat(codes, case["rep"], 1)[:, :Tout])


def test_vq_tie_case_first_index_wins():
    x, embed = R.vq_tie_case()
    codes, _ = R.vq_nearest(x, embed)
    d = R.vq_sqdist(x, embed)
    assert (d.min(-1) == 0).all()
    assert codes[0, :4].tolist() == [5, 5, 5, 299]
    assert ((d == 0).sum(-1) >= 2).sum() > 20, "too few tied columns"
    assert not ((codes >= 512) & (codes < 812)).any() and not (codes == 1000).any()     # never the later copy
    want = O.vq_nearest(torch.from_numpy(embed), torch.from_numpy(x))
    assert np.array_equal(codes, want.numpy())


@pytest.mark.parametrize("n", [1000, 1023, 1024, 1025, 5000])
def test_peak_int16_restatement(n):
    x, lens, gains = R.peak_case(50 + n % 7, n)
    out = R.peak_int16(x, lens, gains)
    assert out.dtype == np.int16 and out.shape == x.shape
    # rows 0 and 2 at gain 0.999 are the oracle's tts_postprocess on the un-padded row
    for b in (0, 2):
        L = int(lens[b])
        assert np.array_equal(out[b, :L], O.tts_postprocess(torch.from_numpy(x[b, :L].copy())))
        assert (out[b, L:] == 0).all()
    # the reference expression itself: a negative peak, and a silent row (0 / 0 = NaN -> 0 in numpy's cast)
    a = torch.from_numpy(x[1].copy())
    assert np.array_equal(out[1], (a / a.abs().max() * 32767.0 * 1.0).numpy().astype("int16")) and out[1].min() == -32767
    z = torch.zeros(8)
    with np.errstate(invalid="ignore"):
        assert (z / z.abs().max() * 32767.0 * 0.999).numpy().astype("int16").tolist() == [0] * 8
    assert (out[3] == 0).all() and (out[4] == 0).all()
    # a gain above 1 saturates instead of wrapping
    assert out[5].max() == 32767 or out[5].min() == -32768
    v = x[5, :n - 1] / np.abs(x[5, :n - 1]).max() * np.float32(32767.0) * gains[5]
    inside = np.abs(v) < 32767
    assert np.array_equal(out[5, :n - 1][inside], v[inside].astype(np.int16))


def test_lstm_restatement_is_torch_float64():
    torch.manual_seed(5)
    ref = torch.nn.LSTM(9, 4, num_layers=2, bidirectional=True, batch_first=True).eval()
    x = torch.randn(3, 11, 9)
    lens = torch.tensor([11, 1, 6])
    y = R.lstm_packed_f64(ref.state_dict(), x, lens, 9, 4, 2)
    assert y.dtype == torch.float64 and y.shape == (3, 11, 8)
    assert (y[1, 1:] == 0).all() and (y[2, 6:] == 0).all()
    # against the oracle's hand-written recurrence on one un-padded row
    sd = {"l." + k: v for k, v in ref.state_dict().items()}
    with torch.no_grad():
        want = O.bilstm(sd, "l", x[2, :6], 2)
    assert float((y[2, :6] - want.double()).abs().max()) < 1e-5
