"""GPU (-m gpu): the pitch edit of csrc/hsp_f0_edit.hip against the float64 restatement of include/hsp.h
(tests/f0_edit_ref.py).

Bars.  The device arithmetic is double, so its error is far below half an fp32 ulp and one ulp covers a rounding tie:
every track value within one fp32 ulp of the float64 reference rounded to fp32 -- 4.8e-7 (f0_edit_ref.ULP_BELOW_8) for
outputs below 8, which f_max <= 2.9 kHz guarantees (asserted) -- and mean_hz within one ulp of its own rounded reference.
Bit equality (torch.equal): a row of a batch against the call on that row alone, identity rows against their input,
zeros over [n_b, n).

B = 4 rows at n in {1, 255, 256, 257, 1003} (one frame; below, at and above the 256 threads of the workgroup; several
strides per thread): row 0 an ordinary track cut at 3 n / 4, row 1 without a voiced frame, row 2 with n_b = 0, row 3 with
one voiced frame.  Every buffer has a padded row stride, the columns past n and the output are poisoned, and the input
holds a voiced 7.0 (1.1 kHz) from a row's length on: a read past n_b moves the mean, a write past n shows."""
import numpy as np
import pytest
import torch

import f0_edit_ref as R
from test_prosody_controls_host import einval_cases

pytestmark = pytest.mark.gpu

NS = (1, 255, 256, 257, 1003)
PAD = 13


def _case(n):
    l = np.zeros((4, n), np.float32)
    l[0] = R.track(n, 10 + n, voiced=0.8)
    l[0, 0] = R.hz_to_l(150.0)                                 # voiced at n = 1 too
    l[2] = R.track(n, 30 + n)
    l[3, n // 2] = R.hz_to_l(210.0)
    lengths = np.array([max(1, 3 * n // 4), n, 0, n], np.int64)
    for b in range(4):
        l[b, lengths[b]:] = 7.0                                # never read
    r = np.random.default_rng(n)
    ops = dict(shift=np.array([3.5, -2.0, 1.0, -7.0], np.float32), range_=np.array([1.6, 0.5, 2.0, 0.0], np.float32),
               target_hz=np.array([0.0, 120.0, 300.0, 180.0], np.float32),
               offsets=r.uniform(-4.0, 4.0, (4, n)).astype(np.float32))
    return l, lengths, ops


def _padded(a, device, fill=float("nan")):
    """A [B, n] device view of row stride n + PAD; the padding holds ``fill``."""
    buf = torch.full((a.shape[0], a.shape[1] + PAD), fill, dtype=torch.float32, device=device)
    buf[:, :a.shape[1]] = torch.from_numpy(a).to(device)
    return buf, buf[:, :a.shape[1]]


def _run(device, l, lengths=None, shift=None, range_=None, target_hz=None, offsets=None, f_min=55.0, f_max=1100.0,
         in_place=False):
    from megatts2_hierspeechpp_amd import functional as Fh
    d = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(device)  # noqa: E731
    _, x = _padded(l, device)
    off = None if offsets is None else _padded(offsets, device)[1]
    obuf, out = (None, x) if in_place else _padded(np.zeros_like(l), device)
    if not in_place:
        obuf.fill_(float("nan"))                               # a frame the kernel does not write shows
    got, mean = Fh.f0_edit(x, d(lengths), d(shift), d(range_), d(target_hz), off, f_min, f_max, out=out, return_mean=True)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    if not in_place:
        assert torch.isnan(obuf[:, l.shape[1]:]).all()         # nothing written past n
    return got.clone(), mean


def _check(got, mean, l, lengths=None, **ops):
    want, want_mean = R.edit_rows(l, lengths, **ops)
    assert want.max() < 8.0
    w32 = want.astype(np.float32)
    err = np.abs(got.cpu().numpy().astype(np.float64) - w32.astype(np.float64)).max()
    m32 = want_mean.astype(np.float32)
    merr = np.abs(mean.cpu().numpy().astype(np.float64) - m32.astype(np.float64))
    print(f"n = {l.shape[1]}: max |out - ref| = {err:.3e} (bar {R.ULP_BELOW_8:.1e}), mean_hz {mean.tolist()}")
    assert err <= R.ULP_BELOW_8
    assert (merr <= np.spacing(m32)).all(), (mean.tolist(), want_mean)
    g = got.cpu().numpy()
    n_b = [l.shape[1]] * l.shape[0] if lengths is None else lengths
    for b, k in enumerate(n_b):
        assert not g[b, k:].any(), b                          # zeros over [n_b, n), bit for bit
        assert np.array_equal(g[b, :k] > 0, l[b, :k] > 0), b  # unvoiced frames stay unvoiced, voiced ones voiced


@pytest.mark.parametrize("n", NS)
def test_every_operand_given_against_float64(device, n):
    l, lengths, ops = _case(n)
    got, mean = _run(device, l, lengths, **ops)
    _check(got, mean, l, lengths, **ops)
    assert float(mean[1]) == 0.0 and float(mean[2]) == 0.0     # no voiced frame; an empty row
    assert float(mean[3]) == pytest.approx(210.0, rel=1e-6)   # one voiced frame is its own mean
    # out == in: the same bits as out of place
    again, mean2 = _run(device, l, lengths, in_place=True, **ops)
    assert torch.equal(again, got) and torch.equal(mean2, mean)
    # row b of the batch is the call on row b alone, bit for bit
    for b in range(4):
        one, m1 = _run(device, l[b:b + 1], lengths[b:b + 1], **{k: v[b:b + 1] for k, v in ops.items()})
        assert torch.equal(one[0], got[b]) and torch.equal(m1[0], mean[b]), b


@pytest.mark.parametrize("n", NS)
def test_each_operand_alone_and_null_lengths(device, n):
    l, _, ops = _case(n)
    l = np.where(l == 7.0, 0.0, l).astype(np.float32)          # lengths == NULL: every row is read whole
    for name in ops:
        got, mean = _run(device, l, None, **{name: ops[name]})
        _check(got, mean, l, None, **{name: ops[name]})
    got, mean = _run(device, l, None, f_min=100.0, f_max=260.0, **ops)     # the clamp at work
    _check(got, mean, l, None, f_min=100.0, f_max=260.0, **ops)
    hz = R.l_to_hz(got.cpu().numpy()[l > 0])
    assert hz.size == 0 or (hz.min() >= 100.0 * (1 - 1e-6) and hz.max() <= 260.0 * (1 + 1e-6))   # one ulp of l: 5e-7 of f


@pytest.mark.parametrize("n", NS)
def test_identity_rows_are_copied_bit_for_bit(device, n):
    l, lengths, ops = _case(n)
    x = torch.from_numpy(l).to(device)
    # every operand NULL: every row an identity row, over its own length; values outside the clamp are kept
    odd = l.copy()
    odd[0, 0] = R.hz_to_l(30.0)
    odd[3, n // 2] = R.hz_to_l(2500.0)
    for src, lens in ((l, lengths), (odd, lengths), (np.where(l == 7.0, 0.0, l).astype(np.float32), None)):
        got, mean = _run(device, src, lens)
        n_b = [n] * 4 if lens is None else lens
        for b, k in enumerate(n_b):
            assert torch.equal(got[b, :k], torch.from_numpy(src).to(device)[b, :k]) and not got[b, k:].any(), b
        want_mean = R.edit_rows(src, lens)[1].astype(np.float32)
        assert (np.abs(mean.cpu().numpy() - want_mean) <= np.spacing(want_mean)).all()
    # identity rows in a mixed batch: rows 0 and 3 have shift 0, range 1 and no target, rows 1 and 2 are edited
    mixed = dict(shift=np.array([0.0, 2.0, -1.0, 0.0], np.float32), range_=np.array([1.0, 1.0, 0.5, 1.0], np.float32),
                 target_hz=np.array([0.0, 0.0, 140.0, -1.0], np.float32))
    got, mean = _run(device, l, lengths, **mixed)
    _check(got, mean, l, lengths, **mixed)
    for b in (0, 3):
        assert torch.equal(got[b, :lengths[b]], x[b, :lengths[b]]), b
    # offsets of zeros are not the identity rule (include/hsp.h): within one ulp, through the arithmetic
    got, mean = _run(device, l, lengths, offsets=np.zeros_like(l))
    _check(got, mean, l, lengths, offsets=np.zeros_like(l))


def test_pitch_edit_apply_is_the_launch(device):
    from megatts2_hierspeechpp_amd.prosody_controls import PitchEdit
    l, lengths, ops = _case(257)
    x = torch.from_numpy(l).to(device)
    e = PitchEdit(shift=ops["shift"].tolist(), range=torch.from_numpy(ops["range_"]), target_hz=ops["target_hz"].tolist(),
                  offsets=[torch.from_numpy(ops["offsets"][b, :200 + 20 * b]) for b in range(4)])
    off = ops["offsets"].copy()
    for b in range(4):
        off[b, 200 + 20 * b:] = 0.0                            # a short row is continued with zeros
    got, mean = e.apply(x, torch.from_numpy(lengths), return_mean=True)
    _check(got, mean, l, lengths, **dict(ops, offsets=off))
    one = PitchEdit(shift=2.0).apply(x[0, :lengths[0]])        # a 1-D track: one row
    _check(one.reshape(1, -1), torch.zeros(1).fill_(float(mean[0])), l[:1, :lengths[0]], None, shift=[2.0])
    assert torch.equal(PitchEdit().apply(x, torch.from_numpy(lengths))[0, :lengths[0]], x[0, :lengths[0]])


def test_bad_arguments_are_refused_before_any_launch():
    assert einval_cases() == 30
