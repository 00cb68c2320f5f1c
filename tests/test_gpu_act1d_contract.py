"""GPU (-m gpu): hsp_act1d_snakebeta_f32 and hsp_act1d_snakebeta_ragged_f32 called through the C ABI, one launch per
case of tests/act1d_ref.py, against the float64 statement of the header contract on the same operands: every edge of the
wave-per-segment kernel (L = 4, a 4-output tail item, waves that walk from one channel's constants to the next, waves of
fewer than four items and of none), the workgroup-tile kernel with no, one and two interior tiles and on L % 4 == 0 rows
that are 4 bytes off 16-byte alignment, cosine arguments of hundreds of revolutions, and a ragged batch whose rows end on
every side of the segment boundaries with NaN / Inf behind each row's end.

Error bar: helpers.tol_for(reference) (1e-4 x max(1, peak)) for every case.  x and y each live in a buffer with 64
sentinel floats on both sides: everything outside y[B][C][L] must keep its bits and x must be bit-identical after the
call.  The measured error, bar and error / estimate ratios of the library this test was first run on are in
profiles/act1d_contract_ratios.txt.  tests/test_act1d_ref_host.py pins the reference and the claims of the case ids on a
CPU.

What the large-argument cases can and cannot see: a kernel that scaled or rounded the cosine's argument differently
(reduced before scaling, dropped kf's 1 / pi) is wrong by beta_inv, hundreds of bars; a kernel that merely lost the fractf
of hsp_snake_hw passes on an MI355X, whose v_cos_f32 reduces its argument itself (same file, second table).

    python -m pytest tests/test_gpu_act1d_contract.py -q -m gpu -s        (-s shows the measured errors)
"""
import numpy as np
import pytest
import torch

import act1d_ref as R
import helpers as H

pytestmark = pytest.mark.gpu


def _dev(a, device):
    t = torch.from_numpy(np.array(a)).to(device)       # a copy: the case arrays are read-only
    assert t.data_ptr() % 16 == 0
    return t


class _Launch:
    """The device operands of one case and the raw C call on them."""

    def __init__(self, c, device, lens="case"):
        from megatts2_hierspeechpp_amd import _lib as L
        self.L, self.c = L, c
        xb, self.x_off = R.x_buffer(c)
        yb, self.y_off = R.y_buffer(c)
        self.x_before, self.y_before = xb, yb
        self.x, self.y = _dev(xb, device), _dev(yb, device)
        self.ea, self.bi, self.filt = _dev(c["alpha_exp"], device), _dev(c["beta_inv"], device), _dev(c["filt"], device)
        lens = c["lens"] if isinstance(lens, str) else lens
        self.lens = None if lens is None else _dev(np.asarray(lens, np.int64), device)
        self.n = c["x"].size

    def views(self):
        B, C, Lc = self.c["B"], self.c["C"], self.c["L"]
        return (self.x[self.x_off:self.x_off + self.n].view(B, C, Lc), self.y[self.y_off:self.y_off + self.n].view(B, C, Lc))

    def call(self, **over):
        """-> status.  ``over``: arguments replaced for a refusal (x, y, lens as addresses; B, C, L)."""
        L, c = self.L, self.c
        a = dict(x=self.x.data_ptr() + 4 * self.x_off, y=self.y.data_ptr() + 4 * self.y_off, B=c["B"], C=c["C"], L=c["L"],
                 lens=None if self.lens is None else self.lens.data_ptr(), ragged=self.lens is not None)
        a.update(over)
        tail = (self.ea.data_ptr(), self.bi.data_ptr(), self.filt.data_ptr(), L.stream_ptr())
        if a["ragged"]:
            rc = L.lib().hsp_act1d_snakebeta_ragged_f32(a["x"], a["y"], a["B"], a["C"], a["L"], a["lens"], *tail)
        else:
            rc = L.lib().hsp_act1d_snakebeta_f32(a["x"], a["y"], a["B"], a["C"], a["L"], *tail)
        torch.cuda.synchronize()
        return rc

    def y_host(self):
        return self.y.cpu().numpy()

    def check_buffers(self, id, written=True):
        """Everything outside y[B][C][L] keeps its bits (all of y when nothing may be written); x is bit-identical."""
        y, x = self.y_host().view(np.uint32), self.x.cpu().numpy().view(np.uint32)
        assert np.array_equal(x, self.x_before.view(np.uint32)), f"{id}: x was written"
        keep = np.ones(y.size, bool)
        if written:
            keep[self.y_off:self.y_off + self.n] = False
        same = y[keep] == self.y_before.view(np.uint32)[keep]
        assert same.all(), f"{id}: {int((~same).sum())} floats outside y[B][C][L] were written " \
                           f"(first at buffer offset {int(np.flatnonzero(keep)[np.argmin(same)])}, y at {self.y_off})"

    def out(self):
        c = self.c
        return self.y_host()[self.y_off:self.y_off + self.n].reshape(c["B"], c["C"], c["L"])


@pytest.mark.parametrize("id", R.IDS)
def test_act1d_contract(id, device):
    c, ref, est = R.case(id)
    run = _Launch(c, device)
    assert run.call() == 0, id
    run.check_buffers(id)
    got = run.out()
    assert np.isfinite(got).all(), id
    valid = np.ones(got.shape, bool)
    if c["lens"] is not None:
        for b, n in enumerate(R.clip_lens(c["lens"], c["L"])):
            valid[b, :, n:] = False
        tail = got[~valid]
        assert not tail.any() and not np.signbit(tail).any(), f"{id}: the zeros from lens[b] on are not exact +0.0"
    d = np.abs(got.astype(np.float64) - ref)
    err, tol = float(d.max()), H.tol_for(ref)
    ratio = float((d[valid] / est[valid]).max())
    print(f"act1d_contract {R.kernel_of(c)} {id}: max|hip - float64| = {err:.3e} (bar {tol:.1e}, ratio {err / tol:.3f}); "
          f"max error / estimate = {ratio:.3f}")
    assert err <= tol, f"{id}: max|hip - ref| = {err:.3e} > {tol:.1e}"


@pytest.mark.parametrize("id", [i for i in R.PLAIN_IDS if i.startswith("seg_")])
def test_ragged_with_full_lengths_is_the_plain_call(id, device):
    """(a) hsp_act1d_snakebeta_ragged_f32 with every lens[b] = L: the bits of hsp_act1d_snakebeta_f32."""
    c, _, _ = R.case(id)
    plain, ragged = _Launch(c, device), _Launch(c, device, lens=[c["L"]] * c["B"])
    assert plain.call() == 0 and ragged.call() == 0
    ragged.check_buffers(id)
    assert np.array_equal(plain.y_host().view(np.uint32), ragged.y_host().view(np.uint32)), id


def test_batched_rows_are_the_solo_calls(device):
    """(b) wave-per-segment kernel: row (b, c) of a batched call has the bits of the B = C = 1 call on that row with that
    channel's constants, wherever the row's items fall in their waves."""
    c, _, _ = R.case(R.BATCH_ROWS_ID)
    run = _Launch(c, device)
    assert run.call() == 0
    got = run.out()
    for b in range(c["B"]):
        for ch in range(c["C"]):
            solo = dict(c, B=1, C=1, x=c["x"][b:b + 1, ch:ch + 1], alpha_exp=c["alpha_exp"][ch:ch + 1],
                        beta_inv=c["beta_inv"][ch:ch + 1])
            assert R.kernel_of(solo) == "seg"
            one = _Launch(solo, device)
            assert one.call() == 0
            assert np.array_equal(one.out()[0, 0].view(np.uint32), got[b, ch].view(np.uint32)), (b, ch)


@pytest.mark.parametrize("id", ["seg_L1988_30_items", "tile_L2051_first_interior", "ragged_L1488_18_rows"])
def test_functional_act1d_is_the_raw_call(id, device):
    """(c) functional.act1d, with and without lens, writes what the raw call writes on the same operands."""
    from megatts2_hierspeechpp_amd import functional as Fh
    c, _, _ = R.case(id)
    raw, wrapped = _Launch(c, device), _Launch(c, device)
    assert raw.call() == 0
    xv, yv = wrapped.views()
    assert xv.is_contiguous() and yv.is_contiguous()
    out = Fh.act1d(xv, wrapped.ea, wrapped.bi, wrapped.filt, out=yv, lens=wrapped.lens)
    torch.cuda.synchronize()
    assert out.data_ptr() == yv.data_ptr()
    assert torch.equal(raw.y.view(torch.int32), wrapped.y.view(torch.int32)), id
    assert torch.equal(raw.x.view(torch.int32), wrapped.x.view(torch.int32)), id


def test_refused_calls_write_nothing(device):
    """HSP_EINVAL and an untouched y: the ragged form on rows that are not 16-byte addressable or without lens, and both
    forms with an empty size or a NULL operand."""
    from megatts2_hierspeechpp_amd import _lib as L
    c, _, _ = R.case("ragged_L1488_18_rows")
    run = _Launch(c, device)
    x, y = run.x.data_ptr() + 4 * run.x_off, run.y.data_ptr() + 4 * run.y_off
    refusals = [dict(lens=None), dict(L=c["L"] - 1), dict(L=c["L"] - 2), dict(x=x + 4), dict(y=y + 4), dict(y=y + 8),
                dict(x=x + 12, y=y + 12), dict(B=0), dict(C=-1), dict(L=0), dict(x=None), dict(y=None)]
    for over in refusals:
        assert run.call(**over) == L.EINVAL, over
    for over in (dict(B=0), dict(C=0), dict(L=-4), dict(x=None), dict(y=None)):
        assert run.call(ragged=False, **over) == L.EINVAL, over
    run.check_buffers("refusals", written=False)
