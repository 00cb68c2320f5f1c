"""GPU (-m gpu): hsp_cprod3_f32 called through the C ABI with hand-filled hsp_cprod3_args, one launch per case of
tests/cprod3_ref.py, against the float64 statement of the header's three products on the same operands: every role a
consumer wave can take (two blocks full / masked, one block full / masked, barrier only), both block orders, one to five
row tiles, four to twenty chunks, plane strides above 2 C Np that differ between xf and yf.

Error bars: helpers.tol_for(reference) for the launch and, element by element, the derived linear bound
2 (C + 8) 2^-24 (|A1| |Xr| + (|A2| + |A3|) (|Xr| + |Xi|)).  The slack of xf between planes and its guard bands hold NaN
(nothing there may be read: the output must be finite); the slack of yf and its guard bands hold a sentinel that must
keep its bits.  The measured errors, bars and error / bound ratios of the library this test was first run on are in
profiles/cprod3_contract_ratios.txt.  tests/test_cprod3_ref_host.py pins the reference and the roles of the table on a
CPU.

    python -m pytest tests/test_gpu_cprod3_contract.py -q -m gpu -s        (-s shows the measured errors)
"""
import ctypes

import numpy as np
import pytest
import torch

import cprod3_ref as R
import helpers as H

pytestmark = pytest.mark.gpu


def _dev(a, device):
    t = torch.from_numpy(np.array(a)).to(device)       # a copy: the case arrays are read-only
    assert t.data_ptr() % 16 == 0
    return t


def _operands(a, device):
    dev = dict(xf=_dev(a["xf"], device), yf=_dev(a["yf"], device), w=_dev(a["w"], device),
               zeros=torch.zeros(64, dtype=torch.float32, device=device))
    return dev, {k: v.data_ptr() for k, v in dev.items()}


def _launch(a, base, **sub):
    from megatts2_hierspeechpp_amd import _lib as L
    s = R.to_struct(a, base, **sub)
    assert L.lib().hsp_cprod3_supported(ctypes.byref(s)) == 1
    L.check(L.lib().hsp_cprod3_f32(ctypes.byref(s), L.stream_ptr()), "hsp_cprod3_f32")


def _check_untouched(id, a, got):
    keep = ~R.written(a)
    same = got.view(np.uint32)[keep] == a["yf"].view(np.uint32)[keep]
    assert same.all(), f"{id}: {int((~same).sum())} floats outside the planes' 2 C Np were written " \
                       f"(first at buffer offset {int(np.flatnonzero(keep)[np.argmin(same)])}, yf at {a['yf_off']})"


@pytest.mark.parametrize("id", R.IDS)
def test_cprod3_contract(id, device):
    a, ref, bound = R.case(id)
    dev, base = _operands(a, device)
    _launch(a, base)
    torch.cuda.synchronize()
    got = dev["yf"].cpu().numpy()
    assert np.array_equal(dev["xf"].cpu().numpy().view(np.uint32), a["xf"].view(np.uint32)), f"{id}: xf was written"
    _check_untouched(id, a, got)
    y = R.planes(got, a["yf_off"], a["yf_bs"], a["bins"], a["C"], a["Np"]).astype(np.float64)
    assert np.isfinite(y).all(), id
    d = np.abs(y - ref)
    err, tol, ratio = float(d.max()), H.tol_for(ref), float((d / bound).max())
    print(f"cprod3_contract {R.block_order(a['bins'])} {id}: max|hip - float64| = {err:.3e} (bar {tol:.1e}, "
          f"ratio {err / tol:.3f}); max error / derived bound = {ratio:.3f}")
    assert err <= tol, f"{id}: max|hip - ref| = {err:.3e} > {tol:.1e}"
    assert ratio <= 1.0, f"{id}: an element is {ratio:.2f} x its derived bound"


def test_both_block_orders_give_the_same_bits(device):
    """The planes of a bins = 8 launch (every tile of a bin on one XCD) against eight bins = 1 launches (the plain
    order) on the same per-bin operands."""
    a, _, _ = R.case(R.ORDER_ID)
    assert R.block_order(a["bins"]) == "xcd" and R.block_order(1) == "plain"
    dev, base = _operands(a, device)
    _launch(a, base)
    torch.cuda.synchronize()
    whole = dev["yf"].cpu().numpy()
    dev1, base1 = _operands(a, device)
    for j in range(a["bins"]):
        _launch(a, base1, bin0=j, bins=1)
    torch.cuda.synchronize()
    single = dev1["yf"].cpu().numpy()
    _check_untouched(R.ORDER_ID, a, single)
    assert np.array_equal(whole.view(np.uint32), single.view(np.uint32))
