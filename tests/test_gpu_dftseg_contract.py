"""GPU (-m gpu): hsp_dftseg_fwd_f32, hsp_dftseg_inv_f32 and hsp_dftseg_pair_f32 called through the C ABI with hand-filled
hsp_dftseg_args, one entry point and one launch per case of tests/dftseg_ref.py, against the float64 statement of the
header contract on the same operands -- every staging path of the forward kernel, both scatters and both epilogue forms
of the inverse, chunked rows, one or two operand buffers, the pair of every AMP block, and one case per kernel in which
every workgroup walks three items or more.

Error bar: helpers.tol_for(reference) (1e-4 x max(1, peak)) for every case, BAR_FACTOR = 1 for both families (the plain
transforms and the ones through the fused activation): the library this test was first run on stayed below half of it
everywhere (profiles/dftseg_contract_ratios.txt).  Every output lives in a sentinel-filled buffer: guard bands, stride
slack, y outside [0, L) of a row, the padding columns [B d nseg, Np) of the spectrum and each bin plane beyond 2 C Np
must keep their bits.  tests/test_dftseg_ref_host.py pins the reference and the claims of the case ids on a CPU.

    python -m pytest tests/test_gpu_dftseg_contract.py -q -m gpu -s        (-s shows the measured errors)
"""
import ctypes

import numpy as np
import pytest
import torch

import dftseg_ref as R
import helpers as H

pytestmark = pytest.mark.gpu

BAR_FACTOR = dict(plain=1, act=1)          # power-of-two multiples of tol_for per family, fixed on the parent's library


def _check_untouched(id, a, name, got, written):
    before = np.asarray(a[name], np.float32)
    same = got.view(np.uint32)[~written] == before.view(np.uint32)[~written]
    assert same.all(), f"{id}: {int((~same).sum())} elements outside the contract's output were written " \
                       f"(first at buffer offset {int(np.flatnonzero(~written)[np.argmin(same)])}, {name} at {a[name + '_off']})"


@pytest.mark.parametrize("id", R.IDS)
def test_dftseg_contract(id, device):
    spec = R.spec_of(id)
    if "persistent" in id:
        cus = torch.cuda.get_device_properties(device).multi_processor_count
        _, items, res = R.launch_shape(spec, cus)
        if items <= 2 * res:
            pytest.skip(f"{id}: {items} items on {res} resident workgroups ({cus} CUs) -- no workgroup walks three items")
    ai, af, ref, written = R.case(id)
    got = R.run_case(ai, af, device)
    a, name = R.output_of(ai, af)
    _check_untouched(id, a, name, got, written)
    g, r = got.astype(np.float64)[written], ref[written]
    assert np.isfinite(g).all(), id
    family = "act" if id in R.ACT_FAMILY else "plain"
    err, tol = float(np.abs(g - r).max()), BAR_FACTOR[family] * H.tol_for(r)
    print(f"dftseg_contract {spec['kind']} {family} {id}: max|hip - float64| = {err:.3e} (bar {tol:.1e}, ratio {err / tol:.3f})")
    assert err <= tol, f"{id}: max|hip - ref| = {err:.3e} > {tol:.1e}"


@pytest.mark.parametrize("id", [s["id"] for s in R.SPECS if s["kind"] != "inv" and "persistent" not in s["id"]])
def test_slot0_is_all_prod3_changes(id, device):
    """The prod3 = 0 and prod3 = 1 spectra of one input are bit-identical outside slot 0 of every column."""
    spec = R.spec_of(id)
    outs = []
    for p3 in (0, 1):
        ai, af = R.build(dict(spec, prod3=p3))
        outs.append(R.run_case(ai, af, device).view(np.uint32))
    lo, hi = af["xf_off"], af["xf_off"] + af["xf_bs"]            # bin plane 0
    assert np.array_equal(outs[0][:lo], outs[1][:lo]) and np.array_equal(outs[0][hi:], outs[1][hi:]), id
    assert not np.array_equal(outs[0][lo:hi], outs[1][lo:hi]), id


@pytest.mark.parametrize("id", [s["id"] for s in R.SPECS if s.get("act_len") and "chunked" not in s["id"]])
def test_full_length_row_is_the_plain_activation(id, device):
    """A row whose act_len equals L is bit-identical to the same launch without act_len."""
    spec = R.spec_of(id)
    ai, af = R.build(spec)
    ragged = R.run_case(ai, af, device).view(np.uint32)
    ai, af = R.build(dict(spec, act_len=None))
    plain = R.run_case(ai, af, device).view(np.uint32)
    nseg, d, C, Np = af["nseg"], af["dil"], af["C"], af["Np"]
    cols = np.zeros(Np, bool)
    for b, n in enumerate(spec["act_len"]):
        if n == af["L"]:
            cols[b * d * nseg:(b + 1) * d * nseg] = True
    assert cols.any()
    view = lambda o: np.stack([o[af["xf_off"] + j * af["xf_bs"]:][:2 * C * Np].reshape(2 * C, Np) for j in range(64)])
    assert np.array_equal(view(ragged)[:, :, cols], view(plain)[:, :, cols]), id
    assert not np.array_equal(view(ragged)[:, :, ~cols], view(plain)[:, :, ~cols]), id


def test_refusals():
    """What the entry points refuse before anything reaches the device (the rest: tests/test_host_logic.py)."""
    from megatts2_hierspeechpp_amd import _lib as L
    lib, base = L.lib(), R.fake_base()
    spec = R.spec_of("fwd_act_ragged_k7_d5_L720")
    _, af = R.build(spec)
    s = R.to_struct(af, base)
    s.act_alpha_exp = s.act_beta_inv = s.act_filt = None         # act_len without act_*
    assert lib.hsp_dftseg_fwd_f32(ctypes.byref(s), None) == L.EINVAL
    _, shifted = R.build(dict(spec, act_len=None, x_shift=1))    # act_* on rows that are not 16-B addressable
    assert lib.hsp_dftseg_fwd_f32(ctypes.byref(R.to_struct(shifted, base)), None) == L.EINVAL
    _, odd = R.build(dict(spec, act_len=None, L=718))
    assert lib.hsp_dftseg_fwd_f32(ctypes.byref(R.to_struct(odd, base)), None) == L.EINVAL
    ai, af = R.build(R.spec_of("pair_k7_d1_L800"))
    for field in ("y", "res"):                                   # the pair writes no tensor between its transforms
        si, sf = R.to_struct(ai, base), R.to_struct(af, base)
        assert lib.hsp_dftseg_pair_supported(ctypes.byref(si), ctypes.byref(sf)) == 1
        setattr(si, field, 0x5000000)
        assert lib.hsp_dftseg_pair_supported(ctypes.byref(si), ctypes.byref(sf)) == 0
        assert lib.hsp_dftseg_pair_f32(ctypes.byref(si), ctypes.byref(sf), None) == L.EINVAL
