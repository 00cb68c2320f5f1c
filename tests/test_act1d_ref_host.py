"""CPU: the ragged restatement of tests/act1d_ref.py against conv_ref.act1d on cut rows, every claim a case id of that
table makes -- which kernel of csrc/hsp_pointwise.hip the case reaches, which 1024-sample tiles take the paired interior
branch, empty and short waves, waves that walk across a channel or a batch row, the share of samples whose cosine
argument passes 256 revolutions, estimate <= half the bar -- and the argument refusals of the two entry points, none of
which needs a device (made-up addresses: every refusal comes before a launch).

    python -m pytest tests/test_act1d_ref_host.py -q
"""
import numpy as np
import pytest

import act1d_ref as R
import helpers as H

P, Q = 0x100000, 0x200000          # made-up 16-byte aligned addresses


def test_ragged_restatement_is_act1d_of_the_cut_rows():
    c, ref, _ = R.case("ragged_L1488_18_rows")
    n = R.clip_lens(c["lens"], c["L"])
    assert n.tolist() == [1, 1, 1, 2, 3, 4, 5, 493, 494, 495, 496, 497, 498, 499, 992, 1487, 1488, 1488]
    assert np.isfinite(ref).all()
    for b, nb in enumerate(n):
        cut = np.ascontiguousarray(c["x"][b:b + 1, :, :nb])
        assert np.isfinite(cut).all() and not np.isfinite(c["x"][b, :, nb:]).any()
        assert np.array_equal(ref[b, :, :nb], R.act1d(cut, c["alpha_exp"], c["beta_inv"], c["filt"])[0])
        assert not ref[b, :, nb:].any() and not np.signbit(ref[b, :, nb:]).any()
        t = np.arange(nb, c["L"])
        assert np.isnan(c["x"][b, :, t[t % 2 == 1]]).all() and np.isposinf(c["x"][b, :, t[t % 2 == 0]]).all()
    # a one-sample row is the activation of a constant: up = x, y = x + beta_inv sin(x alpha_exp)^2 (taps sum to 1)
    x0 = c["x"][0, :, 0].astype(np.float64)
    want = x0 + c["beta_inv"].astype(np.float64) * np.sin(x0 * c["alpha_exp"].astype(np.float64)) ** 2
    assert np.abs(ref[0, :, 0] - want).max() <= 1e-6
    # rows whose end lies 2 and 1 samples before the start of segment 1: slot e = 0 and e = 2 of that item
    assert [2 * (int(v) - R.SEG) + 4 for v in (494, 495)] == [0, 2] and {494, 495} <= set(n.tolist())
    assert R.kernel_of(c) == "seg" and c["L"] % R.SEG == 0


def test_constants_are_distinct_per_channel_and_in_range():
    for id in R.IDS:
        c, _, _ = R.case(id)
        ea, bi = c["alpha_exp"], c["beta_inv"]
        assert len(np.unique(ea)) == c["C"] and len(np.unique(bi)) == c["C"], id
        rest = slice(1, None) if c["big"] else slice(None)
        assert (ea[rest] >= 0.5).all() and (ea[rest] <= 4.0).all() and (bi[rest] >= 0.3).all() and (bi[rest] <= 1.5).all()
        assert c["filt"].shape == (24,) and abs(float(c["filt"][:12].sum()) - 1.0) < 1e-6


@pytest.mark.parametrize("id", R.IDS)
def test_case_reaches_the_kernel_its_id_names(id):
    c, _, _ = R.case(id)
    assert R.kernel_of(c) == ("tile" if id.startswith("tile_") else "seg"), id
    if id.startswith("tile_"):
        assert 1 <= c["B"] * c["C"] <= 3
    if "off1" in id:           # L % 4 == 0: only the view's offset keeps the call off the wave-per-segment kernel
        assert c["L"] % 4 == 0 and (c["x_shift"], c["y_shift"]) in ((1, 0), (0, 1))
        assert R.kernel_of(dict(c, x_shift=0, y_shift=0)) == "seg"
    else:
        assert c["x_shift"] == c["y_shift"] == 0


def test_interior_tiles():
    br = R.tile_branches
    assert br(2050) == [False, False, False]                    # the second tile misses the branch by one slot
    assert br(2051) == [False, True, False]                     # the first length with an interior tile
    assert br(3077) == [False, True, True, False]
    assert br(2052) == [False, True, False]                     # the two misaligned cases take it as well
    assert not any(any(br(L)) for L in range(1, 2051))
    for L in (1, 2, 3, 5, 37, 1023, 1025):
        assert not any(br(L))
    tiles = {s["L"] for s in R.SPECS if s["id"].startswith("tile_")}
    assert tiles == {1, 2, 3, 5, 37, 1023, 1025, 2050, 2051, 2052, 3077}


def test_seg_work_split():
    it = lambda id: R.seg_items(*(R.spec_of(id)[k] for k in "BCL"))
    a = it("seg_L4_both_pads_in_one_item")
    assert a["nwork"] == 1 and a["items"] == [1, 0, 0, 0] and a["tail4"]          # head and tail pad in the one item
    a = it("seg_L8_two_channels_one_wave")
    assert a["items"] == [2, 0, 0, 0] and a["cross_channel"][0] and not a["cross_row"][0]
    a = it("seg_L496_c5_two_empty_waves")
    assert a["items"] == [4, 1, 0, 0] and a["empty"] == [2, 3] and a["cross_channel"][0]
    a = it("seg_L500_tail4")
    assert a["nseg"] == 2 and a["tail4"] and a["items"] == [4, 4, 4, 0] and any(a["cross_row"])
    a = it("seg_L992_short_wave")
    assert a["items"] == [4, 2, 0, 0] and not a["tail4"]
    a = it(R.BATCH_ROWS_ID)
    assert a["nwork"] == 30 and a["nseg"] == 5 and a["tail4"] and a["blocks"] == 2
    assert a["items"] == [4] * 7 + [2] and any(a["cross_channel"]) and any(a["cross_row"])
    a = it("ragged_L1488_18_rows")
    assert a["nseg"] == 3 and a["nwork"] == 108 and min(a["items"][:27]) == 4 and any(a["cross_row"])
    # every wave size below ACT2_ITEMS is in the table
    sizes = {n for s in R.SPECS if R.kernel_of(R.case(s["id"])[0]) == "seg" for n in it(s["id"])["items"]}
    assert sizes == {0, 1, 2, 4}


@pytest.mark.parametrize("id", [s["id"] for s in R.SPECS if s["big"]])
def test_large_argument_channel(id):
    c, ref, est = R.case(id)
    rev = R.revolutions(c["x"], c["alpha_exp"], c["filt"])
    share = float((rev[:, 0] > R.REV_LIMIT).mean())
    print(f"{id}: {100 * share:.1f} % of channel 0 above {R.REV_LIMIT:.0f} revolutions, peak {rev[:, 0].max():.0f}; "
          f"estimate {est.max():.2e} against a bar of {H.tol_for(ref):.2e}")
    assert 0.01 <= share < 1.0
    assert float(rev[:, 1:].max()) < 32.0                        # the other channels stay at a few revolutions
    assert float(c["beta_inv"][0]) >= 0.05                      # sin^2 amplitude: a lost reduction is ~1e3 bars off
    assert float(c["beta_inv"][0]) >= 100 * H.tol_for(ref)


@pytest.mark.parametrize("id", R.IDS)
def test_estimate_is_at_most_half_the_bar(id):
    c, ref, est = R.case(id)
    assert np.isfinite(ref).all() and np.isfinite(est).all() and est.shape == ref.shape
    n = R.clip_lens(c["lens"], c["L"]) if c["lens"] is not None else [c["L"]] * c["B"]
    for b, nb in enumerate(n):
        assert (est[b, :, :nb] > 0).all()
    assert float(est.max()) <= 0.5 * H.tol_for(ref), (id, float(est.max()), H.tol_for(ref))
    if not c["big"] and c["lens"] is None:
        assert float(R.revolutions(c["x"], c["alpha_exp"], c["filt"]).max()) < 32.0


def test_buffers_carry_64_sentinels_on_both_sides():
    for id in R.IDS:
        c, _, _ = R.case(id)
        for (buf, off), shift in ((R.x_buffer(c), c["x_shift"]), (R.y_buffer(c), c["y_shift"])):
            n = c["x"].size
            assert off == R.GUARD + shift and off >= 64 and buf.size - off - n >= 64
            assert (buf[:off] == R.SENT).all() and (buf[off + n:] == R.SENT).all()


# ------------------------------------------------------------------------------------------------ refusals
@pytest.fixture(scope="module")
def lib():
    from megatts2_hierspeechpp_amd import _lib
    return _lib


def _with(args, at, value):
    a = list(args)
    a[at] = value
    return a


PLAIN = [P, Q, 2, 3, 8, P, P, P, None]                # x, y, B, C, L, alpha_exp, beta_inv, filt, stream
RAGGED = [P, Q, 2, 3, 8, P, P, P, P, None]            # x, y, B, C, L, lens, alpha_exp, beta_inv, filt, stream


def test_entry_points_refuse_null_pointers_and_empty_sizes(lib):
    for name, args, ptrs in (("hsp_act1d_snakebeta_f32", PLAIN, (0, 1, 5, 6, 7)),
                             ("hsp_act1d_snakebeta_ragged_f32", RAGGED, (0, 1, 5, 6, 7, 8))):
        fn = getattr(lib.lib(), name)
        assert len(args) == len(lib.SIGNATURES[name][1])
        for at in ptrs:
            assert fn(*_with(args, at, None)) == lib.EINVAL, (name, "NULL at", at)
        for at in (2, 3, 4):
            for bad in (0, -1, -4):
                assert fn(*_with(args, at, bad)) == lib.EINVAL, (name, bad, "at", at)


def test_ragged_entry_point_refuses_rows_that_are_not_16_byte_addressable(lib):
    fn = lib.lib().hsp_act1d_snakebeta_ragged_f32
    for L in (5, 6, 7, 2051):
        assert fn(*_with(RAGGED, 4, L)) == lib.EINVAL, L
    for off in (4, 8, 12):
        assert fn(*_with(RAGGED, 0, P + off)) == lib.EINVAL, ("x", off)
        assert fn(*_with(RAGGED, 1, Q + off)) == lib.EINVAL, ("y", off)
    for L, xo, yo in ((5, 0, 0), (8, 4, 0), (8, 0, 12)):
        assert not R.seg_rows(L, xo, yo)
    assert R.seg_rows(8, 0, 16)
