"""CPU: the float64 restatement of tests/cprod3_ref.py against numpy's complex matrix product, what the case table of
that file reaches -- the five roles a consumer wave of csrc/hsp_cprod3.hip can take, both block orders, chunk and row-tile
counts, the plane strides -- and the argument refusals of hsp_cprod3_f32, which need no device (made-up addresses: every
refusal comes before a launch).

    python -m pytest tests/test_cprod3_ref_host.py -q
"""
import ctypes

import numpy as np
import pytest

import cprod3_ref as R
import helpers as H


def test_three_products_are_the_complex_product():
    """With the matrices (a + b, a, b) of a complex W = a + i b the statement is Y = W X."""
    r = np.random.default_rng(1)
    bins, C, Np = 3, 8, 12
    a, b = r.standard_normal((2, bins, C, C))
    xr, xi = r.standard_normal((2, bins, C, Np))
    y = R.product(xr, xi, np.stack([a + b, a, b], axis=1))
    want = (a + 1j * b) @ (xr + 1j * xi)
    assert np.abs(y[:, :C] - want.real).max() <= 1e-12 and np.abs(y[:, C:] - want.imag).max() <= 1e-12


def test_operands_are_read_through_the_strides_and_the_transposed_weights():
    a, ref, bound = R.case("bins9_C64_Np132_strided")
    bins, C, Np = a["bins"], a["C"], a["Np"]
    assert ref.shape == bound.shape == (bins, 2 * C, Np) and np.isfinite(ref).all() and (bound > 0).all()
    w = a["w"].reshape(bins, 3, C, C).astype(np.float64)                 # [bin][matrix][input channel][output row]
    j, m, n = 7, 5, 131
    p = a["xf_off"] + j * a["xf_bs"]
    xr = a["xf"][p + np.arange(C) * Np + n].astype(np.float64)
    xi = a["xf"][p + (C + np.arange(C)) * Np + n].astype(np.float64)
    k1, k2, k3 = w[j, 0, :, m] @ xr, w[j, 1, :, m] @ (xi - xr), w[j, 2, :, m] @ (xr + xi)
    assert abs(ref[j, m, n] - (k1 - k3)) <= 1e-12 and abs(ref[j, C + m, n] - (k1 + k2)) <= 1e-12
    # the bound is far below the bar and far above the rounding of the float64 reference
    assert float(bound.max()) < H.tol_for(ref) and float(bound.min()) > 1e-9


def test_table_reaches_every_wave_role():
    want = {4: {"one_masked", "barrier_only"}, 96: {"two_full", "one_full"},
            132: {"two_full", "one_masked", "barrier_only"}, 160: {"two_full", "one_full", "barrier_only"},
            164: {"two_full", "two_masked", "barrier_only"}, 196: {"two_full", "one_masked"},
            224: {"two_full", "one_full"}, 256: {"two_full"}}
    assert {s["Np"] for s in R.SPECS} == set(want)
    for Np, rs in want.items():
        assert set(R.roles(Np).values()) == rs, Np
    assert set().union(*want.values()) == set(R.ROLES)
    # the roles the issue names: a live one-block consumer beside a barrier-only wave in ONE tile (Np = 4, the last tile of
    # 132 and 160), the production tail 224 = 128 + 96 as two full + one full, 32 < left < 64
    assert R.roles(4) == {(0, 0): "one_masked", (0, 1): "barrier_only"}
    assert R.roles(132)[(1, 0)] == "one_masked" and R.roles(132)[(1, 1)] == "barrier_only"
    assert R.roles(160)[(1, 0)] == "one_full" and R.roles(224)[(1, 1)] == "one_full" and R.roles(224)[(1, 0)] == "two_full"
    assert R.roles(164)[(1, 0)] == "two_masked" and 32 < 164 - 128 < 64
    # the shapes of the older parity test (test_cprod3_entry_point_vs_numpy) reach every role but the full one-block
    # consumer: Np = 100 and 36 leave 36 columns to a two-block wave
    old = set().union(*(set(R.roles(Np).values()) for Np in (4, 132, 256, 100, 36)))
    assert old == set(R.ROLES) - {"one_full"}


def test_table_reaches_both_block_orders_and_the_tile_counts():
    assert {s["bins"] for s in R.SPECS} == {1, 8, 9, 16} and {s["C"] for s in R.SPECS} == {64, 128, 320}
    assert {R.block_order(s["bins"]) for s in R.SPECS} == {"xcd", "plain"}
    assert sorted({s["C"] // R.KC for s in R.SPECS}) == [4, 8, 20] and sorted({s["C"] // R.BM for s in R.SPECS}) == [1, 2, 5]
    assert len(R.SPECS) == 12
    for s in R.SPECS:       # either order visits every (row tile, column tile, bin) once
        tiles = R.block_tiles(s["bins"], s["C"], s["Np"])
        n = s["bins"] * (s["C"] // R.BM) * -(-s["Np"] // R.BN)
        assert len(tiles) == n == len(set(tiles)), s["id"]
    o = R.spec_of(R.ORDER_ID)
    assert R.block_order(o["bins"]) == "xcd" and R.block_order(1) == "plain"
    tiles = R.block_tiles(o["bins"], o["C"], o["Np"])
    assert [t[2] for t in tiles[:8]] == list(range(8)) and len({t[:2] for t in tiles[:8]}) == 1     # eight bins of one tile


def test_strides_and_buffers():
    strided = [R.case(s["id"])[0] for s in R.SPECS if s["strided"]]
    assert len(strided) >= 3
    for a in strided:
        plane = 2 * a["C"] * a["Np"]
        assert a["xf_bs"] == plane + 4 and a["yf_bs"] == plane + 64 and a["xf_bs"] != a["yf_bs"]
    for id in R.IDS:
        a, _, _ = R.case(id)
        plane = 2 * a["C"] * a["Np"]
        data = np.zeros(a["xf"].size, bool)
        for j in range(a["bins"]):
            data[a["xf_off"] + j * a["xf_bs"]:a["xf_off"] + j * a["xf_bs"] + plane] = True
        assert np.isfinite(a["xf"][data]).all() and np.isnan(a["xf"][~data]).all()
        assert a["xf_off"] >= 64 and a["yf_off"] >= 64 and (~data[-64:]).all()
        assert (a["yf"] == R.SENT).all() and a["yf"].size == 2 * R.GUARD + a["bins"] * a["yf_bs"]
        assert int(R.written(a).sum()) == a["bins"] * plane
        assert a["xf_off"] % 4 == 0 and a["xf_bs"] % 4 == 0 and a["yf_bs"] % 4 == 0


def test_entry_point_refuses_bad_arguments():
    from megatts2_hierspeechpp_amd import _lib as L
    lib, base = L.lib(), R.fake_base()
    a, _, _ = R.case("bins8_C128_Np164_strided")
    plane = 2 * a["C"] * a["Np"]

    def refused(s):
        return lib.hsp_cprod3_supported(ctypes.byref(s)) == 0 and lib.hsp_cprod3_f32(ctypes.byref(s), None) == L.EINVAL

    assert lib.hsp_cprod3_supported(ctypes.byref(R.to_struct(a, base))) == 1
    assert lib.hsp_cprod3_supported(ctypes.byref(R.to_struct(a, base, bin0=3, bins=1))) == 1
    for field, bad in (("xf", None), ("yf", None), ("w", None), ("zeros", None), ("bins", 0), ("bins", -8), ("C", 0),
                       ("C", 96), ("C", 160), ("Np", 0), ("Np", 162), ("Np", 165), ("debug", 1), ("debug", 16384),
                       ("xf_bs", plane - 4), ("yf_bs", plane - 4), ("xf_bs", plane + 2), ("yf_bs", plane + 6)):
        s = R.to_struct(a, base)
        setattr(s, field, bad)
        assert refused(s), (field, bad)
    for field in ("xf", "w"):                                       # 16-byte alignment of the DMA sources
        for off in (4, 8):
            s = R.to_struct(a, base)
            setattr(s, field, getattr(s, field) + off)
            assert refused(s), (field, off)
    assert lib.hsp_cprod3_f32(None, None) == L.EINVAL and lib.hsp_cprod3_supported(None) == 0
