"""CPU: pins tests/dftseg_ref.py, the float64 statement of the hsp_dftseg_args contract that tests/test_gpu_dftseg_contract.py
holds the three transform entry points to -- the reference against torch's float64 conv1d, the two slot-0 forms against
one another, and the claims of the case ids (staging path, chunking, operand buffers, persistent loop) against the
restated host geometry.  The library is asked only for its predicates."""
import ctypes

import numpy as np
import pytest
import torch

import dftseg_ref as R


GEOMS = sorted({(s["k"], s["d"], s["L"]) for s in R.SPECS})


@pytest.mark.parametrize("k,d,L", GEOMS)
def test_inverse_of_product_of_forward_is_conv1d(k, d, L):
    """inv_contract(conj(rfft(w, 128)) fwd_contract(x)) = the same-length dilated conv1d of torch in float64."""
    spec = dict(id="g", kind="fwd", B=2, C=3, L=L, k=k, d=d, seed=k * 1000 + d)
    _, af = R.build(spec)
    xf, _ = R.fwd_contract(af)
    w = np.random.default_rng(k + d).standard_normal((3, 3, k))
    corr = R.correlation_of(af, R.product(xf[R._spec_idx(af)], w))
    x = torch.from_numpy(R.rows(af, "x")[0])
    want = torch.nn.functional.conv1d(x, torch.from_numpy(w), padding=af["pad"], dilation=d).numpy()
    assert np.abs(corr - want).max() <= 1e-11 * max(1.0, np.abs(want).max())


def test_inverse_epilogue_order():
    """y = ((corr + bias + res) + y) * post_scale, on [0, L) of every row and nowhere else."""
    a, _ = R.build(dict(id="e", kind="inv", B=2, C=3, L=50, k=7, d=3, seed=1, bias=True, res=True, acc=True, ps=1 / 3))
    out, wr = R.inv_contract(a)
    corr = R.correlation_of(a, a["xf"].astype(np.float64)[R._spec_idx(a)])
    y0, idx = R.rows(a, "y")
    full = ((corr + a["bias"][None, :3, None].astype(np.float64) + R.rows(a, "res")[0]) + y0) * float(np.float32(1 / 3))
    assert np.array_equal(out[idx], full)
    assert wr.sum() == idx.size and (out[~wr] == R.SENT).all()


@pytest.mark.parametrize("id", [s["id"] for s in R.SPECS if s["kind"] == "fwd" and s["C"] <= 48])
def test_slot0_forms_agree(id):
    """prod3 = 1 puts (-E0, -O0) where prod3 = 0 has (DC, Nyquist) = (E0 + O0, E0 - O0); everything else is the same."""
    spec = R.spec_of(id)
    _, a0 = R.build(dict(spec, prod3=0))
    _, a1 = R.build(dict(spec, prod3=1))
    x0, w0 = R.fwd_contract(a0)
    x1, w1 = R.fwd_contract(a1)
    assert np.array_equal(w0, w1)
    d0, d1 = x0[R._spec_idx(a0)], x1[R._spec_idx(a1)]
    assert np.array_equal(d0[1:], d1[1:])
    C = a0["C"]
    E0, O0 = -d1[0, :C], -d1[0, C:]
    tol = 1e-12 * np.abs(d0[0]).max()
    assert np.abs(d0[0, :C] - (E0 + O0)).max() <= tol and np.abs(d0[0, C:] - (E0 - O0)).max() <= tol


def test_padding_columns_and_plane_slack_are_not_written():
    _, af, ref, written = R.case("fwd_vec_k11_d1_L472_ongrid")
    n, Np, C = af["B"] * af["dil"] * af["nseg"], af["Np"], af["C"]
    assert Np > n and af["xf_bs"] > 2 * C * Np
    assert written.sum() == 64 * 2 * C * n
    assert (ref[~written] == R.SENT).all()


def _struct(a):
    return R.to_struct(a, R.fake_base())


@pytest.mark.parametrize("id", R.IDS)
def test_library_accepts_every_case(id):
    from megatts2_hierspeechpp_amd import _lib as L
    ai, af, _, _ = R.case(id)
    for a in (ai, af):
        if a is not None:
            assert L.lib().hsp_dftseg_supported(ctypes.byref(_struct(a))) == 1, id
    if ai is not None and af is not None:
        assert L.lib().hsp_dftseg_pair_supported(ctypes.byref(_struct(ai)), ctypes.byref(_struct(af))) == 1, id


def _al16(a, name):
    return a[name + "_off"] % 4 == 0 and a[name + "_bs"] % 4 == 0 and a[name + "_cs"] % 4 == 0


@pytest.mark.parametrize("id", R.IDS)
def test_case_ids_say_what_the_cases_do(id):
    spec = R.spec_of(id)
    ai, af, _, _ = R.case(id)
    a = af if spec["kind"] == "fwd" else ai
    cg, items, res = R.launch_shape(spec)
    hop = R.hop_of(a["k"])
    geom = None if spec["kind"] == "pair" else R.ds_geom(a, spec["kind"] == "inv")
    assert cg == 1 or a["C"] % cg, "the last channel group of a case is a partial one"
    if cg == 1:
        assert geom["nchunk"] > 1                                 # one row per item only where the row itself is chunked
    if "_vec_" in id or "_scalar_" in id:
        if spec["kind"] == "fwd":
            vec = a["L"] % 4 == 0 and _al16(a, "x")
        else:
            vec = a["L"] % 4 == 0 and _al16(a, "y") and (a.get("res") is None or _al16(a, "res"))
        assert vec == ("_vec_" in id)
    if spec.get("act") or spec["kind"] == "pair":
        assert a["L"] % 4 == 0 and (spec["kind"] == "pair" or _al16(a, "x"))
    assert ("chunked" in id) == (geom is not None and geom["nchunk"] > 1)
    if "chunked" in id:
        assert 17500 <= a["L"] <= 40000 and a["C"] <= 8
    if "ongrid" in id:
        assert a["L"] % (a["dil"] * hop) == 0
    elif "one_segment" in id:
        assert a["L"] < hop and a["nseg"] == 1
    else:
        assert a["L"] % (a["dil"] * hop)
    if "uneven_phases" in id:                                    # phases 0, 1 hold 8 samples, the others 7
        assert a["L"] % a["dil"]
    if spec["kind"] == "inv":
        assert id.endswith("_nbuf%d" % R.inv_nbuf(a))
    if "persistent" in id:
        assert items > 2 * res, (items, res)                      # every workgroup of a 256-CU device walks >= 3 items
    if "ragged" in id:
        lens = [int(v) for v in af["act_len"]]
        assert 1 in lens and any(v % 4 for v in lens) and a["L"] in lens or "chunked" in id
        if "chunked" not in id:
            assert any(0 < min(v % 240, 240 - v % 240) <= 6 for v in lens)
    if "items_past_end" in id:
        g = R.ds_geom(af, False)
        starts = [af["dil"] * c * g["S"] * hop - af["pad"] for c in range(g["nchunk"])]
        assert any(int(v) <= starts[-1] for v in af["act_len"])


def test_the_table_covers_what_it_must():
    ids = " ".join(R.IDS)
    assert "_nbuf1" in ids and "_nbuf2" in ids
    inv = [s for s in R.SPECS if s["kind"] == "inv"]
    assert {(bool(s.get("res")), bool(s.get("acc"))) for s in inv} == {(False, False), (False, True), (True, False), (True, True)}
    assert any(s.get("ps") for s in inv) and any(not s.get("ps") for s in inv)
    assert any(s.get("bias") for s in inv) and any(not s.get("bias") for s in inv)
    assert any(R.inv_nbuf(R.case(s["id"])[0]) == 1 and R.launch_shape(s)[0] > 1 for s in inv), "nbuf = 1 on unchunked rows"
    for kind in ("fwd", "inv"):
        ks = {s["k"] for s in R.SPECS if s["kind"] == kind}
        ds = {s["d"] for s in R.SPECS if s["kind"] == kind}
        assert {7, 11, 63} <= ks and ks & {33, 35} and {1, 3, 5} <= ds and ds & {2, 4, 8}
    assert {(s["d"], s["k"]) for s in R.SPECS if s["kind"] == "pair"} >= {(d, k) for d in (1, 3, 5) for k in (7, 11)}
    for kind in ("fwd", "inv", "pair"):
        assert any("persistent" in s["id"] for s in R.SPECS if s["kind"] == kind)
    pair = [s for s in R.SPECS if s["kind"] == "pair"]
    assert {bool(s.get("act_len")) for s in pair} == {True, False} and {int(s.get("prod3", 0)) for s in pair} == {0, 1}


def test_strides_differ_from_the_dense_ones():
    for id in R.IDS:
        ai, af, _, _ = R.case(id)
        for a in (ai, af):
            if a is None:
                continue
            assert a["xf_bs"] > 2 * a["C"] * a["Np"]
            for n in ("x", "y", "res"):
                if a.get(n) is not None:
                    assert a[n + "_cs"] > a["L"] and a[n + "_bs"] > a["C"] * a[n + "_cs"]
                    assert a[n][:R.GUARD].tolist() == [R.SENT] * R.GUARD == a[n][-R.GUARD:].tolist()
