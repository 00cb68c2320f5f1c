"""CPU: the host side of the folded-columns form (hsp_conv1d_args.fold_cols) -- hip_layers.fold_cols_wanted on the
geometries of tests/fold_cases.py, and what hsp_conv1d_mfma_plan (validation + selection, never a launch: it reads no
memory) makes of the field.  The struct mirror itself is pinned by tests/test_host_logic.py."""
import ctypes

import pytest

import conv_ref as R
import fold_cases as FC


@pytest.fixture(scope="module")
def L():
    from megatts2_hierspeechpp_amd import _lib
    return _lib


def _plan(L, s):
    out = (ctypes.c_int32 * 4)()
    return L.lib().hsp_conv1d_mfma_plan(ctypes.byref(s), out), tuple(out)


def test_the_field_is_the_last_of_the_struct(L):
    assert L.Conv1dArgs._fields_[-1][0] == "fold_cols"
    assert L.Conv1dArgs().fold_cols == 0          # off unless a caller sets it


def test_predicate_alone():
    from megatts2_hierspeechpp_amd.hip_layers import fold_cols_wanted as want
    gemm = (64, 64, -2, 73728)
    assert want(gemm, 3, 200) and want(gemm, 5, 72) and want(gemm, 9, 8) and want(gemm, 3, 52)
    assert not want(gemm, 1, 200)                  # one utterance: no seam
    assert not want(gemm, 3, 50)                   # T % 4 != 0: a 16-B group would straddle two utterances
    assert not want(gemm, 3, 128)                  # the per-utterance tiles are full already
    assert not want((128, 128, -2, 147456), 3, 200)   # the 128 x 128 shape keeps the per-utterance tiling
    assert not want((64, 64, -1, 0), 3, 200)       # register-path token GEMM
    # conv tiles: 64 x 64 on plain rows and 64 x 128 on gated rows, with the 64-column window slack, no activation prologue
    assert want((64, 64, 64, 81920), 3, 200) and want((64, 128, 32, 81920), 5, 200, gated=True, halo=4)
    assert not want((64, 64, 32, 81920), 3, 200, gated=True)       # the K-split gated tile
    assert not want((64, 128, 32, 81920), 3, 200)                  # no plain 64 x 128 tile carries it
    assert not want((64, 64, 64, 81920), 3, 200, halo=70)          # the wide-halo tile
    assert not want((64, 64, 64, 81920), 3, 200, act1d=True)
    assert not want((128, 128, 32, 81920), 3, 200) and not want((32, 128, 32, 81920), 3, 200)
    assert not want((64, 64, 64, 81920), 3, 50) and not want((64, 64, 64, 81920), 1, 200) and not want((64, 64, 64, 81920), 3, 128)


@pytest.mark.parametrize("B,T", FC.GEOMETRIES)
def test_predicate_on_the_plan_of_each_geometry(B, T, L):
    """The split-row token GEMM of every geometry: the block GEMM takes it whenever T % 4 == 0, and the layer sets the
    field exactly where the folded tiling differs from the per-utterance one."""
    from megatts2_hierspeechpp_amd.hip_layers import fold_cols_wanted as want
    if T % 4:                                      # no 16-B groups: another kernel takes the 1x1, and it refuses the field
        s = FC.to_struct(f"gemm_plain_res_b{B}_t{T}", FC.fake_base(), 0)
        rc, plan = _plan(L, s)
        assert rc == 0 and plan[2] != -2 and not want(plan, B, T), (rc, plan)
        s.fold_cols = 1
        assert _plan(L, s)[0] == L.EINVAL
        return
    id = f"gemm_split_post_acc2_b{B}_t{T}"
    s = FC.to_struct(id, FC.fake_base(), 0)
    rc, plan = _plan(L, s)
    assert rc == 0 and plan[:3] == (64, 64, -2), (id, rc, plan)
    assert want(plan, B, T) == (B > 1), (id, plan)
    s.fold_cols = 1
    assert _plan(L, s) == (0, plan)                # the field changes neither the kernel nor the tile it reports


def test_a_launch_keeps_its_kernel_with_the_field(L):
    """The block GEMM admits a launch by its per-utterance tile count (>= 96 tiles of 64 x 64) whatever the field says: 704
    rows x 3 x 200 columns are 132 tiles per utterance tiling and 110 folded -- and 9 x 8 columns are 99 against 22."""
    for id in ("gemm_plain_res_b3_t200", "gemm_plain_res_b9_t8"):
        s = FC.to_struct(id, FC.fake_base(), 0)
        rc, plan = _plan(L, s)
        assert rc == 0 and plan[:3] == (64, 64, -2), (id, plan)
        s.fold_cols = 1
        assert _plan(L, s) == (0, plan)


def _kind(a):
    return dict(gated=a["rows"] in (R.ROWS_GATE_WN, R.ROWS_GATE_GLU), halo=(a["K"] - 1) * a["dil"])


@pytest.mark.parametrize("id", [i for i in FC.IDS if i.startswith("conv_")])
def test_conv_cases_take_the_tiles_their_ids_name(id, L):
    """The plan of every conv case: the k = 5 / k = 3 convs sit on the 64 x 64 tile (plain rows) or the 64 x 128 tile (gated
    rows, from 49 tiles; the K-split 64 x 64 tile below); hsp_conv1d_mfma_plan answers the same with the field on the
    kernels that implement the form and HSP_EINVAL on the others; the layer's predicate follows the geometry."""
    from megatts2_hierspeechpp_amd import hip_layers as HL
    a = FC.case(id)[0]
    s = FC.to_struct(id, FC.fake_base(), 0)
    rc, plan = _plan(L, s)
    assert rc == 0 and plan[2] > 0 and plan[0] == 64, (id, rc, plan)
    gated = _kind(a)["gated"]
    tiles128 = -(-a["M"] // 64) * -(-a["ncols"] // 128) * a["B"]
    assert plan[1] == ((128 if tiles128 > 48 else 64) if gated else 64), (id, plan)
    impl = HL.fold_cols_kernel(plan, **_kind(a))
    assert impl == (not gated or plan[1] == 128)
    s.fold_cols = 1
    assert _plan(L, s) == ((0, plan) if impl else (L.EINVAL, (0, 0, 0, 0)))
    B, T = a["B"], a["ncols"]
    assert HL.fold_cols_wanted(plan, B, T, **_kind(a)) == (impl and B > 1 and T % 4 == 0 and T % plan[1] != 0)


def test_refusals(L):
    s = FC.to_struct("gemm_plain_res_b3_t200", FC.fake_base(), 0)
    for bad in (2, -1):
        s.fold_cols = bad
        assert _plan(L, s)[0] == L.EINVAL
    # kernels that do not implement the form refuse it: the register-path token GEMM (a small 1x1) ...
    a = R.build(dict(id="small_gemm", entry="mfma", tile=None, seed=1, K=1, Cin=192, Cout=64, B=3, L=200, bias=True))
    s = R.to_struct(a, R.fake_base())
    rc, plan = _plan(L, s)
    assert rc == 0 and plan[2] != -2, plan
    s.fold_cols = 1
    assert _plan(L, s)[0] == L.EINVAL
