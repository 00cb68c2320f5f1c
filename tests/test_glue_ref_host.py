"""CPU: the float64 restatements of tests/glue_ref.py against torch's CPU operations in float64 (1e-12 relative), the
input conditions the GPU kernel tests rely on for the exact seeds those tests use, and the argument refusals of the
entry points, which need no device:

  * every masked_mean row has a mask sum of at least 1,
  * every LayerNorm column has a standard deviation of at least 0.5 (C = 1 excepted: a one-channel column is exactly
    its own mean in any arithmetic, so the normalised value is exactly 0 on both sides),
  * no atan2 / mag_pha input other than the deliberate exact zeros lies within 1e-3 of the branch cut (im = 0, re < 0),
  * the rows of the ragged interpolation cases have the batch's fp32 ratio, so "bitwise equal to the call on the row
    alone" is a fair demand,
  * the float32 framing and ragged reflect-pad restatements (tests/test_gpu_framing_contract.py) equal torch's
    F.pad(mode="reflect") + unfold x window on the CPU exactly.

    python -m pytest tests/test_glue_ref_host.py -q
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import glue_ref as R
import helpers as H

RTOL = 1e-12


@pytest.fixture(autouse=True)
def _threads():
    torch.set_num_threads(min(16, torch.get_num_threads()))


def _t64(a):
    return torch.from_numpy(np.asarray(a, np.float32)).double()


def _same(got, want, name):
    """Element-wise: |got - want| <= 1e-12 max(1, |want|)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    assert float(err.max()) <= RTOL, f"{name}: relative difference {err.max():.2e}"


# ------------------------------------------------------------------------------------------------ LayerNorm
def test_layernorm_table_covers_both_kernels():
    """Every C of the table at two T, every T at two C, both kernels at every T, every operand set in both kernels."""
    cases = R.LN_CASES
    for C in (1, 15, 16, 17, 276, 511, 512, 513, 515, 1024):
        assert len({c["T"] for c in cases if c["C"] == C}) >= 2, C
    for T in (1, 15, 17, 63, 65, 130):
        cs = {c["C"] for c in cases if c["T"] == T}
        assert len(cs) >= 2 and min(cs) <= R.LN_REG_MAX_C < max(cs), (T, cs)
    for reg in (True, False):
        mine = [c for c in cases if (c["C"] <= R.LN_REG_MAX_C) == reg]
        assert {c["ops"] for c in mine} == {"", "m", "a", "s", "mas"}
        assert {c["B"] for c in mine} == {1, 3} and sum(c["offset"] == 100.0 for c in mine) == 1
    assert all(c["offset"] is None or (c["offset"] <= 100.0 and c["ops"] == "") for c in cases)
    assert 24 <= len(cases) + 2 <= 32


def _torch_layernorm(c):
    y = TF.layer_norm(_t64(c["x"]).transpose(1, 2), (c["C"],),
                      _t64(c["gamma"]) if c["gamma"] is not None else None,
                      _t64(c["beta"]) if c["beta"] is not None else None, float(np.float32(c["eps"]))).transpose(1, 2)
    if c["mask"] is not None:
        y = y * _t64(c["mask"]).unsqueeze(1)
    if c["scale"] is not None:
        y = y * (1 + _t64(c["scale"]).unsqueeze(-1)) + _t64(c["shift"]).unsqueeze(-1)
    return y.numpy()


@pytest.mark.parametrize("case", R.LN_CASES + list(R.ln_pair_cases()), ids=R.ln_id)
def test_layernorm_restatement_and_conditions(case):
    c = case if "x" in case else R.ln_case(**case)
    x = c["x"].astype(np.float64)
    if c["C"] > 1:
        assert float(x.std(1).min()) >= R.LN_MIN_STD, x.std(1).min()
    off = np.abs(x.mean(1))
    assert float(off.max()) <= (100.0 if c["offset"] else 10.0) * (1 + 1e-6)
    if c["mask"] is not None:
        m = c["mask"]
        assert set(np.unique(m)) <= {0.0, 1.0} and 1.0 in m.sum(1) and m.sum(1).max() == c["T"]
    for k, bound in (("gamma", 2.0), ("beta", 1.0), ("shift", 1.0)):
        assert c[k] is None or float(np.abs(c[k]).max()) <= bound
    assert c["scale"] is None or float(np.abs(1.0 + c["scale"].astype(np.float64)).max()) <= 2.0 + 1e-6
    _same(R.ln_reference(c), _torch_layernorm(c), R.ln_id(c))


def test_layernorm_pair_shares_its_first_512_channels():
    cut, wide = R.ln_pair_cases()
    assert cut["C"] == R.LN_REG_MAX_C and wide["C"] == R.LN_REG_MAX_C + 1
    assert np.array_equal(cut["x"], wide["x"][:, :cut["C"]]) and np.array_equal(cut["scale"], wide["scale"][:, :cut["C"]])


# ------------------------------------------------------------------------------------------------ activations
def test_act_restatements_match_torch():
    x = R.act_points()
    assert len(x) == 4001 + 2 * len(R.ACT_SPECIAL) and np.signbit(x[x == 0]).any()
    t = _t64(x)
    want = {R.ACT_NONE: t, R.ACT_TANH: torch.tanh(t), R.ACT_GELU_TANH: TF.gelu(t, approximate="tanh"),
            R.ACT_RELU: torch.relu(t), R.ACT_MISH: TF.mish(t), R.ACT_SILU: TF.silu(t), R.ACT_SOFTPLUS: TF.softplus(t),
            R.ACT_GELU_ERF: TF.gelu(t)}
    assert sorted(want) == list(range(8)) and len(R.ACT_NAMES) == 8
    for kind, w in want.items():
        got = R.act(x, kind)
        assert np.isfinite(got).all()
        _same(got, w.numpy(), R.ACT_NAMES[kind])
    # the bands of the GPU comparison leave no point out
    a = np.abs(x)
    covered = sum(int(((a >= lo) & (a < hi)).sum()) if lo else int((a < hi).sum()) for lo, hi in R.ACT_BANDS)
    assert covered == len(x)


# ------------------------------------------------------------------------------------------------ interpolation
@pytest.mark.parametrize("Lin,Lout", R.INTERP_PLAIN + ((64000, 16000), (16000, 48000)))
def test_linear_interp_restatement(Lin, Lout):
    """torch runs in float32 (the index is fp32 by definition): the project's 1e-4 bar."""
    x = R.interp_case(2, 3, Lin, seed=3000 + Lin)
    want = TF.interpolate(torch.from_numpy(x), size=Lout, mode="linear", align_corners=False).numpy()
    got = R.linear_interp(x, Lout)
    err = float(np.abs(got - want).max())
    print(f"interp {Lin}->{Lout}: max|float64 blend - torch fp32| = {err:.2e}")
    assert err <= 0.01 * H.tol_for(got), err
    i0, i1, l1 = R.interp_index(Lin, Lout)
    assert i0.min() >= 0 and i1.max() <= Lin - 1 and ((i1 - i0) >= 0).all() and (l1 >= 0).all() and (l1 < 1).all()


@pytest.mark.parametrize("Lin,ratio", R.INTERP_RAGGED)
def test_ragged_interp_rows_have_the_batch_ratio(Lin, ratio):
    lin, lout = R.interp_ragged_lens(Lin, ratio)
    assert lin.tolist() == [Lin, Lin - 1, 1, 17] and (lout == ratio * lin).all() and lout.max() == ratio * Lin
    batch = np.float32(Lin) / np.float32(ratio * Lin)
    for a, b in zip(lin, lout):
        assert np.float32(a) / np.float32(b) == batch
        i0, i1, _ = R.interp_index(int(a), int(b))           # the row alone never reads past its own length
        assert i1.max() <= a - 1
    x = R.interp_case(4, 2, Lin, seed=7)
    y = R.linear_interp_ragged(x, ratio * Lin, lin, lout)
    for b in range(4):
        assert (y[b, :, lout[b]:] == 0).all() and (y[b, :, :lout[b]] != 0).all()


# ------------------------------------------------------------------------------------------------ reductions
@pytest.mark.parametrize("rows", R.FOLD_ROWS)
def test_fold_weight_norm_restatement(rows):
    for cols in R.FOLD_COLS:
        v, g = R.fold_case(rows, cols)
        assert float(np.abs(v).max(1).min()) >= 0.1 or cols > 1
        want = torch._weight_norm(_t64(v), _t64(g).unsqueeze(1), 0).numpy()
        _same(R.fold_weight_norm(v, g), want, f"fold {rows}x{cols}")


@pytest.mark.parametrize("B,C", R.MM_SHAPES)
def test_masked_mean_conditions(B, C):
    for T in R.MM_TS:
        x, mask, lens = R.masked_mean_case(B, C, T)
        assert float(mask.sum(1).min()) >= 1.0 and (mask.sum(1) == lens).all()
        assert (x != 0).all()                                          # the padded frames hold data
        full, valid = R.masked_mean(x, mask), R.masked_sum_mean(x, mask)
        _same(full, (_t64(x).sum(2) / _t64(mask).sum(1, keepdim=True)).numpy(), "masked_mean")
        padded = lens < T
        assert T == 1 or B == 1 or padded.any()
        # the two readings of "masked mean" are further apart than the bar wherever a row has padding
        assert (np.abs(full - valid)[padded] > 10 * H.tol_for(full)).all()
        assert np.array_equal(full[~padded], valid[~padded])


def test_pointwise_restatements_match_torch():
    st, noise, mask = R.prior_case(2, 3, 65)
    for ns in R.PRIOR_SCALES:
        m, logs = _t64(st)[:, :3], _t64(st)[:, 3:]
        want = (m + _t64(noise) * torch.exp(logs) * float(np.float32(ns))) * _t64(mask).unsqueeze(1)
        _same(R.sample_prior(st, noise, mask, ns), want.numpy(), "sample_prior")
    assert (st != 0).all() and (mask == 0).any() and st[:, 3:].min() >= -6 and st[:, 3:].max() <= 3
    al, bl = R.snake_case(257)
    ea, binv = R.snake_consts(al, bl)
    _same(ea, torch.exp(_t64(al)).numpy(), "snake alpha")
    _same(binv, (1.0 / (torch.exp(_t64(bl)) + 1e-9)).numpy(), "snake beta")
    assert np.abs(al).max() <= 3 and np.abs(bl).max() <= 3
    x = R.interp_case(1, 1, 255, seed=5)[0, 0]
    for a, b in R.AXPBY_AB:
        _same(R.axpby(x, x[::-1], a, b), (float(np.float32(a)) * _t64(x) + float(np.float32(b)) * _t64(x[::-1].copy())).numpy(), "axpby")
    # exact data movement
    xx = np.random.default_rng(1).standard_normal((2, 5, 7)).astype(np.float32)
    assert np.array_equal(R.flip_channels(xx), torch.flip(torch.from_numpy(xx), [1]).numpy())
    for pad in (0, 1, 6):
        assert np.array_equal(R.reflect_pad(xx[0], pad), TF.pad(torch.from_numpy(xx[:1]), (pad, pad), mode="reflect")[0].numpy())
    lens = R.seqmask_lengths(64)
    assert {0, 1, 64, 67}.issubset(lens.tolist()) and lens.min() < 0
    assert R.sequence_mask(lens, 64).sum(1).tolist() == [0, 1, 64, 64, 0, 32]
    src, mp = R.gather_case(257)
    g = R.gather(src, mp)
    assert (mp < 0).any() and (g[mp < 0] == 0).all() and np.array_equal(g[mp >= 0], src[mp[mp >= 0]])
    assert len(np.unique(mp[mp >= 0])) < (mp >= 0).sum()               # repeated sources
    mk = np.random.default_rng(2).uniform(-2, 2, (2, 7)).astype(np.float32)
    assert np.array_equal(R.mask_mul(xx, mk), (torch.from_numpy(xx) * torch.from_numpy(mk).unsqueeze(1)).numpy())


@pytest.mark.parametrize("n_fft,hop,L", [(R.FRAME_N_FFT, R.FRAME_HOP, n) for n in R.FRAME_RAGGED] + [(100, 7, 120)])
def test_framing_restatement_is_torchs_padded_unfold_times_window(n_fft, hop, L):
    """F.pad(reflect) + unfold + one fp32 multiply on the CPU: exactly the restatement, with and without a scale."""
    assert R.FRAME_LS[0] == max(R.FRAME_RAGGED) and R.FRAME_LS[1] == R.FRAME_N_FFT // 2 + 1 == min(R.FRAME_RAGGED)
    x, w = R.frame_rows(1, L, seed=4000 + L)[0], R.frame_window(n_fft)
    assert (x != 0).all() and w[0] == 0 and (w[1:] != 0).all()
    for scale in (None, 3.0, 1.25):
        xs = torch.from_numpy(x) if scale is None else torch.from_numpy(x) * torch.tensor(scale, dtype=torch.float32)
        padded = TF.pad(xs[None, None], (n_fft // 2, n_fft // 2), mode="reflect")[0, 0]
        want = (padded.unfold(0, n_fft, hop) * torch.from_numpy(w)).t().numpy()            # [n_fft, T]
        got = R.stft_frames(x, w, hop, scale)
        assert got.dtype == np.float32 and got.shape == (n_fft, 1 + L // hop) == want.shape
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), scale


def test_ragged_and_packed_framing_restatements_place_the_rows():
    lens = list(R.FRAME_RAGGED)
    first, frames, T_tot = R.packed_table(lens)
    assert frames == [1 + n // R.FRAME_HOP for n in lens] and T_tot == sum(frames) + R.FRAME_GAP * 2
    x, w = R.frame_rows(3, max(lens), seed=4200), R.frame_window()
    f_ld = R.frame_ld(T_tot)
    assert f_ld % 4 == 0 and 0 < f_ld - T_tot < 4
    rag = R.stft_frames_ragged(x, lens, w, R.FRAME_HOP, R.frame_ld(frames[0]))
    for scale in (None, R.FRAME_SCALE):
        pk = R.stft_frames_packed(x, lens, w, R.FRAME_HOP, first, f_ld, scale)
        used = np.zeros(f_ld, bool)
        for b, (s, n) in enumerate(zip(first, frames)):
            want = R.stft_frames(x[b, :lens[b]], w, R.FRAME_HOP, None if scale is None else scale[b])
            assert np.array_equal(pk[:, s:s + n], want) and (scale is not None or np.array_equal(rag[b, :, :n], want))
            assert not rag[b, :, n:].any()
            used[s:s + n] = True
        assert not pk[:, ~used].any() and (pk[1:, used] != 0).all()
    for L, pad in R.PAD_SHAPES:
        xx = R.frame_rows(3, L, seed=4400 + L)
        lens = [L, pad + 1, max(pad + 1, (2 * L) // 3)]
        y = R.reflect_pad_ragged(xx, lens, pad)
        for b, n in enumerate(lens):
            want = TF.pad(torch.from_numpy(xx[b:b + 1, :n].copy())[None], (pad, pad), mode="reflect")[0, 0].numpy()
            assert np.array_equal(y[b, :n + 2 * pad], want) and not y[b, n + 2 * pad:].any()


def test_copy_views_are_the_denoisers_layouts():
    for shape in ((3, 5, 7), (2, 33, 129)):
        views = R.copy_views(shape, seed=1)
        assert [n for n, _, _ in views] == ["permute(1,0,2)", "permute(2,0,1)", "permute(2,1,0)", "t()", "slice"]
        for name, base, view in views:
            assert view.shape == shape and not view.flags["C_CONTIGUOUS"], name
            s, o = R.elem_strides(view), R.elem_offset(base, view)
            idx = o + sum(np.arange(n).reshape([-1 if k == d else 1 for k in range(3)]) * s[d] for d, n in enumerate(shape))
            assert np.array_equal(base.reshape(-1)[idx], view), name
    assert int(np.prod(R.COPY_BIG)) > 4096 * 256 and all(n % 2 for n in R.COPY_BIG[1:])


# ------------------------------------------------------------------------------------------------ denoiser
@pytest.mark.parametrize("nf", R.DN_FREQS)
@pytest.mark.parametrize("T", R.DN_TS)
def test_denoiser_restatements_and_branch_cut(nf, T):
    re, im, zero = R.mag_pha_case(nf, T)
    inner = np.zeros_like(zero)
    inner[1:nf - 1] = True
    assert R.cut_distance(re[inner & ~zero], im[inner & ~zero]) >= R.CUT_CLEARANCE
    for f in (0, nf - 1):                              # the forced bins: noise of both signs, negative real parts
        if T > 1:
            assert (im[f] < 0).any() and (im[f] > 0).any() and (re[f] < 0).any() and (re[f] > 0).any()
        assert (re[f][~zero[f]] != 0).all()
    assert zero.any() and (re[zero] == 0).all() and (im[zero] == 0).all() and not np.signbit(re[zero]).any()
    for c in R.DN_COMPRESS:
        mag, pha = R.mag_pha(re, im, c)
        im0 = im.copy()
        im0[0] = im0[-1] = 0.0
        z = torch.complex(_t64(re), _t64(im0))
        _same(mag, torch.abs(z).pow(float(np.float32(c))).numpy(), "mag")
        _same(pha, torch.angle(z).numpy(), "pha")
        assert (mag[zero] == 0).all() and (pha[zero] == 0).all()
        assert (pha[0][re[0] < 0] == math.pi).all() and (pha[-1][re[-1] < 0] == math.pi).all()
    mg, ph = R.polar_case(nf, T)
    assert (mg == 0).any() and mg.min() >= 0 and np.abs(ph).max() <= np.float32(math.pi)
    assert np.float32(math.pi) in ph and -np.float32(math.pi) in ph
    for p in (1.0, 1.0 / 0.3):
        a, b = R.polar(mg, ph, p)
        z = torch.polar(_t64(mg).pow(float(np.float32(p))), _t64(ph))
        _same(a, z.real.numpy(), "polar re")
        _same(b, z.imag.numpy(), "polar im")


def test_atan2_restatement_and_branch_cut():
    y, x = R.atan2_random_case(70001, seed=2800)
    assert R.cut_distance(x, y) >= R.CUT_CLEARANCE
    for sy in (1, -1):
        for sx in (1, -1):
            assert ((np.sign(y) == sy) & (np.sign(x) == sx)).sum() > 1000
    _same(R.atan2(y, x), torch.atan2(_t64(y), _t64(x)).numpy(), "atan2")
    ya, xa = R.atan2_axis_case()
    assert len({(bool(np.signbit(a)), float(abs(a)), bool(np.signbit(b)), float(abs(b))) for a, b in zip(ya, xa)}) == 12
    want = torch.atan2(torch.from_numpy(ya), torch.from_numpy(xa)).numpy()
    assert np.array_equal(np.arctan2(ya, xa).view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("T,F", R.LSIG)
def test_lsigmoid_restatement(T, F):
    m, slope, mag = R.lsigmoid_case(T, F)
    s = slope[None, :].astype(np.float64) * m
    assert s.max() >= 200.0 and s.min() <= -200.0 and len(np.unique(slope)) > F // 2
    out = R.lsigmoid_mul(m, slope, 2.0, mag)
    _same(out, (_t64(mag) * 2.0 * torch.sigmoid(_t64(slope) * _t64(m))).numpy(), "lsigmoid")
    assert np.isfinite(out).all() and out[-1, 1] < 1e-80 and abs(out[-1, 0] - 2.0 * mag[-1, 0]) < 1e-12


# ------------------------------------------------------------------------------------------------ refusals
def test_gather_helper_refuses_a_strided_destination():
    """hip_layers._gather hands dst.numel() to a kernel that writes consecutive floats: a strided destination (or a map
    of another size or type) is refused before anything is launched."""
    from megatts2_hierspeechpp_amd.hip_layers import _gather
    src, mp = torch.zeros(8), np.zeros(8, np.int32)
    with pytest.raises(AssertionError):
        _gather(src, mp, torch.zeros(4, 2).t())
    with pytest.raises(AssertionError):
        _gather(src, mp[:6], torch.zeros(8))
    with pytest.raises(AssertionError):
        _gather(src, mp.astype(np.int64), torch.zeros(8))


P, Q = 16, 32          # dummy non-NULL pointers: every call below fails its checks before anything is launched

# name -> (arguments of a well-formed call, positions of the required pointers, positions of the sizes)
GOOD = {
    "hsp_layernorm_mod_f32": ([P, Q, 2, 3, 4, 1e-5, None, None, None, 0, None, None, None], (0, 1), (2, 3, 4)),
    "hsp_layernorm_modulate_f32": ([P, Q, 2, 3, 4, 1e-5, None, None, None, 0, None], (0, 1), (2, 3, 4)),
    "hsp_masked_mean_f32": ([P, P, Q, 2, 3, 4, None], (0, 1, 2), (3, 4, 5)),
    "hsp_sample_prior_f32": ([P, P, P, Q, 2, 3, 4, 0.5, None], (0, 1, 2, 3), (4, 5, 6)),
    "hsp_mask_mul_f32": ([P, P, Q, 2, 3, 4, None], (0, 1, 2), (3, 4, 5)),
    "hsp_axpby_f32": ([P, P, Q, 1.0, 1.0, 5, None], (0, 1, 2), (5,)),
    "hsp_act_f32": ([P, Q, 5, 1, None], (0, 1), (2,)),
    "hsp_fold_weight_norm_f32": ([P, P, Q, 3, 4, None], (0, 1, 2), (3, 4)),
    "hsp_gather_f32": ([P, P, Q, 5, None], (0, 1, 2), (3,)),
    "hsp_snake_consts_f32": ([P, P, Q, Q, 5, None], (0, 1, 2, 3), (4,)),
    "hsp_linear_interp_f32": ([P, Q, 2, 3, 4, 5, None], (0, 1), (2, 3, 4, 5)),
    "hsp_linear_interp_ragged_f32": ([P, Q, 2, 3, 4, 5, P, P, None], (0, 1, 6, 7), (2, 3, 4, 5)),
    "hsp_copy_strided_f32": ([P, 12, 4, 1, Q, 2, 3, 4, None], (0, 4), (5, 6, 7)),
    "hsp_mag_pha_f32": ([P, 4, Q, Q, 5, 4, 0.3, None], (0, 2, 3), (4, 5)),
    "hsp_lsigmoid_mul_f32": ([P, P, 2.0, P, Q, 3, 4, None], (0, 1, 3, 4), (5, 6)),
    "hsp_atan2_f32": ([P, P, Q, 5, None], (0, 1, 2), (3,)),
    "hsp_polar_f32": ([P, P, 1.0, Q, 4, Q, 4, 5, 4, None], (0, 1, 3, 5), (7, 8)),
    "hsp_flip_channels_f32": ([P, Q, 2, 3, 4, None], (0, 1), (2, 3, 4)),
    "hsp_sequence_mask_f32": ([P, Q, 2, 3, None], (0, 1), (2, 3)),
    "hsp_reflect_pad_f32": ([P, 8, Q, 2, 8, 3, None], (0, 2), (3, 4)),
}


@pytest.fixture(scope="module")
def lib():
    from megatts2_hierspeechpp_amd import _lib
    return _lib


def _with(args, at, value):
    a = list(args)
    a[at] = value
    return a


@pytest.mark.parametrize("name", sorted(GOOD))
def test_entry_points_refuse_null_pointers_and_empty_sizes(name, lib):
    args, ptrs, sizes = GOOD[name]
    fn = getattr(lib.lib(), name)
    assert len(args) == len(lib.SIGNATURES[name][1])
    for at in ptrs:
        assert fn(*_with(args, at, None)) == lib.EINVAL, (name, "NULL at", at)
    for at in sizes:
        for bad in (0, -1):
            assert fn(*_with(args, at, bad)) == lib.EINVAL, (name, bad, "at", at)


def test_entry_points_refuse_inconsistent_arguments(lib):
    E, L = lib.EINVAL, lib.lib()
    ln, lm = GOOD["hsp_layernorm_mod_f32"][0], GOOD["hsp_layernorm_modulate_f32"][0]
    assert L.hsp_layernorm_mod_f32(*_with(ln, 7, P)) == E                       # shift without scale
    assert L.hsp_layernorm_mod_f32(*_with(ln, 8, P)) == E                       # scale without shift
    assert L.hsp_layernorm_mod_f32(*_with(ln, 10, P)) == E                      # gamma without beta
    assert L.hsp_layernorm_mod_f32(*_with(ln, 11, P)) == E                      # beta without gamma
    assert L.hsp_layernorm_modulate_f32(*_with(lm, 7, P)) == E
    assert L.hsp_layernorm_modulate_f32(*_with(lm, 8, P)) == E
    act = GOOD["hsp_act_f32"][0]
    assert lib.ACT_GELU_ERF == R.ACT_GELU_ERF == 7
    for kind in (-1, lib.ACT_GELU_ERF + 1, 1 << 20):
        assert L.hsp_act_f32(*_with(act, 3, kind)) == E
    assert L.hsp_flip_channels_f32(*_with(GOOD["hsp_flip_channels_f32"][0], 1, P)) == E      # x == y
    rp = GOOD["hsp_reflect_pad_f32"][0]
    for pad in (-1, 8, 9):                                                      # pad < 0, pad >= L
        assert L.hsp_reflect_pad_f32(*_with(rp, 5, pad)) == E
    cs = GOOD["hsp_copy_strided_f32"][0]
    for at in (1, 2, 3):
        assert L.hsp_copy_strided_f32(*_with(cs, at, -1)) == E                  # negative strides
    mp = GOOD["hsp_mag_pha_f32"][0]
    assert L.hsp_mag_pha_f32(*_with(mp, 1, 3)) == E                             # row pitch below T
    assert L.hsp_mag_pha_f32(*_with(mp, 4, 1)) == E                             # one bin: no DC / Nyquist pair
    po = GOOD["hsp_polar_f32"][0]
    assert L.hsp_polar_f32(*_with(po, 4, 3)) == E and L.hsp_polar_f32(*_with(po, 6, 3)) == E


def test_framing_launchers_refuse_what_distinguishes_them(lib):
    """Plain takes any T whose last frame's centre lies inside the signal, ragged exactly T = 1 + L / hop and a lengths
    pointer, packed a checked segment table with no row above 1 + L / hop frames.  (The accepted controls need real
    buffers: tests/test_gpu_framing_contract.py.)"""
    import ctypes
    E, L = lib.EINVAL, lib.lib()
    n, n_fft, hop = 347, R.FRAME_N_FFT, R.FRAME_HOP
    assert L.hsp_stft_frames_f32(P, P, Q, 1, n, n_fft, hop, 71, 72, None) == E            # (T - 1) hop > L
    assert L.hsp_stft_frames_f32(P, P, Q, 1, n, n_fft, hop, 70, 69, None) == E            # f_ld < T
    assert L.hsp_stft_frames_f32(P, P, Q, 1, n_fft // 2, n_fft, hop, 33, 36, None) == E   # L <= n_fft / 2
    assert L.hsp_stft_frames_f32(P, P, Q, 65536, n, n_fft, hop, 70, 72, None) == E
    for T in (69, 71):
        assert L.hsp_stft_frames_ragged_f32(P, n, P, P, Q, 1, n, n_fft, hop, T, 72, None) == E
    assert L.hsp_stft_frames_ragged_f32(P, n, None, P, Q, 1, n, n_fft, hop, 70, 72, None) == E     # NULL lengths
    assert L.hsp_stft_frames_ragged_f32(P, n - 1, P, P, Q, 1, n, n_fft, hop, 70, 72, None) == E    # x_bs < L

    def packed(table, T_tot, f_ld, n_=n, B=None):
        host = (ctypes.c_int32 * len(table))(*table)
        return L.hsp_stft_frames_packed_f32(P, n, P, None, P, Q, P, ctypes.cast(host, ctypes.c_void_p),
                                            len(table) // 2 if B is None else B, n_, n_fft, hop, T_tot, f_ld, None)

    assert packed([0, 71], 71, 72) == E                       # 71 frames > 1 + 347 / 5
    assert packed([3, 70], 70, 72) == E                       # the segment ends past T_tot
    assert packed([0, 70], 70, 69) == E                       # f_ld < T_tot
    assert packed([0, 33], 33, 36, n_=160) == E               # L <= n_fft / 2
    assert packed([0, 70, 69, 70], 139, 140) == E             # overlapping segments
    assert packed([73, 70, 0, 70], 143, 144) == E             # not ascending
    assert packed([0, 70], 70, 72, B=0) == E
    assert L.hsp_stft_frames_packed_f32(P, n, P, None, P, Q, P, None, 1, n, n_fft, hop, 70, 72, None) == E   # no host table
    rr = [P, 350, P, Q, 374, 2, 300, 37, 374, None]           # hsp_reflect_pad_ragged_f32: Lo = L + 2 pad, pitches above
    for at, bad in ((1, 299), (4, 373), (8, 375), (7, 300), (7, -1), (5, 65536), (0, None), (3, None)):
        assert L.hsp_reflect_pad_ragged_f32(*_with(rr, at, bad)) == E, (at, bad)
