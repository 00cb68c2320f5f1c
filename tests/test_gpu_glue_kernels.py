"""GPU (-m gpu): the pointwise and glue entry points of csrc/hsp_pointwise.hip, the four element-wise kernels of
csrc/hsp_denoiser.hip and hsp_copy_strided_f32, each called through the C ABI on its own against the float64 (or, for
data movement, bit-exact float32) restatements of tests/glue_ref.py -- at the sizes where these kernels change
behaviour: both LayerNorm kernels behind hsp_layernorm_mod_f32 (register kernel up to C = 512, loop kernel above) at
channel counts and lengths that are no multiple of their tiles and with every optional operand set, the 4-rows-per-block
/ 64-lanes-per-row reductions at ragged row and column counts, the second trip of the 4096 x 256 grid of copy_strided,
the row-exact promise of the ragged interpolation, the forced +0 of the DC / Nyquist bins in mag_pha, signed zeros in
atan2 and exp overflow in the sigmoid-like functions.

Float outputs meet helpers.tol_for(reference) (1e-4 x max(1, peak)); data movement and the results the operations
define exactly are compared bit for bit.  Every output sits between canaries and every case checks that nothing outside
the region the call owns was written.  The input conditions these comparisons rely on are asserted on a CPU by
tests/test_glue_ref_host.py for the same seeds.

    python -m pytest tests/test_gpu_glue_kernels.py -q -m gpu
"""
import math

import numpy as np
import pytest
import torch

import glue_ref as R
import helpers as H

pytestmark = pytest.mark.gpu

SENT = 1234.5          # canary for float buffers


@pytest.fixture(scope="module")
def lib():
    from megatts2_hierspeechpp_amd import _lib as L
    return L


@pytest.fixture(scope="module")
def Fh():
    from megatts2_hierspeechpp_amd import functional
    return functional


def _buf(full_shape, slices, device, dtype=torch.float32, fill=SENT):
    """A canary-filled buffer and the view of it that the kernel owns."""
    buf = torch.full(full_shape, fill, dtype=dtype, device=device)
    return buf, buf[slices]


def _flat(shape, device, dtype=torch.float32, fill=SENT, guard=96):
    """A contiguous output of ``shape`` with ``guard`` canary elements on both sides."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * guard,), fill, dtype=dtype, device=device)
    return buf, (slice(guard, guard + n),), buf[guard:guard + n].view(shape)


def _outside_untouched(buf, slices, name, fill=SENT):
    c = buf.clone()
    c[slices] = fill
    assert bool((c == fill).all()), f"{name}: memory outside the output region was written"


def _close(got, ref, name):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert np.isfinite(got).all(), name
    err, tol = float(np.abs(got - ref).max()), H.tol_for(ref)
    print(f"{name}: max|hip - float64| = {err:.3e} (bar {tol:.1e})")
    assert err <= tol, f"{name}: max|hip - ref| = {err:.3e} > {tol:.1e}"
    return err


def _bits(got, want, name):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    same = got.view(np.uint32) == want.view(np.uint32)
    assert same.all(), f"{name}: {int((~same).sum())} of {got.size} elements differ bit for bit"


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _call(code):
    torch.cuda.synchronize()
    assert code == 0, code


# ------------------------------------------------------------------------------------------------ LayerNorm
def _run_ln(lib, device, c, modulate_entry=False):
    """x contiguous, y between canaries, shift / scale as columns of two [B, C + 5] buffers (mod_bs = C + 5)."""
    B, C, T = c["B"], c["C"], c["T"]
    x = _dev(c["x"], device)
    ybuf, ysl, y = _flat((B, C, T), device)
    mask = _dev(c["mask"], device) if c["mask"] is not None else None
    gamma = _dev(c["gamma"], device) if c["gamma"] is not None else None
    beta = _dev(c["beta"], device) if c["beta"] is not None else None
    shift = scale = None
    mod_bs = 0
    if c["scale"] is not None:
        _, shift = _buf((B, C + 5), (slice(None), slice(2, C + 2)), device)
        _, scale = _buf((B, C + 5), (slice(None), slice(3, C + 3)), device)
        shift.copy_(_dev(c["shift"], device))
        scale.copy_(_dev(c["scale"], device))
        mod_bs = C + 5
        assert shift.stride(0) == scale.stride(0) == mod_bs
    f = lib.fptr
    if modulate_entry:
        assert gamma is None
        code = lib.lib().hsp_layernorm_modulate_f32(f(x), f(y), B, C, T, c["eps"], f(mask), f(shift), f(scale), mod_bs,
                                                    lib.stream_ptr())
    else:
        code = lib.lib().hsp_layernorm_mod_f32(f(x), f(y), B, C, T, c["eps"], f(mask), f(shift), f(scale), mod_bs,
                                               f(gamma), f(beta), lib.stream_ptr())
    _call(code)
    _outside_untouched(ybuf, ysl, "layernorm " + R.ln_id(c))
    return y.cpu().numpy()


def _check_ln(lib, device, c):
    ref = R.ln_reference(c)
    got = _run_ln(lib, device, c)
    kernel = "register" if c["C"] <= R.LN_REG_MAX_C else "loop"
    err = _close(got, ref, f"layernorm_mod [{kernel} kernel] {R.ln_id(c)}")
    if c["gamma"] is None:          # the SURVEY name of the same launch
        _bits(_run_ln(lib, device, c, modulate_entry=True), got, "layernorm_modulate " + R.ln_id(c))
    return got, err


@pytest.mark.parametrize("case", R.LN_CASES, ids=R.ln_id)
def test_layernorm(case, device, lib):
    c = R.ln_case(**case)
    got, _ = _check_ln(lib, device, c)
    if c["mask"] is not None and c["scale"] is None:          # masked columns are exactly zero
        assert (got[np.broadcast_to(c["mask"][:, None, :] == 0, got.shape)] == 0).all()


def test_layernorm_512_and_513_channels_agree_with_the_reference_alike(device, lib):
    """The last width of the register kernel and the first of the loop kernel on the same numbers (the narrower case
    is the first 512 channels of the wider one), every operand present: both within the bar."""
    cut, wide = R.ln_pair_cases()
    _, e0 = _check_ln(lib, device, cut)
    _, e1 = _check_ln(lib, device, wide)
    print(f"layernorm C=512 (register) {e0:.3e}, C=513 (loop) {e1:.3e}")


def test_layernorm_functional_wrapper(device, lib, Fh):
    """functional.layernorm_mod issues the same launch: bit-equal to the C ABI call."""
    for case in (R.LN_CASES[8], R.LN_CASES[19]):            # C = 276 and C = 515, every operand
        c = R.ln_case(**case)
        assert c["ops"] == "mas"
        want = _run_ln(lib, device, c)
        d = {k: _dev(c[k], device) for k in ("x", "mask", "shift", "scale", "gamma", "beta")}
        y = Fh.layernorm_mod(d["x"], c["eps"], mask=d["mask"].unsqueeze(1), shift=d["shift"], scale=d["scale"],
                             gamma=d["gamma"], beta=d["beta"])
        torch.cuda.synchronize()
        _bits(y.cpu().numpy(), want, "functional.layernorm_mod " + R.ln_id(c))


# ------------------------------------------------------------------------------------------------ reductions
def _run_masked_mean(lib, device, x, mask):
    B, C, T = x.shape
    obuf, osl, out = _flat((B, C), device)
    xd, md = _dev(x, device), _dev(mask, device)
    _call(lib.lib().hsp_masked_mean_f32(lib.fptr(xd), lib.fptr(md), lib.fptr(out), B, C, T, lib.stream_ptr()))
    _outside_untouched(obuf, osl, "masked_mean")
    return out.cpu().numpy()


@pytest.mark.parametrize("B,C", R.MM_SHAPES)
def test_masked_mean(B, C, device, lib, Fh):
    """Sum over ALL frames / mask sum: x is non-zero in the padded frames, so the mean over the valid frames alone is
    a different number -- further from the result than the bar."""
    for T in R.MM_TS:
        x, mask, lens = R.masked_mean_case(B, C, T)
        ref = R.masked_mean(x, mask)
        got = _run_masked_mean(lib, device, x, mask)
        _close(got, ref, f"masked_mean B={B} C={C} T={T}")
        padded = lens < T
        if padded.any():
            other = R.masked_sum_mean(x, mask)
            assert (np.abs(got - other)[padded] > H.tol_for(ref)).all(), "the padded frames were left out of the sum"
    x, mask, _ = R.masked_mean_case(B, C, 65)
    y = Fh.masked_mean(_dev(x, device), _dev(mask, device).unsqueeze(1))
    torch.cuda.synchronize()
    _bits(y.cpu().numpy(), _run_masked_mean(lib, device, x, mask), "functional.masked_mean")


def test_masked_mean_empty_mask_row_is_the_ieee_quotient(device, lib):
    """include/hsp.h: a row whose mask sums to 0 gets sum / 0 (+-inf, NaN for 0 / 0); the other rows are unaffected."""
    x, mask, _ = R.masked_mean_case(3, 5, 65)
    mask[1] = 0.0
    x[1, 1] *= -1.0
    x[1, 2] = 0.0
    got = _run_masked_mean(lib, device, x, mask)
    assert got[1, 0] == np.inf and got[1, 1] == -np.inf and np.isnan(got[1, 2]) and got[1, 3] == np.inf
    keep = [0, 2]
    _close(got[keep], R.masked_mean(x[keep], mask[keep]), "masked_mean next to an empty row")


@pytest.mark.parametrize("rows", R.FOLD_ROWS)
def test_fold_weight_norm(rows, device, lib):
    for cols in R.FOLD_COLS:
        v, g = R.fold_case(rows, cols)
        wbuf, wsl, w = _flat((rows, cols), device)
        vd, gd = _dev(v, device), _dev(g, device)
        _call(lib.lib().hsp_fold_weight_norm_f32(lib.fptr(vd), lib.fptr(gd), lib.fptr(w), rows, cols, lib.stream_ptr()))
        _close(w.cpu().numpy(), R.fold_weight_norm(v, g), f"fold_weight_norm {rows}x{cols}")
        _outside_untouched(wbuf, wsl, "fold_weight_norm")


def test_fold_helper_takes_a_permuted_weight(device):
    """hip_layers._fold on a weight_v whose memory is not row-major (a permuted view): the folded weight is contiguous
    and holds the logical rows.  (An output allocated with v's strides would be filled in the wrong order.)"""
    from megatts2_hierspeechpp_amd.hip_layers import _fold
    r = np.random.default_rng(2150)
    base = r.standard_normal((3, 5, 6)).astype(np.float32)
    g = r.uniform(0.5, 2.0, (6, 1, 1)).astype(np.float32)
    v = _dev(base, device).permute(2, 1, 0)
    assert not v.is_contiguous()
    w = _fold(v, _dev(g, device))
    torch.cuda.synchronize()
    assert w.shape == (6, 5, 3) and w.is_contiguous()
    ref = R.fold_weight_norm(base.transpose(2, 1, 0).reshape(6, 15), g.reshape(6)).reshape(6, 5, 3)
    _close(w.cpu().numpy(), ref, "hip_layers._fold on a permuted weight")


@pytest.mark.parametrize("C", R.SNAKE_CS)
def test_snake_consts(C, device, lib):
    al, bl = R.snake_case(C)
    abuf, asl, ea = _flat((C,), device)
    bbuf, bsl, binv = _flat((C,), device)
    ad, bd = _dev(al, device), _dev(bl, device)
    _call(lib.lib().hsp_snake_consts_f32(lib.fptr(ad), lib.fptr(bd), lib.fptr(ea), lib.fptr(binv), C, lib.stream_ptr()))
    want_a, want_b = R.snake_consts(al, bl)
    _close(ea.cpu().numpy(), want_a, f"snake_consts exp(alpha) C={C}")
    _close(binv.cpu().numpy(), want_b, f"snake_consts 1/(exp(beta)+1e-9) C={C}")
    _outside_untouched(abuf, asl, "snake_consts alpha")
    _outside_untouched(bbuf, bsl, "snake_consts beta")


# ------------------------------------------------------------------------------------------------ exact data movement
def _run_copy(lib, device, base, view, Fh=None):
    shape = view.shape
    xv = torch.as_strided(_dev(base, device).view(-1), shape, R.elem_strides(view), R.elem_offset(base, view))
    ybuf, ysl, y = _flat(shape, device)
    _call(lib.lib().hsp_copy_strided_f32(lib.fptr(xv), xv.stride(0), xv.stride(1), xv.stride(2), lib.fptr(y), *shape,
                                         lib.stream_ptr()))
    _outside_untouched(ybuf, ysl, "copy_strided")
    if Fh is not None:
        z = Fh.copy_strided(xv)
        torch.cuda.synchronize()
        assert z.is_contiguous() and torch.equal(z, y)
    return y.cpu().numpy()


@pytest.mark.parametrize("shape", [(3, 5, 7), (2, 33, 129)], ids=str)
def test_copy_strided(shape, device, lib, Fh):
    for name, base, view in R.copy_views(shape, seed=sum(shape)):
        _bits(_run_copy(lib, device, base, view, Fh), np.ascontiguousarray(view), f"copy_strided {name} {shape}")


def test_copy_strided_second_trip_of_the_capped_grid(device, lib):
    """1 048 576 + 77 elements: the 4096 x 256 threads take a second trip for the last 77."""
    views = R.copy_views(R.COPY_BIG, seed=77)
    for name, base, view in (views[0], views[2]):
        got = _run_copy(lib, device, base, view)
        want = np.ascontiguousarray(view)
        _bits(got.reshape(-1)[4096 * 256:], want.reshape(-1)[4096 * 256:], f"copy_strided {name}: second trip")
        _bits(got, want, f"copy_strided {name} {R.COPY_BIG}")


@pytest.mark.parametrize("C", [1, 2, 5])
@pytest.mark.parametrize("T", [1, 65])
def test_flip_channels(C, T, device, lib, Fh):
    x = np.random.default_rng(10 * C + T).standard_normal((2, C, T)).astype(np.float32)
    xd = _dev(x, device)
    ybuf, ysl, y = _flat(x.shape, device)
    _call(lib.lib().hsp_flip_channels_f32(lib.fptr(xd), lib.fptr(y), 2, C, T, lib.stream_ptr()))
    _bits(y.cpu().numpy(), R.flip_channels(x), f"flip_channels C={C} T={T}")
    _outside_untouched(ybuf, ysl, "flip_channels")
    assert torch.equal(Fh.flip_channels(xd), y)


@pytest.mark.parametrize("n", R.GATHER_NS)
def test_gather(n, device, lib):
    src, mp = R.gather_case(n)
    dbuf, dsl, dst = _flat((n,), device)
    sd, md = _dev(src, device), _dev(mp, device)
    assert md.dtype == torch.int32
    _call(lib.lib().hsp_gather_f32(lib.fptr(sd), lib.ptr(md), lib.fptr(dst), n, lib.stream_ptr()))
    _bits(dst.cpu().numpy(), R.gather(src, mp), f"gather n={n}")
    _outside_untouched(dbuf, dsl, "gather")


@pytest.mark.parametrize("T", [1, 64, 65])
def test_sequence_mask(T, device, lib, Fh):
    lens = R.seqmask_lengths(T)
    B = len(lens)
    mbuf, msl, mask = _flat((B, T), device)
    ld = _dev(lens, device)
    _call(lib.lib().hsp_sequence_mask_f32(lib.ptr(ld), lib.fptr(mask), B, T, lib.stream_ptr()))
    _bits(mask.cpu().numpy(), R.sequence_mask(lens, T), f"sequence_mask T={T}")
    _outside_untouched(mbuf, msl, "sequence_mask")
    w = Fh.sequence_mask(ld, T)
    assert w.shape == (B, 1, T) and torch.equal(w[:, 0], mask)


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 3, 65), (3, 7, 130)], ids=str)
def test_mask_mul_non_binary_mask(shape, device, lib, Fh):
    B, C, T = shape
    r = np.random.default_rng(B + C + T)
    x = r.standard_normal(shape).astype(np.float32)
    mask = r.uniform(-2.0, 2.0, (B, T)).astype(np.float32)
    xd, md = _dev(x, device), _dev(mask, device)
    ybuf, ysl, y = _flat(shape, device)
    _call(lib.lib().hsp_mask_mul_f32(lib.fptr(xd), lib.fptr(md), lib.fptr(y), B, C, T, lib.stream_ptr()))
    _bits(y.cpu().numpy(), R.mask_mul(x, mask), f"mask_mul {shape}")
    _outside_untouched(ybuf, ysl, "mask_mul")
    assert torch.equal(Fh.mask_mul(xd, md.unsqueeze(1)), y)


@pytest.mark.parametrize("L", [2, 37, 300])
def test_reflect_pad_edges(L, device, lib):
    """pad 0, 1 and L - 1 (the widest the operation allows), rows of pitch L + 3; pad = L is refused and writes nothing."""
    B = 3
    x = np.random.default_rng(L).standard_normal((B, L)).astype(np.float32)
    _, xv = _buf((B, L + 3), (slice(None), slice(0, L)), device, fill=9.0e9)
    xv.copy_(_dev(x, device))
    for pad in sorted({0, 1, L - 1}):
        ybuf, ysl, y = _flat((B, L + 2 * pad), device)
        _call(lib.lib().hsp_reflect_pad_f32(lib.fptr(xv), xv.stride(0), lib.fptr(y), B, L, pad, lib.stream_ptr()))
        _bits(y.cpu().numpy(), R.reflect_pad(x, pad), f"reflect_pad L={L} pad={pad}")
        _outside_untouched(ybuf, ysl, "reflect_pad")
    ybuf, ysl, y = _flat((B, 3 * L), device)
    assert lib.lib().hsp_reflect_pad_f32(lib.fptr(xv), xv.stride(0), lib.fptr(y), B, L, L, lib.stream_ptr()) == lib.EINVAL
    torch.cuda.synchronize()
    assert bool((ybuf == SENT).all()), "a refused call wrote to its output"


# ------------------------------------------------------------------------------------------------ element-wise float
@pytest.mark.parametrize("n", R.AXPBY_NS)
def test_axpby(n, device, lib, Fh):
    r = np.random.default_rng(n)
    x, z = r.standard_normal(n).astype(np.float32), r.standard_normal(n).astype(np.float32)
    xd, zd = _dev(x, device), _dev(z, device)
    for a, b in R.AXPBY_AB:
        ybuf, ysl, y = _flat((n,), device)
        _call(lib.lib().hsp_axpby_f32(lib.fptr(xd), lib.fptr(zd), lib.fptr(y), a, b, n, lib.stream_ptr()))
        _close(y.cpu().numpy(), R.axpby(x, z, a, b), f"axpby n={n} a={a:.3g} b={b:.3g}")
        _outside_untouched(ybuf, ysl, "axpby")
        assert torch.equal(Fh.axpby(xd, zd, a, b), y)


@pytest.mark.parametrize("shape", R.PRIOR_SHAPES, ids=str)
def test_sample_prior(shape, device, lib, Fh):
    B, C, T = shape
    stats, noise, mask = R.prior_case(B, C, T)
    sd, nd, md = _dev(stats, device), _dev(noise, device), _dev(mask, device)
    for ns in R.PRIOR_SCALES:
        zbuf, zsl, z = _flat(shape, device)
        _call(lib.lib().hsp_sample_prior_f32(lib.fptr(sd), lib.fptr(nd), lib.fptr(md), lib.fptr(z), B, C, T, ns,
                                             lib.stream_ptr()))
        got = z.cpu().numpy()
        _close(got, R.sample_prior(stats, noise, mask, ns), f"sample_prior {shape} noise_scale={ns}")
        assert (got[np.broadcast_to(mask[:, None, :] == 0, got.shape)] == 0).all()
        _outside_untouched(zbuf, zsl, "sample_prior")
        assert torch.equal(Fh.sample_prior(sd, nd, md.unsqueeze(1), ns), z)


@pytest.mark.parametrize("kind", range(8), ids=R.ACT_NAMES)
def test_act(kind, device, lib, Fh):
    """4001 points on [-30, 30] plus +-0, +-1e-6, +-20, +-20.001, +-88 and +-104: finite everywhere, and within the bar
    of the reference values of every magnitude band (so that the peak of the large inputs does not widen the bar of
    the small ones)."""
    x = R.act_points()
    n = len(x)
    xd = _dev(x, device)
    ybuf, ysl, y = _flat((n,), device)
    _call(lib.lib().hsp_act_f32(lib.fptr(xd), lib.fptr(y), n, kind, lib.stream_ptr()))
    got, ref = y.cpu().numpy(), R.act(x, kind)
    assert np.isfinite(got).all(), x[~np.isfinite(got)]
    _close(got, ref, f"act {R.ACT_NAMES[kind]}")
    a = np.abs(x)
    for lo, hi in R.ACT_BANDS:
        sel = (a < hi) & ((a >= lo) if lo else True)
        _close(got[sel], ref[sel], f"act {R.ACT_NAMES[kind]} |x| in [{lo:g}, {hi:g})")
    if kind == R.ACT_NONE:
        _bits(got, x, "act none")
    if kind == R.ACT_RELU:                       # exact in value (the sign of relu(-0) is not part of the contract)
        assert np.array_equal(got, np.maximum(x, np.float32(0.0)))
    _outside_untouched(ybuf, ysl, "act")
    assert torch.equal(Fh.act(xd, kind), y)


# ------------------------------------------------------------------------------------------------ linear interpolation
def _run_interp(lib, device, x, Lout, lens=None):
    B, C, Lin = x.shape
    xd = _dev(x, device)
    ybuf, ysl, y = _flat((B, C, Lout), device)
    if lens is None:
        code = lib.lib().hsp_linear_interp_f32(lib.fptr(xd), lib.fptr(y), B, C, Lin, Lout, lib.stream_ptr())
    else:
        li, lo = _dev(lens[0], device), _dev(lens[1], device)
        code = lib.lib().hsp_linear_interp_ragged_f32(lib.fptr(xd), lib.fptr(y), B, C, Lin, Lout, lib.ptr(li),
                                                      lib.ptr(lo), lib.stream_ptr())
    _call(code)
    _outside_untouched(ybuf, ysl, "linear_interp")
    return y.cpu().numpy()


@pytest.mark.parametrize("Lin,Lout", R.INTERP_PLAIN)
def test_linear_interp(Lin, Lout, device, lib, Fh):
    for C in R.INTERP_CS:
        x = R.interp_case(2, C, Lin, seed=3100 + Lin + C)
        got = _run_interp(lib, device, x, Lout)
        _close(got, R.linear_interp(x, Lout), f"linear_interp {Lin}->{Lout} C={C}")
    y = Fh.linear_interp(_dev(x, device), Lout)
    torch.cuda.synchronize()
    _bits(y.cpu().numpy(), got, "functional.linear_interp")


@pytest.mark.parametrize("Lin,ratio", R.INTERP_RAGGED)
def test_linear_interp_ragged_rows_equal_their_own_call(Lin, ratio, device, lib, Fh):
    """Row b over its lens_out[b] outputs is bit for bit the plain call on its first lens_in[b] samples, and exactly 0
    after; the input is non-zero past lens_in[b], so a read beyond the valid prefix would show."""
    B, C, Lout = 4, 2, ratio * Lin
    lin, lout = R.interp_ragged_lens(Lin, ratio)
    x = R.interp_case(B, C, Lin, seed=3200 + Lin + ratio)
    got = _run_interp(lib, device, x, Lout, (lin, lout))
    _close(got, R.linear_interp_ragged(x, Lout, lin, lout), f"linear_interp_ragged Lin={Lin} x{ratio}")
    for b in range(B):
        solo = _run_interp(lib, device, x[b:b + 1, :, :lin[b]], int(lout[b]))
        _bits(got[b:b + 1, :, :lout[b]], solo, f"linear_interp_ragged row {b} (lens_in {lin[b]})")
        assert (got[b, :, lout[b]:] == 0).all(), f"row {b}: outputs past lens_out must be exactly zero"
    y = Fh.linear_interp(_dev(x, device), Lout, lens_in=_dev(lin, device), lens_out=_dev(lout, device))
    torch.cuda.synchronize()
    _bits(y.cpu().numpy(), got, "functional.linear_interp (ragged)")


def test_linear_interp_ragged_clamps_its_lengths(device, lib):
    """include/hsp.h: lens_in is clamped into [1, Lin] and lens_out into [0, Lout].  lens_in = 0 with lens_out > Lout:
    nothing outside the buffer is written (checked by _run_interp) and the row is finite; the full row next to it is
    the plain call."""
    Lin, Lout = 40, 80
    x = R.interp_case(2, 2, Lin, seed=3300)
    got = _run_interp(lib, device, x, Lout, (np.array([0, Lin], np.int64), np.array([Lout + 7, Lout], np.int64)))
    assert np.isfinite(got).all()
    _bits(got[1:], _run_interp(lib, device, x[1:], Lout), "linear_interp_ragged: the full row")


# ------------------------------------------------------------------------------------------------ denoiser element-wise
PI32 = np.float32(math.pi)


@pytest.mark.parametrize("nf", R.DN_FREQS)
@pytest.mark.parametrize("T", R.DN_TS)
def test_mag_pha(nf, T, device, lib):
    """Rows of pitch T + 3.  In the first and the last bin the imaginary part is taken as +0 whatever the buffer holds:
    the phase is exactly +pi where the real part is negative (never -pi) and exactly +0 where it is positive.  Bins
    that are exactly zero give magnitude 0 and phase 0."""
    re, im, zero = R.mag_pha_case(nf, T)
    _, spec = _buf((2 * nf, T + 3), (slice(None), slice(0, T)), device, fill=9.0e9)
    spec.copy_(_dev(np.concatenate([re, im], 0), device))
    for c in R.DN_COMPRESS:
        mbuf, msl, mag = _flat((nf, T), device)
        pbuf, psl, pha = _flat((nf, T), device)
        _call(lib.lib().hsp_mag_pha_f32(lib.fptr(spec), spec.stride(0), lib.fptr(mag), lib.fptr(pha), nf, T, c,
                                        lib.stream_ptr()))
        gm, gp = mag.cpu().numpy(), pha.cpu().numpy()
        wm, wp = R.mag_pha(re, im, c)
        _close(gm, wm, f"mag_pha magnitude nf={nf} T={T} compress={c}")
        _close(gp, wp, f"mag_pha phase nf={nf} T={T} compress={c}")
        for f in (0, nf - 1):
            neg, pos = (re[f] < 0) & ~zero[f], (re[f] > 0) & ~zero[f]
            _bits(gp[f][neg], np.full(int(neg.sum()), PI32), f"mag_pha: phase of bin {f} where re < 0")
            _bits(gp[f][pos], np.zeros(int(pos.sum()), np.float32), f"mag_pha: phase of bin {f} where re > 0")
        assert (gm[zero] == 0).all() and (gp[zero] == 0).all()
        _outside_untouched(mbuf, msl, "mag_pha magnitude")
        _outside_untouched(pbuf, psl, "mag_pha phase")


def _run_atan2(lib, device, y, x):
    n = len(y)
    obuf, osl, out = _flat((n,), device)
    yd, xd = _dev(y, device), _dev(x, device)
    _call(lib.lib().hsp_atan2_f32(lib.fptr(yd), lib.fptr(xd), lib.fptr(out), n, lib.stream_ptr()))
    _outside_untouched(obuf, osl, "atan2")
    return out.cpu().numpy()


def test_atan2_axes_and_signed_zeros(device, lib):
    y, x = R.atan2_axis_case()
    _bits(_run_atan2(lib, device, y, x), np.arctan2(y, x), "atan2 on the axes")


@pytest.mark.parametrize("n", [1, 255, 70001])
def test_atan2_quadrants(n, device, lib):
    y, x = R.atan2_random_case(n, seed=2800)
    _close(_run_atan2(lib, device, y, x), R.atan2(y, x), f"atan2 n={n}")


@pytest.mark.parametrize("nf", R.DN_FREQS)
@pytest.mark.parametrize("T", R.DN_TS)
def test_polar(nf, T, device, lib):
    """re rows of pitch T + 2, im rows of pitch T + 5, canaries between the rows."""
    mag, pha = R.polar_case(nf, T)
    md, pd = _dev(mag, device), _dev(pha, device)
    own = (slice(None), slice(0, T))
    for p in (1.0, 1.0 / 0.3):
        rbuf, re = _buf((nf, T + 2), own, device)
        ibuf, im = _buf((nf, T + 5), own, device)
        _call(lib.lib().hsp_polar_f32(lib.fptr(md), lib.fptr(pd), p, lib.fptr(re), re.stride(0), lib.fptr(im),
                                      im.stride(0), nf, T, lib.stream_ptr()))
        wr, wi = R.polar(mag, pha, p)
        gr, gi = re.cpu().numpy(), im.cpu().numpy()
        _close(gr, wr, f"polar re nf={nf} T={T} power={p:.3g}")
        _close(gi, wi, f"polar im nf={nf} T={T} power={p:.3g}")
        assert (gr[mag == 0] == 0).all() and (gi[mag == 0] == 0).all()
        _outside_untouched(rbuf, own, "polar re")
        _outside_untouched(ibuf, own, "polar im")


@pytest.mark.parametrize("T,F", R.LSIG)
def test_lsigmoid_mul(T, F, device, lib):
    """slope[f] runs along the fast axis; slope * m reaches +-200, where exp overflows: finite, -> 0 or -> beta mag."""
    m, slope, mag = R.lsigmoid_case(T, F)
    beta = 2.0
    obuf, osl, out = _flat((T, F), device)
    d = [_dev(a, device) for a in (m, slope, mag)]
    _call(lib.lib().hsp_lsigmoid_mul_f32(lib.fptr(d[0]), lib.fptr(d[1]), beta, lib.fptr(d[2]), lib.fptr(out), T, F,
                                         lib.stream_ptr()))
    got = out.cpu().numpy()
    _close(got, R.lsigmoid_mul(m, slope, beta, mag), f"lsigmoid_mul T={T} F={F}")
    assert got[-1, 1] == 0.0 and got[-1, 0] == np.float32(beta) * mag[-1, 0]
    _outside_untouched(obuf, osl, "lsigmoid_mul")
