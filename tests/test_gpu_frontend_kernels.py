"""GPU (-m gpu): every entry point of csrc/hsp_frontend.hip, called through the C ABI, against the float64 (or, for the
exact operations, float32 same-order) restatements of tests/frontend_ref.py -- at the sizes where these kernels change
behaviour: the second trip of the 4096 x 256 grid-stride loops (> 1 048 576 elements), the 8-group / 32-channel /
32-frame tiling of the Gaussian kernel up to its 438-phone limit, the 256-phone stride of the duration kernel, the
64-thread block of the code search, idle gate threads and the 1024-step padding loop of the LSTM, and a silent row in the
int16 peak normalisation.

Float outputs meet helpers.tol_for(reference) (1e-4 x max(1, peak)); integer outputs and the exact operations are
compared bit for bit.  Every case also checks that nothing outside the region the call owns was written.  The input
conditions these comparisons rely on are asserted on a CPU by tests/test_frontend_ref_host.py for the same seeds.

    python -m pytest tests/test_gpu_frontend_kernels.py -q -m gpu
"""
import math

import numpy as np
import pytest
import torch

import frontend_ref as R
import helpers as H

pytestmark = pytest.mark.gpu

SENT = 1234.5          # canary for float buffers
ISENT = -7             # canary for integer buffers


@pytest.fixture(scope="module")
def lib():
    from megatts2_hierspeechpp_amd import _lib as L
    return L


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


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


# ------------------------------------------------------------------------------------------- Gaussian upsampling
def _run_gauss(lib, device, c, N=None):
    """x is the first C channels of a [B, C + 1, N] buffer (the product's 257-row layout); dur and rng are columns of
    wider buffers; out is contiguous between canaries."""
    B, C, T = c["B"], c["C"], c["T"]
    N = c["N"] if N is None else N
    xbuf = _dev(c["xbuf"], device)
    x = xbuf[:, :C]
    dbuf, dur = _buf((B, c["N"] + 3), (slice(None), slice(0, c["N"])), device)
    rbuf, rng = _buf((B, c["N"] + 5), (slice(None), slice(2, c["N"] + 2)), device)
    dur.copy_(_dev(c["dur"], device))
    rng.copy_(_dev(c["rng"], device))
    obuf, osl, out = _flat((B, C, T), device)
    lens, frames = _dev(c["lens"], device), _dev(c["frames"], device)
    code = lib.lib().hsp_gaussian_upsample_f32(lib.fptr(x), x.stride(0), x.stride(1), lib.fptr(dur), dur.stride(0),
                                               lib.fptr(rng), rng.stride(0), lib.ptr(lens), lib.fptr(frames),
                                               lib.fptr(out), B, C, N, T, lib.stream_ptr())
    torch.cuda.synchronize()
    return code, obuf, osl, out


@pytest.mark.parametrize("case", R.GAUSS_CASES, ids=lambda c: f"n{c['N']}_c{c['C']}_t{c['T']}")
def test_gaussian_upsample(case, device, lib):
    c = R.gauss_case(**case)
    ref = R.gaussian_upsample(c["xbuf"][:, :c["C"]], c["dur"], c["rng"], c["lens"], c["frames"], c["T"])
    code, obuf, osl, out = _run_gauss(lib, device, c)
    assert code == 0
    got = out.cpu().numpy()
    _close(got, ref, f"gaussian N={c['N']} C={c['C']} T={c['T']}")
    for b in range(c["B"]):
        assert (got[b, :, int(c["frames"][b]):] == 0).all(), f"row {b}: frames past frames[b] must be exactly zero"
    _outside_untouched(obuf, osl, "gaussian")


def test_gaussian_upsample_ignores_padding_values(device, lib):
    """Phones n >= len[b] carry no weight whatever x and rng hold there."""
    c = R.gauss_case(seed=31, N=33, C=32)
    ref = R.gaussian_upsample(c["xbuf"][:, :32], c["dur"], c["rng"], c["lens"], c["frames"], c["T"])
    for b in range(c["B"]):
        c["xbuf"][b, :, c["lens"][b]:] = 1e6
        c["rng"][b, c["lens"][b]:] = 1e-7
    code, obuf, osl, out = _run_gauss(lib, device, c)
    assert code == 0
    _close(out.cpu().numpy(), ref, "gaussian, junk in the padding")
    _outside_untouched(obuf, osl, "gaussian, junk in the padding")


def test_gaussian_upsample_refuses_439_phones(device, lib):
    """The launcher's LDS bound (140 N bytes <= 60 KB) is N <= 438: 439 returns EINVAL and writes nothing."""
    c = R.gauss_case(seed=19, N=R.GAUSS_N_LIMIT + 1, C=8)
    code, obuf, osl, out = _run_gauss(lib, device, c)
    assert code == lib.EINVAL
    assert bool((obuf == SENT).all()), "a refused call wrote to its output"


# ------------------------------------------------------------------------------------------- duration rounding
def _run_duration(lib, device, logw, lens, scale, N, dur_init=None):
    """dur is row 4 of a [B, 5, N] buffer (the duration column of the product's xd), logw a column block of a wider
    buffer, frames sits between canaries."""
    B = len(lens)
    xd, dcol = _buf((B, 5, N), (slice(None), 4), device)
    fbuf, fsl, frames = _flat((B,), device)
    if dur_init is not None:
        dcol.copy_(_dev(dur_init, device))
    if logw is not None:
        lbuf, lw = _buf((B, N + 2), (slice(None), slice(1, N + 1)), device)
        lw.copy_(_dev(logw, device))
        lp, ls = lib.fptr(lw), lw.stride(0)
    else:
        lp, ls = None, 0
    lens_d = _dev(lens, device)
    code = lib.lib().hsp_duration_f32(lp, ls, lib.ptr(lens_d), float(scale), lib.fptr(dcol), dcol.stride(0),
                                      lib.fptr(frames), B, N, lib.stream_ptr())
    torch.cuda.synchronize()
    assert code == 0
    _outside_untouched(xd, (slice(None), 4), "duration: dur")
    _outside_untouched(fbuf, fsl, "duration: frames")
    return dcol.cpu().numpy(), frames.cpu().numpy()


@pytest.mark.parametrize("N", R.DUR_NS)
@pytest.mark.parametrize("scale", R.DUR_SCALES)
def test_duration_from_logw(N, scale, device, lib):
    logw, lens = R.duration_case(100 + N, N, scale)
    want, frames, _ = R.duration_exact(logw, lens, scale)
    dur, fr = _run_duration(lib, device, logw, lens, scale, N)
    assert np.array_equal(dur.astype(np.float64), want), f"{int((dur != want).sum())} durations differ from ceil(float64)"
    assert np.array_equal(fr.astype(np.int64), frames) and fr.dtype == np.float32


@pytest.mark.parametrize("scale", [1.0, 2.0])
def test_duration_exact_points(scale, device, lib):
    """logw = 0: exp is exactly 1, so the duration is exactly the scale."""
    N = 257
    lens = np.array([N, 100], np.int64)
    dur, fr = _run_duration(lib, device, np.zeros((2, N), np.float32), lens, scale, N)
    want, frames, _ = R.duration_exact(np.zeros((2, N), np.float32), lens, scale)
    assert np.array_equal(dur, want) and fr.tolist() == [N * scale, 100 * scale] and frames.tolist() == fr.tolist()


@pytest.mark.parametrize("N", [1, 256, 257, 700])
def test_duration_keep_mode(N, device, lib):
    """logw == NULL: valid entries are kept bit for bit (halves included), the padding is cleared, rows are summed."""
    r = np.random.default_rng(200 + N)
    init = (r.integers(0, 41, (4, N)) * 0.5).astype(np.float32)
    lens = np.array([0, max(1, N // 2), N, N + 5], np.int64)
    want, frames = R.duration_keep(init, lens)
    dur, fr = _run_duration(lib, device, None, lens, 1.0, N, dur_init=init)
    assert np.array_equal(dur.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(fr.astype(np.float64), frames)


# ------------------------------------------------------------------------------------------- grid-stride kernels
BIG = (16, 256, 300)          # 1 228 800 elements: the 4096 x 256 grid takes a second trip


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 7, 13), (3, 33, 65), BIG], ids=str)
@pytest.mark.parametrize("ntab,scale", [(1, 1.0), (2, 16.0), (3, 16.0), (3, math.sqrt(192.0))])
def test_embedding_sum(shape, ntab, scale, device, lib):
    B, C, T = shape
    r = np.random.default_rng(300 + C + ntab)
    rows = (126, 11, 4)[:ntab]
    tabs = [r.standard_normal((n, C)).astype(np.float32) for n in rows]
    ids = [r.integers(0, n, (B, T)) for n in rows]
    want = R.embedding_sum(ids, tabs, scale)
    obuf, out = _buf((B, C + 1, T + 3), (slice(None), slice(0, C), slice(0, T)), device)
    idev = [_dev(i, device) for i in ids]
    p = [lib.ptr(i) for i in idev] + [None] * (3 - ntab)
    tdev = [_dev(t, device) for t in tabs]
    tp = [lib.fptr(t) for t in tdev] + [None] * (3 - ntab)
    nr = list(rows) + [0] * (3 - ntab)
    code = lib.lib().hsp_embedding_sum_f32(p[0], p[1], p[2], tp[0], tp[1], tp[2], nr[0], nr[1], nr[2], float(scale),
                                           lib.fptr(out), out.stride(0), out.stride(1), B, C, T, lib.stream_ptr())
    torch.cuda.synchronize()
    assert code == 0
    got = out.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
        f"{int((got != want).sum())} of {got.size} elements differ, max {np.abs(got - want).max():.2e}"
    _outside_untouched(obuf, (slice(None), slice(0, C), slice(0, T)), "embedding_sum")


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 7, 13), (3, 33, 65), BIG], ids=str)
def test_add_cbias(shape, device, lib):
    B, C, T = shape
    r = np.random.default_rng(400 + C)
    xbuf = r.standard_normal((B, C + 1, T + 1)).astype(np.float32)
    cbuf = r.standard_normal((B, C + 2)).astype(np.float32)
    want = R.add_cbias(xbuf[:, :C, :T], cbuf[:, :C])
    xd, cd = _dev(xbuf, device), _dev(cbuf, device)
    x, cb = xd[:, :C, :T], cd[:, :C]
    ybuf, ysl, y = _flat((B, C, T), device)
    code = lib.lib().hsp_add_cbias_f32(lib.fptr(x), x.stride(0), x.stride(1), lib.fptr(cb), cb.stride(0), lib.fptr(y), B, C,
                                       T, lib.stream_ptr())
    torch.cuda.synchronize()
    assert code == 0
    assert np.array_equal(y.cpu().numpy().view(np.uint32), want.view(np.uint32))
    _outside_untouched(ybuf, ysl, "add_cbias")


@pytest.mark.parametrize("n", [1, 255, 257, 4099, 16 * 256 * 300 + 37])
def test_zero_below(n, device, lib):
    thr = math.log(55.0)
    r = np.random.default_rng(500 + n % 97)
    x = (thr + r.standard_normal(n)).astype(np.float32)
    special = np.array([np.float32(thr), -np.inf, np.nan, np.inf, np.nextafter(np.float32(thr), np.float32(0)), -0.0],
                       np.float32)
    for at in (0, n // 2, n - len(special)):          # the last block lies in the loop's second trip for the big n
        if 0 <= at and at + len(special) <= n:
            x[at:at + len(special)] = special
    want = R.zero_below(x, thr)
    ybuf, ysl, y = _flat((n,), device)
    xd = _dev(x, device)
    code = lib.lib().hsp_zero_below_f32(lib.fptr(xd), float(thr), lib.fptr(y), n, lib.stream_ptr())
    torch.cuda.synchronize()
    assert code == 0
    assert np.array_equal(y.cpu().numpy().view(np.uint32), want.view(np.uint32))
    _outside_untouched(ybuf, ysl, "zero_below")


@pytest.mark.parametrize("B,C,L,k", [(1, 1, 8, 8), (2, 20, 307, 8), (3, 5, 29, 3), (1, 3, 7, 7), (16, 20, 26405, 8)])
def test_maxpool1d(B, C, L, k, device, lib):
    """Floor mode (L not a multiple of k), strided input; 16 x 20 x 3300 outputs cross the grid-stride cap."""
    r = np.random.default_rng(600 + L)
    xbuf = r.standard_normal((B, C + 1, L + 3)).astype(np.float32)
    want = R.maxpool1d(xbuf[:, :C, :L], k)
    xd = _dev(xbuf, device)
    x = xd[:, :C, :L]
    ybuf, ysl, y = _flat((B, C, L // k), device)
    code = lib.lib().hsp_maxpool1d_f32(lib.fptr(x), x.stride(0), x.stride(1), lib.fptr(y), B, C, L, k, lib.stream_ptr())
    torch.cuda.synchronize()
    assert code == 0
    assert np.array_equal(y.cpu().numpy().view(np.uint32), want.view(np.uint32))
    _outside_untouched(ybuf, ysl, "maxpool1d")


# ------------------------------------------------------------------------------------------- nearest code
def _run_vq(lib, device, x, embed, B, T, rep, Tout):
    cbuf, codes = _buf((B, Tout + 4), (slice(None), slice(0, Tout)), device, dtype=torch.int64, fill=ISENT)
    e = _dev(embed, device)
    code = lib.lib().hsp_vq_nearest_f32(lib.fptr(x), x.stride(0), x.stride(1), lib.fptr(e), lib.ptr(codes), codes.stride(0),
                                        B, embed.shape[1], T, embed.shape[0], rep, Tout, lib.stream_ptr())
    torch.cuda.synchronize()
    assert code == 0
    _outside_untouched(cbuf, (slice(None), slice(0, Tout)), "vq_nearest", fill=ISENT)
    return codes.cpu().numpy()


@pytest.mark.parametrize("case", R.VQ_CASES, ids=lambda c: f"b{c['B']}_t{c['T']}_r{c['rep']}_cut{c['cut']}")
def test_vq_nearest(case, device, lib):
    """D = 20, 1024 codes; every column must equal the float64 nearest code (the host test asserts that every column's
    margin is at least 1e-4 for these seeds, so none is left out)."""
    xbuf, embed = R.vq_case(**case)
    B, T, rep = case["B"], case["T"], case["rep"]
    Tout = rep * T - case["cut"]
    want, margin = R.vq_nearest(xbuf[:, 1:21, :T], embed, rep, Tout)
    assert float(margin.min()) >= R.VQ_MIN_MARGIN
    x = _dev(xbuf, device)[:, 1:21, :T]
    got = _run_vq(lib, device, x, embed, B, T, rep, Tout)
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {got.size} codes differ"


def test_vq_nearest_ties_go_to_the_first_index(device, lib):
    x, embed = R.vq_tie_case()
    want, _ = R.vq_nearest(x, embed)
    got = _run_vq(lib, device, _dev(x, device), embed, x.shape[0], x.shape[2], 1, x.shape[2])
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {got.size} codes differ"


# ------------------------------------------------------------------------------------------- LSTM
def _lstm_case(device, In, Hd, layers, N, lens, seed):
    from megatts2_hierspeechpp_amd.hip_layers import finalize
    from megatts2_hierspeechpp_amd.ttv_v1.lstm import LSTM
    torch.manual_seed(seed)
    ref = torch.nn.LSTM(In, Hd, num_layers=layers, bidirectional=True, batch_first=True).eval()
    sd = {k: v.detach().clone() for k, v in ref.state_dict().items()}
    mine = LSTM(In, Hd, num_layers=layers)
    mine.load_state_dict(sd, strict=True)
    finalize(mine, device)
    lens = torch.tensor(lens)
    x = torch.randn(len(lens), N, In)
    want = R.lstm_packed_f64(sd, x, torch.clamp(lens, min=1), In, Hd, layers)
    want[lens == 0] = 0.0                        # a packed sequence cannot hold an empty row: it is all padding
    with torch.no_grad():
        got = mine(x.transpose(1, 2).contiguous().to(device), lens.to(device)).transpose(1, 2).cpu()
    torch.cuda.synchronize()
    return got.numpy(), want.numpy(), lens


@pytest.mark.parametrize("Hd,In", [(4, 9), (128, 64), (256, 257)])
@pytest.mark.parametrize("layers", [1, 2])
def test_lstm_against_float64(Hd, In, layers, device):
    """H < 256 leaves gate threads idle; lengths 300 (a long recurrence), 1, 0 and 37 in one batch."""
    got, want, lens = _lstm_case(device, In, Hd, layers, 300, [300, 1, 0, 37], seed=700 + Hd + layers)
    _close(got, want, f"lstm H={Hd} layers={layers}")
    for b, n in enumerate(lens.tolist()):
        assert (got[b, n:] == 0).all(), f"row {b}: steps past its length must be exactly zero"


def test_lstm_padding_loop_second_trip(device):
    """N = 1100 with a 3-step row: 1097 padded steps, more than the 1024 threads that clear them in one trip."""
    got, want, lens = _lstm_case(device, 64, 128, 1, 1100, [1100, 3], seed=771)
    _close(got, want, "lstm N=1100")
    assert (got[1, 3:] == 0).all()


# ------------------------------------------------------------------------------------------- int16 peak normalisation
def _run_peak(lib, device, x, lens, gain=None, gains=None):
    B, n = x.shape
    xbuf = torch.full((B, n + 5), 9.0e9, dtype=torch.float32, device=device)     # junk after every row
    xv = xbuf[:, :n]
    xv.copy_(_dev(x, device))
    obuf, out = _buf((B, n + 3), (slice(None), slice(0, n)), device, dtype=torch.int16, fill=ISENT)
    lens_d = _dev(lens, device) if lens is not None else None
    lp = lib.ptr(lens_d) if lens is not None else None
    gains_d = _dev(gains, device) if gains is not None else None
    if gains is None:
        code = lib.lib().hsp_peak_int16(lib.fptr(xv), xv.stride(0), lp, float(gain), lib.ptr(out), out.stride(0), B, n,
                                        lib.stream_ptr())
    else:
        code = lib.lib().hsp_peak_int16_gains(lib.fptr(xv), xv.stride(0), lp, lib.fptr(gains_d), lib.ptr(out),
                                              out.stride(0), B, n, lib.stream_ptr())
    torch.cuda.synchronize()
    assert code == 0
    _outside_untouched(obuf, (slice(None), slice(0, n)), "peak_int16", fill=ISENT)
    return out.cpu().numpy()


@pytest.mark.parametrize("n", [1000, 1023, 1024, 1025, 5000])
def test_peak_int16(n, device, lib):
    """Both entry points against the float32 numpy restatement in the reference's operation order: bit-equal, since
    division and multiplication are correctly rounded on both sides.  Rows: plain, a negative peak, short, length 0,
    all zeros with a positive length (must come out as zeros, as numpy's NaN -> int16 cast gives), and a gain above 1
    that saturates.  Seen on an MI355X: no difference in any sample."""
    x, lens, gains = R.peak_case(50 + n % 7, n)
    for g in (0.999, 1.0, 1.37):
        gv = np.full(len(lens), g, np.float32)
        got = _run_peak(lib, device, x, lens, gain=float(gv[0]))
        want = R.peak_int16(x, lens, gv)
        assert (got[4] == 0).all(), f"silent row came out as {np.unique(got[4]).tolist()} at gain {g}"
        assert np.array_equal(got, want), f"gain {g}: {int((got != want).sum())} samples differ"
    got = _run_peak(lib, device, x, lens, gains=gains)
    want = R.peak_int16(x, lens, gains)
    assert (got[4] == 0).all(), f"silent row came out as {np.unique(got[4]).tolist()} (per-row gains)"
    assert np.array_equal(got, want), f"per-row gains: {int((got != want).sum())} samples differ"
    assert want[5].max() == 32767 or want[5].min() == -32768       # the clamp bites in this case
    # lengths == NULL: every row over all n samples
    got = _run_peak(lib, device, x, None, gain=0.999)
    assert np.array_equal(got, R.peak_int16(x, None, np.full(len(lens), 0.999, np.float32)))
