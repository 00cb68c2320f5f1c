"""GPU (-m gpu): the seeded prior noise kernels (include/hsp.h "seeded prior noise"), called through the C ABI between
canaries: hsp_randn_rows_f32 against the float64 restatement of tests/prior_noise_ref.py, batch independence bit for
bit, hsp_sample_prior_seeded_f32 against hsp_sample_prior_f32 on the materialised noise bit for bit (and against
float64), and a captured graph that replays with new seeds.

Shapes: one frame, rows of 3 / 4 / 5 frames (below, on and above one group of four), 19 and 65 frames at the model's 192
channels, 1027 frames (256 whole groups and a partial one); T % 4 == 0 on a 16-byte aligned and on a misaligned base
(the vector and the scalar stores); and one launch of 2^28 + 128 groups, 128 more than one trip of the grid-stride loop
(1048576 blocks of 256 threads), whose last 512 frames belong to the second trip.  Seeds from {0, 1, -1, 2^32, 2^40 + 5,
2^63 - 1}: both key words, the sign.  The conditions of the stream are asserted on a CPU by
tests/test_prior_noise_host.py.

Bar: helpers.tol_for(reference) = 1e-4 x max(1, peak), as for every glue kernel; fp32 log, sqrt, sinpi and cospi sit a
few ulp from |n| <= 5.8, so the measured maximum (printed) is near 1e-6.

    python -m pytest tests/test_gpu_prior_noise.py -q -m gpu -s
"""
import numpy as np
import pytest
import torch

import glue_ref as G
import helpers as H
import prior_noise_ref as R

pytestmark = pytest.mark.gpu

SENT = 1234.5          # canary
POOL = [0, 1, -1, 2 ** 32, 2 ** 40 + 5, 2 ** 63 - 1]
SHAPES = [(1, 1, 1), (2, 3, 3), (2, 3, 4), (3, 3, 5), (3, 192, 19), (2, 192, 65), (1, 5, 1027)]
GRID_TRIP = 1048576 * 256     # threads of one trip of the grid-stride loop (csrc/hsp_pointwise.hip: loop_grid)


@pytest.fixture(scope="module")
def lib():
    from megatts2_hierspeechpp_amd import _lib as L
    return L


@pytest.fixture(scope="module")
def Fh():
    from megatts2_hierspeechpp_amd import functional
    return functional


def _seeds(i, B):
    return [POOL[(i + b) % len(POOL)] for b in range(B)]


def _dev_seeds(seeds, device):
    return torch.tensor(seeds, dtype=torch.int64).to(device)


def _between_canaries(shape, device, guard):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * guard,), SENT, dtype=torch.float32, device=device)
    return buf, buf[guard:guard + n].view(shape)


def _guards_untouched(buf, guard, name):
    assert bool((buf[:guard] == SENT).all()) and bool((buf[-guard:] == SENT).all()), \
        f"{name}: memory outside the output region was written"


def _randn(lib, device, seeds, C, T, guard=96):
    """hsp_randn_rows_f32 into a [B, C, T] region with ``guard`` canary floats on both sides (96: a 16-byte aligned
    region, 97: a misaligned one)."""
    B = len(seeds)
    sd = _dev_seeds(seeds, device)
    buf, out = _between_canaries((B, C, T), device, guard)
    assert (out.data_ptr() % 16 == 0) == (guard % 4 == 0)
    code = lib.lib().hsp_randn_rows_f32(lib.ptr(sd), lib.fptr(out), B, C, T, lib.stream_ptr())
    torch.cuda.synchronize()
    assert code == 0, code
    _guards_untouched(buf, guard, f"randn_rows {(B, C, T)}")
    return out


def _close(got, ref, name):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert np.isfinite(got).all(), name
    err, tol = float(np.abs(got - ref).max()), H.tol_for(ref)
    print(f"{name}: max|hip - float64| = {err:.3e} (bar {tol:.1e})")
    assert err <= tol, f"{name}: max|hip - ref| = {err:.3e} > {tol:.1e}"
    return err


# ------------------------------------------------------------------------------------------------ against float64
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=[str(s) for s in SHAPES])
def test_randn_rows_against_float64(i, device, lib):
    B, C, T = SHAPES[i]
    seeds = _seeds(i, B)
    got = _randn(lib, device, seeds, C, T).cpu().numpy()
    _close(got, R.randn_rows(seeds, C, T), f"randn_rows {(B, C, T)} seeds {seeds}")
    assert np.abs(got).max() <= R.R_MAX * (1 + 1e-6)


def test_every_seed_of_the_pool_is_used():
    assert {s for i, (B, _, _) in enumerate(SHAPES) for s in _seeds(i, B)} == set(POOL)


@pytest.mark.parametrize("T", [4, 64, 1028])
def test_vector_and_scalar_stores_give_the_same_bits(T, device, lib):
    """T % 4 == 0: an aligned region takes the 16-byte stores, a misaligned one the scalar stores."""
    seeds = [2 ** 40 + 5, -1]
    a = _randn(lib, device, seeds, 5, T, guard=96)
    b = _randn(lib, device, seeds, 5, T, guard=97)
    assert torch.equal(a, b)
    _close(a.cpu().numpy(), R.randn_rows(seeds, 5, T), f"randn_rows (2, 5, {T}) vector stores")


def test_second_trip_of_the_grid(device, lib):
    """3 x 89478528 groups = one trip of the launcher's grid and 128 groups: the last 512 frames of channel 2 are drawn
    by threads on their second trip.  Compared: the first 64 and the last 4096 frames of every channel."""
    C, T, seed = 3, 4 * 89478528, 2 ** 40 + 5
    assert GRID_TRIP < C * (T // 4) == GRID_TRIP + 128
    out = _randn(lib, device, [seed], C, T)
    head, tail = out[0, :, :64].cpu().numpy(), out[0, :, T - 4096:].cpu().numpy()
    del out
    _close(head, R.randn_row(seed, C, 64), "second trip: first 64 frames")
    _close(tail, R.randn_row(seed, C, T, T - 4096), "second trip: last 4096 frames")


# ------------------------------------------------------------------------------------------------ batch independence
def test_rows_do_not_depend_on_the_batch(device, Fh):
    """The rows of a B = 3, T = 19 call equal three B = 1 calls at T = 14, 19 and 5 on their common frames."""
    seeds = _dev_seeds([2 ** 63 - 1, -1, 2 ** 32], device)
    batch = Fh.randn_rows(seeds, 192, 19)
    assert batch.shape == (3, 192, 19)
    for b, T in enumerate((14, 19, 5)):
        solo = Fh.randn_rows(seeds[b:b + 1], 192, T)
        assert solo.shape == (1, 192, T) and torch.equal(batch[b, :, :T], solo[0]), b
    # a longer row begins with the shorter one; a CPU seed tensor means the same
    assert torch.equal(Fh.randn_rows(seeds.cpu(), 192, 64, device=device)[:, :, :19], batch)
    assert not torch.equal(batch[0], batch[1])


# ------------------------------------------------------------------------------------------------ fused = materialised
def _prior_case(B, C, T, seed):
    r = np.random.default_rng(seed)
    stats = r.standard_normal((B, 2 * C, T)).astype(np.float32)
    stats[:, C:] *= 0.5                                                 # logs: exp() in [0.1, 8]
    lens = np.maximum(1, T - (T // 3) * np.arange(B))                   # ragged: row 0 whole, the others shorter
    mask = (np.arange(T)[None, :] < lens[:, None]).astype(np.float32)
    return stats, mask


@pytest.mark.parametrize("noise_scale", [0.333, 1.0])
@pytest.mark.parametrize("shape", [(3, 192, 19), (2, 3, 5), (1, 192, 20), (2, 5, 64)], ids=str)
def test_fused_equals_materialised(shape, noise_scale, device, lib, Fh):
    B, C, T = shape
    seeds = _seeds(B + T, B)
    stats, mask = _prior_case(B, C, T, T)
    st, mk, sd = torch.from_numpy(stats).to(device), torch.from_numpy(mask).to(device), _dev_seeds(seeds, device)
    noise = Fh.randn_rows(sd, C, T)
    buf, z = _between_canaries((B, C, T), device, 96)
    code = lib.lib().hsp_sample_prior_seeded_f32(lib.fptr(st), lib.ptr(sd), lib.fptr(mk), lib.fptr(z), B, C, T,
                                                 noise_scale, lib.stream_ptr())
    torch.cuda.synchronize()
    assert code == 0, code
    _guards_untouched(buf, 96, f"sample_prior_seeded {shape}")
    want = torch.empty(B, C, T, device=device)
    code = lib.lib().hsp_sample_prior_f32(lib.fptr(st), lib.fptr(noise), lib.fptr(mk), lib.fptr(want), B, C, T,
                                          noise_scale, lib.stream_ptr())
    torch.cuda.synchronize()
    assert code == 0, code
    assert torch.equal(z, want), f"{int((z != want).sum())} of {z.numel()} elements differ bit for bit"
    # the wrapper is these two launches
    assert torch.equal(Fh.sample_prior(st, None, mk.unsqueeze(1), noise_scale, seeds=sd), z)
    assert torch.equal(Fh.sample_prior(st, noise, mk.unsqueeze(1), noise_scale), z)
    ref = G.sample_prior(stats, R.randn_rows(seeds, C, T), mask, noise_scale)
    _close(z.cpu().numpy(), ref, f"sample_prior_seeded {shape} x {noise_scale}")
    assert not z.cpu().numpy()[np.broadcast_to(mask[:, None, :] == 0, z.shape)].any()    # masked frames are zero


def test_int_seeds_give_row_b_the_seed_s_plus_b(device, Fh):
    stats, mask = _prior_case(3, 192, 19, 1)
    st, mk = torch.from_numpy(stats).to(device), torch.from_numpy(mask).to(device).unsqueeze(1)
    a = Fh.sample_prior(st, None, mk, 0.333, seeds=7)
    b = Fh.sample_prior(st, None, mk, 0.333, seeds=torch.tensor([7, 8, 9]))
    assert torch.equal(a, b)
    for r in range(3):                                                   # ... and row r alone draws with 7 + r
        assert torch.equal(Fh.sample_prior(st[r:r + 1], None, mk[r:r + 1], 0.333, seeds=7 + r), a[r:r + 1])


# ------------------------------------------------------------------------------------------------ graph
def test_captured_graph_replays_with_new_seeds(device, Fh):
    stats, mask = _prior_case(3, 192, 19, 2)
    st, mk = torch.from_numpy(stats).to(device), torch.from_numpy(mask).to(device).unsqueeze(1)
    first, new = _dev_seeds([5, 6, 7], device), _dev_seeds([2 ** 40 + 5, -1, 2 ** 63 - 1], device)
    dev_seeds = first.clone()
    eager_first = Fh.sample_prior(st, None, mk, 0.333, seeds=dev_seeds)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        z = Fh.sample_prior(st, None, mk, 0.333, seeds=dev_seeds)
    g.replay()
    torch.cuda.synchronize()
    replay_first = z.clone()
    assert torch.equal(replay_first, eager_first)
    dev_seeds.copy_(new)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(z, Fh.sample_prior(st, None, mk, 0.333, seeds=new))
    assert not torch.equal(z, replay_first)
