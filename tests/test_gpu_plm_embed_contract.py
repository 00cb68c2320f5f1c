"""The prosody LM's embedding entry points against the formula of include/hsp.h, bit for bit, through the C ABI:

    x[b, c, j] = cat(tc[b, :, j], emb[clamp(codes[b, j])])[c] + alpha[0] * pe_t[c, j]

hsp_plm_embed_f32 (side by side with and without padding, fixed pitch, the one-position form, clamped codes, the second
trip of its capped grid), hsp_plm_embed_step_f32 / hsp_plm_embed_sample_f32 (full and n == 1 forms) and
hsp_plm_embed_pos_f32, on small tables of their own (Dtc = 24, Demb = 4, n_emb = 1026, 1024 logits).

The numpy float32 restatement is EXACT, not close: the tests use alpha = 1.0 and alpha = 0.5 only.  A power of two makes
alpha * pe_t exact in float32, so the kernel's single-rounding fmaf(alpha, pe_t, v) and numpy's multiply-then-add round
once, at the same place, and give the same float32.  Any other alpha would need a tolerance.

Every buffer sits inside a larger sentinel-filled one and is compared WHOLE: whatever the header does not document as
written (the guard zones, the inputs, the other entries of `codes`, the columns of a fixed-pitch x beyond n, the rows of
idle slots) must still hold what it held before the call."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DTC, DEMB, N_EMB, N_LOGITS = 24, 4, 1026, 1024
D = DTC + DEMB
GO = 1024
GUARD = 64                       # sentinel elements in front of and behind every buffer
X_SENT, IN_SENT, CODE_SENT = -12345.5, 777.25, -4242
ALPHAS = [1.0, 0.5]


class Boxed:
    """A host array placed inside a larger sentinel-filled device buffer.  ``t``: the device view with the array's
    shape; ``want``: the host image of the whole buffer, which a test edits to what the call should leave behind."""

    def __init__(self, a, device, fill):
        a = np.ascontiguousarray(a)
        self.want = np.full(a.size + 2 * GUARD, fill, a.dtype)
        self.want[GUARD:GUARD + a.size] = a.reshape(-1)
        self.whole = torch.from_numpy(self.want.copy()).to(device)
        self.t = self.whole[GUARD:GUARD + a.size].view(a.shape)

    @property
    def inner(self):
        """The array's part of ``want``, flat (a view: writes land in ``want``)."""
        return self.want[GUARD:len(self.want) - GUARD]

    def check(self, what):
        got = self.whole.cpu().numpy()
        kind = np.int32 if got.dtype == np.float32 else got.dtype            # floats compare as bit patterns
        bad = np.flatnonzero(got.view(kind) != self.want.view(kind))
        assert bad.size == 0, (f"{what}: {bad.size} elements differ, first at {bad[0] - GUARD} of the buffer: "
                               f"got {got[bad[0]]!r}, want {self.want[bad[0]]!r}")


@functools.lru_cache(maxsize=None)
def _tables(P):
    """The embedding table [n_emb, Demb] and the position table [D, P], seeded, shared by every case of that pitch."""
    rng = np.random.default_rng(1234 + P)
    return (rng.standard_normal((N_EMB, DEMB)).astype(np.float32), rng.standard_normal((D, P)).astype(np.float32))


def _inputs(B, T, seed, code_hi=N_EMB):
    rng = np.random.default_rng(seed)
    tc = rng.standard_normal((B, DTC, T)).astype(np.float32)
    codes = rng.integers(0, code_hi, (B, T + 1)).astype(np.int64)
    codes[:, 0] = GO
    return tc, codes


def _ref(tc, codes, emb, pe, alpha, cols):
    """The header's formula in numpy float32 for the positions ``cols`` -> [B, D, len(cols)]."""
    ids = np.clip(codes[:, cols], 0, N_EMB - 1)                             # the documented clamp into [0, n_emb)
    v = np.concatenate([tc[:, :, cols], emb[ids].transpose(0, 2, 1)], axis=1)
    x = v + np.float32(alpha) * pe[None][:, :, cols]
    assert x.dtype == np.float32
    return x


def _scatter(flat, val, x_bs, x_cs):
    """flat[b * x_bs + c * x_cs + j] = val[b, c, j]"""
    B_, D_, n = val.shape
    b, c, j = np.meshgrid(np.arange(B_), np.arange(D_), np.arange(n), indexing="ij")
    flat[b * x_bs + c * x_cs + j] = val


class Operands:
    """Boxed device copies of one case's operands, and the argument head the embed entry points share, with every
    per-position pointer shifted to column ``t``."""

    def __init__(self, device, tc, codes, P, alpha, x_size):
        emb, pe = _tables(P)
        self.np = dict(tc=tc, codes=codes, emb=emb, pe=pe, alpha=alpha)
        self.P = P
        self.tc, self.codes = Boxed(tc, device, IN_SENT), Boxed(codes, device, CODE_SENT)
        self.emb, self.pe = Boxed(emb, device, IN_SENT), Boxed(pe, device, IN_SENT)
        self.alpha = Boxed(np.array([alpha], np.float32), device, IN_SENT)
        self.x = Boxed(np.full(x_size, X_SENT, np.float32), device, X_SENT)
        self.all = dict(tc=self.tc, codes=self.codes, emb=self.emb, pe_t=self.pe, alpha=self.alpha, x=self.x)

    def ref(self, cols):
        n = self.np
        return _ref(n["tc"], n["codes"], n["emb"], n["pe"], n["alpha"], cols)

    def head(self, x_bs, x_cs, B, n, t=0):
        from megatts2_hierspeechpp_amd import _lib as L
        tc, codes = self.tc.t, self.codes.t
        return (L.fptr(tc[:, :, t:]), tc.stride(0), tc.stride(1), DTC, L.ptr(codes[:, t:]), codes.stride(0),
                L.fptr(self.emb.t), DEMB, N_EMB, L.fptr(self.pe.t[:, t:]), self.P, L.fptr(self.alpha.t),
                L.fptr(self.x.t[t:]), x_bs, x_cs, B, n)

    def check(self, what, extra=()):
        torch.cuda.synchronize()
        for name, box in list(self.all.items()) + list(extra):
            box.check(f"{what}: {name}")


def _embed(ops, *head):
    from megatts2_hierspeechpp_amd import _lib as L
    L.check(L.lib().hsp_plm_embed_f32(*ops.head(*head), L.stream_ptr()), "hsp_plm_embed_f32")


# ----------------------------------------------------------------------------------------------- hsp_plm_embed_f32
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("clamped", [False, True])
def test_embed_side_by_side_with_padding(device, alpha, clamped):
    """B = 3, n = 5, x_bs = 5, x_cs = 16: the batch side by side on 15 columns, column 15 of every row zeroed.
    ``clamped``: codes -5 and 5000 embed rows 0 and n_emb - 1."""
    B, n, x_cs = 3, 5, 16
    tc, codes = _inputs(B, n, 1)
    if clamped:
        codes[0, 2], codes[1, 4], codes[2, 1] = -5, 5000, -5
    ops = Operands(device, tc, codes, 64, alpha, D * x_cs)
    _embed(ops, n, x_cs, B, n)
    ref = ops.ref(np.arange(n))
    if clamped:
        emb, pe = _tables(64)
        assert ref[0, DTC, 2] == emb[0, 0] + np.float32(alpha) * pe[DTC, 2]
        assert ref[1, D - 1, 4] == emb[N_EMB - 1, DEMB - 1] + np.float32(alpha) * pe[D - 1, 4]
    _scatter(ops.x.inner, ref, n, x_cs)
    ops.x.inner.reshape(D, x_cs)[:, B * n:] = 0.0
    ops.check("side by side, padded")


@pytest.mark.parametrize("alpha", ALPHAS)
def test_embed_fixed_pitch_zeroes_nothing(device, alpha):
    """x_bs = 8, x_cs = 24 with n = 5: rows of pitch 8; columns 5 .. 7 of every row keep the sentinel."""
    B, n, x_bs, x_cs = 3, 5, 8, 24
    tc, codes = _inputs(B, n, 2)
    ops = Operands(device, tc, codes, 64, alpha, D * x_cs)
    _embed(ops, x_bs, x_cs, B, n)
    _scatter(ops.x.inner, ops.ref(np.arange(n)), x_bs, x_cs)
    assert (ops.x.inner.reshape(D, B, x_bs)[:, :, n:] == X_SENT).all()
    ops.check("fixed pitch")


@pytest.mark.parametrize("alpha", ALPHAS)
def test_embed_one_position_form(device, alpha):
    """n = 1 with tc, codes, pe_t and x shifted to t = 6: only column 6 of a [D, B, 8] buffer is written."""
    B, T, t = 3, 8, 6
    tc, codes = _inputs(B, T, 3)
    ops = Operands(device, tc, codes, 64, alpha, D * B * T)
    _embed(ops, T, B * T, B, 1, t)
    ops.x.inner.reshape(D, B, T)[:, :, t] = ops.ref(np.array([t]))[:, :, 0].T
    ops.check("one position")


def test_embed_second_trip_of_the_capped_grid(device):
    """B * D * n = 1 050 000 elements, just above the 4096 x 256 one trip of the capped grid covers; padded rows."""
    B, n = 3, 12500
    x_cs = B * n + 4
    tc, codes = _inputs(B, n, 4)
    ops = Operands(device, tc, codes, n + 4, 0.5, D * x_cs)
    assert B * D * n > 4096 * 256
    _embed(ops, n, x_cs, B, n)
    _scatter(ops.x.inner, ops.ref(np.arange(n)), n, x_cs)
    ops.x.inner.reshape(D, x_cs)[:, B * n:] = 0.0
    ops.check("capped grid")


# ------------------------------------------------------- hsp_plm_embed_step_f32 / hsp_plm_embed_sample_f32
def _logits(B, seed):
    """[1024, B] scores (element (c, b) at c * B + b, the loop's layout) with a planted tie at the maximum of every
    row: indices 100 + b and 900 both hold 9.0, and the lower one must win the greedy choice."""
    lg = (np.random.default_rng(seed).standard_normal((N_LOGITS, B)) * 2).astype(np.float32)
    for b in range(B):
        lg[100 + b, b] = lg[900, b] = 9.0
    return lg


def _window_case(codes, col, seed):
    """Logits and previous codes under which the repetition penalty DECIDES the draw of column ``col``, so that the
    window of previous codes the kernel reads (columns 1 .. col - 1) shows in the result.  Row b: tokens 500 + b and
    600 + b score 20.0 and are planted at the two ends of the window, codes[b, 1] and codes[b, col - 1]; token 700 + b
    scores 12.0; every other logit is N(0, 1).  With penalty 4 both planted tokens fall to 5.0, token 700 + b then
    holds more than 0.99 of the softmax mass, top-p 0.95 keeps it alone and the draw is 700 + b whatever the seed.  A
    window that misses either end leaves a 20.0 in place, which wins instead."""
    B = codes.shape[0]
    lg = np.random.default_rng(seed).standard_normal((N_LOGITS, B)).astype(np.float32)
    for b in range(B):
        lg[500 + b, b] = lg[600 + b, b] = 20.0
        lg[700 + b, b] = 12.0
        codes[b, 1], codes[b, col - 1] = 500 + b, 600 + b
    return lg


def _sample_args(device, B):
    from megatts2_hierspeechpp_amd.ttv_v1.t2w2v_transformer import PlmSampling
    seeds = (torch.arange(B, dtype=torch.int64) * 977 - 3).to(device)
    return seeds, PlmSampling(temperature=0.9, top_k=30, top_p=0.95, repetition_penalty=4.0).c_args(seeds)


def _choose_and_embed(device, ops, lg, sampled, col, head):
    """Run the fused entry point that chooses ``codes[:, col]`` and return what it must have stored there: np.argmax for
    the greedy form, what hsp_sample_f32 stores for the same arguments (on a copy of the codes) for the sampled one,
    whose logits and codes are a `_window_case`."""
    from megatts2_hierspeechpp_amd import _lib as L
    B = lg.t.shape[1]
    tail = (L.fptr(lg.t), 1, B, N_LOGITS)
    if not sampled:
        L.check(L.lib().hsp_plm_embed_step_f32(*head, *tail, L.stream_ptr()), "hsp_plm_embed_step_f32")
        want = np.argmax(lg.t.cpu().numpy(), axis=0)
        assert want.tolist() == [100 + b for b in range(B)]
        return want
    seeds, a = _sample_args(device, B)
    alone = ops.codes.t.clone()
    L.check(L.lib().hsp_sample_f32(*tail[:3], B, N_LOGITS, L.ptr(alone[:, col:]), alone.stride(0), col, ctypes.byref(a),
                                   L.stream_ptr()), "hsp_sample_f32")
    L.check(L.lib().hsp_plm_embed_sample_f32(*head, *tail, col, ctypes.byref(a), L.stream_ptr()),
            "hsp_plm_embed_sample_f32")
    torch.cuda.synchronize()                                             # `a` points into `seeds`: alive until here
    want = alone[:, col].cpu().numpy()
    assert want.tolist() == [700 + b for b in range(B)]                  # _window_case: the penalty decided
    return want


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
def test_fused_full_form(device, alpha, sampled):
    """B = 3, n = 50: Dtc * n = 1200 elements make two tc parts, the second partial; B * n = 150 columns in rows of
    152.  codes[:, 49] is chosen from the logits, stored, and embedded as the newest column."""
    B, n, x_cs = 3, 50, 152
    tc, codes = _inputs(B, n + 2, 5, code_hi=40)
    lg = Boxed(_window_case(codes, n - 1, 6) if sampled else _logits(B, 6), device, IN_SENT)
    ops = Operands(device, tc, codes, 64, alpha, D * x_cs)
    chosen = _choose_and_embed(device, ops, lg, sampled, n - 1, ops.head(n, x_cs, B, n))
    assert not (chosen == codes[:, n - 1]).all()
    codes[:, n - 1] = chosen                                             # ops.np["codes"] is this array
    ops.codes.inner.reshape(codes.shape)[:, n - 1] = chosen
    _scatter(ops.x.inner, ops.ref(np.arange(n)), n, x_cs)
    ops.x.inner.reshape(D, x_cs)[:, B * n:] = 0.0
    ops.check("fused full form", [("logits", lg)])


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
def test_fused_one_position_form(device, alpha, sampled):
    """n = 1 at t = 6, B = 5: codes[:, 6] is chosen (from the row's codes 1 .. 5 in the sampled form) and only column 6
    of the [D, B, 8] buffer is written."""
    B, T, t = 5, 8, 6
    tc, codes = _inputs(B, T, 7, code_hi=40)
    lg = Boxed(_window_case(codes, t, 8) if sampled else _logits(B, 8), device, IN_SENT)
    ops = Operands(device, tc, codes, 64, alpha, D * B * T)
    chosen = _choose_and_embed(device, ops, lg, sampled, t, ops.head(T, B * T, B, 1, t))
    assert not (chosen == codes[:, t]).all()
    codes[:, t] = chosen
    ops.codes.inner.reshape(codes.shape)[:, t] = chosen
    ops.x.inner.reshape(D, B, T)[:, :, t] = ops.ref(np.array([t]))[:, :, 0].T
    ops.check("fused one position", [("logits", lg)])


# ------------------------------------------------------------------------------------------- hsp_plm_embed_pos_f32
@pytest.mark.parametrize("alpha", ALPHAS)
def test_embed_pos_mixed_batch(device, alpha):
    """Rows at positions 3, 0 and 7 (= max_pos) beside idle rows (-1, 8 > max_pos, INT32_MIN): an active row's column
    of the [D, B] matrix is the formula at t = pos[b] with un-shifted operands, an idle row's keeps the sentinel."""
    from megatts2_hierspeechpp_amd import _lib as L
    pos = [3, -1, 0, 8, 7, -2 ** 31]
    B, T, top = len(pos), 8, 7
    tc, codes = _inputs(B, T, 9)
    codes[4, 7] = 5000                                                   # clamped as in the full form
    ops = Operands(device, tc, codes, 64, alpha, D * B)
    dpos = Boxed(np.array(pos, np.int32), device, -1)
    L.check(L.lib().hsp_plm_embed_pos_f32(*ops.head(1, B, B, 0)[:15], B, L.ptr(dpos.t), top, L.stream_ptr()),
            "hsp_plm_embed_pos_f32")
    for b, t in enumerate(pos):
        if 0 <= t <= top:
            ops.x.inner.reshape(D, B)[:, b] = ops.ref(np.array([t]))[b, :, 0]
    ops.check("per-row positions", [("pos", dpos)])
