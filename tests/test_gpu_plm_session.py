"""GPU checks of the prosody LM's decode sessions (include/hsp.h "per-row positions"): the three position-form entry
points against the header contract and, bit for bit, against the by-value entry points they share their device functions
with; Megatts2PLM1.infer_many against the float64 decode (tests/plm_causal_ref.py) and against infer(causal=True) on
every request alone -- greedy and sampled, captured and eager, across slot counts, the 256-key mark and slot reuse.
Every float comparison: at most 1e-4 of the reference's range."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import plm_causal_ref as R  # noqa: E402
import plm_sampling_ref as S  # noqa: E402
from test_gpu_plm_causal import _Layer, _args, _close  # noqa: E402  (the weights and the argument block of the contract test)

pytestmark = pytest.mark.gpu
D, H, F = 276, 4, 1104
INT32_MIN = -2 ** 31
LENGTHS = [13, 4, 9, 1, 7]


@pytest.fixture(scope="module")
def plm(device):
    from megatts2_hierspeechpp_amd import synth
    from megatts2_hierspeechpp_amd.ttv_v1.t2w2v_transformer import Megatts2PLM1
    m = Megatts2PLM1()
    m.load_state_dict({k: torch.from_numpy(synth.synth_tensor("plm." + k, tuple(v.shape), 7))
                       for k, v in m.state_dict().items()})
    m.finalize(device)
    return m


@pytest.fixture(scope="module")
def layer(device):
    return _Layer(device)


def _bytes(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


def _i32(values, device):
    return torch.tensor(values, dtype=torch.int32, device=device)


# --------------------------------------------------------------------------------- 1. the position-form layer
def _pos_contract(device, layer, pos, top):
    """One call with the per-row positions ``pos`` and a->t = ``top``: active rows against R.decode_layer in float64 and
    bit for bit against hsp_plm_decode_layer_f32 on the row alone; everything else untouched."""
    from megatts2_hierspeechpp_amd import _lib as L
    Dm, B = layer.D, len(pos)
    Tp = top + 1 + 6                                                          # cache pitch above a->t + 1
    active = [0 <= p <= top for p in pos]
    r = np.random.default_rng(300 + B + top)
    x_np = r.standard_normal((Dm, B)).astype(np.float32)
    kc_np = r.standard_normal((Dm, B, Tp)).astype(np.float32)
    vc_np = r.standard_normal((Dm, B, Tp)).astype(np.float32)
    for b, p in enumerate(pos):                                               # columns at or above the row's position: NaN
        kc_np[:, b, min(max(p, 0), Tp):] = np.nan
        vc_np[:, b, min(max(p, 0), Tp):] = np.nan
    xbuf = torch.zeros(Dm, 2 * B, device=device)                              # x, y: strided views between canaries
    x = xbuf[:, ::2]
    x.copy_(torch.from_numpy(x_np))
    ybuf = torch.full((Dm, B + 3), 7.0, device=device)
    y = ybuf[:, 1:B + 1]
    kc, vc = torch.from_numpy(kc_np).to(device), torch.from_numpy(vc_np).to(device)
    a = _args(L, layer, x, y, kc, vc, top, B)
    L.check(L.lib().hsp_plm_decode_layer_pos_f32(ctypes.byref(a), L.ptr(_i32(pos, device)), L.stream_ptr()),
            "hsp_plm_decode_layer_pos_f32")
    torch.cuda.synchronize()
    got_y, got_k, got_v = y.cpu().numpy(), kc.cpu().numpy(), vc.cpu().numpy()
    ws = a._keep.cpu().numpy()
    ws_at, ws_part = ws[:B * Dm].reshape(B, Dm), ws[B * Dm:].reshape(B, 12, Dm)
    assert torch.equal(x.cpu(), torch.from_numpy(x_np))                       # x unchanged
    assert (ybuf[:, 0] == 7).all() and (ybuf[:, B + 1:] == 7).all()
    for b, t in enumerate(pos):
        if not active[b]:
            assert (got_y[:, b] == 7).all(), (b, t)                            # idle: y, caches, workspace untouched
            assert got_k[:, b].tobytes() == kc_np[:, b].tobytes() and got_v[:, b].tobytes() == vc_np[:, b].tobytes(), (b, t)
            assert np.isnan(ws_at[b]).all() and np.isnan(ws_part[b]).all(), (b, t)
            continue
        k64 = kc_np[:, b:b + 1].transpose(1, 0, 2).astype(np.float64)        # [1, D, Tp]
        v64 = vc_np[:, b:b + 1].transpose(1, 0, 2).astype(np.float64)
        want = R.decode_layer(layer.w64, x_np[:, b:b + 1].T.astype(np.float64), k64, v64, t, H=layer.H)
        assert np.isfinite(got_y[:, b]).all()
        _close(got_y[:, b], want[0], f"y B={B} row {b} pos {t}")
        _close(got_k[:, b, t], k64[0, :, t], f"k B={B} row {b} pos {t}")
        _close(got_v[:, b, t], v64[0, :, t], f"v B={B} row {b} pos {t}")
        other = np.arange(Tp) != t
        assert got_k[:, b][:, other].tobytes() == kc_np[:, b][:, other].tobytes(), (b, t)   # NaN columns included
        assert got_v[:, b][:, other].tobytes() == vc_np[:, b][:, other].tobytes(), (b, t)
        # the by-value entry point on this row alone, t = pos[b]: the same bits
        x1, y1 = torch.from_numpy(x_np[:, b:b + 1].copy()).to(device), torch.zeros(Dm, 1, device=device)
        k1, v1 = torch.from_numpy(kc_np[:, b:b + 1].copy()).to(device), torch.from_numpy(vc_np[:, b:b + 1].copy()).to(device)
        a1 = _args(L, layer, x1, y1, k1, v1, t, 1)
        L.check(L.lib().hsp_plm_decode_layer_f32(ctypes.byref(a1), L.stream_ptr()), "hsp_plm_decode_layer_f32")
        torch.cuda.synchronize()
        assert _bytes(y1[:, 0]) == got_y[:, b].tobytes(), (b, t)
        assert _bytes(k1[:, 0, t]) == got_k[:, b, t].tobytes() and _bytes(v1[:, 0, t]) == got_v[:, b, t].tobytes(), (b, t)


@pytest.mark.parametrize("pos", [[0, -1, 4, 65, 256, 63, 257], [64, INT32_MIN, 1, 3, 255], [256], [65], [257], [-1]],
                         ids=["B7", "B5", "B1-top", "B1", "B1-above", "B1-negative"])
def test_layer_pos_contract(device, layer, pos):
    """The positions where the kernel can go wrong: 0 / 1, the 4-key edge, the wave boundary 63 / 64 / 65, 255 / 256 = a->t,
    and the idle values -1, INT32_MIN and a->t + 1."""
    _pos_contract(device, layer, pos, 256)


def test_layer_pos_contract_second_geometry(device):
    _pos_contract(device, _Layer(device, seed=2, D=64, H=8, F=96), [0, 5, -7, 64, 130, 131, 2 ** 31 - 1], 130)


def test_layer_pos_refuses_null_pos_on_the_device(device, layer):
    from megatts2_hierspeechpp_amd import _lib as L
    x, y = torch.zeros(D, 2, device=device), torch.full((D, 2), 5.0, device=device)
    kc, vc = torch.zeros(D, 2, 8, device=device), torch.zeros(D, 2, 8, device=device)
    a = _args(L, layer, x, y, kc, vc, 3, 2)
    assert L.lib().hsp_plm_decode_layer_pos_f32(ctypes.byref(a), None, L.stream_ptr()) == L.EINVAL
    a.t = 16                                                                  # a->t >= cs = 2 * 8
    assert L.lib().hsp_plm_decode_layer_pos_f32(ctypes.byref(a), L.ptr(_i32([0, 1], device)), L.stream_ptr()) == L.EINVAL
    torch.cuda.synchronize()
    assert (y == 5).all() and (kc == 0).all() and (vc == 0).all()             # nothing was launched


# ------------------------------------------------------------------------------------------------ 2. embedding
def test_embed_pos_equals_the_one_position_form(device, plm):
    from megatts2_hierspeechpp_amd import _lib as L
    lib = L.lib()
    r = np.random.default_rng(41)
    pos, top, Tm = [0, 5, -1, 39, 40, INT32_MIN, 17, 18], 39, 40
    B, Dm = len(pos), plm.d_model
    tc = torch.from_numpy(r.standard_normal((B, 256, Tm + 3)).astype(np.float32)).to(device)[:, :, :Tm]   # pitch above T
    codes_np = r.integers(0, 1024, (B, Tm + 1)).astype(np.int64)
    codes_np[:, 0] = plm.GO_ID
    codes_np[6, 17], codes_np[7, 18] = 5000, -5                               # corrupted codes: clamped as the existing kernel does
    codes = torch.from_numpy(codes_np).to(device)
    xbuf = torch.full((Dm, B + 2), 7.0, device=device)
    x = xbuf[:, 1:B + 1]
    emb, pe, al = plm.pc_embedding._w, plm.pos_emb._pe_t, plm.pos_emb._alpha
    P, n_emb = plm.pos_emb.N_POS, plm.pc_embedding.num_embeddings
    L.check(lib.hsp_plm_embed_pos_f32(L.fptr(tc), tc.stride(0), tc.stride(1), 256, L.ptr(codes), codes.stride(0), L.fptr(emb),
                                      plm.vq_dim, n_emb, L.fptr(pe), P, L.fptr(al), L.fptr(x), x.stride(1), x.stride(0), B,
                                      L.ptr(_i32(pos, device)), top, L.stream_ptr()), "hsp_plm_embed_pos_f32")
    torch.cuda.synchronize()
    got = x.cpu().numpy()
    assert (xbuf[:, 0] == 7).all() and (xbuf[:, B + 1] == 7).all()
    assert torch.equal(codes.cpu(), torch.from_numpy(codes_np))
    emb64 = emb.cpu().numpy().astype(np.float64).reshape(n_emb, plm.vq_dim)
    pe64 = pe.cpu().numpy().astype(np.float64).reshape(Dm, P)
    for b, t in enumerate(pos):
        if not 0 <= t <= top:
            assert (got[:, b] == 7).all(), (b, t)                              # idle rows write nothing
            continue
        x1 = torch.zeros(Dm, 1, device=device)
        L.check(lib.hsp_plm_embed_f32(L.fptr(tc[b:b + 1, :, t]), tc.stride(0), tc.stride(1), 256, L.ptr(codes[b:b + 1, t]),
                                      codes.stride(0), L.fptr(emb), plm.vq_dim, n_emb, L.fptr(pe[t:]), P, L.fptr(al),
                                      L.fptr(x1), 1, 1, 1, 1, L.stream_ptr()), "hsp_plm_embed_f32")
        torch.cuda.synchronize()
        assert _bytes(x1[:, 0]) == got[:, b].tobytes(), (b, t)
        code = min(max(int(codes_np[b, t]), 0), n_emb - 1)
        want = np.concatenate([tc[b, :, t].cpu().numpy().astype(np.float64), emb64[code]]) + float(al.cpu()[0]) * pe64[:, t]
        _close(got[:, b], want, f"embed row {b} pos {t}")


# ---------------------------------------------------------------------------------------- 3. choose and advance
POS, LEN, TOP = [0, 5, -1, 39, 40, 12, INT32_MIN], [3, 6, 9, 40, 41, 20, 5], 39
WANT_POS = [1, -1, -1, -1, 40, 13, INT32_MIN]          # t + 1 below len, -1 exactly at len; idle rows keep their value


def _choose_setup(device, seed):
    r = np.random.default_rng(seed)
    B, N = len(POS), 1024
    lg_np = r.standard_normal((N, B)).astype(np.float32) * 3
    lg_np[[100, 700], 0] = lg_np[:, 0].max() + 1.0                            # an exact tie at the top of row 0
    lg_np[[1023, 3], 5] = lg_np[:, 5].max() + 0.5                             # and one whose first index comes last in memory order
    codes_np = r.integers(0, 1024, (B, TOP + 2)).astype(np.int64)
    codes_np[:, 0] = 1024
    return lg_np, codes_np, torch.from_numpy(lg_np).to(device), torch.from_numpy(codes_np).to(device)


def _choose(L, lg, codes, pos, length, sample=None):
    B = lg.shape[1]
    L.check(L.lib().hsp_plm_choose_advance_f32(L.fptr(lg), 1, lg.stride(0), B, lg.shape[0], L.ptr(codes), codes.stride(0),
                                               L.ptr(pos), L.ptr(length), TOP, ctypes.byref(sample) if sample else None,
                                               L.stream_ptr()), "hsp_plm_choose_advance_f32")
    torch.cuda.synchronize()


def _check_untouched(codes, codes_np, pos, chosen):
    got = codes.cpu().numpy()
    assert pos.cpu().tolist() == WANT_POS
    for b, t in enumerate(POS):
        keep = np.ones(codes_np.shape[1], bool)
        if 0 <= t <= TOP:
            keep[t + 1] = False
            assert got[b, t + 1] == chosen[b], (b, t, got[b, t + 1], chosen[b])
        assert np.array_equal(got[b, keep], codes_np[b, keep]), b               # idle rows whole, active rows but one entry


def test_choose_advance_greedy_equals_argmax(device):
    from megatts2_hierspeechpp_amd import _lib as L
    lg_np, codes_np, lg, codes = _choose_setup(device, 51)
    B = len(POS)
    best = torch.full((B,), -3, dtype=torch.int64, device=device)
    L.check(L.lib().hsp_argmax_f32(L.fptr(lg), 1, lg.stride(0), B, 1024, L.ptr(best), 1, L.stream_ptr()), "hsp_argmax_f32")
    pos = _i32(POS, device)
    _choose(L, lg, codes, pos, _i32(LEN, device))
    best = best.cpu().tolist()
    assert best[0] == 100 and best[5] == 3                                     # first maximal index
    assert best == [int(np.argmax(lg_np[:, b])) for b in range(B)]
    _check_untouched(codes, codes_np, pos, best)


def test_choose_advance_sampled_equals_the_reference_sampler(device):
    from megatts2_hierspeechpp_amd import _lib as L
    from megatts2_hierspeechpp_amd.ttv_v1.t2w2v_transformer import PlmSampling
    sp = PlmSampling(temperature=1.1, top_k=40, top_p=0.95, repetition_penalty=1.2)
    lg_np, codes_np, lg, codes = _choose_setup(device, 52)
    seeds = [5, 2 ** 40 + 3, -9, 0, 77, -2 ** 62, 1]
    sd = torch.tensor(seeds, dtype=torch.int64, device=device)
    pos = _i32(POS, device)
    _choose(L, lg, codes, pos, _i32(LEN, device), sp.c_args(sd))
    want = [S.decide(lg_np[:, b], [int(c) for c in codes_np[b, 1:t + 1]], seeds[b], t + 1, temperature=sp.temperature,
                     top_k=sp.top_k, top_p=sp.top_p, repetition_penalty=sp.repetition_penalty)[0] if 0 <= t <= TOP else None
            for b, t in enumerate(POS)]
    _check_untouched(codes, codes_np, pos, want)
    # and the existing launch for the same column of the same rows
    for b, t in enumerate(POS):
        if 0 <= t <= TOP:
            row = torch.from_numpy(codes_np[b:b + 1].copy()).to(device)
            L.check(L.lib().hsp_sample_f32(L.fptr(lg[:, b]), 1, lg.stride(0), 1, 1024, L.ptr(row[:, t + 1:]), row.stride(0),
                                           t + 1, ctypes.byref(sp.c_args(sd[b:b + 1].contiguous())), L.stream_ptr()),
                    "hsp_sample_f32")
            torch.cuda.synchronize()
            assert int(row[0, t + 1]) == want[b], (b, t)


# --------------------------------------------------------------------------------- 4. sessions == the existing decode
def _many(plm, reqs, **kw):
    """infer_many, and the session it made."""
    made, orig = [], plm.decode_session
    plm.decode_session = lambda *a, **k: (made.append(orig(*a, **k)), made[-1])[1]
    try:
        out = plm.infer_many(reqs, **kw)
    finally:
        del plm.decode_session
    torch.cuda.synchronize()
    assert len(made) == 1
    return out, made[0]


@pytest.fixture(scope="module")
def requests13(device, plm):
    """The rows of the float64 decode case (5, 13) cut in time to LENGTHS: by causality their codes are the prefixes of
    the float64 codes (test_plm_causal_host.py checks the top-2 margin of every step of the full rows)."""
    tc_np, want_codes, _, _ = R.decoded((5, 13))
    reqs = [torch.from_numpy(tc_np[i, :, :n].copy()).to(device) for i, n in enumerate(LENGTHS)]
    want = [want_codes[i, :n] for i, n in enumerate(LENGTHS)]
    solo = [plm.infer(q[None].contiguous(), causal=True)[0] for q in reqs]
    for s, w in zip(solo, want):
        assert np.array_equal(s.cpu().numpy(), w)
    return reqs, want, solo


@pytest.mark.parametrize("capture", [True, False], ids=["captured", "eager"])
@pytest.mark.parametrize("slots", [2, 3, 8])
def test_session_equals_float64_and_solo_decode(device, plm, requests13, slots, capture):
    from megatts2_hierspeechpp_amd.ttv_v1.t2w2v_transformer import session_plan
    reqs, want, solo = requests13
    out, ses = _many(plm, reqs, slots=slots, capture=capture)
    assert len(out) == len(reqs)
    for i, (o, w, s) in enumerate(zip(out, want, solo)):
        assert o.dtype == torch.int64 and o.shape == (LENGTHS[i],)
        assert np.array_equal(o.cpu().numpy(), w), i
        assert torch.equal(o, s), i
    steps = session_plan(LENGTHS, slots)[1]
    assert steps == {2: 20, 3: 13, 8: 13}[slots]
    assert ses.steps == steps
    assert (ses.captures, ses.replays) == ((1, steps) if capture else (0, 0))
    assert ses.pos.cpu().tolist() == [-1] * slots                              # every row finished, every slot idle


def test_session_crosses_the_256_key_mark(device, plm):
    tc_np, want_codes, _, _ = R.decoded((2, 260))
    lengths = [260, 70]
    reqs = [torch.from_numpy(tc_np[i, :, :n].copy()).to(device) for i, n in enumerate(lengths)]
    out, ses = _many(plm, reqs, slots=2)
    for i, n in enumerate(lengths):
        assert np.array_equal(out[i].cpu().numpy(), want_codes[i, :n]), i
    assert torch.equal(out[0], plm.infer(reqs[0][None].contiguous(), causal=True)[0])
    assert ses.steps == ses.replays == 260 and ses.captures == 1


# ------------------------------------------------------------------------------------------------- 5. sampling
def test_session_sampling_equals_solo_runs(device, plm):
    from megatts2_hierspeechpp_amd.ttv_v1.t2w2v_transformer import PlmSampling
    sp = PlmSampling(temperature=1.1, top_k=40, top_p=0.95, repetition_penalty=1.2)
    tc_np = R.case_tc((3, 20), [71, 72, 73])
    lengths, seeds = [20, 7, 12], [5, 2 ** 40 + 3, -9]
    reqs = [torch.from_numpy(tc_np[i, :, :n].copy()).to(device) for i, n in enumerate(lengths)]
    out, ses = _many(plm, reqs, slots=2, sampling=sp, seeds=seeds)
    for i, q in enumerate(reqs):
        sd = torch.tensor([seeds[i]], dtype=torch.int64, device=device)
        assert torch.equal(out[i], plm.infer(q[None].contiguous(), sampling=sp, seeds=sd, causal=True)[0]), i
    again, _ = _many(plm, reqs, slots=2, sampling=sp, seeds=seeds)
    assert all(torch.equal(u, v) for u, v in zip(out, again))
    other, _ = _many(plm, reqs, slots=2, sampling=sp, seeds=[s + 1000 for s in seeds])
    assert not all(torch.equal(u, v) for u, v in zip(out, other))
    by_int, _ = _many(plm, reqs, slots=2, sampling=sp, seeds=40)                # an int: request i gets seed + i
    listed, _ = _many(plm, reqs, slots=2, sampling=sp, seeds=[40, 41, 42])
    assert all(torch.equal(u, v) for u, v in zip(by_int, listed))


# ----------------------------------------------------------------------------------------------- 6. slot reuse
@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
def test_a_reused_slot_does_not_see_its_previous_request(device, plm, requests13, sampled):
    """One slot, two requests: the first (its latent scaled by 1e3, and longer than the second) leaves the slot's cache
    and codes poisoned; the second must come out as it does alone."""
    from megatts2_hierspeechpp_amd.ttv_v1.t2w2v_transformer import PlmSampling
    reqs, _, solo = requests13
    sp = PlmSampling(temperature=1.1, top_k=40, top_p=0.95, repetition_penalty=1.2) if sampled else None
    second = reqs[2]
    alone = plm.infer(second[None].contiguous(), sampling=sp, seeds=torch.tensor([9], dtype=torch.int64, device=device),
                      causal=True)[0] if sampled else solo[2]
    out, ses = _many(plm, [reqs[0] * 1e3, second], slots=1, sampling=sp, seeds=[3, 9])
    assert ses.steps == 13 + 9
    assert torch.equal(out[1], alone)
    assert not torch.equal(out[0][:9], alone)


# ------------------------------------------------------------------------------------------------- 7. refusals
def test_session_refusals(device, plm):
    from megatts2_hierspeechpp_amd._lib import HspError
    ses = plm.decode_session(2, 10)
    tc = torch.zeros(256, 11, device=device)
    with pytest.raises(HspError):
        ses.admit(0, tc)                                                       # T > max_len
    with pytest.raises(HspError):
        ses.admit(0, tc[:, :0])                                                # T = 0
    with pytest.raises(HspError):
        ses.admit(2, tc[:, :4])                                                # no such slot
    ses.admit(0, tc[:, :4])
    with pytest.raises(HspError):
        ses.admit(0, tc[:, :4])                                                # busy
    with pytest.raises(HspError):
        ses.capture()                                                          # not with a busy slot
    for _ in range(4):
        assert ses.busy(0)
        ses.step()
    assert not ses.busy(0) and ses.codes_of(0).shape == (4,)
    ses.admit(0, tc[:, :10])                                                   # free again, and max_len itself fits
    for bad in (0, -1):
        with pytest.raises(HspError):
            plm.decode_session(bad, 10)                                        # slots < 1
        with pytest.raises(HspError):
            plm.infer_many([tc[:, :4]], slots=bad)
    with pytest.raises(HspError):
        plm.decode_session(2, plm.pos_emb.N_POS + 1)                           # max_len above the position table
    with pytest.raises(HspError):
        plm.decode_session(2, 0)
    with pytest.raises(HspError):
        plm.infer_many([tc[:, :4], tc[:, :0]], slots=2)                        # an empty request
    torch.cuda.synchronize()
