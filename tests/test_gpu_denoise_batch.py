"""GPU (-m gpu): the batched prompt denoiser.  The packed-layout kernels through the C ABI against
float64 numpy or the same launch on a row alone, the packed network against the network on each row alone, ``denoise_batch`` against
the oracle, the silent row, the capture with no read-back, and the wiring into prompt_mels / vc_batch."""
import ctypes as C

import numpy as np
import pytest
import torch

import denoise_batch_inputs as DI
import helpers as H

pytestmark = pytest.mark.gpu

CANARY = 7.25
SEGS = [(0, 4), (12, 10), (30, 1)]
T_TOT = 40


def _close(got, ref, what):
    err = float(np.abs(got - ref).max())
    print(f"{what}: max err {err:.3e} (tol {H.tol_for(ref):.3e})")
    assert err <= H.tol_for(ref), (what, err, H.tol_for(ref))


def _phase_close(got, ref, ref_mag, what):
    keep = DI.solid(ref_mag)
    assert keep.mean() > 0.5, (what, float(keep.mean()))
    err = float(DI.circular(got, ref)[keep].max())
    print(f"{what}: max circular err {err:.3e} on {keep.mean():.2f} of the bins (tol {H.tol_for(ref):.3e})")
    assert err <= H.tol_for(ref), (what, err)


class _Table:
    """A hand-made segment table (first row, T_b) on both sides."""

    def __init__(self, pairs, device):
        flat = [v for p in pairs for v in p]
        self.host = (C.c_int32 * len(flat))(*flat)
        self.dev = torch.tensor(flat, dtype=torch.int32).to(device)
        self.B = len(pairs)

    def args(self):
        return self.dev.data_ptr(), C.cast(self.host, C.c_void_p), self.B


def _guarded(n, device):
    """n floats with 64 canary values on either side -> (whole buffer, the n-float view)."""
    buf = torch.full((n + 128,), CANARY, dtype=torch.float32, device=device)
    return buf, buf[64:64 + n]


def _canaries_intact(buf):
    return bool((buf[:64] == CANARY).all()) and bool((buf[-64:] == CANARY).all())


# ------------------------------------------------------------------------------------------ kernels, C ABI
@pytest.mark.parametrize("Cc", [1, 64])
def test_segmented_instnorm_against_float64(device, Cc):
    from megatts2_hierspeechpp_amd import _lib as L
    F_, pitch = 5, T_TOT * 5 + 3                    # planes 3 floats apart: the pitch holds canaries too
    r = np.random.default_rng(Cc)
    x = np.full((Cc, pitch), CANARY, np.float32)
    body = (r.standard_normal((Cc, T_TOT, F_)) * 2.0 + 0.5).astype(np.float32)
    valid = np.zeros(T_TOT, bool)
    for s, n in SEGS:
        valid[s:s + n] = True
    body[:, ~valid] = np.nan                          # gap rows: never read, written as exact zeros
    x[:, :T_TOT * F_] = body.reshape(Cc, -1)
    g, b, sl = (r.uniform(0.5, 1.5, Cc).astype(np.float32), r.standard_normal(Cc).astype(np.float32),
                r.uniform(0.05, 0.4, Cc).astype(np.float32))
    buf, xv = _guarded(Cc * pitch, device)
    xv.copy_(torch.from_numpy(x.reshape(-1)))
    tab = _Table(SEGS, device)
    d = lambda a: torch.from_numpy(a).to(device)
    dg, db, dsl = d(g), d(b), d(sl)
    L.check(L.lib().hsp_instnorm_prelu_seg_f32(xv.data_ptr(), pitch, Cc, T_TOT, F_, *tab.args(), dg.data_ptr(), db.data_ptr(),
                                               dsl.data_ptr(), 1e-5, L.stream_ptr()), "hsp_instnorm_prelu_seg_f32")
    got = xv.cpu().numpy().reshape(Cc, pitch)
    assert _canaries_intact(buf) and (got[:, T_TOT * F_:] == CANARY).all()
    got = got[:, :T_TOT * F_].reshape(Cc, T_TOT, F_)
    assert (got[:, ~valid] == 0.0).all() and not np.signbit(got[:, ~valid]).any()
    want = np.zeros((Cc, T_TOT, F_))
    for s, n in SEGS:
        v = body[:, s:s + n].astype(np.float64)
        m, var = v.mean((1, 2), keepdims=True), v.var((1, 2), keepdims=True)
        y = (v - m) / np.sqrt(var + 1e-5) * g[:, None, None] + b[:, None, None]
        want[:, s:s + n] = np.where(y > 0, y, sl[:, None, None] * y)
    # four fp32 roundings (difference, two products, sum) on values of the output's size: a few 2^-24 relative
    err = np.abs(got - want).max()
    assert err <= 4e-6 * max(1.0, np.abs(want).max()), err


def test_bounded_dwconv_against_float64(device):
    from megatts2_hierspeechpp_amd import _lib as L
    A, Cc, K = 2, 3, 31
    r = np.random.default_rng(31)
    x = r.standard_normal((A, Cc, T_TOT)).astype(np.float32)
    valid = np.zeros(T_TOT, bool)
    for s, n in SEGS:
        valid[s:s + n] = True
    x[:, :, ~valid] = np.nan
    p = {k: v.astype(np.float32) for k, v in dict(
        w=r.standard_normal((Cc, K)) * 0.3, bias=r.standard_normal(Cc), bw=r.uniform(0.5, 1.5, Cc), bb=r.standard_normal(Cc),
        bm=r.standard_normal(Cc) * 0.2, bv=r.uniform(0.5, 2.0, Cc)).items()}
    d = {k: torch.from_numpy(v).to(device) for k, v in p.items()}
    dx = torch.from_numpy(x).to(device)
    buf, y = _guarded(A * Cc * T_TOT, device)
    tab = _Table(SEGS, device)
    L.check(L.lib().hsp_dwconv_bn_silu_seg_f32(dx.data_ptr(), d["w"].data_ptr(), d["bias"].data_ptr(), d["bw"].data_ptr(),
                                               d["bb"].data_ptr(), d["bm"].data_ptr(), d["bv"].data_ptr(), 1e-5, y.data_ptr(),
                                               A, Cc, T_TOT, K, *tab.args(), L.stream_ptr()), "hsp_dwconv_bn_silu_seg_f32")
    got = y.cpu().numpy().reshape(A, Cc, T_TOT)
    assert _canaries_intact(buf)
    assert (got[:, :, ~valid] == 0.0).all()
    want = np.zeros((A, Cc, T_TOT))
    for s, n in SEGS:
        seg = np.pad(x[:, :, s:s + n].astype(np.float64), ((0, 0), (0, 0), (K // 2, K // 2)))   # the solo call's zero padding
        for t in range(n):
            acc = (seg[:, :, t:t + K] * p["w"][None].astype(np.float64)).sum(-1) + p["bias"]
            alpha = p["bw"] / np.sqrt(p["bv"].astype(np.float64) + 1e-5)
            v = acc * alpha + (p["bb"] - p["bm"] * alpha)
            want[:, :, s + t] = v / (1.0 + np.exp(-v))
    # 31 fused multiply-adds of O(1) terms in fp32, then the affine map and SiLU: tens of 2^-24 relative
    err = np.abs(got - want).max()
    assert np.isfinite(got).all() and err <= 1e-5 * max(1.0, np.abs(want).max()), err


def test_packed_framing_bit_equal_to_solo_rows(device):
    from megatts2_hierspeechpp_amd import _lib as L
    from megatts2_hierspeechpp_amd.denoiser.packed import Segments
    lens = [300, 900, 8000]
    n_fft, hop = 400, 100
    seg = Segments([1 + n // hop for n in lens], device)
    f_ld = (seg.T_tot + 3) & ~3
    xs = torch.zeros(3, 8000, dtype=torch.float32, device=device)
    for b, n in enumerate(lens):
        xs[b, :n] = torch.from_numpy(DI.tone_row(n, 40 + b)).to(device)
        xs[b, n:] = float("nan")                       # past a row's end: never read
    win = torch.hann_window(n_fft, periodic=True, dtype=torch.float32).to(device)
    dlen = torch.tensor(lens, dtype=torch.int64).to(device)
    buf, fr = _guarded(n_fft * f_ld, device)
    L.check(L.lib().hsp_stft_frames_packed_f32(xs.data_ptr(), xs.stride(0), dlen.data_ptr(), None, win.data_ptr(),
                                               fr.data_ptr(), *seg.args(), 8000, n_fft, hop, seg.T_tot, f_ld,
                                               L.stream_ptr()), "hsp_stft_frames_packed_f32")
    got = fr.reshape(n_fft, f_ld)
    assert _canaries_intact(buf)
    keep = torch.zeros(f_ld, dtype=torch.bool, device=device)
    for b, (n, sl) in enumerate(zip(lens, seg.slices())):
        T = seg.frames[b]
        solo = torch.empty(1, n_fft, T, dtype=torch.float32, device=device)
        row = xs[b, :n].contiguous()
        L.check(L.lib().hsp_stft_frames_f32(row.data_ptr(), win.data_ptr(), solo.data_ptr(), 1, n, n_fft, hop, T, T,
                                            L.stream_ptr()), "hsp_stft_frames_f32")
        assert torch.equal(got[:, sl], solo[0]), b
        keep[sl] = True
    assert not got[:, ~keep].any()                     # gap and pitch columns: zeros
    # with a scale: the frames of the scaled row
    sc = torch.tensor([0.5, 3.0, 1.25], dtype=torch.float32).to(device)
    L.check(L.lib().hsp_stft_frames_packed_f32(xs.data_ptr(), xs.stride(0), dlen.data_ptr(), sc.data_ptr(), win.data_ptr(),
                                               fr.data_ptr(), *seg.args(), 8000, n_fft, hop, seg.T_tot, f_ld,
                                               L.stream_ptr()), "hsp_stft_frames_packed_f32")
    for b, (n, sl) in enumerate(zip(lens, seg.slices())):
        T = seg.frames[b]
        solo = torch.empty(1, n_fft, T, dtype=torch.float32, device=device)
        row = (xs[b, :n] * sc[b]).contiguous()
        L.check(L.lib().hsp_stft_frames_f32(row.data_ptr(), win.data_ptr(), solo.data_ptr(), 1, n, n_fft, hop, T, T,
                                            L.stream_ptr()), "hsp_stft_frames_f32")
        assert torch.equal(got[:, sl], solo[0]), b


def test_segmented_overlap_add_bit_equal_to_solo_rows(device):
    """A row of the batch equals the same launch on that row's frames alone (a one-segment table), bit for bit; and
    every row equals a float64 overlap-add of the same fp32 frames and window: at most four window-weighted terms per
    sum, one divide and one multiply, so 16 roundings of 2^-24 on sum_t |frames w| / den |inv| bound the error."""
    from megatts2_hierspeechpp_amd import _lib as L
    from megatts2_hierspeechpp_amd.denoiser.packed import Segments
    n_fft, hop = 400, 100
    seg = Segments([4, 1, 10, 81], device)             # a one-frame row holds no sample: zeros
    f_ld = (seg.T_tot + 3) & ~3
    g = torch.Generator().manual_seed(3)
    frames = torch.randn(n_fft, f_ld, generator=g).to(device)
    win = torch.hann_window(n_fft, periodic=True, dtype=torch.float32).to(device)
    n_max, pitch = hop * 80, hop * 80 + 5
    buf, out = _guarded(4 * pitch, device)

    def alone(b, inv):
        """The launch on row b's frames alone: one segment (0, T), frames [n_fft, T], output [hop (T - 1)]."""
        T = seg.frames[b]
        n = hop * (T - 1)
        own = frames[:, seg.slices()[b]].contiguous()
        one = Segments([T], device)
        solo = torch.empty(n, dtype=torch.float32, device=device)
        L.check(L.lib().hsp_istft_ola_seg_f32(own.data_ptr(), T, win.data_ptr(), None if inv is None else inv.data_ptr(),
                                              solo.data_ptr(), n, n, n_fft, hop, *one.args(), T, L.stream_ptr()),
                "hsp_istft_ola_seg_f32")
        return solo

    fr64, w64 = frames.cpu().numpy().astype(np.float64), win.cpu().numpy().astype(np.float64)

    def against_float64(got, inv):
        for b, sl in enumerate(seg.slices()):
            T = seg.frames[b]
            n = hop * (T - 1)
            num, mass, den = np.zeros(n), np.zeros(n), np.zeros(n)
            k = np.arange(n_fft)
            for t in range(T):
                at = k + t * hop - n_fft // 2          # frame t, tap k lands on sample k + t hop - n_fft / 2
                ok = (at >= 0) & (at < n)
                term = fr64[k[ok], sl.start + t] * w64[k[ok]]
                num[at[ok]] += term
                mass[at[ok]] += np.abs(term)
                den[at[ok]] += w64[k[ok]] ** 2
            want = num / den * inv[b]
            tol = 16 * 2.0 ** -24 * mass / den * abs(inv[b])
            err = np.abs(got[b, :n].cpu().numpy().astype(np.float64) - want)
            worst = float((err / np.maximum(tol, 1e-300)).max()) if n else 0.0
            print(f"overlap-add row {b} (T = {T}, inv {inv[b]}): worst err / tol {worst:.3f}")
            assert (err <= tol).all(), (b, worst)

    L.check(L.lib().hsp_istft_ola_seg_f32(frames.data_ptr(), f_ld, win.data_ptr(), None, out.data_ptr(), pitch, n_max, n_fft,
                                          hop, *seg.args(), seg.T_tot, L.stream_ptr()), "hsp_istft_ola_seg_f32")
    got = out.reshape(4, pitch)
    assert _canaries_intact(buf) and bool((got[:, n_max:] == CANARY).all())
    for b in range(4):
        T = seg.frames[b]
        n = hop * (T - 1)
        if T >= 2:
            assert torch.equal(got[b, :n], alone(b, None)), b
        assert not got[b, n:n_max].any(), b
    against_float64(got, [1.0, 1.0, 1.0, 1.0])
    # with inverse scales: the row alone at that scale
    scales = [2.0, 1.0, 0.0, 0.37]
    inv = torch.tensor(scales, dtype=torch.float32).to(device)
    L.check(L.lib().hsp_istft_ola_seg_f32(frames.data_ptr(), f_ld, win.data_ptr(), inv.data_ptr(), out.data_ptr(), pitch,
                                          n_max, n_fft, hop, *seg.args(), seg.T_tot, L.stream_ptr()), "hsp_istft_ola_seg_f32")
    assert torch.equal(got[3, :n_max], alone(3, inv[3:4])) and not got[2, :n_max].any()
    assert torch.equal(got[0, :hop * 3], alone(0, inv[0:1]))
    against_float64(got, [float(v) for v in inv.cpu()])


def test_norm_factor_rows_against_numpy(device):
    from megatts2_hierspeechpp_amd import _lib as L
    lens = [300, 900, 8000, 5137]
    xs = np.full((4, 8003), np.nan, np.float32)        # past a row's end: never read
    for b, n in enumerate(lens):
        xs[b, :n] = DI.tone_row(n, 60 + b)
    xs[1, :900] = 0.0                                   # a silent row
    dx = torch.from_numpy(xs).to(device)
    dlen = torch.tensor(lens, dtype=torch.int64).to(device)
    buf, out = _guarded(8, device)
    L.check(L.lib().hsp_norm_factor_rows_f32(dx.data_ptr(), dx.stride(0), dlen.data_ptr(), out[:4].data_ptr(),
                                             out[4:].data_ptr(), 4, 8003, L.stream_ptr()), "hsp_norm_factor_rows_f32")
    got = out.cpu().numpy().astype(np.float64)
    assert _canaries_intact(buf)
    for b, n in enumerate(lens):
        ss = float((xs[b, :n].astype(np.float64) ** 2).sum())
        if ss == 0.0:
            assert got[b] == 0.0 and got[4 + b] == 0.0
            continue
        want = np.sqrt(n / ss)
        # the sum is exact to fp32 (double accumulation), then one rounding of the factor: 2^-23 relative
        assert abs(got[b] / want - 1.0) <= 2.0 ** -22 and abs(got[4 + b] * want - 1.0) <= 2.0 ** -22, b


# ------------------------------------------------------------------------------------------ the network
@pytest.fixture(scope="module")
def net(device):
    from megatts2_hierspeechpp_amd.hip_layers import finalize
    meta, _ = H.load_fixture("denoise_l8000")
    mod = H.build_module(meta)
    mod.load_state_dict(H.synth_sd(meta), strict=True)
    finalize(mod, device)
    return mod


@pytest.fixture(scope="module")
def vc_setup(device):
    return DI.vc_models(device)


@pytest.fixture(scope="module")
def solo(device, net):
    """Per prompt, computed once: the waveform, the (mag, pha) the solo path feeds the network -- the fixture's own
    ``amp_in`` / ``pha_in`` for the two golden rows, the product STFT for the synthetic ones -- and the solo network's
    outputs on them."""
    from megatts2_hierspeechpp_amd.denoiser.infer import mag_pha_stft
    out = {}
    for n, wav in zip(DI.LENGTHS, DI.rows()):
        w = torch.from_numpy(wav).to(device)
        if n in DI.FIXTURES:
            arrays = H.load_fixture(DI.FIXTURES[n])[1]
            mag, pha = torch.from_numpy(arrays["amp_in"]).to(device), torch.from_numpy(arrays["pha_in"]).to(device)
        else:
            norm = float(np.sqrt(n / float((wav.astype(np.float64) ** 2).sum())))
            mag, pha, _ = mag_pha_stft((w * norm).unsqueeze(0), 400, 100, 400, 0.3)
        out[n] = dict(wav=w, mag=mag, pha=pha, net=[t.clone() for t in net(mag, pha)])
    return out


@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_packed_network_equals_solo_network(device, net, solo, order):
    """A short row once behind and once ahead of a long one: every row of the packed pass against the network on that
    row alone, given the same (mag, pha); the golden rows also against the oracle and the goldens' ``out1``."""
    from oracle import hsp_oracle as O
    lens = DI.LENGTHS if order == "ascending" else DI.LENGTHS[::-1]
    frames = [1 + n // 100 for n in lens]
    Tm = max(frames)
    mag = torch.zeros(4, 201, Tm, device=device)
    pha = torch.zeros(4, 201, Tm, device=device)
    for b, n in enumerate(lens):
        mag[b, :, :frames[b]] = solo[n]["mag"][0]
        pha[b, :, :frames[b]] = solo[n]["pha"][0]
    d_mag, d_pha, d_com = net(mag, pha, frames)
    assert d_mag.shape == d_pha.shape == (4, 201, Tm) and d_com.shape == (4, 201, Tm, 2)
    for b, n in enumerate(lens):
        T = frames[b]
        rm, rp, rc = (t.cpu().numpy() for t in solo[n]["net"])
        gm, gp, gc = d_mag[b:b + 1, :, :T].cpu().numpy(), d_pha[b:b + 1, :, :T].cpu().numpy(), d_com[b:b + 1, :, :T].cpu().numpy()
        _close(gm, rm, f"{order} row {n}: magnitude vs solo")
        _phase_close(gp, rp, rm, f"{order} row {n}: phase vs solo")
        _close(gc, rc, f"{order} row {n}: complex vs solo")
        assert not d_mag[b, :, T:].any() and not d_pha[b, :, T:].any() and not d_com[b, :, T:].any(), n
        if n in DI.FIXTURES and order == "ascending":
            meta, arrays = H.load_fixture(DI.FIXTURES[n])
            _, amp_o, pha_o = O.denoise(H.oracle_sd(meta), meta["prefix"], torch.from_numpy(arrays["wav"]),
                                        spectrogram=(torch.from_numpy(arrays["amp_in"]), torch.from_numpy(arrays["pha_in"])))
            _close(gm, amp_o.numpy(), f"row {n}: magnitude vs oracle")
            _phase_close(gp, pha_o.numpy(), amp_o.numpy(), f"row {n}: phase vs oracle")
            _close(gm, arrays["out1"], f"row {n}: magnitude vs golden out1")
    assert bool(torch.isfinite(d_mag).all()) and bool(torch.isfinite(d_pha).all())


def test_mpnet_refuses_device_lengths(device, net):
    from megatts2_hierspeechpp_amd import _lib as L
    z = torch.zeros(2, 201, 10, device=device)
    with pytest.raises(L.HspError):
        net(z, z, torch.tensor([10, 4], device=device))
    with pytest.raises(L.HspError):
        net(z, z)                                      # without lengths: one utterance, as before
    with pytest.raises(L.HspError):
        net(z, z, [10, 11])


def test_one_prompt_is_the_one_segment_batch(device, net):
    """``denoise`` / ``net(mag, pha)`` are the packed pass on a table of one row: bit-equal to the batch of one, at 4
    frames (below every T dilation of the dense blocks), 10 (across dilation 8) and 81 (a golden row)."""
    from megatts2_hierspeechpp_amd import _lib as L
    from megatts2_hierspeechpp_amd.denoiser.infer import denoise, denoise_batch, mag_pha_stft
    for n in (300, 900, 8000):
        w = torch.from_numpy(DI.row(n)).to(device)
        T = 1 + n // 100
        one = denoise(w, net, H.DENOISER_H)
        many, n_out = denoise_batch([w], net, H.DENOISER_H)
        assert one.shape == (1, 100 * (T - 1)) and n_out == [100 * (T - 1)]
        assert torch.equal(one[0], many[0, :n_out[0]]), n
        mag, pha, _ = mag_pha_stft(w.unsqueeze(0), 400, 100, 400, 0.3)
        for a_, b_ in zip(net(mag, pha), net(mag, pha, [T])):
            assert a_.shape == b_.shape and torch.equal(a_, b_), n
    with pytest.raises(L.HspError):
        denoise(torch.zeros(900, device=device), net, H.DENOISER_H)


# ------------------------------------------------------------------------------------------ end to end
def test_denoise_batch_end_to_end(device, net, solo):
    """Each row against the oracle fed the batch's own spectrogram of that row (the method of test_denoise_end_to_end);
    that spectrogram against the solo mag_pha_stft; lengths and the zeros past each row's end."""
    from oracle import hsp_oracle as O
    from megatts2_hierspeechpp_amd.denoiser.infer import denoise_batch, mag_pha_stft
    meta, _ = H.load_fixture("denoise_l8000")
    sd = H.oracle_sd(meta)
    wavs = [solo[n]["wav"] for n in DI.LENGTHS]
    out, out_len, (mag, pha) = denoise_batch(wavs, net, H.DENOISER_H, return_spectrogram=True)
    assert out_len == [100 * (n // 100) for n in DI.LENGTHS] and out.shape == (4, max(out_len))
    assert mag.shape == pha.shape == (4, 201, 145)
    for b, n in enumerate(DI.LENGTHS):
        T = 1 + n // 100
        w = wavs[b].cpu()
        norm = torch.sqrt(len(w) / torch.sum(w ** 2.0))
        sm, sp, _ = mag_pha_stft((w * norm).unsqueeze(0).to(device), 400, 100, 400, 0.3)
        gm, gp = mag[b:b + 1, :, :T].cpu(), pha[b:b + 1, :, :T].cpu()
        _close(gm.numpy(), sm.cpu().numpy(), f"row {n}: batch spectrogram magnitude vs solo")
        _phase_close(gp.numpy(), sp.cpu().numpy(), sm.cpu().numpy(), f"row {n}: batch spectrogram phase vs solo")
        assert not mag[b, :, T:].any() and not pha[b, :, T:].any()
        ref, _, _ = O.denoise(sd, meta["prefix"], w, spectrogram=(gm, gp))
        assert ref.shape == (1, out_len[b])
        _close(out[b:b + 1, :out_len[b]].cpu().numpy(), ref.numpy(), f"row {n}: denoise_batch vs oracle")
        assert not out[b, out_len[b]:].any()
    # the padded-tensor form and the sub-batch split give the same rows
    padded = torch.zeros(4, 14400, device=device)
    for b, n in enumerate(DI.LENGTHS):
        padded[b, :n] = wavs[b]
    out2, len2 = denoise_batch(padded, net, H.DENOISER_H, lengths=DI.LENGTHS)
    assert len2 == out_len and torch.equal(out2, out)
    out3, len3 = denoise_batch(wavs, net, H.DENOISER_H, max_rows=100)      # [300, 900] | [8000] | [14400]
    assert len3 == out_len and out3.shape == out.shape
    _close(out3.cpu().numpy(), out.cpu().numpy(), "sub-batches vs one batch")


def test_stft_and_istft_batch_match_solo_rows(device, solo):
    """The two public spectrogram functions on the four rows, unscaled, against mag_pha_stft / mag_pha_istft per row."""
    from megatts2_hierspeechpp_amd.denoiser.infer import mag_pha_istft, mag_pha_istft_batch, mag_pha_stft, mag_pha_stft_batch
    y = torch.zeros(4, 14400, device=device)
    for b, n in enumerate(DI.LENGTHS):
        y[b, :n] = solo[n]["wav"]
    mag, pha, com = mag_pha_stft_batch(y, DI.LENGTHS, 400, 100, 400, 0.3)
    frames = [1 + n // 100 for n in DI.LENGTHS]
    assert mag.shape == pha.shape == (4, 201, 145) and com.shape == (4, 201, 145, 2)
    wav, out_len = mag_pha_istft_batch(mag, pha, frames, 400, 100, 400, 0.3)
    assert out_len == [100 * (t - 1) for t in frames] and wav.shape == (4, 14400)
    for b, n in enumerate(DI.LENGTHS):
        T = frames[b]
        sm, sp, sc = mag_pha_stft(solo[n]["wav"].unsqueeze(0), 400, 100, 400, 0.3)
        _close(mag[b:b + 1, :, :T].cpu().numpy(), sm.cpu().numpy(), f"row {n}: stft batch magnitude")
        _phase_close(pha[b:b + 1, :, :T].cpu().numpy(), sp.cpu().numpy(), sm.cpu().numpy(), f"row {n}: stft batch phase")
        _close(com[b:b + 1, :, :T].cpu().numpy(), sc.cpu().numpy(), f"row {n}: stft batch complex")
        assert not mag[b, :, T:].any() and not pha[b, :, T:].any() and not com[b, :, T:].any()
        back = mag_pha_istft(mag[b:b + 1, :, :T].contiguous(), pha[b:b + 1, :, :T].contiguous(), 400, 100, 400, 0.3)
        _close(wav[b:b + 1, :out_len[b]].cpu().numpy(), back.cpu().numpy(), f"row {n}: istft batch")
        assert not wav[b, out_len[b]:].any()
        # the round trip returns the waveform (hop-aligned part; the window envelope is exact for Hann at hop = N / 4)
        _close(wav[b, :out_len[b]].cpu().numpy(), solo[n]["wav"][:out_len[b]].cpu().numpy(), f"row {n}: round trip")
    sc3 = torch.tensor([2.0, 0.5, 1.0, 3.0], device=device)
    mag_s, _, _ = mag_pha_stft_batch(y, DI.LENGTHS, 400, 100, 400, 0.3, scale=sc3)
    m1, _, _ = mag_pha_stft((solo[900]["wav"] * 0.5).unsqueeze(0), 400, 100, 400, 0.3)
    _close(mag_s[1:2, :, :10].cpu().numpy(), m1.cpu().numpy(), "scaled row 900")


def test_silent_row_comes_out_as_zeros(device, net, solo):
    from megatts2_hierspeechpp_amd.denoiser.infer import denoise_batch
    loud = solo[8000]["wav"]
    out, n = denoise_batch([torch.zeros(900, device=device), loud], net, H.DENOISER_H)
    alone, n1 = denoise_batch([loud], net, H.DENOISER_H)
    assert n == [900, 8000] and n1 == [8000]
    assert bool(torch.isfinite(out).all()) and not out[0].any()
    _close(out[1:2].cpu().numpy(), alone.cpu().numpy(), "the loud row beside a silent one")


def test_denoise_batch_captures_with_no_read_back(device, net):
    """One eager call, ONE capture, ONE replay on new prompt contents of the same lengths."""
    from megatts2_hierspeechpp_amd.denoiser.infer import denoise_batch
    lens = [900, 8000]
    x = torch.zeros(2, 8000, device=device)
    for b, n in enumerate(lens):
        x[b, :n] = torch.from_numpy(DI.tone_row(n, 70 + b)).to(device)
    run = lambda: denoise_batch(x, net, H.DENOISER_H, lengths=lens)[0]
    run()
    torch.cuda.synchronize()
    from megatts2_hierspeechpp_amd.denoiser import packed
    frames = [1 + n // 100 for n in lens]
    kept = packed.segments_for(frames, device)                       # the eager call's table, from the cache
    assert packed.segments_for(frames, device) is kept
    keys = set(packed._CACHE)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = run()
        inside = packed.segments_for(frames, device)
    # a capture neither reads nor fills the cache: its tables live in the graph's own pool, so evicting the cache
    # leaves the graph intact
    assert inside is not kept and inside.dev.data_ptr() != kept.dev.data_ptr() and set(packed._CACHE) == keys
    del kept, inside
    packed._CACHE.clear()
    junk = torch.full((1 << 20,), -7, dtype=torch.int32, device=device)  # noqa: F841  (takes freed blocks, were there any)
    for b, n in enumerate(lens):
        x[b, :n] = torch.from_numpy(DI.tone_row(n, 80 + b)).to(device)
    g.replay()
    torch.cuda.synchronize()
    replayed = captured.clone()
    eager = run()
    assert bool(replayed.any()) and torch.equal(replayed, eager)


# ------------------------------------------------------------------------------------------ wiring
def test_denoise_prompts_matches_pad_denoise_cut(device, net):
    from megatts2_hierspeechpp_amd import inference_vc as IV
    from megatts2_hierspeechpp_amd.denoiser.infer import denoise
    prompts = [torch.from_numpy(DI.tone_row(n, n)).to(device) for n in (5000, 37777)]
    got = IV.denoise_prompts([prompts[0], prompts[1].reshape(1, -1)], net, H.DENOISER_H)
    for p, g_ in zip(prompts, got):
        n = p.shape[0]
        padded = torch.zeros((n // 1600 + 1) * 1600, device=device)
        padded[:n] = p
        want = denoise(padded, net, H.DENOISER_H)[:, :padded.shape[0]][0, :n]
        assert g_.shape == (n,)
        _close(g_.cpu().numpy(), want.cpu().numpy(), f"denoise_prompts at {n}")


def test_prompt_mels_two_prompts_match_two_calls(device, net, vc_setup):
    from megatts2_hierspeechpp_amd import inference_plm as IP
    _, mel_fn = vc_setup
    audio = torch.stack([torch.from_numpy(DI.tone_row(6000, s)).to(device) for s in (1, 2)])
    ttv2, mel2 = IP.prompt_mels(mel_fn, audio, net, H.DENOISER_H)
    assert mel2.shape[0] == 4 and ttv2.shape[0] == 2
    for b in range(2):
        ttv1, mel1 = IP.prompt_mels(mel_fn, audio[b:b + 1], net, H.DENOISER_H)
        _close(ttv2[b:b + 1].cpu().numpy(), ttv1.cpu().numpy(), f"padded prompt mel {b}")
        _close(mel2[b:b + 1].cpu().numpy(), mel1[:1].cpu().numpy(), f"prompt mel {b}")
        _close(mel2[2 + b:3 + b].cpu().numpy(), mel1[1:].cpu().numpy(), f"denoised prompt mel {b}")


def test_vc_batch_with_a_denoiser(device, net, vc_setup):
    from megatts2_hierspeechpp_amd import _lib as L, inference_vc as IV
    models, mel_fn = vc_setup
    srcs, f0s, prompts, f0t = DI.vc_case(device, [12000, 9000], [8000, 5000], 11)
    T = max(s.shape[-1] for s in srcs) // 320
    noise = torch.from_numpy(np.random.default_rng(4).standard_normal((2, 192, T)).astype(np.float32)).to(device)
    kw = dict(noise=noise, denoise_ratio=0.8)
    den = IV.denoise_prompts(prompts, net, H.DENOISER_H)
    want, n_want = IV.vc_batch(models, mel_fn, srcs, f0s, prompts, f0t, denoised=den, **kw)
    got, n_got = IV.vc_batch(models, mel_fn, srcs, f0s, prompts, f0t, denoiser=net, hps_denoiser=H.DENOISER_H, **kw)
    assert torch.equal(got, want) and torch.equal(n_got, n_want)
    plain, _ = IV.vc_batch(models, mel_fn, srcs, f0s, prompts, f0t, noise=noise)
    assert not torch.equal(plain, got)                 # the denoised style vector took part
    with pytest.raises(L.HspError):
        IV.vc_batch(models, mel_fn, srcs, f0s, prompts, f0t, denoised=den, denoiser=net, hps_denoiser=H.DENOISER_H, **kw)
    with pytest.raises(L.HspError):
        IV.vc_batch(models, mel_fn, srcs, f0s, prompts, f0t, **kw)
    from megatts2_hierspeechpp_amd.denoiser.infer import denoise_batch
    with pytest.raises(L.HspError):                    # lengths that exist only on the device
        denoise_batch(torch.zeros(2, 6000, device=device), net, H.DENOISER_H,
                      lengths=torch.tensor([6000, 6000], device=device))
