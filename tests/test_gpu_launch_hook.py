"""GPU: the measurement contract of hip_layers.LAUNCH_HOOK -- what bench.py's roofline pass and the launch-counting
parity tests are built on.  Every launch site of hip_layers runs once at the smallest shape that reaches it; the
records the hook receives are compared with a literal list (kind, flops, bytes, last argument), order included."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# (kind, flops, bytes, arg): arg is "Conv1dArgs" where the hook gets the launch's argument struct, else the value itself.
# The figures are the formulas of hip_layers worked out by hand for the shapes below, and equal what the hook reported
# before the launch sites were folded into one bracket.
CONV = (3145728, 114688)             # Conv1d 64 -> 64, k 3, B 2, L 64
FWD = ("hsp_dftseg_fwd_f32", 4194304, 364544, None)        # C 128, k 11, B 2, L 100: one segment per row, Np = 4
PROD = ("hsp_cprod3_f32", 25165824, 13107200, None)
INV = ("hsp_dftseg_inv_f32", 4194304, 466944, None)        # with a residual
WN_IN = (53084160, 1585152)          # WN 192, k 5, B 2, T 36: the gated in-conv
EXPECTED = [
    ("hsp_conv1d_mfma_f32",) + CONV + ("Conv1dArgs",),
    ("hsp_conv1d_direct_f32",) + CONV + ("Conv1dArgs",),
    ("hsp_conv1d_mfma_f32", 1048576, 65536, "Conv1dArgs"),      # ConvTranspose1d 64 -> 32, k 4, stride 2, L 32
    ("hsp_conv1d_mfma_f32", 7667712, 307200, "Conv1dArgs"),     # split_out: 192 -> 2 x 192, B 1, T 52
    # (the refused split_out launch reports nothing)
    FWD, PROD, INV, ("hsp_fftconv", 72089600, 1028096, None),
    FWD, PROD, ("hsp_dftseg_pair_f32", 8388608, 524288, None), PROD, INV, ("hsp_fftconv", 144179200, 1748992, 2),
    ("hsp_wn_layer_f32", WN_IN[0] + 2 * 5308416, WN_IN[1] + 313344 + 258048, "Conv1dArgs"),   # in, res, skip
    ("hsp_wn_layer_f32", WN_IN[0] + 5308416, WN_IN[1] + 313344, "Conv1dArgs"),                # last layer: in, skip (+=)
]


def _fill(mod, g):
    with torch.no_grad():
        for n, p_ in mod.named_parameters():
            if n.endswith("weight_g"):
                p_.copy_(0.3 + 0.4 * torch.rand(p_.shape, generator=g))
            else:
                p_.copy_(torch.randn(p_.shape, generator=g) * 0.1)


def test_every_launch_site_reports_once_and_the_hook_changes_no_bit(device, monkeypatch):
    from megatts2_hierspeechpp_amd import _lib as L, activations, hip_layers as HL, modules as M
    from megatts2_hierspeechpp_amd.alias_free_torch import Activation1d
    monkeypatch.setattr(HL, "SURVEY_ABI", False)
    monkeypatch.setattr(HL, "FFT_PRODUCT", "three")
    monkeypatch.setattr(M, "FOLD_MASK", True)
    g = torch.Generator().manual_seed(17)

    class Sites(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.conv = HL.Conv1d(64, 64, 3, padding=1)
            self.convtr = HL.ConvTranspose1d(64, 32, 4, 2, padding=1, weight_norm=True)
            self.split = HL.Conv1d(192, 384, 1, weight_norm=True)
            self.refused = HL.Conv1d(96, 192, 1, weight_norm=True)
            self.a1 = Activation1d(activation=activations.SnakeBeta(128, alpha_logscale=True))
            self.a2 = Activation1d(activation=activations.SnakeBeta(128, alpha_logscale=True))
            self.c1 = HL.Conv1d(128, 128, 11, padding=5, weight_norm=True)
            self.c2 = HL.Conv1d(128, 128, 11, padding=5, weight_norm=True)
            self.wn = M.WN(192, 5, 1, 2, gin_channels=0)

    m = Sites()
    _fill(m, g)
    m.c1.enable_fft()
    m.c2.enable_fft()
    HL.finalize(m, device)
    rnd = lambda *s: torch.randn(*s, generator=g).to(device)
    x64, x32, a192, r192, a96, x128, xw = rnd(2, 64, 64), rnd(2, 64, 32), rnd(1, 192, 52), rnd(1, 192, 52), \
        rnd(2, 96, 40), rnd(2, 128, 100), rnd(2, 192, 36)
    m52 = (torch.rand(1, 1, 52, generator=g) > 0.2).float().to(device)
    mw = (torch.rand(2, 1, 36, generator=g) > 0.2).float().to(device)
    assert m.c1.fft_pair_ok(m.c2, x128)

    def run():
        outs = [m.conv(x64), m.conv(x64, force_direct=True), m.convtr(x32)]
        outs += m.split(a192, res=r192, mask=m52, mask_mode=L.MASK_POST, split_out=(192, None, False))
        assert m.refused(a96, split_out=(96, None, False)) is None     # 96 rows: off the 64-row tile grid
        outs.append(m.c1.forward_fft(x128, act1d=m.a1, res=x128))
        outs.append(m.c1.forward_fft_pair(m.c2, x128, act_first=m.a1, act_second=m.a2, res=x128))
        monkeypatch.setattr(HL, "SURVEY_ABI", True)
        try:
            outs.append(m.wn(xw, mw))
        finally:
            monkeypatch.setattr(HL, "SURVEY_ABI", False)
        torch.cuda.synchronize()
        return [o.clone() for o in outs]

    rec = []
    monkeypatch.setattr(HL, "LAUNCH_HOOK", lambda *r: rec.append(r))
    hooked = run()
    monkeypatch.setattr(HL, "LAUNCH_HOOK", None)
    got = [(k, fl, nb, a if a is None or isinstance(a, int) else type(a).__name__) for k, fl, nb, _, _, a in rec]
    print(got)
    assert got == EXPECTED
    for k, _, _, e0, e1, _ in rec:
        assert e0.query() and e1.query(), k
        assert e0.elapsed_time(e1) >= 0.0, k
    n = len(rec)
    plain = run()
    assert len(rec) == n                                  # hook off: nothing is reported
    assert len(plain) == len(hooked) == 8
    for i, (p_, h_) in enumerate(zip(plain, hooked)):
        assert torch.equal(p_, h_), i


def test_a_prepared_launch_run_is_the_forward_call(device, monkeypatch):
    """Conv1d.prepare(x).run() is what forward(x) does: the same hook record, the same bits."""
    from megatts2_hierspeechpp_amd import hip_layers as HL
    monkeypatch.setattr(HL, "SURVEY_ABI", False)
    g = torch.Generator().manual_seed(23)
    conv = HL.Conv1d(64, 64, 3, padding=1)
    _fill(conv, g)
    HL.finalize(conv, device)
    x = torch.randn(2, 64, 64, generator=g).to(device)
    rec = []
    monkeypatch.setattr(HL, "LAUNCH_HOOK", lambda *r: rec.append(r))
    p = conv.prepare(x)
    assert rec == []                                      # prepared, not issued
    assert p.run() == 0
    y = conv(x)
    torch.cuda.synchronize()
    got = [(k, fl, nb, type(a).__name__) for k, fl, nb, _, _, a in rec]
    assert got == [EXPECTED[0], EXPECTED[0]], got
    assert y.data_ptr() != p.out.data_ptr() and torch.equal(p.out, y) and bool(y.abs().sum() > 0)
