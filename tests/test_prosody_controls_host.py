"""CPU: properties of the float64 restatement of the pitch edit and the scaled durations (tests/f0_edit_ref.py), every
message of `PitchEdit.check`, the width error of ``lf0=``, the range error of the pace scales, the new keywords'
defaults in every harness signature, the agreement of header, binding and struct layout, and the argument checks of the
two new entry points (they reject before any HIP call, so they run here on dummy pointers)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import f0_edit_ref as R
import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hsp_f0_edit_rows_f32", "hsp_duration_scaled_f32")


def _rows(n=300):
    return np.stack([R.track(n, 1), R.track(n, 2, centre_hz=230.0), R.track(n, 3, voiced=0.3)])


# ------------------------------------------------------------------------------------------ the reference's properties
def test_identity_row_is_copied():
    l = _rows()
    out, mean = R.edit_rows(l)
    assert np.array_equal(out, l.astype(np.float64))
    out, _ = R.edit_rows(l, lengths=[300, 120, 0])
    assert np.array_equal(out[1, :120], l[1, :120]) and not out[1, 120:].any() and not out[2].any()
    hz = R.l_to_hz(l[0][l[0] > 0])
    assert abs(mean[0] - np.exp(np.log(hz).mean())) <= 1e-4 * mean[0]      # the geometric mean (fp32 track: 1e-7 relative)
    # offsets of zeros are NOT the identity rule, but give the same track up to rounding
    near, _ = R.edit_rows(l, offsets=np.zeros_like(l))
    assert np.abs(near - l).max() <= 1e-12


def test_shift_12_doubles_every_voiced_hz():
    l = _rows()
    out, _ = R.edit_rows(l, shift=[12.0] * 3, f_max=5000.0)
    v = l > 0
    assert np.abs(R.l_to_hz(out[v]) / R.l_to_hz(l[v]) - 2.0).max() <= 1e-12
    assert np.array_equal(out > 0, v)
    down, _ = R.edit_rows(l, shift=[-12.0] * 3, f_min=10.0)
    assert np.abs(R.l_to_hz(down[v]) / R.l_to_hz(l[v]) - 0.5).max() <= 1e-12


def test_range_0_puts_every_voiced_frame_at_the_geometric_mean():
    l = _rows()
    out, mean = R.edit_rows(l, range_=[0.0] * 3)
    for b in range(3):
        v = l[b] > 0
        assert np.abs(R.l_to_hz(out[b][v]) / mean[b] - 1.0).max() <= 1e-12
    wide, _ = R.edit_rows(l, range_=[2.0] * 3, f_min=1.0, f_max=1e5)
    for b in range(3):
        v = l[b] > 0
        p, q = np.log(R.l_to_hz(l[b][v])), np.log(R.l_to_hz(wide[b][v]))
        assert np.abs((q - q.mean()) - 2.0 * (p - p.mean())).max() <= 1e-10


def test_target_becomes_the_geometric_mean_when_nothing_clamps():
    l = _rows()
    out, _ = R.edit_rows(l, target_hz=[200.0, 120.0, 0.0])
    for b, want in enumerate((200.0, 120.0)):
        hz = R.l_to_hz(out[b][l[b] > 0])
        assert 55.0 < hz.min() and hz.max() < 1100.0                       # nothing clamped
        assert abs(np.exp(np.log(hz).mean()) / want - 1.0) <= 1e-12
    assert np.array_equal(out[2], l[2].astype(np.float64))                 # no target and nothing else: an identity row


def test_unvoiced_frames_and_the_tail_are_zero():
    l = _rows()
    off = np.random.default_rng(4).uniform(-3, 3, l.shape).astype(np.float32)
    out, _ = R.edit_rows(l, lengths=[250, 300, 7], shift=[3.0, -2.0, 1.0], range_=[1.5, 0.5, 1.0], offsets=off)
    for b, n_b in enumerate((250, 300, 7)):
        assert not out[b, n_b:].any()
        assert np.array_equal(out[b, :n_b] > 0, l[b, :n_b] > 0)


def test_a_row_does_not_depend_on_the_other_rows():
    l = _rows()
    kw = dict(shift=[3.0, -2.0, 0.0], range_=[1.5, 0.5, 1.0], target_hz=[0.0, 180.0, 0.0])
    out, mean = R.edit_rows(l, lengths=[250, 300, 7], **kw)
    for b, n_b in enumerate((250, 300, 7)):
        one, m1 = R.edit_rows(l[b:b + 1], lengths=[n_b], **{k: v[b:b + 1] for k, v in kw.items()})
        assert np.array_equal(one[0], out[b]) and m1[0] == mean[b]
    # the samples past a row's length are not read: garbage there changes nothing
    dirty = l.copy()
    dirty[0, 250:] = 9.0
    again, _ = R.edit_rows(dirty, lengths=[250, 300, 7], **kw)
    assert np.array_equal(again, out)


def test_the_clamp_holds():
    l = _rows()
    out, _ = R.edit_rows(l, shift=[40.0, -40.0, 0.0], range_=[1.0, 1.0, 4.0], f_min=70.0, f_max=400.0)
    hz = R.l_to_hz(out[l > 0])
    assert hz.min() >= 70.0 * (1 - 1e-12) and hz.max() <= 400.0 * (1 + 1e-12)
    assert np.abs(R.l_to_hz(out[0][l[0] > 0]) / 400.0 - 1.0).max() <= 1e-12
    assert np.abs(R.l_to_hz(out[1][l[1] > 0]) / 70.0 - 1.0).max() <= 1e-12
    assert R.ULP_BELOW_8 >= 2.0 ** -21 and np.log1p(2900.0) < 8.0


def test_scaled_durations_reference():
    r = np.random.default_rng(5)
    v = np.exp(r.uniform(0.0, 2.0, (3, 9))).astype(np.float32)
    lens = [9, 4, 0]
    ones = np.ones((3, 9), np.float32)
    d, f = R.scaled_durations(v, lens, ones, 1.3)
    want = np.ceil((v * np.float32(1.3)).astype(np.float32))
    assert np.array_equal(d[0], want[0]) and np.array_equal(d[1, :4], want[1, :4]) and not d[1, 4:].any() and not d[2].any()
    assert f.tolist() == [float(want[0].sum()), float(want[1, :4].sum()), 0.0]
    whole = np.round(v)
    d, _ = R.scaled_durations(whole, [9, 9, 9], ones)
    assert np.array_equal(d, whole)                                        # scale 1 leaves whole durations alone
    d, _ = R.scaled_durations(whole, [9, 9, 9], 2.0 * ones)
    assert np.array_equal(d, 2.0 * whole)


# ------------------------------------------------------------------------------------------ PitchEdit and the keywords
def test_pitch_edit_check_messages():
    from megatts2_hierspeechpp_amd import _lib
    from megatts2_hierspeechpp_amd.prosody_controls import PitchEdit, check_pitch
    E = _lib.HspError
    nan, inf = float("nan"), float("inf")
    assert PitchEdit().is_identity and PitchEdit().check(3).is_identity
    assert PitchEdit(shift=[0.0, 0.0], range=[1.0, 1.0], target_hz=[0.0, 0.0]).check(2).is_identity
    assert not PitchEdit(shift=1.0).is_identity and not PitchEdit(range=0.5).is_identity
    assert not PitchEdit(target_hz=150.0).is_identity and not PitchEdit(shift=[0.0, 2.0]).is_identity
    assert not PitchEdit(offsets=torch.zeros(2, 8)).is_identity           # zeros are still an edit (include/hsp.h)
    assert check_pitch(None) is None and check_pitch(PitchEdit(), 4) is None
    assert check_pitch(PitchEdit(shift=2.0), 4).shift == 2.0
    with pytest.raises(Exception):
        PitchEdit().shift = 1.0                                            # frozen
    for kw, msg in ((dict(f_min=nan), "f_min and f_max must be finite"), (dict(f_max=inf), "f_min and f_max must be finite"),
                    (dict(f_min=40.0), "needs 55 <= f_min < f_max"), (dict(f_min=300.0, f_max=300.0), "needs 55 <= f_min < f_max"),
                    (dict(f_min=500.0, f_max=200.0), "needs 55 <= f_min < f_max"),
                    (dict(shift=None), "shift must be a number"), (dict(range=None), "range must be a number"),
                    (dict(shift=nan), "shift must be finite"), (dict(range=inf), "range must be finite"),
                    (dict(target_hz=nan), "target_hz must be finite"),
                    (dict(shift=48.5), r"shift must lie in \[-48, 48\]"), (dict(shift=[0.0, -49.0, 0.0]), "shift must lie in"),
                    (dict(range=-0.1), r"range must lie in \[0, 4\]"), (dict(range=4.5), r"range must lie in \[0, 4\]"),
                    (dict(target_hz=-100.0), "target_hz must be positive"),
                    (dict(shift=[1.0, 2.0]), r"shift must be a float or hold one value per row \(3\)"),
                    (dict(range=torch.ones(4)), r"range must be a float or hold one value per row \(3\)"),
                    (dict(target_hz=np.ones((3, 1))), "target_hz must be a float or hold one value per row"),
                    (dict(offsets=torch.zeros(2, 8)), r"offsets must be \[B = 3, n\]"),
                    (dict(offsets=torch.zeros(8)), r"offsets must be \[B = 3, n\]"),
                    (dict(offsets=[torch.zeros(8)] * 2), "offsets must be .* a list of 3 rows"),
                    (dict(offsets=1.0), "offsets must be a .* tensor or a list of rows"),
                    (dict(offsets=[torch.zeros(4), torch.tensor([0.0, nan]), torch.zeros(2)]), "offsets must be finite")):
        with pytest.raises(E, match=msg):
            PitchEdit(**kw).check(3)
    with pytest.raises(E, match="pitch must be a prosody_controls.PitchEdit"):
        check_pitch(dict(shift=2.0), 1)
    # the rows of a page's edit, as tts_lines slices them
    e = PitchEdit(shift=[0.0, 1.0, 2.0], range=0.5, target_hz=torch.tensor([0.0, 100.0, 200.0]),
                  offsets=[torch.zeros(4), torch.ones(5), torch.zeros(6)]).check(3).rows([2, 1])
    assert e.shift == [2.0, 1.0] and e.range == 0.5 and e.target_hz.tolist() == [200.0, 100.0]
    assert [o.shape[0] for o in e.offsets] == [6, 5]


def test_lf0_width_and_scale_range_errors():
    from megatts2_hierspeechpp_amd import _lib
    from megatts2_hierspeechpp_amd.prosody_controls import check_lf0, check_scales
    E = _lib.HspError
    assert check_lf0(torch.zeros(2, 76), 2, 19).shape == (2, 76) and check_lf0(torch.zeros(76), 1, 19).shape == (1, 76)
    for bad in (torch.zeros(2, 72), torch.zeros(3, 76), torch.zeros(2, 19), torch.zeros(2, 1, 76), [0.0] * 76):
        with pytest.raises(E, match=r"lf0 must be fp32 \[2, 76\] \(4 per frame of the 19 frames"):
            check_lf0(bad, 2, 19)
    # a float alone goes to the unscaled launch, as before
    assert check_scales(1.0, None, [5, 7]) == (1.0, None) and check_scales(1.3, None, [5, 7]) == (1.3, None)
    ls, sc = check_scales([1.3, 0.5], None, [2, 3])
    assert ls == 1.0 and sc.dtype == np.float32
    assert np.array_equal(sc, np.array([[1.3, 1.3, 1.0], [0.5, 0.5, 0.5]], np.float32))
    ls, sc = check_scales(1.3, [[2.0, 0.25], None], [2, 3])
    assert ls == 1.0 and sc.shape == (2, 3)
    assert np.array_equal(sc[0, :2], np.float32(1.3) * np.array([2.0, 0.25], np.float32)) and sc[0, 2] == 1.0
    assert np.array_equal(sc[1], np.full(3, 1.3, np.float32))
    # pinned durations: length_scale has never scaled them; phone_scale alone does
    assert check_scales(1.3, None, [2, 3], True) == (1.3, None) and check_scales([1.3, 2.0], None, [2, 3], True) == (1.0, None)
    assert np.array_equal(check_scales(1.3, [[2.0, 0.5], None], [2, 3], True)[1], np.array([[2, 0.5, 1], [1, 1, 1]], np.float32))
    for ls in (0.2, 4.5, float("nan"), [1.0, 0.1], [1.0, float("inf")]):
        with pytest.raises(E, match=r"length_scale must lie in \[0.25, 4\]"):
            check_scales(ls, None, [2, 3])
    for ps in ([[1.0, 0.2], None], [None, [1.0, 5.0, 1.0]], [[float("nan"), 1.0], None]):
        with pytest.raises(E, match=r"phone_scale of line \d must lie in \[0.25, 4\]"):
            check_scales(1.0, ps, [2, 3])
    with pytest.raises(E, match=r"length_scale must be a float or hold one value per line \(2\)"):
        check_scales([1.0, 1.0, 1.0], None, [2, 3])
    with pytest.raises(E, match=r"phone_scale must be a list of one row per line \(2\)"):
        check_scales(1.0, [[1.0, 1.0]], [2, 3])
    with pytest.raises(E, match="line 1: 2 phone scales for 3 phones"):
        check_scales(1.0, [None, [1.0, 1.0]], [2, 3])


def test_new_keywords_default_to_off_in_every_harness():
    from megatts2_hierspeechpp_amd import inference_plm as IP, inference_vc as IV
    tts_all = (IP.tts, IP.tts_from_codes, IP.tts_from_prompt, IP.tts_from_prompt_file, IP.tts_batch, IP.tts_lines,
               IP.tts_batch_files)
    for f in tts_all + (IV.vc, IV.vc_batch, IV.vc_batch_files):
        p = inspect.signature(f).parameters
        assert p["pitch"].default is None and p["return_lf0"].default is False, f.__name__
    for f in tts_all:
        assert inspect.signature(f).parameters["lf0"].default is None, f.__name__
    for f in (IP.tts, IP.tts_from_prompt, IP.tts_from_prompt_file, IP.tts_batch, IP.tts_lines, IP.tts_batch_files):
        p = inspect.signature(f).parameters
        assert p["length_scale"].default == 1.0 and p["phone_scale"].default is None, f.__name__
    from megatts2_hierspeechpp_amd import functional as Fh
    from megatts2_hierspeechpp_amd.ttv_v1.t2w2v_transformer import SynthesizerTrn
    assert inspect.signature(SynthesizerTrn.inf_extract_tc_latent).parameters["phone_scale"].default is None
    p = inspect.signature(Fh.f0_edit).parameters
    assert (p["f_min"].default, p["f_max"].default) == (55.0, 1100.0)
    assert all(p[k].default is None for k in ("lengths", "shift", "range", "target_hz", "offsets"))
    # the checks run before any device work
    from megatts2_hierspeechpp_amd import _lib
    from megatts2_hierspeechpp_amd.prosody_controls import PitchEdit
    with pytest.raises(_lib.HspError, match="shift must lie in"):
        IV.vc(None, None, None, None, None, None, pitch=PitchEdit(shift=60.0))
    with pytest.raises(_lib.HspError, match="pitch must be a prosody_controls.PitchEdit"):
        IP.tts_from_codes(None, torch.zeros(1, 256, 4), None, None, None, None, None, None, pitch=3.0)
    with pytest.raises(_lib.HspError, match="length_scale must lie in"):
        IP.tts(None, torch.zeros(1, 5, dtype=torch.int64), None, None, None, None, None, None, None, length_scale=8.0)


# ------------------------------------------------------------------------------------------ the C boundary
def test_header_binding_and_struct_layout_agree(tmp_path):
    from megatts2_hierspeechpp_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "hsp.h")).read()
    declared = set(re.findall(r"\b(hsp_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.lib()
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and getattr(lib, name) is not None, name
    assert _lib.SIGNATURES["hsp_f0_edit_rows_f32"][1][0] is C.POINTER(_lib.F0EditArgs)
    assert _lib.SIGNATURES["hsp_duration_scaled_f32"][1] == _lib.SIGNATURES["hsp_duration_f32"][1][:-1] + \
        [C.c_void_p, C.c_int64, C.c_void_p]                                # the same plus scale, sc_bs
    assert lib.hsp_version() == 104                                        # additive: the ABI number stays
    assert "NOT an identity row" in hdr and "bit-identical to hsp_duration_f32" in hdr
    helpers.assert_struct_layouts(tmp_path, {"hsp_f0_edit_args": _lib.F0EditArgs})


def einval_cases():
    """Every HSP_EINVAL case of the two entry points, on dummy pointers: -> the number of cases checked."""
    from megatts2_hierspeechpp_amd import _lib
    lib = _lib.lib()
    p, E = 16, _lib.EINVAL                       # a dummy non-NULL pointer: every call fails its checks first
    B, n = 4, 257
    inf, nan = float("inf"), float("nan")

    def edit(null=False, **kw):
        a = _lib.F0EditArgs()
        a.lf0, a.lf0_bs, a.B, a.n, a.f_min, a.f_max, a.out, a.out_bs = p, n, B, n, 55.0, 1100.0, p, n
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.hsp_f0_edit_rows_f32(None if null else C.byref(a), None)

    assert edit(null=True) == E
    cases = (dict(lf0=None), dict(out=None), dict(B=0), dict(B=-1), dict(B=65536), dict(n=0), dict(n=-3),
             dict(lf0_bs=n - 1), dict(out_bs=n - 1), dict(offsets=p, off_bs=n - 1), dict(f_min=nan), dict(f_max=nan),
             dict(f_min=inf), dict(f_max=inf), dict(f_min=-inf), dict(f_min=0.0), dict(f_min=-55.0),
             dict(f_min=1100.0), dict(f_min=1200.0), dict(f_max=55.0), dict(f_max=20.0))
    for kw in cases:
        assert edit(**kw) == E, kw

    def dur(logw=p, lw_bs=12, lengths=p, ls=1.0, d=p, d_bs=12, frames=p, B=3, N=12, scale=p, sc_bs=12):
        return lib.hsp_duration_scaled_f32(logw, lw_bs, lengths, ls, d, d_bs, frames, B, N, scale, sc_bs, None)

    cases_d = (dict(lengths=None), dict(d=None), dict(frames=None), dict(scale=None), dict(B=0), dict(N=0), dict(sc_bs=11),
               dict(logw=None, scale=None))
    for kw in cases_d:
        assert dur(**kw) == E, kw
    return 1 + len(cases) + len(cases_d)


def test_new_entry_points_reject_bad_arguments():
    assert einval_cases() == 30
