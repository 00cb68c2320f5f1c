"""CPU checks of the float64 restatement the causal-PLM GPU tests compare against (tests/plm_causal_ref.py): it equals the
reference's own forward logits (golden fixture), its K/V-cached decode equals its full causal pass, and every decode case
used on the GPU has a top-2 margin no float32 error within the project's bar can cross."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import plm_causal_ref as R  # noqa: E402


def test_restated_forward_equals_reference_golden():
    g = np.load(os.path.join(HERE, "golden", "causal", "plm_causal_b2_t24.npz"))
    assert g["lens"].tolist() == [24, 17] and g["logits"].shape == (2, 24, 1024)
    lg = R.forward_logits(R.synth_state(), g["tc"], g["p_codes"], g["lens"])
    rng = np.abs(g["logits"]).max()
    for b, n in enumerate(g["lens"]):
        err = np.abs(lg[b, :n] - g["logits"][b, :n]).max()
        print(f"row {b}: max|f64 - reference| = {err:.3e} (range {rng:.3f})")
        assert err <= 1e-4 * rng          # the golden is the reference's float32 run


def test_kv_cached_decode_equals_full_causal_pass():
    """The identity the feature rests on: the step-t logits of a decode are the teacher-forced logits [:, t] of its own
    codes (float64: equal to rounding)."""
    sd = R.synth_state()
    for shape in [(3, 9), (5, 13)]:
        tc, codes, logits, _ = R.decoded(shape)
        full = R.forward_logits(sd, tc, codes, np.full(shape[0], shape[1]))
        assert np.abs(full - logits).max() <= 1e-10 * np.abs(full).max()
    # ragged lens: a short row's valid positions do not depend on what the padding holds
    tc, codes, logits, _ = R.decoded((3, 9))
    lens = np.array([9, 4, 6])
    junk = codes.copy()
    for b, n in enumerate(lens):
        junk[b, n:] = 1025
    full = R.forward_logits(sd, tc, junk, lens)
    for b, n in enumerate(lens):
        assert np.abs(full[b, :n] - logits[b, :n]).max() <= 1e-10 * np.abs(full).max()


@pytest.mark.parametrize("shape", sorted(R.DECODE_CASES))
def test_decode_cases_have_a_safe_top2_margin(shape):
    _, _, logits, margin = R.decoded(shape)
    need = 1e-3 * np.abs(logits).max()
    print(f"{shape}: min margin {margin.min():.4f}, needed {need:.4f}")
    assert (margin >= need).all(), np.argwhere(margin < need)
