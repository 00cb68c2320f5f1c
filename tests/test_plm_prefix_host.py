"""CPU checks behind the prefix tests of the prosody LM (tests/test_gpu_plm_prefix.py): the float64 forced-prefix decode
equals the reference's teacher-forced pass on its own codes, every foreign-prefix case has a top-2 margin no float32 error
within the project's bar can cross and a step-P logit row that visibly depends on the prefix, the argument checks and the
schedule are right, the new entry point refuses what the header says it refuses (no device needed: refusals are decided
before any HIP call), and header, ctypes table, version script and library agree on the new names."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import plm_causal_ref as R  # noqa: E402
import plm_prefix_ref as PR  # noqa: E402
import helpers  # noqa: E402

TOL = 1e-4


# ------------------------------------------------------------------------------------------- the float64 reference
@pytest.mark.parametrize("case", PR.FOREIGN_CASES, ids=lambda c: f"P{c[0]}-T{c[1]}")
def test_foreign_prefix_case(case):
    """(a) the forced decode's logits equal R.forward_logits on its final codes to 1e-9 (at every t, so at t >= P);
    (b) the top-2 gap of every DECODED step is at least 1e-3 of the row's largest |logit|: a float32 error of 1e-4 of the
    range on two logits cannot flip a choice; (c) with the first half of the prefix replaced (codes + 512 mod 1024) the
    float64 logits of step P move by more than 10 x the tolerance: a prefill that ignored or misplaced the cache cannot
    pass the GPU test's logit comparison."""
    P, T, _ = case
    sd = R.synth_state()
    tc, prefix, codes, logits, margin, kv = PR.foreign(case)
    assert np.array_equal(codes[0, :P], prefix)
    full = R.forward_logits(sd, tc, codes, np.array([T]))
    rng = np.abs(full).max()
    assert np.abs(full[0, P:] - logits[0, P:]).max() <= 1e-9 * rng
    assert np.abs(full - logits).max() <= 1e-9 * rng
    need = 1e-3 * np.abs(logits[0, P:]).max()
    print(f"{case}: min margin {margin[0, P:].min() / np.abs(logits[0, P:]).max():.2e} of the range")
    assert (margin[0, P:] >= need).all(), np.argwhere(margin[0, P:] < need)
    # the variant that returns the caches is the same decode as the one on R.greedy_decode's hook
    c2, l2, m2 = PR.forced_decode(sd, tc, [prefix])
    assert np.array_equal(c2, codes) and np.array_equal(l2, logits) and np.array_equal(m2, margin)
    assert all(np.isfinite(k).all() and np.isfinite(v).all() for k, v in kv)
    # sensitivity of step P to the first half of the prefix: teacher-forced logits over positions 0 .. P
    half = (P + 1) // 2
    other = codes[:, :P + 1].copy()
    other[0, :half] = (other[0, :half] + 512) % 1024
    moved = R.forward_logits(sd, tc[:, :, :P + 1], other, np.array([P + 1]))[0, P]
    shift = np.abs(moved - logits[0, P]).max() / np.abs(logits[0, P]).max()
    print(f"{case}: step-P logits move by {shift:.2e} of the range when the first {half} prefix codes change")
    assert shift > 10 * TOL


def test_own_prefix_decode_reproduces_the_row():
    """A decode forced to a row's own first P codes is that row (float64, exactly: the same operations on the same
    inputs): the own-prefix GPU cases may compare against R.decoded's rows, whose margins test_plm_causal_host.py checks."""
    tc, codes, logits, _ = R.decoded((5, 13))
    pre = [codes[i, :p] for i, p in enumerate(PR.OWN_CASES[(5, 13)])]
    c2, l2, _ = PR.forced_decode(R.synth_state(), tc, pre)
    assert np.array_equal(c2, codes) and np.array_equal(l2, logits)


def test_prefill_attn_restatement_equals_the_decode_layers_attention():
    """PR.prefill_attn (the kernel's contract) column i == the attention R.decode_layer computes at t = i from the same
    k / v: checked through a layer whose out-proj is the identity and whose feed-forward is zero."""
    r = np.random.default_rng(3)
    D, H, n = 16, 4, 7
    w = dict(g1=np.ones(D), b1=np.zeros(D), g2=np.ones(D), b2=np.zeros(D), wq=r.standard_normal((D, D)), bq=r.standard_normal(D),
             wk=r.standard_normal((D, D)), bk=r.standard_normal(D), wv=r.standard_normal((D, D)), bv=r.standard_normal(D),
             wo=np.eye(D), bo=np.zeros(D), w1=np.zeros((8, D)), c1=np.zeros(8), w2=np.zeros((D, 8)), c2=np.zeros(D))
    x = r.standard_normal((n, D))
    h = R.layernorm(x, w["g1"], w["b1"])
    qkv = np.concatenate([(h @ w[a].T + w[b]).T for a, b in (("wq", "bq"), ("wk", "bk"), ("wv", "bv"))], 0)   # [3 D, n]
    qkv = np.concatenate([qkv, np.full((3 * D, 2), np.nan)], 1)                   # columns >= n are not read
    out = PR.prefill_attn(qkv, n, D, H)
    kc, vc = np.full((1, D, n), np.nan), np.full((1, D, n), np.nan)
    for t in range(n):
        y = R.decode_layer(w, x[t:t + 1], kc, vc, t, H=H)
        assert np.abs((y[0] - x[t]) - out[:, t]).max() <= 1e-12
    assert np.abs(kc[0] - qkv[D:2 * D, :n]).max() <= 1e-12 and np.abs(vc[0] - qkv[2 * D:, :n]).max() <= 1e-12


# ------------------------------------------------------------------------------------------- argument checks, schedule
def test_check_prefix():
    from megatts2_hierspeechpp_amd._lib import HspError
    from megatts2_hierspeechpp_amd.ttv_v1.t2w2v_transformer import check_prefix
    i64 = lambda *v: torch.tensor(v, dtype=torch.int64)
    assert check_prefix(i64(0, 1023, 5), 4, 1024) == 3
    assert check_prefix(i64(7), 2, 1024) == 1
    assert check_prefix(torch.zeros(2, 5, dtype=torch.int64), 6, 1024, dims=2) == 5
    bad = [(i64(), 4),                                             # P = 0
           (i64(1, 2, 3, 4), 4), (i64(1, 2, 3, 4, 5), 4),          # P >= T
           (torch.tensor([1, 2], dtype=torch.int32), 4), (torch.tensor([1.0, 2.0]), 4), ([1, 2], 4), (None, 4),   # dtype / type
           (torch.zeros(1, 2, dtype=torch.int64), 4), (torch.tensor(3, dtype=torch.int64), 4),                    # not 1-D
           (i64(1, 1024), 4), (i64(-1, 5), 4), (i64(1025), 4)]     # a code outside [0, vq_bins): go / pad ids included
    for p, T in bad:
        with pytest.raises(HspError):
            check_prefix(p, T, 1024)
    with pytest.raises(HspError):
        check_prefix(i64(1, 2), 4, 1024, dims=2)
    with pytest.raises(HspError):
        check_prefix(torch.zeros(2, 0, dtype=torch.int64), 4, 1024, dims=2)    # P = 0 columns


def test_session_plan_on_the_steps_left():
    """A request with a prefix of P of its T codes occupies its slot for T - P steps: the plan is session_plan([T_i - P_i])."""
    from megatts2_hierspeechpp_amd.ttv_v1.t2w2v_transformer import session_plan
    T, P = [13] * 5, PR.OWN_CASES[(5, 13)]
    left = [t - p for t, p in zip(T, P)]
    assert left == [8, 12, 1, 9, 5]
    plan, steps = session_plan(left, 2)
    assert plan == {0: [(0, 0), (1, 1)], 8: [(2, 0)], 9: [(3, 0)], 12: [(4, 1)]} and steps == 18
    assert session_plan(left, 8)[1] == 12
    assert session_plan([260 - 256, 260 - 64], 2)[1] == 196


# --------------------------------------------------------------------------------------------------- the entry point
def _args(L, **kw):
    a = L.PlmPrefillAttnArgs()
    a.qkv, a.out, a.k_cache, a.v_cache = 0x1000, 0x2000, 0x3000, 0x4000         # never dereferenced: every call is refused
    a.q_rs, a.o_rs, a.cs, a.n, a.D, a.H, a.debug = 32, 32, 64, 17, 276, 4, 0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_prefill_attn_refusals_are_decided_on_the_host():
    from megatts2_hierspeechpp_amd import _lib as L
    lib = L.lib()
    call = lambda a: lib.hsp_plm_prefill_attn_f32(ctypes.byref(a), None)
    assert lib.hsp_plm_prefill_attn_f32(None, None) == L.EINVAL
    refused = [dict(qkv=None), dict(k_cache=None), dict(v_cache=None), dict(n=0), dict(n=-3), dict(n=33), dict(q_rs=16),
               dict(o_rs=16), dict(cs=16), dict(q_rs=-32), dict(o_rs=-32), dict(cs=-64), dict(out=None, o_rs=-1),
               dict(D=277), dict(H=0), dict(H=-4), dict(D=0), dict(D=276, H=2), dict(D=16384, H=128), dict(debug=1),
               dict(n=65537, q_rs=70000, o_rs=70000, cs=70000), dict(n=2 ** 31 - 1, q_rs=2 ** 31, o_rs=2 ** 31, cs=2 ** 31)]
    for kw in refused:
        assert call(_args(L, **kw)) == L.EINVAL, kw
    assert lib.hsp_plm_prefill_attn_supported(276, 4) == 1 and lib.hsp_plm_prefill_attn_supported(64, 8) == 1
    assert lib.hsp_plm_prefill_attn_supported(277, 4) == 0 and lib.hsp_plm_prefill_attn_supported(276, 2) == 0
    assert lib.hsp_plm_prefill_attn_supported(512, 4) == 1 and lib.hsp_plm_prefill_attn_supported(0, 1) == 0


def test_names_agree_across_header_ctypes_map_and_library(tmp_path):
    from megatts2_hierspeechpp_amd import _lib as L
    names = ["hsp_plm_prefill_attn_supported", "hsp_plm_prefill_attn_f32"]
    hdr = open(os.path.join(ROOT, "include", "hsp.h")).read()
    declared = set(re.findall(r"\b(hsp_[a-z0-9_]+)\s*\(", hdr))
    lib = L.lib()
    for nm in names:
        assert nm in declared and nm in L.SIGNATURES and getattr(lib, nm) is not None
    assert lib.hsp_version() == 104
    assert int(re.search(r"#define HSP_VERSION (\d+)", hdr).group(1)) == 104
    assert int(re.search(r"#define HSP_PLM_PREFILL_MAX_N (\d+)", hdr).group(1)) == 65536
    # the version script exports the C ABI by its prefix: the new names need no entry of their own, and get none
    vmap = open(os.path.join(ROOT, "megatts2_hierspeechpp_amd", "csrc", "hsp.map")).read()
    assert "global: hsp_*;" in vmap and "local: *;" in vmap
    # the ctypes mirror of the argument block == the header as a C compiler sees it
    helpers.assert_struct_layouts(tmp_path, {"hsp_plm_prefill_attn_args": L.PlmPrefillAttnArgs})
