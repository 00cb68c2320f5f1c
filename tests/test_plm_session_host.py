"""CPU checks of the prosody LM's decode sessions: the schedule (session_plan) against hand-worked cases and its
invariants, and the argument checks of the three per-row-position entry points, which run before any HIP call (so they
run here on dummy pointers)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hsp_plm_decode_layer_pos_f32", "hsp_plm_embed_pos_f32", "hsp_plm_choose_advance_f32")


def _plan():
    from megatts2_hierspeechpp_amd.ttv_v1.t2w2v_transformer import session_plan
    return session_plan


# ------------------------------------------------------------------------------------------------------ schedule
def test_session_plan_hand_worked_case():
    """lengths 13, 4, 9, 1, 7 in 2 slots: requests 0, 1 start at step 0; slot 1 is free after 4 steps and takes request
    2 for steps 4 .. 12; request 0 ends at step 12 too, so 3 and 4 start at step 13 and the 7-frame one ends at step 19:
    20 steps, against 13 + 9 + 7 = 29 for in-order batches of 2 padded to their longest row."""
    adm, steps = _plan()([13, 4, 9, 1, 7], 2)
    assert steps == 20
    assert adm == {0: [(0, 0), (1, 1)], 4: [(2, 1)], 13: [(3, 0), (4, 1)]}
    batches = sum(max(b) for b in ([13, 4], [9, 1], [7]))
    assert batches == 29 and steps < batches


def test_session_plan_edges():
    plan = _plan()
    assert plan([5, 2, 9], 3) == ({0: [(0, 0), (1, 1), (2, 2)]}, 9)            # slots == requests
    assert plan([5, 2, 9], 8) == ({0: [(0, 0), (1, 1), (2, 2)]}, 9)            # more slots than requests
    assert plan([6], 1) == ({0: [(0, 0)]}, 6) and plan([6], 4) == ({0: [(0, 0)]}, 6)
    assert plan([1, 1, 1], 1) == ({0: [(0, 0)], 1: [(1, 0)], 2: [(2, 0)]}, 3)  # length 1: the slot is free the next step
    assert plan([1, 1, 1], 2) == ({0: [(0, 0), (1, 1)], 1: [(2, 0)]}, 2)
    assert plan([3, 1, 1, 1], 2) == ({0: [(0, 0), (1, 1)], 1: [(2, 1)], 2: [(3, 1)]}, 3)
    assert plan([], 2) == ({}, 0)
    from megatts2_hierspeechpp_amd._lib import HspError
    for lengths, slots in (([3, 0], 2), ([3, -1], 2), ([3], 0), ([3], -2)):
        with pytest.raises(HspError):
            plan(lengths, slots)


def test_session_plan_invariants_on_seeded_draws():
    plan = _plan()
    r = np.random.default_rng(20)
    for _ in range(200):
        n, slots = int(r.integers(1, 40)), int(r.integers(1, 9))
        lengths = [int(v) for v in r.integers(1, 30, n)]
        adm, steps = plan(lengths, slots)
        seen = sorted(req for pairs in adm.values() for req, _ in pairs)
        assert seen == list(range(n))                                           # every request exactly once
        busy_until = [0] * slots
        last_step, last_req = 0, -1
        for step in sorted(adm):
            assert step >= last_step
            for req, slot in adm[step]:
                assert req == last_req + 1                                      # in arrival order
                assert 0 <= slot < slots and busy_until[slot] <= step           # never double-booked
                assert slot == min(k for k in range(slots) if busy_until[k] <= step)   # the lowest free slot
                busy_until[slot] = step + lengths[req]
                last_req = req
            last_step = step
        assert steps == max(busy_until)
        assert math.ceil(sum(lengths) / slots) <= steps <= sum(lengths)


# ------------------------------------------------------------------------------------------------ the C boundary
def _lib_or_build():
    from megatts2_hierspeechpp_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


def test_header_binding_and_library_agree_on_the_new_names():
    _lib = _lib_or_build()
    hdr = open(os.path.join(ROOT, "include", "hsp.h")).read()
    declared = set(re.findall(r"\b(hsp_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.lib()
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and getattr(lib, name) is not None, name
    assert lib.hsp_version() == 104                                             # additive: the ABI number stays
    assert "#define HSP_VERSION 104" in hdr


D_ = ctypes.c_void_p(0x1000)        # never dereferenced: every call below is refused before any HIP call


def _decode_args(_lib, **over):
    a = _lib.PlmDecodeArgs()
    for name, ctype in _lib.PlmDecodeArgs._fields_:
        if ctype is ctypes.c_void_p:
            setattr(a, name, 0x1000)
    a.x_bs, a.x_cs, a.y_bs, a.y_cs, a.bs, a.cs = 1, 2, 1, 2, 8, 16
    a.t, a.B, a.D, a.H, a.F, a.eps = 3, 2, 276, 4, 1104, 1e-5
    a.workspace_bytes, a.debug = 4 * 2 * 276 * 13, 0
    for k, v in over.items():
        setattr(a, k, v)
    return a


BAD_LAYER = [("t", -1), ("t", 16), ("t", 2 ** 31 - 1), ("debug", 1), ("B", 0), ("B", 70000), ("D", 277), ("D", 0), ("H", 5),
             ("F", 1102), ("F", 8192 * 12), ("workspace_bytes", 4 * 2 * 276 * 13 - 4), ("workspace_bytes", 0), ("x_bs", -1),
             ("y_cs", -1), ("bs", -1), ("wo_t", 0x1004), ("workspace", 0x1008)]


@pytest.mark.parametrize("field,value", BAD_LAYER, ids=[f"{f}={v}" for f, v in BAD_LAYER])
def test_layer_pos_refuses_what_the_by_value_entry_refuses(field, value):
    _lib = _lib_or_build()
    a = _decode_args(_lib, **{field: value})
    assert _lib.lib().hsp_plm_decode_layer_pos_f32(ctypes.byref(a), D_, None) == _lib.EINVAL
    assert _lib.lib().hsp_plm_decode_layer_f32(ctypes.byref(a), None) == _lib.EINVAL


def test_layer_pos_refuses_null_operands():
    _lib = _lib_or_build()
    call = _lib.lib().hsp_plm_decode_layer_pos_f32
    assert call(None, D_, None) == _lib.EINVAL
    assert call(ctypes.byref(_decode_args(_lib)), None, None) == _lib.EINVAL   # NULL pos: the one refusal it adds
    for name, ctype in _lib.PlmDecodeArgs._fields_:
        if ctype is ctypes.c_void_p:
            assert call(ctypes.byref(_decode_args(_lib, **{name: None})), D_, None) == _lib.EINVAL, name


# hsp_plm_embed_pos_f32(tc, tc_bs, tc_cs, Dtc, codes, codes_bs, emb, Demb, n_emb, pe_t, P, alpha, x, x_bs, x_cs, B, pos,
#                       max_pos, stream)
EMBED = dict(tc=D_, tc_bs=256 * 40, tc_cs=40, Dtc=256, codes=D_, codes_bs=41, emb=D_, Demb=20, n_emb=1026, pe_t=D_, P=4000,
             alpha=D_, x=D_, x_bs=1, x_cs=4, B=4, pos=D_, max_pos=39)


def _embed(_lib, **over):
    a = dict(EMBED, **over)
    return _lib.lib().hsp_plm_embed_pos_f32(*[a[k] for k in EMBED], None)


def test_embed_pos_refusals():
    _lib = _lib_or_build()
    for name in ("tc", "codes", "emb", "pe_t", "alpha", "x", "pos"):
        assert _embed(_lib, **{name: None}) == _lib.EINVAL, name
    for over in (dict(max_pos=4000), dict(max_pos=4001), dict(max_pos=39, P=39), dict(max_pos=-1), dict(B=0), dict(B=-3),
                 dict(B=65536), dict(Dtc=0), dict(Demb=0), dict(n_emb=0), dict(x_bs=-1), dict(x_cs=-1), dict(tc_bs=-1),
                 dict(tc_cs=-1), dict(codes_bs=-1)):
        assert _embed(_lib, **over) == _lib.EINVAL, over


# hsp_plm_choose_advance_f32(logits, l_bs, l_cs, B, N, codes, codes_bs, pos, len, max_pos, args, stream)
CHOOSE = dict(logits=D_, l_bs=1, l_cs=4, B=4, N=1024, codes=D_, codes_bs=41, pos=D_, len=D_, max_pos=39)


def _choose(_lib, args=None, **over):
    a = dict(CHOOSE, **over)
    return _lib.lib().hsp_plm_choose_advance_f32(*[a[k] for k in CHOOSE], args, None)


def test_choose_advance_refusals():
    _lib = _lib_or_build()
    for name in ("logits", "codes", "pos", "len"):
        assert _choose(_lib, **{name: None}) == _lib.EINVAL, name
    for over in (dict(B=0), dict(B=65536), dict(N=0), dict(l_cs=0), dict(l_bs=-1), dict(max_pos=-1), dict(codes_bs=-1)):
        assert _choose(_lib, **over) == _lib.EINVAL, over
    # with sampling: the refusals of hsp_sample_f32
    ok = dict(temperature=1.0, top_k=40, top_p=0.9, repetition_penalty=1.2, seeds=0x1000, probs=None, probs_bs=0)
    for over in (dict(seeds=None), dict(top_k=-1), dict(top_p=0.0), dict(top_p=-0.5), dict(repetition_penalty=0.0),
                 dict(repetition_penalty=float("inf")), dict(temperature=float("nan")), dict(temperature=float("inf")),
                 dict(probs=0x1000, probs_bs=1023)):
        s = _lib.SampleArgs(**dict(ok, **over))
        assert _choose(_lib, ctypes.byref(s)) == _lib.EINVAL, over
        assert _lib.lib().hsp_sample_f32(D_, 1, 4, 4, 1024, D_, 41, 1, ctypes.byref(s), None) == _lib.EINVAL, over
    s = _lib.SampleArgs(**ok)
    assert _choose(_lib, ctypes.byref(s), N=1025) == _lib.EINVAL               # more logits than the sampler holds
    for name in ("logits", "codes", "pos", "len"):
        assert _choose(_lib, ctypes.byref(s), **{name: None}) == _lib.EINVAL, name
