"""Host checks of the sampled PLM decoding: the Philox stream, the numpy restatement against the reference's fixtures,
argument refusals (no GPU needed: the C entry points refuse before any launch) and the ABI of hsp_sample_args."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import plm_sampling_ref as R  # noqa: E402
import helpers  # noqa: E402

GOLD = os.path.join(HERE, "golden", "sampling")


def test_philox_known_answers():
    cases = [([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
             ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
             ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0],
              [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])]
    for ctr, key, want in cases:
        assert R.philox4x32_10(np.array(ctr, np.uint64), np.array(key, np.uint64)).tolist() == want


def _cases():
    d = np.load(os.path.join(GOLD, "plm_sample_cases.npz"))
    meta = json.loads(bytes(d["meta"]).decode())
    for c, m in enumerate(meta):
        prev = [int(t) for t in d["prev"][c][:m["n_prev"]]]
        kw = {k: m[k] for k in ("temperature", "top_k", "top_p", "repetition_penalty")}
        yield d["logits"][c], prev, int(d["seed"][c]), int(d["j"][c]), kw, d["probs"][c], int(d["token"][c])


def test_restatement_reproduces_reference_fixture():
    n = 0
    for logits, prev, seed, j, kw, probs, token in _cases():
        tok, p = R.decide(logits, prev, seed, j, **kw)
        assert np.abs(p - probs).max() <= 1e-6, kw
        assert tok == token, kw
        n += 1
    assert n >= 12


def test_loop_fixture_is_consistent():
    d = np.load(os.path.join(GOLD, "plm_sample_loop.npz"))
    meta = json.loads(bytes(d["meta"]).decode())
    assert d["codes"].shape == (3, 40) and d["seeds"].shape == (3,) and meta["min_gap"] > 1e-4
    assert ((d["codes"] >= 0) & (d["codes"] < 1024)).all()


def test_plm_sampling_validates():
    from megatts2_hierspeechpp_amd.ttv_v1.t2w2v_transformer import PlmSampling
    PlmSampling()
    PlmSampling(temperature=0.0, top_k=1, top_p=1.0, repetition_penalty=0.5)
    for bad in (dict(temperature=-1.0), dict(temperature=float("nan")), dict(temperature=float("inf")),
                dict(top_k=0), dict(top_k=-3), dict(top_k=2.5), dict(top_k=True), dict(top_p=0.0), dict(top_p=-0.1),
                dict(top_p=1.5), dict(top_p=float("nan")), dict(repetition_penalty=0.0),
                dict(repetition_penalty=-1.0), dict(repetition_penalty=float("inf"))):
        with pytest.raises(ValueError):
            PlmSampling(**bad)


def test_c_entry_points_refuse_invalid_arguments():
    from megatts2_hierspeechpp_amd import _lib
    lib = _lib.lib()
    # fake, never dereferenced pointers: every refusal happens on the host before any launch
    p = 0x1000

    def args(**kw):
        a = dict(temperature=1.0, top_k=0, top_p=2.0, repetition_penalty=1.0, seeds=p, probs=None, probs_bs=0)
        a.update(kw)
        return _lib.SampleArgs(**a)

    def sample(a, N=1024, j=1):
        return lib.hsp_sample_f32(p, 1, 4, 4, N, p, 8, j, ctypes.byref(a) if a is not None else None, None)

    def embed(a, n_logits=1024, j=1):
        return lib.hsp_plm_embed_sample_f32(p, 1, 1, 256, p, 8, p, 20, 1026, p, 4000, p, p, 2, 8, 4, 2, p, 1, 4,
                                            n_logits, j, ctypes.byref(a), None)

    bad = [args(top_k=-1), args(top_p=0.0), args(top_p=-1.0), args(top_p=float("nan")), args(repetition_penalty=0.0),
           args(repetition_penalty=-2.0), args(repetition_penalty=float("nan")), args(temperature=float("inf")),
           args(temperature=float("nan")), args(seeds=None)]
    for a in bad:
        assert sample(a) == _lib.EINVAL
        assert embed(a) == _lib.EINVAL
    assert sample(None) == _lib.EINVAL
    assert sample(args(), N=1025) == _lib.EINVAL
    assert embed(args(), n_logits=1025) == _lib.EINVAL
    assert sample(args(), j=0) == _lib.EINVAL
    assert embed(args(), j=3) == _lib.EINVAL     # the full form (n = 2) chooses column n - 1 = 1


def test_sample_args_struct_matches_the_header(tmp_path):
    from megatts2_hierspeechpp_amd import _lib
    helpers.assert_struct_layouts(tmp_path, {"hsp_sample_args": _lib.SampleArgs})


def test_seeds_helper_shapes():
    from megatts2_hierspeechpp_amd.ttv_v1.t2w2v_transformer import plm_seeds
    assert plm_seeds(7, 3, "cpu").tolist() == [7, 8, 9]
    assert plm_seeds(torch.tensor([5, 1], dtype=torch.int32), 2, "cpu").dtype == torch.int64


def test_takes_need_sampling_and_a_positive_count():
    from megatts2_hierspeechpp_amd import _lib, inference_plm as IP
    from megatts2_hierspeechpp_amd.ttv_v1.t2w2v_transformer import PlmSampling
    text = torch.zeros(1, 3, dtype=torch.int64)
    with pytest.raises(_lib.HspError):
        IP.tts_from_prompt(None, None, text, text, text, None, takes=2)
    with pytest.raises(_lib.HspError):
        IP.tts_from_prompt(None, None, text, text, text, None, takes=0, plm_sampling=PlmSampling())


def test_top_word_seed_is_what_the_gpu_test_says():
    """The (seed, column, token) of test_top_word_draw_is_not_infinite draws the largest 24-bit word: u = 1 - 2^-25."""
    q = R.exp_draws(725543, 1)
    assert abs(q[11] - 2.0 ** -25) < 1e-12 and q[11] == q.min()
