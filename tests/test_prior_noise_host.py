"""Host checks (no GPU) of the seeded prior noise (include/hsp.h "seeded prior noise"): the float64 restatement of
tests/prior_noise_ref.py against the contract's known answers, the prefix property, the separation of this stream's
counters from the prosody LM's, the statistical conditions the GPU comparisons rely on, and every refusal that is raised
before any device work: the two entry points' NULL pointers and empty sizes, ``noise`` together with ``noise_seeds`` in
`functional.sample_prior` and in every harness, seed tensors of a wrong shape.

Every statistical bound is a 4.5-sigma bound on a fixed input (n = 192 x 2048 = 393 216 values per row), never a figure
read off the stream: sigma of the mean is 1 / sqrt(n), of the variance sqrt(2 / n), of the fourth moment sqrt(96 / n)
(Var x^4 = 105 - 9), of a mean product of independent normals 1 / sqrt(n); sqrt(n) times the Kolmogorov distance
exceeds 1.95 with probability 2 exp(-2 x 1.95^2) = 1e-3."""
import math

import numpy as np
import pytest
import torch

import prior_noise_ref as R
from plm_sampling_ref import philox4x32_10

from megatts2_hierspeechpp_amd import _lib as L
from megatts2_hierspeechpp_amd import functional as Fh
from megatts2_hierspeechpp_amd import inference_plm as IP
from megatts2_hierspeechpp_amd import inference_vc as IV

SEEDS = [1000, 1001, -1, 2 ** 40 + 5]
C_STAT, T_STAT = 192, 2048


@pytest.fixture(scope="module")
def rows():
    """The four rows of the statistical conditions, computed once and never written."""
    x = R.randn_rows(SEEDS, C_STAT, T_STAT)
    x.setflags(write=False)
    return x


# ------------------------------------------------------------------------------------------------ the stream
@pytest.mark.parametrize("key", sorted(R.KNOWN), ids=lambda k: f"seed{k[0]}-c{k[1]}-t{k[2]}")
def test_known_answers(key):
    seed, c, t0 = key
    want = np.array(R.KNOWN[key])
    got = R.randn_row(seed, c + 1, t0 + len(want))[c, t0:]
    assert np.abs(got - want).max() <= 1e-12, (key, got, want)
    # the same values from a row cut at t0: frames are addressed by their own index
    assert np.array_equal(R.randn_row(seed, c + 1, t0 + len(want), t0)[c], got)


def test_key_is_the_two_halves_of_the_twos_complement_seed():
    assert R.key_of(-1) == (0xFFFFFFFF, 0xFFFFFFFF)
    assert R.key_of(2 ** 40 + 5) == (5, 256)
    assert R.key_of(2 ** 63 - 1) == (0xFFFFFFFF, 0x7FFFFFFF)
    assert R.key_of(-2 ** 63) == (0, 0x80000000)


def test_uniforms_are_exact_in_fp32_and_r_is_bounded():
    """u1 = ((w >> 9) + 0.5) 2^-23 and 2 u2 = (w >> 8) 2^-23 at the ends of the word range: exact in float32, u1 inside
    (0, 1), and r = sqrt(-2 ln u1) at most sqrt(48 ln 2)."""
    for w in (0, 1, 2 ** 31, 2 ** 32 - 1):
        u1 = ((w >> 9) + 0.5) * 2.0 ** -23
        u2x2 = (w >> 8) * 2.0 ** -23
        assert float(np.float32(u1)) == u1 and 0.0 < u1 < 1.0
        assert float(np.float32(u2x2)) == u2x2 and 0.0 <= u2x2 < 2.0
        assert math.sqrt(-2.0 * math.log(u1)) <= R.R_MAX
    assert abs(R.R_MAX - 5.768) < 1e-3


def test_prefix_property(rows):
    """Frames 0 .. T - 1 of a longer row are its first T frames."""
    for b, seed in enumerate(SEEDS):
        assert np.array_equal(R.randn_row(seed, C_STAT, 19), rows[b][:, :19])
    assert np.array_equal(R.randn_rows(SEEDS[:2], 3, 5), rows[:2, :3, :5])


def test_counters_never_coincide_with_the_plm_stream():
    """This stream's counters end in 1, the PLM draws' (i >> 2, j, 0, 0) in 0: for one key the two sets are disjoint,
    and the words they give differ."""
    mine = R.counters(8, 0, 64).reshape(-1, 4)
    assert (mine[:, 3] == R.STREAM).all() and R.STREAM != 0
    i, j = np.meshgrid(np.arange(64, dtype=np.uint64), np.arange(8, dtype=np.uint64))
    plm = np.stack([i, j, np.zeros_like(i), np.zeros_like(i)], -1).reshape(-1, 4)       # plm_sampling_ref.exp_draws
    assert not set(map(tuple, mine.tolist())) & set(map(tuple, plm.tolist()))
    key = np.broadcast_to(np.array(R.key_of(1000), np.uint64), (len(mine), 2))
    assert not (philox4x32_10(mine, key) == philox4x32_10(plm, key)).all(-1).any()


# ------------------------------------------------------------------------------------------------ statistics
def _normal_cdf(x):
    return 0.5 * (1.0 + np.vectorize(math.erf)(x / math.sqrt(2.0)))


@pytest.mark.parametrize("b", range(len(SEEDS)), ids=[f"seed{s}" for s in SEEDS])
def test_moments_ks_and_range(rows, b):
    v = rows[b].ravel()
    n = v.size
    assert n == 393216
    mean, var, m4 = v.mean(), v.var(), (v ** 4).mean()
    s = np.sort(v)
    cdf = _normal_cdf(s)
    k = np.arange(n)
    ks = max(np.abs(cdf - k / n).max(), np.abs(cdf - (k + 1) / n).max()) * math.sqrt(n)
    print(f"seed {SEEDS[b]}: mean {mean:.3e} var-1 {var - 1:.3e} Ex^4-3 {m4 - 3:.3e} KS sqrt(n) {ks:.3f} "
          f"max|x| {np.abs(v).max():.3f}")
    assert abs(mean) <= 4.5 / math.sqrt(n)
    assert abs(var - 1.0) <= 4.5 * math.sqrt(2.0 / n)
    assert abs(m4 - 3.0) <= 4.5 * math.sqrt(96.0 / n)
    assert ks <= 1.95
    assert np.abs(v).max() <= R.R_MAX


def _mean_product(a, b):
    return float((a * b).mean())


def test_rows_channels_and_frames_are_uncorrelated(rows):
    bound = 4.5 / math.sqrt(rows[0].size)
    got = {"row s, s + 1": _mean_product(rows[0], rows[1])}            # seeds 1000 and 1001
    for b, seed in enumerate(SEEDS):
        x = rows[b]
        got[f"seed {seed}: channel c, c + 1"] = _mean_product(x[:-1], x[1:])
        got[f"seed {seed}: frame t, t + 1"] = _mean_product(x[:, :-1], x[:, 1:])
        got[f"seed {seed}: frame t, t + 2"] = _mean_product(x[:, :-2], x[:, 2:])
    for name, v in got.items():
        print(f"{name}: {v:.3e} (bound {bound:.1e})")
        assert abs(v) <= bound, (name, v)


# ------------------------------------------------------------------------------------------------ the C ABI refuses
P, Q = 16, 32          # dummy non-NULL pointers: every call below fails its checks before anything is launched

# name -> (arguments of a well-formed call, positions of the required pointers, positions of the sizes)
GOOD = {
    "hsp_randn_rows_f32": ([P, Q, 2, 3, 4, None], (0, 1), (2, 3, 4)),
    "hsp_sample_prior_seeded_f32": ([P, P, P, Q, 2, 3, 4, 0.5, None], (0, 1, 2, 3), (4, 5, 6)),
}


@pytest.mark.parametrize("name", sorted(GOOD))
def test_entry_points_refuse_null_pointers_and_empty_sizes(name):
    args, ptrs, sizes = GOOD[name]
    fn = getattr(L.lib(), name)
    assert len(args) == len(L.SIGNATURES[name][1])

    def swapped(at, value):
        a = list(args)
        a[at] = value
        return a

    for at in ptrs:
        assert fn(*swapped(at, None)) == L.EINVAL, (name, "NULL at", at)
    for at in sizes:
        for bad in (0, -1):
            assert fn(*swapped(at, bad)) == L.EINVAL, (name, bad, "at", at)


# ------------------------------------------------------------------------------------------------ Python refuses
def test_row_seeds_is_the_one_seed_rule():
    from megatts2_hierspeechpp_amd.ttv_v1 import t2w2v_transformer as T2
    assert T2.plm_seeds is Fh.row_seeds                       # one function, two names
    assert Fh.row_seeds(7, 3, "cpu").tolist() == [7, 8, 9]
    assert Fh.row_seeds(-2, 3, "cpu").tolist() == [-2, -1, 0]
    given = torch.tensor([5, 2 ** 40 + 5, -1], dtype=torch.int64)
    assert Fh.row_seeds(given, 3, "cpu") is given             # used as it is, in place
    assert Fh.row_seeds(given.to(torch.int32)[:2], 2, "cpu").dtype == torch.int64
    with pytest.raises(L.HspError, match="shape"):
        Fh.row_seeds(given, 2, "cpu")


def test_sample_prior_takes_exactly_one_of_noise_and_seeds():
    stats, mask, noise = torch.zeros(2, 6, 5), torch.ones(2, 1, 5), torch.zeros(2, 3, 5)
    with pytest.raises(L.HspError, match="not both"):
        Fh.sample_prior(stats, noise, mask, 1.0, seeds=3)
    with pytest.raises(L.HspError, match="noise or seeds"):
        Fh.sample_prior(stats, None, mask, 1.0)
    for bad in (torch.zeros(3, dtype=torch.int64), torch.zeros(2, 1, dtype=torch.int64), torch.zeros(2)):
        with pytest.raises(L.HspError, match="seeds must be"):
            Fh.sample_prior(stats, None, mask, 1.0, seeds=bad)
    with pytest.raises(L.HspError, match="seeds must be"):
        Fh.sample_prior(stats, None, mask, 1.0, seeds=1.5)


def test_randn_rows_refuses_seeds_that_are_no_vector():
    for bad in (7, torch.zeros(2, 2, dtype=torch.int64), torch.tensor(3)):
        with pytest.raises(L.HspError, match=r"int64 \[B\]"):
            Fh.randn_rows(bad, 192, 8)


def _line(n):
    return (torch.ones(n, dtype=torch.int64), torch.zeros(n, dtype=torch.int64), torch.ones(n, dtype=torch.int64))


LINES = [_line(4), _line(6), _line(3)]
PROMPT = torch.zeros(2000)
NOISE3 = torch.zeros(3, 192, 8)
TEXT3 = torch.ones(3, 4, dtype=torch.int64)


def _no_file(monkeypatch):
    from megatts2_hierspeechpp_amd import audio as A

    def no_load(path, *a, **k):
        raise AssertionError(f"{path} was read")

    monkeypatch.setattr(A, "load", no_load)
    monkeypatch.setattr(A, "load_16k", no_load)


# every harness with models=None: the refusal comes before any model, file or device is touched
BOTH = {
    "tts": lambda: IP.tts(None, TEXT3, *([None] * 7), noise=NOISE3, noise_seeds=7),
    "tts_from_codes": lambda: IP.tts_from_codes(None, torch.zeros(3, 256, 8), *([None] * 6), noise=NOISE3,
                                                noise_seeds=7),
    "tts_from_prompt": lambda: IP.tts_from_prompt(None, None, TEXT3[:1], TEXT3[:1], TEXT3[:1], PROMPT.reshape(1, -1),
                                                  noise=NOISE3[:1], noise_seed=7),
    "tts_from_prompt_file": lambda: IP.tts_from_prompt_file(None, None, TEXT3[:1], TEXT3[:1], TEXT3[:1], "missing.wav",
                                                            noise=NOISE3[:1], noise_seed=7),
    "tts_batch": lambda: IP.tts_batch(None, None, LINES, PROMPT, noise=NOISE3, noise_seeds=7),
    "tts_lines": lambda: IP.tts_lines(None, None, LINES, PROMPT, noise=NOISE3, noise_seeds=7),
    "tts_batch_files": lambda: IP.tts_batch_files(None, None, LINES, "missing.wav", noise=NOISE3, noise_seeds=7),
    "vc": lambda: IV.vc(None, None, torch.zeros(1, 1280), torch.zeros(1, 16), PROMPT, torch.zeros(25),
                        noise=NOISE3[:1], noise_seed=7),
    "vc_batch": lambda: IV.vc_batch(None, None, [torch.zeros(1280)] * 3, [torch.zeros(16)] * 3, PROMPT, torch.zeros(25),
                                    noise=NOISE3, noise_seeds=7),
    "vc_batch_files": lambda: IV.vc_batch_files(None, None, ["a.wav", "b.wav", "c.wav"], "missing.wav", noise=NOISE3,
                                                noise_seeds=7),
}


@pytest.mark.parametrize("name", sorted(BOTH))
def test_every_harness_refuses_noise_together_with_noise_seeds(name, monkeypatch):
    _no_file(monkeypatch)
    with pytest.raises(L.HspError, match="not both"):
        BOTH[name]()


WRONG = torch.zeros(2, dtype=torch.int64)          # three rows, two seeds
WRONG_SHAPE = {
    "tts": lambda s: IP.tts(None, TEXT3, *([None] * 7), noise_seeds=s),
    "tts_from_codes": lambda s: IP.tts_from_codes(None, torch.zeros(3, 256, 8), *([None] * 6), noise_seeds=s),
    "tts_from_prompt": lambda s: IP.tts_from_prompt(None, None, TEXT3[:1], TEXT3[:1], TEXT3[:1], PROMPT.reshape(1, -1),
                                                    noise_seed=s),
    "tts_batch": lambda s: IP.tts_batch(None, None, LINES, PROMPT, noise_seeds=s),
    "tts_lines": lambda s: IP.tts_lines(None, None, LINES, PROMPT, noise_seeds=s),
    "tts_batch_files": lambda s: IP.tts_batch_files(None, None, LINES, "missing.wav", noise_seeds=s),
    "vc": lambda s: IV.vc(None, None, torch.zeros(1, 1280), torch.zeros(1, 16), PROMPT, torch.zeros(25), noise_seed=s),
    "vc_batch": lambda s: IV.vc_batch(None, None, [torch.zeros(1280)] * 3, [torch.zeros(16)] * 3, PROMPT,
                                      torch.zeros(25), noise_seeds=s),
    "vc_batch_files": lambda s: IV.vc_batch_files(None, None, ["a.wav", "b.wav", "c.wav"], "missing.wav",
                                                  noise_seeds=s),
}


@pytest.mark.parametrize("name", sorted(WRONG_SHAPE))
def test_every_harness_refuses_seed_tensors_of_the_wrong_shape(name, monkeypatch):
    _no_file(monkeypatch)
    with pytest.raises(L.HspError, match="noise_seed"):
        WRONG_SHAPE[name](WRONG)
    if name not in ("tts_from_prompt", "vc"):                 # a [B, 1] column is no [B] vector either
        with pytest.raises(L.HspError, match="noise_seed"):
            WRONG_SHAPE[name](torch.zeros(3, 1, dtype=torch.int64))


def test_tts_lines_gives_line_k_the_seed_s_plus_k():
    """An int gives the caller's line k the seed s + k; a tensor holds one per line (what `tts_lines` slices per chunk,
    for ``seeds`` and ``noise_seeds`` alike)."""
    assert IP._line_seeds(7, 5, "noise_seeds").tolist() == [7, 8, 9, 10, 11]
    given = torch.tensor([4, 4, -9], dtype=torch.int32)
    got = IP._line_seeds(given, 3, "noise_seeds")
    assert got.dtype == torch.int64 and got.tolist() == [4, 4, -9]
    with pytest.raises(L.HspError, match="noise_seeds"):
        IP._line_seeds(given, 4, "noise_seeds")
    chunks = IP.line_chunks([4, 6, 3, 6, 1], 2)               # [[4, 2], [0, 1], [3]]
    seeds = IP._line_seeds(7, 5, "noise_seeds")
    assert [[int(seeds[k]) for k in rows] for rows in chunks] == [[11, 9], [7, 8], [10]]


def test_the_new_keywords_default_to_todays_draw():
    import inspect
    from megatts2_hierspeechpp_amd.hierspeechpp_speechsynthesizer import PosteriorSFEncoder, SynthesizerTrn
    for fn in (IP.tts, IP.tts_from_codes, IP.tts_lines, IV.vc_batch, SynthesizerTrn.infer,
               SynthesizerTrn.voice_conversion, SynthesizerTrn.voice_conversion_noise_control,
               PosteriorSFEncoder.forward):
        assert inspect.signature(fn).parameters["noise_seeds"].default is None, fn
    for fn in (IP.tts_from_prompt, IV.vc):
        assert inspect.signature(fn).parameters["noise_seed"].default is None, fn
    assert inspect.signature(Fh.sample_prior).parameters["seeds"].default is None
