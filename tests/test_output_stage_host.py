"""CPU: the output stage (megatts2_hierspeechpp_amd/output.py) -- the one validation and its order, the defaults every
harness signature shares with the dataclass, the result packer, the rate rule, and that every harness rejects a bad
stage before it touches any other argument (so the calls run here on None models)."""
import dataclasses
import inspect
import itertools

import pytest

OUTPUT_KEYWORDS = ("scale_norm", "target_lufs", "limiter", "ceiling_db", "lookahead_ms", "limiter_passes",
                   "return_stats")
UNKNOWN = "unknown scale_norm 'rms'"
LIMITER = "limiter=True needs scale_norm='lufs'"
STATS = "return_stats=True needs limiter=True"


def _harnesses():
    """name -> (harness, its positional arguments as Nones)"""
    from megatts2_hierspeechpp_amd import inference_plm as IP, inference_vc as IV
    from megatts2_hierspeechpp_amd.inference_speechsr import super_resolution
    return {"tts": (IP.tts, 9), "tts_from_codes": (IP.tts_from_codes, 8), "tts_from_prompt": (IP.tts_from_prompt, 6),
            "tts_from_prompt_file": (IP.tts_from_prompt_file, 6), "vc": (IV.vc, 6), "vc_batch": (IV.vc_batch, 6),
            "vc_batch_files": (IV.vc_batch_files, 4), "super_resolution": (super_resolution, 3)}


def test_fields_and_defaults():
    from megatts2_hierspeechpp_amd.output import OutputStage
    got = [(f.name, f.default) for f in dataclasses.fields(OutputStage)]
    assert got == list(zip(OUTPUT_KEYWORDS, ("max", -23.0, False, -1.0, 1.5, 2, False)))
    with pytest.raises(dataclasses.FrozenInstanceError):
        OutputStage().limiter = True
    assert OutputStage.of(dict(scale_norm="lufs", limiter=True, noise=None, output_sr=48000)) == \
        OutputStage(scale_norm="lufs", limiter=True)


def test_check_messages_order_and_valid_combinations():
    from megatts2_hierspeechpp_amd import _lib
    from megatts2_hierspeechpp_amd.output import SCALE_NORMS, OutputStage
    assert SCALE_NORMS == ("max", "prompt", "lufs")

    def raises(match, norms=None, **kw):
        with pytest.raises(_lib.HspError, match=match) as e:
            OutputStage(**kw).check() if norms is None else OutputStage(**kw).check(norms=norms)
        return str(e.value)

    # each invalid combination on its own, with today's texts
    assert raises(UNKNOWN, scale_norm="rms") == "unknown scale_norm 'rms' ('max', 'prompt', 'lufs')"
    assert raises("unknown scale_norm 'prompt'", norms=("max", "lufs"), scale_norm="prompt") == \
        "unknown scale_norm 'prompt' ('max' or 'lufs')"
    for norm in ("max", "prompt"):
        assert raises(LIMITER, scale_norm=norm, limiter=True) == \
            f"limiter=True needs scale_norm='lufs', got {norm!r}: the limiter serves the loudness target"
    for norm in SCALE_NORMS:
        assert raises(STATS, scale_norm=norm, return_stats=True) == \
            "return_stats=True needs limiter=True: the stats are the limiter's"
    # doubly and triply invalid: unknown scale_norm, then the limiter without 'lufs', then the stats without the limiter
    raises(UNKNOWN, scale_norm="rms", limiter=True)
    raises(UNKNOWN, scale_norm="rms", return_stats=True)
    raises(UNKNOWN, scale_norm="rms", limiter=True, return_stats=True)
    raises(LIMITER, scale_norm="max", limiter=True, return_stats=True)
    raises("unknown scale_norm 'prompt'", norms=("max", "lufs"), scale_norm="prompt", limiter=True, return_stats=True)
    # valid: every norm plain, 'lufs' with the limiter, with and without its stats; check() hands the stage back
    for kw in (dict(scale_norm="max"), dict(scale_norm="prompt"), dict(scale_norm="lufs"), dict(),
               dict(scale_norm="lufs", limiter=True), dict(scale_norm="lufs", limiter=True, return_stats=True),
               dict(scale_norm="lufs", limiter=True, ceiling_db=-2.0, lookahead_ms=5.0, limiter_passes=1,
                    target_lufs=-16.0)):
        stage = OutputStage(**kw)
        assert stage.check() is stage
    assert OutputStage(scale_norm="lufs", limiter=True).check(norms=("max", "lufs")).limiter


@pytest.mark.parametrize("name", ["tts", "tts_from_codes", "tts_from_prompt", "vc", "vc_batch", "super_resolution"])
def test_harness_defaults_are_the_dataclass_defaults(name):
    from megatts2_hierspeechpp_amd.output import OutputStage
    ps = inspect.signature(_harnesses()[name][0]).parameters
    for f in dataclasses.fields(OutputStage):
        assert ps[f.name].default == f.default and type(ps[f.name].default) is type(f.default), (name, f.name)


def test_pack_order_and_bare_single_result():
    from megatts2_hierspeechpp_amd.output import pack
    wav, audio, stats, codes = object(), object(), {"min_gain": None}, object()
    assert pack(wav) is wav
    assert pack(wav, (audio, False), (stats, False), (codes, False)) is wav
    for want in itertools.product((False, True), repeat=3):
        got = pack(wav, *zip((audio, stats, codes), want))
        expect = (wav, *(v for v, w in zip((audio, stats, codes), want) if w))
        if any(want):
            assert isinstance(got, tuple) and len(got) == len(expect) and all(g is e for g, e in zip(got, expect)), want
        else:
            assert got is wav
    lengths = object()
    assert pack(wav, (lengths, True), (audio, False), (None, True)) == (wav, lengths, None)   # a wanted None stays


def test_output_rate_and_gain():
    from megatts2_hierspeechpp_amd import inference_plm as IP, inference_vc as IV, output
    assert [output.output_rate(r) for r in (16000, 24000, 48000, 22050)] == [16000, 24000, 48000, 16000]
    assert IV.output_rate is output.output_rate
    assert output.OutputStage(scale_norm="max").gain(None) == 0.999
    assert output.OutputStage(scale_norm="lufs").gain(None) == 0.999
    assert output.OutputStage(scale_norm="lufs", limiter=True).gain(None) == 0.999
    # the names the tests, tools and benchmark helpers import stay where they were
    assert IP.SCALE_NORMS is output.SCALE_NORMS and IP.prompt_peak is output.prompt_peak
    for n in ("output_gain", "peak_int16", "check_limiter", "int16_rows", "write_wav"):
        assert callable(getattr(IP, n)), n
    assert callable(IV.output_length)
    assert IP.output_gain("max", None) == 0.999 and IP.output_gain("lufs", None) == 0.999


@pytest.mark.parametrize("name", ["tts", "tts_from_codes", "tts_from_prompt", "tts_from_prompt_file", "vc", "vc_batch",
                                  "vc_batch_files", "super_resolution"])
def test_every_harness_rejects_a_bad_stage_before_touching_an_argument(name):
    """None for every model, tensor and path: whatever looked at one of them would raise something else."""
    from megatts2_hierspeechpp_amd import _lib
    fn, n_args = _harnesses()[name]
    args = (None,) * n_args
    with pytest.raises(_lib.HspError, match=UNKNOWN):
        fn(*args, scale_norm="rms")
    with pytest.raises(_lib.HspError, match=UNKNOWN):                      # the single order, in every harness
        fn(*args, scale_norm="rms", limiter=True, return_stats=True)
    with pytest.raises(_lib.HspError, match=LIMITER):
        fn(*args, scale_norm="max", limiter=True, return_stats=True)
    with pytest.raises(_lib.HspError, match=STATS):
        fn(*args, scale_norm="lufs", return_stats=True)
    if name == "super_resolution":
        with pytest.raises(_lib.HspError, match=r"unknown scale_norm 'prompt' \('max' or 'lufs'\)"):
            fn(*args, scale_norm="prompt", limiter=True)
