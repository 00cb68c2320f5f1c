"""Host checks (no GPU) of the batched TTS harness of inference_plm: the chunk planner `line_chunks` / `chunk_order`, the
join plan `join_plan`, and every argument error of `tts_batch` / `tts_lines` / `tts_batch_files`, raised with
``models=None`` -- i.e. before any model or device is touched -- and after the output stage's own check."""
import numpy as np
import pytest
import torch

from megatts2_hierspeechpp_amd import _lib as L
from megatts2_hierspeechpp_amd import inference_plm as IP


# ------------------------------------------------------------------------------------------------ planner
@pytest.mark.parametrize("max_batch", [1, 2, 3, 5, 16])
def test_line_chunks_cover_every_line_once(max_batch):
    counts = [int(v) for v in np.random.default_rng(1).integers(1, 40, 13)]
    chunks = IP.line_chunks(counts, max_batch)
    flat = [k for rows in chunks for k in rows]
    assert sorted(flat) == list(range(13))
    assert all(1 <= len(rows) <= max_batch for rows in chunks)
    assert len(chunks) == -(-13 // max_batch)
    assert [counts[k] for k in flat] == sorted(counts)                    # sorted by phone count


def test_line_chunks_sort_is_stable():
    counts = [5, 3, 5, 3, 5, 1]
    assert IP.line_chunks(counts, 2) == [[5, 1], [3, 0], [2, 4]]          # equal counts keep the caller's order
    assert IP.line_chunks(counts, 6) == [[5, 1, 3, 0, 2, 4]]
    assert IP.line_chunks([], 4) == []


def test_chunk_order_restores_the_callers_order():
    counts = [9, 2, 7, 2, 30, 1, 7]
    for max_batch in (1, 2, 3, 7):
        chunks = IP.line_chunks(counts, max_batch)
        flat = [k for rows in chunks for k in rows]
        inv = IP.chunk_order(chunks)
        assert [flat[i] for i in inv] == list(range(len(counts)))


def test_line_chunks_refuses_max_batch_below_one():
    with pytest.raises(L.HspError, match="max_batch"):
        IP.line_chunks([3, 4], 0)


# ------------------------------------------------------------------------------------------------ join plan
@pytest.mark.parametrize("rate", [16000, 24000, 48000])
def test_join_plan_offsets_and_total(rate):
    lengths = [14 * 320 * rate // 16000, 19 * 320 * rate // 16000, 5 * 320 * rate // 16000]
    pause_ms = 12.34
    pause = round(pause_ms * rate / 1000)
    assert pause == {16000: 197, 24000: 296, 48000: 592}[rate]
    offsets, total = IP.join_plan(lengths, rate, pause_ms)
    assert offsets == [0, lengths[0] + pause, lengths[0] + lengths[1] + 2 * pause]
    assert total == sum(lengths) + 2 * pause
    assert IP.join_plan(lengths[:1], rate, pause_ms) == ([0], lengths[0])  # one line: no pause
    assert IP.join_plan([], rate, pause_ms) == ([], 0)
    assert IP.join_plan(lengths, rate, 0.0) == ([0, lengths[0], lengths[0] + lengths[1]], sum(lengths))


def test_join_plan_refuses_a_negative_pause():
    with pytest.raises(L.HspError, match="pause_ms"):
        IP.join_plan([10, 10], 16000, -1.0)


# ------------------------------------------------------------------------------------------------ argument errors
def _line(n, lang_n=None, tone_n=None):
    return (torch.ones(n, dtype=torch.int64), torch.zeros(n if tone_n is None else tone_n, dtype=torch.int64),
            torch.ones(1, n if lang_n is None else lang_n, dtype=torch.int64))


PROMPT = torch.zeros(2000)
LINES = [_line(4), _line(6), _line(3)]

ERRORS = [
    ("dur of another count", dict(dur=[torch.ones(4), torch.ones(6)]), "dur"),
    ("durations that do not fit their line", dict(dur=[torch.ones(4), torch.ones(5), torch.ones(3)]), "durations"),
    ("plm_prefixes of another count", dict(plm_prefixes=[torch.zeros(2, dtype=torch.int64)], plm_causal=True),
     "plm_prefixes"),
    ("plm_prefixes without plm_causal", dict(plm_prefixes=[torch.zeros(2, dtype=torch.int64)] * 3), "plm_causal"),
    ("prosody_codes of another count", dict(prosody_codes=[torch.zeros(8, dtype=torch.int64)] * 2), "prosody_codes"),
    ("prosody_codes with plm_causal", dict(prosody_codes=[torch.zeros(8, dtype=torch.int64)] * 3, plm_causal=True),
     "exclude each other"),
    ("prosody_codes with plm_sampling", dict(prosody_codes=[torch.zeros(8, dtype=torch.int64)] * 3,
                                             plm_sampling=object()), "exclude each other"),
    ("prosody_codes with plm_prefixes", dict(prosody_codes=[torch.zeros(8, dtype=torch.int64)] * 3, plm_causal=True,
                                             plm_prefixes=[torch.zeros(2, dtype=torch.int64)] * 3),
     "exclude each other"),
    ("prosody_lengths without prosody_codes", dict(prosody_lengths=[8, 8, 8]), "prosody_lengths"),
]


@pytest.mark.parametrize("fn", [IP.tts_batch, IP.tts_lines])
@pytest.mark.parametrize("what,kw,match", ERRORS, ids=[e[0] for e in ERRORS])
def test_keyword_errors_before_any_device_work(fn, what, kw, match):
    with pytest.raises(L.HspError, match=match):
        fn(None, None, LINES, PROMPT, **kw)


@pytest.mark.parametrize("fn", [IP.tts_batch, IP.tts_lines])
def test_line_and_prompt_errors_before_any_device_work(fn):
    with pytest.raises(L.HspError, match="empty"):
        fn(None, None, [_line(4), _line(0)], PROMPT)
    with pytest.raises(L.HspError, match="non-empty list"):
        fn(None, None, [], PROMPT)
    with pytest.raises(L.HspError, match="different lengths"):
        fn(None, None, [_line(4), _line(5, lang_n=4)], PROMPT)
    with pytest.raises(L.HspError, match="different lengths"):
        fn(None, None, [_line(4, tone_n=3)], PROMPT)
    with pytest.raises(L.HspError, match="438"):
        fn(None, None, [_line(439)], PROMPT)
    with pytest.raises(L.HspError, match="one prompt or one per line"):
        fn(None, None, LINES, [PROMPT, PROMPT])
    with pytest.raises(L.HspError, match="denoise_ratio"):
        fn(None, None, LINES, PROMPT, denoise_ratio=0.5)
    with pytest.raises(L.HspError, match="not both"):
        fn(None, None, LINES, PROMPT, denoise_ratio=0.5, denoised=PROMPT, denoiser=object(), hps_denoiser=object())


def test_tts_lines_own_errors():
    with pytest.raises(L.HspError, match="max_batch"):
        IP.tts_lines(None, None, LINES, PROMPT, max_batch=0)
    with pytest.raises(L.HspError, match="pause_ms"):
        IP.tts_lines(None, None, LINES, PROMPT, join=True, pause_ms=-0.5)
    with pytest.raises(L.HspError, match="programme has no single prompt"):
        IP.tts_lines(None, None, LINES, PROMPT, join=True, scale_norm="prompt")


@pytest.mark.parametrize("fn", [IP.tts_batch, IP.tts_lines, IP.tts_batch_files])
def test_output_stage_is_checked_first(fn):
    """The order the other harnesses keep: the stage's own errors come before every other one (here: an empty line
    and a wrong prompt count are present too)."""
    bad = [_line(4), _line(0)]
    with pytest.raises(L.HspError, match="unknown scale_norm"):
        fn(None, None, bad, [PROMPT] * 3, scale_norm="rms")
    with pytest.raises(L.HspError, match="limiter=True needs"):
        fn(None, None, bad, [PROMPT] * 3, limiter=True)
    with pytest.raises(L.HspError, match="return_stats=True needs"):
        fn(None, None, bad, [PROMPT] * 3, scale_norm="lufs", return_stats=True)


def test_tts_batch_files_errors_before_any_file_is_read(tmp_path, monkeypatch):
    from megatts2_hierspeechpp_amd import audio as A

    def no_load(path):
        raise AssertionError(f"{path} was read")

    monkeypatch.setattr(A, "load", no_load)
    missing = str(tmp_path / "missing.wav")
    with pytest.raises(L.HspError, match="one prompt file or one per line"):
        IP.tts_batch_files(None, None, LINES, [missing, missing])
    with pytest.raises(L.HspError, match="names"):
        IP.tts_batch_files(None, None, LINES, missing, names=["a", "b"])
    with pytest.raises(L.HspError, match="empty"):
        IP.tts_batch_files(None, None, [_line(4), _line(0)], missing)
    with pytest.raises(L.HspError, match="plm_causal"):
        IP.tts_batch_files(None, None, LINES, missing, plm_prefixes=[torch.zeros(2, dtype=torch.int64)] * 3)


def test_tts_and_tts_from_codes_take_the_new_keywords():
    import inspect
    for fn in (IP.tts, IP.tts_from_codes):
        p = inspect.signature(fn).parameters
        assert p["row_exact"].default is False and p["style"].default is None
    assert inspect.signature(IP.tts_batch).parameters  # importable
    with pytest.raises(L.HspError, match="unknown scale_norm"):
        IP.tts(None, *([None] * 8), scale_norm="rms", row_exact=True)
