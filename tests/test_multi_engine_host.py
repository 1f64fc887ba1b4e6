"""CPU: XTTSv2Engine over several (fake) engines through the TTS facade -- ordering, stream == non-stream, spread, lazy voice
registration, cancellation in the placer's queue and on the engines, one engine dying -- and the ABI facts of aur_get_load."""
import asyncio
import ctypes
import json
import re

import numpy as np
import pytest

from auralis_amd import TTS, TTSRequest
from auralis_amd.api.text import XTTSTokenizer
from auralis_amd.api.xtts_engine import XTTSv2Engine
from tests.fakes_multi import FakeLoadEngine
from tests.test_abi import ROOT, _declared_symbols

COND = {"gpt_cond_latent": np.zeros((1, 32, 1024), np.float32), "speaker_embedding": np.ones((1, 512, 1), np.float32)}
COND_B = {"gpt_cond_latent": np.ones((1, 32, 1024), np.float32), "speaker_embedding": np.zeros((1, 512, 1), np.float32)}
PARA = ("The quick brown fox jumps over the lazy dog near the river bank. It was a bright cold day in April, and the "
        "clocks were striking thirteen! Who would have thought that such a thing could happen? Nobody, really; yet "
        "here we are, walking slowly along the old road, counting the stones and the years that went by.")


def _tts(fakes, concurrency=3):
    eng = XTTSv2Engine(list(fakes), XTTSTokenizer(None, synthetic=True), max_concurrency=concurrency)
    return TTS(scheduler_max_concurrency=concurrency).with_engine(eng), eng


def _marks(arr):
    """the constant runs of a fake waveform: one value (the chunk's seed) per chunk"""
    arr = np.asarray(arr)
    return [float(v) for v in arr[np.r_[True, np.diff(arr) != 0]]]


def _flush(tts):
    """everything queued on the facade's loop so far (cancellations travel as callbacks) has run"""
    for _ in range(3):
        tts._submit(asyncio.sleep(0)).result(timeout=5)


def _settled(eng, timeout=10.0):
    """A result reaches its consumer BEFORE the driver thread runs the placer's hook (EngineDriver.submit_for), and cancelled sequences
    come back through poll() later still: wait until every driver has handed back what it held and the placer has been told."""
    import time
    deadline = time.time() + timeout
    while time.time() < deadline:
        with eng._placer_lock:
            if not any(d._pending or d._on_resolved for d in eng.drivers) and not any(eng._placer.outstanding) and not eng._placer.queued():
                return
        time.sleep(0.001)
    raise AssertionError(f"did not settle: outstanding {eng._placer.outstanding}, queued {eng._placer.queued()}")


def test_one_engine_does_not_go_through_the_placer():
    for arg in (FakeLoadEngine(), [FakeLoadEngine()]):
        eng = XTTSv2Engine(arg, XTTSTokenizer(None, synthetic=True))
        try:
            assert eng._placer is None and eng.natives == [eng.native] and eng.drivers == [eng.driver]
        finally:
            eng.driver.shutdown()


@pytest.mark.parametrize("n_engines", [2, 3])
def test_chunks_come_back_in_order_and_stream_equals_non_stream(n_engines):
    fakes = [FakeLoadEngine(max_seqs=2) for _ in range(n_engines)]
    tts, eng = _tts(fakes)
    try:
        assert eng.natives == fakes and len(eng.drivers) == n_engines and eng.native is fakes[0] and eng.driver is eng.drivers[0]
        text = " ".join([PARA] * 6)
        n_chunks = len(eng.tokenizer.batch_encode_with_split(text, "en"))
        assert n_chunks >= 2 * n_engines
        out = tts.generate_speech(TTSRequest(text=text, speaker_files=[COND], language="en", seed=100))
        assert _marks(out.array) == [100.0 + i for i in range(n_chunks)]          # seeds are request seed + chunk index, in order
        assert all(len(f.submitted) > 0 for f in fakes)                           # every engine received work
        assert sorted(s["seed"] for f in fakes for s in f.submitted) == [100 + i for i in range(n_chunks)]   # each chunk once
        chunks = list(tts.generate_speech(TTSRequest(text=text, speaker_files=[COND], language="en", seed=100, stream=True)))
        assert len(chunks) == n_chunks and np.array_equal(np.concatenate([c.array for c in chunks]), out.array)
        # several requests at once, each in its own order
        async def many():
            return await asyncio.gather(*[tts.generate_speech_async(
                TTSRequest(text=" ".join([PARA] * 3), speaker_files=[COND], language="en", seed=1000 * (k + 1))) for k in range(5)])
        for k, o in enumerate(tts._submit(many()).result(timeout=30)):
            m = _marks(o.array)
            assert m == [1000.0 * (k + 1) + i for i in range(len(m))] and len(m) >= 3
        _settled(eng)
        assert eng._placer.queued() == 0 and eng._placer.outstanding == [0] * n_engines
        assert eng.load() == [{"waiting": 0, "running": 0, "vocoding": 0, "free_slots": 2, "token_budget": 0}] * n_engines
        assert len(eng.get_memory_usage_curve()["engines"]) == n_engines
    finally:
        tts.close()


def test_speed_and_priority_travel_with_the_chunk():
    fakes = [FakeLoadEngine(max_seqs=2) for _ in range(2)]
    tts, eng = _tts(fakes)
    try:
        tts.generate_speech(TTSRequest(text=" ".join([PARA] * 3), speaker_files=[COND], language="en", seed=5, speed=1.25, priority=1))
        subs = sorted((s for f in fakes for s in f.submitted), key=lambda s: s["seed"])
        assert [s["priority"] for s in subs] == [1] + [0] * (len(subs) - 1)
        assert all(s["speed"] == 1.25 for s in subs)
    finally:
        tts.close()


def test_a_voice_is_registered_only_where_its_chunks_ran():
    fakes = [FakeLoadEngine(max_seqs=2) for _ in range(3)]
    tts, eng = _tts(fakes)
    try:
        tts.generate_speech(TTSRequest(text="Only one short chunk for this voice.", speaker_files=[COND_B], language="en", seed=1))
        assert sum(len(f.speakers) for f in fakes) == 1
        tts.generate_speech(TTSRequest(text=" ".join([PARA] * 6), speaker_files=[COND], language="en", seed=2))
        for f in fakes:
            assert set(f.speakers) == {s["speaker_key"] for s in f.submitted}
        assert sum(len(f.speakers) for f in fakes) == 4      # voice A everywhere, voice B on the one engine that ran it
    finally:
        tts.close()


def test_a_consumer_that_closes_its_stream_cancels_queued_and_placed_chunks():
    fakes = [FakeLoadEngine(max_seqs=1, step_delay=0.01) for _ in range(2)]   # backlog 2 each: most of the request waits in the placer
    tts, eng = _tts(fakes)
    try:
        text = " ".join([PARA] * 12)
        n_chunks = len(eng.tokenizer.batch_encode_with_split(text, "en"))
        assert n_chunks >= 12      # four fit on the engines at a time
        gen = tts.generate_speech(TTSRequest(text=text, speaker_files=[COND], language="en", seed=1, stream=True))
        first = next(gen)
        assert _marks(first.array) == [1.0]
        gen.close()
        _flush(tts)
        placed = sum(len(f.submitted) for f in fakes)
        assert placed < n_chunks and eng._placer.queued() == 0        # the rest left the placer's queue; no engine saw them
        assert sum(len(f.cancelled) for f in fakes) >= 1              # ... and what was on an engine was stopped there
        _settled(eng)                                                 # the cancelled sequences have come back through poll()
        assert sum(len(f.submitted) for f in fakes) == placed         # nothing was placed meanwhile
        out = tts.generate_speech(TTSRequest(text=PARA, speaker_files=[COND], language="en", seed=50))
        assert _marks(out.array)[0] == 50.0
        assert sum(len(f.submitted) for f in fakes) - placed == len(_marks(out.array))
        _settled(eng)
        assert eng._placer.outstanding == [0, 0]
    finally:
        tts.close()


def test_a_failing_engine_stops_only_its_own_driver():
    good, bad = FakeLoadEngine(max_seqs=2), FakeLoadEngine(max_seqs=2, fail_on_step=1)
    tts, eng = _tts([good, bad])
    try:
        with pytest.raises(RuntimeError):
            tts.generate_speech(TTSRequest(text=" ".join([PARA] * 3), speaker_files=[COND], language="en", seed=1))
        assert len(bad.submitted) >= 1
        n_bad = len(bad.submitted)
        for k in range(3):
            out = tts.generate_speech(TTSRequest(text=" ".join([PARA] * 3), speaker_files=[COND], language="en", seed=10 * (k + 1)))
            m = _marks(out.array)
            assert m == [10.0 * (k + 1) + i for i in range(len(m))] and len(m) >= 3
        _settled(eng)
        assert eng.drivers[0]._error is None and eng.drivers[1]._error is not None
        assert len(bad.submitted) == n_bad and eng._placer.engines_alive() == [0]
    finally:
        tts.close()


def test_shutdown_fails_what_still_waits_in_the_placer():
    fakes = [FakeLoadEngine(max_seqs=1, step_delay=0.02) for _ in range(2)]
    tts, eng = _tts(fakes)
    try:
        pending = tts._submit(tts.generate_speech_async(TTSRequest(text=" ".join([PARA] * 12), speaker_files=[COND], language="en", seed=1)))
        deadline = __import__("time").time() + 10
        while not eng._placer.queued() and __import__("time").time() < deadline:
            __import__("time").sleep(0.001)
        assert eng._placer.queued() > 0
        tts._submit(eng.shutdown()).result(timeout=10)
        with pytest.raises(RuntimeError):
            pending.result(timeout=10)          # ... instead of waiting for ever for chunks nobody will place
        assert eng._placer.queued() == 0 and eng._placer.engines_alive() == []
    finally:
        tts.close()


def test_device_and_devices_exclude_each_other(tmp_path):
    with pytest.raises(ValueError, match="devices"):
        XTTSv2Engine.from_pretrained(str(tmp_path), device=0, devices=[0, 1])
    (tmp_path / "config.json").write_text(json.dumps({"model_type": "xtts"}))
    with pytest.raises(ValueError, match="devices"):
        TTS().from_pretrained(str(tmp_path), device=1, devices=[0])
    with pytest.raises(ValueError, match="devices"):
        XTTSv2Engine.from_pretrained(str(tmp_path), devices=[])


def test_server_devices_argument():
    import argparse

    from auralis_amd.entrypoints.oai_server import _device_list
    assert _device_list("0,1,2,3") == [0, 1, 2, 3] and _device_list("0,0") == [0, 0]
    for bad in ("", "a,b", "0,-1"):
        with pytest.raises(argparse.ArgumentTypeError):
            _device_list(bad)


# ------------------------------------------------------------------------------------------------ aur_get_load: ABI
def test_aur_get_load_is_in_header_binding_and_library(lib_path):
    from auralis_amd import _lib
    assert "aur_get_load" in _declared_symbols() and "aur_get_load" in _lib.EXPORTS
    assert hasattr(ctypes.CDLL(lib_path), "aur_get_load") and hasattr(_lib.NativeEngine, "load")
    src = re.sub(r"/\*.*?\*/", "", open(ROOT + "/include/auralis_amd.h").read(), flags=re.S)
    body = re.search(r"typedef struct aur_load \{(.*?)\} aur_load;", src, re.S).group(1)
    fields = [d.strip().split()[-1] for d in body.split(";") if d.strip()]
    assert fields == [f for f, _ in _lib.aur_load._fields_] == ["waiting", "running", "vocoding", "free_slots", "token_budget"]
    assert ctypes.sizeof(_lib.aur_load) == 24


def test_aur_get_load_rejects_null_arguments(lib_path):
    from auralis_amd import _lib
    lib = _lib.load_library()
    out = _lib.aur_load()
    assert lib.aur_get_load(None, ctypes.byref(out)) == -1        # AUR_E_INVALID
    assert b"null argument" in lib.aur_last_error()
