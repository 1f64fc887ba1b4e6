"""CPU: the speaking rate on the host side -- TTSRequest.speed, its way to the engine's submit for every chunk, split_requests, and
the server's two speed modes -- with a fake engine."""
import base64
import io

import numpy as np
import pytest

from auralis_amd import TTS, TTSOutput, TTSRequest
from auralis_amd.api.text import XTTSTokenizer
from auralis_amd.api.xtts_engine import XTTSv2Engine
from tests.fakes import FakeNativeEngine

COND = {"gpt_cond_latent": np.zeros((1, 32, 1024), np.float32), "speaker_embedding": np.ones((1, 512, 1), np.float32)}
PARA = ("The quick brown fox jumps over the lazy dog near the river bank. It was a bright cold day in April, and the "
        "clocks were striking thirteen! Who would have thought that such a thing could happen? Nobody, really; yet "
        "here we are, walking slowly along the old road, counting the stones and the years that went by.")
TEXT = " ".join([PARA] * 4)   # long enough for change_speed's 2048-sample STFT window on the fake's ten samples per token


class SpeedFake(FakeNativeEngine):
    """the fake with NativeEngine.submit's `speed` keyword; `speeds` records what arrived (None: the keyword was not passed)"""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.speeds = []

    def submit(self, *a, speed=None, **kw):
        self.speeds.append(speed)
        return super().submit(*a, **kw)


def _tts(fake):
    return TTS(scheduler_max_concurrency=3).with_engine(XTTSv2Engine(fake, XTTSTokenizer(None, synthetic=True), max_concurrency=3))


def test_request_validates_speed():
    assert TTSRequest(text="hi", speaker_files="x", language="en").speed == 1.0
    for ok in (0.5, 0.75, 1, 1.25, 2.0):
        assert TTSRequest(text="hi", speaker_files="x", language="en", speed=ok).speed == ok
    for bad in (0.0, 0.4, 0.49999, 2.0001, 3, -1.0, float("nan"), float("inf"), -float("inf"), None, "fast"):
        with pytest.raises(ValueError):
            TTSRequest(text="hi", speaker_files="x", language="en", speed=bad)


def test_binding_struct_carries_speed_last():
    from auralis_amd import _lib
    assert _lib.aur_seq_desc._fields_[-1][0] == "speed"
    d = _lib.aur_seq_desc()
    assert d.speed == 0.0   # a zeroed descriptor is "unset"


def test_speed_reaches_submit_for_every_chunk():
    fake = SpeedFake(max_seqs=3)
    tts = _tts(fake)
    try:
        tts.generate_speech(TTSRequest(text=" ".join([PARA] * 3), speaker_files=[COND], language="en", speed=1.25, priority=1))
        assert len(fake.submitted) >= 3 and fake.speeds == [1.25] * len(fake.submitted)
        assert [s["priority"] for s in fake.submitted] == [1] + [0] * (len(fake.submitted) - 1)
        n = len(fake.submitted)
        tts.generate_speech(TTSRequest(text=" ".join([PARA] * 2), speaker_files=[COND], language="en"))
        assert len(fake.submitted) > n and fake.speeds[n:] == [None] * (len(fake.submitted) - n)   # speed 1: the keyword is left out
    finally:
        tts.close()


def test_speed_one_works_with_an_engine_that_has_no_speed_keyword():
    tts = _tts(FakeNativeEngine(max_seqs=3))
    try:
        assert len(tts.generate_speech(TTSRequest(text=PARA, speaker_files=[COND], language="en", speed=1.0)).array) > 0
    finally:
        tts.close()


def test_split_requests_keeps_speed_and_zeroes_priority_after_the_first():
    r = TTSRequest(text="a" * 250, speaker_files="x", language="en", speed=0.75, priority=2, temperature=0.3)
    subs = TTS.split_requests(r, max_length=100)
    assert [len(s.text) for s in subs] == [100, 100, 50]
    assert [s.speed for s in subs] == [0.75] * 3 and [s.temperature for s in subs] == [0.3] * 3
    assert [s.priority for s in subs] == [2, 0, 0]
    assert r.priority == 2 and len({s.request_id for s in subs}) == 3
    assert TTS.split_requests(r)[0] is r and r.priority == 2   # a text that is not split is the request itself, untouched


# ---- the server's two modes ----
fastapi_testclient = pytest.importorskip("fastapi.testclient")


def _npz_voice():
    buf = io.BytesIO()
    np.savez(buf, gpt_cond_latent=np.zeros((1, 32, 1024), np.float32), speaker_embedding=np.ones((1, 512, 1), np.float32))
    return base64.b64encode(buf.getvalue()).decode()


def _post(app_args, fake, speed):
    from auralis_amd.entrypoints.oai_server import create_app
    tts = _tts(fake)
    try:
        client = fastapi_testclient.TestClient(create_app(tts, *app_args))
        body = {"input": TEXT, "model": "xtts", "voice": [_npz_voice()], "response_format": "wav",
                "language": "en"}
        if speed is not None:
            body["speed"] = speed
        r = client.post("/v1/audio/speech", json=body)
        assert r.status_code == 200, r.text
        return r.content
    finally:
        tts.close()


def test_server_latent_mode_sets_the_field_and_skips_change_speed(monkeypatch):
    def boom(self, f):
        raise AssertionError("change_speed called in latent mode")
    monkeypatch.setattr(TTSOutput, "change_speed", boom)
    plain = _post((), SpeedFake(max_seqs=2), None)
    for sent, want in ((1.25, 1.25), (0.25, 0.5), (4.0, 2.0), (0.5, 0.5)):   # the OpenAI range is [0.25, 4]: clamped to the engine's
        fake = SpeedFake(max_seqs=2)
        got = _post(("latent",), fake, sent)
        assert fake.speeds == [want] * len(fake.submitted) and fake.speeds
        assert got == plain          # the fake's audio does not depend on speed: the waveform went out as the engine made it
    fake = SpeedFake(max_seqs=2)
    assert _post(("latent",), fake, 1.0) == plain and fake.speeds == [None] * len(fake.submitted)


def test_server_stretch_mode_is_what_it_was():
    """default = "stretch": the engine is not told (a fake without the keyword serves it) and the waveform goes through change_speed"""
    from auralis_amd.entrypoints.oai_server import create_app
    with pytest.raises(ValueError):
        create_app(None, "faster")
    plain = _post((), FakeNativeEngine(max_seqs=2), None)
    for speed in (1.5, 0.75):
        a = _post((), FakeNativeEngine(max_seqs=2), speed)
        b = _post(("stretch",), FakeNativeEngine(max_seqs=2), speed)
        assert a == b and a != plain
        # the same bytes as the facade's output put through change_speed by hand
        tts = _tts(FakeNativeEngine(max_seqs=2))
        try:
            out = tts.generate_speech(TTSRequest(text=TEXT, speaker_files=[COND], language="en"))
            assert out.change_speed(speed).to_bytes("wav") == a
        finally:
            tts.close()
    assert _post(("stretch",), FakeNativeEngine(max_seqs=2), 1.0) == plain
