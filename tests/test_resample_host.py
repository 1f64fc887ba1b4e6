"""CPU: the output sample rate on the host side -- TTSRequest.output_sample_rate, the binding's structs, its way to the engine's
submit for every chunk, the label of the TTSOutput, split_requests, and the server's field, default and error envelope -- with a fake
engine."""
import base64
import io
import sys
import types
import wave

import numpy as np
import pytest

from auralis_amd import TTS, TTSRequest
from auralis_amd.api.text import XTTSTokenizer
from auralis_amd.api.xtts_engine import XTTSv2Engine
from tests.fakes import FakeNativeEngine

COND = {"gpt_cond_latent": np.zeros((1, 32, 1024), np.float32), "speaker_embedding": np.ones((1, 512, 1), np.float32)}
PARA = ("The quick brown fox jumps over the lazy dog near the river bank. It was a bright cold day in April, and the "
        "clocks were striking thirteen! Who would have thought that such a thing could happen? Nobody, really; yet "
        "here we are, walking slowly along the old road, counting the stones and the years that went by.")
RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000)


class RateFake(FakeNativeEngine):
    """the fake with NativeEngine.submit's `sample_rate` keyword and the poll dict's "sample_rate"; `rates` records what arrived
    (None: the keyword was not passed)"""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.rates = []
        self._rate_of = {}

    def submit(self, *a, sample_rate=None, **kw):
        self.rates.append(sample_rate)
        sid = super().submit(*a, **kw)
        self._rate_of[sid] = sample_rate or 24000
        return sid

    def poll(self, *a, **kw):
        out = super().poll(*a, **kw)
        for item in out:
            item["sample_rate"] = self._rate_of.get(item["seq_id"], 24000)
        return out


def _tts(fake):
    return TTS(scheduler_max_concurrency=3).with_engine(XTTSv2Engine(fake, XTTSTokenizer(None, synthetic=True), max_concurrency=3))


def test_request_validates_output_sample_rate():
    assert TTSRequest(text="hi", speaker_files="x", language="en").output_sample_rate == 24000
    for ok in RATES:
        assert TTSRequest(text="hi", speaker_files="x", language="en", output_sample_rate=ok).output_sample_rate == ok
    for bad in (0, 12345, -1, 96000, 11025, 16000.0, "16000", None, True, float("nan")):
        with pytest.raises(ValueError):
            TTSRequest(text="hi", speaker_files="x", language="en", output_sample_rate=bad)
    r = TTSRequest(text="hi", speaker_files="x", language="en", output_sample_rate=8000)
    assert r.copy().output_sample_rate == 8000


def test_binding_structs_carry_the_rate():
    from auralis_amd import _lib
    names = [f for f, _ in _lib.aur_seq_desc._fields_]
    assert names[-2:] == ["sample_rate", "speed"] and names[-3] == "priority"      # directly before speed, which stays last
    assert _lib.aur_result._fields_[-1][0] == "sample_rate"
    assert _lib.aur_seq_desc().sample_rate == 0                                        # a zeroed descriptor is "unset"
    assert "aur_vocode_rate" in _lib.EXPORTS and "aur_dbg_resample_out" in _lib.EXPORTS
    assert [_lib.samples_out(700, r) for r in RATES] == [234, 467, 644, 700, 934, 1287, 1400]
    assert _lib.samples_out(700) == _lib.samples_out(700, 0) == 700
    with pytest.raises(ValueError):
        _lib.samples_out(700, 12345)


def test_rate_reaches_submit_for_every_chunk_and_labels_the_output():
    fake = RateFake(max_seqs=3)
    tts = _tts(fake)
    try:
        out = tts.generate_speech(TTSRequest(text=" ".join([PARA] * 3), speaker_files=[COND], language="en", output_sample_rate=16000))
        assert len(fake.submitted) >= 3 and fake.rates == [16000] * len(fake.submitted)
        assert out.sample_rate == 16000
        chunks = list(tts.generate_speech(TTSRequest(text=" ".join([PARA] * 3), speaker_files=[COND], language="en",
                                                     output_sample_rate=48000, stream=True)))
        assert len(chunks) >= 3 and all(c.sample_rate == 48000 for c in chunks)
        n = len(fake.submitted)
        out = tts.generate_speech(TTSRequest(text=" ".join([PARA] * 2), speaker_files=[COND], language="en"))
        assert len(fake.submitted) > n and fake.rates[n:] == [None] * (len(fake.submitted) - n)   # 24000: the keyword is left out
        assert out.sample_rate == 24000
        with wave.open(io.BytesIO(tts.generate_speech(TTSRequest(text=PARA, speaker_files=[COND], language="en",
                                                                 output_sample_rate=8000)).to_bytes("wav"))) as w:
            assert w.getframerate() == 8000
    finally:
        tts.close()


def test_24000_works_with_an_engine_that_has_no_rate_keyword():
    tts = _tts(FakeNativeEngine(max_seqs=3))
    try:
        out = tts.generate_speech(TTSRequest(text=PARA, speaker_files=[COND], language="en", output_sample_rate=24000))
        assert len(out.array) > 0 and out.sample_rate == 24000        # and a poll dict without "sample_rate" means 24000
    finally:
        tts.close()


def test_rate_reaches_every_engine_of_a_pool():
    from tests.fakes_multi import FakeLoadEngine

    class PoolFake(RateFake, FakeLoadEngine):      # + load() (aur_get_load) and submit's `speed`, what the several-engine path needs
        pass
    fakes = [PoolFake(max_seqs=2), PoolFake(max_seqs=2)]
    tts = TTS(scheduler_max_concurrency=4).with_engine(XTTSv2Engine(fakes, XTTSTokenizer(None, synthetic=True), max_concurrency=2))
    try:
        out = tts.generate_speech(TTSRequest(text=" ".join([PARA] * 4), speaker_files=[COND], language="en", output_sample_rate=44100))
        got = fakes[0].rates + fakes[1].rates
        assert len(got) >= 4 and got == [44100] * len(got) and out.sample_rate == 44100
    finally:
        tts.close()


def test_split_requests_keeps_the_rate():
    r = TTSRequest(text="a" * 250, speaker_files="x", language="en", output_sample_rate=32000, speed=0.75)
    subs = TTS.split_requests(r, max_length=100)
    assert [len(s.text) for s in subs] == [100, 100, 50]
    assert [s.output_sample_rate for s in subs] == [32000] * 3 and [s.speed for s in subs] == [0.75] * 3


# ---- the server ----
fastapi_testclient = pytest.importorskip("fastapi.testclient")


def _npz_voice():
    buf = io.BytesIO()
    np.savez(buf, gpt_cond_latent=np.zeros((1, 32, 1024), np.float32), speaker_embedding=np.ones((1, 512, 1), np.float32))
    return base64.b64encode(buf.getvalue()).decode()


def _post(app_kw, fake, sample_rate):
    from auralis_amd.entrypoints.oai_server import create_app
    tts = _tts(fake)
    try:
        client = fastapi_testclient.TestClient(create_app(tts, **app_kw))
        body = {"input": PARA, "model": "xtts", "voice": [_npz_voice()], "response_format": "wav", "language": "en"}
        if sample_rate is not None:
            body["sample_rate"] = sample_rate
        return client.post("/v1/audio/speech", json=body)
    finally:
        tts.close()


def _wav_rate(content):
    with wave.open(io.BytesIO(content)) as w:
        return w.getframerate()


def test_server_field_default_and_error_envelope():
    from auralis_amd.entrypoints import oai_server
    fake = RateFake(max_seqs=2)
    r = _post({}, fake, 16000)
    assert r.status_code == 200 and _wav_rate(r.content) == 16000 and fake.rates == [16000] * len(fake.submitted) and fake.rates
    fake = RateFake(max_seqs=2)
    r = _post({}, fake, None)                                            # no field, no default: 24000, the engine is not told
    assert r.status_code == 200 and _wav_rate(r.content) == 24000 and fake.rates == [None] * len(fake.submitted)
    r = _post({}, FakeNativeEngine(max_seqs=2), None)                    # ... so an engine without the keyword serves it
    assert r.status_code == 200 and _wav_rate(r.content) == 24000
    fake = RateFake(max_seqs=2)
    r = _post({"sample_rate": 8000}, fake, None)                         # the server's default
    assert r.status_code == 200 and _wav_rate(r.content) == 8000 and fake.rates == [8000] * len(fake.submitted)
    fake = RateFake(max_seqs=2)
    r = _post({"sample_rate": 8000}, fake, 48000)                        # the request's field wins
    assert r.status_code == 200 and _wav_rate(r.content) == 48000 and fake.rates == [48000] * len(fake.submitted)
    fake = RateFake(max_seqs=2)
    r = _post({}, fake, 12345)                                           # the reference's envelope, nothing submitted
    assert r.status_code == 500 and r.json()["error"].startswith("Error generating audio:") and "output_sample_rate" in r.json()["error"]
    assert fake.submitted == []
    with pytest.raises(ValueError):
        oai_server.create_app(None, sample_rate=11025)
    assert "sample_rate" in oai_server._TTS_FIELDS
    chat = oai_server.VoiceChatCompletionRequest(model="m", messages=[], speaker_files=[_npz_voice()], openai_api_url="http://x",
                                                 sample_rate=22050)
    assert chat.to_tts_request("hi").output_sample_rate == 22050 and "sample_rate" not in chat.to_openai_request()
    chat = oai_server.VoiceChatCompletionRequest(model="m", messages=[], speaker_files=[_npz_voice()], openai_api_url="http://x")
    assert chat.to_tts_request("hi").output_sample_rate == 24000 and chat.to_tts_request("hi", sample_rate=16000).output_sample_rate == 16000


def test_server_cli_default(monkeypatch):
    """--sample-rate: 24000 unless given, handed to create_app; an unsupported value stops the parser"""
    from auralis_amd.entrypoints import oai_server
    seen = {}

    class StubTTS:
        def __init__(self, **kw):
            pass

        def from_pretrained(self, *a, **kw):
            return self
    monkeypatch.setitem(sys.modules, "uvicorn", types.SimpleNamespace(run=lambda app, **kw: seen.update(app=app)))
    monkeypatch.setattr(oai_server, "TTS", StubTTS)
    monkeypatch.setattr(sys, "argv", ["oai_server", "--model", "/nowhere"])
    oai_server.main()
    assert seen["app"].state.sample_rate == 24000
    monkeypatch.setattr(sys, "argv", ["oai_server", "--model", "/nowhere", "--sample-rate", "16000"])
    oai_server.main()
    assert seen["app"].state.sample_rate == 16000
    monkeypatch.setattr(sys, "argv", ["oai_server", "--model", "/nowhere", "--sample-rate", "12345"])
    with pytest.raises(SystemExit):
        oai_server.main()
