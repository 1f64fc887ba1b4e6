"""CPU: FLAC on the host side -- the binding's symbols and struct fields, TTSRequest.output_encoding and its way to every chunk's
submit, TTSOutput.encoded and to_bytes, the server's route (never the host writer on the event loop) -- with fake engines; and the
proof, from the host writer's streams alone, that the batch of tests/test_gpu_flac.py reaches every path of the encoder."""
import base64
import io
import threading

import numpy as np
import pytest

from auralis_amd import TTS, TTSOutput, TTSRequest
from auralis_amd.api import flac
from auralis_amd.api.text import XTTSTokenizer
from auralis_amd.api.xtts_engine import XTTSv2Engine
from tests import flac_cases as fc
from tests.fakes import FakeNativeEngine

COND = {"gpt_cond_latent": np.zeros((1, 32, 1024), np.float32), "speaker_embedding": np.ones((1, 512, 1), np.float32)}
PARA = ("The quick brown fox jumps over the lazy dog near the river bank. It was a bright cold day in April, and the "
        "clocks were striking thirteen! Who would have thought that such a thing could happen? Nobody, really; yet "
        "here we are, walking slowly along the old road, counting the stones and the years that went by.")


# ------------------------------------------------------------------------------------------------ binding
def test_exports_and_new_struct_fields():
    from auralis_amd import _lib
    for name in ("aur_encode_flac", "aur_dbg_flac_encode", "aur_flac_bound"):
        assert name in _lib.EXPORTS
    # the new fields sit in front of the members other tests pin to the end of their struct (`speed`, `sample_rate`); nothing else moved
    assert [f for f, _ in _lib.aur_seq_desc._fields_][-5:] == ["ignore_stop", "encoding", "priority", "sample_rate", "speed"]
    assert [f for f, _ in _lib.aur_result._fields_][-4:] == ["error", "enc", "n_enc", "sample_rate"]
    assert _lib.aur_seq_desc().encoding == 0 and _lib.aur_result().n_enc == 0     # a zeroed descriptor encodes nothing
    assert _lib.ENCODINGS[None] == 0 and _lib.ENCODINGS["flac"] == 1
    assert hasattr(_lib.NativeEngine, "encode_flac") and hasattr(_lib.NativeEngine, "dbg_flac_encode")


# ------------------------------------------------------------------------------------------------ request
def test_request_validates_output_encoding_and_copies_carry_it():
    assert TTSRequest(text="hi", speaker_files="x", language="en").output_encoding is None
    r = TTSRequest(text="hi", speaker_files="x", language="en", output_encoding="flac")
    assert r.output_encoding == "flac" and r.copy().output_encoding == "flac"
    for bad in ("FLAC", "wav", "mp3", "", 1, True, b"flac"):
        with pytest.raises(ValueError):
            TTSRequest(text="hi", speaker_files="x", language="en", output_encoding=bad)
    big = TTSRequest(text="a" * 25, speaker_files="x", language="en", output_encoding="flac")
    parts = TTS.split_requests(big, max_length=10)
    assert len(parts) == 3 and all(p.output_encoding == "flac" for p in parts)


class EncFake(FakeNativeEngine):
    """the fake with NativeEngine's `encoding` keyword, the poll dict's "encoded" and the one-shot encode_flac; the streams are the host
    writer's (the real one, whatever a test patches in its place).  Records what arrived and the thread the one-shot entry ran on."""
    _host_writer = staticmethod(flac.encode)

    def __init__(self, **kw):
        super().__init__(**kw)
        self.encodings, self._enc_of, self.one_shot_threads = [], {}, []

    def submit(self, *a, encoding=None, **kw):
        self.encodings.append(encoding)
        sid = super().submit(*a, **kw)
        self._enc_of[sid] = encoding
        return sid

    def poll(self, *a, **kw):
        out = super().poll(*a, **kw)
        for item in out:
            if self._enc_of.get(item["seq_id"]) and len(item["wav"]):
                item["encoded"] = np.frombuffer(self._host_writer(fc.to_int(item["wav"]), 24000, 16), np.uint8)
                item["encoded_format"] = "flac"
        return out

    def encode_flac(self, arrays, rates):
        self.one_shot_threads.append(threading.get_ident())
        return [self._host_writer(fc.to_int(a), int(r), 16) for a, r in zip(arrays, rates)]


def _tts(fake):
    return TTS(scheduler_max_concurrency=3).with_engine(XTTSv2Engine(fake, XTTSTokenizer(None, synthetic=True), max_concurrency=3))


def test_every_chunk_is_submitted_with_the_encoding_and_the_keyword_is_left_out_when_unset():
    fake = EncFake(max_seqs=3)
    tts = _tts(fake)
    try:
        out = tts.generate_speech(TTSRequest(text=PARA, speaker_files=[COND], language="en", output_encoding="flac"))
        assert len(fake.encodings) >= 2 and set(fake.encodings) == {"flac"}
        assert out.encoded is None        # several chunks joined: no stream of the whole
        one = tts.generate_speech(TTSRequest(text="Hello there.", speaker_files=[COND], language="en", output_encoding="flac"))
        assert one.encoded_format == "flac" and one.to_bytes("flac") == flac.encode(fc.to_int(one.array), 24000, 16)
    finally:
        tts.close()
    plain = FakeNativeEngine(max_seqs=3)      # a double without the keyword keeps working while the field is unset
    tts = _tts(plain)
    try:
        assert tts.generate_speech(TTSRequest(text="Hello there.", speaker_files=[COND], language="en")).encoded is None
    finally:
        tts.close()


# ------------------------------------------------------------------------------------------------ output
def test_to_bytes_returns_the_engines_stream_and_transforms_drop_it(monkeypatch):
    x = (0.3 * np.sin(np.arange(3000) * 0.01)).astype(np.float32)
    stream = flac.encode(fc.to_int(x), 24000, 16)
    want24 = flac.encode(np.rint(np.clip(x, -1, 1).astype(np.float64) * 8388607.0).astype(np.int32), 24000, 24)

    def boom(*a, **k):
        raise AssertionError("the host FLAC writer ran")
    real = flac.encode
    monkeypatch.setattr(flac, "encode", boom)
    for enc in (stream, np.frombuffer(stream, np.uint8)):
        out = TTSOutput(array=x, sample_rate=24000, encoded=enc, encoded_format="flac")
        assert out.to_bytes("flac") == stream and out.to_bytes("FLAC", sample_width=2) == stream
        assert isinstance(out.to_bytes("flac"), bytes)
        assert out.to_bytes("pcm") == fc.to_int(x).tobytes()          # other formats: as ever
        with pytest.raises(AssertionError):                           # 24 bit stays on the host writer
            out.to_bytes("flac", sample_width=3)
        for other in (out.resample(16000), out.change_speed(1.25), TTSOutput.from_tensor(out.to_tensor()),
                      TTSOutput.combine_outputs([out, out])):
            assert other.encoded is None and other.encoded_format is None
        kept = TTSOutput.combine_outputs([out])                       # a one-chunk request: the chunk itself
        assert kept.encoded is enc and kept.to_bytes("flac") == stream
    with pytest.raises(AssertionError):
        TTSOutput(array=x, sample_rate=24000).to_bytes("flac")       # no stream: the host writer, as ever
    monkeypatch.setattr(flac, "encode", real)
    assert TTSOutput(array=x, sample_rate=24000, encoded=stream, encoded_format="flac").to_bytes("flac", sample_width=3) == want24


# ------------------------------------------------------------------------------------------------ server
def _voice():
    buf = io.BytesIO()
    np.savez(buf, gpt_cond_latent=COND["gpt_cond_latent"], speaker_embedding=COND["speaker_embedding"])
    return base64.b64encode(buf.getvalue()).decode()


@pytest.mark.parametrize("gpu_encoder", [True, False])
def test_server_never_runs_the_host_writer_on_the_event_loop(monkeypatch, gpu_encoder):
    fastapi_testclient = pytest.importorskip("fastapi.testclient")   # (this test alone needs it)
    from auralis_amd.entrypoints.oai_server import create_app
    fake = EncFake(max_seqs=3) if gpu_encoder else FakeNativeEngine(max_seqs=3)
    tts = _tts(fake)
    writer_threads, loop_threads = [], []
    real = flac.encode

    def spying_writer(*a, **k):
        writer_threads.append(threading.get_ident())
        return real(*a, **k)
    monkeypatch.setattr(flac, "encode", spying_writer)
    try:
        app = create_app(tts)

        @app.get("/whoami")
        async def whoami():   # the server's event loop thread
            loop_threads.append(threading.get_ident())
            return {}
        client = fastapi_testclient.TestClient(app)
        client.get("/whoami")
        facade_loop = []
        tts._loop.call_soon_threadsafe(lambda: facade_loop.append(threading.get_ident()))
        for text, speed in (("Hello there.", 1.0), (PARA, 1.0), (PARA + " " + PARA, 1.25)):
            r = client.post("/v1/audio/speech", json={"input": text, "model": "xtts", "voice": [_voice()], "response_format": "flac",
                                                        "language": "en", "speed": speed})
            assert r.status_code == 200 and r.headers["content-type"] == "audio/flac", r.text
            pcm, sr, bps = flac.decode(r.content)
            assert (sr, bps) == (24000, 16) and len(pcm) > 0
        client.get("/whoami")
        loops = set(loop_threads) | set(facade_loop)
        assert len(loops) >= 2
        if gpu_encoder:
            # chunks carried `encoding` except in the reworked (stretch) request; the joined and the reworked waveform went through the
            # engine's one-shot entry on a worker thread; the host writer never ran at all
            assert fake.encodings.count("flac") >= 3 and fake.encodings[-1] is None
            assert len(fake.one_shot_threads) == 2 and not (set(fake.one_shot_threads) & loops)
            assert writer_threads == []
        else:
            # an engine without the entry: the host writer, on a worker thread, for every response
            assert len(writer_threads) == 3 and not (set(writer_threads) & loops)
    finally:
        tts.close()


def test_server_hands_a_waveform_outside_the_one_shot_limits_to_the_host_writer(monkeypatch):
    """aur_encode_flac takes 1 .. 2^24 samples; a joined waveform beyond that is still served, by the host writer on a worker thread."""
    fastapi_testclient = pytest.importorskip("fastapi.testclient")
    from auralis_amd.entrypoints import oai_server
    assert oai_server.FLAC_ONE_SHOT_MAX_SAMPLES == 1 << 24
    monkeypatch.setattr(oai_server, "FLAC_ONE_SHOT_MAX_SAMPLES", 100)   # (the fake's joined waveform is a few thousand samples)
    fake = EncFake(max_seqs=3)
    tts = _tts(fake)
    writer_threads, real = [], flac.encode

    def spying_writer(*a, **k):
        writer_threads.append(threading.get_ident())
        return real(*a, **k)
    monkeypatch.setattr(flac, "encode", spying_writer)
    try:
        client = fastapi_testclient.TestClient(oai_server.create_app(tts))
        loop_thread = []

        @client.app.get("/whoami")
        async def whoami():
            loop_thread.append(threading.get_ident())
            return {}
        client.get("/whoami")
        r = client.post("/v1/audio/speech", json={"input": PARA, "model": "xtts", "voice": [_voice()], "response_format": "flac", "language": "en"})
        assert r.status_code == 200 and r.headers["content-type"] == "audio/flac", r.text
        pcm, sr, bps = flac.decode(r.content)
        assert (sr, bps) == (24000, 16) and len(pcm) > 100
        assert fake.one_shot_threads == [] and len(writer_threads) == 1 and writer_threads[0] not in loop_thread
    finally:
        tts.close()


# ------------------------------------------------------------------------------------------------ fixture coverage
def test_gpu_batch_reaches_every_path_of_the_encoder():
    """A condition on the inputs of tests/test_gpu_flac.py, proved from the reference streams alone."""
    kinds, pos, ks, number_bytes, lens = set(), set(), set(), set(), set()
    for (x, rate), stream in zip(fc.batch(), fc.references()):
        lens.add(len(x))
        fr = fc.frames(stream)
        assert sum(f["n"] for f in fr) == len(x) and len(fr) == -(-len(x) // fc.BLOCK)
        for f in fr:
            kinds.add((f["kind"], f["order"]))
            number_bytes.add(f["number_bytes"])
            if f["kind"] == "FIXED":
                pos.add(f["po"])
                ks.update(f["ks"])
    assert kinds == {("CONSTANT", None), ("VERBATIM", None)} | {("FIXED", o) for o in range(5)}, kinds
    assert pos == {0, 1, 2, 3, 4}, pos
    assert 0 in ks and max(ks) >= 12, ks
    assert number_bytes == {1, 2}
    assert {1, 2, 4, 5, 15, 16, 17, 255, 256, 4095, 4096, 4097, 8192, 2 * 4096 + 4, 3 * 4096 + 1000, 4096 + 48, 4096 + 64,
            130 * 4096 + 7} <= lens
    assert {r for _, r in fc.batch()} == set(fc.RATES)
    # the (n >> po) <= order stop: the 48- and 64-sample tails sit under predictors of order 3 and 4
    tails = {f["n"]: f for (x, _), s in zip(fc.batch(), fc.references()) for f in fc.frames(s)[-1:] if f["n"] in (48, 64)}
    assert tails[48]["order"] == 3 and tails[64]["order"] == 4
