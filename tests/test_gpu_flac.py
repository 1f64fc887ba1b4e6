"""GPU: the FLAC encoder (csrc/flac_kernels.hip) against the host writer, byte for byte.

Reference everywhere: flac.encode(codecs._to_int(x, 2), rate, 16); in addition flac.decode(stream) -- which verifies CRC-8, CRC-16 and
the MD5 -- must return _to_int(x, 2).  There is no tolerance: the algorithm is integer.  The batch is tests/flac_cases.py; that it
reaches every subframe type, predictor order, partition order, Rice parameters 0 and >= 12 and both frame-number forms is proved on
the CPU from the reference streams alone (tests/test_flac_host.py)."""
import base64
import gc
import io

import numpy as np
import pytest

from tests import flac_cases as fc
from tests.gpu_util import SPK_KEY, make_engine

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A


@pytest.fixture(scope="module")
def bare_engine():
    """the kernels need an engine's stream and nothing else: no weights"""
    from auralis_amd._lib import NativeEngine
    e = NativeEngine(n_layer=1, max_seqs=1)
    yield e
    e.close()


def _check_stream(got: bytes, x, rate, decode=True):
    from auralis_amd.api import flac
    want = fc.reference(x, rate)
    assert len(got) == len(want), (len(x), rate, len(got), len(want))
    if got != want:
        first = next(i for i, (a, b) in enumerate(zip(got, want)) if a != b)
        raise AssertionError(f"row of {len(x)} samples at {rate} Hz: first difference at byte {first} of {len(want)}")
    if decode:
        pcm, sr, bps = flac.decode(got)
        assert (sr, bps) == (rate, 16) and np.array_equal(pcm.reshape(-1), fc.to_int(x).astype(np.int32))


# ------------------------------------------------------------------------------------------------ 1. the kernels alone
@pytest.fixture(scope="module")
def kernel_batch(bare_engine):
    rows = [x for x, _ in fc.batch()]
    rates = [r for _, r in fc.batch()]
    x, lens = fc.padded(rows)   # NaN past every row's length
    out, out_lens = bare_engine.dbg_flac_encode(x, lens, rates, sentinel=SENTINEL)
    return out, out_lens


def test_kernels_match_the_host_writer_on_the_ragged_batch(kernel_batch):
    out, out_lens = kernel_batch
    refs = fc.references()
    for b, ((x, rate), want) in enumerate(zip(fc.batch(), refs)):
        got = out[b, :out_lens[b]].tobytes()
        assert out_lens[b] == len(want), (b, len(x), int(out_lens[b]), len(want))
        if got != want:
            first = next(i for i, (p, q) in enumerate(zip(got, want)) if p != q)
            raise AssertionError(f"row {b} ({len(x)} samples at {rate} Hz): first difference at byte {first} of {len(want)}")


def test_kernel_streams_decode_to_the_int16_samples(kernel_batch):
    from auralis_amd.api import flac
    out, out_lens = kernel_batch
    for b, (x, rate) in enumerate(fc.batch()):
        pcm, sr, bps = flac.decode(out[b, :out_lens[b]].tobytes())   # verifies both CRCs of every frame and the MD5
        assert (sr, bps) == (rate, 16), (b, sr, bps)
        assert np.array_equal(pcm.reshape(-1), fc.to_int(x).astype(np.int32)), b


def test_kernels_leave_the_bytes_behind_a_stream_alone(kernel_batch):
    out, out_lens = kernel_batch
    for b in range(out.shape[0]):
        assert 42 < out_lens[b] <= out.shape[1]
        assert np.all(out[b, out_lens[b]:] == SENTINEL), (b, int(out_lens[b]))


def test_every_row_alone_is_what_it_is_inside_the_batch(bare_engine, kernel_batch):
    out, out_lens = kernel_batch
    for b, (x, rate) in enumerate(fc.batch()):
        x1, l1 = fc.padded([x])
        o1, n1 = bare_engine.dbg_flac_encode(x1, l1, [rate], sentinel=SENTINEL)
        assert n1[0] == out_lens[b] and np.array_equal(o1[0, :n1[0]], out[b, :out_lens[b]]), b
        assert np.all(o1[0, n1[0]:] == SENTINEL), b


# ------------------------------------------------------------------------------------------------ 2. aur_encode_flac
def test_one_shot_entry_gives_the_same_streams(bare_engine):
    rows = [x for x, _ in fc.batch()]
    rates = [r for _, r in fc.batch()]
    got = bare_engine.encode_flac(rows, rates)
    assert got == fc.references()


def test_one_shot_entry_limits(bare_engine):
    from auralis_amd._lib import AurError
    ok = np.zeros(16, np.float32)
    for rows, rates in (([np.zeros(0, np.float32)], [24000]), ([ok, np.zeros((1 << 24) + 1, np.float32)], [24000, 24000]),
                        ([ok], [1 << 20]), ([ok], [0])):
        with pytest.raises(AurError) as ei:
            bare_engine.encode_flac(rows, rates)
        assert ei.value.code == -1, ei.value
    assert bare_engine.encode_flac([ok], [(1 << 20) - 1])[0] == fc.reference(ok, (1 << 20) - 1)


def test_one_shot_entry_three_byte_frame_number(bare_engine):
    """2049 blocks: the last frame's number, 2048, takes three bytes.  All silence (CONSTANT blocks cost the host writer nothing)
    except three blocks."""
    rng = np.random.default_rng(7)
    x = np.zeros(2049 * fc.BLOCK, np.float32)
    for blk, amp in ((0, 0.01), (2047, 0.2), (2048, 1e-3)):
        x[blk * fc.BLOCK:(blk + 1) * fc.BLOCK] = (amp * rng.uniform(-1, 1, fc.BLOCK)).astype(np.float32)
    got = bare_engine.encode_flac([x], [44100])[0]
    want = fc.reference(x, 44100)
    assert len(got) == len(want) and got == want
    assert b"\xff\xf8\xc0\x08\xe0\xa0\x80" in got[-8300:]   # the last frame's header: block size 4096, frame number 2048 in three bytes


# ------------------------------------------------------------------------------------------------ 3. through aur_submit
def _by_id(outs):
    return {o["seq_id"]: o for o in outs}


@pytest.fixture(scope="module")
def submit_cases(dims):
    from auralis_amd.checkpoint import make_synthetic_text_ids
    # (text ids, speed, sample rate, encoded?) -- encoded sequences beside default ones, stretched and resampled ones among them
    spec = [(0.0, 0, True), (0.75, 8000, True), (1.6, 48000, True), (0.0, 0, False), (0.0, 24000, True), (1.6, 8000, False)]
    return [(make_synthetic_text_ids(dims, n_text=9 + 3 * k, seed=200 + k), sp, sr, enc) for k, (sp, sr, enc) in enumerate(spec)]


def _submit(e, case, k, encoded):
    ids, sp, sr, _ = case
    return e.submit(ids, SPK_KEY, temperature=0.8 if k % 2 else 0.0, top_k=50, top_p=0.85, max_tokens=14 + 5 * k, seed=400 + k, ignore_stop=True,
                    speed=sp, sample_rate=sr, **({"encoding": "flac"} if encoded else {}))


def test_submit_with_encoding_delivers_the_stream_of_the_delivered_wav(submit_cases):
    # the same sequences without `encoding`, then a default-only batch, on an engine that never encodes
    plain_e, *_ = make_engine(2, max_seqs=8, return_latents=True)
    try:
        sids = [_submit(plain_e, c, k, False) for k, c in enumerate(submit_cases)]
        plain = _by_id(plain_e.run_until_done())
        plain = [plain[s] for s in sids]
        sids = [_submit(plain_e, c, k, False) for k, c in enumerate(submit_cases[:2])]
        fresh_tail = _by_id(plain_e.run_until_done())
        fresh_tail = [fresh_tail[s] for s in sids]
    finally:
        plain_e.close()
    e, *_ = make_engine(2, max_seqs=8, return_latents=True)
    try:
        sids = [_submit(e, c, k, c[3]) for k, c in enumerate(submit_cases)]
        got = _by_id(e.run_until_done())
        got = [got[s] for s in sids]
        for k, (c, g, p) in enumerate(zip(submit_cases, got, plain)):
            assert g["error"] == 0 and p["error"] == 0
            # tokens, latents and wav do not depend on the encoding
            assert g["tokens"].tolist() == p["tokens"].tolist(), k
            assert np.array_equal(g["latents"], p["latents"]) and np.array_equal(g["wav"], p["wav"]), k
            assert g["sample_rate"] == (c[2] or 24000)
            if c[3]:
                assert g["encoded_format"] == "flac"
                _check_stream(g["encoded"].tobytes(), g["wav"], g["sample_rate"])
            else:
                assert "encoded" not in g
        # batch == solo
        for k in (1, 2):
            sid = _submit(e, submit_cases[k], k, True)
            solo = _by_id(e.run_until_done())[sid]
            assert np.array_equal(solo["wav"], got[k]["wav"]) and solo["encoded"].tobytes() == got[k]["encoded"].tobytes(), k
        # a default-only batch behind them is bitwise what it is on an engine that never encoded
        tail = [_submit(e, c, k, False) for k, c in enumerate(submit_cases[:2])]
        after = _by_id(e.run_until_done())
        for s, f in zip(tail, fresh_tail):
            assert "encoded" not in after[s]
            assert after[s]["tokens"].tolist() == f["tokens"].tolist() and np.array_equal(after[s]["wav"], f["wav"])
    finally:
        e.close()


def test_submit_rejects_an_unknown_encoding(submit_cases):
    from auralis_amd._lib import AurError
    e, *_ = make_engine(2, max_seqs=2)
    try:
        with pytest.raises(AurError) as ei:
            e.submit(submit_cases[0][0], SPK_KEY, max_tokens=4, encoding=2)
        assert ei.value.code == -1
    finally:
        e.close()


def test_cancel_and_injected_vocoder_failure_leave_the_gauges_back(submit_cases, monkeypatch):
    from auralis_amd._lib import AurError
    monkeypatch.setenv("AUR_TEST_FAIL_VOC", "2")     # read when the engine is created: its second vocoder launch throws
    e, *_ = make_engine(2, max_seqs=4)
    monkeypatch.delenv("AUR_TEST_FAIL_VOC")
    try:
        # an encoded sequence cancelled while it decodes, beside one that finishes
        keep = _submit(e, submit_cases[0], 0, True)
        drop = e.submit(submit_cases[1][0], SPK_KEY, temperature=0.0, max_tokens=400, ignore_stop=True, encoding="flac")
        e.step()
        e.cancel(drop)
        outs = _by_id(e.run_until_done())
        assert outs[drop]["error"] == -5 and len(outs[drop]["wav"]) == 0 and "encoded" not in outs[drop]
        _check_stream(outs[keep]["encoded"].tobytes(), outs[keep]["wav"], 24000)
        # the injected failure hits a pass with encoded sequences: they fail like any other queue entry
        sids = [_submit(e, c, k, True) for k, c in enumerate(submit_cases[:2])]
        with pytest.raises(AurError) as ei:
            for _ in range(200):
                e.step()
        assert ei.value.code == -2 and "AUR_TEST_FAIL_VOC" in str(ei.value)
        failed = _by_id(e.poll())
        assert sorted(failed) == sorted(sids) and all(o["error"] == -2 and "encoded" not in o for o in failed.values())
        # ... and the engine goes on encoding
        again = _submit(e, submit_cases[2], 2, True)
        out = _by_id(e.run_until_done())[again]
        _check_stream(out["encoded"].tobytes(), out["wav"], 48000)
        del outs, out, failed
        gc.collect()
        st = e.stats()
        assert st["sequences_tracked"] == 0 and st["result_blocks_free"] == st["result_blocks"], st
        assert st["kv_blocks_total"] - st["kv_blocks_free"] == 2
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ 4. facade and server
TEXT = "The harbour lights came on one by one while the last ferry crossed the bay."
LONG = ("It was a bright cold day in April, and the clocks were striking thirteen. Nobody in the street seemed to notice, and the wind "
        "kept pushing the dust along the old road as if nothing had happened at all. Who would have thought that such a thing could "
        "happen? Nobody, really; yet here we are, walking slowly along the old road, counting the stones and the years that went by. "
        "The lamps came on one by one along the harbour wall, and the last ferry crossed the bay without a sound; somebody waved from "
        "the quay, and then the evening closed over the water as it always does, slowly at first and then all at once. Nobody spoke. "
        "The tide went out, the gulls went quiet, and the town put out its lights one window at a time until only the lighthouse was left.")
KW = dict(temperature=0.75, top_p=0.85, top_k=50, repetition_penalty=5.0, language="en")


@pytest.fixture(scope="module")
def served(tmp_path_factory, dims):
    fastapi_testclient = pytest.importorskip("fastapi.testclient")   # (the facade and server tests alone need it)
    from auralis_amd import TTS
    from auralis_amd.checkpoint import make_synthetic_conditioning, make_synthetic_gpt, make_synthetic_xtts, save_checkpoint
    from auralis_amd.entrypoints.oai_server import create_app
    root = str(tmp_path_factory.mktemp("flac_ckpt"))
    gpt_sd = make_synthetic_gpt(dims.gpt, seed=1234, n_layer=2)
    gpt_sd["mel_head.bias"][1025] = 3.0      # natural stop after a handful of tokens
    save_checkpoint(root, gpt_sd, make_synthetic_xtts(dims, seed=1234, gpt_sd=gpt_sd), dims, synthetic_tokenizer=True)
    cond, spk = make_synthetic_conditioning(dims)
    buf = io.BytesIO()
    np.savez(buf, gpt_cond_latent=cond.numpy(), speaker_embedding=spk.numpy())
    tts = TTS(scheduler_max_concurrency=4).from_pretrained(root)
    client = fastapi_testclient.TestClient(create_app(tts))
    yield tts, client, buf.getvalue()
    tts.close()


@pytest.fixture
def no_host_writer(monkeypatch):
    from auralis_amd.api import flac

    def boom(*a, **k):
        raise AssertionError("the host FLAC writer ran")
    real = flac.encode
    monkeypatch.setattr(flac, "encode", boom)
    return real


def test_request_with_output_encoding_carries_the_engines_stream(served, no_host_writer):
    from auralis_amd import TTSRequest
    from auralis_amd.api import flac
    tts, _, voice = served
    out = tts.generate_speech(TTSRequest(text=TEXT, speaker_files=[voice], seed=11, output_encoding="flac", **KW))
    assert out.encoded is not None and out.encoded_format == "flac"
    data = out.to_bytes("flac")
    assert data == no_host_writer(fc.to_int(out.array), 24000, 16)
    pcm, sr, bps = flac.decode(data)
    assert (sr, bps) == (24000, 16) and np.array_equal(pcm.reshape(-1), fc.to_int(out.array).astype(np.int32)) and np.abs(pcm).max() > 0
    plain = tts.generate_speech(TTSRequest(text=TEXT, speaker_files=[voice], seed=11, **KW))
    assert plain.encoded is None and np.array_equal(plain.array, out.array)


@pytest.mark.parametrize("case", ["one_chunk", "three_chunks", "stretch"])
def test_speech_route_flac_never_runs_the_host_writer(served, no_host_writer, case):
    from auralis_amd import TTSRequest
    from auralis_amd.api import flac
    tts, client, voice = served
    text = LONG if case == "three_chunks" else TEXT
    body = {"input": text, "model": "xtts", "voice": [base64.b64encode(voice).decode()], "response_format": "flac", "seed": 31, **KW}
    if case == "stretch":
        body["speed"] = 1.25
    r = client.post("/v1/audio/speech", json=body)
    assert r.status_code == 200, r.text
    assert r.headers["content-type"] == "audio/flac"
    direct = tts.generate_speech(TTSRequest(text=text, speaker_files=[voice], seed=31, **KW))
    if case == "three_chunks":
        assert len(tts.tts_engine.tokenizer.batch_encode_with_split(text, "en")) >= 3
    if case == "stretch":
        direct = direct.change_speed(1.25)
    want = fc.to_int(direct.array)
    pcm, sr, bps = flac.decode(r.content)
    assert (sr, bps) == (24000, 16) and len(want) > 0
    assert np.array_equal(pcm.reshape(-1), want.astype(np.int32))
    assert r.content == no_host_writer(want, 24000, 16)
