"""GPU: several engines in one process behind the facade (`from_pretrained(devices=[...])`, auralis_amd/api/dispatch.py).  Results
are bitwise batch-invariant, so where a chunk runs cannot change it: every test compares with ONE engine serving the same requests.
Synthetic 2-layer checkpoint, 4 slots per engine, at most 48 tokens per chunk."""
import asyncio
import gc
import threading
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

S1 = "The quick brown fox jumps over the lazy dog near the river bank."
PARA = ("It was a bright cold day in April, and the clocks were striking thirteen! Who would have thought that such a thing could "
        "happen? Nobody, really; yet here we are, walking slowly along the old road, counting the stones and the years that went by. ")
MONTHS = ["April", "March", "June", "July", "August", "October", "December", "January", "May", "November"]
MAX_TOKENS = 48


def paras(n, first=0):
    """n chunks' worth of text, no two chunks alike"""
    return " ".join(PARA.strip().replace("April", MONTHS[(first + j) % len(MONTHS)]) for j in range(n))


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory, dims):
    from auralis_amd.checkpoint import make_synthetic_gpt, make_synthetic_xtts, save_checkpoint
    d = tmp_path_factory.mktemp("ckpt2")
    gpt_sd = make_synthetic_gpt(dims.gpt, seed=1234, n_layer=2)
    gpt_sd["mel_head.bias"][1025] = 3.0          # sequences stop by themselves after a handful of tokens
    save_checkpoint(str(d), gpt_sd, make_synthetic_xtts(dims, seed=1234, gpt_sd=gpt_sd), dims, synthetic_tokenizer=True)
    return str(d)


@pytest.fixture(scope="module")
def voices(dims):
    from auralis_amd.checkpoint import make_synthetic_conditioning
    cond, spk = make_synthetic_conditioning(dims)
    cond, spk = cond.numpy(), spk.numpy()
    return [{"gpt_cond_latent": cond, "speaker_embedding": spk},
            {"gpt_cond_latent": np.ascontiguousarray(cond[:, ::-1]) * 0.9, "speaker_embedding": np.roll(spk, 7, axis=1)},
            {"gpt_cond_latent": np.roll(cond, 3, axis=1) * 1.1, "speaker_embedding": np.ascontiguousarray(spk[:, ::-1])}]


def _open(ckpt, **kw):
    from auralis_amd import TTS
    tts = TTS(scheduler_max_concurrency=4).from_pretrained(ckpt, **kw)
    tts.tts_engine.gpt_max_audio_tokens = MAX_TOKENS
    return tts


@pytest.fixture(scope="module")
def one(ckpt):
    tts = _open(ckpt)                       # today's construction: one engine, 4 slots
    yield tts
    tts.close()


@pytest.fixture(scope="module")
def duo(ckpt):
    tts = _open(ckpt, devices=[0, 0])       # two engines on one GPU
    yield tts
    tts.close()


def _requests(voices):
    """Twelve requests of one to five chunks: greedy and sampled (fixed seed), one at speed 1.25, one urgent, two voices."""
    from auralis_amd import TTSRequest
    out = []
    for k in range(12):
        text = S1 if k % 5 == 0 else paras(1 + k % 5, first=k)
        out.append(TTSRequest(text=text, speaker_files=[voices[k % 2]], language="en", seed=100 + 17 * k, stream=True,
                              temperature=0.0 if k % 2 == 0 else 0.75, speed=1.25 if k == 3 else 1.0, priority=1 if k == 6 else 0))
    return out


def _run_all(tts, requests):
    """All requests at once through generate_speech_async -> per request, per chunk (token count, waveform copy)"""
    async def one_request(r):
        return [(int(c.token_length), np.array(c.array)) async for c in await tts.generate_speech_async(r)]

    async def every():
        return await asyncio.gather(*[one_request(r) for r in requests])
    return tts._submit(every()).result(timeout=120)


def _same(got, ref):
    assert len(got) == len(ref)
    for g, r in zip(got, ref):
        assert [n for n, _ in g] == [n for n, _ in r]
        assert len(g) == len(r) and all(np.array_equal(a, b) for (_, a), (_, b) in zip(g, r))


@pytest.fixture(scope="module")
def reference(one, voices):
    ref = _run_all(one, _requests(voices))
    n_chunks = [len(r) for r in ref]
    assert min(n_chunks) == 1 and max(n_chunks) == 5 and all(0 < n <= MAX_TOKENS and len(a) > 0 for r in ref for n, a in r)
    return ref


def _idle(eng, timeout=30.0):
    """the cancelled sequences have come back through poll() and every engine has nothing ahead of it"""
    deadline = time.time() + timeout
    while time.time() < deadline:
        if not any(d._pending for d in eng.drivers) and eng._placer.queued() == 0:
            return
        time.sleep(0.002)
    raise AssertionError("engines did not drain")


def test_two_engines_on_one_device_equal_one_engine_bitwise(duo, reference, voices):
    eng = duo.tts_engine
    assert len(eng.natives) == 2 and eng.native is eng.natives[0] and [n.max_seqs for n in eng.natives] == [4, 4]
    _same(_run_all(duo, _requests(voices)), reference)
    for n in eng.natives:
        assert n.stats()["tokens_generated"] > 0        # both engines decoded
    _idle(eng)
    assert eng.load() == [{"waiting": 0, "running": 0, "vocoding": 0, "free_slots": 4, "token_budget": 0}] * 2
    assert [e["device"] for e in eng.get_memory_usage_curve()["engines"]] == [0, 0]


def test_stream_equals_non_stream_on_two_engines(duo, voices):
    from auralis_amd import TTSRequest
    text = paras(5)
    assert len(duo.tts_engine.tokenizer.batch_encode_with_split(text, "en")) == 5
    kw = dict(text=text, speaker_files=[voices[0]], language="en", seed=9, temperature=0.75)
    whole = duo.generate_speech(TTSRequest(**kw))
    chunks = list(duo.generate_speech(TTSRequest(stream=True, **kw)))
    assert len(chunks) == 5 and np.array_equal(np.concatenate([c.array for c in chunks]), whole.array)


def test_a_consumer_that_walks_away_leaves_both_engines_empty(ckpt, voices):
    from auralis_amd import TTSRequest
    tts = _open(ckpt, devices=[0, 0])
    try:
        eng = tts.tts_engine
        eng.fixed_length = True                 # every chunk runs its 48 tokens: there is something to stop
        probe = TTSRequest(text=S1, speaker_files=[voices[0]], language="en", seed=5)
        before = tts.generate_speech(probe).array.copy()
        text = paras(10)
        n_chunks = len(eng.tokenizer.batch_encode_with_split(text, "en"))
        assert n_chunks == 10
        gen = tts.generate_speech(TTSRequest(text=text, speaker_files=[voices[0]], language="en", seed=40, stream=True))
        c = next(gen)
        assert len(c.array) > 0
        del c
        gen.close()
        _idle(eng)
        for _ in range(3):                      # (results that arrived for cancelled futures are dropped on the loop)
            tts._submit(asyncio.sleep(0)).result(timeout=5)
        gc.collect()                            # (the chunk that was read was a lease on a result block)
        for n in eng.natives:
            st = n.stats()
            assert st["sequences_tracked"] == 0 and st["result_blocks"] == st["result_blocks_free"], st
        assert eng.load() == [{"waiting": 0, "running": 0, "vocoding": 0, "free_slots": 4, "token_budget": 0}] * 2
        assert sum(d.cancelled for d in eng.drivers) >= 1
        assert np.array_equal(tts.generate_speech(probe).array, before)
    finally:
        tts.close()


def test_voice_table_pressure_goes_through_reregistration(ckpt, one, voices):
    """max_speakers=2 per engine and three voices taking turns: a voice evicted from an engine is registered there again when one of
    its chunks is placed on it (has_conditioning / set_conditioning, and reregister inside the submission)."""
    from auralis_amd import TTSRequest
    tts = _open(ckpt, devices=[0, 0], max_speakers=2)
    try:
        eng = tts.tts_engine
        registered = []
        for i, n in enumerate(eng.natives):
            n.set_conditioning = (lambda key, g, s, i=i, f=n.set_conditioning: (registered.append((i, key)), f(key, g, s))[1])
        for k in range(9):
            kw = dict(text=paras(2 + k % 2, first=k), speaker_files=[voices[k % 3]], language="en", seed=300 + k, temperature=0.75)
            got = tts.generate_speech(TTSRequest(**kw))
            ref = one.generate_speech(TTSRequest(**kw))
            assert len(got.array) > 0 and np.array_equal(got.array, ref.array), k
        assert all(n.stats()["speakers"] <= 2 for n in eng.natives)
        assert len(registered) > len(set(registered))          # some (engine, voice) pair was registered more than once
    finally:
        tts.close()


def test_get_load_while_the_engine_steps():
    from tests.gpu_util import SPK_KEY, make_engine
    eng = make_engine(2, max_seqs=4)[0]
    try:
        assert eng.load() == {"waiting": 0, "running": 0, "vocoding": 0, "free_slots": 4, "token_budget": 0}
        seen, bad, stop = [], [], threading.Event()
        total = sum(MAX_TOKENS - 8 * i for i in range(4))      # of one wave; the waves do not overlap

        def watch():
            while not stop.is_set():
                l = eng.load()
                seen.append(l)
                if not (all(0 <= l[k] <= 4 for k in ("waiting", "running", "vocoding", "free_slots")) and 0 <= l["token_budget"] <= total):
                    bad.append(l)
        t = threading.Thread(target=watch)
        for wave in range(2):                   # four sequences at a time: as many as the engine has slots
            for i in range(4):
                eng.submit(list(range(5, 25 + 3 * i)), SPK_KEY, temperature=0.75, seed=wave * 10 + i, max_tokens=MAX_TOKENS - 8 * i, ignore_stop=True)
            l = eng.load()
            assert l["waiting"] == 4 and l["running"] == 0 and l["token_budget"] == total
            if wave == 0:
                t.start()
            done = eng.run_until_done()
            assert len(done) == 4 and all(d["error"] == 0 for d in done)
        stop.set()
        t.join(timeout=10)
        assert not bad, bad[:3]
        assert len(seen) > 10 and any(l["running"] > 0 for l in seen) and any(0 < l["token_budget"] < total for l in seen)
        assert eng.load() == {"waiting": 0, "running": 0, "vocoding": 0, "free_slots": 4, "token_budget": 0}
    finally:
        eng.close()


def test_two_real_devices_equal_one_engine_bitwise(ckpt, reference, voices):
    """The only test that can catch a missing device bind: two engines on two GPUs, driven from two driver threads and the event loop."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip(f"needs two visible GPUs, {torch.cuda.device_count()} visible")
    tts = _open(ckpt, devices=[0, 1])
    try:
        eng = tts.tts_engine
        _same(_run_all(tts, _requests(voices)), reference)
        for n in eng.natives:
            assert n.stats()["tokens_generated"] > 0
        _idle(eng)
        assert eng.load() == [{"waiting": 0, "running": 0, "vocoding": 0, "free_slots": 4, "token_budget": 0}] * 2
        assert [e["device"] for e in eng.get_memory_usage_curve()["engines"]] == [0, 1]
    finally:
        tts.close()
