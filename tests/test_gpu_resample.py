"""GPU: the output sample rate (aur_seq_desc.sample_rate) from the kernel up -- resample_out_kernel alone, aur_vocode_rate, sequences
through aur_submit, and the facade -- against the float64 dense reference of tests/resample_ref.py.

Tolerance (derived in tests/resample_ref.py, not measured): |kernel - ref64| <= (T + 2) 2^-24 sum_k |c[p][k] x_k| for the T taps the
kernel keeps of a phase.  Every test prints the largest measured error / bound."""
import io
import wave

import numpy as np
import pytest
import torch

from tests import resample_ref as RR
from tests.gpu_util import SPK_KEY, make_engine

pytestmark = pytest.mark.gpu

SENT = -777.0
CLASSES = (24000,) + RR.RATES
PARA = ("The quick brown fox jumps over the lazy dog near the river bank. It was a bright cold day in April, and the "
        "clocks were striking thirteen! Who would have thought that such a thing could happen? Nobody, really; yet "
        "here we are, walking slowly along the old road, counting the stones and the years that went by.")


@pytest.fixture(scope="module")
def eng32():
    e, gpt_sd, xtts_sd, cond, spk = make_engine(1, max_seqs=4)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng16():
    e, gpt_sd, xtts_sd, cond, spk = make_engine(1, max_seqs=4, vocoder_fp16=True)
    yield e
    e.close()


def _ratio(got, x24, rate):
    """largest |got - ref64(x24)| / bound over the utterance (0 where both the error and the bound are 0); asserts the length"""
    ref, absdot = RR.resample_ref(x24, rate)
    assert got.shape == ref.shape == (RR.n_out(len(x24), rate),), (rate, got.shape, ref.shape)
    if rate in (0, 24000):
        assert np.array_equal(got.view(np.int32), np.asarray(x24, np.float32).view(np.int32)), "24000: copied bit for bit"
        return 0.0
    tol = RR.bound(absdot, RR.KEPT_TAPS[rate])
    err = np.abs(got.astype(np.float64) - ref)
    assert np.isfinite(got).all() and (err <= tol).all(), (rate, len(x24), float((err / np.maximum(tol, 1e-300)).max()))
    return float((err / np.maximum(tol, 1e-300)).max())


def _len_for(n_out, rate):
    """the shortest input whose output has at least n_out samples (exactly n_out wherever the rate can give that)"""
    n = 1
    while RR.n_out(n, rate) < n_out:
        n += 1
    return n


# ---- 1. the kernel alone ----
def test_resample_kernel_ragged_batch(eng32):
    """One ragged batch with every class, 24000 among them: lengths 1, 2, 255, 256, 257, and per class the inputs whose outputs end
    at S - 1, S, S + 1 (S = the kernel's output tile; the next reachable length where the rate cannot give that one) and beyond 3 S.
    Rows are NaN past lens[b]: a kernel that reads instead of zero-filling by the length fails."""
    from auralis_amd._lib import RESAMPLE_TILE as S, samples_out
    lens, rates = [], []
    for rate in CLASSES:
        for n in (1, 2, 255, 256, 257, _len_for(S - 1, rate), _len_for(S, rate), _len_for(S + 1, rate), _len_for(3 * S + 7, rate)):
            lens.append(n)
            rates.append(rate)
    B, L = len(lens), max(lens)
    x = torch.randn(B, L, generator=torch.Generator().manual_seed(77)).numpy()
    x[0, 0] = -0.0                        # (a 24000 row: the copy keeps the sign of a zero)
    for b, n in enumerate(lens):
        x[b, n:] = np.nan
    out, guard = eng32.dbg_resample_out(x, lens, rates)
    assert guard == 0
    assert out.shape == (B, max(samples_out(n, r) for n, r in zip(lens, rates)))
    worst = {}
    for b, (n, rate) in enumerate(zip(lens, rates)):
        no = RR.n_out(n, rate)
        assert no == samples_out(n, rate)
        assert (out[b, no:] == SENT).all(), (rate, n, "written past the utterance's last sample")
        worst[rate] = max(worst.get(rate, 0.0), _ratio(out[b, :no], x[b, :n], rate))
    tails = sorted({RR.n_out(n, r) for n, r in zip(lens, rates)})
    assert {S - 1, S, S + 1} <= set(tails) and tails[-1] > 3 * S
    print("resample_out_kernel, max |err| / bound per rate: " + ", ".join(f"{r}: {v:.3f}" for r, v in worst.items()))
    # each utterance alone = the same utterance inside the batch, bit for bit
    for b, (n, rate) in enumerate(zip(lens, rates)):
        solo, g = eng32.dbg_resample_out(x[b:b + 1, :n], [n], [rate])
        no = RR.n_out(n, rate)
        assert g == 0 and solo.shape == (1, no)
        assert np.array_equal(solo[0].view(np.int32), out[b, :no].view(np.int32)), (rate, n)


def test_resample_kernel_refuses_an_unsupported_rate(eng32):
    from auralis_amd._lib import AurError
    import ctypes as C
    x = np.zeros((1, 8), np.float32)
    lens, out, bad = np.array([8], np.int32), np.zeros((1, 8), np.float32), C.c_int64(0)
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    for rate in (12345, -1, 96000):
        r = np.array([rate], np.int32)
        rc = eng32.lib.aur_dbg_resample_out(eng32.h, x.ctypes.data_as(fp), lens.ctypes.data_as(ip), r.ctypes.data_as(ip), 1, 8,
                                            out.ctypes.data_as(fp), 8, SENT, C.byref(bad))
        assert rc == -1, rate
        with pytest.raises(AurError):
            eng32._check(rc)


# ---- 2. vocode(..., sample_rate=) ----
@pytest.mark.parametrize("f16", [False, True])
def test_vocode_with_sample_rate(eng32, eng16, f16):
    from auralis_amd._lib import AurError
    e = eng16 if f16 else eng32
    gen = torch.Generator().manual_seed(9)
    lens = [31, 7, 18, 12, 5, 9, 11]
    rates = [16000, 24000, 44100, 8000, 22050, 32000, 48000]
    lat = torch.zeros(len(lens), max(lens), 1024)
    for b, n in enumerate(lens):
        lat[b, :n] = torch.randn(n, 1024, generator=gen)
    lat = lat.numpy()
    plain = e.vocode(lat, lens, SPK_KEY)
    got = e.vocode(lat, lens, SPK_KEY, sample_rate=rates)
    worst = max(_ratio(got[b], plain[b], rates[b]) for b in range(len(lens)))
    print(f"vocode sample_rate, fp16={f16}: max |err| / bound {worst:.3f}")
    # bitwise the kernel alone on the same call's 24 kHz result
    n24 = [len(w) for w in plain]
    x = np.full((len(lens), max(n24)), np.nan, np.float32)
    for b, w in enumerate(plain):
        x[b, :n24[b]] = w
    alone, guard = e.dbg_resample_out(x, n24, rates)
    assert guard == 0
    for b in range(len(lens)):
        assert np.array_equal(got[b].view(np.int32), alone[b, :len(got[b])].view(np.int32)), rates[b]
    # nothing asked for: the plain vocoder, bit for bit
    for same in (e.vocode(lat, lens, SPK_KEY, sample_rate=None), e.vocode(lat, lens, SPK_KEY, sample_rate=[24000] * len(lens)),
                 e.vocode(lat, lens, SPK_KEY, sample_rate=[0] * len(lens))):
        assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(same, plain))
    # speed applies first: the resampler sees the waveform that speed produced
    speeds = [1.25, 0.0, 0.8, 1.0, 2.0, 0.5, 1.0]
    fast = e.vocode(lat, lens, SPK_KEY, speed=speeds)
    both = e.vocode(lat, lens, SPK_KEY, speed=speeds, sample_rate=rates)
    for b in range(len(lens)):
        _ratio(both[b], fast[b], rates[b])
    for bad in (12345, -1, 96000):
        with pytest.raises(AurError) as ei:
            e.vocode(lat, lens, SPK_KEY, sample_rate=[16000, bad] + [24000] * (len(lens) - 2))
        assert ei.value.code == -1, bad
    assert np.array_equal(e.vocode(lat, lens, SPK_KEY)[0], plain[0])      # the engine is still usable


# ---- 3. through aur_submit ----
def _text_ids(k):
    from auralis_amd.checkpoint import make_synthetic_text_ids
    from auralis_amd.config import XTTSDims
    return make_synthetic_text_ids(XTTSDims(), n_text=10 + k)


def _run(e, rates, max_tokens, speeds=None, one_at_a_time=False):
    """submit one sequence per entry of `rates` (None: the keyword is left out); results in submission order"""
    out, ids = [], []
    for k, sr in enumerate(rates):
        kw = {} if sr is None else {"sample_rate": sr}
        if speeds and speeds[k] is not None:
            kw["speed"] = speeds[k]
        ids.append(e.submit(_text_ids(k), SPK_KEY, temperature=0.7, max_tokens=max_tokens[k], seed=900 + k, ignore_stop=True, **kw))
        if one_at_a_time:
            out += e.run_until_done()
    if not one_at_a_time:
        out = e.run_until_done()
    by_id = {r["seq_id"]: r for r in out}
    assert sorted(by_id) == sorted(ids) and all(r["error"] == 0 for r in out)
    return [by_id[i] for i in ids]


@pytest.mark.parametrize("f16", [False, True])
def test_submit_with_sample_rate(eng32, eng16, f16):
    from auralis_amd._lib import AurError, samples_for, samples_out
    e = eng16 if f16 else eng32
    rates, max_tokens = [None, 16000, 44100, 8000], [9, 12, 7, 10]
    base = _run(e, [None] * 4, max_tokens)
    worst = 0.0
    for speeds in (None, [None, 1.25, None, None]):
        got = _run(e, rates, max_tokens, speeds)
        solo = _run(e, rates, max_tokens, speeds, one_at_a_time=True)
        for k, (a, b, c) in enumerate(zip(base, got, solo)):
            rate, sp = rates[k] or 24000, (speeds[k] if speeds and speeds[k] else 0.0)
            n = len(b["tokens"])
            assert n == max_tokens[k]
            assert np.array_equal(a["tokens"], b["tokens"]) and np.array_equal(a["latents"], b["latents"])   # decoding does not depend on it
            assert b["sample_rate"] == c["sample_rate"] == rate and a["sample_rate"] == 24000
            x24 = a["wav"] if sp == 0.0 else e.vocode(b["latents"], [n], SPK_KEY, speed=[sp])[0]          # speed applies first
            assert len(x24) == samples_for(n, sp)
            assert b["wav"].shape == (samples_out(len(x24), rate),) == (RR.n_out(len(x24), rate),)
            worst = max(worst, _ratio(b["wav"], x24, rate))
            assert np.array_equal(b["wav"].view(np.int32), c["wav"].view(np.int32)) and np.array_equal(b["tokens"], c["tokens"]), k   # batch = solo
    print(f"submit sample_rate, fp16={f16}: max |err| / bound {worst:.3f}")
    for bad in (12345, -1, 96000):
        with pytest.raises(AurError) as ei:
            e.submit(_text_ids(0), SPK_KEY, max_tokens=4, sample_rate=bad)
        assert ei.value.code == -1, bad
    st = e.stats()
    assert st["sequences_tracked"] == 0 and st["result_blocks_free"] == st["result_blocks"]
    again = _run(e, [None] * 4, max_tokens)            # a default batch behind resampled ones is what it was
    for a, b in zip(base, again):
        assert np.array_equal(a["wav"].view(np.int32), b["wav"].view(np.int32)) and np.array_equal(a["tokens"], b["tokens"])
        assert b["sample_rate"] == 24000
    st = e.stats()
    assert st["sequences_tracked"] == 0 and st["result_blocks_free"] == st["result_blocks"]


def test_samples_generated_counts_delivered_samples(eng32):
    from auralis_amd._lib import samples_for, samples_out
    before = eng32.stats()["samples_generated"]
    _run(eng32, [8000, 48000], [6, 6])
    n24 = samples_for(6)
    assert eng32.stats()["samples_generated"] - before == samples_out(n24, 8000) + samples_out(n24, 48000)


# ---- 4. the facade ----
def test_generate_speech_with_output_sample_rate():
    from auralis_amd import TTS, TTSRequest
    from auralis_amd._lib import samples_for, samples_out
    from auralis_amd.api.text import XTTSTokenizer
    from auralis_amd.api.xtts_engine import XTTSv2Engine
    native, gpt_sd, xtts_sd, cond, spk = make_engine(1, max_seqs=4, vocoder_fp16=True)
    tts = TTS(scheduler_max_concurrency=4).with_engine(XTTSv2Engine(native, XTTSTokenizer(None, synthetic=True), gpt_max_audio_tokens=14))
    voice = {"gpt_cond_latent": cond.numpy(), "speaker_embedding": spk.numpy()}
    try:
        def chunks(rate, stream):
            req = TTSRequest(text=PARA, speaker_files=[voice], language="en", seed=21, stream=stream, output_sample_rate=rate)
            out = tts.generate_speech(req)
            return list(out) if stream else out
        base = chunks(24000, True)
        low = chunks(16000, True)
        assert len(base) == len(low) >= 2
        assert all(c.sample_rate == 16000 for c in low) and all(c.sample_rate == 24000 for c in base)
        assert [c.token_length for c in base] == [c.token_length for c in low]
        assert [len(c.array) for c in base] == [samples_for(c.token_length) for c in base]
        assert [len(c.array) for c in low] == [samples_out(samples_for(c.token_length), 16000) for c in low]
        for a, b in zip(base, low):
            _ratio(np.asarray(b.array), np.asarray(a.array), 16000)
        whole = chunks(16000, False)
        assert whole.sample_rate == 16000 and whole.token_length == sum(c.token_length for c in low)
        assert np.array_equal(whole.array, np.concatenate([c.array for c in low]))
        with wave.open(io.BytesIO(whole.to_bytes("wav"))) as w:
            assert w.getframerate() == 16000 and w.getnframes() == len(whole.array)
    finally:
        tts.close()
