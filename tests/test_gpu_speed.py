"""GPU: the speaking rate (aur_seq_desc.speed) from the kernel up -- interp3_kernel / interp3_h_kernel alone, aur_vocode_speed against
the oracle on pre-stretched latents, sequences through aur_submit, the vocoder pass's workspace bound, and the facade.

Measured maxima on the MI355X are printed by each test."""
import numpy as np
import pytest
import torch

from tests import speed_ref as S
from tests import vocoder_ref as R
from tests.gpu_util import SPK_KEY, make_engine, rms

pytestmark = pytest.mark.gpu

SENT = -777.0
PARA = ("The quick brown fox jumps over the lazy dog near the river bank. It was a bright cold day in April, and the "
        "clocks were striking thirteen! Who would have thought that such a thing could happen? Nobody, really; yet "
        "here we are, walking slowly along the old road, counting the stones and the years that went by.")


def _h(a):
    return np.asarray(a, dtype=np.float32).astype(np.float16).astype(np.float32)


@pytest.fixture(scope="module")
def eng16():
    e, gpt_sd, xtts_sd, cond, spk = make_engine(1, max_seqs=2, vocoder_fp16=True)
    yield e, xtts_sd, spk
    e.close()


@pytest.fixture(scope="module")
def eng32():
    e, gpt_sd, xtts_sd, cond, spk = make_engine(1, max_seqs=4)
    yield e, xtts_sd, spk
    e.close()


# ---- 1. the kernel alone ----
def test_interp3_both_forms(eng16):
    """The 36 (n_lat, speed) pairs as one ragged batch.  fp32 form: |z - ref| <= 1.5e-6, test_interp2_both_forms' 1e-6 with half as much
    again for the third fp32 blend; halves form: exactly fp16 of the fp32 form, as there."""
    eng = eng16[0]
    C = 32
    lat = torch.randn(6, 64, C, generator=torch.Generator().manual_seed(13)).numpy()
    n_lat = [n for n, _ in S.PAIRS]
    speed = [sp for _, sp in S.PAIRS]
    rows = [(5 * i + 2) % 6 for i in range(len(S.PAIRS))]
    frames = [R.frames_for(S.stretched_rows(n, sp)) for n, sp in S.PAIRS]
    assert max(frames) == 557        # (64, 0.5): three 256-position blocks, two block boundaries crossed
    z, guard = eng.dbg_interp3(lat, rows, n_lat, speed, max(frames))
    zh, guard_h = eng.dbg_interp3(lat, rows, n_lat, speed, max(frames), out_f16=True)
    assert guard == 0 and guard_h == 0
    ref = S.interp3_ref(lat, rows, n_lat, speed)
    worst = 0.0
    for b, n in enumerate(frames):
        assert ref[b].shape == (C, n)
        err = np.abs(z[b, :, :n] - ref[b]).max()
        worst = max(worst, err)
        assert err <= 1.5e-6, (S.PAIRS[b], err)
        assert (z[b, :, n:] == SENT).all() and (zh[b, :, n:] == SENT).all(), S.PAIRS[b]
        assert np.array_equal(zh[b, :, :n], _h(z[b, :, :n])), ("halves form != fp16 of the fp32 form", S.PAIRS[b])
    print(f"interp3 fp32 form, 36 pairs: max err {worst:.3e}; halves form = fp16 of it bitwise")
    # a stretch that keeps the rows -- speed 1.0, and (3, 0.8), (1, 0.75), ... -- is the two-stage kernel's result bit for bit
    keep = [b for b, (n, sp) in enumerate(S.PAIRS) if S.stretched_rows(n, sp) == n]
    assert {S.PAIRS[b] for b in keep} >= {(n, 1.0) for n in S.N_LATS} | {(3, 0.8)}
    kf = [frames[b] for b in keep]
    z2, g2 = eng.dbg_interp2(lat, [rows[b] for b in keep], [n_lat[b] for b in keep], max(kf))
    z2h, g2h = eng.dbg_interp2(lat, [rows[b] for b in keep], [n_lat[b] for b in keep], max(kf), out_f16=True)
    assert g2 == 0 and g2h == 0
    for i, b in enumerate(keep):
        assert np.array_equal(z[b, :, :frames[b]], z2[i, :, :kf[i]]) and np.array_equal(zh[b, :, :frames[b]], z2h[i, :, :kf[i]]), S.PAIRS[b]
    # one utterance alone = the same utterance inside the batch
    for pair in ((64, 0.5), (7, 2.0), (1, 2.0), (31, 1.0)):
        b = S.PAIRS.index(pair)
        za, ga = eng.dbg_interp3(lat, rows[b:b + 1], n_lat[b:b + 1], speed[b:b + 1], frames[b])
        zha, gha = eng.dbg_interp3(lat, rows[b:b + 1], n_lat[b:b + 1], speed[b:b + 1], frames[b], out_f16=True)
        assert ga == 0 and gha == 0
        assert np.array_equal(za[0], z[b, :, :frames[b]]) and np.array_equal(zha[0], zh[b, :, :frames[b]]), pair


def test_interp3_refuses_a_speed_outside_the_range(eng16):
    from auralis_amd._lib import AurError
    lat = np.zeros((1, 4, 32), np.float32)
    for bad in (0.4, 2.5, float("nan"), float("inf"), -1.0):
        with pytest.raises(AurError) as ei:
            eng16[0].dbg_interp3(lat, None, [4], [bad], 17)
        assert ei.value.code == -1


# ---- 2. vocode(..., speed=) against the oracle on latents pre-stretched with torch ----
@pytest.mark.parametrize("f16", [False, True])
def test_vocode_speed_matches_oracle_on_prestretched_latents(eng32, eng16, f16):
    from oracle import xtts_oracle as O
    e, xtts_sd, spk = eng16 if f16 else eng32
    w = O.vocoder_effective_weights(xtts_sd)
    gen = torch.Generator().manual_seed(9)
    lens, speeds = [31, 7, 18], [0.75, 1.0, 1.6]
    lat = torch.zeros(3, 31, 1024)
    for b, n in enumerate(lens):
        lat[b, :n] = torch.randn(n, 1024, generator=gen)
    wavs = e.vocode(lat.numpy(), lens, SPK_KEY, speed=speeds)
    for b, n in enumerate(lens):
        pre = S.torch_stretch(lat[b, :n].numpy(), speeds[b]).float()[None]
        assert pre.shape[1] == S.stretched_rows(n, speeds[b])
        ref = O.hifi_decoder_forward(w, pre, spk).reshape(-1).numpy()
        assert wavs[b].shape == ref.shape == (S.samples_for(n, speeds[b]),)
        err, sig = rms(wavs[b] - ref), rms(ref)
        print(f"vocode speed={speeds[b]} n_lat={n} fp16={f16}: rms err {err:.3e} signal rms {sig:.3e}")
        assert err <= 1e-3 and err <= 1e-2 * sig, (b, err, sig)     # _check of tests/test_gpu_vocoder.py
    plain = e.vocode(lat.numpy(), lens, SPK_KEY)
    assert np.array_equal(wavs[1], plain[1])                         # the speed-1.0 member of the mixed batch
    unset = e.vocode(lat.numpy(), lens, SPK_KEY, speed=[0.0, 0.0, 0.0])
    assert all(np.array_equal(a, b) for a, b in zip(unset, plain))
    from auralis_amd._lib import AurError
    with pytest.raises(AurError) as ei:
        e.vocode(lat.numpy(), lens, SPK_KEY, speed=[1.0, 0.3, 1.0])
    assert ei.value.code == -1


# ---- 3. through aur_submit ----
def _text_ids(k):
    from auralis_amd.checkpoint import make_synthetic_text_ids
    from auralis_amd.config import XTTSDims
    return make_synthetic_text_ids(XTTSDims(), n_text=10 + k)


def _run(e, speeds, max_tokens, one_at_a_time=False):
    """submit one sequence per entry of `speeds` (None: the keyword is left out); results in submission order"""
    out = []
    ids = []
    for k, sp in enumerate(speeds):
        kw = {} if sp is None else {"speed": sp}
        ids.append(e.submit(_text_ids(k), SPK_KEY, temperature=0.7, max_tokens=max_tokens[k], seed=900 + k, ignore_stop=True, **kw))
        if one_at_a_time:
            out += e.run_until_done()
    if not one_at_a_time:
        out = e.run_until_done()
    by_id = {r["seq_id"]: r for r in out}
    assert sorted(by_id) == sorted(ids) and all(r["error"] == 0 for r in out)
    return [by_id[i] for i in ids]


def test_submit_with_speed(eng32):
    from auralis_amd._lib import AurError
    e = eng32[0]
    speeds, max_tokens = [None, 0.5, 1.0, 2.0], [9, 12, 7, 10]
    base = _run(e, [None] * 4, max_tokens)
    got = _run(e, speeds, max_tokens)
    solo = _run(e, speeds, max_tokens, one_at_a_time=True)
    for k, (a, b, c) in enumerate(zip(base, got, solo)):
        sp = speeds[k] or 0.0
        n = len(b["tokens"])
        assert n == max_tokens[k]
        assert np.array_equal(a["tokens"], b["tokens"]) and np.array_equal(a["latents"], b["latents"])     # speed does not touch decoding
        assert b["latents"].shape == (n, 1024)                                                             # the unstretched rows
        assert b["wav"].shape == (S.samples_for(n, sp),) == (256 * R.frames_for(S.stretched_rows(n, sp)),)
        assert np.array_equal(b["wav"], e.vocode(b["latents"], [n], SPK_KEY, speed=[sp])[0]), k
        assert np.array_equal(b["wav"], c["wav"]) and np.array_equal(b["tokens"], c["tokens"]), k         # batch invariant
        if S.stretched_rows(n, sp) == n:
            assert np.array_equal(a["wav"], b["wav"])
    assert len(got[1]["wav"]) > len(base[1]["wav"]) > 0 and len(got[3]["wav"]) < len(base[3]["wav"])
    for bad in (0.4, float("nan"), 2.01, float("inf"), -1.0):
        with pytest.raises(AurError) as ei:
            e.submit(_text_ids(0), SPK_KEY, max_tokens=4, speed=bad)
        assert ei.value.code == -1, bad
    again = _run(e, [1.25], [6])                                                                           # the engine is still usable
    assert again[0]["wav"].shape == (S.samples_for(6, 1.25),)
    assert e.stats()["sequences_tracked"] == 0


# ---- 4. the vocoder pass's workspace bound ----
def test_vocoder_pass_is_split_at_the_workspace_bound():
    """max_seqs = 2: a pass may hold B * maxT <= 2 * frames_for(608) = 5294 frames.  310 tokens at 0.5x are 620 rows = 2699 frames, so
    two such utterances do not fit one pass: each goes alone, all three finish, bit for bit as alone, and nothing is left behind."""
    e, *_ = make_engine(1, max_seqs=2, vocoder_fp16=True)
    try:
        n = 310
        assert 2 * R.frames_for(S.stretched_rows(n, 0.5)) > 2 * R.frames_for(608) >= R.frames_for(S.stretched_rows(n, 0.5))
        solo = _run(e, [0.5] * 3, [n] * 3, one_at_a_time=True)
        idle = e.stats()
        assert idle["sequences_tracked"] == 0 and idle["result_blocks_free"] == idle["result_blocks"]
        got = _run(e, [0.5] * 3, [n] * 3)
        st = e.stats()
        for a, b in zip(solo, got):
            assert b["wav"].shape == (S.samples_for(n, 0.5),) and np.array_equal(a["tokens"], b["tokens"])
            assert np.array_equal(a["wav"], b["wav"])
        assert st["vocoder_batches"] - idle["vocoder_batches"] == 3          # two finish together and still go one per pass
        assert st["sequences_tracked"] == 0 and st["kv_blocks_free"] == idle["kv_blocks_free"] and st["kv_blocks_total"] == idle["kv_blocks_total"]
        assert st["result_blocks_free"] == st["result_blocks"]
        # at speed 1 the same two fit one pass, as before
        _run(e, [None] * 3, [n] * 3)
        assert e.stats()["vocoder_batches"] - st["vocoder_batches"] == 2
    finally:
        e.close()


# ---- 5. the facade ----
def test_generate_speech_with_speed():
    from auralis_amd import TTS, TTSRequest
    from auralis_amd.api.text import XTTSTokenizer
    from auralis_amd.api.xtts_engine import XTTSv2Engine
    native, gpt_sd, xtts_sd, cond, spk = make_engine(1, max_seqs=4, vocoder_fp16=True)
    tts = TTS(scheduler_max_concurrency=4).with_engine(XTTSv2Engine(native, XTTSTokenizer(None, synthetic=True), gpt_max_audio_tokens=14))
    voice = {"gpt_cond_latent": cond.numpy(), "speaker_embedding": spk.numpy()}
    try:
        def chunks(speed, stream):
            req = TTSRequest(text=PARA, speaker_files=[voice], language="en", seed=21, stream=stream, speed=speed)
            out = tts.generate_speech(req)
            return list(out) if stream else out
        base = chunks(1.0, True)
        fast = chunks(1.25, True)
        assert len(base) == len(fast) >= 2
        assert [c.token_length for c in base] == [c.token_length for c in fast]
        assert [len(c.array) for c in base] == [S.samples_for(c.token_length, 1.0) for c in base]
        assert [len(c.array) for c in fast] == [S.samples_for(c.token_length, 1.25) for c in fast]
        whole = chunks(1.25, False)
        assert whole.token_length == sum(c.token_length for c in fast)
        assert len(whole.array) == sum(S.samples_for(c.token_length, 1.25) for c in fast) < sum(len(c.array) for c in base)
        assert np.array_equal(whole.array, np.concatenate([c.array for c in fast]))
    finally:
        tts.close()
