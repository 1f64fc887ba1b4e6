"""GPU: aur_config.gpt_fp16 -- the four per-layer GPT linears streamed as fp16 by the decode GEMMs (gemm_rows_kernel PREC 2).

The mode is the exact model on the effective weights W'' of weights.gpt_fp16_effective (include/auralis_amd.h).  The synthetic
checkpoint's LayerNorms are gamma = 1, beta = 0, which makes the folding rule trivial, so the engine-level tests load it with
seeded LayerNorm parameters (gamma = 1 + 0.2 N(0,1), beta = 0.05 N(0,1)).  Everything is compared GPU against GPU or against the
CPU oracle run here; the last test only REPORTS how far the mode drifts from the exact goldens (not part of the contract)."""
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from auralis_amd.weights import fp16_effective_matrix, gpt_fp16_effective, pack_all
from tests.gpu_util import SPK_KEY, make_engine, packed_weights, rms

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REPORT = os.path.join(os.environ.get("AUR_REPORT_DIR", "out"), "gpt_fp16_report.json")   # (/out/ is git-ignored)
SAMPLING = dict(temperature=0.75, top_p=0.85, top_k=50, repetition_penalty=5.0)
T = 280


def _gelu_new(x):
    return 0.5 * x * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (x + 0.044715 * x ** 3)))


def _first_diff(a, b):
    a, b = list(a), list(b)
    for i in range(min(len(a), len(b))):
        if a[i] != b[i]:
            return i
    return None if len(a) == len(b) else min(len(a), len(b))


# ---- the kernel alone ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kern():
    e16, *_ = make_engine(1, max_seqs=8, gpt_fp16=True)
    e32, *_ = make_engine(1, max_seqs=8)
    yield e16, e32
    e16.close()
    e32.close()


@pytest.mark.parametrize("M,N,K,epi,ln", [(64, 3072, 1024, 0, True), (64, 4096, 1024, 1, True), (64, 1024, 1024, 2, False),
                                          (64, 1024, 4096, 2, False), (64, 1088, 1024, 0, False), (1, 4096, 1024, 1, True),
                                          (17, 1024, 4096, 2, False), (37, 3072, 1024, 0, True), (5, 1088, 1024, 0, False),
                                          (130, 4096, 1024, 1, True), (200, 1024, 4096, 0, False), (48, 1024, 1024, 2, False)])
def test_fp16_decode_gemm_computes_the_effective_weights(kern, M, N, K, epi, ln):
    """PREC 2 against float64 of LN(X) W'' + b: as accurate as the exact engine is on its own weights, and measurably NOT the raw W."""
    e16, e32 = kern
    g = torch.Generator().manual_seed(M * 11 + N + K + epi)
    X = torch.randn(M, K, generator=g) * (3.0 if ln else 1.0) + (0.5 if ln else 0.0)
    W = torch.randn(K, N, generator=g) * 0.05
    bias = torch.randn(N, generator=g)
    gamma = torch.randn(K, generator=g) if ln else None
    beta = torch.randn(K, generator=g) if ln else None
    res = torch.randn(M, N, generator=g) if epi == 2 else None
    A = (F.layer_norm(X.double(), (K,), gamma.double(), beta.double(), 1e-5) if ln else X.double()).numpy()
    _, Weff = fp16_effective_matrix(W.numpy(), None if gamma is None else gamma.numpy())

    def ref(Wm):
        r = A @ np.asarray(Wm, np.float64) + bias.double().numpy()
        if epi == 1:
            r = _gelu_new(r)
        if epi == 2:
            r = r + res.double().numpy()
        return r
    args = (X.numpy(), W.numpy(), bias.numpy(), None if gamma is None else gamma.numpy(), None if beta is None else beta.numpy(),
            None if res is None else res.numpy(), epi)
    got16, got32 = e16.dbg_gemm_rows(*args), e32.dbg_gemm_rows(*args)
    r_eff, r_raw = ref(Weff), ref(W.numpy())
    err16, err32, err_raw = np.abs(got16 - r_eff).max(), np.abs(got32 - r_raw).max(), np.abs(got16 - r_raw).max()
    print(f"M={M} N={N} K={K} epi={epi} ln={ln}: fp16 vs W'' {err16:.3e}, exact vs W {err32:.3e}, fp16 vs raw W {err_raw:.3e}")
    assert err16 <= 1.5 * err32 + 1e-6 * max(1.0, np.abs(r_eff).max()), (err16, err32)
    assert err_raw >= 10.0 * err16, (err_raw, err16)


def test_fp16_decode_gemm_is_batch_invariant_bitwise(kern):
    e16, _ = kern
    g = torch.Generator().manual_seed(5)
    for K, N, ln in ((1024, 4096, True), (4096, 1024, False), (1024, 1024, False), (1024, 3072, True)):
        X = torch.randn(150, K, generator=g)
        W = torch.randn(K, N, generator=g) * 0.05
        gamma = (1.0 + 0.2 * torch.randn(K, generator=g)).numpy() if ln else None
        beta = (0.05 * torch.randn(K, generator=g)).numpy() if ln else None
        full = e16.dbg_gemm_rows(X.numpy(), W.numpy(), None, gamma, beta, None, 0)
        for m in (1, 16, 17, 33, 64, 100):
            part = e16.dbg_gemm_rows(X[:m].numpy(), W.numpy(), None, gamma, beta, None, 0)
            assert np.array_equal(full[:m], part), (K, N, m)


@pytest.mark.parametrize("M", [1, 16, 32])
def test_fp16_ksplit_projection_hand_off(kern, M):
    e16, _ = kern
    assert e16.dbg_gemm_rows_ksplit_stress(M, 3000) == 0


# ---- engines on a checkpoint with non-trivial LayerNorms --------------------------------------------------------------------------
def _with_ln(gpt_sd, seed=2024):
    g = torch.Generator().manual_seed(seed)
    sd = dict(gpt_sd)
    for key in sorted(k for k in gpt_sd if re.fullmatch(r"gpt\.h\.\d+\.ln_[12]\.(weight|bias)", k)):
        n = gpt_sd[key].numel()
        sd[key] = 1.0 + 0.2 * torch.randn(n, generator=g) if key.endswith("weight") else 0.05 * torch.randn(n, generator=g)
    return sd


def _engine(packed, n_layer, max_seqs, **kw):
    from auralis_amd._lib import NativeEngine
    from auralis_amd.checkpoint import make_synthetic_conditioning
    from auralis_amd.config import XTTSDims
    e = NativeEngine(n_layer=n_layer, max_seqs=max_seqs, **kw)
    e.load_weights(packed)
    cond, spk = make_synthetic_conditioning(XTTSDims())
    e.set_conditioning(SPK_KEY, cond.numpy(), spk.numpy())
    return e


def _c2_prompts():
    g, gw = np.load(os.path.join(GOLD, "c2_L30_T280.npz")), np.load(os.path.join(GOLD, "c2w_L30_T280.npz"))
    return {"c2": g["text_ids"].tolist(), "c2w_12": gw["text_ids_12"].tolist(), "c2w_13": gw["text_ids_13"].tolist()}


def _c3_ids():
    return np.load(os.path.join(GOLD, "c3w_L30_T280.npz"))["text_ids"].tolist()


def _run_c2(e, names=None):
    out = {}
    for name, ids in _c2_prompts().items():
        if names is None or name in names:
            e.submit(ids, SPK_KEY, temperature=0.0, max_tokens=T, ignore_stop=True)
            out[name] = e.run_until_done()[0]
    return out


def _run_c3(e, seeds):
    ids = _c3_ids()
    sid = {e.submit(ids, SPK_KEY, max_tokens=T, seed=s, ignore_stop=True, **SAMPLING): s for s in seeds}
    got = {sid[o["seq_id"]]: o for o in e.run_until_done()}
    assert len(got) == len(seeds)
    return got


@pytest.fixture(scope="module")
def ln30():
    """(gpt_sd with seeded LayerNorms, xtts_sd, the fp16 engine loaded with them, and its C2 / C3 results)"""
    _, gpt_sd, xtts_sd = packed_weights(30)
    sd = _with_ln(gpt_sd)
    e = _engine(pack_all(sd, xtts_sd), 30, 64, vocoder_fp16=True, gpt_fp16=True)
    res = {"c2": _run_c2(e), "c3": _run_c3(e, list(range(64)))}
    yield sd, xtts_sd, e, res
    e.close()


def test_engine_on_effective_weights_is_bitwise_the_engine_on_raw_weights(ln30):
    """Idempotence: an fp16 engine loaded with gpt_fp16_effective(W) produces the ids, latents and waveforms of one loaded with W."""
    sd, xtts_sd, _, res = ln30
    e = _engine(pack_all(gpt_fp16_effective(sd), xtts_sd), 30, 64, vocoder_fp16=True, gpt_fp16=True)
    try:
        c2 = _run_c2(e, {"c2"})["c2"]
        c3 = _run_c3(e, list(range(8)))
    finally:
        e.close()
    pairs = [("c2", c2, res["c2"]["c2"])] + [(f"c3 seed {s}", c3[s], res["c3"][s]) for s in range(8)]
    for name, a, b in pairs:
        assert a["tokens"].tolist() == b["tokens"].tolist(), name
        assert np.array_equal(a["latents"], b["latents"]), name
        assert np.array_equal(a["wav"], b["wav"]), name


def test_fp16_engine_equals_the_exact_engine_on_the_effective_weights(ln30, dims):
    """The contract: the fp16 engine on W is the exact engine on W'' = gpt_fp16_effective(W), up to fp32-class rounding: greedy ids
    of the three C2 prompts and sampled ids of all 64 C3 seeds equal, stash latents within 5e-3, waveforms within 1e-3 RMS / 1 %.
    A greedy divergence is accepted only at a genuine near-tie: the CPU oracle on W'' must show a top-2 margin below 1e-4 at that
    step, and the ids must agree before it."""
    sd, xtts_sd, _, res = ln30
    sd_eff = gpt_fp16_effective(sd)
    e = _engine(pack_all(sd_eff, xtts_sd), 30, 64, vocoder_fp16=True)
    try:
        c2 = _run_c2(e)
        c3 = _run_c3(e, list(range(64)))
    finally:
        e.close()
    for name, ids in _c2_prompts().items():
        a, b = res["c2"][name], c2[name]
        d = _first_diff(a["tokens"], b["tokens"])
        if d is not None:
            from auralis_amd.checkpoint import make_synthetic_conditioning
            from oracle import xtts_oracle as O
            cond, _ = make_synthetic_conditioning(dims)
            gpt = O.GPTOracle(sd_eff, xtts_sd)
            ref = gpt.generate(gpt.build_cond(cond, ids), O.SamplingCfg(temperature=0.0, max_tokens=d + 1, ignore_stop=True),
                               return_debug=True)
            assert ref["tokens"][:d] == a["tokens"][:d].tolist(), (name, d)
            assert ref["margins"][d] < 1e-4, (name, d, ref["margins"][d])
            continue
        assert np.abs(a["latents"] - b["latents"]).max() < 5e-3, name
        err, sig = rms(a["wav"] - b["wav"]), rms(b["wav"])
        assert err <= 1e-3 and err <= 1e-2 * sig, (name, err, sig)
    bad = [(s, _first_diff(res["c3"][s]["tokens"], c3[s]["tokens"])) for s in range(64)
           if res["c3"][s]["tokens"].tolist() != c3[s]["tokens"].tolist()]
    assert not bad, f"(seed, first differing step): {bad}"


def test_fp16_c3_sequences_equal_their_solo_runs(ln30):
    _, _, e, res = ln30
    ids = _c3_ids()
    for s in range(8):
        e.submit(ids, SPK_KEY, max_tokens=T, seed=s, ignore_stop=True, **SAMPLING)
        solo = e.run_until_done()[0]
        assert solo["tokens"].tolist() == res["c3"][s]["tokens"].tolist(), s
        assert np.array_equal(solo["wav"], res["c3"][s]["wav"]), s


def test_fp16_engine_matches_the_oracle_on_effective_weights(dims):
    """Anchor: 3 layers, 60 greedy tokens; GPTOracle + the oracle vocoder on W'' on the CPU: ids bit-exact, waveform within 1e-3 RMS."""
    from auralis_amd.checkpoint import make_synthetic_conditioning, make_synthetic_text_ids
    from oracle import xtts_oracle as O
    _, gpt_sd, xtts_sd = packed_weights(3)
    sd = _with_ln(gpt_sd, seed=7)
    e = _engine(pack_all(sd, xtts_sd), 3, 2, gpt_fp16=True)
    try:
        ids = make_synthetic_text_ids(dims, n_text=24)
        e.submit(ids, SPK_KEY, temperature=0.0, max_tokens=60, ignore_stop=True)
        got = e.run_until_done()[0]
    finally:
        e.close()
    cond, spk = make_synthetic_conditioning(dims)
    gpt = O.GPTOracle(gpt_fp16_effective(sd), xtts_sd)
    c = gpt.build_cond(cond, ids)
    ref = gpt.generate(c, O.SamplingCfg(temperature=0.0, max_tokens=60, ignore_stop=True), return_debug=True)
    assert got["tokens"].tolist() == ref["tokens"], min(ref["margins"])
    lat_ref = gpt.second_pass_latents(c, ref["tokens"])[0]
    wav_ref = O.hifi_decoder_forward(O.vocoder_effective_weights(xtts_sd), lat_ref[None], spk).reshape(-1).numpy()
    assert got["wav"].shape == wav_ref.shape
    assert rms(got["wav"] - wav_ref) <= 1e-3, rms(got["wav"] - wav_ref)


def test_facade_fp16_equals_a_direct_fp16_engine(tmp_path, dims):
    """TTS().from_pretrained(dir, gpt="fp16") runs the fp16 engine: its audio equals a direct gpt_fp16 NativeEngine fed what the
    facade submitted; streaming equals non-streaming."""
    from auralis_amd import TTS, TTSRequest
    from auralis_amd.checkpoint import make_synthetic_conditioning, make_synthetic_gpt, make_synthetic_xtts, save_checkpoint
    gpt_sd = _with_ln(make_synthetic_gpt(dims.gpt, seed=1234, n_layer=2), seed=11)
    gpt_sd["mel_head.bias"][1025] = 3.0      # sequences stop by themselves after a handful of tokens
    xtts_sd = make_synthetic_xtts(dims, seed=1234, gpt_sd=gpt_sd)
    save_checkpoint(str(tmp_path), gpt_sd, xtts_sd, dims, synthetic_tokenizer=True)
    cond, spk = make_synthetic_conditioning(dims)
    voice = {"gpt_cond_latent": cond.numpy(), "speaker_embedding": spk.numpy()}
    text = "The quick brown fox jumps over the lazy dog near the river bank, and nobody saw it happen."
    tts = TTS(scheduler_max_concurrency=2).from_pretrained(str(tmp_path), gpt="fp16")
    try:
        native = tts.tts_engine.native
        sent, orig = [], native.submit

        def spy(*a, **kw):
            sent.append((a, kw))
            return orig(*a, **kw)
        native.submit = spy
        out = tts.generate_speech(TTSRequest(text=text, speaker_files=[voice], language="en", temperature=0.0, seed=5))
        assert len(sent) == 1 and len(out.array) > 0
        chunks = list(tts.generate_speech(TTSRequest(text=text, speaker_files=[voice], language="en", temperature=0.0, seed=5,
                                                     stream=True)))
        assert np.array_equal(np.concatenate([c.array for c in chunks]), out.array)
    finally:
        tts.close()
    a, kw = sent[0]
    key = kw["speaker_key"] if "speaker_key" in kw else a[1]
    e = _engine(pack_all(gpt_sd, xtts_sd), 2, 2, vocoder_fp16=True, gpt_fp16=True)
    try:
        e.set_conditioning(key, cond.numpy(), spk.numpy())
        e.submit(*a, **kw)
        direct = e.run_until_done()[0]
    finally:
        e.close()
    assert np.array_equal(direct["wav"], out.array)


def test_fp16_with_exact_gemms_or_out_of_range_weights_is_rejected():
    from auralis_amd._lib import AurError, NativeEngine
    with pytest.raises(AurError) as ei:
        NativeEngine(n_layer=1, max_seqs=2, gpt_fp16=True, gemm_f32_exact=True)
    assert ei.value.code == -1   # AUR_E_INVALID
    packed = dict(packed_weights(1)[0])
    w = packed["gpt.h.0.mlp.c_proj.w"].copy()
    w[3, 4] = 70000.0
    e = NativeEngine(n_layer=1, max_seqs=2, gpt_fp16=True)
    try:
        with pytest.raises(AurError) as ei:
            e.load_weights({**packed, "gpt.h.0.mlp.c_proj.w": w})
        assert ei.value.code == -1
    finally:
        e.close()


def test_drift_report_against_the_exact_goldens():
    """How far the reference's precision drifts from the exact goldens (the original checkpoint, gamma = 1): fp16 weights, and fp16
    weights with the fp16 K/V pool.  Only validity is asserted; the numbers go to
    $AUR_REPORT_DIR/gpt_fp16_report.json (default out/)."""
    packed, _, _ = packed_weights(30)
    g2, gw, g3 = (np.load(os.path.join(GOLD, n)) for n in ("c2_L30_T280.npz", "c2w_L30_T280.npz", "c3w_L30_T280.npz"))
    want = {"c2": (g2["tokens"], g2["latents"]), "c2w_12": (gw["tokens_12"], gw["latents_12"]),
            "c2w_13": (gw["tokens_13"], gw["latents_13"])}
    report = {}
    for mode, kw in (("gpt_fp16", {}), ("gpt_fp16+kv_fp16", {"kv_fp16": True})):
        e = _engine(packed, 30, 64, vocoder_fp16=True, gpt_fp16=True, **kw)
        try:
            c2, c3 = _run_c2(e), _run_c3(e, [int(s) for s in g3["seeds"]])
        finally:
            e.close()
        seqs = {}
        for name, (tok, lat) in want.items():
            o = c2[name]
            d = _first_diff(o["tokens"], tok)
            n = T if d is None else d
            seqs[name] = {"first_diff": d, "latent_err_equal_prefix": float(np.abs(o["latents"][:n] - lat[:n]).max()) if n else None}
        for k, s in enumerate(g3["seeds"].tolist()):
            seqs[f"c3_seed{s}"] = {"first_diff": _first_diff(c3[s]["tokens"], g3["tokens"][k])}
        for o in list(c2.values()) + list(c3.values()):
            assert len(o["tokens"]) == T and o["tokens"].min() >= 0 and o["tokens"].max() < 1026
            assert len(o["wav"]) > 0 and np.isfinite(o["wav"]).all()
        report[mode] = {"fraction_fully_equal": sum(v["first_diff"] is None for v in seqs.values()) / len(seqs), "sequences": seqs}
        print(mode, "fully equal:", report[mode]["fraction_fully_equal"])
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    with open(REPORT, "w") as f:
        json.dump(report, f, indent=1)
