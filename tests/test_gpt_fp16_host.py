"""aur_config.gpt_fp16 on the host (no GPU): the effective-weight rule's host mirror (weights.gpt_fp16_effective) and the
`gpt=` / `kv=` knobs of XTTSv2Engine.from_pretrained down to the NativeEngine arguments."""
import numpy as np
import pytest
import torch

from auralis_amd.weights import GPT_FP16_LINEARS, gpt_fp16_effective


def _sd(n_layer=2, seed=3, H=64):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for i in range(n_layer):
        p = f"gpt.h.{i}."
        for ln in ("ln_1", "ln_2"):
            sd[p + ln + ".weight"] = 1.0 + 0.2 * torch.randn(H, generator=g)
            sd[p + ln + ".bias"] = 0.05 * torch.randn(H, generator=g)
        for lin, k, n in (("attn.c_attn", H, 3 * H), ("attn.c_proj", H, H), ("mlp.c_fc", H, 4 * H), ("mlp.c_proj", 4 * H, H)):
            sd[p + lin + ".weight"] = 0.02 * torch.randn(k, n, generator=g)
            sd[p + lin + ".bias"] = 0.02 * torch.randn(n, generator=g)
    sd["gpt.wte.weight"] = torch.randn(8, H, generator=g)
    return sd


def _f16(a):
    return np.asarray(a, np.float32).astype(np.float16)


def test_effective_weights_follow_the_rule():
    sd = _sd()
    eff = gpt_fp16_effective(sd)
    assert eff["gpt.wte.weight"] is sd["gpt.wte.weight"]   # everything else passes through
    for i in range(2):
        for lin, ln in GPT_FP16_LINEARS:
            key = f"gpt.h.{i}.{lin}.weight"
            w, we = sd[key].numpy(), eff[key].numpy()
            assert we.dtype == np.float32 and we.shape == w.shape
            if ln is None:
                assert np.array_equal(we, _f16(w).astype(np.float32))     # fp16-representable: the fp16 copy itself
                assert np.array_equal(_f16(we).astype(np.float32), we)
            else:
                g = sd[f"gpt.h.{i}.{ln}.weight"].numpy()[:, None]
                f = _f16(g * w)                                            # what the decode GEMM streams
                assert np.array_equal(_f16(g * we), f), key                 # fp16_rne(gamma * W'') == f
                assert np.array_equal(we, (f.astype(np.float32) / g).astype(np.float32)), key
            # the rounding is really applied (and is no more than fp16's half ulp, relative)
            assert not np.array_equal(we, w)
            assert np.all(np.abs(we - w) <= np.abs(w) * 2.0 ** -10 + 2.0 ** -22)


def test_effective_weights_are_idempotent_bit_for_bit():
    once = gpt_fp16_effective(_sd())
    twice = gpt_fp16_effective(once)
    for k in once:
        assert np.array_equal(once[k].numpy().view(np.uint32), twice[k].numpy().view(np.uint32)), k


def test_zero_gain_rows_take_the_plain_fp16_rounding():
    sd = _sd(n_layer=1)
    g = sd["gpt.h.0.ln_1.weight"].clone()
    g[[0, 5, 17]] = 0.0
    sd["gpt.h.0.ln_1.weight"] = g
    w = sd["gpt.h.0.attn.c_attn.weight"].numpy()
    we = gpt_fp16_effective(sd)["gpt.h.0.attn.c_attn.weight"].numpy()
    for k in (0, 5, 17):
        assert np.array_equal(we[k], _f16(w[k]).astype(np.float32))
    assert np.isfinite(we).all()
    again = gpt_fp16_effective({**sd, "gpt.h.0.attn.c_attn.weight": torch.from_numpy(we)})["gpt.h.0.attn.c_attn.weight"].numpy()
    assert np.array_equal(again.view(np.uint32), we.view(np.uint32))


@pytest.mark.parametrize("case", ["proj_range", "fold_range", "nan"])
def test_weights_the_mode_rejects_raise(case):
    sd = _sd(n_layer=1)
    if case == "proj_range":
        sd["gpt.h.0.mlp.c_proj.weight"][3, 4] = 70000.0                    # beyond fp16's 65504
    elif case == "fold_range":
        sd["gpt.h.0.ln_2.weight"][7] = 100.0
        sd["gpt.h.0.mlp.c_fc.weight"][7, 1] = 1000.0                       # gamma * W = 1e5 after folding
    else:
        sd["gpt.h.0.attn.c_attn.weight"][0, 0] = float("nan")
    with pytest.raises(ValueError, match="gpt_fp16"):
        gpt_fp16_effective(sd)


def test_effective_weights_of_a_folded_matrix_in_range_but_large_pass():
    sd = _sd(n_layer=1)
    sd["gpt.h.0.ln_2.weight"][7] = 10.0
    sd["gpt.h.0.mlp.c_fc.weight"][7, 1] = 6000.0                           # 60000 after folding: still an fp16 value
    assert np.isfinite(gpt_fp16_effective(sd)["gpt.h.0.mlp.c_fc.weight"].numpy()).all()


class _Captured(Exception):
    pass


@pytest.fixture(scope="module")
def ckpt_dir(tmp_path_factory):
    from auralis_amd.checkpoint import make_synthetic_gpt, make_synthetic_xtts, save_checkpoint
    from auralis_amd.config import XTTSDims
    dims = XTTSDims()
    root = tmp_path_factory.mktemp("ckpt")
    gpt_sd = make_synthetic_gpt(dims.gpt, seed=1234, n_layer=1)
    save_checkpoint(str(root), gpt_sd, make_synthetic_xtts(dims, seed=1234, gpt_sd=gpt_sd), dims, synthetic_tokenizer=True)
    return str(root)


def _engine_kwargs(monkeypatch, root, **kw):
    from auralis_amd import _lib
    from auralis_amd.api.xtts_engine import XTTSv2Engine
    seen = {}

    def fake(**a):
        seen.update(a)
        raise _Captured
    monkeypatch.setattr(_lib, "NativeEngine", fake)
    with pytest.raises(_Captured):
        XTTSv2Engine.from_pretrained(root, **kw)
    return seen


def test_from_pretrained_precision_knobs_reach_the_engine_config(monkeypatch, ckpt_dir):
    base = _engine_kwargs(monkeypatch, ckpt_dir)
    assert base["gpt_fp16"] is False and base["kv_fp16"] is False                     # defaults: the exact contract
    assert _engine_kwargs(monkeypatch, ckpt_dir, gpt="fp16")["gpt_fp16"] is True
    kv = _engine_kwargs(monkeypatch, ckpt_dir, kv="fp16")
    assert kv["kv_fp16"] is True and kv["gpt_fp16"] is False
    both = _engine_kwargs(monkeypatch, ckpt_dir, gpt="fp16", kv="fp16", vocoder="fp32")
    assert both["gpt_fp16"] and both["kv_fp16"] and both["vocoder_fp16"] is False
    assert {k: v for k, v in _engine_kwargs(monkeypatch, ckpt_dir, gpt="fp32", kv="fp32").items()} == base


def test_from_pretrained_forwards_the_knobs_through_the_facade(monkeypatch, ckpt_dir):
    from auralis_amd import TTS, _lib
    seen = {}

    def fake(**a):
        seen.update(a)
        raise _Captured
    monkeypatch.setattr(_lib, "NativeEngine", fake)
    with pytest.raises(_Captured):
        TTS().from_pretrained(ckpt_dir, gpt="fp16", kv="fp16")
    assert seen["gpt_fp16"] is True and seen["kv_fp16"] is True


@pytest.mark.parametrize("kw", [{"gpt": "bf16"}, {"kv": "fp8"}, {"gpt": "FP16"}, {"kv": None}])
def test_from_pretrained_rejects_other_precisions(monkeypatch, ckpt_dir, kw):
    from auralis_amd import _lib
    from auralis_amd.api.xtts_engine import XTTSv2Engine
    monkeypatch.setattr(_lib, "NativeEngine", lambda **a: pytest.fail("engine created despite a bad precision"))
    with pytest.raises(ValueError):
        XTTSv2Engine.from_pretrained(ckpt_dir, **kw)


def test_server_cli_offers_the_precision_switches():
    import inspect

    from auralis_amd.entrypoints import oai_server
    src = inspect.getsource(oai_server.main)
    assert '"--gpt"' in src and '"--kv"' in src and "gpt=a.gpt, kv=a.kv" in src


def test_config_struct_ends_with_gpt_fp16():
    from auralis_amd._lib import aur_config
    assert aur_config._fields_[-1] == ("gpt_fp16", __import__("ctypes").c_int32)
    assert aur_config().gpt_fp16 == 0
