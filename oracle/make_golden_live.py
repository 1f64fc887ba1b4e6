"""Generate tests/golden/live_reference.npz: what the REFERENCE's own modules return on the seeded inputs of the CPU tests that
compare the oracle with them (build container only; the tests use the live modules when the reference is present and this
fixture otherwise).

TEST INFRASTRUCTURE ONLY.  Usage: python -m oracle.make_golden_live
Stored (weights are the seeded synthetic ones, so only outputs are kept):
  cond_shapes      JSON {parameter name: shape} of ConditioningEncoder + PerceiverResampler + ResNetSpeakerEncoder
  cond_enc_h, cond_perceiver_l, cond_speaker   ConditioningEncoder / PerceiverResampler / speaker encoder outputs (cond_outputs)
  vocoder_T9       HifiDecoder on 9 seeded latent frames (vocoder_output)
  gpt_L<l>_X<n>_K<k>   GPT2Model.forward rows (gpt_rows) for every GPT_CASES entry
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "live_reference.npz")
GPT_CASES = [(1, 3, 1), (3, 17, 9)]


def cond_shapes():
    from oracle.ref_import import load_reference_hifigan, load_reference_xtts_layer
    le, pe, hg = load_reference_xtts_layer("latent_encoder"), load_reference_xtts_layer("perceiver_encoder"), load_reference_hifigan()
    ref = {}
    ref.update({"conditioning_encoder." + k: tuple(v.shape) for k, v in le.ConditioningEncoder(80, 1024, num_attn_heads=16).state_dict().items()})
    ref.update({"conditioning_perceiver." + k: tuple(v.shape) for k, v in pe.PerceiverResampler(
        dim=1024, depth=2, dim_context=1024, num_latents=32, dim_head=64, heads=8, ff_mult=4).state_dict().items()})
    se = hg.HifiDecoder().speaker_encoder
    ref.update({"hifigan_decoder.speaker_encoder." + k: tuple(v.shape) for k, v in se.state_dict().items()})
    return ref


def cond_mels():
    return (torch.randn(1, 80, 57, generator=torch.Generator().manual_seed(1)),
            torch.rand(2, 64, 120, generator=torch.Generator().manual_seed(2)) * 3.0)


def cond_outputs(cond_sd):
    """(encoder rows, perceiver latents) on cond_mels()[0] and the l2-normalised speaker embedding on cond_mels()[1]"""
    from oracle.ref_import import load_reference_hifigan, load_reference_xtts_layer
    le, pe = load_reference_xtts_layer("latent_encoder"), load_reference_xtts_layer("perceiver_encoder")
    enc = le.ConditioningEncoder(80, 1024, num_attn_heads=16).eval()
    enc.load_state_dict({k[len("conditioning_encoder."):]: v for k, v in cond_sd.items() if k.startswith("conditioning_encoder.")})
    per = pe.PerceiverResampler(dim=1024, depth=2, dim_context=1024, num_latents=32, dim_head=64, heads=8, ff_mult=4).eval()
    per.load_state_dict({k[len("conditioning_perceiver."):]: v for k, v in cond_sd.items() if k.startswith("conditioning_perceiver.")})
    se = load_reference_hifigan().HifiDecoder().speaker_encoder.eval()
    se.load_state_dict({k[len("hifigan_decoder.speaker_encoder."):]: v for k, v in cond_sd.items()
                        if k.startswith("hifigan_decoder.speaker_encoder.")})
    se.use_torch_spec = False            # the torchaudio mel front-end is stubbed offline: feed the mel directly
    mel, mel_spk = cond_mels()
    with torch.no_grad():
        h = enc(mel)
        return h, per(h.permute(0, 2, 1)), se(mel_spk.clone(), l2_norm=True)


def vocoder_latents():
    torch.manual_seed(3)
    return torch.randn(1, 9, 1024)


def vocoder_output(xtts_sd, spk):
    from oracle.ref_import import build_reference_decoder
    dec = build_reference_decoder(xtts_sd)
    with torch.no_grad():
        return dec(vocoder_latents(), g=spk)


def gpt_case(dims, n_layer, n_text, n_tok):
    """The seeded inputs of one case: (gpt_sd, xtts_sd, conditioning rows, mel tokens)"""
    from auralis_amd.checkpoint import (make_synthetic_conditioning, make_synthetic_gpt, make_synthetic_text_ids,
                                        make_synthetic_xtts)
    from oracle import xtts_oracle as O
    gpt_sd = make_synthetic_gpt(dims.gpt, seed=77, n_layer=n_layer)
    xtts_sd = make_synthetic_xtts(dims, seed=77, gpt_sd=gpt_sd)
    cond, _ = make_synthetic_conditioning(dims)
    ids = list(make_synthetic_text_ids(dims, n_text=n_text, seed=3))
    toks = torch.randint(0, 1024, (n_tok,), generator=torch.Generator().manual_seed(n_tok)).tolist()
    return gpt_sd, xtts_sd, O.GPTOracle(gpt_sd, xtts_sd).build_cond(cond, ids), toks


def gpt_rows(gpt_sd, n_layer, c, toks):
    from oracle.ref_gpt_import import build_reference_gpt2model
    model = build_reference_gpt2model(gpt_sd, n_layer)
    n_tok = len(toks)
    with torch.no_grad():
        return model(input_ids=torch.tensor(toks), position_ids=torch.arange(1, n_tok + 1), kv_caches=[None] * n_layer,
                     attn_metadata=None, intermediate_tensors=None, input_embeds=[c[None]], starting_sequence_start_ids=[0],
                     is_profiling_run=False, is_logit_only=torch.tensor([False]))


def gpt_key(n_layer, n_text, n_tok):
    return f"gpt_L{n_layer}_X{n_text}_K{n_tok}"


def main():
    from auralis_amd.checkpoint import make_synthetic_conditioning, make_synthetic_conditioning_weights, make_synthetic_xtts
    from auralis_amd.config import XTTSDims
    dims = XTTSDims()
    out = {"cond_shapes": np.array(json.dumps({k: list(v) for k, v in cond_shapes().items()}, sort_keys=True))}
    h, lat, spk = cond_outputs(make_synthetic_conditioning_weights(dims, seed=99))
    out.update(cond_enc_h=h.numpy(), cond_perceiver_l=lat.numpy(), cond_speaker=spk.numpy())
    out["vocoder_T9"] = vocoder_output(make_synthetic_xtts(dims, seed=1234), make_synthetic_conditioning(dims)[1]).numpy()
    for case in GPT_CASES:
        gpt_sd, _, c, toks = gpt_case(dims, *case)
        out[gpt_key(*case)] = gpt_rows(gpt_sd, case[0], c, toks).numpy()
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: " + ", ".join(f"{k} {np.shape(v)}" for k, v in out.items()))


if __name__ == "__main__":
    main()
