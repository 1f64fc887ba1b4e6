"""What the native output sample rate costs, on one engine in ONE process (prints JSON lines; run on the GPU box).

  python tools/out_rate_ab.py [--reps 3] [--tokens 280] [--layers 2]

64 sampled utterances of fixed length go through aur_submit at 24000, 16000 and 48000 in turn, `reps` rounds (after one warm-up pass
of each): aur_stats.vocoder_ms of the batch -- the whole vocoder passes, conv_post's staging store and resample_out_kernel included
-- and the wall time.  The vocoder's time does not depend on the GPT's depth, so the default engine has two layers.  Beside it, the
host path the native rate replaces: TTSOutput.resample (scipy's resample_poly in float64) over the same 64 waveforms of the 24000
run, wall time on this box's CPU, one thread.  The last line is a summary with medians."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RATES = (24000, 16000, 48000)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tokens", type=int, default=280)
    ap.add_argument("--layers", type=int, default=2)
    a = ap.parse_args()
    import torch
    from auralis_amd import TTSOutput
    from auralis_amd._lib import NativeEngine
    from auralis_amd.checkpoint import make_synthetic_conditioning, make_synthetic_gpt, make_synthetic_text_ids, make_synthetic_xtts
    from auralis_amd.config import XTTSDims
    from auralis_amd.weights import pack_all
    assert torch.cuda.is_available(), "out_rate_ab needs the MI355X"
    dims = XTTSDims()
    gpt_sd = make_synthetic_gpt(dims.gpt, seed=1234, n_layer=a.layers)
    e = NativeEngine(n_layer=a.layers, max_seqs=64, vocoder_fp16=True, return_latents=False)
    e.load_weights(pack_all(gpt_sd, make_synthetic_xtts(dims, seed=1234, gpt_sd=gpt_sd)))
    cond, spk = make_synthetic_conditioning(dims)
    e.set_conditioning(1, cond.numpy(), spk.numpy())
    ids = make_synthetic_text_ids(dims, n_text=70, seed=11)

    def run(rate):
        e.sync()
        e.reset_stats()
        t0 = time.perf_counter()
        for b in range(64):
            e.submit(ids, 1, temperature=0.75, top_p=0.85, top_k=50, repetition_penalty=5.0, max_tokens=a.tokens, seed=b, ignore_stop=True,
                     **({} if rate == 24000 else {"sample_rate": rate}))
        outs = e.run_until_done()
        dt = time.perf_counter() - t0
        s = e.stats()
        assert all(o["error"] == 0 and o["sample_rate"] == rate for o in outs)
        return outs, {"vocoder_ms": s["vocoder_ms"], "vocoder_batches": s["vocoder_batches"], "wall_ms": dt * 1e3,
                      "samples": sum(len(o["wav"]) for o in outs)}

    wavs = None
    for rate in RATES:   # warm-up: every shape, the staging buffer
        outs, _ = run(rate)
        if rate == 24000:
            wavs = [o["wav"] for o in outs]
    res = {r: [] for r in RATES}
    host = {r: [] for r in RATES if r != 24000}
    for rep in range(a.reps):
        for rate in (RATES if rep % 2 == 0 else RATES[::-1]):
            _, m = run(rate)
            res[rate].append(m)
            print(json.dumps({"rep": rep, "rate": rate, **{k: round(v, 3) for k, v in m.items()}}), flush=True)
        for rate in host:
            t0 = time.perf_counter()
            n = sum(len(TTSOutput(array=w, sample_rate=24000).resample(rate).array) for w in wavs)
            host[rate].append((time.perf_counter() - t0) * 1e3)
            print(json.dumps({"rep": rep, "rate": rate, "host_resample_ms_64": round(host[rate][-1], 3), "samples": n}), flush=True)
    e.close()
    med = {r: statistics.median(m["vocoder_ms"] for m in res[r]) for r in RATES}
    summary = {"tokens": a.tokens, "layers": a.layers, "reps": a.reps,
               "vocoder_ms_64": {str(r): round(med[r], 3) for r in RATES},
               "wall_ms_64": {str(r): round(statistics.median(m["wall_ms"] for m in res[r]), 3) for r in RATES},
               "native_extra_ms_64": {str(r): round(med[r] - med[24000], 3) for r in host},
               "host_resample_ms_64": {str(r): round(statistics.median(host[r]), 3) for r in host}}
    print(json.dumps({"summary": summary}), flush=True)


if __name__ == "__main__":
    main()
