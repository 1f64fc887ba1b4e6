"""What the native FLAC encoding costs, on one engine in ONE process (prints JSON lines; run on the GPU box).

  python tools/flac_ab.py [--reps 3] [--tokens 280] [--layers 2]

(b) 64 sampled utterances of fixed length go through aur_submit without and with `encoding="flac"` in turn, `reps` rounds (after one
warm-up pass of each): aur_stats.vocoder_ms of the batch (the vocoder passes themselves; the encoder's three kernels and the copies of
an encoded pass run behind them on the same stream and are NOT inside that event pair) and the wall time, which holds everything.
The vocoder's time does not depend on the GPT's depth, so the default engine has two layers.
(c) one waveform of 312 064 samples (a 200-character utterance at 24 kHz, taken from the runs above and tiled) through aur_encode_flac
against flac.encode on this box's CPU, one thread; the two streams are compared.
Kernel times per kind come from a kernel trace of this tool (rocprofv3 --kernel-trace --stats -- python tools/flac_ab.py --reps 1):
flac_md5_kernel, flac_frame_kernel (quantisation, costs, Rice choice, bit packing and the CRC-16: one form was built, 36-byte pieces
per thread combined through the CRC's linearity, so there is no second CRC figure to set beside it), flac_assemble_kernel.
The last line is a summary with medians."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ONE_SHOT_SAMPLES = 312064


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tokens", type=int, default=280)
    ap.add_argument("--layers", type=int, default=2)
    a = ap.parse_args()
    import numpy as np
    import torch
    from auralis_amd._lib import NativeEngine
    from auralis_amd.api import codecs, flac
    from auralis_amd.checkpoint import make_synthetic_conditioning, make_synthetic_gpt, make_synthetic_text_ids, make_synthetic_xtts
    from auralis_amd.config import XTTSDims
    from auralis_amd.weights import pack_all
    assert torch.cuda.is_available(), "flac_ab needs the MI355X"
    dims = XTTSDims()
    gpt_sd = make_synthetic_gpt(dims.gpt, seed=1234, n_layer=a.layers)
    e = NativeEngine(n_layer=a.layers, max_seqs=64, vocoder_fp16=True, return_latents=False)
    e.load_weights(pack_all(gpt_sd, make_synthetic_xtts(dims, seed=1234, gpt_sd=gpt_sd)))
    cond, spk = make_synthetic_conditioning(dims)
    e.set_conditioning(1, cond.numpy(), spk.numpy())
    ids = make_synthetic_text_ids(dims, n_text=70, seed=11)

    def run(encoded):
        e.sync()
        e.reset_stats()
        t0 = time.perf_counter()
        for b in range(64):
            e.submit(ids, 1, temperature=0.75, top_p=0.85, top_k=50, repetition_penalty=5.0, max_tokens=a.tokens, seed=b, ignore_stop=True,
                     **({"encoding": "flac"} if encoded else {}))
        outs = e.run_until_done()
        dt = time.perf_counter() - t0
        s = e.stats()
        assert all(o["error"] == 0 and ("encoded" in o) == encoded for o in outs)
        return outs, {"vocoder_ms": s["vocoder_ms"], "vocoder_batches": s["vocoder_batches"], "wall_ms": dt * 1e3,
                      "samples": sum(len(o["wav"]) for o in outs), "stream_bytes": sum(len(o.get("encoded", ())) for o in outs)}

    wav = None
    for encoded in (False, True):   # warm-up: every shape, the encoder's buffers
        outs, _ = run(encoded)
        if encoded:
            o = outs[0]
            assert o["encoded"].tobytes() == flac.encode(codecs._to_int(o["wav"], 2), 24000, 16), "stream differs from the host writer's"
            wav = np.resize(o["wav"], ONE_SHOT_SAMPLES).astype(np.float32)
    res = {False: [], True: []}
    for rep in range(a.reps):
        for encoded in ((False, True) if rep % 2 == 0 else (True, False)):
            _, m = run(encoded)
            res[encoded].append(m)
            print(json.dumps({"rep": rep, "encoding": "flac" if encoded else None, **{k: round(v, 3) for k, v in m.items()}}), flush=True)
    one_gpu, one_host = [], []
    e.encode_flac([wav], [24000])   # warm-up: the one-shot entry's buffers
    for rep in range(a.reps):
        t0 = time.perf_counter()
        got = e.encode_flac([wav], [24000])[0]
        one_gpu.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        want = flac.encode(codecs._to_int(wav, 2), 24000, 16)
        one_host.append((time.perf_counter() - t0) * 1e3)
        assert got == want, "one-shot stream differs from the host writer's"
        print(json.dumps({"rep": rep, "one_shot_samples": ONE_SHOT_SAMPLES, "aur_encode_flac_ms": round(one_gpu[-1], 3),
                          "host_flac_encode_ms": round(one_host[-1], 3), "stream_bytes": len(got)}), flush=True)
    e.close()

    def med(key, encoded):
        return statistics.median(m[key] for m in res[encoded])
    summary = {"tokens": a.tokens, "layers": a.layers, "reps": a.reps,
               "vocoder_ms_64": {"none": round(med("vocoder_ms", False), 3), "flac": round(med("vocoder_ms", True), 3)},
               "wall_ms_64": {"none": round(med("wall_ms", False), 3), "flac": round(med("wall_ms", True), 3)},
               "encoder_extra_wall_ms_64": round(med("wall_ms", True) - med("wall_ms", False), 3),
               "one_shot_ms": {"aur_encode_flac": round(statistics.median(one_gpu), 3), "host_flac_encode": round(statistics.median(one_host), 3)}}
    print(json.dumps({"summary": summary}), flush=True)


if __name__ == "__main__":
    main()
