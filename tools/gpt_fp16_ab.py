"""Same-box A/B of aur_config.gpt_fp16 against the exact engine, in ONE process (prints JSON lines; run on the GPU box).

  python tools/gpt_fp16_ab.py [--reps 4] [--tokens 280] [--kv]

Two engines of the bench configuration (30 layers, 64 slots, fp16-input vocoder, synthetic checkpoint of true shapes) are resident
at once: `exact` (default config) and `fp16` (gpt_fp16 = 1; with --kv both also run the fp16 K/V pool).  After one warm-up pass of
each, the workloads alternate engine by engine in ABBA order, so the two see the same box state:
  * C3: 64 sampled utterances, 70 text ids, fixed length (ignore_stop) -- wall ms per batch, audio samples/s, decode ms per step
    (aur_stats.decode_ms / decode_steps);
  * C2: one greedy utterance -- wall ms, decode ms per step (launch-bound: 154 launches a step for one row).
Then each engine runs C3 once more in profile mode (aur_set_profile: replay batches of 30 back-to-back launches per GEMM kind) for
the per-kind GEMM microseconds per launch and their sum per layer.  The last line is a summary with medians."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KINDS = ["qkv", "proj", "fc", "proj2", "head"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--tokens", type=int, default=280)
    ap.add_argument("--layers", type=int, default=30)
    ap.add_argument("--kv", action="store_true", help="both engines with the fp16 K/V pool (aur_config.kv_fp16)")
    a = ap.parse_args()
    import torch
    from auralis_amd._lib import NativeEngine
    from auralis_amd.checkpoint import make_synthetic_conditioning, make_synthetic_gpt, make_synthetic_text_ids, make_synthetic_xtts
    from auralis_amd.config import XTTSDims
    from auralis_amd.weights import pack_all
    assert torch.cuda.is_available(), "gpt_fp16_ab needs the MI355X"
    dims = XTTSDims()
    gpt_sd = make_synthetic_gpt(dims.gpt, seed=1234, n_layer=a.layers)
    packed = pack_all(gpt_sd, make_synthetic_xtts(dims, seed=1234, gpt_sd=gpt_sd))
    cond, spk = make_synthetic_conditioning(dims)
    ids = make_synthetic_text_ids(dims, n_text=70, seed=11)
    engines = {}
    for name, f16 in (("exact", False), ("fp16", True)):
        e = NativeEngine(n_layer=a.layers, max_seqs=64, vocoder_fp16=True, return_latents=False, kv_fp16=a.kv, gpt_fp16=f16)
        e.load_weights(packed)
        e.set_conditioning(1, cond.numpy(), spk.numpy())
        engines[name] = e

    def run(e, batch, sampled):
        e.sync()
        e.reset_stats()
        t0 = time.perf_counter()
        for b in range(batch):
            e.submit(ids, 1, temperature=0.75 if sampled else 0.0, top_p=0.85, top_k=50, repetition_penalty=5.0, max_tokens=a.tokens,
                     seed=b, ignore_stop=True)
        outs = e.run_until_done()
        dt = time.perf_counter() - t0
        s = e.stats()
        return {"wall_ms": dt * 1e3, "samples_per_s": sum(len(o["wav"]) for o in outs) / dt,
                "decode_ms_per_step": s["decode_ms"] / max(1, s["decode_steps"]), "steps": s["decode_steps"]}

    for name, e in engines.items():   # warm-up: every shape of both workloads
        run(e, 64, True)
        run(e, 1, False)
    res = {n: {"c3": [], "c2": []} for n in engines}
    for r in range(a.reps):
        order = ["exact", "fp16"] if r % 2 == 0 else ["fp16", "exact"]
        for wl, batch, sampled in (("c3", 64, True), ("c2", 1, False)):
            for name in order:
                m = run(engines[name], batch, sampled)
                res[name][wl].append(m)
                print(json.dumps({"rep": r, "engine": name, "workload": wl, **{k: round(v, 4) for k, v in m.items()}}), flush=True)
    prof = {}
    for name, e in engines.items():
        e.set_profile(8)
        run(e, 64, True)
        s = e.stats()
        e.set_profile(0)
        us = [s["gemm_kind_ms"][k] * 1e3 / max(1, s["gemm_kind_launches"][k]) for k in range(5)]
        prof[name] = {"gemm_us_per_launch": dict(zip(KINDS, [round(u, 3) for u in us])), "gemm_us_per_layer": round(sum(us[:4]), 3),
                      "gemm_GBps": round(sum(s["gemm_kind_bytes"][:4]) / max(1e-9, sum(s["gemm_kind_ms"][:4]) * 1e-3) / 1e9, 1)}
        print(json.dumps({"engine": name, "profile_c3": prof[name]}), flush=True)

    def med(name, wl, key):
        return round(statistics.median(m[key] for m in res[name][wl]), 4)
    summary = {"kv_fp16": a.kv, "reps": a.reps, "tokens": a.tokens}
    for name in engines:
        summary[name] = {"c3_wall_ms": med(name, "c3", "wall_ms"), "c3_samples_per_s": med(name, "c3", "samples_per_s"),
                         "c3_decode_ms_per_step": med(name, "c3", "decode_ms_per_step"), "c2_wall_ms": med(name, "c2", "wall_ms"),
                         "c2_decode_ms_per_step": med(name, "c2", "decode_ms_per_step"), **prof[name]}
    summary["fp16_over_exact"] = {
        "c3_samples_per_s": round(summary["fp16"]["c3_samples_per_s"] / summary["exact"]["c3_samples_per_s"], 4),
        "c3_decode_step": round(summary["fp16"]["c3_decode_ms_per_step"] / summary["exact"]["c3_decode_ms_per_step"], 4),
        "c2_decode_step": round(summary["fp16"]["c2_decode_ms_per_step"] / summary["exact"]["c2_decode_ms_per_step"], 4),
        "gemm_us_per_layer": round(summary["fp16"]["gemm_us_per_layer"] / summary["exact"]["gemm_us_per_layer"], 4)}
    for e in engines.values():
        e.close()
    print(json.dumps({"summary": summary}), flush=True)


if __name__ == "__main__":
    main()
