"""Test doubles for the plugin over several engines (CPU): FakeNativeEngine with the two things that path needs on top -- the `speed`
field of submit and load() (aur_get_load)."""
from tests.fakes import FakeNativeEngine


class FakeLoadEngine(FakeNativeEngine):
    def submit(self, text_ids, speaker_key, speed=0.0, **kw):
        sid = super().submit(text_ids, speaker_key, **kw)
        self.submitted[-1]["speed"] = speed
        self.submitted[-1]["speaker_key"] = speaker_key
        return sid

    def load(self):
        """as aur_get_load; a fake sequence's `left` steps stand for max_tokens - generated"""
        waiting, running = list(self.waiting), list(self.running)
        return {"waiting": len(waiting), "running": len(running), "vocoding": 0, "free_slots": self.max_seqs - len(running),
                "token_budget": sum(s["left"] for s in waiting + running)}

    def poll(self, cap=64, want_latents=True, copy=True):
        """Sequence ids repeat across engines, so the audio names the chunk by its SEED here (request seed + chunk index): what a
        test of ordering across engines can tell apart."""
        import numpy as np
        seeds = {s["seq_id"]: s["seed"] for s in self.submitted}
        out = super().poll(cap, want_latents, copy)
        for item in out:
            if len(item["wav"]):
                item["wav"] = np.full(len(item["wav"]), float(seeds[item["seq_id"]]), dtype=np.float32)
        return out
