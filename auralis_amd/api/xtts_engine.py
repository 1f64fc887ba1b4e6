"""XTTSv2Engine — the reference's engine plugin (src/auralis/models/xttsv2/XTTSv2.py:39-820) re-based on the HIP
library: same public methods, same return shapes; vLLM, the second GPT pass and the torch HiFi-GAN are replaced by
aur_submit / aur_step / aur_poll_finished.

`speaker_files` may be reference audio (paths or bytes; RIFF/WAVE and FLAC natively, api/codecs.py): conditioning is computed
once per speaker on the GPU by the HIP kernels behind aur_compute_conditioning (csrc/cond_net.h, SURVEY §8f #1;
auralis_amd/conditioning.py is the PyTorch restatement the tests compare it with), a path/bytes of an .npz holding
`gpt_cond_latent` [1,32,1024] and `speaker_embedding` [1,512,1], or a dict / tuple with those arrays."""
from __future__ import annotations

import asyncio
import collections
import hashlib
import json
import os
import threading
import time
from typing import Any, AsyncGenerator, List, Optional, Sequence, Tuple

import numpy as np

from .dispatch import ChunkPlacer, EngineUnavailable
from .driver import EngineDriver
from .engine_base import BaseAsyncTTSEngine, ConditioningConfig, register_model
from .output import TTSOutput
from .requests import TTSRequest
from .text import XTTSTokenizer


try:                       # 133 KB per request: xxh3 takes ~10 us, blake2b ~190 us of the event-loop thread
    from xxhash import xxh3_64 as _Hash64
except ImportError:        # same role, slower
    def _Hash64():
        return hashlib.blake2b(digest_size=8)


def _content_key(g: np.ndarray, s: np.ndarray) -> int:
    """64-bit key of a voice's conditioning CONTENT (fed through the buffer protocol: no copy).  Keys are local to a process."""
    h = _Hash64()
    h.update(np.ascontiguousarray(g).data)
    h.update(np.ascontiguousarray(s).data)
    return int.from_bytes(h.digest(), "little")


class ChunkHandle:
    """Opaque per-chunk "token generator" handed to the facade (the reference passes a vLLM async generator)."""

    def __init__(self, future: "asyncio.Future", request_id: str, n_text: int):
        self.future = future
        self.request_id = request_id
        self.n_text = n_text

    def cancel(self):
        """Nobody will read this chunk: stop it in the engine (EngineDriver -> aur_cancel).  Nothing happens once it is resolved."""
        fut = self.future
        if not fut.done():
            fut.get_loop().call_soon_threadsafe(fut.cancel)


class _Chunk:
    """One chunk on its way through the placer (several engines): its future, what to submit, and where it is."""
    __slots__ = ("future", "loop", "seq", "key", "g", "s", "engine", "sid")

    def __init__(self, future, loop, seq, key, g, s):
        self.future, self.loop, self.seq, self.key, self.g, self.s = future, loop, seq, key, g, s
        self.engine = -1      # index of the engine it was placed on (-1: still in the placer's queue)
        self.sid = None       # its sequence id there


class XTTSv2Engine(BaseAsyncTTSEngine):
    model_type = "xtts"

    def __init__(self, native_engine: Any, tokenizer: XTTSTokenizer, max_concurrency: int = 10,
                 gpt_max_audio_tokens: int = 605, conditioning_weights: Optional[dict] = None):
        """`native_engine`: one engine, or a sequence of them (one per GPU; the same GPU may carry more than one).  With a sequence
        the plugin holds `natives`, one EngineDriver each in `drivers`, and a ChunkPlacer (api/dispatch.py) that decides where a
        chunk runs; `native` / `driver` stay as names of the first.  `max_concurrency` is slots PER ENGINE."""
        many = isinstance(native_engine, (list, tuple))
        self.natives = list(native_engine) if many else [native_engine]
        if not self.natives:
            raise ValueError("XTTSv2Engine needs at least one native engine")
        native_engine = self.natives[0]
        self.native = native_engine
        self.conditioning_weights = conditioning_weights   # xtts-v2.safetensors tensors of the once-per-speaker modules
        self._cond_cache = collections.OrderedDict()   # LRU, bounded (a serving process sees an open-ended set of voices)
        self._cond_cache_max = 64
        self.tokenizer = tokenizer
        self.max_concurrency = max_concurrency
        self.gpt_max_audio_tokens = gpt_max_audio_tokens
        self.driver = EngineDriver(native_engine)
        self.drivers = [self.driver] + [EngineDriver(n) for n in self.natives[1:]]
        # one engine: no placer, chunks go straight to its driver as they always did
        self._placer: Optional[ChunkPlacer] = None
        if len(self.natives) > 1:
            self._placer_lock = threading.Lock()     # every call into the placer, from the event loop and from the driver threads
            self._placer = ChunkPlacer([int(getattr(n, "max_seqs", max_concurrency)) for n in self.natives], self._place,
                                       budget=lambda e: self.natives[e].load()["token_budget"],
                                       running=lambda e: self.natives[e].load()["running"])
            self._speakers_on = [dict() for _ in self.natives]   # engines without aur_has_conditioning (test doubles)
        self._speakers = {}
        self._seed_counter = 0
        # bench / test knob (aur_seq_desc.ignore_stop): every chunk runs to gpt_max_audio_tokens whatever it samples, so that
        # runs do identical work (SURVEY 8d "fixed-length mode"); never set by from_pretrained
        self.fixed_length = False

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path: str, max_concurrency: int = 10, device: Optional[int] = None,
                        vocoder: str = "fp16", gpt: str = "fp32", kv: str = "fp32", devices: Optional[Sequence[int]] = None,
                        **kwargs) -> "XTTSv2Engine":
        """Load a checkpoint directory in the reference's on-disk format (checkpoint.py docstring).  kwargs the
        reference forwards to vLLM (tensor_parallel_size, pipeline_parallel_size, gpt_model, torch_dtype, device_map;
        XTTSv2.py:235-243) are accepted; tp/pp other than 1 are rejected (the path shards by utterance).
        `admit_min_batch` / `vocoder_min_batch` are the batcher's two grouping knobs, `max_speakers` the size of the engine's voice
        table (include/auralis_amd.h, aur_config).  gpt="fp16" keeps the four per-layer GPT linears as fp16 for the decode GEMMs
        (aur_config.gpt_fp16: the exact model on effective weights, weights.gpt_fp16_effective), kv="fp16" the K/V pool
        (aur_config.kv_fp16); "fp32" (default) is the exact contract for both.

        `device` (default 0): the GPU of the one engine.  `devices=[0, 1, ...]`: one engine per entry, all in this process, behind
        a ChunkPlacer; the checkpoint is read and packed once and loaded into each.  A device may appear twice (two engines on one
        GPU).  `max_concurrency` is slots PER ENGINE: devices=[0, 1, 2, 3] with max_concurrency=64 decodes up to 256 chunks at
        once.  Passing both `device` and `devices` is a ValueError."""
        if device is not None and devices is not None:
            raise ValueError("pass device= (one engine) or devices= (one engine per entry), not both")
        if devices is not None:
            devices = [int(d) for d in devices]
            if not devices:
                raise ValueError("devices= needs at least one device index")
        device = 0 if device is None else device
        from .._lib import NativeEngine
        from ..checkpoint import load_checkpoint, read_checkpoint_config
        from ..weights import pack_all
        for knob, v in (("gpt", gpt), ("kv", kv)):
            if v not in ("fp32", "fp16"):
                raise ValueError(f"{knob}={v!r}: expected 'fp32' or 'fp16'")
        if kwargs.get("tensor_parallel_size", 1) != 1 or kwargs.get("pipeline_parallel_size", 1) != 1:
            raise ValueError("the MI355X path replicates the 0.4 B-parameter model per GPU; use one engine per GPU")
        gpt_sd, xtts_sd = load_checkpoint(pretrained_model_name_or_path)
        # both config.json are read and checked against what the kernels are compiled for (XTTSv2.py:276-277 builds
        # XTTSGPTConfig / XTTSConfig from them); the activation and the generation length come from the file
        ck = read_checkpoint_config(pretrained_model_name_or_path, gpt_sd)
        # vocoder="fp16": HiFi-GAN convs on fp16-input / fp32-accumulate MFMA (waveform within 1e-5 RMS of the fp32
        # path, the reference's own GPU path autocasts to fp16); vocoder="fp32": exact-f32 MFMA parity mode
        def make(dev):
            return NativeEngine(n_layer=ck.n_layer, max_seqs=max(1, max_concurrency), device=dev,
                                vocoder_fp16=(vocoder == "fp16"), return_latents=False, gelu_erf=ck.gelu_erf,
                                admit_min_batch=int(kwargs.get("admit_min_batch", 0)), vocoder_min_batch=int(kwargs.get("vocoder_min_batch", 0)),
                                max_speakers=int(kwargs.get("max_speakers", 0)), urgent_rows=int(kwargs.get("urgent_rows", 0)),
                                gpt_fp16=(gpt == "fp16"), kv_fp16=(kv == "fp16"))
        packed = pack_all(gpt_sd, xtts_sd)
        packed_cond = None
        if any(k.startswith("conditioning_encoder.") for k in xtts_sd):
            from ..weights import pack_conditioning
            packed_cond = pack_conditioning(xtts_sd)
        natives = []
        for dev in ([device] if devices is None else devices):
            native = make(dev)
            natives.append(native)
            native.load_weights(packed)
            if packed_cond is not None:
                native.load_weights(packed_cond)
        tok_file = None
        for cand in ("tokenizer.json", os.path.join("gpt", "tokenizer.json")):
            p = os.path.join(pretrained_model_name_or_path, cand)
            if os.path.isfile(p):
                tok_file = p
        synthetic_tok = False
        cfg_path = os.path.join(pretrained_model_name_or_path, "core_xttsv2", "config.json")
        if tok_file is None and os.path.isfile(cfg_path):
            with open(cfg_path) as f:
                synthetic_tok = bool(json.load(f).get("synthetic_tokenizer", False))
        vocab = xtts_sd["text_embedding.weight"].shape[0]
        cond_w = {k: v for k, v in xtts_sd.items()
                  if k.startswith(("conditioning_", "hifigan_decoder.speaker_encoder.", "mel_stats"))}
        return cls(natives[0] if devices is None else natives, XTTSTokenizer(tok_file, vocab_size=vocab, synthetic=synthetic_tok), max_concurrency=max_concurrency,
                   gpt_max_audio_tokens=ck.gpt_max_audio_tokens,
                   conditioning_weights=cond_w if any(k.startswith("conditioning_encoder.") for k in cond_w) else None)

    @property
    def conditioning_config(self) -> ConditioningConfig:
        return ConditioningConfig(speaker_embeddings=True, gpt_like_decoder_conditioning=True)

    @property
    def device(self):
        return "cuda"

    @property
    def dtype(self):
        return "float32"

    def get_memory_usage_curve(self):
        """KV blocks per concurrent sequence (replaces the vLLM gpu_memory_utilization heuristic, XTTSv2.py:152-171)."""
        s = self.native.stats()
        per_seq_mb = 66 * 2 * 16 * 16 * 64 * 4 * self.native.n_layer / 2 ** 20
        out = {"kv_mb_per_sequence": per_seq_mb, "kv_blocks_total": s.get("kv_blocks_total", 0)}
        if self._placer is not None:   # several engines: the values above are the first one's, every engine's are listed
            out["engines"] = [{"kv_mb_per_sequence": 66 * 2 * 16 * 16 * 64 * 4 * n.n_layer / 2 ** 20,
                               "kv_blocks_total": n.stats().get("kv_blocks_total", 0), "max_seqs": getattr(n, "max_seqs", None),
                               "device": getattr(n, "device", None)} for n in self.natives]
        return out

    def load(self) -> List[dict]:
        """aur_get_load of every engine, in `natives` order: {waiting, running, vocoding, free_slots, token_budget} (host only; safe
        while the engines step)."""
        return [n.load() for n in self.natives]

    def _least_loaded_native(self):
        """Where once-per-voice work (aur_compute_conditioning) runs: with several engines, the one with the least ahead of it."""
        if self._placer is None:
            return self.native
        loads = self.load()
        e = min(range(len(loads)), key=lambda i: (loads[i]["waiting"] + loads[i]["running"] + loads[i]["vocoding"], loads[i]["token_budget"], i))
        return self.natives[e]

    # ------------------------------------------------------------------ conditioning
    async def get_audio_conditioning(self, audio_reference, max_ref_length=30, gpt_cond_len=6, gpt_cond_chunk_len=6,
                                     librosa_trim_db=None, sound_norm_refs=False, load_sr=22050):
        """-> (gpt_cond_latent [1,32,1024], speaker_embedding [1,512,1]) as float32 numpy arrays."""
        refs = list(audio_reference) if isinstance(audio_reference, (list, tuple)) else [audio_reference]
        if len(refs) == 2 and hasattr(refs[0], "shape") and hasattr(refs[1], "shape"):
            refs = [{"gpt_cond_latent": refs[0], "speaker_embedding": refs[1]}]
        ref = refs[0]

        def _is_npz(r):
            return (isinstance(r, str) and r.endswith(".npz")) or (isinstance(r, (bytes, bytearray)) and r[:2] == b"PK")
        if isinstance(ref, dict):
            g, s = ref["gpt_cond_latent"], ref["speaker_embedding"]
        elif _is_npz(ref):
            import io
            z = np.load(ref if isinstance(ref, str) else io.BytesIO(ref))
            g, s = z["gpt_cond_latent"], z["speaker_embedding"]
        else:
            if self.conditioning_weights is None:
                raise NotImplementedError(
                    "this checkpoint carries no conditioning_encoder / perceiver / speaker_encoder weights: pass "
                    "precomputed conditioning (.npz or dict with gpt_cond_latent [1,32,1024], speaker_embedding [1,512,1])")
            from .. import conditioning as Cn
            # cache key = full content of every reference (a path is keyed by the bytes it holds now, not by its name) + every
            # parameter that changes the result
            hk = hashlib.blake2b(digest_size=16)
            for r in refs:
                if isinstance(r, (bytes, bytearray, memoryview)):
                    data = bytes(r)
                else:
                    with open(r, "rb") as f:
                        data = f.read()
                hk.update(len(data).to_bytes(8, "little"))
                hk.update(data)
            hk.update(f"{max_ref_length}/{gpt_cond_len}/{gpt_cond_chunk_len}/{librosa_trim_db}/{sound_norm_refs}/{load_sr}".encode())
            key = hk.digest()
            if key in self._cond_cache:
                self._cond_cache.move_to_end(key)
            else:
                hip = getattr(self._least_loaded_native(), "compute_conditioning", None)
                if hip is None:
                    raise RuntimeError("the engine has no compute_conditioning entry point: speaker conditioning from reference "
                                       "audio runs in HIP (aur_compute_conditioning); there is no PyTorch fallback in the product")

                # loader on the host (decode, mono, resample to 22 050 Hz, clip: utilities.py:74-98), networks in HIP
                def _run():
                    pcm = []
                    for r in refs:
                        a = Cn.load_audio(r, load_sr)
                        if load_sr != 22050:
                            a = Cn.resample(a, load_sr, 22050)
                        pcm.append(a[0].numpy())
                    return hip(pcm, max_ref_length=max_ref_length, gpt_cond_len=gpt_cond_len,
                               gpt_cond_chunk_len=gpt_cond_chunk_len, sound_norm_refs=sound_norm_refs)
                self._cond_cache[key] = await asyncio.to_thread(_run)
                while len(self._cond_cache) > self._cond_cache_max:
                    self._cond_cache.popitem(last=False)
            g, s = self._cond_cache[key]
        g = np.asarray(getattr(g, "numpy", lambda: g)(), dtype=np.float32).reshape(1, 32, 1024)
        s = np.asarray(getattr(s, "numpy", lambda: s)(), dtype=np.float32).reshape(1, 512, 1)
        return g, s

    def _register_speaker(self, g: np.ndarray, s: np.ndarray) -> int:
        """Content-addressed speaker key.  The engine's speaker table is bounded (aur_config.max_speakers) and evicts the least
        recently used idle voice, so presence is asked of the engine itself (aur_has_conditioning, which also refreshes the
        voice's LRU stamp) instead of being mirrored in an ever-growing Python dict; an evicted voice is simply re-registered."""
        key = _content_key(g, s)
        has = getattr(self.native, "has_conditioning", None)
        if has is not None:
            if not has(key):
                self.native.set_conditioning(key, g, s)
        elif key not in self._speakers:   # engines without the query (test doubles)
            self.native.set_conditioning(key, g, s)
            self._speakers[key] = True
        return key

    # ------------------------------------------------------------------ phase 1
    async def get_generation_context(self, request: TTSRequest, gpt_cond_latent=None, speaker_embeddings=None
                                     ) -> Tuple[List[ChunkHandle], List[str], Any, Any]:
        if gpt_cond_latent is None or speaker_embeddings is None:
            gpt_cond_latent, speaker_embeddings = await self.get_audio_conditioning(
                request.speaker_files, request.max_ref_length, request.gpt_cond_len, request.gpt_cond_chunk_len)
        g_np = np.asarray(gpt_cond_latent, dtype=np.float32)
        s_np = np.asarray(speaker_embeddings, dtype=np.float32)
        # (several engines: a voice is registered on an engine when a chunk is placed there, _place)
        key = self._register_speaker(g_np, s_np) if self._placer is None else _content_key(g_np, s_np)
        chunks = self.tokenizer.batch_encode_with_split(request.text, request.language)
        loop = asyncio.get_running_loop()
        handles, ids = [], []
        for idx, text_ids in enumerate(chunks):
            if request.seed is None:
                self._seed_counter += 1
                # stable across processes (Python's hash() of a str is salted per process)
                seed = (int.from_bytes(hashlib.blake2b(str(request.request_id).encode(), digest_size=4).digest(), "little")
                        ^ self._seed_counter) & 0xFFFFFFFF
            else:
                seed = (request.seed + idx) & 0xFFFFFFFF
            seq = dict(text_ids=text_ids, speaker_key=key, temperature=request.temperature,
                       top_p=request.top_p, top_k=request.top_k,
                       repetition_penalty=request.repetition_penalty,
                       max_tokens=self.gpt_max_audio_tokens, seed=seed,
                       **({"ignore_stop": True} if self.fixed_length else {}),
                       # a latency-critical request: its first chunk is the one somebody waits for
                       **({"priority": int(request.priority)} if idx == 0 and getattr(request, "priority", 0) > 0 else {}),
                       # the speaking rate belongs to the whole request: every chunk carries it
                       **({"speed": float(request.speed)} if getattr(request, "speed", 1.0) != 1.0 else {}),
                       # so does the output rate; 24000 leaves the keyword out (engines and test doubles without it keep working)
                       **({"sample_rate": int(request.output_sample_rate)}
                          if getattr(request, "output_sample_rate", 24000) != 24000 else {}),
                       # and the encoding of the delivered audio (aur_seq_desc.encoding); unset leaves the keyword out too
                       **({"encoding": str(request.output_encoding)} if getattr(request, "output_encoding", None) else {}))
            if self._placer is None:
                fut = self.driver.submit(loop, reregister=lambda: self.native.set_conditioning(key, g_np, s_np), **seq)
            else:
                fut = self._submit_placed(loop, seq, key, g_np, s_np)
            rid = f"{request.request_id}_{idx}"
            handles.append(ChunkHandle(fut, rid, len(text_ids)))
            ids.append(rid)
        return handles, ids, speaker_embeddings, gpt_cond_latent

    # ------------------------------------------------------------------ several engines: placement
    def _submit_placed(self, loop, seq: dict, key: int, g_np: np.ndarray, s_np: np.ndarray) -> "asyncio.Future":
        """Event loop: the chunk's future exists from now on, the chunk itself goes to the placer -- onto an engine at once if one has
        room, into the placer's queue otherwise."""
        chunk = _Chunk(loop.create_future(), loop, seq, key, g_np, s_np)
        # a consumer that walks away cancels the future: the chunk leaves the placer's queue, or its engine is told (aur_cancel)
        chunk.future.add_done_callback(lambda f, c=chunk: self._chunk_done(f, c))
        with self._placer_lock:
            self._placer.submit(chunk, int(seq.get("priority", 0)))
            self._fail_orphans()
        return chunk.future

    def _register_on(self, e: int, chunk: _Chunk):
        """The has_conditioning / set_conditioning handshake of _register_speaker, on engine e."""
        native = self.natives[e]
        has = getattr(native, "has_conditioning", None)
        if has is not None:
            if not has(chunk.key):
                native.set_conditioning(chunk.key, chunk.g, chunk.s)
        elif chunk.key not in self._speakers_on[e]:
            native.set_conditioning(chunk.key, chunk.g, chunk.s)
            self._speakers_on[e][chunk.key] = True

    def _place(self, e: int, chunk: _Chunk):
        """ChunkPlacer's callback (placer lock held; event loop or a driver thread).  Never waits for an event loop.  It can wait for
        an ENGINE, though: the first placement of a voice on engine e (or its re-registration after an eviction) is
        aur_set_conditioning, which waits for e's running step, and the placer lock is held meanwhile -- the other drivers' hooks and
        the event loop's submissions queue up behind it for that long.  No deadlock (a step never takes the placer lock); the cost
        is unmeasured."""
        drv = self.drivers[e]
        if drv._error is not None or drv._stop:
            raise EngineUnavailable(f"engine {e}: driver stopped")
        native = self.natives[e]
        try:
            self._register_on(e, chunk)
            chunk.sid = drv.submit_for(chunk.future, chunk.loop, on_resolved=lambda: self._resolved(e),
                                       reregister=lambda: native.set_conditioning(chunk.key, chunk.g, chunk.s), **chunk.seq)
            chunk.engine = e
            return True
        except Exception as exc:   # noqa: BLE001 - this chunk's own failure (a bad id, a full voice table): its future gets it
            if drv._error is not None:
                raise EngineUnavailable(f"engine {e}: driver stopped") from exc
            chunk.loop.call_soon_threadsafe(lambda f=chunk.future, x=exc: (not f.done()) and f.set_exception(x))
            return False

    def _resolved(self, e: int):
        """Driver thread of engine e: one of its sequences has resolved; the placer tops the engine up (or, when the driver has
        stopped, takes the engine out and routes what is queued to the others)."""
        with self._placer_lock:
            gone = self._placer.engine_dead(e) if self.drivers[e]._error is not None and self._placer.alive[e] else []
            self._placer.resolved(e)
            self._fail_orphans(gone)

    def _fail_orphans(self, gone=()):
        """(placer lock held) chunks still queued when the last engine went: their futures fail, as a stopped driver's do."""
        for chunk in list(gone) + self._placer.orphans():
            exc = RuntimeError("engine driver stopped: no engine left to place the chunk on")
            chunk.loop.call_soon_threadsafe(lambda f=chunk.future, x=exc: (not f.done()) and f.set_exception(x))

    def _chunk_done(self, fut: "asyncio.Future", chunk: _Chunk):
        if not fut.cancelled():
            return
        with self._placer_lock:
            if self._placer.cancel(chunk):      # still queued: no engine ever sees it
                return
            e, sid = chunk.engine, chunk.sid
        if e >= 0 and sid is not None:
            self.drivers[e].cancel_seq(sid)

    # ------------------------------------------------------------------ phase 2
    async def process_tokens_to_speech(self, generator: ChunkHandle, speaker_embeddings=None, multimodal_data=None,
                                       request: Optional[TTSRequest] = None) -> AsyncGenerator[TTSOutput, None]:
        assert speaker_embeddings is not None, "Speaker embeddings must be provided for speech generation with XTTSv2."
        item = await generator.future
        # item["wav"] is the engine's own pinned result block (EngineDriver polls with copy=False): the TTSOutput's array is a view
        # of it and gives the block back when it is dropped (ResultLease); nothing is copied between the GPU's store and the caller
        yield TTSOutput(array=item["wav"], sample_rate=int(item.get("sample_rate", 24000)),
                        start_time=request.start_time if request is not None else None,
                        token_length=int(len(item["tokens"])),
                        # TTSRequest.output_encoding: the engine's stream of exactly this array, a view under the same lease
                        encoded=item.get("encoded"), encoded_format=item.get("encoded_format"))

    @property
    def native_flac(self) -> bool:
        """Every engine behind the plugin encodes FLAC on the GPU (aur_seq_desc.encoding, aur_encode_flac); test doubles may not."""
        return all(hasattr(n, "encode_flac") for n in self.natives)

    async def encode_flac(self, output: TTSOutput) -> bytes:
        """The 16-bit FLAC stream of a finished waveform, encoded on the GPU by the one-shot entry (aur_encode_flac) of the least-loaded
        engine, on a worker thread: the event loop never runs an encoder.  For audio the per-chunk encoding cannot cover (several chunks
        joined by combine_outputs, a waveform reworked on the host)."""
        native = self._least_loaded_native()
        one_shot = getattr(native, "encode_flac", None)
        if one_shot is None:
            raise RuntimeError("the engine has no encode_flac entry point (aur_encode_flac)")
        arr = np.asarray(output.array, dtype=np.float32).reshape(-1)
        return (await asyncio.to_thread(one_shot, [arr], [int(output.sample_rate)]))[0]

    async def shutdown(self):
        if self._placer is not None:
            with self._placer_lock:   # nothing is placed from here on; what still waits in the placer's queue fails now
                gone = []
                for e in range(len(self.natives)):
                    gone += self._placer.engine_dead(e)
                self._fail_orphans(gone)
        for drv in self.drivers:      # every driver first: no thread steps an engine while another one is closed
            drv.shutdown()
        if self._placer is not None:  # what was on an engine gets the same answer as what was still queued
            for drv in self.drivers:
                drv._fail_all(RuntimeError("engine shut down"))
        for native in self.natives:
            close = getattr(native, "close", None)
            if close:
                close()


register_model("xtts", XTTSv2Engine)
