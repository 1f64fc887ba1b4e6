"""ctypes binding of include/auralis_amd.h (the stub a reference maintainer would add).

There is deliberately no fallback: if the HIP library is missing or no MI355X is visible, loading /
engine creation raises.  Nothing here imports oracle/.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import threading
import weakref
from typing import Dict, List, Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AURALIS_AMD_LIB") or os.path.join(_HERE, "_C", "libauralis_amd.so")   # override: A/B builds


class AurError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"auralis_amd error {code}: {msg}")
        self.code = code


class aur_config(C.Structure):
    _fields_ = [("n_layer", C.c_int32), ("max_seqs", C.c_int32), ("max_prefill_rows", C.c_int32),
                ("max_speakers", C.c_int32), ("vocoder_min_batch", C.c_int32), ("profile", C.c_int32),
                ("vocoder_fp16", C.c_int32), ("second_pass", C.c_int32), ("return_latents", C.c_int32), ("kv_fp16", C.c_int32),
                ("gemm_f32_exact", C.c_int32), ("gelu_erf", C.c_int32), ("admit_min_batch", C.c_int32), ("urgent_rows", C.c_int32),
                ("gpt_fp16", C.c_int32)]


class aur_tensor_desc(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data", C.POINTER(C.c_float)), ("numel", C.c_int64)]


class aur_cond_params(C.Structure):
    _fields_ = [("max_ref_length", C.c_int32), ("gpt_cond_len", C.c_int32), ("gpt_cond_chunk_len", C.c_int32),
                ("sound_norm_refs", C.c_int32)]


class aur_seq_desc(C.Structure):
    _fields_ = [("text_ids", C.POINTER(C.c_int32)), ("n_text", C.c_int32), ("speaker_key", C.c_uint64),
                ("temperature", C.c_float), ("top_p", C.c_float), ("top_k", C.c_int32),
                ("repetition_penalty", C.c_float), ("max_tokens", C.c_int32), ("seed", C.c_uint32),
                ("ignore_stop", C.c_int32), ("encoding", C.c_int32), ("priority", C.c_int32), ("sample_rate", C.c_int32),
                ("speed", C.c_float)]


class aur_result(C.Structure):
    _fields_ = [("seq_id", C.c_uint64), ("n_tokens", C.c_int32), ("tokens", C.POINTER(C.c_int32)),
                ("n_samples", C.c_int32), ("wav", C.POINTER(C.c_float)), ("n_latent_rows", C.c_int32),
                ("latents", C.POINTER(C.c_float)), ("error", C.c_int32), ("enc", C.POINTER(C.c_uint8)),
                ("n_enc", C.c_int64), ("sample_rate", C.c_int32)]


class aur_stats(C.Structure):
    _fields_ = [("steps", C.c_int64), ("prefill_rows", C.c_int64), ("decode_rows", C.c_int64),
                ("tokens_generated", C.c_int64), ("samples_generated", C.c_int64), ("vocoder_batches", C.c_int64),
                ("conv_launches", C.c_int64), ("conv_ms", C.c_double), ("conv_flops", C.c_double),
                ("conv_bytes", C.c_double), ("gemm_launches", C.c_int64), ("gemm_ms", C.c_double), ("gemm_ms_raw", C.c_double),
                ("event_pair_overhead_ms", C.c_double), ("gemm_flops", C.c_double),
                ("gemm_bytes", C.c_double), ("vocoder_ms", C.c_double), ("gpt_ms", C.c_double),
                ("kv_blocks_total", C.c_int64), ("kv_blocks_free", C.c_int64),
                ("gemm_kind_launches", C.c_int64 * 5), ("gemm_kind_ms", C.c_double * 5), ("gemm_kind_bytes", C.c_double * 5),
                ("gemm_kind_flops", C.c_double * 5), ("attn_launches", C.c_int64), ("attn_ms", C.c_double),
                ("attn_bytes", C.c_double), ("decode_steps", C.c_int64), ("decode_ms", C.c_double), ("prefill_ms", C.c_double),
                ("decode_weight_bytes", C.c_double), ("decode_kv_bytes", C.c_double),
                ("conv_class_launches", C.c_int64 * 5), ("conv_class_ms", C.c_double * 5), ("conv_class_bytes", C.c_double * 5),
                ("conv_class_flops", C.c_double * 5), ("prefill_batches", C.c_int64),
                ("result_blocks", C.c_int64), ("result_blocks_free", C.c_int64), ("result_block_bytes", C.c_int64),
                ("speakers", C.c_int64), ("sequences_tracked", C.c_int64)]

    def as_dict(self) -> Dict[str, float]:
        out = {}
        for n, _ in self._fields_:
            v = getattr(self, n)
            out[n] = list(v) if hasattr(v, "__len__") else v
        return out


class aur_load(C.Structure):
    _fields_ = [("waiting", C.c_int32), ("running", C.c_int32), ("vocoding", C.c_int32), ("free_slots", C.c_int32),
                ("token_budget", C.c_int64)]


# every symbol include/auralis_amd.h declares (checked by tests/test_abi.py)
EXPORTS = [
    "aur_last_error", "aur_version", "aur_engine_create", "aur_engine_destroy", "aur_load_weights",
    "aur_set_conditioning", "aur_set_conditioning_device", "aur_has_conditioning", "aur_compute_conditioning", "aur_comm_unique_id", "aur_comm_init", "aur_broadcast_conditioning",
    "aur_comm_info", "aur_conditioning_checksum",
    "aur_submit", "aur_step", "aur_poll_finished",
    "aur_release", "aur_cancel", "aur_vocode", "aur_vocode_speed", "aur_vocode_rate", "aur_sync", "aur_get_stats", "aur_get_load", "aur_reset_stats", "aur_set_profile", "aur_dbg_gemm", "aur_dbg_gemm_rows", "aur_dbg_gemm_rows_ksplit_stress", "aur_dbg_lane_xor_selftest",
    "aur_dbg_paged_attention", "aur_dbg_prompt_attention", "aur_dbg_layernorm", "aur_dbg_conv1d", "aur_dbg_conv1d_f16", "aur_dbg_prefill", "aur_dbg_sample",
    "aur_dbg_conv1d_args", "aur_dbg_resblock_round_f16", "aur_dbg_interp2", "aur_dbg_interp3", "aur_dbg_conv_post", "aur_dbg_resample_out",
    "aur_dbg_gemm_tile", "aur_dbg_qkv_rows", "aur_dbg_rows_ln",
    "aur_flac_bound", "aur_encode_flac", "aur_dbg_flac_encode",
]

_lib = None


def load_library(path: Optional[str] = None) -> C.CDLL:
    """dlopen the in-tree HIP library; raises if it was not built (no silent fallback)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    # torch first: it bundles its own libamdhip64; loading ours after it makes both share ONE HIP runtime
    # (loading the system runtime first and torch's second leaves the process with no visible device).
    import torch  # noqa: F401
    p = path or LIB_PATH
    if not os.path.isfile(p):
        raise FileNotFoundError(
            f"{p} not found: build it with `python -m auralis_amd.build` (hipcc --offload-arch=gfx950). "
            "The MI355X path has no CPU fallback.")
    lib = C.CDLL(p)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    eng = C.c_void_p
    lib.aur_last_error.restype = C.c_char_p
    lib.aur_last_error.argtypes = []
    lib.aur_version.restype = C.c_int
    sig = {
        "aur_engine_create": [C.POINTER(aur_config), C.c_int, C.POINTER(eng)],
        "aur_engine_destroy": [eng],
        "aur_load_weights": [eng, C.POINTER(aur_tensor_desc), C.c_size_t],
        "aur_set_conditioning": [eng, C.c_uint64, fp, fp],
        "aur_set_conditioning_device": [eng, C.c_uint64, C.c_void_p, C.c_void_p],
        "aur_has_conditioning": [eng, C.c_uint64, ip],
        "aur_comm_unique_id": [C.POINTER(C.c_uint8)],
        "aur_comm_init": [eng, C.POINTER(C.c_uint8), C.c_int32, C.c_int32],
        "aur_broadcast_conditioning": [eng, C.c_uint64, C.c_int32],
        "aur_comm_info": [eng, ip, ip],
        "aur_conditioning_checksum": [eng, C.c_uint64, C.POINTER(C.c_uint64)],
        "aur_compute_conditioning": [eng, C.POINTER(fp), ip, C.c_int32, C.POINTER(aur_cond_params), fp, fp],
        "aur_submit": [eng, C.POINTER(aur_seq_desc), C.POINTER(C.c_uint64)],
        "aur_step": [eng, ip, ip],
        "aur_poll_finished": [eng, C.POINTER(aur_result), C.c_size_t, C.POINTER(C.c_size_t)],
        "aur_release": [eng, C.c_uint64],
        "aur_cancel": [eng, C.c_uint64],
        "aur_vocode": [eng, fp, ip, C.c_int32, C.c_int32, C.c_uint64, fp, C.c_int64, ip],
        "aur_vocode_speed": [eng, fp, ip, fp, C.c_int32, C.c_int32, C.c_uint64, fp, C.c_int64, ip],
        "aur_vocode_rate": [eng, fp, ip, fp, ip, C.c_int32, C.c_int32, C.c_uint64, fp, C.c_int64, ip],
        "aur_sync": [eng],
        "aur_get_stats": [eng, C.POINTER(aur_stats)],
        "aur_get_load": [eng, C.POINTER(aur_load)],
        "aur_reset_stats": [eng],
        "aur_set_profile": [eng, C.c_int32],
        "aur_dbg_gemm": [eng, fp, fp, fp, C.c_int32, C.c_int32, C.c_int32],
        "aur_dbg_gemm_tile": [eng, fp, C.c_int32, fp, fp, fp] + [C.c_int32] * 7,
        "aur_dbg_qkv_rows": [eng, fp, fp, fp, ip, ip] + [C.c_int32] * 5 + [fp, fp, fp, C.POINTER(C.c_int64)],
        "aur_dbg_rows_ln": [eng, fp, C.c_int32, fp, fp, fp, fp, fp, C.c_int32],
        "aur_dbg_gemm_rows": [eng, fp, fp, fp, fp, fp, fp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32],
        "aur_dbg_gemm_rows_ksplit_stress": [eng, C.c_int32, C.c_int32, C.POINTER(C.c_int64)],
        "aur_dbg_lane_xor_selftest": [eng, C.c_int32, C.POINTER(C.c_int64)],
        "aur_dbg_paged_attention": [eng, fp, fp, fp, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32, C.c_int32, fp],
        "aur_dbg_prompt_attention": [eng, fp, fp, fp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                     C.c_int32, fp],
        "aur_dbg_layernorm": [eng, fp, fp, fp, fp, C.c_int32],
        "aur_dbg_conv1d": [eng, fp, fp, fp, fp, fp, ip, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                           C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_int32],
        "aur_dbg_conv1d_f16": [eng, fp, C.c_void_p, fp, fp, fp, ip, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                               C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_int32],
        "aur_dbg_conv1d_args": [eng, C.c_int32, fp, C.c_void_p, fp, fp, ip, C.c_int32, C.c_int32, fp, fp, fp, ip] + [C.c_int32] * 8 +
                               [C.c_float, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float, C.POINTER(C.c_int64)],
        "aur_dbg_resblock_round_f16": [eng, fp, C.c_void_p, C.c_void_p, fp, fp, fp, fp, ip] + [C.c_int32] * 6 +
                                      [C.c_float, C.c_float, C.POINTER(C.c_int64)],
        "aur_dbg_interp2": [eng, fp, ip, ip] + [C.c_int32] * 6 + [fp, C.c_float, C.POINTER(C.c_int64)],
        "aur_dbg_interp3": [eng, fp, ip, ip, fp] + [C.c_int32] * 6 + [fp, C.c_float, C.POINTER(C.c_int64)],
        "aur_dbg_conv_post": [eng, fp, fp, ip, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, fp, C.c_float, C.POINTER(C.c_int64)],
        "aur_dbg_resample_out": [eng, fp, ip, ip, C.c_int32, C.c_int32, fp, C.c_int32, C.c_float, C.POINTER(C.c_int64)],
        "aur_encode_flac": [eng, C.POINTER(fp), ip, ip, C.c_int32, C.POINTER(C.c_uint8), C.c_int64, C.POINTER(C.c_int64)],
        "aur_dbg_flac_encode": [eng, fp, ip, ip, C.c_int32, C.c_int64, C.POINTER(C.c_uint8), C.c_int64, ip],
        "aur_dbg_prefill": [eng, ip, C.c_int32, C.c_uint64, C.c_float, fp, fp],
        "aur_dbg_sample": [eng, fp, C.c_int32, C.c_float, C.c_float, C.c_int32, C.c_float,
                           C.POINTER(C.c_uint8), C.c_uint32, C.c_int32, ip],
    }
    for name, argtypes in sig.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = C.c_int
    lib.aur_flac_bound.argtypes = [C.c_int64]
    lib.aur_flac_bound.restype = C.c_int64
    if path is None:
        _lib = lib
    return lib


def stretched_rows(n_lat: int, speed: float) -> int:
    """Latent rows after the speed stretch (aur_seq_desc.speed; 0 = unset = 1): L0' = max(1, floor(n_lat * ls)), ls = 1 / speed in
    double on the float32 value that crosses the ABI -- the rule of csrc/vocoder_kernels.h, for sizing output buffers."""
    sp = float(np.float32(speed))
    return max(1, int(np.floor(float(n_lat) * (1.0 if sp == 0.0 else 1.0 / sp))))


def samples_for(n_lat: int, speed: float = 0.0) -> int:
    """Samples the vocoder makes of n_lat latent rows at `speed`: 256 * floor(4 L0' * 24000 / 22050)."""
    return 256 * int(np.floor(float(4 * stretched_rows(n_lat, speed)) * (24000.0 / 22050.0)))


# output sample rates the engine delivers (aur_seq_desc.sample_rate; 0 = unset = 24000)
OUTPUT_SAMPLE_RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000)
ENCODINGS = {None: 0, "": 0, "flac": 1}   # aur_seq_desc.encoding (AUR_ENC_FLAC16 = 1)
FLAC_MAX_SAMPLES = 1 << 24                # per stream of aur_encode_flac
RESAMPLE_TILE = 1024   # output samples one workgroup of resample_out_kernel owns (kResampleTile, csrc/vocoder_kernels.h)


def samples_out(n: int, rate: int = 0) -> int:
    """Samples that n samples at 24 kHz become at `rate` (0 = unset = 24000): ceil(n new / orig), 24000:rate reduced by their gcd --
    the rule of csrc/vocoder_kernels.h, for sizing output buffers."""
    rate = int(rate) or 24000
    if rate not in OUTPUT_SAMPLE_RATES:
        raise ValueError(f"sample rate {rate} is not one of {OUTPUT_SAMPLE_RATES}")
    g = math.gcd(24000, rate)
    return -(-int(n) * (rate // g) // (24000 // g))


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


def _i32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.int32)


def _fp(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def _ip(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))


class ResultLease:
    """One finished sequence's hold on its pinned result block (aur_result.wav / .latents stay valid until aur_release).
    `release()` is idempotent; dropping the last reference releases too, so an array built on the lease (poll(copy=False))
    returns the block when the array -- and every view of it -- is gone.  The reference hands out plain numpy copies
    (XTTSv2.py:804-811); the lease is what lets this path hand out the engine's own buffer instead."""
    __slots__ = ("_eng", "seq_id", "nbytes", "__weakref__")

    def __init__(self, eng: "NativeEngine", seq_id: int, nbytes: int):
        self._eng, self.seq_id, self.nbytes = eng, seq_id, nbytes

    def release(self):
        eng, self._eng = self._eng, None
        if eng is not None:
            eng._lease_dropped(self)

    def __del__(self):
        try:
            self.release()
        except Exception:   # interpreter shutdown
            pass


class _PinnedView:
    """__array_interface__ over `n` elements at `addr`; numpy keeps this object (and through it the lease) as the array's base."""
    __slots__ = ("__array_interface__", "lease")

    def __init__(self, addr: int, shape, typestr: str, lease: ResultLease):
        self.__array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (addr, False), "version": 3}
        self.lease = lease


class NativeEngine:
    """Thin object wrapper over the C ABI; one instance per GPU."""
    # poll(copy=False) hands out views of pinned host memory; past this many leased bytes (waveforms somebody keeps) new
    # results are copied instead, so that kept outputs cost pageable memory like the reference's, not pinned blocks
    # (a result at an output rate of 48000 holds twice the pinned bytes of the same utterance at 24000, one at 8000 a third: the
    # budget counts bytes, so fewer of the former stay leased)
    LEASE_BUDGET_BYTES = 2 << 30

    def __init__(self, n_layer: int = 30, max_seqs: int = 64, device: int = 0, max_prefill_rows: int = 0,
                 max_speakers: int = 0, vocoder_min_batch: int = 0, profile: bool = False, vocoder_fp16: bool = False,
                 second_pass: bool = False, return_latents: bool = True, kv_fp16: bool = False,
                 gemm_f32_exact: bool = False, gelu_erf: bool = False, admit_min_batch: int = 0, urgent_rows: int = 0,
                 gpt_fp16: bool = False):
        self.lib = load_library()
        cfg = aur_config(n_layer, max_seqs, max_prefill_rows, max_speakers, vocoder_min_batch, int(profile),
                         int(vocoder_fp16), int(second_pass), int(return_latents), int(kv_fp16), int(gemm_f32_exact), int(gelu_erf), int(admit_min_batch), int(urgent_rows),
                         int(gpt_fp16))
        h = C.c_void_p()
        self._check(self.lib.aur_engine_create(C.byref(cfg), device, C.byref(h)))
        self.h = h
        self.max_seqs = max_seqs
        self.n_layer = n_layer
        self.device = device
        self._lease_lock = threading.Lock()
        self._leases: Dict[int, "weakref.ref"] = {}   # seq_id -> lease handed out by poll(copy=False)
        self._leased_bytes = 0
        self._closing = False

    def _check(self, rc: int):
        if rc != 0:
            raise AurError(rc, self.lib.aur_last_error().decode("utf-8", "replace"))

    def close(self):
        """Destroy the engine.  While arrays handed out by poll(copy=False) are alive their memory belongs to the engine, so the
        destruction waits for the last of them (it then happens on the thread that drops it)."""
        if not getattr(self, "h", None):
            return
        with self._lease_lock:
            self._closing = True
            if self._leases:
                return
            h, self.h = self.h, None
        self.lib.aur_engine_destroy(h)

    def _lease_dropped(self, lease: "ResultLease"):
        with self._lease_lock:
            if self._leases.pop(lease.seq_id, None) is None:
                return
            self._leased_bytes -= lease.nbytes
            h = self.h
            last = self._closing and not self._leases
            if last:
                self.h = None
        if h:
            self.lib.aur_release(h, lease.seq_id)
            if last:
                self.lib.aur_engine_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- weights / conditioning ------------------------------------------------------------------------
    def load_weights(self, packed: Dict[str, np.ndarray]):
        names = list(packed.keys())
        arrs = [_f32(packed[n]) for n in names]
        descs = (aur_tensor_desc * len(names))()
        keep = []
        for i, (n, a) in enumerate(zip(names, arrs)):
            b = n.encode()
            keep.append(b)
            descs[i].name = b
            descs[i].data = _fp(a)
            descs[i].numel = a.size
        self._check(self.lib.aur_load_weights(self.h, descs, len(names)))

    def set_conditioning(self, key: int, gpt_cond_latent, speaker_embedding):
        g = _f32(np.asarray(gpt_cond_latent).reshape(32, 1024))
        s = _f32(np.asarray(speaker_embedding).reshape(512))
        self._check(self.lib.aur_set_conditioning(self.h, key, _fp(g), _fp(s)))

    def has_conditioning(self, key: int) -> bool:
        out = C.c_int32()
        self._check(self.lib.aur_has_conditioning(self.h, key, C.byref(out)))
        return bool(out.value)

    def compute_conditioning(self, references, max_ref_length: int = 30, gpt_cond_len: int = 6, gpt_cond_chunk_len: int = 6,
                             sound_norm_refs: bool = False):
        """Reference audio (list of mono float32 arrays at 22 050 Hz) -> (gpt_cond_latent [1,32,1024], speaker_embedding
        [1,512,1]) computed by the HIP kernels (needs weights.pack_conditioning in load_weights)."""
        arrs = [_f32(np.asarray(r).reshape(-1)) for r in references]
        ptrs = (C.POINTER(C.c_float) * len(arrs))(*[_fp(a) for a in arrs])
        ns = _i32([a.size for a in arrs])
        p = aur_cond_params(int(max_ref_length), int(gpt_cond_len), int(gpt_cond_chunk_len), int(bool(sound_norm_refs)))
        g = np.empty((1, 32, 1024), np.float32)
        s = np.empty((1, 512, 1), np.float32)
        self._check(self.lib.aur_compute_conditioning(self.h, ptrs, _ip(ns), len(arrs), C.byref(p), _fp(g), _fp(s)))
        return g, s

    # -- RCCL inside the library (one engine per GPU per process) -------------------------------------
    @staticmethod
    def comm_unique_id() -> bytes:
        buf = (C.c_uint8 * 128)()
        rc = load_library().aur_comm_unique_id(buf)
        if rc != 0:
            raise AurError(rc, load_library().aur_last_error().decode("utf-8", "replace"))
        return bytes(buf)

    def comm_init(self, unique_id: bytes, rank: int, world: int):
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        self._check(self.lib.aur_comm_init(self.h, buf, rank, world))

    def broadcast_conditioning(self, key: int, root: int = 0):
        """Collective over the engine's communicator: the voice `key` registered on `root` arrives on every other rank."""
        self._check(self.lib.aur_broadcast_conditioning(self.h, key, root))

    def comm_info(self):
        """(ranks, rank) as the engine's RCCL communicator reports them (ncclCommCount / ncclCommUserRank); (0, -1) before comm_init."""
        n, r = C.c_int32(0), C.c_int32(-1)
        self._check(self.lib.aur_comm_info(self.h, C.byref(n), C.byref(r)))
        return int(n.value), int(r.value)

    def conditioning_checksum(self, key: int) -> int:
        """FNV-1a over the voice's conditioning as it sits in device memory (cross-rank equality check after a broadcast)."""
        out = C.c_uint64(0)
        self._check(self.lib.aur_conditioning_checksum(self.h, key, C.byref(out)))
        return int(out.value)

    def set_conditioning_device(self, key: int, d_gpt_cond_ptr: int, d_spk_ptr: int):
        self._check(self.lib.aur_set_conditioning_device(self.h, key, C.c_void_p(d_gpt_cond_ptr), C.c_void_p(d_spk_ptr)))

    # -- sequences -------------------------------------------------------------------------------------
    def submit(self, text_ids: Sequence[int], speaker_key: int, temperature: float = 0.75, top_p: float = 0.85,
               top_k: int = 50, repetition_penalty: float = 5.0, max_tokens: int = 605, seed: int = 0,
               ignore_stop: bool = False, priority: int = 0, speed: float = 0.0, sample_rate: int = 0, encoding=None) -> int:
        """`speed`: aur_seq_desc.speed, 0 = unset (= 1.0), else in [0.5, 2.0]; `sample_rate`: aur_seq_desc.sample_rate, 0 = unset
        (= 24000), else one of OUTPUT_SAMPLE_RATES (anything else: AurError, AUR_E_INVALID); `encoding`: aur_seq_desc.encoding, None / 0
        or "flac" / AUR_ENC_FLAC16 (the result then carries `encoded`, the 16-bit FLAC stream of `wav`)."""
        enc = ENCODINGS[encoding] if encoding in ENCODINGS else int(encoding)
        ids = _i32(list(text_ids))
        d = aur_seq_desc(_ip(ids), len(ids), speaker_key, temperature, top_p, top_k, repetition_penalty,
                         max_tokens, seed & 0xFFFFFFFF, int(ignore_stop), enc, int(priority), int(sample_rate), float(speed))
        sid = C.c_uint64()
        self._check(self.lib.aur_submit(self.h, C.byref(d), C.byref(sid)))
        return sid.value

    def step(self):
        live, fin = C.c_int32(), C.c_int32()
        self._check(self.lib.aur_step(self.h, C.byref(live), C.byref(fin)))
        return live.value, fin.value

    def poll(self, cap: int = 64, want_latents: bool = True, copy: bool = True) -> List[dict]:
        """Finished sequences.  copy=True: owned numpy arrays, the engine's result block is released at once.  copy=False: `wav`
        (and `latents`) are VIEWS of the engine's pinned result block (aur_result.wav / .latents); the item's `lease`
        (ResultLease) gives the block back -- explicitly (lease.release() / release(seq_id)) or when the last array over it is
        dropped.  Token ids are always copied (a few hundred int32)."""
        res = (aur_result * cap)()
        n = C.c_size_t()
        self._check(self.lib.aur_poll_finished(self.h, res, cap, C.byref(n)))
        out = []
        for i in range(n.value):
            r = res[i]
            nbytes = 4 * (r.n_samples + (r.n_latent_rows * 1024 if want_latents else 0)) + int(r.n_enc)   # the lease budget counts the stream too
            lease = None
            if not copy and nbytes:
                with self._lease_lock:
                    if self._leased_bytes + nbytes <= self.LEASE_BUDGET_BYTES:
                        lease = ResultLease(self, r.seq_id, nbytes)
                        self._leases[r.seq_id] = weakref.ref(lease)
                        self._leased_bytes += nbytes

            def arr(ptr, shape):
                if lease is None:
                    return np.ctypeslib.as_array(ptr, shape=shape).copy()
                return np.asarray(_PinnedView(C.addressof(ptr.contents), shape, "<f4" if ptr._type_ is C.c_float else "|u1", lease))
            item = {
                "seq_id": r.seq_id,
                "tokens": (np.ctypeslib.as_array(r.tokens, shape=(r.n_tokens,)).copy() if r.n_tokens
                           else np.zeros(0, dtype=np.int32)),
                "wav": (arr(r.wav, (r.n_samples,)) if r.n_samples
                        else np.zeros(0, dtype=np.float32)),   # failed sequences carry no audio (error != 0)
                "error": r.error,
                "sample_rate": r.sample_rate,
            }
            if want_latents and r.n_latent_rows:
                item["latents"] = arr(r.latents, (r.n_latent_rows, 1024))
            if r.n_enc:   # aur_seq_desc.encoding: uint8 array (a view under the same lease when copy=False)
                item["encoded"] = arr(r.enc, (int(r.n_enc),))
                item["encoded_format"] = "flac"
            if lease is None:
                self._check(self.lib.aur_release(self.h, r.seq_id))
            else:
                item["lease"] = lease
            out.append(item)
        return out

    def encode_flac(self, arrays, rates) -> List[bytes]:
        """aur_encode_flac: finished float waveforms (one mono array each) with a sample rate per row -> 16-bit FLAC streams encoded on
        the GPU, byte for byte flac.encode(codecs._to_int(x, 2), rate, 16).  1 <= samples <= 2^24 per row, rate < 2^20."""
        arrs = [_f32(np.asarray(a).reshape(-1)) for a in arrays]
        B = len(arrs)
        if isinstance(rates, (int, np.integer)):
            rates = [int(rates)] * B
        if B == 0 or len(rates) != B:
            raise ValueError("encode_flac: one sample rate per array, at least one array")
        ptrs = (C.POINTER(C.c_float) * B)(*[_fp(a) for a in arrs])
        ns = _i32([a.size for a in arrs])
        sr = _i32([int(r) for r in rates])
        stride = int(self.lib.aur_flac_bound(max(1, min(int(ns.max()), FLAC_MAX_SAMPLES))))
        out = np.empty((B, stride), np.uint8)
        lens = np.zeros(B, np.int64)
        self._check(self.lib.aur_encode_flac(self.h, ptrs, _ip(ns), _ip(sr), B, out.ctypes.data_as(C.POINTER(C.c_uint8)), stride,
                                             lens.ctypes.data_as(C.POINTER(C.c_int64))))
        return [out[b, :int(lens[b])].tobytes() for b in range(B)]

    def release(self, seq_id: int):
        """Give a sequence's result block back now (after poll(copy=False)); the arrays over it must not be used afterwards.
        A sequence whose lease is already gone is not an error."""
        with self._lease_lock:
            ref = self._leases.get(seq_id)
        lease = ref() if ref is not None else None
        if lease is not None:
            lease.release()
        elif ref is not None:     # the lease object is being finalised: its __del__ releases
            return

    def cancel(self, seq_id: int):
        """aur_cancel: stop a sequence nobody waits for any more.  It is still reported by poll() (error = AUR_E_CANCELLED = -5, the
        tokens generated so far, no audio).  Does not wait for a running step."""
        self._check(self.lib.aur_cancel(self.h, seq_id))

    def run_until_done(self, max_steps: int = 100000, copy: bool = True) -> List[dict]:
        """Drive aur_step until nothing is live; returns finished results in completion order (copy: see poll)."""
        done: List[dict] = []
        last_fin = -1
        for _ in range(max_steps):
            live, fin = self.step()
            if fin != last_fin or live == 0:   # aur_step's second output counts finished sequences: poll only when it moved
                while True:                    # a vocoder batch (or a failed step) can finish more than one poll's worth at once
                    got = self.poll(cap=64, copy=copy)
                    done.extend(got)
                    if len(got) < 64:
                        break
                last_fin = fin
            if live == 0:
                break
        else:
            raise RuntimeError("run_until_done: step limit reached")
        return done

    def vocode(self, latents: np.ndarray, n_lat: Optional[Sequence[int]], speaker_key: int,
               speed: Optional[Sequence[float]] = None, sample_rate: Optional[Sequence[int]] = None) -> List[np.ndarray]:
        """`speed` (optional, one per utterance, as aur_seq_desc.speed): aur_vocode_speed; None: aur_vocode.  `sample_rate` (optional,
        one per utterance, as aur_seq_desc.sample_rate): aur_vocode_rate."""
        lat = _f32(latents)
        if lat.ndim == 2:
            lat = lat[None]
        B, t_max, _ = lat.shape
        nl = _i32(n_lat if n_lat is not None else [t_max] * B)
        stride = int(np.floor(np.floor(t_max * 4.0) * (24000 / 22050))) * 256
        ns = np.zeros(B, dtype=np.int32)
        if sample_rate is not None:
            sp = None if speed is None else _f32(np.asarray(speed).reshape(B))
            sr = _i32(np.asarray(sample_rate).reshape(B))
            try:   # (what the engine refuses gets any stride)
                stride = max([stride] + [samples_out(samples_for(int(n), 0.0 if sp is None else float(sp[b])), int(sr[b]))
                                         for b, n in enumerate(nl)])
            except (ValueError, OverflowError):
                pass
            wav = np.zeros((B, stride), dtype=np.float32)
            self._check(self.lib.aur_vocode_rate(self.h, _fp(lat), _ip(nl), _fp(sp), _ip(sr), B, t_max, speaker_key, _fp(wav), stride,
                                                 _ip(ns)))
            return [wav[b, : ns[b]].copy() for b in range(B)]
        if speed is None:
            wav = np.zeros((B, stride), dtype=np.float32)
            self._check(self.lib.aur_vocode(self.h, _fp(lat), _ip(nl), B, t_max, speaker_key, _fp(wav), stride, _ip(ns)))
            return [wav[b, : ns[b]].copy() for b in range(B)]
        sp = _f32(np.asarray(speed).reshape(B))
        if np.isfinite(sp).all() and ((sp == 0) | ((sp >= 0.5) & (sp <= 2.0))).all():   # (else the engine refuses; any stride will do)
            stride = max([stride] + [samples_for(int(n), float(v)) for n, v in zip(nl, sp)])
        wav = np.zeros((B, stride), dtype=np.float32)
        self._check(self.lib.aur_vocode_speed(self.h, _fp(lat), _ip(nl), _fp(sp), B, t_max, speaker_key, _fp(wav), stride, _ip(ns)))
        return [wav[b, : ns[b]].copy() for b in range(B)]

    def sync(self):
        self._check(self.lib.aur_sync(self.h))

    def stats(self) -> Dict[str, float]:
        s = aur_stats()
        self._check(self.lib.aur_get_stats(self.h, C.byref(s)))
        return s.as_dict()

    def load(self) -> Dict[str, int]:
        """aur_get_load: {waiting, running, vocoding, free_slots, token_budget}.  Host only (no HIP call, does not wait for a step):
        callable from any thread while the driver thread is inside step()."""
        l = aur_load()
        self._check(self.lib.aur_get_load(self.h, C.byref(l)))
        return {n: int(getattr(l, n)) for n, _ in l._fields_}

    def reset_stats(self):
        self._check(self.lib.aur_reset_stats(self.h))

    def set_profile(self, every: int):
        """Profile mode on (every > 0: conv launches event-timed, replay batches after every `every`-th decode step) / off (0)."""
        self._check(self.lib.aur_set_profile(self.h, int(every)))

    # -- per-kernel debug entry points -------------------------------------------------------------------
    def dbg_gemm(self, X, W) -> np.ndarray:
        """prefill-regime GEMM (gemm_tile_kernel): X @ W"""
        X, W = _f32(X), _f32(W)
        M, K = X.shape
        K2, N = W.shape
        assert K == K2
        out = np.empty((M, N), dtype=np.float32)
        self._check(self.lib.aur_dbg_gemm(self.h, _fp(X), _fp(W), _fp(out), M, N, K))
        return out

    def dbg_gemm_tile(self, X, W, bias=None, slabs: int = 1, epi: int = 0, erf: bool = False, exact: bool = False, K=None) -> np.ndarray:
        """launch_gemm_tile on X [M][ldx] (K: the leading columns that count, default all) and W [K][N].  epi 0: the raw slabs
        [slabs][M][N]; epi 1: gelu(X @ W + bias) [M][N], erf or tanh form.  exact: the exact-f32 kernel whatever the engine's mode."""
        X, W = _f32(X), _f32(W)
        M, ldx = X.shape
        K2, N = W.shape
        K = ldx if K is None else int(K)
        assert K == K2 and ldx >= K
        bias = None if bias is None else _f32(bias)
        out = np.empty((M, N) if epi else (slabs, M, N), dtype=np.float32)
        self._check(self.lib.aur_dbg_gemm_tile(self.h, _fp(X), ldx, _fp(W), _fp(bias), _fp(out), M, N, K, int(slabs), int(epi),
                                               int(bool(erf)), int(bool(exact))))
        return out

    def dbg_qkv_rows(self, X, W, bias, row_seq, row_pos, k, v, fused: bool, kv_half: bool = False):
        """The prompt-row QKV GEMM + epilogue on a paged pool built from k / v [n_seq][ctx_max][1024] -> (q [M][1024], the pool read
        back as k, v, stray pool words)."""
        X, W, bias, row_seq, row_pos = _f32(X), _f32(W), _f32(bias), _i32(row_seq), _i32(row_pos)
        k, v = _f32(k).copy(), _f32(v).copy()
        assert X.shape[1] == 1024 and W.shape == (1024, 3072) and k.shape == v.shape and k.shape[2] == 1024
        q = np.empty((X.shape[0], 1024), dtype=np.float32)
        stray = C.c_int64(-1)
        self._check(self.lib.aur_dbg_qkv_rows(self.h, _fp(X), _fp(W), _fp(bias), _ip(row_seq), _ip(row_pos), X.shape[0], k.shape[0], k.shape[1],
                                              int(bool(fused)), int(bool(kv_half)), _fp(q), _fp(k), _fp(v), C.byref(stray)))
        return q, k, v, int(stray.value)

    def dbg_rows_ln(self, P, bias, h, gamma, beta):
        """rows_ln_kernel with slabs P [S][M][1024] (None: S = 0) -> (h + sum_s P[s] + bias, LayerNorm of it)"""
        h, gamma, beta = _f32(h).copy(), _f32(gamma), _f32(beta)
        P = None if P is None else _f32(P)
        bias = None if bias is None else _f32(bias)
        S = 0 if P is None else P.shape[0]
        assert P is None or P.shape[1:] == h.shape
        out = np.empty_like(h)
        self._check(self.lib.aur_dbg_rows_ln(self.h, _fp(P), S, _fp(bias), _fp(h), _fp(gamma), _fp(beta), _fp(out), h.shape[0]))
        return h, out

    def dbg_gemm_rows(self, X, W, bias=None, gamma=None, beta=None, res=None, epi: int = 0) -> np.ndarray:
        """Decode-regime GEMM: epi 0 bias, 1 bias + gelu_new, 2 res + (X @ W + bias); gamma/beta => LayerNorm prologue."""
        X, W = _f32(X), _f32(W)
        M, K = X.shape
        K2, N = W.shape
        assert K == K2
        out = _f32(res).copy() if res is not None else np.zeros((M, N), dtype=np.float32)
        bias = None if bias is None else _f32(bias)
        ln = gamma is not None
        gamma = None if gamma is None else _f32(gamma)
        beta = None if beta is None else _f32(beta)
        self._check(self.lib.aur_dbg_gemm_rows(self.h, _fp(X), _fp(W), _fp(bias), _fp(gamma), _fp(beta), _fp(out), M, N, K,
                                               epi, int(ln)))
        return out

    def dbg_gemm_rows_ksplit_stress(self, M: int, iters: int) -> int:
        """`iters` back-to-back K-split projection launches at M rows vs the unsplit kernel, bitwise on the device: differing words."""
        bad = C.c_int64(-1)
        self._check(self.lib.aur_dbg_gemm_rows_ksplit_stress(self.h, int(M), int(iters), C.byref(bad)))
        return int(bad.value)

    def dbg_lane_xor_selftest(self, blocks: int = 64) -> int:
        """lane_xor<J> / wave_sum / wave_max (DPP + lane swaps) vs the shuffles they replace, on the GPU: results that differ bitwise."""
        bad = C.c_int64(-1)
        self._check(self.lib.aur_dbg_lane_xor_selftest(self.h, int(blocks), C.byref(bad)))
        return int(bad.value)

    def dbg_paged_attention(self, q, k, v, ctx, shared=0, kv_half=False) -> np.ndarray:
        """q [M][1024], k / v [M][ctx_max][1024], ctx [M] -> [M][1024]: the decode attention kernel on a paged pool built from k / v."""
        q, k, v, ctx = _f32(q), _f32(k), _f32(v), _i32(ctx)
        out = np.empty_like(q)
        self._check(self.lib.aur_dbg_paged_attention(self.h, _fp(q), _fp(k), _fp(v), ctx.ctypes.data_as(C.POINTER(C.c_int32)), q.shape[0],
                                                     k.shape[1], int(shared), int(bool(kv_half)), _fp(out)))
        return out

    def dbg_prompt_attention(self, q, k, v, row_seq, row_pos, shared=0, kv_half=False) -> np.ndarray:
        """q [M][1024], k / v [n_seq][ctx_max][1024], row_seq / row_pos [M] -> [M][1024]: the prefill attention kernel on a paged pool."""
        q, k, v, row_seq, row_pos = _f32(q), _f32(k), _f32(v), _i32(row_seq), _i32(row_pos)
        out = np.empty_like(q)
        ip = C.POINTER(C.c_int32)
        self._check(self.lib.aur_dbg_prompt_attention(self.h, _fp(q), _fp(k), _fp(v), row_seq.ctypes.data_as(ip), row_pos.ctypes.data_as(ip),
                                                      q.shape[0], k.shape[0], k.shape[1], int(shared), int(bool(kv_half)), _fp(out)))
        return out

    def dbg_layernorm(self, h, gamma, beta) -> np.ndarray:
        h, gamma, beta = _f32(h), _f32(gamma), _f32(beta)
        out = np.empty_like(h)
        self._check(self.lib.aur_dbg_layernorm(self.h, _fp(h), _fp(gamma), _fp(beta), _fp(out), h.shape[0]))
        return out

    def dbg_conv1d(self, x, wp, bias, res, lens, ks, dil, padl, slope, cout, ups_s=0, ups_p=0) -> np.ndarray:
        x, wp = _f32(x), _f32(wp)
        B, cin, L = x.shape
        mtot = wp.shape[0] * wp.shape[3]
        lout = L * max(1, ups_s)
        bias = None if bias is None else _f32(bias)
        res = None if res is None else _f32(res)
        out = np.empty((B, cout, lout), dtype=np.float32)
        lens = _i32(lens)
        self._check(self.lib.aur_dbg_conv1d(self.h, _fp(x), _fp(wp), _fp(bias), _fp(res), _fp(out), _ip(lens), B, cin,
                                            mtot, cout, L, ks, dil, padl, slope, ups_s, ups_p))
        return out

    def dbg_conv1d_f16(self, x, wp16, bias, res, lens, ks, dil, padl, slope, cout, mtot, ups_s=0, ups_p=0) -> np.ndarray:
        x = _f32(x)
        wp16 = np.ascontiguousarray(wp16, dtype=np.float16)
        B, cin, L = x.shape
        lout = L * max(1, ups_s)
        bias = None if bias is None else _f32(bias)
        res = None if res is None else _f32(res)
        out = np.empty((B, cout, lout), dtype=np.float32)
        lens = _i32(lens)
        self._check(self.lib.aur_dbg_conv1d_f16(self.h, _fp(x), wp16.ctypes.data_as(C.c_void_p), _fp(bias), _fp(res),
                                                _fp(out), _ip(lens), B, cin, mtot, cout, L, ks, dil, padl, slope, ups_s, ups_p))
        return out

    # The vocoder's kernels one at a time.  Tensors are plain [B][C][L] float32 arrays (L = max(lens)); outputs start as `sentinel`
    # unless the caller passes their initial content, and come back with the number of guard words the kernel changed (0 expected).
    def dbg_conv1d_args(self, variant, x, w, lens, ks, dil, padl, cout, slope=1.0, bias=None, cond=None, cond_row=None, res=None,
                        mrf=None, out=None, mrf_mode=0, out_slope=1.0, res_unact=1.0, ups_s=0, ups_p=0, sentinel=-777.0):
        """One ConvArgs launch: variant 0 fp32 kernel (w packed float32), 1 / 2 interleaved halves, register / LDS-DMA staged (w packed
        float16).  Returns (out, mrf, guard words changed); out is None in modes 1 / 2, mrf in mode 0."""
        x, lens = _f32(x), _i32(lens)
        w = np.ascontiguousarray(w, dtype=np.float32 if variant == 0 else np.float16)
        B, cin, L = x.shape
        mtot = w.size // (cin * ks)
        shape = (B, cout, L * max(1, ups_s))
        bias = None if bias is None else _f32(bias)
        res = None if res is None else _f32(res)
        cond = None if cond is None else _f32(cond)
        cond_row = None if cond_row is None else _i32(cond_row)
        cond_rows, cond_stride = cond.shape if cond is not None else (0, 0)
        if mrf_mode != 0:
            mrf = np.full(shape, sentinel, dtype=np.float32) if mrf is None else _f32(mrf).copy()
        if mrf_mode in (0, 3):
            out = np.full(shape, sentinel, dtype=np.float32) if out is None else _f32(out).copy()
        assert (res is None or res.shape == shape) and (mrf is None or mrf.shape == shape) and (out is None or out.shape == shape)
        bad = C.c_int64(-1)
        self._check(self.lib.aur_dbg_conv1d_args(self.h, variant, _fp(x), w.ctypes.data_as(C.c_void_p), _fp(bias), _fp(cond), _ip(cond_row),
                                                 cond_rows, cond_stride, _fp(res), _fp(mrf), _fp(out), _ip(lens), B, cin, mtot, cout, L, ks,
                                                 dil, padl, slope, ups_s, ups_p, mrf_mode, out_slope, res_unact, sentinel, C.byref(bad)))
        return out, mrf, int(bad.value)

    def dbg_resblock_round_f16(self, y, w1, w2, b1, b2, lens, ks, dil, mrf_mode=0, e_slope=0.1, mrf=None, out=None, sentinel=-777.0):
        """One fused ResBlock round on the activated stream y [B][C][L]; w1 / w2 packed float16.  Returns (out, mrf, guard words
        changed) as dbg_conv1d_args: out is None in modes 1 / 2, mrf in mode 0.  out=y hands the launcher one tensor for both (it
        refuses)."""
        alias = out is y
        y, lens, b1, b2 = _f32(y), _i32(lens), _f32(b1), _f32(b2)
        w1, w2 = np.ascontiguousarray(w1, dtype=np.float16), np.ascontiguousarray(w2, dtype=np.float16)
        B, ch, L = y.shape
        if mrf_mode != 0:
            mrf = np.full(y.shape, sentinel, dtype=np.float32) if mrf is None else _f32(mrf).copy()
        if alias:
            out = y
        elif mrf_mode in (0, 3):
            out = np.full(y.shape, sentinel, dtype=np.float32) if out is None else _f32(out).copy()
        bad = C.c_int64(-1)
        self._check(self.lib.aur_dbg_resblock_round_f16(self.h, _fp(y), w1.ctypes.data_as(C.c_void_p), w2.ctypes.data_as(C.c_void_p), _fp(b1),
                                                        _fp(b2), _fp(mrf), _fp(out), _ip(lens), B, ch, L, ks, dil, mrf_mode, e_slope, sentinel,
                                                        C.byref(bad)))
        return out, mrf, int(bad.value)

    def dbg_interp2(self, lat, lat_row, n_lat, frames, out_f16=False, sentinel=-777.0):
        """The two chained interpolations: lat [R][n_max][C], utterance b blends n_lat[b] rows of lat[lat_row[b]]; frames = the longest
        utterance's vocoder frames (the row stride of z).  Returns (z [B][C][frames], guard words changed)."""
        lat, n_lat = _f32(lat), _i32(n_lat)
        lat_row = None if lat_row is None else _i32(lat_row)
        R, n_max, ch = lat.shape
        z = np.full((len(n_lat), ch, frames), sentinel, dtype=np.float32)
        bad = C.c_int64(-1)
        self._check(self.lib.aur_dbg_interp2(self.h, _fp(lat), _ip(lat_row), _ip(n_lat), R, n_max, len(n_lat), ch, frames, int(bool(out_f16)),
                                             _fp(z), sentinel, C.byref(bad)))
        return z, int(bad.value)

    def dbg_interp3(self, lat, lat_row, n_lat, speed, frames, out_f16=False, sentinel=-777.0):
        """dbg_interp2 with the speed stretch in front: speed [B] as aur_seq_desc.speed; frames = the longest utterance's vocoder frames
        after its stretch.  Returns (z [B][C][frames], guard words changed)."""
        lat, n_lat, speed = _f32(lat), _i32(n_lat), _f32(speed)
        lat_row = None if lat_row is None else _i32(lat_row)
        R, n_max, ch = lat.shape
        assert speed.shape == n_lat.shape
        z = np.full((len(n_lat), ch, frames), sentinel, dtype=np.float32)
        bad = C.c_int64(-1)
        self._check(self.lib.aur_dbg_interp3(self.h, _fp(lat), _ip(lat_row), _ip(n_lat), _fp(speed), R, n_max, len(n_lat), ch, frames,
                                             int(bool(out_f16)), _fp(z), sentinel, C.byref(bad)))
        return z, int(bad.value)

    def dbg_conv_post(self, x, w, lens, slope=0.01, x_f16_act=False, sentinel=-777.0):
        """conv_post + tanh on x [B][Cin][L], w [Cin][7].  Returns (wav [B][L], guard words changed)."""
        x, w, lens = _f32(x), _f32(w), _i32(lens)
        B, cin, L = x.shape
        wav = np.full((B, L), sentinel, dtype=np.float32)
        bad = C.c_int64(-1)
        self._check(self.lib.aur_dbg_conv_post(self.h, _fp(x), _fp(w), _ip(lens), B, cin, L, slope, int(bool(x_f16_act)), _fp(wav), sentinel,
                                               C.byref(bad)))
        return wav, int(bad.value)

    def dbg_flac_encode(self, x, lens, rates, sentinel=0x5A):
        """The FLAC kernels alone on x [B][stride] (lens[b] samples count, rates[b] Hz) -> (out [B][out_stride] uint8 that started as
        `sentinel` bytes, out_lens [B]): stream b is out[b, :out_lens[b]], everything behind it must still be the sentinel."""
        x = _f32(x)
        B, stride = x.shape
        lens, rates = _i32(lens), _i32(rates)
        out_stride = int(self.lib.aur_flac_bound(int(lens.max())))
        out = np.full((B, out_stride), sentinel, dtype=np.uint8)
        out_lens = np.zeros(B, np.int32)
        self._check(self.lib.aur_dbg_flac_encode(self.h, _fp(x), _ip(lens), _ip(rates), B, stride, out.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                 out_stride, _ip(out_lens)))
        return out, out_lens

    def dbg_resample_out(self, x, lens, rate, sentinel=-777.0):
        """The output-rate resampler alone on x [B][L] (L = max(lens)), rate [B] as aur_seq_desc.sample_rate.  Returns
        (out [B][max samples_out(lens[b], rate[b])], guard words changed)."""
        x, lens, rate = _f32(x), _i32(lens), _i32(rate)
        B, L = x.shape
        assert lens.shape == rate.shape == (B,)
        lout = max(samples_out(int(n), int(r)) for n, r in zip(lens, rate))
        out = np.full((B, lout), sentinel, dtype=np.float32)
        bad = C.c_int64(-1)
        self._check(self.lib.aur_dbg_resample_out(self.h, _fp(x), _ip(lens), _ip(rate), B, L, _fp(out), lout, sentinel, C.byref(bad)))
        return out, int(bad.value)

    def dbg_prefill(self, text_ids, speaker_key: int, repetition_penalty: float = 1.0):
        ids = _i32(list(text_ids))
        n_rows = 32 + len(ids) + 1
        rows = np.empty((n_rows, 1024), dtype=np.float32)
        logits = np.empty(1026, dtype=np.float32)
        self._check(self.lib.aur_dbg_prefill(self.h, _ip(ids), len(ids), speaker_key, repetition_penalty, _fp(rows), _fp(logits)))
        return rows, logits

    def dbg_sample(self, logits, temperature, top_p, top_k, repetition_penalty=1.0, seen=None, seed=0, step=0):
        lg = _f32(logits)
        if lg.ndim == 1:
            lg = lg[None]
        B = lg.shape[0]
        toks = np.zeros(B, dtype=np.int32)
        sp = None
        if seen is not None:
            seen = np.ascontiguousarray(seen, dtype=np.uint8).reshape(B, 1026)
            sp = seen.ctypes.data_as(C.POINTER(C.c_uint8))
        self._check(self.lib.aur_dbg_sample(self.h, _fp(lg), B, temperature, top_p, top_k, repetition_penalty, sp,
                                            seed & 0xFFFFFFFF, step, _ip(toks)))
        return toks
