"""The input batch of the FLAC encoder tests (tests/test_flac_host.py proves its coverage on the CPU from the host writer's streams
alone, tests/test_gpu_flac.py runs it on the GPU) and a frame-by-frame reader of what the writer chose.

Reference everywhere: flac.encode(codecs._to_int(x, 2), rate, 16), byte for byte."""
import functools

import numpy as np

from auralis_amd.api import codecs, flac

BLOCK = 4096
RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000)


def _sine(n, w, amp=0.9, phase=0.3):
    return (amp * np.sin(w * np.arange(n, dtype=np.float64) + phase)).astype(np.float32)


def _noise(rng, n, amp):
    return (amp * rng.uniform(-1.0, 1.0, n)).astype(np.float32)


def _walk(rng, n, step=1e-3):
    return np.cumsum(step * rng.standard_normal(n)).astype(np.float32)


def _chirp(n, w0=1e-3, w1=0.4, amp=0.7):
    t = np.arange(n, dtype=np.float64)
    return (amp * np.sin(w0 * t + (w1 - w0) * t * t / (2.0 * max(n, 1)))).astype(np.float32)


def _steps(rng, n, parts):
    """noise whose amplitude changes from one n / parts stretch to the next (what makes a partition order pay)"""
    amp = np.repeat(10.0 ** -rng.permutation(np.linspace(1.0, 4.0, parts)), n // parts)
    return (amp * rng.uniform(-1.0, 1.0, n)).astype(np.float32)


@functools.lru_cache(maxsize=1)
def batch():
    """-> list of (float32 samples, rate): ragged rows, every rate class, every path of the encoder."""
    rng = np.random.default_rng(20240611)
    spike = np.zeros(BLOCK + 64, np.float32)
    spike[1777] = 1.0                                    # one full-scale spike in silence: long unary runs
    spike[BLOCK:] = _sine(64, 0.05)                      # tail of 64 under a smooth sine (order 4: (n >> 4) <= order stops the list)
    walk48 = np.concatenate([_walk(rng, BLOCK), _sine(48, 0.01)])   # tail of 48, order 3
    special = _noise(rng, BLOCK, 1e-3)
    special[:12] = [2.5, -3.0, 1.0, -1.0, -0.0, 0.0, 1e-40, -1e-40, 1.0000001, -1.0000001, 0.99999994, -0.99999994]
    special[100:104] = [1e-38, -1e-38, 3.0517578e-05, -3.0517578e-05]
    stepped = np.concatenate([_steps(rng, BLOCK, 2), _steps(rng, BLOCK, 4), _steps(rng, BLOCK, 8), _chirp(1000)])   # 3 * 4096 + 1000
    two = np.concatenate([_sine(BLOCK, 0.002), _noise(rng, BLOCK, 0.25)])                                       # order 2; k = 13
    long_row = np.zeros(130 * BLOCK + 7, np.float32)     # the frame number crosses 127 -> 128 (1- and 2-byte form)
    for blk in (0, 126, 127, 128, 129):
        long_row[blk * BLOCK:(blk + 1) * BLOCK] = _noise(rng, BLOCK, 0.05 if blk % 2 else 1e-3)
    long_row[130 * BLOCK:] = _noise(rng, 7, 0.3)
    rows = [
        np.asarray([0.5], np.float32),
        np.asarray([0.1, -0.1], np.float32),
        _noise(rng, 4, 0.1),
        _noise(rng, 5, 0.1),
        _sine(15, 0.3),
        _noise(rng, 16, 1e-4),
        np.zeros(17, np.float32),
        _chirp(255),
        _walk(rng, 256),
        _sine(4095, 0.01),                               # order 3
        _noise(rng, BLOCK, 1.0),                         # full-scale white noise: VERBATIM
        _sine(4097, 0.05),                               # order 4; a last block of one sample
        two,                                             # 8192
        _noise(rng, 2 * BLOCK + 4, 1e-4),                # k = 0..2; a last block of four samples
        stepped,
        walk48,
        spike,
        np.full(BLOCK, 0.25, np.float32),
        np.full(BLOCK + 100, -1.0, np.float32),
        special,
        np.zeros(2 * BLOCK, np.float32),                 # digital silence
        _noise(rng, 300, 0.02),
        long_row,
    ]
    return [(r, RATES[i % len(RATES)]) for i, r in enumerate(rows)]


def to_int(x):
    return codecs._to_int(x, 2)


def reference(x, rate):
    return flac.encode(to_int(x), int(rate), 16)


@functools.lru_cache(maxsize=1)
def references():
    """The host writer's stream of every row of batch(), computed once."""
    return [reference(x, r) for x, r in batch()]


def padded(rows, fill=np.nan):
    """rows -> ([B][stride] float32 filled with `fill` past each row's length, lens)"""
    lens = np.asarray([len(r) for r in rows], np.int32)
    x = np.full((len(rows), int(lens.max())), fill, np.float32)
    for b, r in enumerate(rows):
        x[b, :len(r)] = r
    return x, lens


def frames(stream):
    """What the writer chose, frame by frame: dicts {number_bytes, n, kind ("CONSTANT" | "VERBATIM" | "FIXED"), order, po, ks}.
    Walks the stream with the reader's own bit functions (the residuals are skipped code by code, not predicted)."""
    assert stream[:4] == b"fLaC" and stream[4] == 0x80
    pos, out = 42, []
    while pos < len(stream):
        assert stream[pos] == 0xFF and stream[pos + 1] == 0xF8
        br = flac._Bits(stream, pos)
        br.read(16)
        bs_code = br.read(4)
        br.read(12)
        lead, extra = br.read(8), 0
        while lead & (0x80 >> extra):
            extra += 1
        for _ in range(max(0, extra - 1)):
            br.read(8)
        n = br.read(16) + 1 if bs_code == 7 else 256 << (bs_code - 8)
        br.read(8)   # CRC-8
        assert br.read(1) == 0
        typ = br.read(6)
        assert br.read(1) == 0
        f = {"number_bytes": max(1, extra), "n": n, "kind": None, "order": None, "po": None, "ks": []}
        if typ == 0:
            f["kind"] = "CONSTANT"
            br.read(16)
        elif typ == 1:
            f["kind"] = "VERBATIM"
            br.p += 16 * n
        else:
            assert 8 <= typ <= 12
            f["kind"], f["order"] = "FIXED", typ - 8
            br.p += 16 * f["order"]
            assert br.read(2) == 0
            f["po"] = br.read(4)
            for part in range(1 << f["po"]):
                k = br.read(4)
                f["ks"].append(k)
                for _ in range((n >> f["po"]) - (f["order"] if part == 0 else 0)):
                    br.unary()
                    br.p += k
        br.align()
        pos = (br.p >> 3) + 2
        out.append(f)
    return out
