"""Float64 reference of the engine's output sample rate (aur_seq_desc.sample_rate): the Hann-windowed sinc of
torchaudio.functional.resample (lowpass_filter_width 6, rolloff 0.99) from 24 kHz, in its DENSE form -- every tap of every phase, one
matrix product -- written from the rule in include/auralis_amd.h and independently of the kernel's sparse table.

The tolerance of a kernel output that keeps T taps of a phase (derived, not measured): an fp32 dot product of T terms is within
T 2^-24 sum_k |c_k x_k| of the exact one (one rounding per fma, first order), each coefficient is rounded once to fp32 (one more
2^-24 on every term), and one 2^-24 is left for the second-order terms:   |kernel - ref64| <= (T + 2) 2^-24 sum_k |c[p][k] x_k|."""
import math

import numpy as np

ORIG_RATE = 24000
RATES = (8000, 16000, 22050, 32000, 44100, 48000)
# taps of a phase that are not zero in fp32 (the clamped region |t| = 6 is): what the kernel keeps
KEPT_TAPS = {8000: 37, 16000: 19, 22050: 14, 32000: 13, 44100: 13, 48000: 13}


def reduced(rate):
    g = math.gcd(ORIG_RATE, int(rate))
    return ORIG_RATE // g, int(rate) // g


def n_out(n, rate):
    """ceil(n new / orig); rate 0 (unset) and 24000 keep n"""
    if rate in (0, ORIG_RATE):
        return int(n)
    orig, new = reduced(rate)
    return -(-int(n) * new // orig)


def dense_kernel(rate):
    """-> (c [new][2 width + orig] float64, orig, new, width)"""
    orig, new = reduced(rate)
    base = min(orig, new) * 0.99
    width = math.ceil(6 * orig / base)
    k = np.arange(2 * width + orig, dtype=np.float64)
    p = np.arange(new, dtype=np.float64)
    t = (-p[:, None] / new + (k[None, :] - width) / orig) * base
    t = np.clip(t, -6.0, 6.0)
    window = np.cos(t * math.pi / 12.0) ** 2
    tp = t * math.pi
    sinc = np.where(tp == 0, 1.0, np.sin(tp) / np.where(tp == 0, 1.0, tp))
    return sinc * window * (base / orig), orig, new, width


def dense_taps(rate):
    orig, new = reduced(rate)
    return dense_kernel(rate)[0].shape[1]


def resample_ref(x, rate):
    """x [n] at 24 kHz -> (y [n_out] float64, absdot [n_out] = sum_k |c[p][k] x_k|, the scale of the tolerance)"""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    n = len(x)
    if rate in (0, ORIG_RATE):
        return x.copy(), np.abs(x)
    c, orig, new, width = dense_kernel(rate)
    K = c.shape[1]
    blocks = n // orig + 1
    xpad = np.zeros(width + (blocks - 1) * orig + K + n, dtype=np.float64)
    xpad[width:width + n] = x
    win = np.stack([xpad[j * orig:j * orig + K] for j in range(blocks)])        # [blocks][K]
    y = (win @ c.T).reshape(-1)[:n_out(n, rate)]
    a = (np.abs(win) @ np.abs(c).T).reshape(-1)[:n_out(n, rate)]
    return y, a


def bound(absdot, taps):
    return (taps + 2) * 2.0 ** -24 * np.asarray(absdot, dtype=np.float64)
