"""Float64 restatement of what the prompt-row (prefill) GEMM launcher and its consumers compute (auralis_amd/csrc/gpt_kernels.h:
launch_gemm_tile, launch_rows_ln, launch_qkv_epilogue), one operation at a time, for the per-kernel tests.  Plain numpy.
tests/test_prefill_ref.py holds these against torch's float64 gelu / layer_norm and a plain loop on the CPU;
tests/test_gpu_prefill_kernels.py holds the kernels against them.

    slabs      P[s] = X[:, s K' : (s + 1) K'] @ W[s K' : (s + 1) K'],  K' = K / slabs
    GELU       gelu(X @ W + bias), tanh form ("gelu_new") or erf form ("gelu")
    rows_ln    h' = h + sum_s P[s] + bias;  out = (h' - mean) / sqrt(var + eps) * gamma + beta  (biased variance over the 1024 columns)
    QKV        y = X @ W + bias, 3072 columns: column n of row m is q[m][n] for n < 1024, else K (1024 <= n < 2048) or V (n >= 2048)
               of token row_pos[m] of sequence row_seq[m], column n % 1024 (head (n % 1024) / 64, element n % 64 inside a token)"""
import math

import numpy as np

HIDDEN = 1024
_erf = np.frompyfunc(math.erf, 1, 1)   # libm's erf, element by element: numpy has none, and torch's is what the CPU test compares with


def f64(a):
    return np.asarray(a, dtype=np.float64)


def gelu_tanh(x):
    x = f64(x)
    return 0.5 * x * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def gelu_erf(x):
    x = f64(x)
    return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)).astype(np.float64))


def gelu(x, erf):
    return gelu_erf(x) if erf else gelu_tanh(x)


def slabs_ref(X, W, slabs):
    """[slabs][M][N]: slab s is the product over its K / slabs consecutive k"""
    X, W = f64(X), f64(W)
    K = W.shape[0]
    assert X.shape[1] == K and K % slabs == 0
    kp = K // slabs
    return np.stack([X[:, s * kp:(s + 1) * kp] @ W[s * kp:(s + 1) * kp] for s in range(slabs)])


def rows_ln_ref(h, P, bias, gamma, beta, eps=1e-5):
    """(h', out): h' = h + sum_s P[s] + bias (h itself when P is None), out = LayerNorm(h') over the last axis"""
    h2 = f64(h)
    if P is not None:
        h2 = h2 + f64(P).sum(axis=0) + f64(bias)
    mean = h2.mean(axis=-1, keepdims=True)
    var = ((h2 - mean) ** 2).mean(axis=-1, keepdims=True)
    return h2, (h2 - mean) / np.sqrt(var + eps) * f64(gamma) + f64(beta)


def ragged_rows(starts, lengths):
    """(row_seq, row_pos) of prompt rows: sequence i contributes lengths[i] consecutive rows at positions starts[i], starts[i] + 1, ..."""
    row_seq = np.concatenate([np.full(n, i, dtype=np.int32) for i, n in enumerate(lengths)])
    row_pos = np.concatenate([np.arange(s, s + n, dtype=np.int32) for s, n in zip(starts, lengths)])
    return row_seq, row_pos


def qkv_dest(m, n, row_seq, row_pos):
    """where column n of row m of the QKV product goes: ("q", m, n) or ("k" | "v", sequence, position, column)"""
    u, d = divmod(int(n), HIDDEN)
    if u == 0:
        return ("q", int(m), d)
    return ("k" if u == 1 else "v", int(row_seq[m]), int(row_pos[m]), d)


def qkv_scatter_ref(y, row_seq, row_pos, k, v):
    """y [M][3072] -> (q [M][1024], k', v' [n_seq][ctx_max][1024], written [n_seq][ctx_max] bool): the pool arrays with the rows'
    K / V columns stored at (row_seq[m], row_pos[m]) and everything else as it was"""
    y = f64(y)
    assert y.shape[1] == 3 * HIDDEN
    k2, v2 = f64(k).copy(), f64(v).copy()
    written = np.zeros(k2.shape[:2], dtype=bool)
    assert not written[row_seq, row_pos].any() and len(set(zip(row_seq.tolist(), row_pos.tolist()))) == len(row_seq), "one row per token"
    k2[row_seq, row_pos] = y[:, HIDDEN:2 * HIDDEN]
    v2[row_seq, row_pos] = y[:, 2 * HIDDEN:]
    written[row_seq, row_pos] = True
    return y[:, :HIDDEN].copy(), k2, v2, written
