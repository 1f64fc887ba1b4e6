"""GPU: the prompt-row GEMM family one launcher at a time against float64 (tests/prefill_ref.py): launch_gemm_tile with its bias +
GELU epilogue, its K slabs and their consumer rows_ln_kernel, the QKV epilogue in both forms (fused into the GEMM, and
qkv_epilogue_kernel behind the plain GEMM) on fp32 and fp16 paged pools, and the exact-f32 kernel at the shapes of the
speaker-conditioning network, through aur_dbg_gemm_tile / aur_dbg_qkv_rows / aur_dbg_rows_ln.

Three engines: split arithmetic on pre-split weight planes (the default), split arithmetic splitting the weights per tile
(AUR_GEMM_PRESPLIT=0), exact-f32 MFMA (aur_config.gemm_f32_exact).  The tile shape of a launch follows from M, N and the slab count
(gpt_kernels.hip: launch_gemm_tile; T = ceil(M / 128)):
    pre-split planes (N % 128 == 0): 128 x 128 when slabs * (N / 128) * T >= 200, else 128 x 64 when slabs * (N / 64) * T >= 200,
                                     else 64 x 64
    split per tile:                  the same rule for N <= 1024, 128 x 128 for every wider N
    exact f32:                       64 x 64 for N <= 1024 or N % 128 != 0, else 128 x 128
The M values below are the smallest that reach each shape; every test says which it reaches.

The bound against float64 is test_gpu_kernels.py: test_gemm_tile's, 2e-4 * max(1, max |ref|), unless a test says otherwise."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import prefill_ref as R
from tests.gpu_util import make_engine

pytestmark = pytest.mark.gpu

SPLIT = ("presplit", "onthefly")
MODES = SPLIT + ("exact",)


@pytest.fixture(scope="module")
def engines():
    made = {}
    try:
        made["presplit"] = make_engine(1, max_seqs=8)[0]
        with pytest.MonkeyPatch.context() as mp:   # read when the engine is created
            mp.setenv("AUR_GEMM_PRESPLIT", "0")
            made["onthefly"] = make_engine(1, max_seqs=8)[0]
        made["exact"] = make_engine(1, max_seqs=8, gemm_f32_exact=True)[0]
        yield made
    finally:
        for e in made.values():
            e.close()


def bound(ref):
    return 2e-4 * max(1.0, float(np.abs(ref).max()))


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def randn(g, *shape):
    return torch.randn(*shape, generator=g).numpy()


# ---------------------------------------------------------------------------------------------------------------------------------
# bias + GELU epilogue
@functools.lru_cache(maxsize=None)
def gelu_case(N, K, M):
    """pre-activations ~ N(0, 1.6^2): both GELU forms are exercised over their curved part"""
    g = torch.Generator().manual_seed(N + K)
    X, W, bias = randn(g, M, K), randn(g, K, N) * np.float32(1.6 / np.sqrt(K)), randn(g, N) * np.float32(0.1)
    pre = R.f64(X) @ R.f64(W) + R.f64(bias)
    return X, W, bias, pre, {False: R.gelu_tanh(pre), True: R.gelu_erf(pre)}


def run_gelu(engines, N, K, Ms, erf):
    X, W, bias, _, refs = gelu_case(N, K, max(Ms))
    ref = refs[erf]
    got = {}
    for mode in MODES:
        for M in Ms:
            out = engines[mode].dbg_gemm_tile(X[:M], W, bias, epi=1, erf=erf)
            err = np.abs(out - ref[:M]).max()
            print(f"gelu erf={int(erf)} {mode} M={M} N={N} K={K}: max err {err:.3e}, bound {bound(ref[:M]):.3e}")
            assert np.isfinite(out).all() and err < bound(ref[:M]), (mode, M, err)
            got[mode, M] = out
        for M in Ms:   # batch invariance across tile shapes, the epilogue on
            assert same_bits(got[mode, max(Ms)][:M], got[mode, M]), (mode, M)
    for M in Ms:
        assert same_bits(got["presplit", M], got["onthefly", M]), M


@pytest.mark.parametrize("erf", [False, True])
def test_gelu_epilogue_fc_shape(engines, erf):
    """N = 4096, K = 1024, the FC GEMM.  Pre-split planes: M = 1, 71, 129 run 64 x 64 (32 * T < 200 and 64 * T < 200 up to T = 3),
    400 runs 128 x 64 (T = 4: 256), 800 runs 128 x 128 (T = 7: 224).  Split per tile and exact f32: 128 x 128 at every M."""
    run_gelu(engines, 4096, 1024, (1, 71, 129, 400, 800), erf)


@pytest.mark.parametrize("erf", [False, True])
def test_gelu_epilogue_narrow_shapes(engines, erf):
    """N = 1024 is where the kernels without pre-split planes leave 128 x 128: split per tile runs 64 x 64 at M = 71 and 128 x 64 at
    M = 1537 (T = 13: 16 * 13 = 208 >= 200 > 8 * 13), exact f32 runs 64 x 64; pre-split planes 64 x 64 and 128 x 64.  K = 64 keeps it
    small: four k steps, two passes of the split kernel's two-step loop."""
    run_gelu(engines, 1024, 64, (71, 1537), erf)


def test_gelu_erf_flag_selects_the_form(engines):
    """The two GELU forms are at most 4.7e-4 apart, inside the 2e-4 * max|ref| bound above, so a kernel that ignored `erf` would
    pass there.  Here the bound is 4 x the error of a plain float32 CPU evaluation (torch fp32 matmul + bias + fp32 gelu) against
    float64, + 1e-6: the margin test_gemm_tile_split_arithmetic_matches_exact_f32 gives the split arithmetic over fp32.  The inputs
    must tell the forms apart: they differ by more than 5 x that bound on at least a quarter of the elements."""
    M = 71
    X, W, bias, pre, refs = gelu_case(4096, 1024, 800)
    X, pre = X[:M], pre[:M]
    pre32 = torch.from_numpy(X) @ torch.from_numpy(W) + torch.from_numpy(bias)
    bounds = {}
    for erf, approx in ((False, "tanh"), (True, "none")):
        e32 = np.abs(F.gelu(pre32, approximate=approx).double().numpy() - refs[erf][:M]).max()
        bounds[erf] = 4.0 * e32 + 1e-6
        print(f"erf={int(erf)}: fp32 CPU max err {e32:.3e} -> bound {bounds[erf]:.3e}")
    apart = np.abs(refs[False][:M] - refs[True][:M])
    frac = float((apart > 5.0 * max(bounds.values())).mean())
    print(f"forms differ by more than 5 x bound on {100 * frac:.1f} % of the elements (max {apart.max():.3e})")
    assert frac >= 0.25, frac
    for erf in (False, True):
        out = engines["presplit"].dbg_gemm_tile(X, W, bias, epi=1, erf=erf)
        err, wrong = np.abs(out - refs[erf][:M]).max(), np.abs(out - refs[not erf][:M]).max()
        print(f"erf={int(erf)}: max err {err:.3e} against its own form, {wrong:.3e} against the other")
        assert err < bounds[erf], (erf, err, bounds[erf])


# ---------------------------------------------------------------------------------------------------------------------------------
# K slabs and rows_ln_kernel behind them
SLAB_MS = (1, 71, 400, 800)


@functools.lru_cache(maxsize=None)
def slab_case():
    g = torch.Generator().manual_seed(4096)
    X, W = randn(g, max(SLAB_MS), 4096), randn(g, 4096, 1024) * np.float32(0.05)
    return X, W, {s: R.slabs_ref(X, W, s) for s in (1, 2, 4)}


@functools.lru_cache(maxsize=None)
def ln_case():
    g = torch.Generator().manual_seed(7)
    return randn(g, max(SLAB_MS), 1024) * np.float32(3.0) + np.float32(0.5), randn(g, 1024), randn(g, 1024), randn(g, 1024)


@pytest.mark.parametrize("slabs", [1, 2, 4])
def test_k_slabs_proj2_shape(engines, slabs):
    """K = 4096, N = 1024 (the proj2 GEMM; the engine runs it with 4 slabs).  Both split-arithmetic forms count the slabs into the tile
    choice: with 4 slabs M = 800 runs 128 x 128 (4 * 8 * 7 = 224), M = 400 runs 128 x 64 (4 * 16 * 4 = 256), 71 and 1 run 64 x 64;
    with 2 slabs 800 runs 128 x 64 (2 * 16 * 7 = 224) and the rest 64 x 64; with one slab everything runs 64 x 64, as on exact f32.
    Every slab against float64 of ITS k range -- a wrong slab offset of X, W, P or of the pre-split planes moves a slab to other k."""
    X, W, refs = slab_case()
    ref = refs[slabs]
    got = {}
    for mode in MODES:
        for M in SLAB_MS:
            out = engines[mode].dbg_gemm_tile(X[:M], W, slabs=slabs)
            assert out.shape == (slabs, M, 1024) and np.isfinite(out).all(), (mode, M)
            for s in range(slabs):
                err = np.abs(out[s] - ref[s, :M]).max()
                assert err < bound(ref[s, :M]), (mode, M, s, err)
            got[mode, M] = out
        for M in SLAB_MS:
            assert same_bits(got[mode, max(SLAB_MS)][:, :M], got[mode, M]), (mode, M)
    for M in SLAB_MS:
        for s in range(slabs):
            assert same_bits(got["presplit", M][s], got["onthefly", M][s]), (M, s)


def test_k_slabs_into_rows_ln(engines):
    """The proj2 chain of forward_rows: four slabs, then rows_ln_kernel with S = 4 sums them in a fixed order, adds the bias, updates
    the residual h in place and normalises it.  Updated h and the LayerNorm output against float64 of the whole chain within
    2e-5 * max(1, max |ref|), test_layernorm's bound scaled; rows of the 800-row chain equal the 71-row chain bit for bit."""
    X, W, refs = slab_case()
    h, bias, gamma, beta = ln_case()
    ref_h, ref_out = R.rows_ln_ref(h, refs[4], bias, gamma, beta)
    for mode in MODES:
        got = {}
        for M in SLAB_MS:
            P = engines[mode].dbg_gemm_tile(X[:M], W, slabs=4)
            h2, out = engines[mode].dbg_rows_ln(P, bias, h[:M], gamma, beta)
            for name, a, r in (("h", h2, ref_h[:M]), ("out", out, ref_out[:M])):
                err, b = np.abs(a - r).max(), 2e-5 * max(1.0, float(np.abs(r).max()))
                print(f"rows_ln S=4 {mode} M={M} {name}: max err {err:.3e}, bound {b:.3e}")
                assert np.isfinite(a).all() and err < b, (mode, M, name, err, b)
            got[M] = (h2, out)
        assert same_bits(got[800][0][:71], got[71][0]) and same_bits(got[800][1][:71], got[71][1]), mode


@pytest.mark.parametrize("S", [0, 1, 2, 3, 4, 5])
def test_rows_ln_slab_counts(engines, S):
    """rows_ln_kernel alone on given slabs: slab_sum loads four slabs at a time at clamped indices, so S = 1..3 and 5 take its
    partial groups; S = 0 leaves h alone (aur_dbg_layernorm's case).  The slabs are summed in fp32, hence the scaled bound."""
    g = torch.Generator().manual_seed(100 + S)
    M = 37
    h, bias, gamma, beta = randn(g, M, 1024) * np.float32(3.0) + np.float32(0.5), randn(g, 1024), randn(g, 1024), randn(g, 1024)
    P = randn(g, S, M, 1024) if S else None
    ref_h, ref_out = R.rows_ln_ref(h, P, bias, gamma, beta)
    h2, out = engines["presplit"].dbg_rows_ln(P, bias if S else None, h, gamma, beta)
    if S == 0:
        assert same_bits(h2, h)
    for a, r in ((h2, ref_h), (out, ref_out)):
        err = np.abs(a - r).max()
        assert err < 2e-5 * max(1.0, float(np.abs(r).max())), (S, err)


# ---------------------------------------------------------------------------------------------------------------------------------
# QKV epilogue
# M -> (first position, rows) per sequence and ctx_max: positions ascend by one inside a sequence, sequence 0 starts behind a 32-token
# prefix, runs cross several 16-token block boundaries and end in mid-block; ctx_max is no multiple of 16 (a last block with a tail)
QKV_ROWS = {
    1: ([37], [1], 41),
    71: ([32, 0], [45, 26], 79),
    200: ([32, 0, 7], [100, 61, 39], 135),
    600: ([32, 0, 16, 3], [300, 150, 101, 49], 335),
    1100: ([32, 0, 5, 16], [640, 250, 147, 63], 675),
}


@functools.lru_cache(maxsize=None)
def qkv_weights():
    g = torch.Generator().manual_seed(3072)
    return randn(g, 1024, 3072) * np.float32(0.05), randn(g, 3072)


@pytest.mark.parametrize("M", sorted(QKV_ROWS))
def test_qkv_epilogue(engines, M):
    """N = 3072, K = 1024.  Pre-split planes: M = 1, 71, 200 run 64 x 64 (48 * T < 200 up to T = 4), 600 runs 128 x 64 (T = 5: 240),
    1100 runs 128 x 128 (24 * 9 = 216); split per tile and exact f32 run 128 x 128.  Row tiles with rows past M (every M here) stage
    the K / V address of row M - 1 for them and must not store.  Per engine, pool type and form:
      1. q rows against float64;  2. K and V at every written (sequence, position) against float64, the fp16 pool with one rounding
      to nearest on top (2^-11 |ref|);  3. every other element of the pool arrays bit for bit as it was, and no stray word in the
      pool outside the contexts;  4. fused == separate bit for bit (both add one bias to one fp32 total: slab_sum with S = 1 is
      (0 + p) + bias);  5. pre-split == split per tile bit for bit."""
    starts, lengths, ctx_max = QKV_ROWS[M]
    row_seq, row_pos = R.ragged_rows(starts, lengths)
    assert len(row_seq) == M and row_pos.max() < ctx_max <= 1056
    n_seq = len(starts)
    W, bias = qkv_weights()
    g = torch.Generator().manual_seed(M)
    X = randn(g, M, 1024)
    y = R.f64(X) @ R.f64(W) + R.f64(bias)
    k0, v0 = randn(g, n_seq, ctx_max, 1024), randn(g, n_seq, ctx_max, 1024)
    for kv_half in (False, True):
        ka, va = (k0.astype(np.float16).astype(np.float32), v0.astype(np.float16).astype(np.float32)) if kv_half else (k0, v0)
        ref_q, ref_k, ref_v, written = R.qkv_scatter_ref(y, row_seq, row_pos, ka, va)
        got = {}
        for mode in MODES:
            for fused in ((True, False) if mode in SPLIT else (False,)):
                q, k, v, stray = engines[mode].dbg_qkv_rows(X, W, bias, row_seq, row_pos, ka, va, fused=fused, kv_half=kv_half)
                tag = (mode, fused, kv_half)
                assert np.isfinite(q).all() and np.abs(q - ref_q).max() < bound(ref_q), tag
                for a, r, a0 in ((k, ref_k, ka), (v, ref_v, va)):
                    rw = r[written]
                    tol = bound(rw) + (2.0 ** -11 * np.abs(rw) if kv_half else 0.0)
                    assert (np.abs(a[written] - rw) < tol).all(), tag
                    assert same_bits(a[~written], a0[~written]), tag
                assert stray == 0, tag
                got[mode, fused] = (q, k, v)
        for mode in SPLIT:
            assert all(same_bits(a, b) for a, b in zip(got[mode, True], got[mode, False])), (mode, kv_half)
        for fused in (True, False):
            assert all(same_bits(a, b) for a, b in zip(got["presplit", fused], got["onthefly", fused])), (fused, kv_half)


def test_qkv_rows_refuses_what_it_cannot_run(engines):
    """Nothing reaches a kernel: the fused form on an exact-f32 engine and positions outside the pool are argument errors."""
    from auralis_amd._lib import AurError
    W, bias = qkv_weights()
    X = np.zeros((2, 1024), np.float32)
    k = np.zeros((1, 20, 1024), np.float32)
    ok = (np.array([0, 0], np.int32), np.array([3, 4], np.int32))
    with pytest.raises(AurError):
        engines["exact"].dbg_qkv_rows(X, W, bias, *ok, k, k, fused=True)
    for rs, rp in (([0, 1], [3, 4]), ([0, 0], [3, 20]), ([0, -1], [3, 4]), ([0, 0], [-1, 4])):
        with pytest.raises(AurError):
            engines["presplit"].dbg_qkv_rows(X, W, bias, np.array(rs, np.int32), np.array(rp, np.int32), k, k, fused=True)


# ---------------------------------------------------------------------------------------------------------------------------------
# the exact-f32 kernel as the speaker-conditioning network calls it (cond_net.h: gemm(), weights.py: pack_conditioning), on a default
# engine.  (N, K): what the shape is in the network and what it exercises
COND_SHAPES = [
    (64, 16),       # first ResNet convolution, 1 -> 64 channels im2col'ed: a single k step, one 64-column tile, N % 128 != 0
    (1024, 80),     # ConditioningEncoder init, 80 mel bins: 5 k steps, K % 32 != 0
    (128, 272),     # speaker mel filterbank: 17 k steps, one column tile pair
    (128, 1040),    # GPT mel filterbank: 65 k steps
    (640, 512),     # speaker DFT: 10 column tiles of 64, the plain tile order
    (2176, 2048),   # GPT DFT: 128 x 128 tiles, 17 column tiles, the plain tile order
    (2048, 128),    # attentive pooling logits: 128 x 128 tiles, 16 column tiles, the XCD-aware order
    (64, 576),      # ResNet layer 1 convolutions
    (1024, 2736),   # perceiver feed-forward out: 171 k steps
]
COND_MS = (1, 63, 65, 130)


@pytest.mark.parametrize("N,K", COND_SHAPES)
def test_exact_f32_kernel_at_conditioning_shapes(engines, N, K):
    g = torch.Generator().manual_seed(N * 7 + K)
    X, W = randn(g, max(COND_MS), K), randn(g, K, N) * np.float32(1.0 / np.sqrt(K))
    ref = R.slabs_ref(X, W, 1)[0]
    for M in COND_MS:
        out = engines["presplit"].dbg_gemm_tile(X[:M], W, exact=True)[0]
        err = np.abs(out - ref[:M]).max()
        assert np.isfinite(out).all() and err < bound(ref[:M]), (M, err)
        # ... and it is the kernel an exact-f32 engine runs
        if M == 65:
            assert same_bits(out, engines["exact"].dbg_gemm_tile(X[:M], W)[0])


@pytest.mark.parametrize("mode,exact,N,K", [("presplit", True, 1024, 80), ("presplit", True, 2176, 2048), ("presplit", False, 1024, 1024),
                                            ("onthefly", False, 1024, 1024), ("presplit", False, 3072, 1024)])
def test_row_stride_wider_than_k(engines, mode, exact, N, K):
    """ldx = K + 16, the 16 padding columns of every row NaN (cond_net.h hands rows of padded buffers): nothing past column K is read,
    and the result is bit for bit the one on packed rows."""
    g = torch.Generator().manual_seed(N + K + 16)
    M = 130
    X, W = randn(g, M, K), randn(g, K, N) * np.float32(1.0 / np.sqrt(K))
    Xp = np.full((M, K + 16), np.nan, np.float32)
    Xp[:, :K] = X
    ref = R.slabs_ref(X, W, 1)[0]
    out = engines[mode].dbg_gemm_tile(Xp, W, exact=exact, K=K)[0]
    assert np.isfinite(out).all() and np.abs(out - ref).max() < bound(ref)
    assert same_bits(out, engines[mode].dbg_gemm_tile(X, W, exact=exact)[0])
