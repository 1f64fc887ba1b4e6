"""CPU: the float64 references of the prompt-row GEMM family (tests/prefill_ref.py) against torch in float64 and plain loops."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import prefill_ref as R


def test_both_gelu_forms_equal_torch_in_float64():
    x = torch.cat([torch.randn(4000, generator=torch.Generator().manual_seed(3), dtype=torch.float64) * 1.6,
                   torch.tensor([0.0, -0.0, 1e-30, -1e-30, 6.0, -6.0, 12.0, -12.0, 40.0, -40.0], dtype=torch.float64)])
    for erf, approx in ((False, "tanh"), (True, "none")):
        got = R.gelu(x.numpy(), erf)
        assert got.dtype == np.float64
        assert np.abs(got - F.gelu(x, approximate=approx).numpy()).max() < 1e-14, approx
    # the two forms are different functions: 4.7e-4 apart at their widest, the figure the GPU test of the `erf` flag rests on
    g = np.linspace(-6.0, 6.0, 240001)
    d = np.abs(R.gelu_tanh(g) - R.gelu_erf(g)).max()
    assert 4.6e-4 < d < 4.8e-4, d


def test_rows_ln_equals_torch_layer_norm_in_float64():
    g = torch.Generator().manual_seed(4)
    h = torch.randn(7, 1024, generator=g, dtype=torch.float64) * 3 + 0.5
    P = torch.randn(4, 7, 1024, generator=g, dtype=torch.float64)
    bias, gamma, beta = (torch.randn(1024, generator=g, dtype=torch.float64) for _ in range(3))
    h2, out = R.rows_ln_ref(h.numpy(), P.numpy(), bias.numpy(), gamma.numpy(), beta.numpy())
    want_h = h + P[0] + P[1] + P[2] + P[3] + bias
    assert np.abs(h2 - want_h.numpy()).max() < 1e-13
    assert np.abs(out - F.layer_norm(want_h, (1024,), gamma, beta, 1e-5).numpy()).max() < 1e-12
    # no slabs: h is left alone
    h0, out0 = R.rows_ln_ref(h.numpy(), None, None, gamma.numpy(), beta.numpy())
    assert np.array_equal(h0, h.numpy())
    assert np.abs(out0 - F.layer_norm(h, (1024,), gamma, beta, 1e-5).numpy()).max() < 1e-12


def test_slabs_sum_to_the_product():
    g = torch.Generator().manual_seed(5)
    X = torch.randn(5, 64, generator=g, dtype=torch.float64)
    W = torch.randn(64, 8, generator=g, dtype=torch.float64)
    for s in (1, 2, 4):
        P = R.slabs_ref(X.numpy(), W.numpy(), s)
        assert P.shape == (s, 5, 8)
        assert np.abs(P.sum(axis=0) - (X @ W).numpy()).max() < 1e-13
        assert np.abs(P[s - 1] - (X[:, 64 - 64 // s:] @ W[64 - 64 // s:]).numpy()).max() < 1e-13


def test_qkv_scatter_equals_a_plain_loop():
    row_seq, row_pos = R.ragged_rows([32, 0, 5], [20, 3, 12])
    assert row_seq.tolist() == [0] * 20 + [1] * 3 + [2] * 12
    assert row_pos.tolist() == list(range(32, 52)) + [0, 1, 2] + list(range(5, 17))
    M, n_seq, ctx = len(row_seq), 3, 53
    rng = np.random.default_rng(6)
    y = rng.standard_normal((M, 3072))
    k0, v0 = rng.standard_normal((n_seq, ctx, 1024)), rng.standard_normal((n_seq, ctx, 1024))
    q, k, v, written = R.qkv_scatter_ref(y, row_seq, row_pos, k0, v0)
    wq, wk, wv = np.full((M, 1024), np.nan), k0.copy(), v0.copy()
    touched = set()
    for m in range(M):
        for n in range(3072):
            dest = R.qkv_dest(m, n, row_seq, row_pos)
            if dest[0] == "q":
                assert dest == ("q", m, n)
                wq[m, n] = y[m, n]
            else:
                kind, sq, pos, col = dest
                assert kind == ("k" if n < 2048 else "v") and col == n % 1024 and (sq, pos) == (row_seq[m], row_pos[m])
                (wk if kind == "k" else wv)[sq, pos, col] = y[m, n]
                touched.add((sq, pos))
    assert np.array_equal(q, wq) and np.array_equal(k, wk) and np.array_equal(v, wv)
    assert {(int(a), int(b)) for a, b in zip(*np.nonzero(written))} == touched and written.sum() == M
    assert np.array_equal(k[~written], k0[~written]) and np.array_equal(v[~written], v0[~written])
