"""CPU: the float64 reference of the per-kernel vocoder tests (tests/vocoder_ref.py) against torch's own convolutions, the oracle's
ResBlock and F.interpolate -- so that tests/test_gpu_vocoder_kernels.py compares the kernels with something that is itself checked."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from auralis_amd import weights as Wt
from oracle import xtts_oracle as O
from tests import vocoder_ref as R

KD = [(k, d) for k in (3, 7, 11) for d in (1, 3, 5)]
LENS = [37, 64, 5]   # ragged: shorter than the widest halo (50), a power of two, longer


def _rand(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


@pytest.mark.parametrize("k,d", KD)
def test_conv_reference_equals_torch_conv1d_on_ragged_lengths(k, d):
    g = torch.Generator().manual_seed(16 * k + d)
    cin, cout, L = 6, 5, max(LENS)
    x, w, b = _rand(g, 3, cin, L), _rand(g, cout, cin, k), _rand(g, cout)
    cond, res, mrf = _rand(g, 4, cout + 2), _rand(g, 3, cout, L), _rand(g, 3, cout, L)
    pad = (k - 1) // 2 * d
    for mode in range(4):
        got = R.conv_ref(x.numpy(), w.numpy(), LENS, d, pad, slope=0.1, bias=b.numpy(), cond=cond.numpy(), cond_row=[2, 0, 3],
                         res=res.numpy(), mrf=mrf.numpy(), mrf_mode=mode)
        for bi, n in enumerate(LENS):
            ref = F.conv1d(F.leaky_relu(x[bi:bi + 1, :, :n], 0.1), w, b, dilation=d, padding=pad)[0]
            ref = ref + cond[[2, 0, 3][bi], :cout, None] + res[bi, :, :n]
            ref = (ref, ref, ref + mrf[bi, :, :n], (ref + mrf[bi, :, :n]) / 3)[mode]
            assert np.abs(got[bi, :, :n] - ref.numpy()).max() < 1e-12
            assert np.isnan(got[bi, :, n:]).all()


def test_conv_reference_unactivates_the_residual():
    g = torch.Generator().manual_seed(5)
    x, w = _rand(g, 1, 4, 9), _rand(g, 4, 4, 3)
    y = R.lrelu(x.numpy(), 0.1)
    got = R.conv_ref(np.zeros_like(y), w.numpy(), [9], 1, 1, res=y, res_unact=10.0)
    assert np.abs(got - x.numpy()).max() < 1e-15


@pytest.mark.parametrize("s,k", [(8, 16), (2, 4)])
def test_conv_reference_equals_torch_conv_transpose1d_on_ragged_lengths(s, k):
    g = torch.Generator().manual_seed(s)
    cin, cout, L = 6, 5, max(LENS)
    x, w, b = _rand(g, 3, cin, L), _rand(g, cin, cout, k), _rand(g, cout)
    got = R.conv_ref(x.numpy(), Wt.polyphase_convT(w, s).numpy(), LENS, 1, 1, slope=0.1, bias=b.numpy(), ups_s=s, ups_p=(k - s) // 2)
    for bi, n in enumerate(LENS):
        ref = F.conv_transpose1d(F.leaky_relu(x[bi:bi + 1, :, :n], 0.1), w, b, stride=s, padding=(k - s) // 2)[0]
        assert ref.shape[1] == n * s
        assert np.abs(got[bi, :, :n * s] - ref.numpy()).max() < 1e-12
        assert np.isnan(got[bi, :, n * s:]).all()


def test_round_reference_chained_equals_the_oracles_resblock():
    """Three rounds (dilations 1, 3, 5) of round_ref on the activated stream = one ResBlock1 of the oracle's generator, taken from
    hifigan_forward with one upsampling stage and one ResBlock (its MRF mean over one block is the block's output)."""
    g = torch.Generator().manual_seed(77)
    C, k, T = 4, 7, 23
    w = {"conv_pre.weight": _rand(g, 2 * C, 3, 7), "conv_pre.bias": _rand(g, 2 * C), "cond_layer.weight": _rand(g, 2 * C, 2, 1),
         "cond_layer.bias": _rand(g, 2 * C), "ups.0.weight": _rand(g, 2 * C, C, 4) / 4, "ups.0.bias": _rand(g, C),
         "conds.0.weight": _rand(g, C, 2, 1), "conds.0.bias": _rand(g, C), "conv_post.weight": _rand(g, 1, C, 7)}
    for c in range(3):
        for n in ("convs1", "convs2"):
            w[f"resblocks.0.{n}.{c}.weight"] = _rand(g, C, C, k) / (C * k) ** 0.5
            w[f"resblocks.0.{n}.{c}.bias"] = _rand(g, C)
    col = {}
    O.hifigan_forward(w, _rand(g, 3, T), _rand(g, 1, 2, 1), ups=((2, 4),), rb_kernels=(k,), collect=col)
    x = col["ups.0"].numpy()
    L = x.shape[2]
    for c, d in enumerate((1, 3, 5)):
        _, x = R.round_ref(R.lrelu(x, 0.1), w[f"resblocks.0.convs1.{c}.weight"].numpy(), w[f"resblocks.0.convs1.{c}.bias"].numpy(),
                           w[f"resblocks.0.convs2.{c}.weight"].numpy(), w[f"resblocks.0.convs2.{c}.bias"].numpy(), [L], d)
    assert np.abs(x - col["mrf.0"].numpy()).max() < 1e-12


def test_round_reference_pads_the_conv1_output_with_zeros():
    """conv2 sees h == 0 outside the utterance, not conv1 evaluated there: with a bias on conv1 the two differ at the ends"""
    g = torch.Generator().manual_seed(3)
    C, k, n = 4, 3, 11
    y, w1, w2 = _rand(g, 2, C, n + 6).numpy(), _rand(g, C, C, k).numpy(), _rand(g, C, C, k).numpy()
    b1, b2 = np.full(C, 2.0), np.zeros(C)
    h, v = R.round_ref(y, w1, b1, w2, b2, [n + 6, n], 1)
    assert (h[1, :, n:] == 0).all() and np.isnan(v[1, :, n:]).all()
    alone = R.round_ref(y[1:, :, :n], w1, b1, w2, b2, [n], 1)[1]
    assert np.array_equal(v[1, :, :n], alone[0])


def test_interp_reference_equals_two_chained_torch_interpolations():
    g = torch.Generator().manual_seed(9)
    n_lat, C = [1, 2, 7, 31], 8
    lat = torch.randn(6, 31, C, generator=g)
    rows = [4, 0, 5, 2]
    got = R.interp2_ref(lat.numpy(), rows, n_lat)
    for b, n in enumerate(n_lat):
        z = F.interpolate(lat[rows[b], :n].T[None], scale_factor=4.0, mode="linear", align_corners=False)
        z = F.interpolate(z, scale_factor=24000 / 22050, mode="linear", align_corners=False)[0]
        assert got[b].shape == tuple(z.shape) == (C, R.frames_for(n))
        assert np.abs(got[b] - z.double().numpy()).max() < 1e-6


def test_conv_post_reference_and_fp16_spacing():
    g = torch.Generator().manual_seed(2)
    x, w = _rand(g, 2, 5, 40), _rand(g, 5, 7) / 6
    s, wav = R.conv_post_ref(x.numpy(), w.numpy(), [40, 17], 0.01)
    for bi, n in enumerate([40, 17]):
        ref = torch.tanh(F.conv1d(F.leaky_relu(x[bi:bi + 1, :, :n], 0.01), w[None], padding=3))[0, 0]
        assert np.abs(wav[bi, :n] - ref.numpy()).max() < 1e-12
    for v in (0.0, 1e-9, 2.0 ** -14, 0.3, 1.0, 1.5, 2.0, -777.0, 32768.0):
        want = float(np.spacing(np.float16(abs(v)))) if abs(v) >= 2.0 ** -24 else 2.0 ** -24
        assert float(R.ulp16(v)) == want, v
