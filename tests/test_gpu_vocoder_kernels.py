"""GPU: every kernel the fp16 vocoder launches (HifiGan::forward with vocoder_fp16), one at a time, against the float64 reference of
tests/vocoder_ref.py on the fp16-rounded operands actually uploaded -- the LDS-DMA conv in its 8-wave all-halves form and its 4-wave
transposed-conv form, the fused ResBlock round, interp2 and conv_post -- plus the fp32 conv kernel's conditioning and MRF modes.

Bound per element of a halves output:  |got - ref| <= 0.5 * ulp16(ref) + 3e-5 * max(1, max|ref|)  (the one fp16 rounding of the
store, and the bound test_gpu_kernels.py::test_conv1d_mfma_f16 uses for this MFMA arithmetic); fp32 outputs the second term alone
(2e-5 on the fp32 kernel, as test_conv1d_mfma).  Every case also checks that positions past an utterance still hold the sentinel the
tensor was uploaded with, that the guards around every output buffer are untouched, and that utterance 0 alone equals its rows of the
batch bit for bit.  Lengths are [2 * NT + 1, NT, 5] for the position tile NT of the kernel under test."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from auralis_amd import weights as Wt
from auralis_amd._lib import AurError
from tests import vocoder_ref as R
from tests.gpu_util import make_engine

pytestmark = pytest.mark.gpu

SENT = -777.0
KD = [(k, d) for k in (3, 7, 11) for d in (1, 3, 5)]
COND_ROW = [2, 0, 1]


@pytest.fixture(scope="module")
def eng():
    e, *_ = make_engine(1, max_seqs=2, vocoder_fp16=True)
    yield e
    e.close()


def _gen(*key):
    return torch.Generator().manual_seed(sum(int(v) * 1000 ** i for i, v in enumerate(key)) + 7)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g).numpy()


def _h(a):
    """round to fp16, as float32: what the harness uploads exactly"""
    return np.asarray(a, dtype=np.float32).astype(np.float16).astype(np.float32)


def _stream(g, *shape, slope=0.1):
    """an activated stream as the vocoder stores it: fp16(lrelu(x, slope)), x ~ N(0, 1)"""
    return _h(R.lrelu(_randn(g, *shape), slope))


def _weight(g, cout, cin, k):
    return _randn(g, cout, cin, k) / np.float32((cin * k) ** 0.5)


def _lens(nt):
    return [2 * nt + 1, nt, 5]


def _running_sum(g, lens, C):
    """a running MRF sum ~ N(0, 1) rounded to fp16; the sentinel where no utterance owns the position"""
    m = _h(_randn(g, len(lens), C, max(lens)))
    for b, n in enumerate(lens):
        m[b, :, n:] = SENT
    return m


def _check(got, ref, lens, tag, half=True, rel=3e-5):
    """the module's bound on every element an utterance owns, the sentinel everywhere else; ref [B][C][L] float64 (NaN outside)"""
    for b, n in enumerate(lens):
        r, g_ = ref[b, :, :n], got[b, :, :n].astype(np.float64)
        assert np.isfinite(r).all()
        bound = rel * max(1.0, np.abs(r).max()) + (0.5 * R.ulp16(r) if half else 0.0)
        err = np.abs(g_ - r)
        print(f"{tag} b={b} n={n}: max err {err.max():.3e}, max err / bound {(err / bound).max():.3f}, max|ref| {np.abs(r).max():.3f}")
        bad = np.argwhere(err > bound)
        assert bad.size == 0, (tag, b, len(bad), bad[:8].tolist(), err.max())
        assert (got[b, :, n:] == SENT).all(), (tag, b, "written past the utterance")


def _first(arrs, lens):
    """utterance 0 alone: the leading batch item of every tensor (None stays None)"""
    return [None if a is None else a[:1] for a in arrs], lens[:1]


# ---- a. the 8-wave LDS-DMA conv, all-halves epilogue (conv_pre, the ResBlock convs of the 256- and 128-channel stages) ----
@pytest.mark.parametrize("k,d", KD)
def test_dma_conv_all_halves_modes_against_float64(eng, k, d):
    g = _gen(k, d, 1)
    cin, cout, lens = 64, 128, _lens(512)
    L, pad = max(lens), (k - 1) // 2 * d
    x, res = _stream(g, 3, cin, L), _stream(g, 3, cout, L)
    w16, bias, mrf = _h(_weight(g, cout, cin, k)), _randn(g, cout), _running_sum(g, lens, cout)
    wp = Wt.pack_conv_f16(torch.from_numpy(w16)).numpy()
    for mode, osl in [(0, 0.1), (1, 1.0), (2, 1.0), (3, 0.1), (3, 0.01)]:
        tag = f"dma k{k} d{d} mode{mode} slope{osl}"
        kw = dict(bias=bias, res=res, mrf=mrf if mode >= 2 else None, mrf_mode=mode, out_slope=osl, res_unact=10.0)
        out2, mrf2, guard2 = eng.dbg_conv1d_args(2, x, wp, lens, k, d, pad, cout, **kw)
        out1, mrf1, guard1 = eng.dbg_conv1d_args(1, x, wp, lens, k, d, pad, cout, **kw)
        assert guard2 == 0 and guard1 == 0, tag
        v = R.conv_ref(x, w16, lens, d, pad, bias=bias, res=res, res_unact=10.0, mrf=mrf, mrf_mode=mode)
        if mode in (0, 3):
            _check(out2, R.lrelu(v, osl), lens, tag)
            assert np.array_equal(out1, out2), tag + ": register-staged != LDS-DMA"
        if mode in (1, 2):
            _check(mrf2, v, lens, tag)
            assert np.array_equal(mrf1, mrf2), tag + ": register-staged != LDS-DMA"
        if mode == 3:
            assert np.array_equal(mrf2, mrf), tag + ": mode 3 only reads the running sum"
        (x0, res0, mrf0), l0 = _first([x, res, kw["mrf"]], lens)
        outa, mrfa, guarda = eng.dbg_conv1d_args(2, x0, wp, l0, k, d, pad, cout, **dict(kw, res=res0, mrf=mrf0))
        assert guarda == 0
        assert np.array_equal((outa if mode in (0, 3) else mrfa)[0], (out2 if mode in (0, 3) else mrf2)[0]), tag + ": not batch invariant"


def test_dma_conv_shaped_like_conv_pre(eng):
    """k = 7, identity input activation (z is stored as is), speaker conditioning through a permuted cond_row, no residual"""
    g = _gen(70)
    cin, cout, k, lens = 64, 128, 7, _lens(512)
    L = max(lens)
    x, w16, bias, cond = _h(_randn(g, 3, cin, L)), _h(_weight(g, cout, cin, k)), _randn(g, cout), _randn(g, 3, cout + 16)
    wp = Wt.pack_conv_f16(torch.from_numpy(w16)).numpy()
    kw = dict(bias=bias, cond=cond, out_slope=0.1)
    out2, _, guard2 = eng.dbg_conv1d_args(2, x, wp, lens, k, 1, 3, cout, cond_row=COND_ROW, **kw)
    out1, _, guard1 = eng.dbg_conv1d_args(1, x, wp, lens, k, 1, 3, cout, cond_row=COND_ROW, **kw)
    assert guard1 == 0 and guard2 == 0
    _check(out2, R.lrelu(R.conv_ref(x, w16, lens, 1, 3, bias=bias, cond=cond, cond_row=COND_ROW), 0.1), lens, "conv_pre")
    assert np.array_equal(out1, out2)
    outa, _, guarda = eng.dbg_conv1d_args(2, x[:1], wp, lens[:1], k, 1, 3, cout, cond_row=COND_ROW[:1], **kw)
    assert guarda == 0 and np.array_equal(outa[0], out2[0])


# ---- b. the four transposed convs: 4-wave LDS-DMA conv, k = 2 over the polyphase virtual channels, conv_epilogue_ups ----
@pytest.mark.parametrize("cin,cout,s,p", [(64, 32, 8, 4), (128, 64, 2, 1), (64, 32, 2, 1)])
def test_transposed_conv_into_activated_halves_against_float64(eng, cin, cout, s, p):
    g = _gen(cin, cout, s, 2)
    k, lens = 2 * s, _lens(256)
    L = max(lens)
    x, w16, bias, cond = _stream(g, 3, cin, L), _h(_randn(g, cin, cout, k) / np.float32((cin * k) ** 0.5)), _randn(g, cout), _randn(g, 3, cout + 16)
    wp = Wt.pack_conv_f16(Wt.polyphase_convT(torch.from_numpy(w16), s)).numpy()
    kw = dict(bias=bias, cond=cond, out_slope=0.1, ups_s=s, ups_p=p)
    out2, _, guard2 = eng.dbg_conv1d_args(2, x, wp, lens, 2, 1, 1, cout, cond_row=COND_ROW, **kw)
    out1, _, guard1 = eng.dbg_conv1d_args(1, x, wp, lens, 2, 1, 1, cout, cond_row=COND_ROW, **kw)
    assert guard1 == 0 and guard2 == 0
    ref = np.full(out2.shape, np.nan)
    for b, n in enumerate(lens):   # output lengths len * s: the t < 0 and t >= len_out vectors are dropped
        r = F.conv_transpose1d(torch.from_numpy(x[b:b + 1, :, :n]).double(), torch.from_numpy(w16).double(), torch.from_numpy(bias).double(),
                               stride=s, padding=p)[0].numpy()
        assert r.shape[1] == n * s
        ref[b, :, :n * s] = R.lrelu(r + cond[COND_ROW[b], :cout, None].astype(np.float64), 0.1)
    _check(out2, ref, [n * s for n in lens], f"convT {cin}->{cout} s{s}")
    assert np.array_equal(out1, out2), "register-staged != LDS-DMA"
    outa, _, guarda = eng.dbg_conv1d_args(2, x[:1], wp, lens[:1], 2, 1, 1, cout, cond_row=COND_ROW[:1], **kw)
    assert guarda == 0 and np.array_equal(outa[0], out2[0])


# ---- c. the fused ResBlock round (64- and 32-channel stages) = the two launches it replaces, tied to float64 through the GPU's h ----
@pytest.mark.parametrize("k,d", KD)
@pytest.mark.parametrize("C", [64, 32])
def test_fused_round_equals_its_two_launches_and_float64(eng, C, k, d):
    g = _gen(C, k, d, 3)
    nt2 = (128 if (C == 64 and k < 11) else 256) - (k - 1)
    lens = _lens(nt2)
    L, variant = max(lens), 2 if C == 64 else 1
    y, mrf = _stream(g, 3, C, L), _running_sum(g, lens, C)
    w1, w2, b1, b2 = _h(_weight(g, C, C, k)), _h(_weight(g, C, C, k)), _randn(g, C), _randn(g, C)
    wp1, wp2 = (Wt.pack_conv_f16(torch.from_numpy(w)).numpy() for w in (w1, w2))
    # conv1 -> h = fp16(lrelu(. + b1, 0.1)) in HBM, checked by the rule; everything after it is referred to THIS h
    h, _, guard = eng.dbg_conv1d_args(variant, y, wp1, lens, k, d, (k - 1) // 2 * d, C, bias=b1, out_slope=0.1)
    assert guard == 0
    _check(h, R.lrelu(R.conv_ref(y, w1, lens, d, (k - 1) // 2 * d, bias=b1), 0.1), lens, f"round C{C} k{k} d{d} conv1")
    for mode in range(4):
        tag = f"round C{C} k{k} d{d} mode{mode}"
        esl = 0.1 if C == 64 else 0.01   # the slope the stage's MRF mean is stored with (0.01 feeds conv_post)
        m_in = mrf if mode >= 2 else None
        out2, mrf2, guard = eng.dbg_conv1d_args(variant, h, wp2, lens, k, 1, (k - 1) // 2, C, bias=b2, res=y, res_unact=10.0, mrf=m_in,
                                                mrf_mode=mode, out_slope=esl if mode == 3 else 0.1)
        assert guard == 0, tag
        two = out2 if mode in (0, 3) else mrf2
        f_out, f_mrf, guard = eng.dbg_resblock_round_f16(y, wp1, wp2, b1, b2, lens, k, d, mrf_mode=mode, e_slope=esl, mrf=m_in)
        assert guard == 0, tag
        fused = f_out if mode in (0, 3) else f_mrf
        if mode == 3:
            assert np.array_equal(f_mrf, mrf) and np.array_equal(mrf2, mrf), tag + ": mode 3 only reads the running sum"
        assert np.array_equal(fused, two), tag + ": fused != conv1 then conv2"
        v = R.conv_ref(h, w2, lens, 1, (k - 1) // 2, bias=b2, res=y, res_unact=10.0, mrf=mrf, mrf_mode=mode)
        _check(fused, R.lrelu(v, 0.1 if mode == 0 else esl) if mode in (0, 3) else v, lens, tag)
        a_out, a_mrf, guard = eng.dbg_resblock_round_f16(y[:1], wp1, wp2, b1, b2, lens[:1], k, d, mrf_mode=mode, e_slope=esl,
                                                         mrf=None if m_in is None else m_in[:1])
        assert guard == 0 and np.array_equal((a_out if mode in (0, 3) else a_mrf)[0], fused[0]), tag + ": not batch invariant"


def test_fused_round_refuses_out_aliasing_its_input(eng):
    """neighbouring tiles read y's halo, so mode 0 may not write the stream in place"""
    g = _gen(4)
    y = _stream(g, 1, 32, 40)
    wp = Wt.pack_conv_f16(torch.from_numpy(_h(_weight(g, 32, 32, 3)))).numpy()
    b1, b2 = _randn(g, 32), _randn(g, 32)
    out, _, guard = eng.dbg_resblock_round_f16(y, wp, wp, b1, b2, [40], 3, 1, mrf_mode=0)   # the same call with an output of its own runs
    assert guard == 0 and (out != SENT).all()
    with pytest.raises(AurError, match="outputs of the mode"):
        eng.dbg_resblock_round_f16(y, wp, wp, b1, b2, [40], 3, 1, mrf_mode=0, out=y)


# ---- d. the fp32 kernel (the exact-mode vocoder): conditioning and the MRF modes ----
@pytest.mark.parametrize("k,d", [(3, 1), (7, 3), (11, 5)])
def test_fp32_conv_cond_and_mrf_modes_against_float64(eng, k, d):
    g = _gen(k, d, 5)
    cin, cout, lens = 32, 64, _lens(256)
    L, pad = max(lens), (k - 1) // 2 * d
    x, res, mrf = _randn(g, 3, cin, L), _randn(g, 3, cout, L), _running_sum(g, lens, cout)
    w, bias, cond = _weight(g, cout, cin, k), _randn(g, cout), _randn(g, 3, cout + 16)
    wp = Wt.pack_conv(torch.from_numpy(w)).numpy()
    for mode in range(4):
        tag = f"fp32 k{k} d{d} mode{mode}"
        kw = dict(slope=0.1, bias=bias, cond=cond, res=res, mrf_mode=mode)
        out, m, guard = eng.dbg_conv1d_args(0, x, wp, lens, k, d, pad, cout, cond_row=COND_ROW, mrf=mrf if mode >= 2 else None, **kw)
        assert guard == 0, tag
        v = R.conv_ref(x, w, lens, d, pad, slope=0.1, bias=bias, cond=cond, cond_row=COND_ROW, res=res, mrf=mrf, mrf_mode=mode)
        _check(out if mode in (0, 3) else m, v, lens, tag, half=False, rel=2e-5)
        if mode == 3:
            assert np.array_equal(m, mrf)
        outa, ma, guard = eng.dbg_conv1d_args(0, x[:1], wp, lens[:1], k, d, pad, cout, cond_row=COND_ROW[:1],
                                              mrf=mrf[:1] if mode >= 2 else None, **dict(kw, res=res[:1]))
        assert guard == 0 and np.array_equal((outa if mode in (0, 3) else ma)[0], (out if mode in (0, 3) else m)[0]), tag


# ---- e. interp2 ----
def test_interp2_both_forms(eng):
    g = _gen(6)
    n_lat, C, rows = [1, 2, 7, 31], 32, [4, 0, 5, 2]
    lat = _randn(g, 6, 31, C)
    frames = [R.frames_for(n) for n in n_lat]
    z, guard = eng.dbg_interp2(lat, rows, n_lat, max(frames))
    zh, guard_h = eng.dbg_interp2(lat, rows, n_lat, max(frames), out_f16=True)
    assert guard == 0 and guard_h == 0
    ref = R.interp2_ref(lat, rows, n_lat)
    for b, n in enumerate(frames):
        err = np.abs(z[b, :, :n] - ref[b]).max()
        print(f"interp2 n_lat={n_lat[b]} frames={n}: max err {err:.3e}")
        assert err <= 1e-6, (b, err)
        assert (z[b, :, n:] == SENT).all() and (zh[b, :, n:] == SENT).all()
        assert np.array_equal(zh[b, :, :n], _h(z[b, :, :n])), "halves form != fp16 of the fp32 form"
    za, guard = eng.dbg_interp2(lat, rows[:1], n_lat[:1], frames[0])
    zha, guard_h = eng.dbg_interp2(lat, rows[:1], n_lat[:1], frames[0], out_f16=True)
    assert guard == 0 and guard_h == 0
    assert np.array_equal(za[0], z[0, :, :frames[0]]) and np.array_equal(zha[0], zh[0, :, :frames[0]])


# ---- f. conv_post ----
@pytest.mark.parametrize("halves", [False, True])
def test_conv_post_against_float64(eng, halves):
    g = _gen(8, int(halves))
    cin, lens = 32, _lens(256)
    x = _stream(g, 3, cin, max(lens), slope=0.01) if halves else _randn(g, 3, cin, max(lens))
    w = _weight(g, 1, cin, 7)[0]
    wav, guard = eng.dbg_conv_post(x, w, lens, slope=0.01, x_f16_act=halves)
    assert guard == 0
    s, ref = R.conv_post_ref(x, w, lens, 1.0 if halves else 0.01)
    for b, n in enumerate(lens):
        err, bound = np.abs(wav[b, :n] - ref[b, :n]).max(), 2e-5 * max(1.0, np.abs(s[b, :n]).max())   # tanh does not expand errors
        print(f"conv_post halves={halves} b={b}: max err {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (b, err)
        assert (wav[b, n:] == SENT).all()
    wava, guard = eng.dbg_conv_post(x[:1], w, lens[:1], slope=0.01, x_f16_act=halves)
    assert guard == 0 and np.array_equal(wava[0], wav[0])
