"""CPU: the float64 reference of the output sample rate (tests/resample_ref.py) pinned to the project's statement of torchaudio's
algorithm (auralis_amd/conditioning.py: resample, fp32 torch), the length rule, the kept-tap counts, and a tone."""
import numpy as np
import pytest
import torch

from auralis_amd.conditioning import resample
from tests import resample_ref as RR

LENGTHS = (1, 2, 255, 700)


@pytest.mark.parametrize("rate", RR.RATES)
def test_ref_matches_conditioning_resample(rate):
    """Equal lengths; |fp32 torch - ref64| within the dot-product bound taken with the DENSE tap count (torch's conv1d runs over
    every tap of the phase, in whatever order)."""
    gen = torch.Generator().manual_seed(1000 + rate)
    worst = 0.0
    for n in LENGTHS:
        x = torch.randn(n, generator=gen)
        got = resample(x[None], RR.ORIG_RATE, rate)[0].numpy()
        ref, absdot = RR.resample_ref(x.numpy(), rate)
        assert got.shape == ref.shape == (RR.n_out(n, rate),), (rate, n)
        tol = RR.bound(absdot, RR.dense_taps(rate))
        err = np.abs(got - ref)
        assert (err <= tol).all(), (rate, n, float((err / np.maximum(tol, 1e-300)).max()))
        worst = max(worst, float((err / np.maximum(tol, 1e-300)).max()))
    print(f"rate {rate}: conditioning.resample (fp32) vs ref64, max err / bound {worst:.3f}")


def test_length_rule_and_identity():
    assert [RR.n_out(700, r) for r in RR.RATES] == [234, 467, 644, 934, 1287, 1400]
    assert RR.n_out(1, 8000) == 1 and RR.n_out(3, 8000) == 1 and RR.n_out(4, 8000) == 2
    assert RR.n_out(255, 0) == RR.n_out(255, 24000) == 255
    x = np.linspace(-1, 1, 17)
    y, a = RR.resample_ref(x, 24000)
    assert np.array_equal(y, x) and np.array_equal(a, np.abs(x))


@pytest.mark.parametrize("rate", RR.RATES)
def test_kept_taps_are_the_nonzero_run_in_fp32(rate):
    """The clamped region (|t| = 6) is exactly zero once rounded to fp32; what is left of a phase is one run of at most KEPT_TAPS."""
    c = RR.dense_kernel(rate)[0].astype(np.float32)
    runs = []
    for row in c:
        nz = np.flatnonzero(row)
        assert len(nz), rate
        runs.append(nz[-1] - nz[0] + 1)
    assert max(runs) == RR.KEPT_TAPS[rate], (rate, max(runs))
    assert c.shape[0] * max(runs) <= 147 * 14


@pytest.mark.parametrize("rate", RR.RATES)
def test_a_1khz_tone_stays_a_1khz_tone(rate):
    """0.1 s of a 1 kHz sine: away from the ends (6 zero crossings of the filter at the lower rate, taken as 5 ms) the output is the
    same sine sampled at the new rate.  1 kHz is at most a quarter of the narrowest pass band (0.99 * 4 kHz), where the Hann-windowed
    sinc of width 6 is flat to well under 1 %: gain within 1 %, residual below 1 % of the amplitude."""
    n = 2400
    x = np.sin(2 * np.pi * 1000.0 * np.arange(n) / RR.ORIG_RATE)
    y, _ = RR.resample_ref(x, rate)
    m = np.arange(len(y))
    keep = (m > 0.005 * rate) & (m < len(y) - 0.005 * rate)
    basis = np.stack([np.sin(2 * np.pi * 1000.0 * m / rate), np.cos(2 * np.pi * 1000.0 * m / rate)], axis=1)
    coef, *_ = np.linalg.lstsq(basis[keep], y[keep], rcond=None)
    resid = y[keep] - basis[keep] @ coef
    amp = float(np.hypot(*coef))
    print(f"rate {rate}: amplitude {amp:.5f}, phase term {coef[1]:+.2e}, residual rms {np.sqrt(np.mean(resid ** 2)):.2e}")
    assert abs(amp - 1.0) <= 0.01 and abs(coef[1]) <= 0.01
    assert np.sqrt(np.mean(resid ** 2)) <= 0.01
    spec = np.abs(np.fft.rfft(y[keep] * np.hanning(keep.sum())))
    peak_hz = np.argmax(spec) * rate / keep.sum()
    assert abs(peak_hz - 1000.0) <= rate / keep.sum()          # the strongest bin is the one that holds 1 kHz
