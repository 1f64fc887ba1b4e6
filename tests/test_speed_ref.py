"""CPU: the three-stage interpolation reference (tests/speed_ref.py) against three chained torch interpolations, compared in
float64, and the length rule of aur_seq_desc.speed: samples = 256 * frames_for(max(1, floor(n_lat * ls))), ls = 1 / float32(speed).

torch runs on float32 latents, as in test_vocoder_ref.py and as XTTS itself does: its index arithmetic follows the tensor's dtype,
and that float32 arithmetic is what lin_src models and the kernel computes.  (On float64 tensors torch takes the source positions
in double; a float32 position near 250 is 1.5e-5 off, so the float32 index model sits 3.8e-6 from that chain at (31, 0.5) -- the
model's own distance from exact positions, not an error of the blends.)"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import speed_ref as S
from tests import vocoder_ref as R

# (n_lat, speed) -> rows after the stretch, worked out by hand from the rule: floor(n / speed) in double on the float32 speed.
# float32(0.8) = 0.800000011920929 > 0.8, so n / 0.8 lands just below n * 1.25: 64 -> 79, not 80.  The other five speeds are exact
# in float32.  (1, 1.25) and (1, 2.0) floor to 0 rows and are clamped to 1.
ROWS = {
    (1, 0.5): 2, (1, 0.75): 1, (1, 0.8): 1, (1, 1.0): 1, (1, 1.25): 1, (1, 2.0): 1,
    (2, 0.5): 4, (2, 0.75): 2, (2, 0.8): 2, (2, 1.0): 2, (2, 1.25): 1, (2, 2.0): 1,
    (3, 0.5): 6, (3, 0.75): 4, (3, 0.8): 3, (3, 1.0): 3, (3, 1.25): 2, (3, 2.0): 1,
    (7, 0.5): 14, (7, 0.75): 9, (7, 0.8): 8, (7, 1.0): 7, (7, 1.25): 5, (7, 2.0): 3,
    (31, 0.5): 62, (31, 0.75): 41, (31, 0.8): 38, (31, 1.0): 31, (31, 1.25): 24, (31, 2.0): 15,
    (64, 0.5): 128, (64, 0.75): 85, (64, 0.8): 79, (64, 1.0): 64, (64, 1.25): 51, (64, 2.0): 32,
}


def test_lengths_of_all_pairs():
    assert sorted(ROWS) == sorted(S.PAIRS) and len(S.PAIRS) == 36
    for (n, sp), rows in ROWS.items():
        assert S.stretched_rows(n, sp) == rows, (n, sp)
        assert S.samples_for(n, sp) == 256 * int(np.floor(4 * rows * 24000.0 / 22050.0)), (n, sp)
    assert S.stretched_rows(1, 2.0) == 1            # the clamp: floor(0.5) = 0 rows, torch raises, the row is copied
    assert S.stretched_rows(3, 0.8) == 3            # floor(3.75): the length is kept, a copy
    assert S.samples_for(64, 0.5) == 256 * 557      # crosses two 256-position blocks of the kernel
    assert S.stretched_rows(7, 0.0) == 7 and S.samples_for(7, 0.0) == 256 * R.frames_for(7)   # 0 = unset


def test_binding_sizes_its_buffers_by_the_same_rule():
    from auralis_amd import _lib
    for n, sp in S.PAIRS + [(605, 0.5), (605, 2.0), (280, 0.0)]:
        assert _lib.stretched_rows(n, sp) == S.stretched_rows(n, sp) and _lib.samples_for(n, sp) == S.samples_for(n, sp), (n, sp)


def test_torch_raises_where_the_clamp_applies():
    with pytest.raises(RuntimeError):
        F.interpolate(torch.zeros(1, 4, 1), scale_factor=S.length_scale(2.0), mode="linear")


@pytest.fixture(scope="module")
def lat():
    return torch.randn(3, 64, 8, generator=torch.Generator().manual_seed(11))


def test_interp3_reference_equals_three_chained_torch_interpolations(lat):
    """every pair where torch does not raise; the bound test_vocoder_ref.py holds interp2_ref to"""
    raised = []
    for i, (n, sp) in enumerate(S.PAIRS):
        row = i % 3
        got = S.interp3_ref(lat.numpy(), [row], [n], [sp])[0]
        x = lat[row, :n].T[None]
        try:
            z = F.interpolate(x, scale_factor=S.length_scale(sp), mode="linear", align_corners=False)
        except RuntimeError:
            raised.append((n, sp))
            continue
        assert z.shape[-1] == S.stretched_rows(n, sp), (n, sp)
        z = F.interpolate(z, scale_factor=4.0, mode="linear", align_corners=False)
        z = F.interpolate(z, scale_factor=24000 / 22050, mode="linear", align_corners=False)[0]
        assert got.shape == tuple(z.shape) == (8, R.frames_for(S.stretched_rows(n, sp))), (n, sp)
        assert np.abs(got - z.double().numpy()).max() < 1e-6, (n, sp)
    assert raised == [(1, 1.25), (1, 2.0)]   # floor(1 / speed) = 0 rows: the clamp's cases


def test_interp3_reference_special_rows(lat):
    a = lat.numpy()
    # a stretch that keeps the length is a copy: interp2_ref's values, whatever the scale ((3, 0.8), speed 1, unset) -- to the
    # difference between the once- and the twice-rounded source positions of the two modules, inside interp2_ref's own bound here
    for n, sp in ((3, 0.8), (7, 1.0), (31, 0.0), (1, 0.75)):
        assert np.abs(S.interp3_ref(a, [1], [n], [sp])[0] - R.interp2_ref(a, [1], [n])[0]).max() < 1e-6, (n, sp)
    # ... and exactly the same thing as speed 1, at any length
    for n, sp in ((3, 0.8), (64, 0.0), (1, 0.75)):
        assert np.array_equal(S.interp3_ref(a, [1], [n], [sp])[0], S.interp3_ref(a, [1], [n], [1.0])[0])
    # the clamp copies the single row: every position holds it (to the rounding of (1 - lam) a + lam a, as interp2_ref at n_lat = 1)
    z = S.interp3_ref(a, [2], [1], [2.0])[0]
    assert z.shape == (8, 4) and np.allclose(z, np.repeat(a[2, 0].astype(np.float64)[:, None], 4, axis=1), rtol=1e-15, atol=0)
    # (1, 0.5): two rows, both the single latent row
    assert S.interp3_ref(a, [0], [1], [0.5])[0].shape == (8, R.frames_for(2))
    # the stretch alone, as the GPU tests pre-stretch latents for the oracle
    for n, sp in ((7, 2.0), (31, 0.75), (1, 2.0), (3, 0.8)):
        assert tuple(S.torch_stretch(a[0, :n], sp).shape) == (S.stretched_rows(n, sp), 8)
