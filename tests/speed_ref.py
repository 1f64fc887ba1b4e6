"""Float64 reference of the speed stretch (aur_seq_desc.speed) in front of the vocoder's two interpolations: the three-stage form of
vocoder_ref.interp2_ref, with the same float32 index model.  One definition of the semantics for the CPU and the GPU tests:

    ls  = 1.0 / float64(float32(speed))            (0 = unset = 1.0; the float that crosses the ABI, widened to double)
    L0' = max(1, floor(n_lat * ls))                (rows after the stretch; the max covers n_lat = 1 at speed > 1, where torch raises)
    r0  = float32(1.0 / ls)                        (the scale torch hands its kernel: float(1 / scale_factor))
    stage 0: lin_src(r0, s, n_lat) for s < L0', a copy when L0' == n_lat; stages 1 and 2 as interp2_ref on L0' rows
    samples = 256 * frames_for(L0')

lin_src here is vocoder_ref.lin_src with ONE rounding of the source position, src = fl32(r * (j + 0.5) - 0.5): what torch's float32
CPU kernel and the HIP kernels compute (both contract the product and the subtraction into an fma; the kernels' ISA shows
v_fma_f32 src, r, j + 0.5, -0.5).  vocoder_ref.lin_src rounds the product first; the two stay within ~2e-7 of each other up to ~130
positions, the lengths interp2_ref is tested at, and then differ by an ulp of the position (1.5e-5 of the weight near position 250,
5.6e-6 of the value at 64 rows), which is past the 1e-6 this reference is held to against torch at 557 positions.  The product of a float32
scale and j + 0.5 is exact in float64, so the float64 expression below, rounded once, is that fma."""
import numpy as np

from tests.vocoder_ref import R1, R2, frames_for, lerp

N_LATS = (1, 2, 3, 7, 31, 64)
SPEEDS = (0.5, 0.75, 0.8, 1.0, 1.25, 2.0)
PAIRS = [(n, s) for n in N_LATS for s in SPEEDS]


def lin_src(r, j, L):
    """source rows and weight of F.interpolate(mode="linear", align_corners=False) in float32, the source position rounded once:
    src = max(fl32(r * (j + 0.5) - 0.5), 0); i0 = floor(src); i1 = min(i0 + 1, L - 1); lam = src - i0"""
    j = np.asarray(j).astype(np.float64)
    src = np.maximum((np.float64(np.float32(r)) * (j + 0.5) - 0.5).astype(np.float32), np.float32(0.0))
    i0 = np.floor(src).astype(np.int64)
    i1 = np.minimum(i0 + 1, L - 1)
    return i0, i1, (src - i0.astype(np.float32)).astype(np.float32)


def length_scale(speed):
    sp = float(np.float32(speed))
    return 1.0 if sp == 0.0 else 1.0 / sp


def stretched_rows(n_lat, speed):
    return max(1, int(np.floor(float(n_lat) * length_scale(speed))))


def samples_for(n_lat, speed):
    return 256 * frames_for(stretched_rows(n_lat, speed))


def interp3_ref(lat, lat_row, n_lat, speed):
    """z[b] = interp(interp(interp(lat[lat_row[b]][:n_lat[b]]^T, x 1/speed[b]), x4), x24000/22050): a list of float64
    [C][frames_for(L0'_b)].  Indices and weights in float32, blends in float64, innermost stage first."""
    lat = np.asarray(lat, dtype=np.float64)
    out = []
    for b, n in enumerate(n_lat):
        x = lat[b if lat_row is None else int(lat_row[b]), :n].T          # [C][n]
        l0 = stretched_rows(n, speed[b])
        r0 = np.float32(1.0 / length_scale(speed[b]))

        def stage0(s):
            if l0 == n:   # torch copies when an interpolation leaves the length unchanged, whatever the scale
                return x[:, s]
            k0, k1, lam0 = lin_src(r0, s, n)
            return lerp(x[:, k0], x[:, k1], lam0)
        i0, i1, lam2 = lin_src(R2, np.arange(frames_for(l0)), 4 * l0)
        if frames_for(l0) == 4 * l0:
            i0 = i1 = np.arange(4 * l0)
            lam2 = np.zeros(4 * l0, dtype=np.float32)
        ys = []
        for idx in (i0, i1):
            s0, s1, lam1 = lin_src(R1, idx, l0)
            ys.append(lerp(stage0(s0), stage0(s1), lam1))
        out.append(lerp(ys[0], ys[1], lam2))
    return out


def torch_stretch(lat_rows, speed):
    """The stretch alone with torch, float64: lat_rows [n][C] -> [L0'][C].  n = 1 at speed > 1 (torch raises): the row is copied."""
    import torch
    import torch.nn.functional as F
    x = torch.as_tensor(np.asarray(lat_rows), dtype=torch.float64)
    ls = length_scale(speed)
    if int(np.floor(x.shape[0] * ls)) < 1:
        return x.clone()
    return F.interpolate(x.T[None], scale_factor=ls, mode="linear", align_corners=False)[0].T.contiguous()
