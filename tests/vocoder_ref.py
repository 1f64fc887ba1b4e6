"""Float64 restatement of the vocoder kernels' contracts (auralis_amd/csrc/vocoder_kernels.h), one operation at a time, for the per-kernel
tests: the masked conv of ConvArgs with its epilogue, one fused ResBlock round, the two chained interpolations and conv_post.
Plain numpy on [B][C][L] arrays; positions an utterance does not own come back as NaN.  tests/test_vocoder_ref.py holds these
against torch's own convolutions and the oracle on the CPU; tests/test_gpu_vocoder_kernels.py holds the kernels against them."""
import numpy as np


def lrelu(v, slope):
    v = np.asarray(v, dtype=np.float64)
    return np.where(v > 0, v, v * slope)


def ulp16(v):
    """spacing of fp16 at |v|: 2^(floor(log2 |v|) - 10), 2^-24 over the subnormals and zero"""
    a = np.abs(np.asarray(v, dtype=np.float64))
    _, e = np.frexp(np.maximum(a, 2.0 ** -14))   # a = m * 2^e, 0.5 <= m < 1
    return np.ldexp(1.0, e - 11)


def unact(y, res_unact):
    """the residual read back from the activated stream: y < 0 ? y * res_unact : y"""
    y = np.asarray(y, dtype=np.float64)
    return np.where(y < 0, y * res_unact, y)


def conv_ref(x, w, lens, dil, padl, slope=1.0, bias=None, cond=None, cond_row=None, res=None, res_unact=None, mrf=None, mrf_mode=0,
             ups_s=0, ups_p=0):
    """ConvArgs: the value the epilogue holds before its store, float64 [B][Cout][L * max(1, ups_s)].
         y[b][v][q] = sum_{ci, j} w[v][ci][j] * lrelu(x[b][ci][q + j * dil - padl], slope),   x == 0 outside [0, lens[b])
       plain conv: co = v, t = q, q < len; polyphase transposed conv (stride ups_s, padding ups_p): v = co * s + r lands at
       t = q * s + r - p for q <= len, kept where 0 <= t < len * s.  Then + bias[co] + cond[cond_row[b]][co] + the residual (res as is,
       or un-activated when res_unact is given), and the MRF fold: mode 1 v, mode 2 mrf + v, mode 3 (mrf + v) / 3.
       w is the virtual weight [Mtot][Cin][k]; pass slope = 1 for a stream that is stored activated."""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    B, cin, L = x.shape
    mtot, cin_w, k = w.shape
    assert cin == cin_w
    s = max(1, ups_s)
    cout = mtot // s
    out = np.full((B, cout, L * s), np.nan)
    for b in range(B):
        n = int(lens[b])
        n_q = n + 1 if ups_s else n
        xp = np.zeros((cin, padl + n_q + (k - 1) * dil + 1))
        xp[:, padl:padl + n] = lrelu(x[b, :, :n], slope)
        y = np.zeros((mtot, n_q))
        for j in range(k):
            y += w[:, :, j] @ xp[:, j * dil:j * dil + n_q]
        if ups_s:
            v = np.zeros((cout, n * s))
            for r in range(s):
                t = np.arange(n_q) * s + r - ups_p
                ok = (t >= 0) & (t < n * s)
                v[:, t[ok]] = y[r::s][:, ok]
        else:
            v = y
        if bias is not None:
            v = v + np.asarray(bias, dtype=np.float64)[:, None]
        if cond is not None:
            v = v + np.asarray(cond, dtype=np.float64)[int(cond_row[b]), :cout, None]
        if res is not None:
            r_ = np.asarray(res[b, :, :n * s], dtype=np.float64)
            v = v + (r_ if res_unact is None else unact(r_, res_unact))
        if mrf_mode >= 2:
            v = v + np.asarray(mrf[b, :, :n * s], dtype=np.float64)
        if mrf_mode == 3:
            v = v / 3.0
        out[b, :, :n * s] = v
    return out


def round_ref(y, w1, b1, w2, b2, lens, dil):
    """One ResBlock round on the activated stream y = lrelu(x, 0.1) (RoundArgs) without the fp16 rounding of h:
    h = lrelu(conv1(y) + b1, 0.1), zero outside the utterance (conv2 pads the conv1 OUTPUT); v = x + conv2(h) + b2 with x = y
    un-activated.  Returns (h, v).  (The GPU test takes conv2's reference from the GPU's own rounded h instead: conv_ref on it.)"""
    k = np.asarray(w1).shape[2]
    h = np.nan_to_num(lrelu(conv_ref(y, w1, lens, dil, (k - 1) // 2 * dil, bias=b1), 0.1), nan=0.0)
    v = conv_ref(h, w2, lens, 1, (k - 1) // 2, bias=b2, res=y, res_unact=10.0)
    return h, v


R1 = np.float32(1.0 / (1024.0 / 256.0))
R2 = np.float32(1.0 / (24000.0 / 22050.0))


def lin_src(r, j, L):
    """source rows and weight of F.interpolate(mode="linear", align_corners=False), float32 as the kernel's lin_src:
    src = max(r * (j + 0.5) - 0.5, 0); i0 = floor(src); i1 = min(i0 + 1, L - 1); lam = src - i0"""
    j = np.asarray(j).astype(np.float32)
    src = np.maximum(np.float32(r) * (j + np.float32(0.5)) - np.float32(0.5), np.float32(0.0)).astype(np.float32)
    i0 = np.floor(src).astype(np.int64)
    i1 = np.minimum(i0 + 1, L - 1)
    return i0, i1, (src - i0.astype(np.float32)).astype(np.float32)


def lerp(a, b, lam):
    lam = lam.astype(np.float64)
    return (1.0 - lam) * a + lam * b


def frames_for(n_lat):
    return int(np.floor(float(4 * n_lat) * (24000.0 / 22050.0)))


def interp2_ref(lat, lat_row, n_lat):
    """z[b] = interp(interp(lat[lat_row[b]][:n_lat[b]]^T, x4), x24000/22050): a list of float64 [C][frames_for(n_lat[b])].  Indices and
    weights in float32, blends in float64.  (The first interpolation never keeps the length; the second does for n_lat <= 2.)"""
    lat = np.asarray(lat, dtype=np.float64)
    out = []
    for b, n in enumerate(n_lat):
        x = lat[b if lat_row is None else int(lat_row[b]), :n].T          # [C][n]
        i0, i1, lam2 = lin_src(R2, np.arange(frames_for(n)), 4 * n)
        if frames_for(n) == 4 * n:   # n <= 2: torch copies when an interpolation leaves the length unchanged, whatever the scale
            i0 = i1 = np.arange(4 * n)
            lam2 = np.zeros(4 * n, dtype=np.float32)
        ys = []
        for idx in (i0, i1):
            k0, k1, lam1 = lin_src(R1, idx, n)
            ys.append(lerp(x[:, k0], x[:, k1], lam1))
        out.append(lerp(ys[0], ys[1], lam2))
    return out


def conv_post_ref(x, w, lens, slope):
    """(pre-tanh sum, wav): s[b][t] = sum_{ci, j} w[ci][j] * lrelu(x[b][ci][t + j - 3], slope), wav = tanh(s); slope = 1 for the
    activated halves form"""
    s = conv_ref(x, np.asarray(w, dtype=np.float64)[None], lens, 1, 3, slope=slope)[:, 0]
    return s, np.tanh(s)
