"""The arithmetic ss.active.ftpPhase is measured against, in numpy: the demodulation of Fourier-transform profilometry as
the reference computes it (simplestereo/active.py:675-737 -- gray by channel maximum, np.fft.fft along x, the band mask on
np.fft.fftfreq, np.fft.ifft, np.angle of ghat * conj(g0hat)), plus an extended-precision direct evaluation of the same
band-limited sums that serves as the truth of tests/golden/ftp_cases.*."""
import numpy as np

LD = np.longdouble


def gray(img):
    """[H, W] stays; [H, W, 3] is reduced by the channel maximum."""
    img = np.asarray(img)
    return img if img.ndim == 2 else img.max(axis=2)


def band(fc, radius_factor, h):
    """fmin[h], fmax[h] of the pass band, in fp64."""
    f = np.broadcast_to(np.asarray(fc, dtype=np.float64), (h,)).copy()
    with np.errstate(all="ignore"):
        radius = radius_factor * f
        return f - radius, f + radius


def signed_bins(w):
    """Signed bin index of every position of an np.fft.fft output of length w (the integers fftfreq scales by 1/w)."""
    return np.concatenate([np.arange(0, (w - 1) // 2 + 1), np.arange(-(w // 2), 0)]).astype(np.int64)


def keep_mask(w, fmin, fmax):
    """[h, w] bool in fft order: True where the reference leaves the bin alone."""
    freqs = np.fft.fftfreq(w)
    with np.errstate(all="ignore"):
        low = (freqs.reshape(1, -1) - np.asarray(fmin, dtype=np.float64).reshape(-1, 1)) < 0
        high = (freqs.reshape(1, -1) - np.asarray(fmax, dtype=np.float64).reshape(-1, 1)) > 0
    return ~low & ~high


def band_ranges(w, fmin, fmax):
    """(slo[h], shi[h]) of the kept bins per row from the numpy mask; (0, -1) for an empty row.  Asserts contiguity."""
    k = keep_mask(w, fmin, fmax)
    s = signed_bins(w)
    order = np.argsort(s)
    lo = np.zeros(k.shape[0], dtype=np.int64)
    hi = -np.ones(k.shape[0], dtype=np.int64)
    for y in range(k.shape[0]):
        kept = s[order][k[y][order]]
        if kept.size:
            assert kept[-1] - kept[0] + 1 == kept.size
            lo[y], hi[y] = kept[0], kept[-1]
    return lo, hi


def ftp_phase_numpy(img_obj, img_ref, fc, radius_factor):
    """The wrapped phase the numpy way."""
    g, g0 = gray(img_obj), gray(img_ref)
    h, w = g.shape
    fmin, fmax = band(fc, radius_factor, h)
    cut = ~keep_mask(w, fmin, fmax)
    G = np.fft.fft(g, axis=1)
    G0 = np.fft.fft(g0, axis=1)
    G[cut] = 0
    G0[cut] = 0
    ghat = np.fft.ifft(G, axis=1)
    g0hat = np.fft.ifft(G0, axis=1)
    return np.angle(ghat * np.conjugate(g0hat))


def wrap_err(a, b):
    """|a - b| as an angle: the distance on the circle, exact for small differences."""
    d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    return np.abs(np.arctan2(np.sin(d), np.cos(d)))


def truth_longdouble(img_obj, img_ref, fc, radius_factor):
    """(phase fp64 [h, w], ratio fp64 [h, w]): the band-limited sums evaluated directly in np.longdouble and rounded once;
    ratio = |z| over its row's maximum (1 on rows with an empty band, whose phase is 0)."""
    g, g0 = gray(img_obj).astype(LD), gray(img_ref).astype(LD)
    h, w = g.shape
    fmin, fmax = band(fc, radius_factor, h)
    lo, hi = band_ranges(w, fmin, fmax)
    two_pi = LD(8) * np.arctan(LD(1))
    x = np.arange(w, dtype=np.int64)
    phase = np.zeros((h, w), dtype=np.float64)
    ratio = np.ones((h, w), dtype=np.float64)
    for y in range(h):
        if hi[y] < lo[y]:
            continue
        s = np.arange(lo[y], hi[y] + 1, dtype=np.int64)
        ang = two_pi * (np.outer(s, x) % w).astype(LD) / LD(w)           # [K, w], the angle reduced exactly
        c, sn = np.cos(ang), np.sin(ang)

        def back_and_forth(row):
            gr, gi = c @ row, -(sn @ row)                                # G[s]
            return gr @ c - gi @ sn, gr @ sn + gi @ c                    # ghat[x] (times w)
        ar, ai = back_and_forth(g[y])
        br, bi = back_and_forth(g0[y])
        zr, zi = ar * br + ai * bi, ai * br - ar * bi
        phase[y] = np.arctan2(zi, zr).astype(np.float64)
        mod = np.hypot(zr, zi)
        ratio[y] = (mod / mod.max()).astype(np.float64)
    return phase, ratio
