"""The fp64 numpy restatement of the bias field correction (--prep_bias n4), written from the rule."""
import math

import numpy as np

BINS, LEVELS, PAD = 200, 4, 512


def samples(extent):
    """The sampled full-grid indices of an axis: stride 4 from 2, or every index when that gives fewer than 8."""
    x = np.arange(2, extent, 4)
    return x if len(x) >= 8 else np.arange(extent)


def dense_weights(extent, level, index):
    """len(index) x (n + 3): row i holds the four cubic B-spline basis values of index[i] at its span, zeros elsewhere."""
    n = 2 ** level
    t = (np.asarray(index, dtype=np.float64) + 0.5) / extent * n
    k = np.floor(t).astype(int)
    a = t - k
    basis = [(1 - a) ** 3 / 6, (3 * a ** 3 - 6 * a ** 2 + 4) / 6, (-3 * a ** 3 + 3 * a ** 2 + 3 * a + 1) / 6, a ** 3 / 6]
    out = np.zeros((len(k), n + 3))
    for j, b in enumerate(basis):
        out[np.arange(len(k)), k + j] = b
    return out


def log_mask(v):
    m = np.isfinite(v) & (v > 0)
    return np.where(m, np.log(np.where(m, v, 1).astype(np.float64)), 0).astype(np.float32), m


def position(r, lo, hi):
    """(k, a): r lies between bin centres k and k + 1 at fraction a; fp64 from the fp32 r, lo and hi."""
    t = (r.astype(np.float64) - np.float64(lo)) * (199.0 / (np.float64(hi) - np.float64(lo)))
    k = np.clip(np.floor(t).astype(np.int64), 0, BINS - 2)
    return k, np.clip(t - k, 0.0, 1.0)


def histogram(r):
    """(counters in units of 1 / 65536, lo, hi) of the fp32 values r."""
    lo, hi = np.float32(r.min()), np.float32(r.max())
    h = np.zeros(BINS, dtype=np.int64)
    if hi > lo:
        k, a = position(r, lo, hi)
        q = np.floor(a * 65536.0 + 0.5).astype(np.int64)
        np.add.at(h, k, 65536 - q)
        np.add.at(h, k + 1, q)
    return h, float(lo), float(hi)


def sharpen(h, lo, hi):
    slope, at = (hi - lo) / (BINS - 1), (PAD - BINS) // 2
    v = np.zeros(PAD)
    v[at:at + BINS] = h
    sigma = 0.15 / slope / (2 * math.sqrt(2 * math.log(2)))            # the Gaussian of FWHM 0.15, in bins
    i = np.minimum(np.arange(PAD), PAD - np.arange(PAD)).astype(np.float64)
    ff = np.fft.fft(np.exp(-i ** 2 / (2 * sigma ** 2)) / (sigma * math.sqrt(2 * math.pi)))
    u = np.maximum(np.fft.ifft(np.fft.fft(v) * np.conj(ff) / (np.abs(ff) ** 2 + 0.01)).real, 0)
    centre = lo + (np.arange(PAD) - at) * slope
    den = np.fft.ifft(np.fft.fft(u) * ff).real
    num = np.fft.ifft(np.fft.fft(u * centre) * ff).real
    return np.where(den != 0, num / np.where(den != 0, den, 1), 0)[at:at + BINS]


def lattice(e, m, axes):
    """phi of the residual e over the samples m; axes: per axis the dense weights of its samples.  S separates."""
    cube = [w ** 3 / (w ** 2).sum(1, keepdims=True) for w in axes]
    delta = np.einsum("dhw,da,hb,wc->abc", np.where(m, e, 0.0), *cube)
    omega = np.einsum("dhw,da,hb,wc->abc", m.astype(np.float64), *[w ** 2 for w in axes])
    return np.where(omega != 0, delta / np.where(omega != 0, omega, 1), 0.0)


def evaluate(phi, axes):
    return np.einsum("abc,da,hb,wc->dhw", phi, *axes)


def fit_step(u_s, f_s, m_s, table, lo, hi, axes):
    """One iteration from the sampled fp32 u and f: (e, phi, df, sum exp(df), sum exp(df)^2 over m), all fp64."""
    r = u_s - f_s                                            # fp32, as the rule has it
    k, a = position(r, lo, hi)
    e = r.astype(np.float64) - (table[k] * (1.0 - a) + table[k + 1] * a)
    phi = lattice(e, m_s, axes)
    df = evaluate(phi, axes)
    x = np.exp(df[m_s])
    return e, phi, df, x.sum(), (x * x).sum()


def correct(v):
    """(corrected fp32 volume, iterations per level, exp(f) on the full grid) of the fp32 volume v."""
    u, m = log_mask(v)
    idx = [samples(n) for n in v.shape]
    grid = np.ix_(*idx)
    u_s, m_s, f_s = u[grid], m[grid], np.zeros([len(i) for i in idx], dtype=np.float32)
    field, iters = np.zeros(v.shape), []
    for level in range(LEVELS):
        axes = [dense_weights(n, level, i) for n, i in zip(v.shape, idx)]
        total, done = 0.0, 0
        while done < 50:
            h, lo, hi = histogram((u_s - f_s)[m_s])
            if not hi > lo:
                break
            _, phi, df, s1, s2 = fit_step(u_s, f_s, m_s, sharpen(h / 65536.0, lo, hi), lo, hi, axes)
            total, done = total + phi, done + 1
            f_s = f_s + df.astype(np.float32)
            n = int(m_s.sum())
            if math.sqrt(max(s2 / n - (s1 / n) ** 2, 0.0)) / (s1 / n) < 0.001:
                break
        iters.append(done)
        field = field + evaluate(total, [dense_weights(n, level, np.arange(n)) for n in v.shape])
    return (v.astype(np.float64) / np.exp(field)).astype(np.float32), iters, np.exp(field)


def phantom(shape=(48, 40, 36), seed=3):
    """(scan, truth field, tissue labels): three piecewise-constant tissues in background 0 under a quadratic field."""
    z = np.stack(np.meshgrid(*[np.linspace(-1, 1, n) for n in shape], indexing="ij"))
    rad = np.sqrt((z ** 2).sum(0))
    tissue = np.where(rad < 0.6, 3, np.where(rad < 1.0, 2, np.where(rad < 1.5, 1, 0)))
    rng = np.random.default_rng(seed)
    clean = np.array([0.0, 300.0, 600.0, 900.0])[tissue] * (1 + 0.01 * rng.standard_normal(shape))
    field = np.exp(0.2 * (0.6 * z[0] - 0.5 * z[1] * z[2] + 0.7 * z[2] ** 2 - 0.4 * z[0] ** 2))
    return (clean * field).astype(np.float32), field, tissue

