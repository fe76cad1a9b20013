"""The float64 numpy restatement of the gradient-descent exit-wave and aberration fit (emdenoise.psiart; include/emdenoise.h "Exit
wave and aberrations by gradient descent"), written from psi-art.py:97-130 (the grid), :170-223 and :293-297 (the CTF), :298-313 (the
model and the loss), :304 (the optimiser) and :334-348 (the bootstrapping window), and independent of the library.  The reference
does not run as committed and TensorFlow is not run: the formulas of the header are the specification, and tests/test_psiart.py
checks the hand-written reverse pass below against torch's autograd on the CPU.

Two evaluations of the same formulas give the yardstick of the device tests: ``fft=NumpyFFT, ctf_dtype=float64`` (as written) and
``fft=Radix2FFT, ctf_dtype=longdouble`` (chi, T and the basis functions in extended precision, rounded to float64)."""
import functools

import numpy as np

from tests.exitwave_ref import NumpyFFT, Radix2FFT, rel_l2, true_wave   # noqa: F401  (re-exported for the tests)

SYMBOLS = ("a22", "phi22", "a20", "a33", "phi33", "a31", "phi31", "a44", "phi44", "a42", "phi42", "a40", "a55", "phi55", "a53", "phi53",
           "a51", "phi51", "a66", "phi66", "a64", "phi64", "a62", "phi62", "a60")
NPARAM = 27
I_A20, I_SPREAD, I_OFFSET = 2, 25, 26
# (order n, multiplicity m, index of the amplitude, index of the azimuth or None): the terms of get_chi
TERMS = ((2, 2, 0, 1), (2, 0, 2, None), (3, 3, 3, 4), (3, 1, 5, 6), (4, 4, 7, 8), (4, 2, 9, 10), (4, 0, 11, None), (5, 5, 12, 13),
         (5, 3, 14, 15), (5, 1, 16, 17), (6, 6, 18, 19), (6, 4, 20, 21), (6, 2, 22, 23), (6, 0, 24, None))


def energy2wavelength(v0):
    """psi-art.py:85-92, in Angstrom."""
    m0 = 0.5109989461 * 10 ** 3
    h = 4.135667662 * 10 ** (-15) * 10 ** (-3)
    c = 2.99792458 * 10 ** 8
    return h * c / np.sqrt(v0 * (2 * m0 + v0)) * 1.e10


def defocus_ramp(n, middle=None):
    """3 |k - middle| (psi-art.py:293-294)."""
    middle = n // 2 if middle is None else middle
    return np.array([np.abs(i) * 3 for i in range(-middle, n - middle)], np.float64)


def boot_weights(n, middle, boot_size):
    """The weights of ``tf.add_n(mse_losses[lb:ub]) / (boot_size + 1)`` (psi-art.py:338-348)."""
    lb = middle - boot_size // 2 - boot_size % 2
    ub = middle + boot_size // 2
    if lb < 0:
        ub += np.absolute(lb)
        lb = 0
    if ub >= n:
        lb -= ub - (n - 1)
        ub = n - 1
    w = np.zeros(n)
    w[lb:ub] = 1.0 / (boot_size + 1)
    return w


def _pi(dtype):
    return np.arccos(dtype(-1))


@functools.lru_cache(maxsize=None)
def polar_grid(S, sampling, wavelength, dtype=np.float64):
    """(theta, phi) [S,S]: kx[i][j] = f[i], ky[i][j] = f[j], f = fftfreq(S, sampling).  Cached: do not write into the result."""
    f = np.fft.fftfreq(S, sampling).astype(dtype)
    kx, ky = f[:, None] * np.ones(S, dtype)[None, :], np.ones(S, dtype)[:, None] * f[None, :]
    return dtype(wavelength) * np.sqrt(kx * kx + ky * ky), np.arctan2(ky, kx)


def ctf_parts(S, sampling, wavelength, params, dtype=np.float64):
    """-> dict in ``dtype``: tbase = chi_base / pi (every term but a20's), q = theta^2 / lam (so chi_k / pi = tbase + a20_k q), T, basis
    [25] = d chi / d p (a20's entry is (pi / lam) theta^2), dlnT = d ln T / d focal_spread."""
    p = [dtype(v) for v in params]
    lam, pi = dtype(wavelength), _pi(dtype)
    th, phi = polar_grid(S, sampling, wavelength, dtype)
    total = np.zeros((S, S), dtype)
    basis = [None] * 25
    for n, m, ia, ip in TERMS:
        r = th ** n / dtype(n)
        if ip is None:
            basis[ia] = (dtype(2) * pi / lam) * r
            if ia != I_A20:
                total = total + p[ia] * r
        else:
            ang = dtype(m) * (phi - p[ip])
            c, s = np.cos(ang), np.sin(ang)
            total = total + p[ia] * c * r
            basis[ia] = (dtype(2) * pi / lam) * r * c
            basis[ip] = (dtype(2) * pi / lam) * r * p[ia] * dtype(m) * s
    x = dtype(0.5) * pi / lam * p[I_SPREAD] * th * th
    T = np.exp(-np.sign(p[I_SPREAD]) * x * x)
    y = dtype(0.5) * pi * th * th / lam
    return {"tbase": (dtype(2) / lam) * total, "q": th * th / lam, "T": T, "basis": basis,
            "dlnT": -dtype(2) * np.abs(p[I_SPREAD]) * y * y}


def offset_of(u, scale):
    return scale * np.tanh(u / scale)


def ctf(S, sampling, wavelength, params, ramp, offset_scale=1.0, dtype=np.float64, parts=None):
    """C [n,S,S] complex128 and max |chi|: C_k = (cos(pi r) - i sin(pi r)) T with r = fmod(chi_k / pi, 2)."""
    parts = parts or ctf_parts(S, sampling, wavelength, params, dtype)
    pi = _pi(dtype)
    off = offset_of(dtype(params[I_OFFSET]), dtype(offset_scale))
    out, chimax = [], 0.0
    for rk in ramp:
        t = parts["tbase"] + (dtype(params[I_A20]) * dtype(rk) + off) * parts["q"]
        chimax = max(chimax, float(np.abs(t).max() * pi))
        r = np.fmod(t, dtype(2))
        out.append((np.cos(pi * r) * parts["T"]).astype(np.float64) - 1j * (np.sin(pi * r) * parts["T"]).astype(np.float64))
    return np.stack(out), chimax


def targets(images, amplitudes=False):
    x = np.asarray(images, np.float32).astype(np.float64)
    return np.abs(x) if amplitudes else np.sqrt(np.maximum(x, 0.0))


def loss_and_gradients(images, amp, phase, params, ramp, weights, wavelength, sampling, offset_scale=1.0, normalise=True,
                       amplitudes=False, fft=NumpyFFT, ctf_dtype=np.float64):
    """-> dict: C, b, p [N,S,S]; losses [N + 1] (per image, then L); g_amp, g_phase [S,S]; g_params [27]; abs_terms [27] (the sum of
    the absolute values of every scalar gradient's terms); ratio = min_k min|b_k| / mean|b_k|; chimax; kappa [N] = sum r^2 / sum d^2."""
    images = np.asarray(images)
    N, S = images.shape[0], images.shape[-1]
    n = float(S * S)
    A, P = np.asarray(amp, np.float64), np.asarray(phase, np.float64)
    params = np.asarray(params, np.float64)
    parts = ctf_parts(S, sampling, wavelength, params, ctf_dtype)
    C, chimax = ctf(S, sampling, wavelength, params, ramp, offset_scale, ctf_dtype, parts)
    basis = [np.asarray(b, np.float64) for b in parts["basis"]]
    dlnT = np.asarray(parts["dlnT"], np.float64)
    r = targets(images, amplitudes)
    psi = A * (np.cos(P) + 1j * np.sin(P))
    ph = fft.fft2(psi)
    b, p, losses, kappa = [], [], [], []
    Gpsi = np.zeros((S, S), np.complex128)
    s_im, s_ramp, s_re = np.zeros((S, S)), np.zeros((S, S)), np.zeros((S, S))
    a_im, a_ramp, a_re = np.zeros((S, S)), np.zeros((S, S)), np.zeros((S, S))
    ratio = np.inf
    for k in range(N):
        bk = fft.ifft2(C[k] * ph)
        m = np.abs(bk)
        M = m.mean()
        ratio = min(ratio, float(m.min() / M))
        c = r[k].mean() / M if normalise else 1.0
        pk = c * m
        d = pk - r[k]
        losses.append((d * d).mean())
        kappa.append(float((r[k] * r[k]).sum() / (d * d).sum()))
        gm = d - (d * m).sum() / (n * M) if normalise else d
        gm = weights[k] * (2.0 * c / n) * gm
        with np.errstate(invalid="ignore", divide="ignore"):
            Gb = np.where(m > 0, gm * bk / m, 0.0)
        F = fft.fft2(Gb)
        Gpsi = Gpsi + fft.ifft2(np.conj(C[k]) * F)
        z = np.conj(F / n) * C[k] * ph
        s_im, s_ramp, s_re = s_im + z.imag, s_ramp + ramp[k] * z.imag, s_re + z.real
        a_im, a_ramp, a_re = a_im + np.abs(z.imag), a_ramp + np.abs(ramp[k] * z.imag), a_re + np.abs(z.real)
        b.append(bk)
        p.append(pk)
    losses = np.array(losses)
    g, at = np.zeros(NPARAM), np.zeros(NPARAM)
    for i in range(25):
        g[i], at[i] = (s_im * basis[i]).sum(), (a_im * np.abs(basis[i])).sum()
    g[I_A20], at[I_A20] = (s_ramp * basis[I_A20]).sum(), (a_ramp * np.abs(basis[I_A20])).sum()
    sech2 = 1.0 - np.tanh(params[I_OFFSET] / offset_scale) ** 2
    g[I_OFFSET], at[I_OFFSET] = sech2 * (s_im * basis[I_A20]).sum(), sech2 * (a_im * np.abs(basis[I_A20])).sum()
    g[I_SPREAD], at[I_SPREAD] = (s_re * dlnT).sum(), (a_re * np.abs(dlnT)).sum()
    cP, sP = np.cos(P), np.sin(P)
    return {"C": C, "b": np.stack(b), "p": np.stack(p), "losses": np.append(losses, (np.asarray(weights) * losses).sum()),
            "g_amp": cP * Gpsi.real + sP * Gpsi.imag, "g_phase": A * (-sP * Gpsi.real + cP * Gpsi.imag), "g_params": g,
            "abs_terms": at, "ratio": ratio, "chimax": chimax, "kappa": np.array(kappa)}


class Fit:
    """The trajectory: A, P, params and their Adam moments (TF's form); ``step()`` returns the losses [N + 1] before the update."""

    def __init__(self, images, amp, phase, params, ramp, weights, rates, wavelength, sampling, offset_scale=1.0, normalise=True,
                 amplitudes=False, beta1=0.99, beta2=0.999, epsilon=0.1, fft=NumpyFFT, ctf_dtype=np.float64):
        self.images, self.ramp, self.weights = images, np.asarray(ramp, np.float64), np.asarray(weights, np.float64)
        self.x = [np.array(amp, np.float64), np.array(phase, np.float64), np.array(params, np.float64)]
        self.m = [np.zeros_like(v) for v in self.x]
        self.v = [np.zeros_like(v) for v in self.x]
        self.rates = np.asarray(rates, np.float64)
        self.kw = dict(wavelength=wavelength, sampling=sampling, offset_scale=offset_scale, normalise=normalise, amplitudes=amplitudes,
                       fft=fft, ctf_dtype=ctf_dtype)
        self.beta1, self.beta2, self.epsilon, self.t = beta1, beta2, epsilon, 0
        self.scale, self.losses = np.zeros(NPARAM), None   # the largest sum of |terms| of every scalar gradient so far; the last losses

    def step(self):
        out = loss_and_gradients(self.images, self.x[0], self.x[1], self.x[2], self.ramp, self.weights, **self.kw)
        self.t += 1
        self.scale, self.losses = np.maximum(self.scale, out["abs_terms"]), out["losses"]
        corr = np.sqrt(1.0 - self.beta2 ** self.t) / (1.0 - self.beta1 ** self.t)
        for j, g in enumerate((out["g_amp"], out["g_phase"], out["g_params"])):
            lr = (np.full(g.shape, self.rates[j]) if j < 2 else self.rates[2:]) * corr
            on = lr != 0.0
            m = self.beta1 * self.m[j] + (1.0 - self.beta1) * g
            v = self.beta2 * self.v[j] + (1.0 - self.beta2) * g * g
            x = self.x[j] - lr * m / (np.sqrt(v) + self.epsilon)
            self.m[j], self.v[j], self.x[j] = np.where(on, m, self.m[j]), np.where(on, v, self.v[j]), np.where(on, x, self.x[j])
        return out["losses"]

    def state(self):
        """A, P, params, their first and second moments, and the last losses, as a dict of copies."""
        names = ("amp", "phase", "params")
        out = {n: x.copy() for n, x in zip(names, self.x)}
        out.update({"m_" + n: x.copy() for n, x in zip(names, self.m)})
        out.update({"v_" + n: x.copy() for n, x in zip(names, self.v)})
        out["losses"] = self.losses.copy()
        return out


def state_distance(got, want, scale):
    """The largest distance between two states: fields and their moments by relative L2; the scalars by |difference| / |value|; their
    moments entry by entry against ``scale`` (the largest sum of |terms| of that gradient along the trajectory; squared for v),
    since single scalar gradients cancel heavily; the losses relative."""
    d = {}
    for n in ("amp", "phase", "m_amp", "v_amp", "m_phase", "v_phase"):
        d[n] = rel_l2(got[n], want[n])
    with np.errstate(invalid="ignore", divide="ignore"):
        d["params"] = float(np.nanmax(np.where(want["params"] != 0, np.abs(got["params"] - want["params"]) / np.abs(want["params"]),
                                               np.where(got["params"] == want["params"], 0.0, np.inf))))
        ok = scale > 0
        d["m_params"] = float((np.abs(got["m_params"] - want["m_params"])[ok] / scale[ok]).max())
        d["v_params"] = float((np.abs(got["v_params"] - want["v_params"])[ok] / scale[ok] ** 2).max())
    d["losses"] = float(np.abs(got["losses"] / want["losses"] - 1.0).max())
    return d


# ---- the inputs of the tests ----------------------------------------------------------------------------------------------------

LAM, SAMPLING, SCALE = float(energy2wavelength(200)), 0.5, 5.0


def all_coefficient_point(S, seed=0):
    """Every coefficient non-zero: each amplitude's term contributes kappa in 1.5 .. 4.5 rad at the grid's largest theta
    (a_nm = kappa n lam / (2 pi theta_max^n)), azimuths in (-1, 1) away from 0, focal spread 15 .. 20, u 0.2 .. 0.3."""
    rng = np.random.default_rng(1000 + S + seed)
    th_max = float(polar_grid(S, SAMPLING, LAM)[0].max())
    p = np.zeros(NPARAM)
    for n, m, ia, ip in TERMS:
        p[ia] = rng.uniform(1.5, 4.5) * rng.choice([-1.0, 1.0]) * n * LAM / (2.0 * np.pi * th_max ** n)
        if ip is not None:
            p[ip] = rng.uniform(0.1, 1.0) * rng.choice([-1.0, 1.0])
    p[I_SPREAD], p[I_OFFSET] = rng.uniform(15.0, 20.0), rng.uniform(0.2, 0.3)
    return p


@functools.lru_cache(maxsize=None)
def case(N, S, spread=True):
    """The all-coefficient case of (N, S): the images come from the true wave at the true parameters, the evaluation point is off
    them (so that the residual is not rounding noise).  Cached: do not write into the result."""
    truth = all_coefficient_point(S)
    if not spread:
        truth[I_SPREAD] = 0.0
    ramp = defocus_ramp(N)
    w = true_wave(S)
    C, _ = ctf(S, SAMPLING, LAM, truth, ramp, SCALE)
    images = np.stack([np.abs(np.fft.ifft2(C[k] * np.fft.fft2(w))) ** 2 for k in range(N)]).astype(np.float32)
    rng = np.random.default_rng(2000 + S)
    params = truth * (1.0 + 0.1 * rng.uniform(-1.0, 1.0, NPARAM))
    amp = np.abs(w) * (1.0 + 0.02 * rng.uniform(-1.0, 1.0, (S, S)))
    phase = 0.8 * np.angle(w) + 0.02 * rng.uniform(-1.0, 1.0, (S, S))
    weights = rng.uniform(0.5, 1.5, N) / N
    return {"images": images, "amp": amp, "phase": phase, "params": params, "ramp": ramp, "weights": weights, "truth": truth}
