"""The float64 numpy restatement of the psi-art fit with per-image sub-pixel shifts (emdenoise.psiart with ``shifts``; include/emdenoise.h
"The same fit with a trainable sub-pixel shift of every image"), built on tests/psiart_ref.py's ``ctf_parts``,
``targets`` and FFT classes and independent of the library.  ``shifts`` is [N,2] in pixels, along axis 0 then axis 1; with
``f = numpy.fft.fftfreq(S)``

    chi_k / pi = (tbase + a20_k q) + 2 (f[i] d0_k + f[j] d1_k),    C_k = (cospi(.) - i sinpi(.)) T,

that is C_k times exp(-2 pi i (f_i d0_k + f_j d1_k)): prediction k is moved circularly by (d0_k, d1_k).  The gradients are
dL/dd0_k = sum Im z_k 2 pi f[i] and dL/dd1_k = sum Im z_k 2 pi f[j], sums per image.  tests/test_psiart_shift.py holds them against
torch's autograd on the CPU.  With all shifts 0 every operation of ``psiart_ref.loss_and_gradients`` is made in its order on its
values (t + 0 is t), so the results are equal bit for bit.

The same two evaluations as in psiart_ref give the yardsticks of the device tests: ``fft=NumpyFFT, ctf_dtype=float64`` and
``fft=Radix2FFT, ctf_dtype=longdouble`` (the shift's term is then formed in extended precision too)."""
import numpy as np

from tests import psiart_ref as R
from tests.psiart_ref import NumpyFFT, Radix2FFT, rel_l2   # noqa: F401  (re-exported for the tests)


def shift_terms(S, shifts, dtype=np.float64):
    """[N,S,S] in ``dtype``: 2 (f[i] d0_k + f[j] d1_k), what the shift of image k adds to chi_k / pi."""
    f = np.fft.fftfreq(S).astype(dtype)                                    # i' / S: exact, S is a power of two
    d = np.asarray(shifts, np.float64).astype(dtype)
    return dtype(2) * (f[None, :, None] * d[:, 0, None, None] + f[None, None, :] * d[:, 1, None, None])


def ctf(S, sampling, wavelength, params, ramp, shifts, offset_scale=1.0, dtype=np.float64, parts=None):
    """``psiart_ref.ctf`` with the shifts' terms added to t once tbase + a20_k q is formed: C [n,S,S] complex128 and max |chi|."""
    parts = parts or R.ctf_parts(S, sampling, wavelength, params, dtype)
    pi = R._pi(dtype)
    off = R.offset_of(dtype(params[R.I_OFFSET]), dtype(offset_scale))
    sh = shift_terms(S, shifts, dtype)
    out, chimax = [], 0.0
    for k, rk in enumerate(ramp):
        t = (parts["tbase"] + (dtype(params[R.I_A20]) * dtype(rk) + off) * parts["q"]) + sh[k]
        chimax = max(chimax, float(np.abs(t).max() * pi))
        r = np.fmod(t, dtype(2))
        out.append((np.cos(pi * r) * parts["T"]).astype(np.float64) - 1j * (np.sin(pi * r) * parts["T"]).astype(np.float64))
    return np.stack(out), chimax


def loss_and_gradients(images, amp, phase, params, shifts, ramp, weights, wavelength, sampling, offset_scale=1.0, normalise=True,
                       amplitudes=False, fft=NumpyFFT, ctf_dtype=np.float64):
    """The dict of ``psiart_ref.loss_and_gradients`` and g_shifts [N,2], abs_terms_shifts [N,2] (the sum of |terms| of every entry)."""
    images = np.asarray(images)
    N, S = images.shape[0], images.shape[-1]
    n = float(S * S)
    A, P = np.asarray(amp, np.float64), np.asarray(phase, np.float64)
    params = np.asarray(params, np.float64)
    parts = R.ctf_parts(S, sampling, wavelength, params, ctf_dtype)
    C, chimax = ctf(S, sampling, wavelength, params, ramp, shifts, offset_scale, ctf_dtype, parts)
    basis = [np.asarray(b, np.float64) for b in parts["basis"]]
    dlnT = np.asarray(parts["dlnT"], np.float64)
    f = np.fft.fftfreq(S).astype(ctf_dtype)
    w0 = np.asarray((ctf_dtype(2) * R._pi(ctf_dtype) * f)[:, None] * np.ones(S, ctf_dtype)[None, :], np.float64)   # d chi_k / d d0_k
    w1 = np.ascontiguousarray(w0.T)                                                                               # d chi_k / d d1_k
    r = R.targets(images, amplitudes)
    psi = A * (np.cos(P) + 1j * np.sin(P))
    ph = fft.fft2(psi)
    b, p, losses, kappa = [], [], [], []
    Gpsi = np.zeros((S, S), np.complex128)
    s_im, s_ramp, s_re = np.zeros((S, S)), np.zeros((S, S)), np.zeros((S, S))
    a_im, a_ramp, a_re = np.zeros((S, S)), np.zeros((S, S)), np.zeros((S, S))
    gs, ats = np.zeros((N, 2)), np.zeros((N, 2))
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
        gs[k] = (z.imag * w0).sum(), (z.imag * w1).sum()
        ats[k] = (np.abs(z.imag) * np.abs(w0)).sum(), (np.abs(z.imag) * np.abs(w1)).sum()
        b.append(bk)
        p.append(pk)
    losses = np.array(losses)
    g, at = np.zeros(R.NPARAM), np.zeros(R.NPARAM)
    for i in range(25):
        g[i], at[i] = (s_im * basis[i]).sum(), (a_im * np.abs(basis[i])).sum()
    g[R.I_A20], at[R.I_A20] = (s_ramp * basis[R.I_A20]).sum(), (a_ramp * np.abs(basis[R.I_A20])).sum()
    sech2 = 1.0 - np.tanh(params[R.I_OFFSET] / offset_scale) ** 2
    g[R.I_OFFSET], at[R.I_OFFSET] = sech2 * (s_im * basis[R.I_A20]).sum(), sech2 * (a_im * np.abs(basis[R.I_A20])).sum()
    g[R.I_SPREAD], at[R.I_SPREAD] = (s_re * dlnT).sum(), (a_re * np.abs(dlnT)).sum()
    cP, sP = np.cos(P), np.sin(P)
    return {"C": C, "b": np.stack(b), "p": np.stack(p), "losses": np.append(losses, (np.asarray(weights) * losses).sum()),
            "g_amp": cP * Gpsi.real + sP * Gpsi.imag, "g_phase": A * (-sP * Gpsi.real + cP * Gpsi.imag), "g_params": g,
            "abs_terms": at, "g_shifts": gs, "abs_terms_shifts": ats, "ratio": ratio, "chimax": chimax, "kappa": np.array(kappa)}


class Fit:
    """``psiart_ref.Fit`` with the shifts as a fourth trained tensor: ``shift_rates`` [N], one rate per image for both of its axes; a
    rate of 0 leaves that image's shift and its moments as they are."""

    def __init__(self, images, amp, phase, params, shifts, ramp, weights, rates, shift_rates, wavelength, sampling, offset_scale=1.0,
                 normalise=True, amplitudes=False, beta1=0.99, beta2=0.999, epsilon=0.1, fft=NumpyFFT, ctf_dtype=np.float64):
        self.images, self.ramp, self.weights = images, np.asarray(ramp, np.float64), np.asarray(weights, np.float64)
        self.x = [np.array(amp, np.float64), np.array(phase, np.float64), np.array(params, np.float64), np.array(shifts, np.float64)]
        self.m = [np.zeros_like(v) for v in self.x]
        self.v = [np.zeros_like(v) for v in self.x]
        self.rates, self.shift_rates = np.asarray(rates, np.float64), np.asarray(shift_rates, np.float64)
        self.kw = dict(wavelength=wavelength, sampling=sampling, offset_scale=offset_scale, normalise=normalise, amplitudes=amplitudes,
                       fft=fft, ctf_dtype=ctf_dtype)
        self.beta1, self.beta2, self.epsilon, self.t = beta1, beta2, epsilon, 0
        # the largest sums of |terms| so far, of the scalar gradients and of the shift gradients; the last losses
        self.scale, self.scale_shifts, self.losses = np.zeros(R.NPARAM), np.zeros(self.x[3].shape), None

    def step(self):
        out = loss_and_gradients(self.images, self.x[0], self.x[1], self.x[2], self.x[3], self.ramp, self.weights, **self.kw)
        self.t += 1
        self.scale, self.losses = np.maximum(self.scale, out["abs_terms"]), out["losses"]
        self.scale_shifts = np.maximum(self.scale_shifts, out["abs_terms_shifts"])
        corr = np.sqrt(1.0 - self.beta2 ** self.t) / (1.0 - self.beta1 ** self.t)
        rates = (np.full(self.x[0].shape, self.rates[0]), np.full(self.x[1].shape, self.rates[1]), self.rates[2:],
                 np.repeat(self.shift_rates[:, None], 2, axis=1))
        for j, g in enumerate((out["g_amp"], out["g_phase"], out["g_params"], out["g_shifts"])):
            lr = rates[j] * corr
            on = lr != 0.0
            m = self.beta1 * self.m[j] + (1.0 - self.beta1) * g
            v = self.beta2 * self.v[j] + (1.0 - self.beta2) * g * g
            x = self.x[j] - lr * m / (np.sqrt(v) + self.epsilon)
            self.m[j], self.v[j], self.x[j] = np.where(on, m, self.m[j]), np.where(on, v, self.v[j]), np.where(on, x, self.x[j])
        return out["losses"]

    def state(self):
        """A, P, params, shifts, their first and second moments, and the last losses, as a dict of copies."""
        names = ("amp", "phase", "params", "shifts")
        out = {n: x.copy() for n, x in zip(names, self.x)}
        out.update({"m_" + n: x.copy() for n, x in zip(names, self.m)})
        out.update({"v_" + n: x.copy() for n, x in zip(names, self.v)})
        out["losses"] = self.losses.copy()
        return out


def state_distance(got, want, scale, scale_shifts):
    """``psiart_ref.state_distance`` and, by its rule for the scalars, the shifts (|difference| / |value|; an entry that is 0 must be
    equal) and their moments entry by entry against ``scale_shifts`` (squared for v)."""
    d = R.state_distance(got, want, scale)
    g, w = {k: np.asarray(got[k]).reshape(-1) for k in ("shifts", "m_shifts", "v_shifts")}, \
        {k: np.asarray(want[k]).reshape(-1) for k in ("shifts", "m_shifts", "v_shifts")}
    s = np.asarray(scale_shifts).reshape(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        d["shifts"] = float(np.nanmax(np.where(w["shifts"] != 0, np.abs(g["shifts"] - w["shifts"]) / np.abs(w["shifts"]),
                                               np.where(g["shifts"] == w["shifts"], 0.0, np.inf))))
        ok = s > 0
        d["m_shifts"] = float((np.abs(g["m_shifts"] - w["m_shifts"])[ok] / s[ok]).max())
        d["v_shifts"] = float((np.abs(g["v_shifts"] - w["v_shifts"])[ok] / s[ok] ** 2).max())
    return d


# ---- the inputs of the tests ----------------------------------------------------------------------------------------------------

def integer_roll(p, shifts):
    """numpy.roll of every prediction by its whole-pixel shift."""
    return np.stack([np.roll(pk, (int(a), int(b)), (0, 1)) for pk, (a, b) in zip(p, np.asarray(shifts))])


def case(N, S, seed=0):
    """``psiart_ref.case(N, S)`` with shifts: true shifts seeded in +-0.6 px move the images (through the model's own phase, so the
    images are float32(|b_k|^2) at the truth), and the evaluation point is off them by +-0.2 px, so every shift is within +-0.8 px."""
    c = dict(R.case(N, S))
    rng = np.random.default_rng(3000 + 64 * N + S + seed)
    true_shifts = rng.uniform(-0.6, 0.6, (N, 2))
    C, _ = ctf(S, R.SAMPLING, R.LAM, c["truth"], c["ramp"], true_shifts, R.SCALE)
    w = R.true_wave(S)
    c["images"] = np.stack([np.abs(np.fft.ifft2(C[k] * np.fft.fft2(w))) ** 2 for k in range(N)]).astype(np.float32)
    c["true_shifts"] = true_shifts
    c["shifts"] = true_shifts + 0.2 * rng.choice([-1.0, 1.0], (N, 2)) * rng.uniform(0.5, 1.0, (N, 2))
    return c
