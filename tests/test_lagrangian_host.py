"""Lagrangian spectra, autocovariance and dispersion (niwqg_amd/lagrangian.py), the parts that need no GPU:
the numpy restatements against closed forms, every argument error raised before the device is touched, the bookkeeping of the
groups, and the declarations of the new entry points."""
import ctypes
import os
import re

import numpy as np
import pytest

from niwqg_amd import _lib, lagrangian
from niwqg_amd.particles import Trajectory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def traj(x=None, y=None, dt=2.0, **values):
    some = next(iter(values.values())) if values else x
    T, n = np.shape(some)
    x = np.zeros((T, n)) if x is None else x
    y = np.zeros((T, n)) if y is None else y
    return Trajectory(np.arange(T), dt * np.arange(T), x, y, values)


# ---- the restatements against closed forms ----------------------------------------------------------------------------------
@pytest.mark.parametrize("T, F", [(16, 16), (12, 24)])
def test_pure_lines_land_in_their_bin(T, F):
    """x_n(i) = a_i e^{-i omega_p n Delta} with omega_p a frequency of the F-point transform: with a boxcar window and no demeaning
    all the power is in the bin of +omega_p, and Parseval holds as the module states it"""
    dt, n = 2.0, 5
    bins = np.array([1, 3, F - 2, 0, 5])                         # FFT bins: F - 2 is a negative frequency
    amp = np.array([1.0, 2.0, 0.5, 3.0, 1.5])
    om = 2 * np.pi * np.fft.fftfreq(F, dt)[bins]
    t = dt * np.arange(T)
    phi = amp[None] * np.exp(-1j * om[None] * t[:, None])
    tr = traj(phi=phi, dt=dt)
    for i in range(n):
        g = np.zeros(n, int)
        g[i] = 1
        omega, P, counts = lagrangian.reference_spectrum(tr, "phi", window="boxcar", demean=False, groups=g, nfft=F, dt_rec=dt)
        assert list(counts) == [n - 1, 1] and P.shape == (F, 2)
        assert np.all(np.diff(omega) > 0)
        k = int(np.argmax(P[:, 1]))
        assert abs(omega[k] - om[i]) <= 1e-12 * abs(omega).max()
        if F == T:                                               # an exact line of the transform: nothing leaks
            assert P[:, 1].sum() - P[k, 1] <= 1e-24 * P[k, 1] + 1e-28
        assert abs(P[:, 1].sum() - 0.5 * amp[i] ** 2) <= 1e-13 * amp[i] ** 2
    # Parseval with a window and demeaning: sum_p P = the mean over particles of 1/2 sum w^2 |x'|^2 / sum w^2
    w = 1.0 + 0.3 * np.sin(np.arange(T))
    omega, P, _ = lagrangian.reference_spectrum(tr, "phi", window=w, demean=True, nfft=F, dt_rec=dt)
    xp = phi - phi.mean(axis=0)[None]
    want = np.mean(0.5 * (w[:, None] ** 2 * abs(xp) ** 2).sum(axis=0) / (w * w).sum())
    assert P.shape == (F,) and abs(P.sum() - want) <= 1e-13 * want


def test_rotary_sign_and_real_series():
    """u + i v of a clockwise circle (u = cos, v = -sin: e^{-i omega t}) lands at +omega; a real series splits evenly"""
    T, dt = 32, 0.5
    om = 2 * np.pi * np.fft.fftfreq(T, dt)[5]
    t = dt * np.arange(T)[:, None] * np.ones((1, 3))
    tr = traj(u=np.cos(om * t), v=-np.sin(om * t), dt=dt)
    omega, P, _ = lagrangian.reference_spectrum(tr, "uv", window="boxcar", demean=False, dt_rec=dt)
    assert abs(omega[np.argmax(P)] - om) <= 1e-12 * om and om > 0
    omega, Pu, _ = lagrangian.reference_spectrum(tr, "u", window="boxcar", demean=False, dt_rec=dt)
    k = np.argsort(Pu)[-2:]
    assert np.allclose(sorted(omega[k]), [-om, om], rtol=1e-12) and abs(Pu[k[0]] - Pu[k[1]]) <= 1e-14 * Pu.max()


def test_ballistic_dispersion():
    """x = x0 + c t: A2 = <|c|^2> tau^2, D2 = <|dr0 + dc tau|^2>, kurtosis from the fourth moments"""
    rng = np.random.default_rng(1)
    n, T, dt = 40, 9, 3.0
    x0, y0 = rng.uniform(0, 10, n), rng.uniform(0, 10, n)
    cx, cy = rng.standard_normal(n), rng.standard_normal(n)
    tau = dt * np.arange(T)
    tr = traj(x=x0[None] + cx[None] * tau[:, None], y=y0[None] + cy[None] * tau[:, None], dt=dt)
    i, j = rng.permutation(n)[:15], (rng.permutation(n)[:15])
    j = np.where(i == j, (j + 1) % n, j)
    groups = np.arange(n) % 3
    d = lagrangian.reference_dispersion(tr, pairs=(i, j), groups=groups)
    for g in range(3):
        c2 = (cx ** 2 + cy ** 2)[groups == g]
        assert np.allclose(d["A2"][:, g], c2.mean() * tau ** 2, rtol=1e-12, atol=0)
        assert np.allclose(d["A_xy"][:, g], (cx * cy)[groups == g].mean() * tau ** 2, rtol=1e-11, atol=1e-13)
        assert np.allclose(d["dx"][:, g], cx[groups == g].mean() * tau, rtol=1e-11, atol=1e-13)
        assert np.allclose(d["M4"][:, g], (c2 ** 2).mean() * tau ** 4, rtol=1e-12, atol=0)
    sx = (x0[i] - x0[j])[None] + (cx[i] - cx[j])[None] * tau[:, None]
    sy = (y0[i] - y0[j])[None] + (cy[i] - cy[j])[None] * tau[:, None]
    assert np.allclose(d["D2"], (sx ** 2 + sy ** 2).mean(axis=1), rtol=1e-12, atol=0)
    assert np.allclose(d["D_xx"] + d["D_yy"], d["D2"], rtol=1e-14, atol=0)
    assert np.allclose(d["S4"], ((sx ** 2 + sy ** 2) ** 2).mean(axis=1), rtol=1e-12, atol=0)
    # the object's kurtosis is the ratio of the same moments
    D = lagrangian.Dispersion(tr.t, tr.step, np.array([n]), np.zeros((T, 1, 6)), None, 0, False)
    D.M4, D.A2 = d["M4"][:, 0], d["A2"][:, 0]
    with np.errstate(all="ignore"):
        assert np.allclose(D.kurtosis()[1:], d["M4"][1:, 0] / d["A2"][1:, 0] ** 2, rtol=1e-15) and np.isnan(D.kurtosis()[0])
    with pytest.raises(ValueError, match="no pairs"):
        D.pair_kurtosis()


@pytest.mark.parametrize("demean", [False, True])
def test_autocovariance_against_double_loops(demean):
    rng = np.random.default_rng(2)
    T, n = 11, 6
    u, v = rng.standard_normal((T, n)), rng.standard_normal((T, n))
    tr = traj(u=u, v=v, dt=0.25)
    groups = np.array([0, 2, 2, 0, 2, 0])                        # group 1 is empty
    for name, x in (("u", u.astype(complex)), ("uv", u + 1j * v)):
        lag, R, counts = lagrangian.reference_autocovariance(tr, name, max_lag=7, demean=demean, groups=groups, dt_rec=0.25)
        assert np.array_equal(lag, 0.25 * np.arange(8)) and R.shape == (8, 3) and list(counts) == [3, 0, 3]
        assert np.iscomplexobj(R) == (name == "uv")
        want = np.zeros((8, 3), complex)
        for g in (0, 2):
            for k in range(8):
                acc = 0.0
                for i in np.flatnonzero(groups == g):
                    xi = x[:, i] - (x[:, i].mean() if demean else 0.0)
                    s = 0.0
                    for m in range(T - k):
                        s += np.conj(xi[m]) * xi[m + k]
                    acc += s / (T - k)
                want[k, g] = acc / 3
        assert np.all(np.isnan(R[:, 1]))
        assert np.abs(R[:, [0, 2]] - want[:, [0, 2]]).max() <= 1e-14 * np.abs(want).max()
        # the device's route -- a boxcar table of F = 2T, transformed on the host -- gives the same numbers
        sums = np.zeros((2 * T, 3))
        xp = x - (x.mean(axis=0)[None] if demean else 0.0)
        X = 2 * T * np.fft.ifft(xp, n=2 * T, axis=0)
        for g in range(3):
            sums[:, g] = 0.5 * (abs(X[:, groups == g]) ** 2).sum(axis=1) / (2 * T * T)
        Rt = lagrangian._autocov_from_table(sums, counts, T, 7, name == "u", True)
        assert np.abs(Rt[:, [0, 2]] - want[:, [0, 2]]).max() <= 1e-13 * np.abs(want).max() and np.all(np.isnan(Rt[:, 1]))


def test_diffusivity_is_the_cumulative_trapezoid():
    lag = 0.5 * np.arange(6)
    R = np.array([4.0, 3.0, 1.0, -0.5, 0.25, 0.0])
    trapz = getattr(np, "trapezoid", None) or np.trapz
    A = lagrangian.Autocovariance("u", lag, R, np.array([3]))
    assert np.allclose(A.diffusivity(), [trapz(R[:k + 1], lag[:k + 1]) for k in range(6)], rtol=1e-15)
    B = lagrangian.Autocovariance("uv", lag, np.stack([R + 2j, 2 * R - 1j], axis=1), np.array([3, 3]))
    assert np.allclose(B.diffusivity()[:, 1], [trapz(R[:k + 1], lag[:k + 1]) for k in range(6)], rtol=1e-15)
    assert np.allclose(B.diffusivity()[:, 0], 0.5 * A.diffusivity(), rtol=1e-15)


@pytest.mark.parametrize("T, F", [(16, 16), (12, 24), (7, 7)])
def test_longdouble_direct_dft_against_numpy(T, F):
    rng = np.random.default_rng(3)
    n = 9
    phi = rng.standard_normal((T, n)) + 1j * rng.standard_normal((T, n))
    groups = np.arange(n) % 2
    o1, P1, _ = lagrangian.reference_spectrum(traj(phi=phi), "phi", groups=groups, nfft=F, dt_rec=2.0)
    o2, P2, _ = lagrangian.reference_spectrum(traj(phi=phi.astype(np.clongdouble)), "phi", groups=groups, nfft=F, dt_rec=2.0)
    assert P2.dtype == np.longdouble and np.array_equal(o1, o2)
    assert float(np.abs(P1 - P2).max()) <= 1e-13 * float(P2.sum())
    q = rng.standard_normal((T, n))
    _, Q1, _ = lagrangian.reference_spectrum(traj(q=q), "q", window="boxcar", dt_rec=2.0)
    _, Q2, _ = lagrangian.reference_spectrum(traj(q=q.astype(np.longdouble)), "q", window="boxcar", dt_rec=2.0)
    assert Q2.dtype == np.longdouble and float(np.abs(Q1 - Q2).max()) <= 1e-13 * float(Q2.sum())


# ---- argument errors, before the device ------------------------------------------------------------------------------------------
class NoDevice(object):
    def __getattr__(self, name):
        raise AssertionError("the device was touched: %s" % name)


class Model(object):
    dt = 2.0


class FakeParticles(object):
    """what lagrangian.py reads of a Particles object; every device pass fails the test"""

    def __init__(self, n=10, record=("u", "v", "q"), record_every=1, held=8, attached=True):
        self.n, self.record, self.record_every, self.held = n, tuple(record), record_every, held
        self.m, self.tc0, self.ctx = (Model() if attached else None), 0, NoDevice()

    def _check(self):
        if self.m is None:
            raise RuntimeError("particles: detached")

    def _held(self):
        return self.held

    def _record_steps(self):
        return np.arange(self.held)

    def _lagr_spectrum(self, *a):
        raise AssertionError("the device was touched")

    _lagr_dispersion = _lagr_spectrum


def test_every_argument_error_is_raised_before_the_device():
    P = FakeParticles()
    S, A, D = lagrangian.spectrum, lagrangian.autocovariance, lagrangian.dispersion
    with pytest.raises(ValueError, match="unknown name"):
        S(P, names=["zeta"])
    with pytest.raises(ValueError, match="'phi' is not recorded"):
        S(P, names="phi")
    with pytest.raises(ValueError, match="'uv' needs both"):
        S(FakeParticles(record=("u", "q")), names="uv")
    with pytest.raises(ValueError, match="'uv' needs both"):
        A(FakeParticles(record=("v",)), "uv")
    with pytest.raises(ValueError, match="no names"):
        S(FakeParticles(record=()))
    with pytest.raises(ValueError, match="shape"):
        S(P, window=np.ones(7))
    with pytest.raises(ValueError, match="finite"):
        S(P, window=[1, 1, 1, np.nan, 1, 1, 1, 1])
    with pytest.raises(ValueError, match="window = 'hamming'"):
        S(P, window="hamming")
    with pytest.raises(ValueError, match="zero everywhere"):
        S(P, window=np.zeros(8))
    with pytest.raises(ValueError, match="nfft"):
        S(P, nfft=7)
    with pytest.raises(ValueError, match="nfft"):
        S(P, nfft=8.0)
    with pytest.raises(ValueError, match="nfft"):
        S(P, nfft=9000)
    with pytest.raises(ValueError, match="chunk"):
        S(P, chunk=-1)
    for bad in (np.full(10, -1), np.full(10, 256), np.zeros(9, int), np.zeros(10)):
        for call in (lambda: S(P, groups=bad), lambda: A(P, "u", groups=bad), lambda: D(P, groups=bad)):
            with pytest.raises(ValueError, match="group"):
                call()
    with pytest.raises(ValueError, match="max_lag"):
        A(P, "u", max_lag=8)
    with pytest.raises(ValueError, match="unknown name"):
        A(P, "w")
    for bad in (([0, 1], [1, 10]), ([-1], [2]), ([3, 4], [5, 4]), ([1, 2], [3]), ([0.5], [1.0]), 3, ([], [])):
        with pytest.raises(ValueError, match="pair"):
            D(P, pairs=bad)
    for fn in (lambda Q: S(Q), lambda Q: A(Q, "u"), lambda Q: D(Q)):
        with pytest.raises(ValueError, match="record_every = 0"):
            fn(FakeParticles(record_every=0, held=0))
        with pytest.raises(ValueError, match="at least 2"):
            fn(FakeParticles(held=1))
        with pytest.raises(RuntimeError, match="detached"):
            fn(FakeParticles(attached=False))


def test_default_names():
    assert lagrangian.available(("u", "v", "q", "phi")) == ["uv", "q", "phi"]
    assert lagrangian.available(("phi", "u")) == ["phi", "u"]
    assert lagrangian.check_names(("q", "v", "u"), None) == ["uv", "q"]
    assert lagrangian.check_names(("q", "v", "u"), "v") == ["v"]
    assert np.array_equal(lagrangian.check_window("hann", 12), 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(12) / 12))
    assert lagrangian.check_nfft(None, 12) == 12 and lagrangian.check_nfft(16384, 12) == 16384


# ---- group bookkeeping --------------------------------------------------------------------------------------------------------
def test_groups_stable_order_offsets_and_an_empty_group():
    labels = np.array([2, 0, 2, 3, 0, 2, 0])
    order, offsets, counts, G = lagrangian.check_groups(labels, 7)
    assert G == 4 and order.dtype == np.int32 and offsets.dtype == np.int32
    assert list(order) == [1, 4, 6, 0, 2, 5, 3]                  # stable: the particles of a group keep their order
    assert list(offsets) == [0, 3, 3, 6, 7] and list(counts) == [3, 0, 3, 1]
    for g in range(G):
        assert np.array_equal(order[offsets[g]:offsets[g + 1]], np.flatnonzero(labels == g))
    order, offsets, counts, G = lagrangian.check_groups(None, 5)
    assert G == 1 and list(order) == [0, 1, 2, 3, 4] and list(offsets) == [0, 5] and list(counts) == [5]
    # sums -> means: the empty group is NaN, without groups the axis goes
    sums = np.arange(8.0).reshape(2, 4)
    m = lagrangian._per_group(sums, np.array([3, 0, 3, 1]), True)
    assert np.all(np.isnan(m[:, 1])) and np.array_equal(m[:, [0, 2, 3]], sums[:, [0, 2, 3]] / [3, 3, 1])
    assert lagrangian._per_group(sums[:, :1], np.array([4]), False).shape == (2,)
    assert lagrangian.check_groups(np.array([255, 0], np.uint8), 2)[3] == 256


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def test_entries_declared_with_the_documented_arguments():
    header = open(os.path.join(ROOT, "include", "niwqg_amd.h")).read()
    protos = {name: params for name, _, params in _lib.PROTOTYPES}
    want = {"nq_lagr_spectrum": 11, "nq_lagr_dispersion": 10, "nq_any_lagr_spectrum": 14, "nq_any_lagr_dispersion": 12}
    for name, nargs in want.items():
        assert name in _lib.EXPORTS and re.search(r"\bint %s\(" % name, header), name
        assert len(protos[name]) == nargs, (name, protos[name])
        argtypes, restype = _lib.signature((name, "int", protos[name]))
        assert restype is ctypes.c_int and argtypes[0] is ctypes.c_void_p
    assert [p for _, p in protos["nq_lagr_spectrum"]] == ["ctx", "name", "T", "nfft", "window", "demean", "G", "order", "offsets", "chunk",
                                                         "out"]


def test_entries_exported_and_null_handles_refused():
    import niwqg_amd
    niwqg_amd.build()
    L = _lib.lib()
    w = (ctypes.c_double * 4)()
    i = (ctypes.c_int * 4)(0, 1, 2, 3)
    o = (ctypes.c_int * 2)(0, 4)
    assert L.nq_lagr_spectrum(None, 0, 4, 4, w, 0, 1, i, o, 0, w) != 0
    assert L.nq_lagr_dispersion(None, 4, 1, i, o, 0, None, None, w, None) != 0
    assert L.nq_any_lagr_spectrum(None, 4, 4, None, None, 2, 4, w, 0, 1, i, o, 0, w) == -1
    assert L.nq_any_lagr_dispersion(None, 4, 4, None, 1, i, o, 0, None, None, w, None) == -1
