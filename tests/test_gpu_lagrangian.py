"""Lagrangian spectra, autocovariance and dispersion of the particle records on the device (niwqg_amd/lagrangian.py, nq_lagr_*,
nq_any_lagr_*): the device tables against the numpy restatement applied to the downloaded trajectory of the
same run (double and extended precision), Parseval, an exact flow, the Doppler shift that is gone along trajectories, determinism,
no side effects and the lifecycle.  Every run has 300 particles: more than one 256-thread workgroup, with a tail of 44.

Observed on an MI355X (the tests print them with -s; the bars are asserted):
  spectra, max |device - numpy| / sum of the table, every case      1.1e-15  (bar 1e-12; against the longdouble restatement 2.2e-16)
  Parseval, relative                                                  5.4e-16  (bar 1e-12)
  dispersion, max |device - numpy| / max of the series                2.5e-14  (bar 1e-12)
  autocovariance, max |device - direct sums| / R(0)                   5.1e-15  (bar 1e-12)
  exact flow, error of A2 / of D2 over the propagated bound           1.2e-07 / 5.7e-07
  Doppler test, share of the power outside the bin of +Omega          1.1e-28  (printed, not asserted)
"""
import ctypes

import numpy as np
import pytest

from test_gpu_forcing import pair
from test_gpu_particles import particle_set, _euler_model, velocity
from test_particles_host import interp as interpolate
from test_oracle_golden import notebook_kwargs

pytestmark = pytest.mark.gpu

N = 300
# (kind, nx, mask): the fused plans at 64^2, "mask" (dealias without the filter) is the dual-copy context, 48^2 is the any-size path
MODELS = [("coupled", 64, "filter"), ("qg", 64, "filter"), ("ybj", 64, "filter"), ("coupled", 64, "mask"), ("coupled", 48, "filter")]
# (capacity, steps, nfft): a wrapped ring (22 records written into 16 slots: the oldest sits in slot 6), a ring holding 7 of 16, and
# 12 records transformed at length 24 (not a power of two)
RINGS = [(16, 21, None), (16, 6, None), (12, 14, 24)]
ARRAY_WINDOW = "array"
GROUPS3 = np.where(np.arange(N) % 2 == 1, 2, 0)                 # G = 3, group 1 is empty


def model(kind, nx, mask="filter"):
    m, _, init, _ = pair(kind, nx, mask, oracle=False)
    init(m)
    return m


def names_of(kind):
    return ("u", "v", "q") if kind == "qg" else ("u", "v", "q", "phi")


def advance(m, steps, batched=True):
    if batched and not getattr(m, "_any_size", False):
        m._ctx.step(steps)                    # one call: the records are written without a host visit
    else:
        for _ in range(steps):
            m._step_forward()


def run(kind, nx, mask, capacity, steps, batched=True):
    from niwqg_amd import particles
    m = model(kind, nx, mask)
    x, y = particle_set(m, N)
    P = particles.attach(m, x, y, record_every=1, capacity=capacity, record=names_of(kind))
    advance(m, steps, batched)
    return m, P


@pytest.fixture(scope="module")
def recorded():
    """(kind, nx, mask, capacity, steps) -> model, particles, their downloaded trajectory and 200 random pairs; run once and only
    read afterwards"""
    cache = {}

    def get(kind, nx, mask, capacity, steps):
        key = (kind, nx, mask, capacity, steps)
        if key not in cache:
            m, P = run(*key)
            rng = np.random.default_rng(11)
            i = rng.integers(0, N, 200)
            j = (i + rng.integers(1, N, 200)) % N
            cache[key] = (m, P, P.trajectory(), (i, j))
        return cache[key]
    return get


def window_of(window, T):
    return 0.25 + np.arange(T) % 5 if window == ARRAY_WINDOW else window


def rel_err(dev, ref):
    """max |dev - ref| over the finite entries of ref, over their sum; NaN entries (an empty group) must be NaN in both"""
    dev, ref = np.asarray(dev), np.asarray(ref, dtype=np.longdouble if np.asarray(ref).dtype == np.longdouble else np.float64)
    assert dev.shape == ref.shape
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(dev), nan)
    return float(np.abs(dev[~nan] - ref[~nan]).max() / ref[~nan].sum())


# ---- 1. the tables against the restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity, steps, nfft", RINGS)
@pytest.mark.parametrize("kind, nx, mask", MODELS)
def test_spectra_against_the_restatement(recorded, kind, nx, mask, capacity, steps, nfft):
    from niwqg_amd import lagrangian
    m, P, tr, _ = recorded(kind, nx, mask, capacity, steps)
    if mask == "mask":
        assert m._dual
    assert getattr(m, "_any_size", False) == (nx == 48)
    T = min(capacity, steps + 1)
    assert tr.x.shape == (T, N) and tr.step[0] == steps + 1 - T
    names = ["uv", "q"] + ([] if kind == "qg" else ["phi"])
    worst = 0.0
    for window in ("boxcar", "hann", ARRAY_WINDOW):
        for demean in (True, False):
            for groups in (None, GROUPS3):
                w = window_of(window, T)
                ref = {n: lagrangian.reference_spectrum(tr, n, w, demean, groups, nfft, dt_rec=m.dt) for n in names}
                for chunk in (0, 128):                      # 128: three chunks, the last one of 44
                    S = lagrangian.spectrum(P, None, w, demean, groups, nfft, chunk=chunk)
                    assert sorted(S.values) == sorted(names)
                    assert np.array_equal(S.step, tr.step) and list(S.counts) == ([N] if groups is None else [150, 0, 150])
                    for n in names:
                        omega, want, counts = ref[n]
                        assert np.array_equal(S.omega, omega) and np.array_equal(S.counts, counts)
                        assert S.values[n].shape == ((nfft or T,) if groups is None else (nfft or T, 3))
                        assert np.nansum(S.values[n]) > 0
                        worst = max(worst, rel_err(S.values[n], want))
    print("lagrangian spectra %s %d %s ring %d/%d nfft %s: max |device - numpy| / sum = %.3e" % (kind, nx, mask, T, capacity, nfft, worst))
    assert worst <= 1e-12
    one = lagrangian.spectrum(P, "u", nfft=nfft)
    assert list(one.values) == ["u"] and np.all(np.diff(one.omega) > 0) and len(one.omega) == (nfft or T)


def test_spectrum_against_the_longdouble_restatement(recorded):
    from niwqg_amd import lagrangian
    from niwqg_amd.particles import Trajectory
    m, P, tr, _ = recorded("coupled", 64, "filter", 16, 21)
    ext = Trajectory(tr.step, tr.t, tr.x, tr.y, {"phi": tr.values["phi"].astype(np.clongdouble), "u": tr.values["u"].astype(np.longdouble),
                                                "v": tr.values["v"].astype(np.longdouble)})
    S = lagrangian.spectrum(P, ["phi", "uv"], "hann", True, GROUPS3, chunk=128)
    for n in ("phi", "uv"):
        _, want, _ = lagrangian.reference_spectrum(ext, n, "hann", True, GROUPS3, dt_rec=m.dt)
        assert want.dtype == np.longdouble
        err = rel_err(S.values[n], want)
        print("lagrangian spectrum of %s against the longdouble restatement: %.3e of the sum" % (n, err))
        assert err <= 1e-12


# ---- 2. Parseval ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, nx, mask", MODELS)
def test_parseval(recorded, kind, nx, mask):
    from niwqg_amd import lagrangian
    m, P, tr, _ = recorded(kind, nx, mask, 16, 21)
    w = window_of(ARRAY_WINDOW, 16)
    S = lagrangian.spectrum(P, None, w, True, GROUPS3, nfft=24)
    for n, table in S.values.items():
        x = lagrangian._compose(tr, n)
        xp = x - x.mean(axis=0)[None]
        per = 0.5 * ((w * w)[:, None] * np.abs(xp) ** 2).sum(axis=0) / (w * w).sum()
        for g in (0, 2):
            want = per[GROUPS3 == g].mean()
            err = abs(table[:, g].sum() - want) / want
            print("parseval %s %d %s %s group %d: %.3e" % (kind, nx, mask, n, g, err))
            assert err <= 1e-12


# ---- 3. dispersion against the restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity, steps, nfft", RINGS)
@pytest.mark.parametrize("kind, nx, mask", MODELS)
def test_dispersion_against_the_restatement(recorded, kind, nx, mask, capacity, steps, nfft):
    from niwqg_amd import lagrangian
    m, P, tr, pairs = recorded(kind, nx, mask, capacity, steps)
    worst = 0.0
    for groups in (None, GROUPS3):
        want = lagrangian.reference_dispersion(tr, pairs, groups)
        D = lagrangian.dispersion(P, pairs, groups)
        assert np.array_equal(D.t, tr.t) and np.array_equal(D.step, tr.step) and np.array_equal(D.counts, want["counts"]) and D.npairs == 200
        for key in ("dx", "dy", "A_xx", "A_yy", "A_xy", "A2", "M4", "D_xx", "D_yy", "D_xy", "D2", "S4"):
            a, b = getattr(D, key), want[key]
            assert a.shape == b.shape == ((len(tr.t),) if groups is None or key[0] in "DS" else (len(tr.t), 3)), key
            nan = np.isnan(b)
            assert np.array_equal(np.isnan(a), nan) and (not nan.any() or (groups is not None and nan[:, 1].all() and not nan[:, [0, 2]].any()))
            scale = np.abs(b[~nan]).max()
            assert scale > 0, key
            worst = max(worst, np.abs(a[~nan] - b[~nan]).max() / scale)
        assert np.all(np.nan_to_num(D.A2[0]) == 0) and np.all(D.D2 > 0)
        k = D.kurtosis()
        assert np.allclose(k[1:], D.M4[1:] / D.A2[1:] ** 2, rtol=1e-15, atol=0, equal_nan=True)
        assert np.allclose(D.pair_kurtosis(), D.S4 / D.D2 ** 2, rtol=1e-15, atol=0) and np.all(D.pair_kurtosis() >= 1 - 1e-12)
    print("lagrangian dispersion %s %d %s ring %d/%d: max |device - numpy| / max = %.3e" % (kind, nx, mask, len(tr.t), capacity, worst))
    assert worst <= 1e-12
    alone = lagrangian.dispersion(P)
    assert alone.D2 is None and alone.npairs == 0 and alone.A2.shape == (len(tr.t),)


# ---- 4. autocovariance against the direct sums -----------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity, steps", [(16, 21), (12, 14)])
@pytest.mark.parametrize("kind, nx, mask", MODELS)
def test_autocovariance_against_the_direct_sums(recorded, kind, nx, mask, capacity, steps):
    from niwqg_amd import lagrangian
    m, P, tr, _ = recorded(kind, nx, mask, capacity, steps)
    T = len(tr.t)
    worst = 0.0
    trapz = getattr(np, "trapezoid", None) or np.trapz
    for name in ("uv", "u", "q") + (() if kind == "qg" else ("phi",)):
        for demean, groups, max_lag, chunk in ((True, None, None, 0), (False, GROUPS3, 5, 128)):
            lag, want, counts = lagrangian.reference_autocovariance(tr, name, max_lag, demean, groups, dt_rec=m.dt)
            R = lagrangian.autocovariance(P, name, max_lag, demean, groups, chunk=chunk)
            K = T - 1 if max_lag is None else max_lag
            assert np.array_equal(R.lag, lag) and np.array_equal(R.lag, m.dt * np.arange(K + 1)) and np.array_equal(R.counts, counts)
            assert R.values.shape == want.shape == ((K + 1,) if groups is None else (K + 1, 3))
            assert np.iscomplexobj(R.values) == (name in ("uv", "phi"))
            cols = [slice(None)] if groups is None else [(slice(None), 0), (slice(None), 2)]
            if groups is not None:
                assert np.all(np.isnan(R.values[:, 1])) and np.all(np.isnan(want[:, 1]))
            for c in cols:
                r0 = abs(want[c][0])
                assert r0 > 0 and abs(np.imag(want[c][0])) <= 1e-15 * r0
                worst = max(worst, np.abs(R.values[c] - want[c]).max() / r0)
            kd = R.diffusivity()
            f = 1.0 if name in ("u", "q") else 0.5
            for c in cols:
                ref = np.array([f * trapz(np.real(R.values[c][:k + 1]), R.lag[:k + 1]) for k in range(K + 1)])
                assert np.allclose(kd[c], ref, rtol=1e-13, atol=1e-15 * np.abs(ref).max())
    print("lagrangian autocovariance %s %d %s T = %d: max |device - direct sums| / R(0) = %.3e" % (kind, nx, mask, T, worst))
    assert worst <= 1e-12


# ---- 5. an exact flow ------------------------------------------------------------------------------------------------------------------
def test_zonal_jet_dispersion_is_ballistic():
    """QGModel 64^2, U = 0.3, psi = 1e4 cos(k y): every particle moves at the constant (U + u(y0), 0), so A2 = <(U + u)^2> tau^2 and
    D2 = <|dr0 + du tau|^2>.  Positions are good to eps = 1e-9 L (test_gpu_particles.test_zonal_jet_with_uniform_flow), so a mean
    of squares of them is good to 2 eps max|d| + eps^2."""
    from niwqg_amd import particles, lagrangian
    m = _euler_model("qg", 64, 1000.0, U=0.3)
    X, Y = np.meshgrid((np.arange(64) + 0.5) * m.L / 64, (np.arange(64) + 0.5) * m.L / 64)
    k = 2 * 2 * np.pi / m.L
    m.set_q(-k * k * 1e4 * np.cos(k * Y))
    x0, y0 = particle_set(m, N)
    y0 = np.fmod(np.abs(y0), m.L)
    P = particles.attach(m, x0, y0, record_every=2, capacity=16, record=("u",))
    m._ctx.step(30)
    rng = np.random.default_rng(5)
    i = rng.integers(0, N, 200)
    j = (i + rng.integers(1, N, 200)) % N
    D = lagrangian.dispersion(P, pairs=(i, j), groups=GROUPS3)
    tau = D.t - D.t[0]
    assert np.allclose(tau, 2000.0 * np.arange(16), rtol=1e-14, atol=0)
    u = velocity(m)[0][:, 0]
    c = 0.3 + interpolate(np.tile(u[:, None], (1, 64)), x0, y0, m.L)
    eps = 1e-9 * m.L
    worst = 0.0
    for g in (0, 2):
        cg = c[GROUPS3 == g]
        bound = 2 * eps * np.abs(cg).max() * tau + eps ** 2
        worst = max(worst, (np.abs(D.A2[:, g] - (cg ** 2).mean() * tau ** 2) / bound).max())
        assert np.all(np.abs(D.A2[:, g] - (cg ** 2).mean() * tau ** 2) <= bound)
        assert np.all(np.abs(D.dx[:, g] - cg.mean() * tau) <= eps)
        assert np.all(D.A_yy[:, g] <= bound) and np.all(np.abs(D.A_xy[:, g]) <= bound)
    sx = (x0[i] - x0[j])[None] + (c[i] - c[j])[None] * tau[:, None]
    sy = (y0[i] - y0[j])[None] * np.ones((16, 1))
    want = (sx ** 2 + sy ** 2).mean(axis=1)
    bound = 2 * eps * np.sqrt(sx ** 2 + sy ** 2).max(axis=1) + eps ** 2
    print("zonal jet: |A2 - <(U + u)^2> tau^2| / bound <= %.3e, |D2 - <|dr0 + du tau|^2>| / bound <= %.3e"
          % (worst, (np.abs(D.D2 - want) / bound).max()))
    assert np.all(np.abs(D.D2 - want) <= bound)
    assert np.all(np.abs(D.D_yy - (sy ** 2).mean(axis=1)) <= bound)


# ---- 6. the Doppler shift is gone along trajectories ---------------------------------------------------------------------------------
def test_no_doppler_shift_along_trajectories():
    """YBJModel without dissipation, q = 0, a uniform flow U = dx / dt: phi-hat(l, k) turns as e^{-i (Omega + k U) t}, a particle moves
    one cell per step (its fractional position in the stencil stays what it was), so the series along it is e^{i k x0 - i Omega t}:
    one line at +Omega, where the recorder of section 5j sees Omega + k U."""
    import niwqg_amd
    from niwqg_amd import particles, lagrangian, _lib
    nx, T, p0 = 64, 16, 3
    kw = notebook_kwargs(nx, False)
    kw.update(U=0.0, nuw=0.0, nu4w=0.0, muw=0.0, use_filter=False)
    probe = niwqg_amd.YBJModel.Model(**kw)
    Om = 0.5 * probe.f * 25 * probe.dk ** 2 / probe.kappa2
    kw["dt"] = 2 * np.pi * p0 / (Om * T)
    kw["U"] = (probe.L / nx) / kw["dt"]
    m = niwqg_amd.YBJModel.Model(**kw)
    m.set_q(np.zeros((nx, nx)))
    ph = np.zeros((nx, nx), complex)
    ph[4, 3] = (0.3 - 0.4j) * nx * nx                      # (l, k) = (4, 3) and (3, 4): kappa^2 = 25 dk^2 both, k_x = 3 and 4
    ph[3, 4] = (0.1 + 0.2j) * nx * nx
    m.set_phi(np.fft.ifft2(ph))
    c = m._ctx
    c._chk(c.L.nq_upload_spectral(c.h, 1, _lib._dptr(np.ascontiguousarray(ph).view(np.float64))), "nq_upload_spectral")
    assert np.array_equal(c.field(_lib.F_PHIH), ph)
    x0, y0 = particle_set(m, N)
    P = particles.attach(m, x0, y0, record_every=1, capacity=T, record=("phi",))
    m._ctx.step(T - 1)
    S = lagrangian.spectrum(P, "phi", "boxcar", demean=False)
    table = S.values["phi"]
    ip = int(np.argmax(table))
    assert abs(S.omega[ip] - Om) <= 1e-12 * Om and S.omega[ip] > 0
    for kx in (3, 4):                                     # where the Eulerian lines would land
        ie = int(np.argmin(np.abs(S.omega - (Om + kx * m.dk * m.U))))
        assert ie != ip and table[ie] < table[ip]
    tr = P.trajectory()
    _, want, _ = lagrangian.reference_spectrum(tr, "phi", "boxcar", False, dt_rec=m.dt)
    assert rel_err(table, want) <= 1e-12
    print("no Doppler shift: share of the power outside the bin of +Omega = %.3e" % (np.delete(table, ip).sum() / table.sum()))


# ---- 7. determinism and no side effects -------------------------------------------------------------------------------------------------
def all_tables(P, pairs):
    from niwqg_amd import lagrangian
    S = lagrangian.spectrum(P, None, "hann", True, GROUPS3, chunk=128)
    R = lagrangian.autocovariance(P, "uv", groups=GROUPS3)
    D = lagrangian.dispersion(P, pairs, GROUPS3)
    out = dict(("S_" + n, v) for n, v in S.values.items())
    out.update(R=R.values, A2=D.A2, M4=D.M4, dx=D.dx, D2=D.D2, S4=D.S4, D_xy=D.D_xy)
    return out


@pytest.mark.parametrize("nx", [64, 48])
def test_two_calls_give_the_same_bits(recorded, nx):
    m, P, tr, pairs = recorded("coupled", nx, "filter", 16, 21)
    a, b = all_tables(P, pairs), all_tables(P, pairs)
    for key in a:
        assert np.array_equal(a[key], b[key], equal_nan=True), key


def test_batched_and_single_steps_give_the_same_tables(recorded):
    m, P, tr, pairs = recorded("coupled", 64, "filter", 16, 21)
    m2, P2 = run("coupled", 64, "filter", 16, 21, batched=False)
    a, b = all_tables(P, pairs), all_tables(P2, pairs)
    for key in a:
        assert np.array_equal(a[key], b[key], equal_nan=True), key
    P2.detach()


@pytest.mark.parametrize("nx", [64, 48])
def test_no_side_effects(nx):
    from niwqg_amd import particles
    A, B = model("coupled", nx), model("coupled", nx)
    x, y = particle_set(A, N)
    PA, PB = (particles.attach(m, x, y, record_every=1, capacity=8, record=("u", "v", "q", "phi")) for m in (A, B))
    i = np.arange(0, N - 1)
    for s in range(13):
        A._step_forward()
        B._step_forward()
        if s in (2, 6, 11):
            all_tables(PA, (i, i + 1))
    for n in ("qh", "phih", "ph"):
        assert np.array_equal(np.array(getattr(A, n)), np.array(getattr(B, n))), n
    for a, b in zip(PA.positions(), PB.positions()):
        assert np.array_equal(a, b)
    ta, tb = PA.trajectory(), PB.trajectory()
    assert np.array_equal(ta.x, tb.x) and np.array_equal(ta.y, tb.y) and np.array_equal(ta.step, tb.step)
    for n in ta.values:
        assert np.array_equal(ta.values[n], tb.values[n]), n


# ---- 8. lifecycle ------------------------------------------------------------------------------------------------------------------------
def test_device_memory_comes_and_goes():
    from niwqg_amd import particles, lagrangian
    m = model("coupled", 64)
    m._step_forward()                         # (what the first step allocates on its own is there before the count)
    b0 = m._ctx.device_bytes()
    x, y = particle_set(m, N)
    P = particles.attach(m, x, y, record_every=1, capacity=8, record=("u", "v", "phi"))
    m._ctx.step(5)
    b1 = m._ctx.device_bytes()
    assert b1 > b0
    lagrangian.dispersion(P)
    b2 = m._ctx.device_bytes()
    assert b2 > b1
    lagrangian.spectrum(P, nfft=12)
    b3 = m._ctx.device_bytes()
    assert b3 >= b2 + 12 * N * 16               # at least the work plane
    lagrangian.spectrum(P, "uv", "boxcar", False, nfft=12, chunk=128)
    lagrangian.dispersion(P)
    assert m._ctx.device_bytes() == b3          # later calls that need no more fit what is there
    # three groups: two more offsets (ints) and 6 records x 2 groups x 6 sums more in the table; everything is allocated again and
    # nothing is left behind
    lagrangian.dispersion(P, groups=GROUPS3)
    assert m._ctx.device_bytes() == b3 + 2 * 4 + 6 * 2 * 6 * 8
    P.detach()
    P.detach()
    assert m._ctx.device_bytes() == b0
    for call in (lambda: lagrangian.spectrum(P), lambda: lagrangian.autocovariance(P, "uv"), lambda: lagrangian.dispersion(P)):
        with pytest.raises(RuntimeError, match="detached"):
            call()


def _c_calls(L, h, T=2, n=4):
    w = np.ones(max(T, 1))
    out = np.empty(64 * 6)
    order, offs = np.arange(n, dtype=np.int32), np.array([0, n], np.int32)
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    return (L.nq_lagr_spectrum(h, 0, T, T, dp(w), 0, 1, ip(order), ip(offs), 0, dp(out)),
            L.nq_lagr_dispersion(h, T, 1, ip(order), ip(offs), 0, None, None, dp(out), None))


def test_refusals_of_the_library():
    from niwqg_amd import particles, lagrangian, _lib
    m = model("qg", 64)
    L, h = _lib.lib(), m._ctx.h
    assert _c_calls(L, h) == (-4, -4)                                       # no particles attached
    x, y = particle_set(m, 4)
    P = particles.attach(m, x, y, record_every=0)
    for call in (lambda: lagrangian.spectrum(P), lambda: lagrangian.autocovariance(P, "u"), lambda: lagrangian.dispersion(P)):
        with pytest.raises(ValueError, match="record_every = 0"):
            call()
    assert _c_calls(L, h) == (-1, -1)
    assert b"record_every = 0" in L.nq_last_error(h)
    P.detach()
    P = particles.attach(m, x, y, record_every=3, capacity=4, record=("u", "q"))
    m._ctx.step(2)
    for call in (lambda: lagrangian.spectrum(P), lambda: lagrangian.autocovariance(P, "u"), lambda: lagrangian.dispersion(P)):
        with pytest.raises(ValueError, match="1 record held"):
            call()
    assert _c_calls(L, h, T=1) == (-1, -1)
    m._ctx.step(1)                                                          # the second record
    assert _c_calls(L, h) == (0, 0)
    assert _c_calls(L, h, T=3) == (-1, -1)                                  # not the number of held records
    with pytest.raises(RuntimeError, match="not recorded"):
        m._ctx.lagr_spectrum(1, 2, 2, np.ones(2), False, 1, np.arange(4, dtype=np.int32), np.array([0, 4], np.int32), 0)
    with pytest.raises(RuntimeError, match="outside"):                     # the library checks the index list itself
        m._ctx.lagr_spectrum(0, 2, 2, np.ones(2), False, 1, np.array([0, 1, 2, 4], np.int32), np.array([0, 4], np.int32), 0)
    with pytest.raises(RuntimeError, match="pair index"):
        m._ctx.lagr_dispersion(2, 1, np.arange(4, dtype=np.int32), np.array([0, 4], np.int32), (np.array([0], np.int32), np.array([4], np.int32)))
    with pytest.raises(ValueError, match="'uv' needs both"):
        lagrangian.spectrum(P, "uv")
    with pytest.raises(ValueError, match="'phi' is not recorded"):
        lagrangian.spectrum(P, "phi")
    assert sorted(lagrangian.spectrum(P).values) == ["q", "u"]
    P.detach()


def test_slab_ranks_refuse():
    import niwqg_amd
    from niwqg_amd import _lib
    m = niwqg_amd.CoupledModel.Model(slab=2, **notebook_kwargs(64, True))
    assert _c_calls(_lib.lib(), m._ctx.sim.ranks[0].h) == (-4, -4)


def test_a_non_finite_particle_turns_its_group_nan():
    """On the any-size path the positions are an engine plane: one particle's coordinate is made NaN there.  Its records are NaN
    from then on (section 5g), so the tables of its group are NaN and those of the other groups stay finite.  On a fused context the
    recipe of test_gpu_particles.test_non_finite_state_turns_particles_nan (a NaN in the state) takes every particle: every table
    is NaN."""
    from niwqg_amd import particles, lagrangian, _lib
    m = model("coupled", 48)
    x, y = particle_set(m, N)
    P = particles.attach(m, x, y, record_every=1, capacity=8, record=("u", "v", "phi"))
    pos = (x + 1j * y).reshape(1, -1)
    pos[0, 7] = np.nan + 1j * y[7]                          # particle 7: group 2 of GROUPS3
    e = P.eng
    e.chk(e.L.nq_any_upload(e.h, P.pos.ptr, _lib._dptr(np.ascontiguousarray(pos).view(np.float64)), pos.size), "nq_any_upload")
    advance(m, 5)
    groups = np.where(np.arange(N) == 7, 1, GROUPS3)        # three groups of 150, 1 and 149: the middle one is the NaN particle
    S = lagrangian.spectrum(P, None, "hann", True, groups)
    D = lagrangian.dispersion(P, groups=groups)
    R = lagrangian.autocovariance(P, "uv", groups=groups)
    assert list(S.counts) == [150, 1, 149]
    for table in list(S.values.values()) + [D.A2[1:], D.M4[1:], D.dx[1:], R.values]:
        assert np.all(np.isnan(table[:, 1])) and np.all(np.isfinite(table[:, [0, 2]]))
    with_it = lagrangian.spectrum(P, "uv", groups=GROUPS3).values["uv"]
    assert np.all(np.isnan(with_it[:, 2])) and np.all(np.isfinite(with_it[:, 0]))       # nothing is filtered silently
    P.detach()
    m = model("coupled", 64)
    q = np.array(m.q)
    q[5, 7] = np.nan
    m.set_q(q)
    P = particles.attach(m, x, y, record_every=1, capacity=4, record=("u", "phi"))
    m._ctx.step(2)
    S = lagrangian.spectrum(P, None, "boxcar", False, GROUPS3)
    assert all(np.all(np.isnan(v)) for v in S.values.values())
    assert np.all(np.isnan(lagrangian.dispersion(P).A2[1:]))
    P.detach()
