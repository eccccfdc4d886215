"""CPU-only checks of ray mode (niwqg_amd/particles.py): the derivative weights of the Keys interpolant, the
numpy restatement ``rk4_rays`` on zero flow, on x-uniform planes, with eta = 0 and on a steady random flow, where the drift of the
interpolated omega falls at second order or better when dt is halved; the argument checks before the device is touched; the
header's entry points and name codes.

The steady flow (``steady_flow``: modes |kappa| <= 4, max |u| = 0.1 m/s on the notebook's domain), its rays (``ray_set``) and the
time steps DT_OMEGA -> DT_OMEGA / 2 over T_OMEGA are shared with tests/test_gpu_rays.py.  Observed with numpy (-s prints them):
  omega drift (rms over 2000 rays) over 3e5 s at dt = 1e4 -> 5e3 s     5.689e-12 -> 1.400e-12 1/s (x4.06; |omega| up to 9.4e-6:
                                                                        1.5e-7 relative, rounding 2e-16)
  k in x-uniform planes after 100 steps                                 max |k - k0| / |k0| = 9.6e-16, while l moved by 21 |l0| at most
"""
import os

import numpy as np
import pytest

from test_particles_host import _fake, _models, _NoDevice
from test_drifters_host import rk4_old

L = 2 * np.pi * 200e3                                     # the notebook's domain and wave parameters (tests/test_oracle_golden.py)
F0, MZ, NB = 1e-4, 2 * np.pi / 280.0, 0.01
ETA = F0 / (MZ * F0 / NB) ** 2                            # hslash = f / kappa^2
K0 = 10 * 2 * np.pi / L
DT_OMEGA, T_OMEGA = 1e4, 3e5                              # 30 and 60 steps


def steady_flow(nx, seed=3, umax=0.1, kmax=4):
    """(q, u, v) of a random streamfunction with modes 0 < |kappa| <= kmax: q its Laplacian (zeta), max(|u|, |v|) = umax"""
    rng = np.random.default_rng(seed)
    n = np.fft.fftfreq(nx, 1.0 / nx)
    kx, ly = np.meshgrid(n, n)
    kap2 = kx ** 2 + ly ** 2
    ph = np.fft.fft2(rng.standard_normal((nx, nx))) * ((kap2 > 0) & (kap2 <= kmax ** 2))
    dk = 2 * np.pi / L
    u, v = np.fft.ifft2(-1j * ly * dk * ph).real, np.fft.ifft2(1j * kx * dk * ph).real
    s = umax / max(np.abs(u).max(), np.abs(v).max())
    return np.fft.ifft2(-kap2 * dk * dk * ph).real * s, u * s, v * s


def ray_set(n, seed=11):
    """n rays anywhere in the domain, wavenumbers 0.3 K0 .. K0 in every direction"""
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(0, L, n), rng.uniform(0, L, n)
    th, r = rng.uniform(0, 2 * np.pi, n), K0 * rng.uniform(0.3, 1.0, n)
    return x, y, r * np.cos(th), r * np.sin(th)


# ---- the derivative weights ----------------------------------------------------------------------------------------------------
def test_keys_dweights_are_the_derivative_of_keys_weights():
    from niwqg_amd import particles
    t = np.random.default_rng(0).uniform(0.0, 1.0, 2000)
    dw = particles.keys_dweights(t)
    h = 1e-5                                              # central differences of cubics: error h^2 |w'''| / 6 <= 1.5e-10, rounding 1e-11
    lo, hi = particles.keys_weights(t - h), particles.keys_weights(t + h)
    for o in range(4):
        assert np.max(np.abs((hi[o] - lo[o]) / (2 * h) - dw[o])) <= 1e-9
    assert np.max(np.abs(dw[0] + dw[1] + dw[2] + dw[3])) <= 4e-16 * 5                      # they sum to 0 (|w'| <= 5/4 each ... 5 ulps)
    assert np.max(np.abs((-dw[0] + dw[2] + 2 * dw[3]) - 1.0)) <= 1e-15                     # sum o_i w'_i = 1: a linear ramp has slope 1
    # the end points: the interpolant is C^1, w'(1) of one cell is w'(0) of the next, shifted by one node
    a, b = particles.keys_dweights(1.0), particles.keys_dweights(0.0)
    assert [float(v) for v in a] == [0.0] + [float(v) for v in b[:3]] and float(b[3]) == 0.0


def test_interpolate_d_is_the_gradient_of_interpolate():
    from niwqg_amd import particles
    rng = np.random.default_rng(1)
    n, Lx = 16, 3.0
    plane = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    x, y = rng.uniform(-Lx, 2 * Lx, 400), rng.uniform(-Lx, 2 * Lx, 400)
    f, fx, fy = particles.interpolate_d(plane, x, y, Lx)
    assert np.array_equal(f, particles.interpolate(plane, x, y, Lx))                       # the same sums in the same order
    h = 1e-6
    dx = (particles.interpolate(plane, x + h, y, Lx) - particles.interpolate(plane, x - h, y, Lx)) / (2 * h)
    dy = (particles.interpolate(plane, x, y + h, Lx) - particles.interpolate(plane, x, y - h, Lx)) / (2 * h)
    # (second differences of a C^1 piecewise cubic: h |f''| ~ 1e-6 (n / L)^2 |f| where a cell face lies inside the difference)
    scale = np.abs(plane).max() * (n / Lx)
    assert np.max(np.abs(fx - dx)) <= 1e-4 * scale and np.max(np.abs(fy - dy)) <= 1e-4 * scale
    assert np.max(np.abs(fx)) > 0.1 * scale
    out = particles.interpolate_d(plane, np.array([np.nan, 1.0]), np.array([1.0, np.inf]), Lx)
    assert all(np.all(np.isnan(o)) for o in out)


# ---- rk4_rays ------------------------------------------------------------------------------------------------------------------
def test_zero_flow_moves_the_ray_at_its_group_velocity():
    from niwqg_amd import particles
    n, nsteps, dt, Ub = 16, 25, 1e4, -0.1
    Z = np.zeros((n, n))
    U = np.zeros((n, n), complex)
    x0, y0, k0, l0 = ray_set(300)
    x, y, k, l = x0, y0, k0, l0
    for _ in range(nsteps):
        x, y, k, l = particles.rk4_rays(x, y, k, l, U, U, Z, Z, Ub, ETA, dt, L)
    assert np.array_equal(k, k0) and np.array_equal(l, l0)                                 # bit for bit
    t = nsteps * dt
    assert np.max(np.abs(x - x0 - (Ub + ETA * k0) * t)) <= 1e-13 * L and np.max(np.abs(y - y0 - ETA * l0 * t)) <= 1e-13 * L
    assert np.max(np.abs(x - x0)) > 1e-3 * L


def test_k_is_conserved_in_x_uniform_planes():
    from niwqg_amd import particles
    n, dt = 64, 1e4
    rng = np.random.default_rng(4)
    yy = (np.arange(n) + 0.5) * L / n
    prof = sum(rng.standard_normal() * np.sin(2 * np.pi * j * yy / L + rng.uniform(0, 6)) for j in (1, 2, 3))
    u = np.repeat((0.1 * prof / np.abs(prof).max())[:, None], n, axis=1)
    q = -np.gradient(u, L / n, axis=0)                                                      # zeta = -u_y: depends on y only
    U = u + 0j
    x, y, k0, l0 = ray_set(300)
    k, l = k0, l0
    for _ in range(100):
        x, y, k, l = particles.rk4_rays(x, y, k, l, U, U, q, q, 0.0, ETA, dt, L)
    print("x-uniform planes: max |k - k0| / |k0| = %.3e, max |l - l0| / |l0| = %.3e" % (np.max(np.abs(k - k0) / np.abs(k0)), np.max(np.abs(l - l0) / np.abs(l0))))
    assert np.all(np.abs(k - k0) <= 1e-14 * np.abs(k0))
    assert np.max(np.abs(l - l0) / np.abs(l0)) > 1e-3


def test_eta_zero_gives_the_positions_of_plain_particles():
    from niwqg_amd import particles
    rng = np.random.default_rng(2)
    n, nsteps, dt = 32, 20, 1e4
    q0, u0, v0 = steady_flow(n, seed=6)
    q1, u1, v1 = steady_flow(n, seed=7)
    x0, y0, k0, l0 = ray_set(300)
    x, y, k, l = x0, y0, k0, l0
    xo, yo = x0, y0
    xw, yw = x0, y0
    P = rng.standard_normal((n, n)) + 0j
    for s in range(nsteps):
        x, y, k, l = particles.rk4_rays(x, y, k, l, (u0, v0), (u1, v1), q0, q1, -0.1, 0.0, dt, L)
        xo, yo = rk4_old(xo, yo, (u0, v0), (u1, v1), -0.1, dt, L, particles.interpolate)
        xw, yw = particles.rk4_wave(xw, yw, (u0, v0), (u1, v1), P, P, -0.1, 0.0, F0, s * dt, dt, L)
    assert max(np.max(np.abs(x - xo)), np.max(np.abs(y - yo))) <= 1e-13 * L
    assert max(np.max(np.abs(x - xw)), np.max(np.abs(y - yw))) <= 1e-13 * L
    assert np.max(np.abs(k - k0) / np.abs(k0)) > 1e-3                                      # the wavevector evolves nevertheless
    assert np.max(np.hypot(x - x0, y - y0)) > 1e-3 * L


N_OMEGA = 2000


def rms(a):
    return float(np.sqrt(np.mean(np.square(a))))


def omega_drift(nx, dt, T=T_OMEGA, n=N_OMEGA, Ub=-0.1):
    """the drift: the rms over the rays of omega(T) - omega(0) of the interpolated omega on the steady flow; and max |omega(0)|.
    The drift of one ray is a sum of kicks where it crosses a cell face (w'' jumps there), of either sign: the largest of a few
    hundred is an extreme value that scatters by a factor of 3 between ray sets (its ratio under halving went from 2.0 to 6.9 in
    numpy), the rms over 2000 rays is the ensemble's (3.4 to 4.5 over four ray sets and three flows)."""
    from niwqg_amd import particles
    q, u, v = steady_flow(nx)
    U = u + 1j * v
    x, y, k, l = ray_set(n)
    w0 = particles.ray_omega_at(x, y, k, l, U, q, Ub, ETA, L)
    for _ in range(int(round(T / dt))):
        x, y, k, l = particles.rk4_rays(x, y, k, l, U, U, q, q, Ub, ETA, dt, L)
    return rms(particles.ray_omega_at(x, y, k, l, U, q, Ub, ETA, L) - w0), np.max(np.abs(w0))


def test_omega_drift_falls_when_dt_is_halved():
    """the discrete rays are Hamilton's equations of the interpolated omega: on a steady flow its drift is the time stepping's
    alone, second order at least (w'' jumps at cell faces; 4 is the asymptote of the ratio)"""
    d1, top = omega_drift(64, DT_OMEGA)
    d2, _ = omega_drift(64, DT_OMEGA / 2)
    print("omega drift over %.0e s: dt = %.0e: %.3e, dt = %.0e: %.3e (x%.2f); max |omega| = %.3e" % (T_OMEGA, DT_OMEGA, d1, DT_OMEGA / 2, d2, d1 / d2, top))
    assert d2 >= 1e3 * np.finfo(float).eps * top                                           # far above the rounding: the ratio is seen
    assert d1 / d2 >= 2.5


def test_rk4_rays_keeps_nan_and_takes_steady_planes():
    from niwqg_amd import particles
    q, u, v = steady_flow(16)
    x, y, k, l = ray_set(20)
    x = x.copy()
    x[3] = np.nan
    k = k.copy()
    k[5] = np.inf
    out = particles.rk4_rays(x, y, k, l, (u, v), (u, v), q, q, 0.0, ETA, 1e4, L)
    for o in out:
        assert np.isnan(o[3]) and np.isnan(o[5]) and np.all(np.isfinite(np.delete(o, [3, 5])))
    # `is`-steady planes and equal copies give the same step up to the rounding of the mean (a + a) / 2 = a: bit for bit
    U = u + 1j * v
    a = particles.rk4_rays(y, y, l, l, U, U, q, q, 0.1, ETA, 1e4, L)
    b = particles.rk4_rays(y, y, l, l, U, U.copy(), q, q.copy(), 0.1, ETA, 1e4, L)
    assert all(np.array_equal(p, r) for p, r in zip(a, b))


def test_ray_omega_is_the_dispersion_relation():
    from niwqg_amd import particles
    rng = np.random.default_rng(8)
    u, v, z, k, l = rng.standard_normal((5, 40))
    want = (u - 0.3) * k + v * l + z / 2 + 0.7 / 2 * (k ** 2 + l ** 2)
    assert np.max(np.abs(particles.ray_omega(u, v, z, k, l, -0.3, 0.7) - want)) <= 1e-14


# ---- arguments, before the device is touched -----------------------------------------------------------------------------------
@pytest.mark.parametrize("rays, eta, match", [
    (([1.0, 2.0], [1.0]), 1.0, "shapes"),
    (([1.0], [1.0]), 1.0, "shapes"),
    (([1.0, np.nan], [1.0, 2.0]), 1.0, "non-finite"),
    (([1.0, 2.0], [np.inf, 2.0]), 1.0, "non-finite"),
    ((np.zeros((2, 1)), np.zeros((2, 1))), 1.0, "shapes"),
    (([1.0, 2.0],), 1.0, "rays = "),
    (5.0, 1.0, "rays = "),
    (([1.0, 2.0], [1.0, 2.0]), np.nan, "eta"),
    (([1.0, 2.0], [1.0, 2.0]), "x", "eta"),
    (None, 1.0, "without rays"),
])
def test_ray_argument_errors_are_raised_before_the_device(rays, eta, match):
    from niwqg_amd import particles
    for m in _models()[:3]:
        with pytest.raises(ValueError, match=match):
            particles.attach(m, [0.0, 1.0], [0.0, 1.0], rays=rays, eta=eta)
        assert "_particles" not in m.__dict__


def test_rays_exclude_wave_qg_and_slabs_and_own_their_names():
    from niwqg_amd import particles
    from niwqg_amd.slab import SlabContext
    good = ([1e-5], [2e-5])
    for m in _models()[:3]:
        with pytest.raises(ValueError, match="exclude each other"):
            particles.attach(m, [0.0], [0.0], wave=1.0, rays=good, eta=1.0)
        with pytest.raises(ValueError, match="need ray mode"):
            particles.attach(m, [0.0], [0.0], record_every=1, record=("u", "omega"))
        with pytest.raises(ValueError, match="'k', 'l' need ray mode"):
            particles._names(m, ("k", "zeta", "l"), "sample", False)
        assert particles._names(m, ("k", "l", "zeta", "omega"), "sample", True) == ["k", "l", "zeta", "omega"]
        assert particles._names(m, ("zeta",), "sample", False) == ["zeta"]                  # zeta needs no mode
        assert particles.available(m, rays=True) == ["u", "v", "q", "phi", "zeta", "k", "l", "omega"]
        assert particles.available(m) == ["u", "v", "q", "phi"]
    qg = _models()[3]
    with pytest.raises(ValueError, match="QGModel has no near-inertial waves"):
        particles.attach(qg, [0.0], [0.0], rays=good, eta=1.0)
    with pytest.raises(ValueError, match="valid names: u, v, q$"):
        particles.attach(qg, [0.0], [0.0], record_every=1, record=("zeta",))
    assert particles.available(qg, rays=True) == ["u", "v", "q"]
    # Lagrangian spectra of the new columns are out of scope: refused by name, and left out of the default list
    from niwqg_amd import lagrangian
    assert lagrangian.available(("u", "v", "k", "l", "zeta", "omega", "phi")) == ["uv", "phi"]
    with pytest.raises(ValueError, match="unknown name 'omega'"):
        lagrangian.check_names(("u", "omega"), ["omega"])
    s = _fake("CoupledModel", _ctx=SlabContext.__new__(SlabContext), tc=0, t=0.0)
    with pytest.raises(NotImplementedError, match="slab"):
        particles.attach(s, [1.0], [2.0], rays=good, eta=1.0)


def test_header_declares_the_ray_entry_points_and_codes():
    from niwqg_amd import _abi, _lib, particles
    here = os.path.dirname(os.path.abspath(__file__))
    prototypes, constants, _ = _abi.read(open(os.path.join(os.path.dirname(here), "include", "niwqg_amd.h")).read())
    by_name = {name: (ret, params) for name, ret, params in prototypes}
    ret, params = by_name["nq_particles_rays"]
    assert ret == "int" and [t for t, _ in params] == ["nq_ctx*", "const double*", "const double*", "double"]
    assert [t for t, _ in by_name["nq_particles_get_rays"][1]] == ["nq_ctx*", "double*", "double*"]
    assert "nq_any_particles_rk4_rays" in by_name and "nq_any_interp_omega" in by_name
    codes = [constants[k] for k in ("NQ_PT_K", "NQ_PT_L", "NQ_PT_ZETA", "NQ_PT_OMEGA")]
    taken = {0, 1, 2, 3, 4, constants["NQ_PT_UW"], constants["NQ_PT_VW"], constants["NQ_LAGR_UVW"], constants["NQ_LAGR_UVT"]}
    assert len(set(codes)) == 4 and not set(codes) & taken                                 # unused codes
    assert [particles._CODES[n] for n in ("k", "l", "zeta", "omega")] == codes == [_lib.PT_K, _lib.PT_L, _lib.PT_ZETA, _lib.PT_OMEGA]
    assert not set(("k", "l", "zeta", "omega")) & set(particles._LAGR_CODES)                # Lagrangian spectra of them: out of scope


def test_ray_entries_are_exported_and_refuse_null():
    import niwqg_amd
    niwqg_amd.build()
    from niwqg_amd import _lib
    Lb = _lib.lib()
    for name in ("nq_particles_rays", "nq_particles_get_rays", "nq_any_particles_rk4_rays", "nq_any_interp_omega"):
        assert name in _lib.EXPORTS and getattr(Lb, name).argtypes is not None, name
    assert Lb.nq_particles_rays(None, None, None, 1.0) != 0
    assert Lb.nq_particles_get_rays(None, None, None) != 0
    assert Lb.nq_any_particles_rk4_rays(None, None, None, 1, None, None, None, None, 8, 1.0, 1.0, 0.0, 1.0, 1.0) == -1
    assert Lb.nq_any_interp_omega(None, None, None, None, None, None, 1, 8, 1.0, 1.0, 0.0, 1.0) == -1
