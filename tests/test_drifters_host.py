"""CPU-only checks of drifter mode (niwqg_amd/particles.py): the numpy restatement ``rk4_wave`` draws the
exact inertial circle within the Simpson bound and at fourth order, reduces to the step of ``wave=None`` bit for bit, the
``wave=`` argument and the new names are checked before the device is touched, and the header declares the entry points and the
four name codes."""
import os

import numpy as np
import pytest

from test_particles_host import _fake, _models, _NoDevice


def rk4_old(x, y, U0, U1, Ub, dt, L, interpolate):
    """the step of ``wave=None`` (tests/test_gpu_particles.py: rk4), restated here with the interpolation rule passed in"""
    a, b = U0[0] + 1j * U0[1], U1[0] + 1j * U1[1]

    def vel(px, py, which):
        if which == 0:
            w = interpolate(a, px, py, L)
        elif which == 1:
            w = interpolate(b, px, py, L)
        else:
            w = 0.5 * (interpolate(a, px, py, L) + interpolate(b, px, py, L))
        return w.real + Ub, w.imag
    k1 = vel(x, y, 0)
    k2 = vel(x + 0.5 * dt * k1[0], y + 0.5 * dt * k1[1], 2)
    k3 = vel(x + 0.5 * dt * k2[0], y + 0.5 * dt * k2[1], 2)
    k4 = vel(x + dt * k3[0], y + dt * k3[1], 1)
    return (x + dt / 6 * (k1[0] + 2 * k2[0] + 2 * k3[0] + k4[0]), y + dt / 6 * (k1[1] + 2 * k2[1] + 2 * k3[1] + k4[1]))


def circle(z0, Ub, a, A, f0, t):
    """the exact path through (Ub, 0) + a A e^{-i f0 t}, uniform A: z0 + Ub t + (i a A / f0)(e^{-i f0 t} - 1)"""
    return z0 + Ub * t + 1j * a * A / f0 * (np.exp(-1j * f0 * t) - 1.0)


def simpson_bound(a, A, f0, dt, T, L):
    """RK4 on a velocity that does not depend on the position is composite Simpson with h = dt/2: the error after the time T is at
    most a |A| T (f0 dt)^4 / 2880; 1e-12 L for the rounding"""
    return a * abs(A) * T * (f0 * dt) ** 4 / 2880.0 + 1e-12 * L


def _circle_errors(f0dt, Ub=0.03):
    from niwqg_amd import particles
    n, L, f0, a, A = 8, 2 * np.pi * 1e5, 1e-4, 1.5, 0.1 * np.exp(0.7j)
    dt = f0dt / f0
    nsteps = int(round(2 * np.pi / f0dt))                  # one inertial period, to the step
    U = np.zeros((n, n), complex)
    P = np.full((n, n), A)
    x, y = np.array([0.31 * L, 0.0]), np.array([0.72 * L, 0.9 * L])
    z0 = x + 1j * y
    errs = []
    for s in range(nsteps):
        x, y = particles.rk4_wave(x, y, U, U, P, P, Ub, a, f0, s * dt, dt, L)
        t = (s + 1) * dt
        errs.append(np.max(np.abs(x + 1j * y - circle(z0, Ub, a, A, f0, t))))
        assert errs[-1] <= simpson_bound(a, A, f0, dt, t, L), (s, errs[-1])
    return np.array(errs), nsteps


def test_rk4_wave_draws_the_inertial_circle_within_the_simpson_bound():
    e1, n1 = _circle_errors(0.25)
    e2, n2 = _circle_errors(0.125)
    assert n2 == 2 * n1
    assert e1.max() > 1e-4                                 # the bound is not met trivially: the error is far above the rounding
    # halving dt divides the error by 16 (at least 12: the margin is for the rounding floor), after the run and half way round
    print("rk4_wave circle: error after the run %.3e -> %.3e, half way %.3e -> %.3e" % (e1[-1], e2[-1], e1[n1 // 2 - 1], e2[n1 - 1]))
    assert e1[-1] / e2[-1] >= 12 and e1[n1 // 2 - 1] / e2[n1 - 1] >= 12


def test_rk4_wave_with_zero_amplitude_is_the_old_step_bit_for_bit():
    from niwqg_amd import particles
    rng = np.random.default_rng(2)
    n, L = 16, 3.0
    U0, U1 = rng.standard_normal((2, n, n)), rng.standard_normal((2, n, n))
    P0, P1 = rng.standard_normal((2, n, n)) + 1j * rng.standard_normal((2, n, n))
    x, y = rng.uniform(-L, 2 * L, 300), rng.uniform(-L, 2 * L, 300)
    want = rk4_old(x, y, U0, U1, 0.2, 0.05, L, particles.interpolate)
    got = particles.rk4_wave(x, y, U0, U1, P0, P1, 0.2, 0.0, 1.3, 0.4, 0.05, L)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    got = particles.rk4_wave(x, y, U0[0] + 1j * U0[1], U1[0] + 1j * U1[1], P0, P1, 0.2, 0.0, 1.3, 0.4, 0.05, L)      # complex planes
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    moved = particles.rk4_wave(x, y, U0, U1, P0, P1, 0.2, 0.5, 1.3, 0.4, 0.05, L)
    assert np.max(np.abs(moved[0] - want[0])) > 1e-3
    # a NaN coordinate stays NaN
    xn = x.copy()
    xn[3] = np.nan
    out = particles.rk4_wave(xn, y, U0, U1, P0, P1, 0.2, 0.5, 1.3, 0.4, 0.05, L)
    assert np.isnan(out[0][3]) and np.isnan(out[1][3]) and np.all(np.isfinite(np.delete(out[0], 3)))


def test_wave_velocity_is_the_rotated_field():
    from niwqg_amd import particles
    rng = np.random.default_rng(3)
    phi = rng.standard_normal(50) + 1j * rng.standard_normal(50)
    w = particles.wave_velocity(phi, 0.7, 1e-4, 12345.0)
    assert np.max(np.abs(w - 0.7 * phi * np.exp(-1j * 1e-4 * 12345.0))) <= 1e-15


@pytest.mark.parametrize("wave", [0, -1, np.nan, np.inf, "x", True, 0.0, -np.inf, 1j, [1.0]])
def test_wave_argument_errors_are_raised_before_the_device(wave):
    from niwqg_amd import particles
    for m in _models():
        with pytest.raises(ValueError, match="wave"):
            particles.attach(m, [0.0], [0.0], wave=wave)
        assert "_particles" not in m.__dict__


def test_wave_and_its_names_are_for_the_kernel_family_only():
    from niwqg_amd import particles, lagrangian
    qg = _fake("QGModel", _ctx=_NoDevice(), tc=0, t=0.0)
    with pytest.raises(ValueError, match="QGModel has no wave field"):
        particles.attach(qg, [0.0], [0.0], wave=1.0)
    with pytest.raises(ValueError, match="valid names: u, v, q$"):
        particles.attach(qg, [0.0], [0.0], record_every=1, record=("uw",))
    with pytest.raises(ValueError, match="'vw'"):
        particles._names(qg, ("u", "vw"), "sample")
    for m in _models()[:3]:
        assert particles._names(m, ("uw", "vw", "phi"), "sample") == ["uw", "vw", "phi"]
        assert particles.available(m, wave=True) == ["u", "v", "q", "phi", "uw", "vw"]
    assert particles.available(qg, wave=True) == ["u", "v", "q"]
    # the composites need the columns they are made of, and raise as "uv" does
    with pytest.raises(ValueError, match="'uvt' needs 'u' and 'v' and 'uw' and 'vw' recorded"):
        lagrangian.check_names(("u", "v", "uw"), ["uvt"])
    with pytest.raises(ValueError, match="'uvw' needs 'uw' and 'vw' recorded"):
        lagrangian.check_names(("u", "v", "uw"), ["uvw"])
    with pytest.raises(ValueError, match="'uv' needs both"):
        lagrangian.check_names(("u", "uw", "vw"), ["uv"])
    assert lagrangian.check_names(("u", "v", "uw", "vw"), ["uvt", "uvw", "uw"]) == ["uvt", "uvw", "uw"]
    assert lagrangian.available(("u", "v", "phi", "uw", "vw")) == ["uv", "uvw", "uvt", "phi"]
    assert lagrangian.available(("uw", "vw", "q")) == ["uvw", "q"]
    assert lagrangian.available(("u", "uw", "v")) == ["uv", "uw"]


def test_slab_models_are_refused_with_wave():
    from niwqg_amd import particles
    from niwqg_amd.slab import SlabContext
    m = _fake("CoupledModel", _ctx=SlabContext.__new__(SlabContext), tc=0, t=0.0)
    with pytest.raises(NotImplementedError, match="slab"):
        particles.attach(m, [1.0], [2.0], wave=0.5)


def test_reference_composites():
    from niwqg_amd import lagrangian, particles
    rng = np.random.default_rng(5)
    v = {k: rng.standard_normal((6, 3)) for k in ("u", "v", "uw", "vw")}
    tr = particles.Trajectory(np.arange(6), np.arange(6.0), None, None, v)
    assert np.array_equal(lagrangian._compose(tr, "uvw"), v["uw"] + 1j * v["vw"])
    assert np.array_equal(lagrangian._compose(tr, "uvt"), (v["u"] + v["uw"]) + 1j * (v["v"] + v["vw"]))
    del v["vw"]
    with pytest.raises(ValueError, match="needs"):
        lagrangian._compose(tr, "uvt")


def test_header_declares_the_entry_points_and_the_name_codes():
    from niwqg_amd import _abi, _lib, particles
    here = os.path.dirname(os.path.abspath(__file__))
    prototypes, constants, _ = _abi.read(open(os.path.join(os.path.dirname(here), "include", "niwqg_amd.h")).read())
    by_name = {name: (ret, params) for name, ret, params in prototypes}
    ret, params = by_name["nq_particles_wave"]
    assert ret == "int" and [t for t, _ in params] == ["nq_ctx*", "double", "double", "double"]
    assert [n for _, n in params] == ["ctx", "amplitude", "f0", "t0"]
    assert [t for t, _ in by_name["nq_any_particles_rk4_wave"][1]][-3:] == ["double", "double", "double"]
    # nq_particles_attach and nq_any_particles_rk4 keep their signatures
    assert len(by_name["nq_particles_attach"][1]) == 10 and len(by_name["nq_any_particles_rk4"][1]) == 10
    codes = {k: constants[k] for k in ("NQ_PT_UW", "NQ_PT_VW", "NQ_LAGR_UVW", "NQ_LAGR_UVT")}
    assert len(set(codes.values())) == 4 and not set(codes.values()) & {0, 1, 2, 3, 4}         # u, v, q, phi and "uv" keep theirs
    assert particles._CODES["uw"] == _lib.PT_UW == codes["NQ_PT_UW"] and particles._CODES["vw"] == codes["NQ_PT_VW"]
    assert particles._LAGR_CODES["uvw"] == codes["NQ_LAGR_UVW"] and particles._LAGR_CODES["uvt"] == codes["NQ_LAGR_UVT"]
    assert {k: particles._LAGR_CODES[k] for k in ("u", "v", "q", "phi", "uv")} == dict(u=0, v=1, q=2, phi=3, uv=4)


def test_entries_are_exported_and_refuse_null():
    import niwqg_amd
    niwqg_amd.build()
    from niwqg_amd import _lib
    L = _lib.lib()
    for name in ("nq_particles_wave", "nq_particles_clock", "nq_any_particles_rk4_wave", "nq_any_interp_wave"):
        assert name in _lib.EXPORTS and getattr(L, name).argtypes is not None, name
    assert L.nq_particles_wave(None, 1.0, 1e-4, 0.0) != 0
    assert L.nq_particles_clock(None, 1e-4, 0.0) != 0
    assert L.nq_any_particles_rk4_wave(None, None, 1, None, None, None, None, 8, 1.0, 1.0, 0.0, 1.0, 1.0, 1e-4, 0.0) == -1
    assert L.nq_any_interp_wave(None, None, None, None, 1, 8, 1.0, 1.0, 1.0, 1e-4, 0.0) == -1
