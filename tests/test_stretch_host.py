"""CPU-only checks of stretch mode (niwqg_amd/particles.py): the numpy restatement ``rk4_tangent`` carries the
exact Jacobian of the discrete position map (against central differences of neighbouring runs, with and without the wave
velocity), integrates a shear exactly, finds e^{+-T} at a hyperbolic point and keeps det F = 1 to second order in dx; ``ln_sigma``
against the SVD; ``lattice``; the argument checks before the device is touched; the header's entry points and name codes.

Flows on a 2 pi box, n = 64 and 128, 257 random particles, dt = 0.05, 40 steps (T = 2).  Every figure is printed before it is
asserted (-s shows them); the bars are those of the feature's specification.
"""
import os

import numpy as np
import pytest

from test_particles_host import _fake, _models, _NoDevice

L = 2 * np.pi
NP, DT, STEPS = 257, 0.05, 40
T_END = DT * STEPS


def grid(n):
    """coordinates of the grid values: [j, i] at ((i + 1/2) dx, (j + 1/2) dy)"""
    c = (np.arange(n) + 0.5) * (L / n)
    return np.meshgrid(c, c)


def cellular(n):
    """u + i v of psi = sin x sin y: u = -psi_y, v = psi_x"""
    X, Y = grid(n)
    return -np.sin(X) * np.cos(Y) + 1j * (np.cos(X) * np.sin(Y))


def wave_planes(n):
    """a smooth periodic phi at the start and at the end of a step (it turns and grows a little in between)"""
    X, Y = grid(n)
    p0 = (0.3 + 0.2 * np.cos(X) + 0.1 * np.sin(2 * Y)) + 1j * (0.1 * np.sin(X + Y) - 0.2 * np.cos(Y))
    return p0, p0 * (1.01 * np.exp(0.02j))


def start(seed=5):
    rng = np.random.default_rng(seed)
    return rng.uniform(0, L, NP), rng.uniform(0, L, NP)


def run(x, y, U, Ub=0.0, **wave):
    from niwqg_amd import particles
    F = np.tile(np.eye(2), (len(x), 1, 1))
    for s in range(STEPS):
        x, y, F = particles.rk4_tangent(x, y, F, U, U, Ub, DT, L, t=s * DT, **wave)
    return x, y, F


def fd_jacobian(x0, y0, U, eps=1e-5, **wave):
    """central differences of the final positions of runs started at x0 +- eps and y0 +- eps"""
    J = np.empty((len(x0), 2, 2))
    for col, (dx, dy) in enumerate(((eps, 0.0), (0.0, eps))):
        xp, yp, _ = run(x0 + dx, y0 + dy, U, **wave)
        xm, ym, _ = run(x0 - dx, y0 - dy, U, **wave)
        J[:, 0, col] = (xp - xm) / (2 * eps)
        J[:, 1, col] = (yp - ym) / (2 * eps)
    return J


@pytest.mark.parametrize("n", [64, 128])
def test_F_is_the_exact_jacobian_of_the_discrete_map(n):
    U = cellular(n)
    x0, y0 = start()
    _, _, F = run(x0, y0, U)
    err, big = np.max(np.abs(F - fd_jacobian(x0, y0, U))), np.max(np.abs(F))
    print("n = %d: max |F - central differences| = %.3e, max |F| = %.3f" % (n, err, big))
    assert big > 2.0                                      # the flow did stretch
    assert err <= 1e-5 * big


@pytest.mark.parametrize("n", [64, 128])
def test_F_is_the_exact_jacobian_with_the_wave_velocity(n):
    """drifter + stretch: the same check with a != 0 on a smooth periodic phi; det F leaves 1"""
    U = cellular(n)
    P0, P1 = wave_planes(n)
    wave = dict(P0=P0, P1=P1, a=0.5, f0=3.0)
    x0, y0 = start(6)
    _, _, F = run(x0, y0, U, **wave)
    err, big = np.max(np.abs(F - fd_jacobian(x0, y0, U, **wave))), np.max(np.abs(F))
    from niwqg_amd import particles
    print("n = %d, a = 0.5: max |F - central differences| = %.3e, max |F| = %.3f, max |det F - 1| = %.3e"
          % (n, err, big, np.max(np.abs(particles.det(F) - 1))))
    assert err <= 1e-5 * big
    assert np.max(np.abs(particles.det(F) - 1)) > 1e-2    # the drifter velocity is compressible


@pytest.mark.parametrize("n", [64, 128])
def test_shear_is_integrated_exactly(n):
    """u = sin y, Ub = 0.3: A = [[0, u_y], [0, 0]] is nilpotent and constant along the path, RK4 is exact"""
    from niwqg_amd import particles
    _, Y = grid(n)
    U = np.sin(Y) + 0j
    x0, y0 = start(7)
    _, _, F = run(x0, y0, U, Ub=0.3)
    uy = particles.interpolate_d(U, x0, y0, L)[2].real
    e12 = np.max(np.abs(F[:, 0, 1] - T_END * uy))
    rest = max(np.max(np.abs(F[:, 0, 0] - 1)), np.max(np.abs(F[:, 1, 0])), np.max(np.abs(F[:, 1, 1] - 1)))
    print("n = %d: max |F12 - T u_y| = %.3e, the other entries off the identity by %.3e" % (n, e12, rest))
    assert np.max(np.abs(F[:, 0, 1])) > 1.0
    assert e12 <= 1e-12
    assert rest <= 1e-14


def test_hyperbolic_point_stretches_at_the_strain_rate():
    """the origin of the cellular flow: u = -x, v = y to first order, F = diag(e^-T, e^T)"""
    U = cellular(64)
    x, y, F = run(np.zeros(1), np.zeros(1), U)
    print("F11 e^T = %.6f, F22 e^-T = %.6f, the point moved by %.1e" % (F[0, 0, 0] * np.exp(T_END), F[0, 1, 1] * np.exp(-T_END), np.hypot(x, y)[0]))
    assert abs(F[0, 1, 1] / np.exp(T_END) - 1) <= 0.01
    assert abs(F[0, 0, 0] / np.exp(-T_END) - 1) <= 0.01


def test_determinant_converges_at_second_order():
    """the interpolated velocity is solenoidal to second order only: max |det F - 1| falls by 3 or more from n = 64 to 128"""
    from niwqg_amd import particles
    x0, y0 = start()
    d = [np.max(np.abs(particles.det(run(x0, y0, cellular(n))[2]) - 1)) for n in (64, 128)]
    print("max |det F - 1|: %.3e (n = 64) -> %.3e (n = 128), x%.2f" % (d[0], d[1], d[0] / d[1]))
    assert d[0] >= 3 * d[1]


def test_ln_sigma_is_the_largest_singular_value():
    from niwqg_amd import particles
    rng = np.random.default_rng(2)
    F = rng.standard_normal((2000, 2, 2)) * np.exp(rng.uniform(-3, 3, (2000, 1, 1)))
    want = np.log(np.linalg.svd(F, compute_uv=False)[:, 0])
    got = particles.ln_sigma(F)
    rel = np.max(np.abs(got - want) / np.abs(want))
    print("ln_sigma against the SVD: %.3e relative" % rel)
    assert rel <= 1e-13
    near = np.eye(2) + 1e-9 * rng.standard_normal((2000, 2, 2))
    err = np.max(np.abs(particles.ln_sigma(near) - np.log(np.linalg.svd(near, compute_uv=False)[:, 0])))
    print("near the identity: %.3e absolute" % err)
    assert err <= 1e-13
    assert particles.ln_sigma(np.eye(2)) == 0.0 and particles.det(np.eye(2)) == 1.0
    assert particles.ln_sigma(F).shape == (2000,) and particles.ln_sigma(F.reshape(40, 50, 2, 2)).shape == (40, 50)


def test_lattice_is_row_major_at_box_centres():
    from niwqg_amd import particles
    m = _fake("CoupledModel", L=8.0, W=4.0)
    x, y = particles.lattice(m, 4)
    assert x.shape == y.shape == (16,)
    assert np.array_equal(x.reshape(4, 4)[0], [1.0, 3.0, 5.0, 7.0]) and np.array_equal(y.reshape(4, 4)[:, 0], [0.5, 1.5, 2.5, 3.5])
    assert np.all(x.reshape(4, 4) == x.reshape(4, 4)[0][None]) and np.all(y.reshape(4, 4) == y.reshape(4, 4)[:, :1])
    for bad in (0, 2.5, True):
        with pytest.raises(ValueError, match="lattice"):
            particles.lattice(m, bad)


def test_stretch_arguments_are_checked_before_the_device():
    from niwqg_amd import particles
    from niwqg_amd.slab import SlabContext
    good = (np.array([1.0]), np.array([2.0]))
    for m in _models():                                   # every class, QGModel included
        with pytest.raises(ValueError, match="shape"):
            particles.attach(m, [0.0], [0.0], stretch=np.eye(2))
        with pytest.raises(ValueError, match="shape"):
            particles.attach(m, [0.0, 1.0], [0.0, 1.0], stretch=np.ones((1, 2, 2)))
        with pytest.raises(ValueError, match="non-finite"):
            particles.attach(m, [0.0], [0.0], stretch=np.array([[[1.0, 0.0], [np.nan, 1.0]]]))
        with pytest.raises(ValueError, match="non-finite"):
            particles.attach(m, [0.0], [0.0], stretch=np.array([[[1.0, np.inf], [0.0, 1.0]]]))
        with pytest.raises(ValueError, match="real numbers"):
            particles.attach(m, [0.0], [0.0], stretch="yes")
        with pytest.raises(ValueError, match="'f11', 'det' need stretch mode"):
            particles.attach(m, [0.0], [0.0], record_every=1, record=("u", "f11", "det"))
        with pytest.raises(ValueError, match="'lnsigma' need stretch mode"):
            particles._names(m, ("u", "lnsigma"), "sample", False, False)
        assert particles._names(m, particles.STRETCH_NAMES, "sample", False, True) == list(particles.STRETCH_NAMES)
        assert particles.available(m, stretch=True)[-6:] == ["f11", "f12", "f21", "f22", "lnsigma", "det"]
        assert not set(particles.STRETCH_NAMES) & set(particles.available(m, wave=True, rays=True))
    for m in _models()[:3]:                               # ray mode and stretch mode exclude each other
        with pytest.raises(ValueError, match="rays= and stretch= exclude each other"):
            particles.attach(m, [0.0], [0.0], rays=good, eta=1.0, stretch=True)
    assert particles.available(_models()[3], stretch=True) == ["u", "v", "q", "f11", "f12", "f21", "f22", "lnsigma", "det"]
    s = _fake("CoupledModel", _ctx=SlabContext.__new__(SlabContext), tc=0, t=0.0)
    with pytest.raises(NotImplementedError, match="slab"):
        particles.attach(s, [1.0], [2.0], stretch=True)
    # Lagrangian spectra of the new columns are out of scope: refused by name, and left out of the default list
    from niwqg_amd import lagrangian
    assert lagrangian.available(("u", "v", "f11", "f12", "f21", "f22", "lnsigma", "det")) == ["uv"]
    with pytest.raises(ValueError, match="unknown name 'lnsigma'"):
        lagrangian.check_names(("u", "lnsigma"), ["lnsigma"])


def test_header_declares_the_stretch_entry_points_and_codes():
    from niwqg_amd import _abi, _lib, particles
    here = os.path.dirname(os.path.abspath(__file__))
    prototypes, constants, _ = _abi.read(open(os.path.join(os.path.dirname(here), "include", "niwqg_amd.h")).read())
    by_name = {name: (ret, params) for name, ret, params in prototypes}
    ret, params = by_name["nq_particles_tangent"]
    assert ret == "int" and [t for t, _ in params] == ["nq_ctx*", "const double*"]
    assert [t for t, _ in by_name["nq_particles_get_tangent"][1]] == ["nq_ctx*", "double*"]
    assert [t for t, _ in by_name["nq_particles_tangent_reset"][1]] == ["nq_ctx*"]
    assert [t for t, _ in by_name["nq_lagr_stretching"][1]] == ["nq_ctx*", "int", "int", "const int*", "const int*", "double*"]
    for name in ("nq_any_particles_rk4_tangent", "nq_any_particles_rk4_wave_tangent", "nq_any_lagr_stretching"):
        assert name in by_name
    names = ("f11", "f12", "f21", "f22", "lnsigma", "det")
    codes = [constants["NQ_PT_" + n.upper()] for n in names]
    assert codes == [13, 14, 15, 16, 17, 18] and constants["NQ_PT_OMEGA"] == 12          # the enum goes on after omega
    assert [particles._CODES[n] for n in names] == codes
    assert len(set(particles._CODES.values())) == len(particles._CODES)
    assert not set(names) & set(particles._LAGR_CODES)


def test_stretch_entries_are_exported_and_refuse_null():
    import niwqg_amd
    niwqg_amd.build()
    from niwqg_amd import _lib
    Lb = _lib.lib()
    for name in ("nq_particles_tangent", "nq_particles_get_tangent", "nq_particles_tangent_reset", "nq_particles_tangent_step0",
                 "nq_lagr_stretching", "nq_any_particles_rk4_tangent", "nq_any_particles_rk4_wave_tangent", "nq_any_tangent_value",
                 "nq_any_lagr_stretching"):
        assert name in _lib.EXPORTS and getattr(Lb, name).argtypes is not None, name
    assert Lb.nq_particles_tangent(None, None) != 0
    assert Lb.nq_particles_get_tangent(None, None) != 0
    assert Lb.nq_particles_tangent_reset(None) != 0
    assert Lb.nq_particles_tangent_step0(None, None) != 0
    assert Lb.nq_lagr_stretching(None, 2, 1, None, None, None) != 0
    assert Lb.nq_any_particles_rk4_tangent(None, None, None, None, 1, None, None, 8, 1.0, 1.0, 0.0, 1.0) == -1
    assert Lb.nq_any_particles_rk4_wave_tangent(None, None, None, None, 1, None, None, None, None, 8, 1.0, 1.0, 0.0, 1.0, 1.0, 1.0, 0.0) == -1
    assert Lb.nq_any_tangent_value(None, None, None, None, 1, 0) == -1
    assert Lb.nq_any_lagr_stretching(None, 1, 2, None, 2, 1, None, None, None) == -1
