"""CPU-only checks of the Lagrangian-particle module (niwqg_amd/particles.py): every refusal is raised before the device is
touched, slab models are refused, the C entries are exported and typed, and the numpy restatement of the interpolation rule
has the properties the device kernels are specified by (exact at nodes, periodic, third order, NaN-safe)."""
import ctypes

import numpy as np
import pytest


def _fake(module, **attrs):
    cls = __import__("niwqg_amd." + module, fromlist=["Model"]).Model
    m = cls.__new__(cls)
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


class _NoDevice(object):
    """a context any use of which fails the test"""

    def __getattr__(self, name):
        raise AssertionError("the device was touched: %s" % name)


def _models():
    return [_fake(mod, _ctx=_NoDevice(), tc=0, t=0.0) for mod in ("CoupledModel", "UnCoupledModel", "YBJModel", "QGModel")]


def test_available_names_per_class():
    from niwqg_amd import particles
    for m in _models():
        want = ["u", "v", "q"] if type(m).__module__.endswith("QGModel") else ["u", "v", "q", "phi"]
        assert particles.available(m) == want


@pytest.mark.parametrize("args, kwargs, match", [
    (([0.0, 1.0], [0.0]), {}, "differ in length"),
    (([], []), {}, "no particles"),
    ((np.zeros((2, 2)), np.zeros((2, 2))), {}, "1-D"),
    (([0.0, np.nan], [0.0, 1.0]), {}, "non-finite"),
    (([0.0, 1.0], [np.inf, 1.0]), {}, "non-finite"),
    (([0.0], [0.0]), dict(record_every=-1), "record_every"),
    (([0.0], [0.0]), dict(record_every=2, capacity=0), "capacity"),
    (([0.0], [0.0]), dict(record_every=1, record=("w",)), "'w'"),
    (([0.0], [0.0]), dict(record_every=1, record=("u", "u")), "twice"),
])
def test_argument_errors_are_raised_before_the_device(args, kwargs, match):
    from niwqg_amd import particles
    for m in _models():
        with pytest.raises(ValueError, match=match):
            particles.attach(m, *args, **kwargs)


def test_phi_is_for_the_kernel_family_only():
    from niwqg_amd import particles
    qg = _fake("QGModel", _ctx=_NoDevice(), tc=0, t=0.0)
    with pytest.raises(ValueError, match="valid names: u, v, q$"):
        particles.attach(qg, [0.0], [0.0], record_every=1, record=("phi",))
    with pytest.raises(ValueError, match="'phi'"):
        particles._names(qg, ("u", "phi"), "sample")
    for m in _models()[:3]:
        assert particles._names(m, ("phi", "q"), "sample") == ["phi", "q"]


def test_second_attach_is_refused():
    from niwqg_amd import particles
    m = _models()[0]
    m.__dict__["_particles"] = object()
    with pytest.raises(RuntimeError, match="attached already"):
        particles.attach(m, [0.0], [0.0])


def test_slab_models_are_refused():
    from niwqg_amd import particles
    from niwqg_amd.slab import SlabContext
    for mod in ("CoupledModel", "QGModel", "YBJModel"):
        m = _fake(mod, _ctx=SlabContext.__new__(SlabContext), tc=0, t=0.0)
        with pytest.raises(NotImplementedError, match="slab"):
            particles.attach(m, [1.0, 2.0], [3.0, 4.0])
        assert "_particles" not in m.__dict__


def test_particle_entries_are_exported_and_typed():
    import niwqg_amd
    niwqg_amd.build()
    from niwqg_amd import _lib
    L = _lib.lib()
    names = ("nq_particles_attach", "nq_particles_detach", "nq_particles_get", "nq_particles_sample", "nq_particles_records",
             "nq_any_particles_rk4", "nq_any_interp")
    for name in names:
        assert name in _lib.EXPORTS and getattr(L, name).argtypes is not None, name
    assert L.nq_particles_attach.argtypes[1] is ctypes.c_int
    assert L.nq_particles_attach.argtypes[4] is ctypes.c_double
    assert L.nq_any_particles_rk4.argtypes[-1] is ctypes.c_double
    # null contexts and engines are refused without a device
    x = (ctypes.c_double * 1)(0.0)
    assert L.nq_particles_attach(None, 1, x, x, 1.0, 1.0, 0, 0, 0, None) != 0
    assert L.nq_particles_detach(None) != 0
    assert L.nq_particles_get(None, x, x) != 0
    assert L.nq_particles_sample(None, 0, None, None) != 0
    assert L.nq_particles_records(None, None, None, None) != 0
    assert L.nq_any_particles_rk4(None, None, 1, None, None, 8, 1.0, 1.0, 0.0, 1.0) == -1
    assert L.nq_any_interp(None, None, None, None, 1, 8, 1.0, 1.0) == -1


# ---- the numpy restatement ------------------------------------------------------------------------------------------------
# Written from the contract, independently of niwqg_amd.particles: Keys' kernel (a = -1/2) as a function
# of the distance to a node, the 4 x 4 nodes whose distance is below 2 along each axis, grid value [j, i] at
# ((i + 1/2) dx, (j + 1/2) dy), periodic; NaN for a non-finite coordinate.  test_gpu_particles.py uses it as its oracle.
def keys_kernel(s):
    a = np.abs(np.asarray(s, np.float64))
    near = (1.5 * a - 2.5) * a * a + 1.0
    far = ((-0.5 * a + 2.5) * a - 4.0) * a + 2.0
    return np.where(a <= 1.0, near, np.where(a < 2.0, far, 0.0))


def stencil(x, L, n):
    """(finite, node indices (4, m), weights (4, m)) of the points x along one axis"""
    x = np.asarray(x, np.float64)
    finite = np.isfinite(x)
    u = np.mod(np.where(finite, x, 0.0), L)
    u = np.where(u >= L, u - L, u)                    # (np.mod can round up to L for tiny negative x)
    s = u / (L / n) - 0.5                             # in node units
    first = np.floor(s).astype(np.int64) - 1
    nodes = first[None, :] + np.arange(4)[:, None]
    return finite, np.mod(nodes, n), keys_kernel(s[None, :] - nodes)


def interp(plane, x, y, L):
    """the (n, n) plane (real or complex) at the points (x, y) of the periodic square [0, L)^2"""
    plane = np.asarray(plane)
    n = plane.shape[0]
    x, y = np.atleast_1d(np.asarray(x, np.float64)), np.atleast_1d(np.asarray(y, np.float64))
    fx, ix, wx = stencil(x, L, n)
    fy, iy, wy = stencil(y, L, n)
    out = np.zeros(x.shape, np.result_type(plane.dtype, np.float64))
    for a in range(4):
        row = np.zeros_like(out)
        for b in range(4):
            row = row + wx[b] * plane[iy[a], ix[b]]
        out = out + wy[a] * row
    return np.where(fx & fy, out, np.nan)


def _grid(n, L):
    x = (np.arange(n) + 0.5) * L / n
    return np.meshgrid(x, x)          # X[j, i] = x_i, Y[j, i] = y_j


def test_restatement_is_exact_at_nodes():
    rng = np.random.default_rng(1)
    n, L = 32, 7.0
    f = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    X, Y = _grid(n, L)
    got = interp(f, X.ravel(), Y.ravel(), L)
    assert np.max(np.abs(got - f.ravel())) < 1e-13


def test_restatement_is_periodic():
    rng = np.random.default_rng(2)
    n, L = 16, 3.0
    f = rng.standard_normal((n, n))
    x, y = rng.uniform(0, L, 200), rng.uniform(0, L, 200)
    a = interp(f, x, y, L)
    for sx, sy in ((L, 0), (0, L), (-L, 2 * L), (5 * L, -3 * L)):
        b = interp(f, x + sx, y + sy, L)
        assert np.max(np.abs(a - b)) < 1e-12
    # the periodic seam: a point just below L and one at 0 see the same wrap-around stencil
    assert abs(interp(f, [L * (1 - 1e-15)], [0.1], L)[0] - interp(f, [0.0], [0.1], L)[0]) < 1e-12


def test_restatement_is_third_order():
    L = 2 * np.pi
    rng = np.random.default_rng(3)
    x, y = rng.uniform(0, L, 500), rng.uniform(0, L, 500)

    def field(X, Y):
        return np.sin(2 * X + 1.0) * np.cos(3 * Y) + 0.5 * np.cos(X - 2 * Y)

    errs = []
    for n in (32, 64, 128):
        X, Y = _grid(n, L)
        errs.append(np.max(np.abs(interp(field(X, Y), x, y, L) - field(x, y))))
    for a, b in zip(errs, errs[1:]):
        assert 6.0 < a / b < 11.0, errs


def test_restatement_non_finite_gives_nan_and_stays_in_range():
    n, L = 8, 1.0
    f = np.arange(n * n, dtype=float).reshape(n, n)
    bad = np.array([np.nan, np.inf, -np.inf, 1e300, -1e300, 1e-320, -1e-320, L, -L, 0.0])
    v = interp(f, bad, np.full(bad.size, 0.3), L)
    assert np.all(np.isnan(v[:3])) and np.all(np.isfinite(v[3:]))
    finite, idx, w = stencil(bad, L, n)
    assert idx.min() >= 0 and idx.max() < n
    assert np.allclose(w[:, finite].sum(axis=0), 1.0)


def test_package_interpolate_matches_the_restatement():
    """niwqg_amd.particles.interpolate (the rule in numpy for users) against the restatement above"""
    from niwqg_amd.particles import interpolate
    rng = np.random.default_rng(4)
    n, L = 24, 5.0
    f = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    x = np.concatenate([rng.uniform(-3 * L, 4 * L, 500), [0.0, L, -L, np.nan, np.inf, 1e-320, -1e-320]])
    y = np.concatenate([rng.uniform(-3 * L, 4 * L, 500), [L, 0.0, 2 * L, 0.1, 0.2, 0.3, -1e-320]])
    a, b = interpolate(f, x, y, L), interp(f, x, y, L)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(b)
    assert np.max(np.abs(a[ok] - b[ok])) < 1e-12
