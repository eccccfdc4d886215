"""Ray mode of the Lagrangian particles (niwqg_amd/particles.py ``attach(..., rays=(k0, l0))``, nq_particles_rays,
nq_any_particles_rk4_rays): positions and wavevectors against the numpy restatement ``particles.rk4_rays`` fed
with the model's own velocity and zeta after every step, eta = 0 against plain particles, k conserved in a shear, the rest state,
the conservation of the interpolated omega on a steady flow, state changes between steps, batching and determinism, bit-identical
model outputs, the records, and the refusals with the lifecycle.  Grids are 64^2 unless a case says otherwise; 48^2 and 96^2 take
the any-size path.

The planes of the host copy: (u, v) of ``m.ph`` (``velocity`` of tests/test_gpu_particles.py) and zeta = q_psi of the state the last
inversion saw, ``ifft2(-wv2 ph).real + mean(q)`` with the mean read from ``m.qh[0, 0]`` (``zeta`` below).  A bare ``set_phi`` on
CoupledModel inverts nothing (quirk Q2): ph, and with it this zeta, stay what they were, and so does the device's plane, formed
again from the (q, q_w) rows the last inversion left.

Observed on an MI355X (the tests print them with -s; the bars are asserted):
  positions, max |device - rk4_rays| after 20 steps, every case        2.3e-10 m  (bar 1e-12 L = 1.3e-6 m; they moved up to 5.9e4 m)
  wavevectors, max |device - rk4_rays| after 20 steps, every case      3.4e-20 1/m (bar 1e-12 max(|k|, |l|) = 5.0e-17)
  the same after 3 steps at 256^2 .. 2048^2 (every row plan)             3.6e-12 m, 6.8e-21 1/m
  shear on YBJModel, 50 steps, max |k - k0| / |k0|                      1.5e-15    (bar 1e-13; l moved by 2.6e2 |l0| at most)
  rest state, max |x - x0 - (U + eta k) t| after 20 steps               2.3e-9 m   (bar 1e-13 L = 1.3e-7 m); k, l bit-identical
  omega drift (rms over 2000 rays) over 3e5 s, dt = 1e4 -> 5e3 s        5.689e-12 -> 1.400e-12 1/s (x4.06), max |omega| 9.4e-6:
                                                                        numpy's figures (tests/test_rays_host.py) digit for digit
  records, max |omega - ray_omega(columns)|                             1.7e-21    (bar 1e-14 of the largest term = 5.7e-20)
  records, max |zeta - host zeta at the ray|                            1.1e-21    (bar 1e-12 max |zeta| = 2.0e-18)
"""
import numpy as np
import pytest

from test_gpu_spectra import make
from test_gpu_particles import particle_set, outputs, assert_same, set_tmax, velocity
from test_oracle_golden import notebook_kwargs
from test_gpu_drifters import drifter_model
from test_rays_host import ray_set, steady_flow, rms, ETA, DT_OMEGA, T_OMEGA, N_OMEGA

pytestmark = pytest.mark.gpu

N = 400


def zeta(m):
    """q_psi of the state the last inversion saw, from the psi-hat and the q-hat the model holds (Kernel family)"""
    nx = m.nx
    k = np.fft.fftfreq(nx, 1.0 / nx) * m.dk
    wv2 = k[None, :] ** 2 + k[:, None] ** 2
    return np.fft.ifft2(-wv2 * np.array(m.ph)).real + np.array(m.qh)[0, 0].real / nx ** 2


def rays_for(m, n, seed=11):
    """the positions of ``particle_set`` (nodes, the seam, far-out points) with the wavevectors of ``ray_set``"""
    x, y = particle_set(m, n)
    _, _, k, l = ray_set(n, seed)
    return x, y, k, l


class Host(object):
    """a host copy of the rays, advanced with particles.rk4_rays from the fields the model returns after every step"""

    def __init__(self, m, x, y, k, l, eta=None):
        self.m, self.p = m, tuple(np.array(a) for a in (x, y, k, l))
        self.eta = m.hslash if eta is None else eta
        self.refresh()

    def refresh(self):
        """after a change of the state between two steps"""
        self.U0, self.Z0 = velocity(self.m), zeta(self.m)

    def step(self):
        from niwqg_amd import particles
        m = self.m
        m._step_forward()
        U1, Z1 = velocity(m), zeta(m)
        self.p = particles.rk4_rays(*self.p, self.U0, U1, self.Z0, Z1, m.U, self.eta, m.dt, m.L)
        self.U0, self.Z0 = U1, Z1

    def errors(self, P):
        """(max position error, max wavevector error, max(|k|, |l|) over the rays)"""
        (xa, ya), (ka, la) = P.positions(), P.wavevectors()
        x, y, k, l = self.p
        return (max(np.max(np.abs(xa - x)), np.max(np.abs(ya - y))), max(np.max(np.abs(ka - k)), np.max(np.abs(la - l))),
                max(np.max(np.abs(k)), np.max(np.abs(l))))

    def check(self, P, tag=""):
        ex, ek, top = self.errors(P)
        print("rays %s: max |device - rk4_rays| positions %.3e (bar %.3e), wavevectors %.3e (bar %.3e)" % (tag, ex, 1e-12 * self.m.L, ek, 1e-12 * top))
        assert ex <= 1e-12 * self.m.L and ek <= 1e-12 * top


# ---- 1. the restatement ----------------------------------------------------------------------------------------------------------
def check_restatement(kind, nx, nsteps=20):
    from niwqg_amd import particles
    A, B = drifter_model(kind, nx), drifter_model(kind, nx)
    assert getattr(A, "_any_size", False) == (nx in (48, 96))
    x, y, k, l = rays_for(A, N)
    P = particles.attach(A, x, y, rays=(k, l))
    assert P.rays and P.eta == A.hslash
    H = Host(B, x, y, k, l)
    set_tmax(A, nsteps)
    A.run()
    for _ in range(nsteps):
        H.step()
    assert A.tc == B.tc == nsteps
    if kind == "uncoupled":
        assert A.U != 0
    H.check(P, "%s %d" % (kind, nx))
    (xa, ya), (ka, la) = P.positions(), P.wavevectors()
    print("rays %s %d: moved %.3e m, max |k - k0| / |k0| = %.3e" % (kind, nx, np.max(np.hypot(xa - x, ya - y)), np.max(np.abs(ka - k) / np.abs(k))))
    assert np.max(np.hypot(xa - x, ya - y)) > 1e-5 * A.L
    assert np.max(np.abs(ka - k) / np.abs(k)) > 1e-3
    P.detach()


@pytest.mark.parametrize("kind, nx", [("coupled", 64), ("uncoupled", 64), ("ybj", 64), ("coupled", 128)])
def test_restatement_fused(kind, nx):
    check_restatement(kind, nx)


@pytest.mark.parametrize("nx", [48, 96])
def test_restatement_anysize(nx):
    check_restatement("coupled", nx)


@pytest.mark.parametrize("nx", [256, 512, 1024, 2048])
def test_larger_row_plans(nx):
    """every row plan lays its points out in its own way: the zeta plane of k_x_get_zeta against the host's at the rays, and three
    steps of the rays against the restatement"""
    from niwqg_amd import particles
    m = drifter_model("coupled", nx)
    x, y, k, l = rays_for(m, 200)
    P = particles.attach(m, x, y, rays=(k, l))
    Z = zeta(m)
    assert np.max(np.abs(P.sample("zeta")["zeta"] - particles.interpolate(Z, x, y, m.L))) <= 1e-12 * np.abs(Z).max()
    H = Host(m, x, y, k, l)
    for _ in range(3):
        H.step()
    H.check(P, "coupled %d" % nx)
    assert np.max(np.abs(P.wavevectors()[0] - k) / np.abs(k)) > 1e-3
    P.detach()


# ---- 2. eta = 0: the positions of plain particles ------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [64, 48])
def test_eta_zero_moves_the_rays_as_plain_particles(nx):
    from niwqg_amd import particles
    A, B = drifter_model("coupled", nx), drifter_model("coupled", nx)
    x, y, k, l = rays_for(A, N)
    P, Q = particles.attach(A, x, y, rays=(k, l), eta=0.0), particles.attach(B, x, y)
    for m in (A, B):
        for _ in range(10):
            m._step_forward()
    (xa, ya), (xb, yb) = P.positions(), Q.positions()
    assert max(np.max(np.abs(xa - xb)), np.max(np.abs(ya - yb))) <= 1e-12 * A.L
    ka, la = P.wavevectors()
    assert np.max(np.abs(ka - k) / np.abs(k)) > 1e-3                        # k evolves nevertheless
    assert np.max(np.hypot(xa - x, ya - y)) > 1e-5 * A.L


# ---- 3. a shear on YBJModel: k is conserved ------------------------------------------------------------------------------------------
def test_k_is_conserved_in_a_shear():
    from niwqg_amd import particles
    m = drifter_model("ybj", 64)
    yy = (np.arange(64) + 0.5) * m.L / 64
    prof = np.sin(2 * np.pi * yy / m.L) + 0.5 * np.cos(2 * np.pi * 3 * yy / m.L + 0.3)
    m.set_q(np.repeat((2e-6 * prof)[:, None], 64, axis=1))                   # q = q(y): u = u(y), v = 0
    assert np.abs(velocity(m)[0]).max() > 0.01 and np.abs(velocity(m)[1]).max() <= 1e-12
    x, y, k, l = rays_for(m, N)
    P = particles.attach(m, x, y, rays=(k, l))
    m._ctx.step(50)
    ka, la = P.wavevectors()
    print("rays in a shear: max |k - k0| / |k0| = %.3e (bar 1e-13), max |l - l0| / |l0| = %.3e" % (np.max(np.abs(ka - k) / np.abs(k)), np.max(np.abs(la - l) / np.abs(l))))
    assert np.all(np.abs(ka - k) <= 1e-13 * np.abs(k))
    assert np.max(np.abs(la - l) / np.abs(l)) > 1e-3                        # the zeta_y and u_y terms move l


# ---- 4. the rest state ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, nx", [("coupled", 64), ("ybj", 64), ("coupled", 48)])
def test_rest_state(kind, nx):
    import niwqg_amd
    from niwqg_amd import particles
    kw = notebook_kwargs(nx, False)
    m = {"coupled": niwqg_amd.CoupledModel, "ybj": niwqg_amd.YBJModel}[kind].Model(**kw)
    m.set_q(np.zeros((nx, nx)))
    m.set_phi(np.zeros((nx, nx), complex))
    assert m.U != 0
    x, y, k, l = ray_set(N)                                   # (inside the domain: the bar is below the rounding of a far-out coordinate)
    P = particles.attach(m, x, y, rays=(k, l))
    nsteps = 20
    for _ in range(nsteps):
        m._step_forward()
    ka, la = P.wavevectors()
    assert np.array_equal(ka, k) and np.array_equal(la, l)                  # bit for bit
    xa, ya = P.positions()
    t = nsteps * m.dt
    err = max(np.max(np.abs(xa - x - (m.U + m.hslash * k) * t)), np.max(np.abs(ya - y - m.hslash * l * t)))
    print("rays at rest %s %d: max |x - x0 - (U + eta k) t| = %.3e (bar %.3e)" % (kind, nx, err, 1e-13 * m.L))
    assert err <= 1e-13 * m.L
    assert np.max(np.abs(xa - x)) > 1e-3 * m.L


# ---- 5. omega is conserved on a steady flow, up to the time stepping ------------------------------------------------------------------
def omega_drift_device(dt):
    import niwqg_amd
    from niwqg_amd import particles
    kw = notebook_kwargs(64, False)
    kw.update(dt=dt)
    m = niwqg_amd.YBJModel.Model(**kw)
    q, u, v = steady_flow(64)
    m.set_q(q)
    m.set_phi(np.zeros((64, 64), complex))
    assert abs(m.hslash - ETA) <= 1e-14 * ETA and m.U == -0.1
    assert np.max(np.abs(velocity(m)[0] - u)) <= 1e-12 * 0.1                # the flow of the host test
    x, y, k, l = ray_set(N_OMEGA)
    nsteps = int(round(T_OMEGA / dt))
    P = particles.attach(m, x, y, record_every=nsteps, capacity=2, record=("omega",), rays=(k, l))
    m._ctx.step(nsteps)
    w = P.trajectory().values["omega"]
    assert w.shape == (2, N_OMEGA)
    return rms(w[1] - w[0]), np.max(np.abs(w[0]))


def test_omega_drift_falls_when_dt_is_halved():
    d1, top = omega_drift_device(DT_OMEGA)
    d2, _ = omega_drift_device(DT_OMEGA / 2)
    print("rays, omega drift (rms over %d rays) over %.0e s: dt = %.0e: %.3e, dt = %.0e: %.3e (x%.2f); max |omega| = %.3e"
          % (N_OMEGA, T_OMEGA, DT_OMEGA, d1, DT_OMEGA / 2, d2, d1 / d2, top))
    assert d2 >= 1e3 * np.finfo(float).eps * top
    assert d1 / d2 >= 2.5


# ---- 6. state changes between steps --------------------------------------------------------------------------------------------------
def test_state_changes_between_steps():
    from niwqg_amd import particles
    m = drifter_model("coupled", 64)
    rng = np.random.default_rng(9)
    x, y, k, l = rays_for(m, N)
    P = particles.attach(m, x, y, rays=(k, l))
    H = Host(m, x, y, k, l)                                   # (the model itself is stepped by the host copy)
    H.step()
    H.step()
    ph_before, z_before = np.array(m.ph), H.Z0
    m.set_phi(np.array(m.phi) * (1.3 - 0.4j) + 0.01)
    assert np.array_equal(np.array(m.ph), ph_before)         # quirk Q2: no inversion; zeta0 stays the q_psi that matches the held ph
    H.refresh()
    assert np.array_equal(H.Z0, z_before)
    assert np.max(np.abs(P.sample("zeta")["zeta"] - particles.interpolate(z_before, *P.positions(), m.L))) <= 1e-12 * np.abs(z_before).max()
    H.step()
    H.check(P, "after set_phi")
    m.set_q(np.array(m.q) * 0.7 + 0.1 * np.array(m.q).std() * rng.standard_normal(m.q.shape))
    H.refresh()
    assert np.max(np.abs(H.Z0 - z_before)) > 0.05 * np.abs(z_before).max()
    H.step()
    m._invert()
    H.refresh()
    H.step()
    H.step()
    H.check(P, "after set_q and _invert")
    assert np.max(np.hypot(*np.subtract(P.positions(), (x, y)))) > 1e-5 * m.L


# ---- 7. batching and determinism -----------------------------------------------------------------------------------------------------
COLUMNS = ("k", "l", "zeta", "omega", "u")


@pytest.mark.parametrize("kind", ["coupled", "ybj"])
def test_batching_and_determinism(kind):
    from niwqg_amd import particles
    res = []
    for mode in ("batched", "single", "batched"):
        m = drifter_model(kind, 64)
        x, y, k, l = rays_for(m, N)
        P = particles.attach(m, x, y, record_every=2, capacity=3, record=COLUMNS, rays=(k, l))
        if mode == "batched":
            m._ctx.step(8)
        else:
            for _ in range(8):
                m._ctx.step(1)
        tr = P.trajectory()
        assert list(tr.step) == [4, 6, 8]
        res.append([*P.positions(), *P.wavevectors(), tr.x, tr.y] + [tr.values[c] for c in COLUMNS])
    for other in res[1:]:
        for a, b in zip(res[0], other):
            assert np.array_equal(a, b)


# ---- 8. non-interference -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["coupled", "uncoupled", "ybj"])
def test_model_outputs_are_those_of_a_run_without_rays(kind):
    from niwqg_amd import particles
    A, C = drifter_model(kind, 64, tdiags=3), drifter_model(kind, 64, tdiags=3)
    for m in (A, C):
        m.twrite = 5
        set_tmax(m, 12)
    x, y, k, l = rays_for(A, N)
    P = particles.attach(A, x, y, record_every=3, capacity=4, record=("k", "omega", "zeta"), rays=(k, l))
    A.run()
    C.run()
    assert_same(outputs(A, kind), outputs(C, kind), kind)     # bit for bit, but the atomically reduced scalars (1e-12)
    P.detach()
    assert A._ctx.device_bytes() == C._ctx.device_bytes()


# ---- 9. records ------------------------------------------------------------------------------------------------------------------------
RECORD = ("u", "v", "zeta", "k", "l", "omega")


@pytest.mark.parametrize("nx", [64, 48])
def test_records(nx):
    from niwqg_amd import particles, lagrangian
    m = drifter_model("coupled", nx)
    q = np.array(m.q)
    m.set_q(q + 0.3 * q.std())                               # a mean of q: it enters omega and the "zeta" column
    x, y, k, l = rays_for(m, 300)
    for _ in range(3):
        m._step_forward()
    tc0 = m.tc
    P = particles.attach(m, x, y, record_every=2, capacity=6, record=RECORD, rays=(k, l))
    z0 = P.trajectory().values                               # the record taken at attach holds the ray's columns (written again by the mode)
    assert np.array_equal(z0["k"][0], k) and np.array_equal(z0["l"][0], l)
    w0 = particles.ray_omega(z0["u"][0], z0["v"][0], z0["zeta"][0], k, l, m.U, m.hslash)
    assert np.max(np.abs(z0["omega"][0] - w0)) <= 1e-14 * np.abs(w0).max() and np.abs(w0).max() > 0
    for _ in range(14):                                      # 8 records into 6 slots: the ring wrapped
        m._step_forward()
    tr = P.trajectory()
    assert list(tr.step - tc0) == [4, 6, 8, 10, 12, 14]
    v = tr.values
    eta = m.hslash
    terms = np.max([np.abs((v["u"] + m.U) * v["k"]), np.abs(v["v"] * v["l"]), np.abs(0.5 * v["zeta"]), 0.5 * eta * (v["k"] ** 2 + v["l"] ** 2)])
    err = np.max(np.abs(v["omega"] - particles.ray_omega(v["u"], v["v"], v["zeta"], v["k"], v["l"], m.U, eta)))
    print("ray records %d: max |omega - ray_omega(columns)| = %.3e (bar %.3e)" % (nx, err, 1e-14 * terms))
    assert err <= 1e-14 * terms and np.abs(v["omega"]).max() > 0.01 * terms
    # the last record is the current state's: the zeta column is the host's zeta at the ray, the mean of q included
    Z = zeta(m)
    assert abs(Z.mean()) > 0.1 * Z.std()
    errz = np.max(np.abs(v["zeta"][-1] - particles.interpolate(Z, tr.x[-1], tr.y[-1], m.L)))
    print("ray records %d: max |zeta - host zeta at the ray| = %.3e (bar %.3e)" % (nx, errz, 1e-12 * np.abs(Z).max()))
    assert errz <= 1e-12 * np.abs(Z).max()
    smp = P.sample(RECORD)
    for name in RECORD:
        assert np.array_equal(smp[name], v[name][-1]), name
    ka, la = P.wavevectors()
    assert np.array_equal(ka, v["k"][-1]) and np.array_equal(la, v["l"][-1])
    assert sorted(P.sample()) == ["phi", "q", "u", "v"]      # the default stays the fields of the state
    # dispersion reads x and y only: it runs on a ray ring unchanged
    D = lagrangian.dispersion(P)
    want = lagrangian.reference_dispersion(tr)
    for key in ("dx", "dy", "A_xx", "A_yy", "A_xy", "A2", "M4"):
        a, b = getattr(D, key), want[key]
        assert a.shape == b.shape and np.max(np.abs(a - b)) <= 1e-12 * np.abs(b).max(), key
    assert D.A2[-1] > 0
    P.detach()


def test_zeta_without_ray_mode():
    """"zeta" is a name of plain particles too; "k", "l", "omega" are not"""
    from niwqg_amd import particles
    m = drifter_model("uncoupled", 64)
    x, y = particle_set(m, 200)
    P = particles.attach(m, x, y, record_every=1, capacity=2, record=("zeta", "q"))
    m._ctx.step(2)
    tr = P.trajectory()
    assert np.max(np.abs(tr.values["zeta"][-1] - particles.interpolate(zeta(m), tr.x[-1], tr.y[-1], m.L))) <= 1e-12 * np.abs(zeta(m)).max()
    assert np.max(np.abs(tr.values["zeta"] - tr.values["q"])) <= 1e-12 * np.abs(zeta(m)).max()       # UnCoupledModel: q_psi = q
    with pytest.raises(ValueError, match="need ray mode"):
        P.sample("omega")
    with pytest.raises(RuntimeError, match="without rays"):
        P.wavevectors()
    P.detach()


# ---- 10. refusals and the lifecycle --------------------------------------------------------------------------------------------------
def test_refusals_leave_the_model_usable():
    import ctypes
    import niwqg_amd
    from niwqg_amd import particles, _lib
    Lb = _lib.lib()
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    one = np.array([1e-5])
    codes = lambda *c: (ctypes.c_int * len(c))(*c)

    qg = make("qg", 64)
    with pytest.raises(ValueError, match="QGModel has no near-inertial waves"):
        particles.attach(qg, [1.0], [2.0], rays=(one, one))
    P = particles.attach(qg, [1.0], [2.0])
    assert Lb.nq_particles_rays(qg._ctx.h, dp(one), dp(one), 1.0) == -4                  # QGModel, through the raw ABI
    assert Lb.nq_particles_get_rays(qg._ctx.h, dp(one.copy()), dp(one.copy())) == -4
    out = np.empty(1)
    assert Lb.nq_particles_sample(qg._ctx.h, 1, codes(_lib.PT_ZETA), dp(out)) == -1
    qg._ctx.step(2)
    assert np.all(np.isfinite(P.positions()[0]))
    P.detach()

    m = drifter_model("coupled", 64)
    x, y, k, l = rays_for(m, 100)
    h = m._ctx.h
    for bad, match in ((([1.0], [1.0]), "shapes"), ((k, np.where(np.arange(100) == 7, np.nan, l)), "non-finite")):
        with pytest.raises(ValueError, match=match):
            particles.attach(m, x, y, rays=bad)
    with pytest.raises(ValueError, match="exclude each other"):
        particles.attach(m, x, y, rays=(k, l), wave=1.0)
    assert "_particles" not in m.__dict__
    assert Lb.nq_particles_rays(h, dp(k), dp(l), 1.0) == -4                               # no particles attached
    assert b"no particles" in Lb.nq_last_error(h)
    m._step_forward()                                                                    # (the lazy allocations of a first step)
    np.array(m.phi), np.array(m.u), np.array(m.v), np.array(m.q)
    b0 = m._ctx.device_bytes()
    P = particles.attach(m, x, y, record_every=1, capacity=4, record=("u", "v"))
    b1 = m._ctx.device_bytes()
    kn, li = k.copy(), l.copy()
    kn[3], li[5] = np.nan, np.inf
    assert Lb.nq_particles_rays(h, dp(kn), dp(l), 1.0) == -1 and Lb.nq_particles_rays(h, dp(k), dp(li), 1.0) == -1
    assert Lb.nq_particles_rays(h, dp(k), dp(l), float("nan")) == -1 and Lb.nq_particles_rays(h, dp(k), dp(l), float("inf")) == -1
    assert Lb.nq_particles_rays(h, None, dp(l), 1.0) == -1 and Lb.nq_particles_rays(h, dp(k), None, 1.0) == -1
    out = np.empty(100)
    for code in (_lib.PT_K, _lib.PT_L, _lib.PT_OMEGA):                                    # the ray's names without the mode
        assert Lb.nq_particles_sample(h, 1, codes(code), dp(out)) == -1
    assert Lb.nq_particles_get_rays(h, dp(out), dp(out.copy())) == -4
    with pytest.raises(ValueError, match="need ray mode"):
        P.sample(("u", "k"))
    assert m._ctx.device_bytes() == b1                                                   # a refused call allocates nothing
    m._step_forward()
    assert Lb.nq_particles_rays(h, dp(k), dp(l), 1.0) == -4                               # after a step
    assert b"moved already" in Lb.nq_last_error(h)
    assert m._ctx.device_bytes() == b1
    m._step_forward()                                                                    # still plain particles, and usable
    assert np.all(np.isfinite(P.positions()[0]))
    P.detach()
    assert m._ctx.device_bytes() == b0
    # the two modes exclude each other, in either order
    P = particles.attach(m, x, y, wave=1.0)
    bw = m._ctx.device_bytes()
    assert Lb.nq_particles_rays(h, dp(k), dp(l), 1.0) == -4 and b"drifter mode" in Lb.nq_last_error(h)
    assert m._ctx.device_bytes() == bw
    P.detach()
    P = particles.attach(m, x, y)
    plain = m._ctx.device_bytes()
    P.detach()
    # attach, detach and attach again with other wavevectors
    ends = []
    for s in (1.0, -0.5):
        P = particles.attach(m, x, y, rays=(s * k, s * l))
        assert m._ctx.device_bytes() == plain + 2 * 64 * 64 * 8 + 2 * 100 * 8            # two zeta planes, two arrays of n doubles
        assert Lb.nq_particles_rays(h, dp(k), dp(l), 1.0) == -4 and b"on already" in Lb.nq_last_error(h)
        assert Lb.nq_particles_wave(h, 1.0, m.f, 0.0) == -4 and b"ray mode" in Lb.nq_last_error(h)
        ka, la = P.wavevectors()
        assert np.array_equal(ka, s * k) and np.array_equal(la, s * l)
        H = Host(m, x, y, s * k, s * l)
        H.step()
        H.step()
        H.check(P, "lifecycle")
        ends.append(P.positions())
        P.detach()
        assert m._ctx.device_bytes() == b0
    assert np.max(np.hypot(ends[0][0] - ends[1][0], ends[0][1] - ends[1][1])) > 1e-6 * m.L
    # YBJModel: one zeta plane
    yb = drifter_model("ybj", 64)
    P = particles.attach(yb, x, y)
    plain = yb._ctx.device_bytes()
    P.detach()
    P = particles.attach(yb, x, y, rays=(k, l))
    assert yb._ctx.device_bytes() == plain + 64 * 64 * 8 + 2 * 100 * 8
    P.detach()
    # a slab rank
    s = niwqg_amd.CoupledModel.Model(slab=2, **notebook_kwargs(64, True))
    assert Lb.nq_particles_rays(s._ctx.sim.ranks[0].h, dp(one), dp(one), 1.0) == -4
    assert Lb.nq_particles_get_rays(s._ctx.sim.ranks[0].h, dp(one.copy()), dp(one.copy())) == -4
    with pytest.raises(NotImplementedError, match="slab"):
        particles.attach(s, [1.0], [2.0], rays=(one, one))
