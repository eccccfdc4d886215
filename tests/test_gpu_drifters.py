"""Drifter mode of the Lagrangian particles (niwqg_amd/particles.py ``attach(..., wave=a)``, nq_particles_wave,
nq_any_particles_rk4_wave): positions against the numpy restatement ``particles.rk4_wave`` fed with the
model's own velocity and phi after every step, the exact inertial circle within the Simpson bound and at fourth order, state changes
between steps, batching and determinism, bit-identical model outputs, the "uw" / "vw" records and the "uvw" / "uvt" Lagrangian
spectra, and the refusals with the lifecycle.  Grids are 64^2 unless a case says otherwise; 48^2 and 96^2 take the any-size path.

The frequency axis of ``lagrangian.spectrum`` follows ``frequency.py``: a series turning as e^{-i omega t} appears at +omega.  The
wave velocity a phi e^{-i f0 t} of a uniform phi turns clockwise; in the e^{+i omega t} convention of drifter papers that is the
bin of -f0, on this axis it is the bin omega = +f0.  ``test_inertial_peak`` finds it from the definition of the transform.

The velocity planes of the host copy are u = -d psi/dy, v = d psi/dx of ``m.ph``, the psi-hat the model holds (``velocity`` of
tests/test_gpu_particles.py), as the contract of section 5g has it.  ``m.u`` and ``m.v`` are not that after a step: like the
reference they return what the step's FOURTH STAGE left behind, and a host copy fed with them misses the device by metres
(4.7 m after 20 steps of CoupledModel at 64^2, 0.5 m on QGModel with ``wave=None``; YBJModel, whose psi is steady, agrees).
``m.phi`` is the new state's.

Observed on an MI355X (the tests print them with -s; the bars are asserted):
  positions, max |device - rk4_wave| after 20 steps, every case        3.5e-10 m  (bar 1e-12 L = 1.3e-6 m; they moved up to 4.4e4 m)
  inertial circle, error after one period, f0 dt = 0.25 -> 0.125       6.8e-5 -> 4.2e-6 m (x16.0); half way 4.1e-3 -> 2.5e-4 m (x16.0)
  records, max |uw + i vw - a phi e^{-i f0 t_s}|                         7.8e-18    (bar 1e-14 a max|phi| = 4.4e-16)
  "uvw" / "uvt" / "uw" spectra, max |device - numpy| / sum              3.5e-16    (bar 1e-12)
  inertial peak, mirrored bin over the peak                             1.1e-32    (bar 1e-10)
"""
import numpy as np
import pytest

from test_gpu_spectra import make, K0
from test_gpu_particles import particle_set, outputs, assert_same, set_tmax, velocity
from test_oracle_golden import notebook_kwargs
from test_drifters_host import rk4_old, circle, simpson_bound

pytestmark = pytest.mark.gpu

N = 1000
A_WAVE = 1.5


def drifter_model(kind, nx, tdiags=10 ** 9):
    """the dipole with smooth random vorticity of test_gpu_spectra.make, and a wave packet on a weak uniform wave"""
    from niwqg_amd import InitialConditions as ic
    m = make(kind, nx, "filter", tdiags=tdiags)
    m.set_phi(0.1 * ic.WavePacket(m, k=2 * K0, l=K0, R=m.L / 6, x0=m.L / 2, y0=m.L / 2) + 0.02 * (1 + 0.5j))
    return m


def state(m):
    """(u, v) of the psi-hat the model holds (see the module's doc), and its phi"""
    return velocity(m), np.array(m.phi)


class Host(object):
    """a host copy of the particles, advanced with particles.rk4_wave from the fields the model returns after every step"""

    def __init__(self, m, x, y, a):
        self.m, self.x, self.y, self.a = m, np.array(x), np.array(y), a
        self.t0, self.s = m.t, 0
        self.U0, self.P0 = state(m)

    def refresh(self):
        """after a change of the state between two steps"""
        self.U0, self.P0 = state(self.m)

    def step(self):
        from niwqg_amd import particles
        m = self.m
        m._step_forward()
        U1, P1 = state(m)
        self.x, self.y = particles.rk4_wave(self.x, self.y, self.U0, U1, self.P0, P1, m.U, self.a, m.f, self.t0 + self.s * m.dt, m.dt, m.L)
        self.U0, self.P0 = U1, P1
        self.s += 1

    def error(self, P):
        xa, ya = P.positions()
        return max(np.max(np.abs(xa - self.x)), np.max(np.abs(ya - self.y)))


# ---- 1. the restatement ----------------------------------------------------------------------------------------------------------
def check_restatement(kind, nx, nsteps=20):
    from niwqg_amd import particles
    A, B = drifter_model(kind, nx), drifter_model(kind, nx)
    assert getattr(A, "_any_size", False) == (nx in (48, 96))
    x, y = particle_set(A, N)
    P = particles.attach(A, x, y, wave=A_WAVE)
    H = Host(B, x, y, A_WAVE)
    set_tmax(A, nsteps)
    A.run()
    for _ in range(nsteps):
        H.step()
    assert A.tc == B.tc == nsteps
    if kind == "uncoupled":
        assert A.U != 0
    err = H.error(P)
    xa, ya = P.positions()
    print("drifters %s %d: max |device - rk4_wave| = %.3e (tolerance %.3e), moved %.3e" % (kind, nx, err, 1e-12 * A.L, np.max(np.hypot(xa - x, ya - y))))
    assert err <= 1e-12 * A.L
    assert np.max(np.hypot(xa - x, ya - y)) > 1e-5 * A.L
    P.detach()


@pytest.mark.parametrize("kind, nx", [("coupled", 64), ("uncoupled", 64), ("ybj", 64), ("coupled", 128)])
def test_restatement_fused(kind, nx):
    check_restatement(kind, nx)


@pytest.mark.parametrize("nx", [48, 96])
def test_restatement_anysize(nx):
    check_restatement("coupled", nx)


def test_wave_changes_the_path():
    """the same particles with and without the wave velocity end far apart (the restatement test cannot pass by ignoring it)"""
    from niwqg_amd import particles
    A, B = drifter_model("coupled", 64), drifter_model("coupled", 64)
    x, y = particle_set(A, 200)
    P, Q = particles.attach(A, x, y, wave=A_WAVE), particles.attach(B, x, y)
    A._ctx.step(10)
    B._ctx.step(10)
    (xa, ya), (xb, yb) = P.positions(), Q.positions()
    assert np.max(np.hypot(xa - xb, ya - yb)) > 1e-4 * A.L


# ---- 2. the exact inertial circle ------------------------------------------------------------------------------------------------
F0DT = 0.25


def uniform_wave_model(kind, f0dt, U=0.0, A=0.1 * np.exp(0.7j), nx=64):
    """uniform phi = A (only the (0, 0) mode), q = 0, no damping and no drag anywhere: phi stays A"""
    import niwqg_amd
    kw = notebook_kwargs(nx, False)
    kw.update(dt=f0dt / kw["f"], U=U, nu4=0.0, nu=0.0, mu=0.0, nu4w=0.0, nuw=0.0, muw=0.0)
    cls = {"coupled": niwqg_amd.CoupledModel, "ybj": niwqg_amd.YBJModel}[kind]
    m = cls.Model(**kw)
    m.set_q(np.zeros((nx, nx)))
    m.set_phi(np.full((nx, nx), A))
    return m, A


def circle_errors(kind, f0dt, U, a=A_WAVE):
    from niwqg_amd import particles
    m, A = uniform_wave_model(kind, f0dt, U)
    nsteps = int(round(2 * np.pi / f0dt))                    # one inertial period, to the step
    x0, y0 = np.array([0.31 * m.L, 0.0]), np.array([0.72 * m.L, 0.9 * m.L])
    P = particles.attach(m, x0, y0, record_every=1, capacity=nsteps + 1, wave=a)
    m._ctx.step(nsteps)
    tr = P.trajectory()
    assert tr.x.shape == (nsteps + 1, 2)
    t = np.arange(nsteps + 1) * m.dt
    z = tr.x + 1j * tr.y
    err = np.max(np.abs(z - circle((x0 + 1j * y0)[None, :], U, a, A, m.f, t[:, None])), axis=1)
    for s in range(nsteps + 1):
        assert err[s] <= simpson_bound(a, A, m.f, m.dt, t[s], m.L), (s, err[s])
    assert np.max(np.abs(np.array(m.phi) - A)) <= 1e-14 * abs(A)      # phi stayed uniform
    # a twin with wave=None: only the uniform flow moves the particle
    w, _ = uniform_wave_model(kind, f0dt, U)
    Q = particles.attach(w, x0, y0)
    w._ctx.step(nsteps)
    xq, yq = Q.positions()
    assert max(np.max(np.abs(xq - x0 - U * t[-1])), np.max(np.abs(yq - y0))) <= 1e-12 * m.L
    return err, nsteps, a * abs(A) / m.f


@pytest.mark.parametrize("kind, U", [("coupled", 0.0), ("ybj", 0.05)])
def test_exact_inertial_circle(kind, U):
    e1, n1, radius = circle_errors(kind, F0DT, U)
    e2, n2, _ = circle_errors(kind, F0DT / 2, U)
    assert n2 == 2 * n1
    print("inertial circle %s (radius %.1f m): error after one period %.3e -> %.3e (x%.1f), half way %.3e -> %.3e (x%.1f)"
          % (kind, radius, e1[-1], e2[-1], e1[-1] / e2[-1], e1[n1 // 2], e2[n1], e1[n1 // 2] / e2[n1]))
    assert e1.max() > 1e-6 * radius                        # far above the rounding: the bound and the order are seen
    assert e1[-1] / e2[-1] >= 12 and e1[n1 // 2] / e2[n1] >= 12


# ---- 3. state changes between steps ----------------------------------------------------------------------------------------------
def test_state_changes_between_steps():
    from niwqg_amd import particles
    m = drifter_model("coupled", 64)
    rng = np.random.default_rng(9)
    x, y = particle_set(m, 500)
    P = particles.attach(m, x, y, wave=A_WAVE)
    H = Host(m, x, y, A_WAVE)                                 # (the model itself is stepped by the host copy)
    H.step()
    H.step()
    ph_before, u_before = np.array(m.ph), velocity(m)[0]
    m.set_phi(np.array(m.phi) * (1.3 - 0.4j) + 0.01)
    assert np.array_equal(np.array(m.ph), ph_before)                          # quirk Q2: no inversion, U0 is what it was
    H.refresh()
    assert np.array_equal(H.U0[0], u_before)
    H.step()
    assert H.error(P) <= 1e-12 * m.L
    m.set_q(np.array(m.q) * 0.7 + 0.1 * np.array(m.q).std() * rng.standard_normal(m.q.shape))
    H.refresh()
    H.step()
    m._invert()
    H.refresh()
    H.step()
    H.step()
    assert H.error(P) <= 1e-12 * m.L
    # with the OLD phi as Phi0 the host copy would have missed the tolerance by far: the check above sees the re-formed plane
    assert np.max(np.hypot(*np.subtract(P.positions(), (x, y)))) > 1e-5 * m.L


def test_set_phi_is_seen_by_the_next_step():
    """two runs that differ only in a set_phi between two steps end apart, and each follows its own restatement"""
    from niwqg_amd import particles
    ends = []
    for scale in (1.0, -1.0):
        m = drifter_model("ybj", 64)
        x, y = particle_set(m, 200)
        P = particles.attach(m, x, y, wave=A_WAVE)
        H = Host(m, x, y, A_WAVE)
        H.step()
        m.set_phi(np.array(m.phi) * scale)
        H.refresh()
        H.step()
        assert H.error(P) <= 1e-12 * m.L
        ends.append(P.positions())
    assert np.max(np.hypot(ends[0][0] - ends[1][0], ends[0][1] - ends[1][1])) > 1e-5 * m.L


# ---- 4. batching and determinism -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["coupled", "ybj"])
def test_batching_and_determinism(kind):
    from niwqg_amd import particles
    res = []
    for mode in ("batched", "single", "batched"):
        m = drifter_model(kind, 64)
        x, y = particle_set(m, N)
        P = particles.attach(m, x, y, record_every=2, capacity=3, record=("uw", "vw", "phi", "u"), wave=A_WAVE)
        if mode == "batched":
            m._ctx.step(8)
        else:
            for _ in range(8):
                m._ctx.step(1)
        tr = P.trajectory()
        assert list(tr.step) == [4, 6, 8]
        res.append([*P.positions(), tr.x, tr.y] + [tr.values[k] for k in ("uw", "vw", "phi", "u")])
    for other in res[1:]:
        for a, b in zip(res[0], other):
            assert np.array_equal(a, b)


# ---- 5. non-interference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["coupled", "uncoupled", "ybj"])
def test_model_outputs_are_those_of_a_run_without_drifters(kind):
    from niwqg_amd import particles
    A, C = drifter_model(kind, 64, tdiags=3), drifter_model(kind, 64, tdiags=3)
    for m in (A, C):
        m.twrite = 5
        set_tmax(m, 12)
    x, y = particle_set(A, N)
    P = particles.attach(A, x, y, record_every=3, capacity=4, record=("uw", "vw"), wave=A_WAVE)
    A.run()
    C.run()
    assert_same(outputs(A, kind), outputs(C, kind), kind)     # bit for bit, but the atomically reduced scalars (1e-12)
    P.detach()
    assert A._ctx.device_bytes() == C._ctx.device_bytes()


@pytest.mark.parametrize("kind", ["coupled", "qg"])
def test_without_wave_the_old_rule_holds(kind):
    """wave=None: the positions are those of the rule before drifter mode (rk4 of tests/test_gpu_particles.py, restated in
    test_drifters_host.py) fed with the velocity of the psi-hat the model holds"""
    from niwqg_amd import particles
    from test_particles_host import interp
    A, B = (make(kind, 64), make(kind, 64)) if kind == "qg" else (drifter_model(kind, 64), drifter_model(kind, 64))
    x, y = particle_set(A, N)
    P = particles.attach(A, x, y, wave=None)
    A._ctx.step(10)
    U0 = velocity(B)
    for _ in range(10):
        B._step_forward()
        U1 = velocity(B)
        x, y = rk4_old(x, y, U0, U1, B.U, B.dt, B.L, interp)
        U0 = U1
    xa, ya = P.positions()
    assert max(np.max(np.abs(xa - x)), np.max(np.abs(ya - y))) <= 1e-12 * A.L


# ---- 6. records and Lagrangian names ---------------------------------------------------------------------------------------------
RECORD = ("u", "v", "phi", "uw", "vw")


@pytest.mark.parametrize("nx, wave", [(64, 0.7), (64, None), (48, 0.7)])
def test_records_and_lagrangian_names(nx, wave):
    from niwqg_amd import particles, lagrangian
    m = drifter_model("coupled", nx)
    a = 1.0 if wave is None else wave
    x, y = particle_set(m, 300)
    for _ in range(3):                                       # attach at t0 > 0: the clock starts from m.t at attach
        m._step_forward()
    t0, tc0 = m.t, m.tc
    assert t0 > 0
    P = particles.attach(m, x, y, record_every=2, capacity=6, record=RECORD, wave=wave)
    for _ in range(14):                                      # 8 records into 6 slots: the ring wrapped
        m._step_forward()
    tr = P.trajectory()
    assert list(tr.step - tc0) == [4, 6, 8, 10, 12, 14]
    worst, top = 0.0, 0.0
    for r, s in enumerate(tr.step - tc0):
        want = a * tr.values["phi"][r] * np.exp(-1j * m.f * (t0 + s * m.dt))
        worst = max(worst, np.max(np.abs(tr.values["uw"][r] + 1j * tr.values["vw"][r] - want)))
        top = max(top, np.abs(tr.values["phi"][r]).max())
    print("drifter records %d wave=%s: max |uw + i vw - a phi e^{-i f0 t_s}| = %.3e (bar %.3e)" % (nx, wave, worst, 1e-14 * top * a))
    assert worst <= 1e-14 * top * a
    assert np.abs(tr.values["uw"]).max() > 0.01 * a
    # sample(): the same values as the record of this step
    smp = P.sample(("uw", "phi", "vw"))
    assert np.array_equal(smp["uw"], tr.values["uw"][-1]) and np.array_equal(smp["vw"], tr.values["vw"][-1])
    assert np.array_equal(smp["phi"], tr.values["phi"][-1])
    assert sorted(P.sample()) == ["phi", "q", "u", "v"]      # the default stays the fields of the state
    # the Lagrangian names
    assert lagrangian.available(P.record) == ["uv", "uvw", "uvt", "phi"]
    S = lagrangian.spectrum(P, ["uvw", "uvt", "uw"], "hann", True, None, 8)
    for name in ("uvw", "uvt", "uw"):
        omega, ref, _ = lagrangian.reference_spectrum(tr, name, "hann", True, None, 8, dt_rec=2 * m.dt)
        err = float(np.abs(S.values[name] - ref).max() / ref.sum())
        print("lagrangian spectrum of %s: max |device - numpy| / sum = %.3e" % (name, err))
        assert np.array_equal(S.omega, omega) and err <= 1e-12 and ref.sum() > 0
    R = lagrangian.autocovariance(P, "uvt", max_lag=3)
    _, want, _ = lagrangian.reference_autocovariance(tr, "uvt", max_lag=3, dt_rec=2 * m.dt)
    assert np.iscomplexobj(R.values) and np.max(np.abs(R.values - want)) <= 1e-12 * abs(want[0])
    P.detach()


def test_inertial_peak():
    """uniform phi, 32 records one step apart with f0 dt = 2 pi / 16: f0 sits on bin 2 of 32 exactly.  The clockwise wave velocity
    fills that bin (omega = +f0 on this axis: see the module's doc); its mirror holds less than 1e-10 of it"""
    from niwqg_amd import particles, lagrangian
    m, A = uniform_wave_model("coupled", 2 * np.pi / 16)
    x, y = particle_set(m, 300)
    P = particles.attach(m, x, y, record_every=1, capacity=32, record=RECORD, wave=A_WAVE)
    m._ctx.step(31)
    S = lagrangian.spectrum(P, ["uvw", "uvt"], "boxcar", False)
    T = 32
    p = int(np.argmin(np.abs(S.omega - m.f)))
    assert abs(S.omega[p] - m.f) <= 1e-12 * m.f
    # the bin by the definition X_p = sum_n x_n e^{+2 pi i p n / T} of a series e^{-i f0 n dt}: 2 pi p / T = f0 dt, p = 2
    series = np.exp(-1j * m.f * m.dt * np.arange(T))
    Xp = np.abs(np.array([np.sum(series * np.exp(2j * np.pi * q * np.arange(T) / T)) for q in range(T)])) ** 2
    assert int(np.argmax(Xp)) == 2 and np.isclose(2 * np.pi * 2 / (T * m.dt), S.omega[p], rtol=1e-12, atol=0)
    mirror = int(np.argmin(np.abs(S.omega + m.f)))
    for name in ("uvw", "uvt"):
        v = S.values[name]
        print("inertial peak of %s: bin %d holds %.3e, its mirror %.3e, the rest at most %.3e" % (name, p, v[p], v[mirror], np.delete(v, p).max()))
        assert int(np.argmax(v)) == p
        assert v[mirror] <= 1e-10 * v[p]
    # all of the power: 1/2 a^2 |A|^2 per record (Parseval, boxcar)
    assert np.isclose(S.values["uvw"][p], 0.5 * (A_WAVE * abs(A)) ** 2, rtol=1e-10, atol=0)


# ---- 7. refusals and the lifecycle -----------------------------------------------------------------------------------------------
def test_refusals_leave_the_model_usable():
    import niwqg_amd
    from niwqg_amd import particles, lagrangian, _lib
    qg = make("qg", 64)
    with pytest.raises(ValueError, match="QGModel has no wave field"):
        particles.attach(qg, [1.0], [2.0], wave=1.0)
    with pytest.raises(ValueError, match="valid names"):
        particles.attach(qg, [1.0], [2.0], record_every=1, record=("uw",))
    P = particles.attach(qg, [1.0], [2.0])
    with pytest.raises(ValueError, match="valid names"):
        P.sample("uw")
    L = _lib.lib()
    assert L.nq_particles_wave(qg._ctx.h, 1.0, 1e-4, 0.0) == -4                 # QGModel, through the raw ABI
    assert L.nq_particles_clock(qg._ctx.h, 1e-4, 0.0) == -4
    qg._ctx.step(2)
    assert np.all(np.isfinite(P.positions()[0]))
    P.detach()

    m = drifter_model("coupled", 64)
    x, y = particle_set(m, 100)
    for wave in (0, -1, np.nan, np.inf, "x", True):
        with pytest.raises(ValueError, match="wave"):
            particles.attach(m, x, y, wave=wave)
    h = m._ctx.h
    assert L.nq_particles_wave(h, 1.0, m.f, 0.0) == -4                           # no particles attached
    assert b"no particles" in L.nq_last_error(h)
    m._step_forward()                                                            # (the lazy allocations of a first step)
    np.array(m.phi), np.array(m.u), np.array(m.v), np.array(m.q)
    b0 = m._ctx.device_bytes()
    P = particles.attach(m, x, y, record_every=1, capacity=4, record=("u", "v"))
    b1 = m._ctx.device_bytes()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert L.nq_particles_wave(h, bad, m.f, 0.0) == -1
    assert L.nq_particles_wave(h, 1.0, float("nan"), 0.0) == -1 and L.nq_particles_wave(h, 1.0, m.f, float("inf")) == -1
    assert m._ctx.device_bytes() == b1                                           # a refused call allocates nothing
    m._step_forward()
    assert L.nq_particles_wave(h, 1.0, m.f, 0.0) == -4                           # after a step
    assert b"moved already" in L.nq_last_error(h)
    assert L.nq_particles_clock(h, m.f, 0.0) == -4
    with pytest.raises(ValueError, match="'uvt' needs"):                         # as "uv" does without u or v
        lagrangian.spectrum(P, "uvt")
    with pytest.raises(ValueError, match="'uvw' needs"):
        lagrangian.autocovariance(P, "uvw")
    with pytest.raises(RuntimeError, match="not recorded"):                      # the library checks for itself
        m._ctx.lagr_spectrum(_lib.LAGR_UVT, 2, 2, np.ones(2), False, 1, np.arange(100, dtype=np.int32), np.array([0, 100], np.int32), 0)
    m._step_forward()                                                            # still the particles of wave=None, and usable
    assert np.all(np.isfinite(P.positions()[0]))
    P.detach()
    assert m._ctx.device_bytes() == b0
    P = particles.attach(m, x, y)
    plain = m._ctx.device_bytes()
    P.detach()
    # attach, detach and attach again with another amplitude
    ends = []
    for a in (0.5, 2.0):
        P = particles.attach(m, x, y, wave=a)
        assert P.wave == a
        assert m._ctx.device_bytes() == plain + 2 * 64 * 64 * 16                 # two more double2 planes
        assert L.nq_particles_wave(h, 1.0, m.f, 0.0) == -4                       # the mode is on already
        H = Host(m, x, y, a)
        H.step()
        H.step()
        assert H.error(P) <= 1e-12 * m.L
        ends.append(P.positions())
        P.detach()
        assert m._ctx.device_bytes() == b0
    assert np.max(np.hypot(ends[0][0] - ends[1][0], ends[0][1] - ends[1][1])) > 1e-6 * m.L
    # a slab rank
    s = niwqg_amd.CoupledModel.Model(slab=2, **notebook_kwargs(64, True))
    assert L.nq_particles_wave(s._ctx.sim.ranks[0].h, 1.0, 1e-4, 0.0) == -4
    assert L.nq_particles_clock(s._ctx.sim.ranks[0].h, 1e-4, 0.0) == -4
    with pytest.raises(NotImplementedError, match="slab"):
        particles.attach(s, [1.0], [2.0], wave=1.0)
