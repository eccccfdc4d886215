"""Stretch mode of the Lagrangian particles (niwqg_amd/particles.py ``attach(..., stretch=True)``, nq_particles_tangent,
nq_any_particles_rk4_tangent): positions and the deformation gradient F against the numpy restatement
``particles.rk4_tangent`` fed with the model's own velocity (and phi) after every step, on every model class; the compressible
signal of drifter mode; positions and model outputs against runs without the mode; batching and determinism; the records;
``lagrangian.stretching`` against host sums; the reset; the refusals; an FTLE map on a lattice.

Shapes: 257 particles (one full 256-thread block and a one-particle tail), a handful within one cell of each periodic seam and a
handful more than one L outside the box; fused grids 64^2 (8 rows per workgroup in the velocity row pass) and 128^2, 48^2 on the
any-size path.  The bars of the restatement are those of ray mode's test: 1e-12 L for positions, 1e-12 max |F| for F.  Every
figure is printed before it is asserted (-s shows them).

Observed on an MI355X:
  positions, max |device - rk4_tangent| after 20 steps, every case      2.3e-10 m  (bar 1e-12 L = 1.3e-6 m)
  F, max |device - rk4_tangent| after 20 steps, every case              7.8e-16    (bar 1e-12 max |F| = 1.2e-12 .. 1.9e-12); max |F - I| 0.48 .. 1.1
  max |det F - 1| with wave=1.0 against wave=None, 64^2 / 48^2          8.6e-2 against 2.8e-3 (x30) / 6.9e-2 against 2.9e-3 (x24)
  positions against a plain run                                          bit-identical without the wave; 2.9e-11 m with wave=1.0
  records, "lnsigma" against ln_sigma(columns) / "det" against det       1.4e-17 / 0 (bar 1e-14)
  lagrangian.stretching against the host sums                            1.8e-15 at most (bar 1e-12)
"""
import ctypes

import numpy as np
import pytest

from test_gpu_spectra import make
from test_gpu_particles import outputs, assert_same, set_tmax, velocity
from test_gpu_drifters import drifter_model

pytestmark = pytest.mark.gpu

N = 257
NAMES = ("f11", "f12", "f21", "f22", "lnsigma", "det")


def model(kind, nx, **kw):
    return make("qg", nx, "filter", **kw) if kind == "qg" else drifter_model(kind, nx, **kw)


def particle_set(m, n=N, seed=5):
    """random points; the first ones within one cell of each periodic seam, then more than one L outside the box"""
    L, dx = m.L, m.L / m.nx
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(0, L, n), rng.uniform(0, L, n)
    special = [(0.3 * dx, 0.5 * L), (L - 0.4 * dx, 0.25 * L), (0.6 * L, 0.2 * dx), (0.1 * L, L - 0.7 * dx), (0.9 * dx, L - 0.1 * dx),
               (0.0, 0.0), (np.nextafter(L, 0), np.nextafter(L, 0)),
               (-1.3 * L, 0.5 * L), (2.6 * L, -1.7 * L), (41.2 * L, -17.9 * L), (0.4 * L, 3.0 * L + 0.2 * dx), (-2.0 * L - 0.3 * dx, 5.5 * L)]
    for i, (a, b) in enumerate(special):
        x[i], y[i] = a, b
    return x, y


def eye(n=N):
    return np.tile(np.eye(2), (n, 1, 1))


class Host(object):
    """a host copy of the particles and their F, advanced with particles.rk4_tangent from the fields the model returns after every
    step (the model itself is stepped here)"""

    def __init__(self, m, x, y, F=None, wave=None):
        self.m, self.x, self.y, self.wave = m, np.array(x), np.array(y), wave
        self.F = eye(len(x)) if F is None else np.array(F)
        self.t0, self.s = m.t, 0
        self.refresh()

    def refresh(self):
        self.U0 = velocity(self.m)
        self.P0 = np.array(self.m.phi) if self.wave is not None else None

    def step(self):
        from niwqg_amd import particles
        m = self.m
        m._step_forward()
        U1 = velocity(m)
        kw = {}
        if self.wave is not None:
            kw = dict(P0=self.P0, P1=np.array(m.phi), a=self.wave, f0=m.f, t=self.t0 + self.s * m.dt)
        self.x, self.y, self.F = particles.rk4_tangent(self.x, self.y, self.F, self.U0, U1, m.U, m.dt, m.L, **kw)
        self.U0 = U1
        if self.wave is not None:
            self.P0 = kw["P1"]
        self.s += 1

    def check(self, P, tag=""):
        (xa, ya), Fa = P.positions(), P.deformation()
        ex = max(np.max(np.abs(xa - self.x)), np.max(np.abs(ya - self.y)))
        eF, top = np.max(np.abs(Fa - self.F)), np.max(np.abs(self.F))
        off = np.max(np.abs(Fa - np.eye(2)))
        print("stretch %s: max |device - rk4_tangent| positions %.3e (bar %.3e), F %.3e (bar %.3e); max |F - I| = %.3e"
              % (tag, ex, 1e-12 * self.m.L, eF, 1e-12 * top, off))
        assert Fa.shape == (len(self.x), 2, 2)
        assert ex <= 1e-12 * self.m.L and eF <= 1e-12 * top
        assert off > 1e-3                                     # agreement at the identity cannot pass
        return Fa


# ---- 1. the restatement ----------------------------------------------------------------------------------------------------------
def check_restatement(kind, nx, wave=None, nsteps=20):
    from niwqg_amd import particles
    A, B = model(kind, nx), model(kind, nx)
    assert getattr(A, "_any_size", False) == (nx == 48)
    x, y = particle_set(A)
    P = particles.attach(A, x, y, wave=wave, stretch=True)
    assert P.stretch and P.stretch_step0 == 0
    assert np.array_equal(P.deformation(), eye())
    H = Host(B, x, y, wave=wave)
    set_tmax(A, nsteps)
    A.run()
    for _ in range(nsteps):
        H.step()
    assert A.tc == B.tc == nsteps
    Fa = H.check(P, "%s %d%s" % (kind, nx, "" if wave is None else " wave=%g" % wave))
    xa, ya = P.positions()
    assert np.max(np.hypot(xa - x, ya - y)) > 1e-5 * A.L
    P.detach()
    return Fa


@pytest.mark.parametrize("kind, nx", [("coupled", 64), ("uncoupled", 64), ("ybj", 64), ("qg", 64), ("coupled", 128)])
def test_restatement_fused(kind, nx):
    check_restatement(kind, nx)


@pytest.mark.parametrize("kind", ["coupled", "qg"])
def test_restatement_anysize(kind):
    check_restatement(kind, 48)


def test_restatement_from_a_given_F():
    """a starting F other than the identity, through attach(stretch=F0)"""
    from niwqg_amd import particles
    A, B = model("coupled", 64), model("coupled", 64)
    x, y = particle_set(A)
    F0 = eye() + 0.3 * np.random.default_rng(3).standard_normal((N, 2, 2))
    P = particles.attach(A, x, y, stretch=F0)
    assert np.array_equal(P.deformation(), F0)
    H = Host(B, x, y, F=F0)
    A._ctx.step(5)
    for _ in range(5):
        H.step()
    H.check(P, "coupled 64 from F0")


# ---- 2. drifter mode together with stretch: the compressible case ------------------------------------------------------------------
@pytest.mark.parametrize("nx", [64, 48])
def test_drifters_with_stretch(nx):
    from niwqg_amd import particles
    Fw = check_restatement("coupled", nx, wave=1.0)
    F0 = check_restatement("coupled", nx)                     # wave=None from the same state
    dw, d0 = np.max(np.abs(particles.det(Fw) - 1)), np.max(np.abs(particles.det(F0) - 1))
    print("stretch coupled %d: max |det F - 1| = %.3e with wave=1.0, %.3e with wave=None (x%.1f)" % (nx, dw, d0, dw / d0))
    assert dw > 10 * d0


# ---- 3. positions are those of a run without the mode -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, nx, wave", [("coupled", 64, None), ("coupled", 64, 1.0), ("qg", 64, None), ("coupled", 48, None)])
def test_positions_are_those_of_a_plain_run(kind, nx, wave):
    from niwqg_amd import particles
    A, B = model(kind, nx), model(kind, nx)
    x, y = particle_set(A)
    P, Q = particles.attach(A, x, y, wave=wave, stretch=True), particles.attach(B, x, y, wave=wave)
    for m in (A, B):
        for _ in range(10):
            m._step_forward()
    (xa, ya), (xb, yb) = P.positions(), Q.positions()
    err = max(np.max(np.abs(xa - xb)), np.max(np.abs(ya - yb)))
    print("stretch %s %d wave=%s: positions against a plain run %.3e (bar %.3e), bit-identical: %s"
          % (kind, nx, wave, err, 1e-12 * A.L, np.array_equal(xa, xb) and np.array_equal(ya, yb)))
    assert err <= 1e-12 * A.L
    assert np.max(np.hypot(xa - x, ya - y)) > 1e-5 * A.L


# ---- 4. the model is that of a run without the mode ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["coupled", "uncoupled", "ybj", "qg"])
def test_model_outputs_are_those_of_a_run_without_stretch(kind):
    from niwqg_amd import particles
    A, C = model(kind, 64, tdiags=3), model(kind, 64, tdiags=3)
    for m in (A, C):
        m.twrite = 5
        set_tmax(m, 12)
    x, y = particle_set(A)
    P = particles.attach(A, x, y, record_every=3, capacity=4, record=("f11", "lnsigma", "det"), stretch=True)
    A.run()
    C.run()
    assert_same(outputs(A, kind), outputs(C, kind), kind)     # bit for bit, but the atomically reduced scalars (1e-12)
    assert np.max(np.abs(P.deformation() - np.eye(2))) > 1e-4
    P.detach()
    assert A._ctx.device_bytes() == C._ctx.device_bytes()


# ---- 5. batching and determinism -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, wave", [("coupled", None), ("coupled", 1.0), ("qg", None)])
def test_batching_and_determinism(kind, wave):
    from niwqg_amd import particles
    res = []
    for mode in ("batched", "single", "batched"):
        m = model(kind, 64)
        x, y = particle_set(m)
        P = particles.attach(m, x, y, record_every=2, capacity=3, record=NAMES, wave=wave, stretch=True)
        if mode == "batched":
            m._ctx.step(8)
        else:
            for _ in range(8):
                m._ctx.step(1)
        tr = P.trajectory()
        assert list(tr.step) == [4, 6, 8]
        res.append([*P.positions(), P.deformation(), tr.x, tr.y] + [tr.values[c] for c in NAMES])
    assert np.max(np.abs(res[0][2] - np.eye(2))) > 1e-4
    for other in res[1:]:
        for a, b in zip(res[0], other):
            assert np.array_equal(a, b)


# ---- 6. records ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, nx", [("coupled", 64), ("qg", 64), ("coupled", 48)])
def test_records(kind, nx):
    from niwqg_amd import particles
    m = model(kind, nx)
    x, y = particle_set(m)
    P = particles.attach(m, x, y, record_every=2, capacity=8, record=("u",) + NAMES, stretch=True)
    for _ in range(6):
        m._step_forward()
    tr = P.trajectory()
    assert list(tr.step) == [0, 2, 4, 6]
    v = tr.values
    F = np.stack([np.stack([v["f11"], v["f12"]], -1), np.stack([v["f21"], v["f22"]], -1)], -2)          # (T, n, 2, 2)
    assert np.array_equal(F[0], eye())                        # the record of step 0: the identity, after the mode was set
    assert np.array_equal(v["lnsigma"][0], np.zeros(N)) and np.array_equal(v["det"][0], np.ones(N))
    assert np.array_equal(F[-1], P.deformation())
    ls, dt = particles.ln_sigma(F), particles.det(F)
    e1 = np.max(np.abs(v["lnsigma"] - ls) / np.maximum(1.0, np.abs(ls)))
    e2 = np.max(np.abs(v["det"] - dt) / np.maximum(1.0, np.abs(dt)))
    print("stretch records %s %d: lnsigma against ln_sigma(columns) %.3e, det %.3e (bar 1e-14)" % (kind, nx, e1, e2))
    assert e1 <= 1e-14 and e2 <= 1e-14
    assert np.max(np.abs(ls[-1])) > 1e-4
    s = P.sample(NAMES)
    for c in NAMES:
        assert np.array_equal(s[c], v[c][-1]), c
    assert "f11" not in P.sample()                            # the default list is the state's


def test_records_without_the_mode_hold_nan():
    from niwqg_amd import _lib
    m = model("qg", 64)
    x, y = particle_set(m)
    codes = (ctypes.c_int * 2)(_lib.PT_F11, _lib.PT_DET)      # through the raw ABI: attach accepts the names, the mode is set after it
    Lb, h = _lib.lib(), m._ctx.h
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert Lb.nq_particles_attach(h, N, dp(x), dp(y), m.L, m.L, 1, 4, 2, codes) == 0
    m._ctx.step(1)
    _, out = m._ctx.particles_records(N)
    assert out.shape == (2, 4, N) and np.all(np.isnan(out[:, 2:])) and np.all(np.isfinite(out[:, :2]))
    assert Lb.nq_particles_detach(h) == 0


# ---- 7. lagrangian.stretching ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, nx, wave", [("coupled", 64, 1.0), ("qg", 64, None), ("coupled", 48, None)])
def test_stretching_tables(kind, nx, wave):
    from niwqg_amd import particles, lagrangian
    m = model(kind, nx)
    x, y = particle_set(m)
    P = particles.attach(m, x, y, record_every=2, capacity=8, record=("f11", "f12", "u", "f21", "f22"), wave=wave, stretch=True)
    for _ in range(10):
        m._step_forward()
    groups = np.zeros(N, np.int64)                            # three groups of unequal size, one of them of size 1
    groups[100:] = 2
    groups[17] = 1
    S = lagrangian.stretching(P, groups=groups)
    ref = lagrangian.reference_stretching(P.trajectory(), groups=groups)
    assert list(S.counts) == [99, 1, 157] and S.mean_lnsigma.shape == (6, 3)
    for key in ("mean_lnsigma", "var_lnsigma", "mean_det", "var_det"):
        a, b = getattr(S, key), ref[key]
        # the variance is a difference of two means: its bar is that of the means it is formed from
        scale = np.abs(b) if key.startswith("mean") else np.abs(b) + ref["mean" + key[3:]] ** 2
        err = np.max(np.abs(a - b) / np.where(scale > 0, scale, 1.0))
        print("stretching %s %d: %s against the host sums %.3e (bar 1e-12)" % (kind, nx, key, err))
        assert err <= 1e-12
    assert np.max(np.abs(S.mean_lnsigma[-1])) > 1e-4
    S2 = lagrangian.stretching(P, groups=groups)
    for key in ("mean_lnsigma", "var_lnsigma", "mean_det", "var_det"):
        assert np.array_equal(getattr(S, key), getattr(S2, key))
    f = S.ftle()
    assert f.shape == (6, 3) and np.all(np.isnan(f[0])) and np.all(np.isfinite(f[1:]))
    assert np.allclose(f[1:], S.mean_lnsigma[1:] / (S.t[1:] - S.t[0])[:, None], rtol=1e-15, atol=0)
    one = lagrangian.stretching(P)                            # without groups: (T,)
    assert one.mean_lnsigma.shape == (6,) and np.isnan(one.ftle()[0])
    lam = lagrangian.ftle(P)
    assert np.array_equal(lam, P.sample("lnsigma")["lnsigma"] / (S.t[-1] - S.t[0]))


# ---- 8. the reset ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [64, 48])
def test_reset_deformation(nx):
    from niwqg_amd import particles, lagrangian
    m = model("coupled", nx)
    x, y = particle_set(m)
    P = particles.attach(m, x, y, record_every=1, capacity=3, record=("f11", "f12", "f21", "f22"), stretch=True)
    for _ in range(4):
        m._step_forward()
    assert np.max(np.abs(P.deformation() - np.eye(2))) > 1e-5 and P.stretch_step0 == 0
    before = P.trajectory()
    P.reset_deformation()
    assert np.array_equal(P.deformation(), eye()) and P.stretch_step0 == 4
    after = P.trajectory()
    assert list(after.step) == list(before.step) and np.array_equal(after.values["f11"], before.values["f11"])     # no record written
    with pytest.raises(RuntimeError, match="before the reset at particle step 4"):
        lagrangian.stretching(P)
    for _ in range(2):
        m._step_forward()
    with pytest.raises(RuntimeError, match="before the reset"):      # records 4 (old), 5, 6
        lagrangian.stretching(P)
    m._step_forward()                                          # records 5, 6, 7: all written after the reset
    S = lagrangian.stretching(P)
    ref = lagrangian.reference_stretching(P.trajectory())
    assert np.allclose(S.mean_lnsigma, ref["mean_lnsigma"], rtol=1e-12, atol=0)
    assert np.all(np.isfinite(S.ftle())) and S.t0 < S.t[0]     # t0 is the reset's time: no record sits on it
    assert np.allclose(S.ftle(), S.mean_lnsigma / (S.t - S.t0), rtol=1e-15, atol=0)
    # F restarted from the identity at step 4: one host step from there
    H = Host(m, *P.positions(), F=P.deformation())
    H.step()
    Fa = P.deformation()
    assert np.max(np.abs(Fa - H.F)) <= 1e-12 * np.max(np.abs(H.F))


# ---- 9. refusals and the lifecycle -------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_model_usable():
    from niwqg_amd import particles, lagrangian, _lib
    Lb = _lib.lib()
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    m, twin = model("coupled", 64), model("coupled", 64)
    x, y = particle_set(m)
    k, l = np.full(N, 1e-4), np.full(N, -2e-4)
    h = m._ctx.h
    with pytest.raises(ValueError, match="exclude each other"):
        particles.attach(m, x, y, rays=(k, l), stretch=True)
    with pytest.raises(ValueError, match="shape"):
        particles.attach(m, x, y, stretch=np.ones((N, 2)))
    bad = eye()
    bad[N - 1, 1, 0] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        particles.attach(m, x, y, stretch=bad)
    assert "_particles" not in m.__dict__
    assert Lb.nq_particles_tangent(h, None) == -4 and b"no particles" in Lb.nq_last_error(h)
    m._step_forward()                                                            # (the lazy allocations of a first step)
    twin._step_forward()
    b0 = m._ctx.device_bytes()
    P = particles.attach(m, x, y, record_every=1, capacity=4, record=("u", "v"))
    b1 = m._ctx.device_bytes()
    for name in NAMES:                                                           # the names without the mode
        with pytest.raises(ValueError, match="need stretch mode"):
            P.sample(name)
        assert Lb.nq_particles_sample(h, 1, (ctypes.c_int * 1)(particles._CODES[name]), dp(np.empty(N))) == -1
    with pytest.raises(ValueError, match="need stretch mode"):
        particles.attach(twin, x, y, record_every=1, record=("det",))
    with pytest.raises(RuntimeError, match="without stretch="):
        P.deformation()
    with pytest.raises(ValueError, match="without stretch="):
        lagrangian.stretching(P)
    out = np.empty((4, N))
    assert Lb.nq_particles_get_tangent(h, dp(out)) == -4 and Lb.nq_particles_tangent_reset(h) == -4
    F0 = np.ascontiguousarray(eye().reshape(N, 4).T)
    F0[2, 5] = np.nan
    assert Lb.nq_particles_tangent(h, dp(F0)) == -1 and b"not finite" in Lb.nq_last_error(h)
    assert m._ctx.device_bytes() == b1                                           # a refused call allocates nothing
    m._step_forward()
    twin._step_forward()
    assert Lb.nq_particles_tangent(h, None) == -4 and b"moved already" in Lb.nq_last_error(h)      # after a step
    m._step_forward()                                                            # still the particles of stretch=None, and usable
    twin._step_forward()
    assert np.all(np.isfinite(P.positions()[0]))
    P.detach()
    assert m._ctx.device_bytes() == b0
    # ray mode and the tangent exclude each other, in either order, through the raw ABI
    P = particles.attach(m, x, y, rays=(k, l))
    assert Lb.nq_particles_tangent(h, None) == -4 and b"ray mode" in Lb.nq_last_error(h)
    P.detach()
    P = particles.attach(m, x, y)
    plain = m._ctx.device_bytes()
    P.detach()
    P = particles.attach(m, x, y, wave=1.0, stretch=True)                        # either order relative to the wave: here after it
    assert m._ctx.device_bytes() == plain + 2 * 64 * 64 * 16 + 4 * N * 8         # the wave's two phi planes; 32 B a particle, no plane
    P.detach()
    P = particles.attach(m, x, y, stretch=True)
    assert m._ctx.device_bytes() == plain + 4 * N * 8
    assert Lb.nq_particles_rays(h, dp(k), dp(l), 1.0) == -4 and b"stretch mode" in Lb.nq_last_error(h)
    assert Lb.nq_particles_tangent(h, None) == -4 and b"on already" in Lb.nq_last_error(h)
    assert m._ctx.device_bytes() == plain + 4 * N * 8
    assert Lb.nq_particles_wave(h, 1.0, m.f, m.t) == 0                           # and the wave after the tangent
    assert m._ctx.device_bytes() == plain + 2 * 64 * 64 * 16 + 4 * N * 8
    assert Lb.nq_lagr_stretching(h, 2, 1, None, None, dp(np.empty(8))) == -1     # record_every = 0
    with pytest.raises(ValueError, match="record_every = 0"):
        lagrangian.stretching(P)
    P.detach()
    # the f-columns not all recorded
    P = particles.attach(m, x, y, record_every=1, capacity=4, record=("f11", "f22"), stretch=True)
    m._step_forward()
    twin._step_forward()
    with pytest.raises(ValueError, match="needs 'f11', 'f12', 'f21', 'f22' recorded"):
        lagrangian.stretching(P)
    order, offs = np.arange(N, dtype=np.int32), np.array([0, N], np.int32)
    with pytest.raises(RuntimeError, match="must be recorded"):
        m._ctx.lagr_stretching(2, 1, order, offs)
    with pytest.raises(RuntimeError, match="nq_lagr_spectrum"):                  # no Lagrangian spectra of the new columns
        m._ctx.lagr_spectrum(_lib.PT_F11, 2, 2, np.ones(2), False, 1, order, offs, 0)
    P.detach()
    assert m._ctx.device_bytes() == b0
    # after every refusal the model is still usable: a plain step afterwards matches the twin's
    m._step_forward()
    twin._step_forward()
    assert m.tc == twin.tc and np.array_equal(np.array(m.qh), np.array(twin.qh)) and np.array_equal(np.array(m.phih), np.array(twin.phih))


def test_slab_ranks_refuse():
    import niwqg_amd
    from niwqg_amd import particles, _lib
    from test_oracle_golden import notebook_kwargs
    Lb = _lib.lib()
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    s = niwqg_amd.CoupledModel.Model(slab=2, **notebook_kwargs(64, True))
    with pytest.raises(NotImplementedError, match="slab"):
        particles.attach(s, [1.0], [2.0], stretch=True)
    h = s._ctx.sim.ranks[0].h
    assert Lb.nq_particles_tangent(h, None) == -4 and Lb.nq_particles_get_tangent(h, dp(np.ones(4))) == -4
    assert Lb.nq_particles_tangent_reset(h) == -4
    assert Lb.nq_lagr_stretching(h, 2, 1, None, None, dp(np.ones(8))) == -4


# ---- 10. a map of the finite-time Lyapunov exponent ----------------------------------------------------------------------------------
def test_ftle_map_on_a_lattice():
    from niwqg_amd import particles, lagrangian
    m = make("qg", 64, "filter")                              # the Lamb dipole (with its smooth random vorticity)
    x, y = particles.lattice(m, 8)
    P = particles.attach(m, x, y, stretch=True)
    assert np.all(np.isnan(lagrangian.ftle(P)))               # t = t0
    m._ctx.step(20)
    lam = lagrangian.ftle(P).reshape(8, 8)
    print("FTLE map on the dipole after 20 steps: %.3e .. %.3e 1/s" % (lam.min(), lam.max()))
    assert np.all(np.isfinite(lam)) and np.all(lam > 0)
