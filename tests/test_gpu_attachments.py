"""The three attachments of the step together (niwqg_amd/_attach.py, csrc/nq_lib.hip: DevOwned, RecordRing and nq_step's hook
pair): forcing, particles and the recorder on one model, both rings wrapping, batched against single
steps bit for bit, and the one byte counter through attach, the first spectrum, every detach order and close."""
import numpy as np
import pytest

from test_gpu_forcing import pair, amplitudes

pytestmark = pytest.mark.gpu

NSTEPS = 8
# (kind, nx): 64 is a fused context (the library's hooks), 96 the any-size path (the Python Ring and the shared _step_etdrk4,
# once per family)
CASES = [("coupled", 64), ("coupled", 96), ("qg", 96)]


def attached(kind, nx):
    """a model with forcing, 37 recording particles and a recorder; both rings (3 records, one every 2 steps) wrap in 8 steps"""
    from niwqg_amd import forcing, frequency, particles
    m, _, init, _ = pair(kind, nx, "filter", oracle=False)
    init(m)
    m._step_forward()                          # (the first diagnostics tick allocates the context's own tick planes)
    b0 = m._ctx.device_bytes()
    qg = kind == "qg"
    Aq, Aphi = amplitudes(nx, "q" if qg else "q+phi")
    F = forcing.attach(m, q=Aq, phi=Aphi, seed=11)
    rng = np.random.default_rng(5)
    P = particles.attach(m, rng.uniform(0, m.L, 37), rng.uniform(0, m.W, 37), record_every=2, capacity=3,
                         record=("q",) if qg else ("q", "phi"))
    R = frequency.attach(m, 4, every=2, length=3, fields=("q", "psi") if qg else None)
    return m, F, P, R, b0


def batched(m, n):
    """n steps as ``run`` takes them: the steps between two host-visible events go into one nq_step call (fused contexts; the
    any-size path steps from Python).  Returns the longest such call."""
    if getattr(m, "_any_size", False):
        for _ in range(n):
            m._step_forward()
        return 0
    longest = 0
    while n > 0:
        quiet = m._quiet_steps(n)
        if quiet > 0:
            m._ctx.step(quiet)
            for _ in range(quiet):
                m.tc += 1
                m.t += m.dt
            m._after_steps()
        m._step_forward()
        n -= quiet + 1
        longest = max(longest, quiet)
    return longest


@pytest.mark.parametrize("kind, nx", CASES)
def test_three_attachments_batched_and_stepwise(kind, nx):
    A, FA, PA, RA, a0 = attached(kind, nx)
    B, FB, PB, RB, b0 = attached(kind, nx)
    fused = nx == 64
    assert batched(A, NSTEPS) == (NSTEPS - 1 if fused else 0)       # (quiet steps: all but the last go in one call)
    for _ in range(NSTEPS):
        B._step_forward()
    # the state, and every attachment's view of the run
    for n in ("qh", "ph") + (() if kind == "qg" else ("phih",)):
        a, b = np.array(getattr(A, n)), np.array(getattr(B, n))
        assert np.all(np.isfinite(a)) and np.array_equal(a, b), n
    for a, b in zip(PA.positions(), PB.positions()):
        assert np.all(np.isfinite(a)) and np.array_equal(a, b)
    ta, tb = PA.trajectory(), PB.trajectory()
    assert np.array_equal(ta.step, [5, 7, 9]) and np.array_equal(tb.step, ta.step) and np.array_equal(ta.t, tb.t)   # (attached at tc = 1)
    assert np.array_equal(ta.x, tb.x) and np.array_equal(ta.y, tb.y) and sorted(ta.values) == sorted(PA.record)
    for n in PA.record:
        assert ta.values[n].shape == (3, 37) and np.array_equal(ta.values[n], tb.values[n]), n
    assert np.array_equal(ta.x[-1], PA.positions()[0])              # the newest record is the current position
    assert RA.info() == RB.info() == {"written": 5, "held": 3, "steps": NSTEPS}
    for n in RA.fields:
        sa, sb = RA.series(n), RB.series(n)
        assert np.array_equal(sa.step, [4, 6, 8]) and np.array_equal(sb.step, sa.step)
        assert np.any(sa.values != 0) and np.array_equal(sa.values, sb.values), n
    assert FA.state() == FB.state() == {"seed": 11, "step": NSTEPS}
    assert FA.work() == FB.work() and FA.work()["q"] != 0.0
    # the engine of the spectrum counts as the recorder's
    before = A._ctx.device_bytes()
    SA, SB = RA.spectrum("boxcar"), RB.spectrum("boxcar")
    for n in RA.fields:
        assert np.all(np.isfinite(SA.values[n])) and np.array_equal(SA.values[n], SB.values[n]), n
    if fused:
        assert A._ctx.device_bytes() > before
        assert A._ctx.device_bytes() == B._ctx.device_bytes()
    # detach in both orders: every detach gives bytes back, the last one all of them
    for m, order, base in ((A, (RA, PA, FA), a0), (B, (FB, PB, RB), b0)):
        for att in order:
            held = m._ctx.device_bytes()
            att.detach()
            if fused:
                assert m._ctx.device_bytes() < held, type(att).__name__
        if fused:
            assert m._ctx.device_bytes() == base
        assert not any(s in m.__dict__ for s in ("_particles", "_forcing", "_frequency"))
    A._step_forward()                                               # the model steps on without them
    assert np.all(np.isfinite(np.array(A.qh)))


@pytest.mark.parametrize("kind, nx", CASES)
def test_close_with_everything_attached(kind, nx):
    C, FC, PC, RC, _ = attached(kind, nx)
    batched(C, 3)
    RC.spectrum("boxcar")
    C._ctx.close()                                                  # nq_destroy releases the three itself
    if nx == 64:
        assert C._ctx.h is None
    D = attached(kind, nx)[0]                                       # and the device is fine afterwards
    batched(D, 2)
    assert np.all(np.isfinite(np.array(D.qh)))
