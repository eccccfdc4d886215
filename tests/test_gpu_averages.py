"""Time-mean and covariance maps accumulated in the step (niwqg_amd/averages.py, nq_avg_*, nq_any_moments; DESIGN.md section
5l): one sample is the field, the sums are the sequential fp64 sums of the sampled states (first moments bit for bit, products
within the contraction allowance), the cadence inside batched calls, non-interference and lifecycle, the hook order after the
forcing, determinism, the statistics' own identities, and the library's refusals.

Shapes: the Kernel family's row kernel at nx = 64 (eight rows per workgroup), 512 (one row, one wave) and 1024 (the first
multi-wave plan); QGModel (the element-wise kernel on its two download planes) at 64 with and without the passive scalar; the
any-size path at 48 and 96."""
import ctypes

import numpy as np
import pytest

from test_gpu_spectra import make
from test_oracle_golden import notebook_kwargs

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
REAL = {"coupled": ("q", "q_psi", "phi2"), "uncoupled": ("q", "q_psi", "phi2"), "ybj": ("q", "q_psi", "phi2"), "qg": ("q",), "qgc": ("q", "c")}


def all_fields(kind):
    return REAL[kind] + (("phi",) if kind in ("coupled", "uncoupled", "ybj") else ())


def all_pairs(kind):
    r = REAL[kind]
    return tuple((a, b) for i, a in enumerate(r) for b in r[i:])


def any_size(m):
    return bool(getattr(m, "_any_size", False))


def advance(m, n, batched=False):
    """n steps: one batched library call on the fused contexts when asked for, else single steps"""
    if batched and not any_size(m):
        m._ctx.step(n)
        m._after_steps()
    else:
        for _ in range(n):
            m._step_forward()


def own(m, name):
    """the model's own read of a field (any-size q_psi: the plane field_pdfs forms there, m.q_psi is only current at a tick)"""
    if name == "phi2":
        p = np.array(m.phi)
        return p.real * p.real + p.imag * p.imag
    if name == "q_psi" and any_size(m):
        return m._pdf_planes(["q_psi"])["q_psi"][0].get()
    from niwqg_amd import flow
    if name in flow.NAMES:                                 # no attribute of the model: the numpy restatement from m.ph, m.phih, m.q_psi
        return flow.reference(m, [name])[name]
    return np.array(getattr(m, name))


def attach_all(m, kind, every):
    from niwqg_amd import averages
    return averages.attach(m, all_fields(kind), all_pairs(kind), every=every)


def one_sample(A):
    """the state as the averages see it: {name: plane} of one sample on zeroed sums (0 + x = x exactly)"""
    A.reset()
    A.sample()
    R = A.result()
    assert R.n == 1
    return {n: R.sums[n].copy() for n in A.fields}


CASES = [("coupled", 64, "filter"), ("coupled", 512, "filter"), ("coupled", 1024, "filter"), ("uncoupled", 64, "filter"),
         ("ybj", 64, "filter"), ("coupled", 64, "mask"), ("qg", 64, "filter"), ("qgc", 64, "filter"),
         ("coupled", 48, "filter"), ("coupled", 96, "filter"), ("qgc", 48, "filter")]


# ---- 1. one sample is the field ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, nx, mask", CASES)
def test_one_sample_is_the_field(kind, nx, mask):
    from niwqg_amd import averages
    m = make(kind, nx, mask)
    if mask == "mask":
        assert m._dual
    assert averages.available(m) == list(all_fields(kind))
    A = attach_all(m, kind, 0)
    advance(m, 3)
    assert A.info() == {"n": 0, "steps": 3}
    A.sample()
    R = A.result()
    assert R.n == 1 and R.steps == 3
    same_plane = kind in ("qg", "qgc") or any_size(m)          # the sample reads the very plane the model's read returns
    for n in A.fields:
        got, want = R.sums[n], own(m, n)
        assert got.shape == (nx, nx) and got.dtype == (np.complex128 if n == "phi" else np.float64) and np.any(want != 0)
        err, top = np.abs(got - want).max(), np.abs(want).max()
        print("%s %d %s %s: max |S - field| / max |field| = %.3g" % (kind, nx, mask, n, err / top))
        if same_plane and n != "phi2":
            assert np.array_equal(got, want), n
        elif same_plane:
            # |phi|^2 is formed from the plane, re re + im im: the device may contract it into one fma, numpy rounds both products
            # and the sum; each is within 2 ulp of the exact value, so the two are within 4 ulp of each other
            assert np.all(np.abs(got - want) <= 4 * U * want), n
        else:
            # two device routes to one quantity (the row kernel's registers / the read's transforms): the standing 1e-12
            assert err <= 1e-12 * top, (n, err, top)
    for a, b in A.products:                                    # one sample of a product is x y, up to the contraction
        x, y = R.sums[a], R.sums[b]
        assert np.all(np.abs(R.sums[a + "*" + b] - x * y) <= 2 * U * np.abs(x * y)), (a, b)
    A.detach()


# ---- 2, 6, 7. the sequential sum, determinism, the statistics -----------------------------------------------------------------------
SEQ = [("coupled", 64, "filter", None), ("coupled", 512, "filter", None), ("coupled", 1024, "filter", ("q_psi", "phi2")),
       ("coupled", 64, "mask", None), ("ybj", 64, "filter", None), ("qgc", 64, "filter", None), ("coupled", 48, "filter", None)]


def run_b(kind, nx, mask, names, nsteps=7):
    from niwqg_amd import averages
    m = make(kind, nx, mask)
    if names is None:
        B = attach_all(m, kind, 1)
    else:
        B = averages.attach(m, names, tuple((a, b) for i, a in enumerate(names) for b in names[i:]), every=1)
    advance(m, nsteps, batched=True)
    return m, B, B.result()


@pytest.fixture(scope="module")
def sequences():
    """(kind, nx, mask, names) -> (x_k of model A, model B, its result): run once, only read afterwards"""
    cache = {}

    def get(key):
        if key not in cache:
            from niwqg_amd import averages
            kind, nx, mask, names = key
            a = make(kind, nx, mask)
            A = attach_all(a, kind, 0) if names is None else averages.attach(a, names, every=0)
            xs = []
            for _ in range(7):
                advance(a, 1)
                xs.append(one_sample(A))
            cache[key] = (xs,) + run_b(kind, nx, mask, names)
        return cache[key]
    return get


@pytest.mark.parametrize("key", SEQ)
def test_sums_are_the_sequential_sums(sequences, key):
    from niwqg_amd import averages
    xs, m, B, R = sequences(key)
    assert R.n == 7 and R.steps == 7 and B.info() == {"n": 7, "steps": 7}
    sums = {n: np.zeros_like(xs[0][n]) for n in B.fields}
    sums.update({a + "*" + b: np.zeros(xs[0][a].shape) for a, b in B.products})
    mag = {k: np.zeros(v.shape) for k, v in sums.items() if "*" in k}
    for x in xs:
        averages.accumulate(sums, x)
        for a, b in B.products:
            mag[a + "*" + b] += np.abs(x[a] * x[b])
    for n in B.fields:
        assert np.any(xs[-1][n] != xs[0][n]) or (key[0] == "ybj" and n in ("q", "q_psi")), n       # (the state moved)
        assert np.array_equal(R.sums[n], sums[n]), (n, np.abs(R.sums[n] - sums[n]).max())
    for a, b in B.products:
        k = a + "*" + b
        d = np.abs(R.sums[k] - sums[k])
        print("%s %s: max |S_dev - S_numpy| / allowance = %.3g" % (key, k, (d / np.maximum(2 * 7 * U * mag[k], 1e-300)).max()))
        assert np.all(d <= 2 * 7 * U * mag[k]), k


@pytest.mark.parametrize("key", [SEQ[0], SEQ[5], SEQ[6]])
def test_two_fresh_runs_are_bit_identical(sequences, key):
    _, _, _, R = sequences(key)
    _, _, R2 = run_b(*key)
    assert sorted(R.sums) == sorted(R2.sums) and R2.n == R.n
    for k in R.sums:
        assert R.sums[k].tobytes() == R2.sums[k].tobytes(), k


@pytest.mark.parametrize("key", [SEQ[0], SEQ[1], SEQ[5], SEQ[6]])
def test_statistics(sequences, key):
    _, _, B, R = sequences(key)
    real = [n for n in B.fields if n != "phi"]
    for a in real:
        v = R.variance(a)
        assert np.all(v >= -1e-12 * (R.sums[a + "*" + a] / R.n).max()), a
        assert np.array_equal(R.covariance(a, a), v)
        for b in real:
            c = R.correlation(a, b)
            ok = ~np.isnan(c)
            assert ok.any() and np.all(np.abs(c[ok]) <= 1 + 1e-9), (a, b)
            assert np.array_equal(ok, (v > 0) & (R.variance(b) > 0))
    with pytest.raises(KeyError, match="fields"):
        R.mean("zeta")


def test_steady_q_of_ybj(sequences):
    xs, m, B, R = sequences(SEQ[4])
    q, x = np.array(m.q), xs[0]["q"]
    top = np.abs(q).max()
    for k in xs:
        assert np.array_equal(k["q"], x)                       # steady: every sample sees the same rows
    # the same value added n times: the sequential sum is within n ulp of n x, point by point
    assert np.all(np.abs(R.mean("q") - x) <= R.n * U * np.abs(x))
    print("ybj: max |mean(q) - m.q| / max |q| = %.3g (bound %.3g), max |var| / max q^2 = %.3g"
          % (np.abs(R.mean("q") - q).max() / top, R.n * U, np.abs(R.variance("q")).max() / top ** 2))
    assert np.abs(R.mean("q") - q).max() <= R.n * U * top
    assert np.abs(R.variance("q")).max() <= R.n * U * top ** 2


# ---- 3. cadence ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, nx", [("coupled", 64), ("qgc", 64), ("coupled", 48)])
def test_cadence(kind, nx):
    from niwqg_amd import averages
    a, b = make(kind, nx), make(kind, nx)
    A, B = attach_all(a, kind, 0), attach_all(b, kind, 3)
    xs = []
    for step in range(1, 11):
        advance(a, 1)
        assert A.info() == {"n": 0, "steps": step}             # every = 0: never on its own
        if step in (3, 6, 9):
            xs.append(one_sample(A))
            A.reset()
    with pytest.raises(RuntimeError, match="no sample"):
        A.result()
    for n, batched in ((1, False), (4, True), (1, False), (3, True), (1, False)):     # 10 steps, single and batched calls mixed
        advance(b, n, batched)
    R = B.result()
    assert R.n == 3 and R.steps == 10
    sums = {n: np.zeros_like(xs[0][n]) for n in B.fields}
    sums.update({p + "*" + q: np.zeros(xs[0][p].shape) for p, q in B.products})
    mag = {k: np.zeros(v.shape) for k, v in sums.items() if "*" in k}
    for x in xs:
        averages.accumulate(sums, x)
        for p, q in B.products:
            mag[p + "*" + q] += np.abs(x[p] * x[q])
    for n in B.fields:
        assert np.array_equal(R.sums[n], sums[n]), n
    for k in mag:
        assert np.all(np.abs(R.sums[k] - sums[k]) <= 2 * 3 * U * mag[k]), k
    # reset keeps the step counter, and so the phase of `every`
    B.reset()
    assert B.info() == {"n": 0, "steps": 10}
    advance(b, 1)
    assert B.info()["n"] == 0
    advance(b, 1, True)
    assert B.info() == {"n": 1, "steps": 12}


# ---- 4. non-interference and lifecycle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["coupled", "qgc"])
def test_no_side_effects(kind):
    from test_gpu_particles import outputs, assert_same, set_tmax
    A, B = make(kind, 64, tdiags=3), make(kind, 64, tdiags=3)
    for m in (A, B):
        m.twrite = 5
        set_tmax(m, 20)
    b0 = A._ctx.device_bytes()
    Av = attach_all(A, kind, 1)
    nplanes = len(REAL[kind]) + len(all_pairs(kind)) + (2 if kind == "coupled" else 0)
    assert A._ctx.device_bytes() == b0 + nplanes * 64 * 64 * 8
    for m in (A, B):
        m.run()
    assert Av.info() == {"n": 20, "steps": 20}
    for name in ("qh", "ph") + (("phih",) if kind == "coupled" else ()):
        assert np.array_equal(np.array(getattr(A, name)), np.array(getattr(B, name))), name
    assert_same(outputs(A, kind), outputs(B, kind), kind)      # (its rounded scalars at 1e-12, everything else bit for bit)
    Av.detach()
    Av.detach()
    assert A._ctx.device_bytes() == B._ctx.device_bytes()
    with pytest.raises(RuntimeError, match="^averages: detached$"):
        Av.result()


def test_lifecycle_beside_the_other_attachments():
    from niwqg_amd import averages, forcing, frequency, particles
    from test_gpu_forcing import amplitudes
    from test_gpu_particles import particle_set
    m = make("coupled", 64)
    advance(m, 1)                                  # (what the first step allocates on its own is there before the count)
    b0 = m._ctx.device_bytes()
    Aq, Aphi = amplitudes(64, "q+phi")
    x, y = particle_set(m, 100)
    for order in ((0, 1, 2, 3), (3, 1, 0, 2), (2, 3, 1, 0)):
        att = [particles.attach(m, x, y), forcing.attach(m, q=Aq, phi=Aphi, seed=2), frequency.attach(m, 8, length=4),
               attach_all(m, "coupled", 1)]
        with pytest.raises(RuntimeError, match="already"):
            averages.attach(m, ["q"])
        advance(m, 3, batched=True)
        assert att[3].result().n == 3
        for i in order:
            b = m._ctx.device_bytes()
            att[i].detach()
            assert m._ctx.device_bytes() < b
        assert m._ctx.device_bytes() == b0
    with pytest.raises(RuntimeError, match="nq_avg_info"):
        m._ctx.avg_info()


def test_any_size_lifecycle():
    from niwqg_amd import averages
    m = make("coupled", 48)
    A = averages.attach(m, ["phi2"], [("phi2", "phi2")])
    with pytest.raises(RuntimeError, match="already"):
        averages.attach(m, ["q"])
    advance(m, 2)
    assert A.result().n == 2
    A.detach()
    with pytest.raises(RuntimeError, match="^averages: detached$"):
        A.sample()
    averages.attach(m, ["q"], every=0).detach()


# ---- 5. after forcing ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, nx", [("coupled", 64), ("qg", 64), ("coupled", 48)])
def test_the_sample_of_a_forced_step_is_the_forced_state(kind, nx):
    from niwqg_amd import averages, forcing
    from test_gpu_forcing import amplitudes
    Aq, _ = amplitudes(nx, "q")
    f, u = make(kind, nx), make(kind, nx)
    forcing.attach(f, q=Aq, seed=9)
    F, Un = averages.attach(f, ["q"], every=1), averages.attach(u, ["q"], every=1)
    advance(f, 1, batched=True)
    advance(u, 1, batched=True)
    got, want, other = F.result().sums["q"], np.array(f.q), Un.result().sums["q"]
    top = np.abs(want).max()
    if kind == "qg" or any_size(f):
        assert np.array_equal(got, want)
    else:
        assert np.abs(got - want).max() <= 1e-12 * top
    assert np.abs(got - other).max() > 1e-6 * top              # the kick is far above either tolerance


# ---- 8. refusals on the device side ------------------------------------------------------------------------------------------------
def test_library_refusals():
    from niwqg_amd import _lib
    m = make("qgc", 64)
    c, L = m._ctx, _lib.lib()
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    assert L.nq_avg_attach(c.h, 1, ints(_lib.AVG_PHI), 0, None, 1) == -1                          # no wave field on QGModel
    assert L.nq_avg_attach(c.h, 1, ints(_lib.AVG_QPSI), 0, None, 1) == -1
    assert L.nq_avg_attach(c.h, 1, ints(_lib.AVG_Q), 1, ints(_lib.AVG_Q, _lib.AVG_C), 1) == -1    # a pair naming a field not kept
    assert L.nq_avg_attach(c.h, 2, ints(_lib.AVG_Q, _lib.AVG_Q), 0, None, 1) == -1
    assert L.nq_avg_attach(c.h, 1, ints(_lib.AVG_Q), 0, None, -1) == -1
    assert L.nq_avg_sample(c.h) == -4 and L.nq_avg_detach(c.h) == -4                               # nothing got attached
    b0 = c.device_bytes()
    c.avg_attach([_lib.AVG_Q, _lib.AVG_C], [(_lib.AVG_C, _lib.AVG_Q)], 2)
    assert L.nq_avg_attach(c.h, 1, ints(_lib.AVG_Q), 0, None, 1) == -4                            # a second attach
    with pytest.raises(RuntimeError, match="plane 3 of 3"):
        c.avg_read(3)
    advance(m, 4, batched=True)                                                                  # the context still steps
    assert c.avg_info() == (2, 4, 3)
    c.avg_detach()
    assert c.device_bytes() == b0
    k = make("coupled", 64)
    assert L.nq_avg_attach(k._ctx.h, 2, ints(_lib.AVG_Q, _lib.AVG_PHI), 1, ints(_lib.AVG_Q, _lib.AVG_PHI), 1) == -1     # phi in a product
    assert L.nq_avg_attach(k._ctx.h, 1, ints(_lib.AVG_C), 0, None, 1) == -1
    advance(k, 1)


def test_slab_ranks_refuse():
    import niwqg_amd
    from niwqg_amd import averages, _lib
    m = niwqg_amd.CoupledModel.Model(slab=2, **notebook_kwargs(64, True))
    with pytest.raises(NotImplementedError, match="slab"):
        averages.attach(m, ["q"])
    L = _lib.lib()
    h = m._ctx.sim.ranks[0].h
    f = (ctypes.c_int * 1)(0)
    i3 = (ctypes.c_longlong * 3)()
    d = np.zeros(4)
    assert L.nq_avg_attach(h, 1, f, 0, None, 1) == -4
    assert L.nq_avg_detach(h) == -4
    assert L.nq_avg_sample(h) == -4
    assert L.nq_avg_reset(h) == -4
    assert L.nq_avg_info(h, i3) == -4
    assert L.nq_avg_read(h, 0, _lib._dptr(d)) == -4
