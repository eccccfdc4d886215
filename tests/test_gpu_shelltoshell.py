"""Shell-to-shell transfers (niwqg_amd/shelltoshell.py, csrc/nq_s2s.hpp): the device rows equal the numpy
restatement ``shelltoshell.reference``, their sum over the donor bands closes on the transfer the device bins by another path
(``spectral_transfer``), the band-to-band matrices are antisymmetric where the definitions say so, bands and calls are
bit-reproducible, nothing disturbs the run, and the models and grids without the transfers refuse.

Grids: 64 (eight rows per workgroup), 128 (four), 512 (one row, one wave), 1024 (two waves per row): the smallest shapes at which
the row plan changes; 2048 and 4096 once, closure only, 3 bands, on a band-limited state; the rows against
the reference at 256, 1024 and 2048, the closure on a broadband state at 4096, the two-pass tiles at 64 ... 512 and another column
split at 1024 are in tests/test_gpu_plan_ladder_analysis.py and the children of tests/test_gpu_plan_ladder.py, through ``check_rows``,
``check_closure`` and ``check_antisymmetry`` of this module.  States: those of test_gpu_flow.make, white part included (the
Nyquist lines carry energy), set and then advanced 3 steps, so quirks Q1 and Q2 are live ("broadband"); and a state band-limited
to shell nx/8, just set ("fresh"): nothing on the shells >= nx/2 and alias-free triple products (on CoupledModel psi carries up
to 2 nx/8 through q_w: the factors' top shells sum to 4 nx/8 < nx).

Bounds, all relative to sum_{Q, b} |T(b | Q)| of the name: device against numpy 1e-10 (DESIGN.md section 5f's bound for a device
table against numpy); closure and antisymmetry 1e-12, the project's standing bound of two device routes to one number."""
import numpy as np
import pytest

from test_oracle_golden import notebook_kwargs, K0, U0
from test_gpu_at_size import rough_kwargs
import test_gpu_flow
from test_gpu_flow import make, advance

pytestmark = pytest.mark.gpu

# one more mask for test_gpu_flow.make: the 2/3 rule, which makes the context keep both copies of q-hat (dual_q)
test_gpu_flow.MASKS.setdefault("dealias", dict(use_filter=False, dealias=True))

SIZES = (64, 128, 512, 1024)
KINDS = ("coupled", "uncoupled", "ybj", "qg")
CASES = [(k, nx, "none") for k in KINDS for nx in SIZES] + [("coupled", nx, "filter") for nx in SIZES] + [("coupled", 128, "dealias")]


def edges(nx):
    """eight sharp bands that cover every shell below nx/2"""
    return [0, 1, 2, 3, 4, 8, 16, max(nx // 4, 24), nx // 2]


def set_bandlimited(m, kind, top, seed=5):
    """q and phi with nothing on the shells > top"""
    from niwqg_amd.spectra import shell_of
    nx = m.nx
    rng = np.random.default_rng(seed + nx)
    n = np.append(np.arange(0, nx // 2), np.arange(-(nx // 2), 0))
    keep = shell_of(n[None, :], n[:, None]) <= top

    def noise(cplx):
        zh = np.zeros((nx, nx), np.complex128)
        zh[keep] = rng.standard_normal(keep.sum()) + 1j * rng.standard_normal(keep.sum())      # one transform per field
        zh[0, 0] = 0.0
        z = np.fft.ifft2(zh)
        return z if cplx else z.real
    if kind != "qg":                                      # phi first: set_q then inverts with THIS phi (set_phi does not, quirk Q2)
        p = noise(True)
        m.set_phi(0.2 * (1 + 0.5j) / np.sqrt(2) + 0.05 * p / np.abs(p).std())
    q = noise(False)
    m.set_q(U0 * K0 * q / q.std())
    return m


@pytest.fixture(scope="module")
def cases():
    """(kind, nx, mask, state) -> the model, the tables and the device result, formed once and only read afterwards; state
    "broadband": test_gpu_flow.make's after 3 batched steps, "fresh": band-limited to nx/8, just set"""
    cache = {}

    def get(kind, nx, mask, state="broadband"):
        from niwqg_amd import shelltoshell
        key = (kind, nx, mask, state)
        if key not in cache:
            m = make(kind, nx, mask)
            if state == "fresh":
                set_bandlimited(m, kind, nx // 8)
            else:
                advance(m, 3, batched=True)
            R = shelltoshell.shell_to_shell(m, edges(nx))
            assert list(R.names) == shelltoshell.available(m) and R.raw.shape == (8, 4, len(R.table[0]))
            cache[key] = dict(m=m, tab=R.table, R=R)
        return cache[key]
    yield get
    for c in cache.values():
        c["m"]._ctx.close()


# ---- 1. the device rows equal the reference --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, nx, mask", [c for c in CASES if c[1] <= 512])
def test_rows_equal_the_reference(cases, kind, nx, mask):
    c = cases(kind, nx, mask)
    m, R = c["m"], c["R"]
    assert bool(m._ctx.dual_q) == (mask == "dealias")
    check_rows(m, R, kind, nx, mask)


def check_rows(m, R, kind, nx, mask):
    """the rows of R against shelltoshell.reference on R's own table, 1e-10 of sum |T| per name"""
    from niwqg_amd import shelltoshell
    ref = shelltoshell.reference(m, R.table, R.names)
    for name in R.names:
        err, scale = np.abs(R.rows[name] - ref[name]).max(), np.abs(ref[name]).sum()
        print("%s %d %s %s: max |device - reference| / sum |T| = %.3g" % (kind, nx, mask, name, err / scale))
        assert scale > 0 and err <= 1e-10 * scale, (name, err, scale)
    # rows of the names the model lacks stay zero
    for row in set(range(4)) - {shelltoshell.ROWS[n][0] for n in R.names}:
        assert not R.raw[:, row].any()


# ---- 2. the sum over the donor bands closes on spectral_transfer ------------------------------------------------------------------
def check_closure(m, R, names, tag):
    from niwqg_amd.transfer import spectral_transfer
    st = spectral_transfer(m)
    for name in names:
        err, scale = np.abs(R.rows[name].sum(axis=0) - st.transfer[name]).max(), np.abs(R.rows[name]).sum()
        print("%s %s: closure %.3g" % (tag, name, err / scale))
        assert scale > 0 and err <= 1e-12 * scale, (name, err, scale)


@pytest.mark.parametrize("kind, nx", [(k, nx) for k in KINDS for nx in SIZES])
def test_closure_on_a_fresh_bandlimited_state(cases, kind, nx):
    c = cases(kind, nx, "none", "fresh")
    assert np.array_equal(c["tab"][:, :nx // 2].sum(axis=0), np.ones(nx // 2))
    check_closure(c["m"], c["R"], c["R"].names, "%s %d fresh" % (kind, nx))


@pytest.mark.parametrize("nx", SIZES)
def test_closure_after_steps_with_the_filter(cases, nx):
    """the filter leaves <= e^-34.5 = 1e-15 per step on the shells >= nx/2; CoupledModel's gradients are current after a step"""
    c = cases("coupled", nx, "filter")
    check_closure(c["m"], c["R"], c["R"].names, "coupled %d filter, 3 steps" % nx)


@pytest.mark.parametrize("nx", [2048, 4096])
def test_closure_on_the_larger_plans(nx):
    import niwqg_amd
    from niwqg_amd import shelltoshell
    m = niwqg_amd.CoupledModel.Model(**rough_kwargs(nx))
    set_bandlimited(m, "coupled", nx // 8)
    R = shelltoshell.shell_to_shell(m, [0, 16, nx // 16, nx // 2])
    assert R.raw.shape[0] == 3
    check_closure(m, R, shelltoshell.NAMES, "coupled %d" % nx)
    m._ctx.close()


# ---- 3. antisymmetry ---------------------------------------------------------------------------------------------------------------
def check_antisymmetry(R, name, tag):
    M = R.matrix(name)
    err, scale = np.abs(M + M.T).max(), np.abs(R.rows[name]).sum()
    print("%s %s: max |M + M^T| / sum |T| = %.3g" % (tag, name, err / scale))
    assert M.shape == (len(R.table),) * 2 and scale > 0 and np.abs(M).max() > 1e-6 * scale
    assert err <= 1e-12 * scale, (name, err, scale)                   # the diagonal included: M[K, K] + M[K, K]


@pytest.mark.parametrize("kind, nx, mask", [c for c in CASES if c[0] != "qg"])
def test_refraction_is_antisymmetric_on_any_state(cases, kind, nx, mask):
    check_antisymmetry(cases(kind, nx, mask)["R"], "ke_niw_ref", "%s %d %s broadband" % (kind, nx, mask))


@pytest.mark.parametrize("kind, nx", [(k, nx) for k in KINDS for nx in SIZES])
def test_advection_is_antisymmetric_without_aliasing(cases, kind, nx):
    R = cases(kind, nx, "none", "fresh")["R"]
    for name in [n for n in ("ens", "ke_niw_adv") if n in R.names]:
        check_antisymmetry(R, name, "%s %d fresh" % (kind, nx))


# ---- 4. bands and calls are bit-reproducible ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, nx", [("coupled", 64), ("uncoupled", 512), ("qg", 128), ("ybj", 1024), ("coupled", 1024)])
def test_bands_and_calls_are_bit_identical(cases, kind, nx):
    from niwqg_amd import shelltoshell
    c = cases(kind, nx, "none")
    m, R = c["m"], c["R"]
    again = shelltoshell.shell_to_shell(m, edges(nx))
    assert again.raw.tobytes() == R.raw.tobytes()
    # one band alone against the same band as the fifth of eight: nothing of the bands before it is left in the scratch
    one = shelltoshell.shell_to_shell(m, table=c["tab"][4])
    assert one.raw.shape[0] == 1 and one.raw[0].tobytes() == R.raw[4].tobytes()
    last = shelltoshell.shell_to_shell(m, edges(nx)[7:])
    assert last.raw[0].tobytes() == R.raw[7].tobytes() and last.edges.tolist() == edges(nx)[7:]
    assert last.k_edges.tolist() == [e * m.dk for e in edges(nx)[7:]]
    # one name alone: the same rows of the same kernels
    for name in R.names:
        sub = shelltoshell.shell_to_shell(m, edges(nx), names=name)
        assert sub.names == (name,) and sub.rows[name].tobytes() == R.rows[name].tobytes(), name
        row = shelltoshell.ROWS[name][0]
        assert sub.raw[:, row].tobytes() == R.raw[:, row].tobytes()
        others = set(range(4)) - ({0, 1} if row < 2 else {row})
        assert not sub.raw[:, sorted(others)].any(), name


# ---- 5. the run is left alone --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, mask", [("coupled", "filter"), ("coupled", "dealias"), ("uncoupled", "none"), ("ybj", "none"), ("qg", "none")])
def test_calls_leave_the_run_alone(kind, mask):
    """10 steps with a call after every step against 10 steps without: q-hat, psi-hat, phi-hat and the step's budget increments
    (Ke, Pw, Kw; the model's totals start from an atomically reduced value whose last bits differ between any two runs,
    tests/test_gpu_spectra.py: ATOMIC) are bit-identical, and the other diagnostics return what they returned before a call"""
    from niwqg_amd import coarse, shelltoshell
    from niwqg_amd.spectra import isotropic_spectra
    from niwqg_amd.transfer import spectral_transfer
    a, b = make(kind, 128, mask), make(kind, 128, mask)
    inc = {id(a): [], id(b): []}
    for _ in range(10):
        for m in (a, b):
            m._ctx.step(1)
            if m is a:
                shelltoshell.shell_to_shell(a, [0, 3, 40, 64])
            if kind in ("coupled", "uncoupled"):                     # QGModel and YBJModel keep no budgets
                inc[id(m)].append(m._ctx.take_budget_increments())
    a._after_steps()
    b._after_steps()
    for n in ("qh", "ph") + (("phih",) if kind != "qg" else ()):
        assert np.array(getattr(a, n)).tobytes() == np.array(getattr(b, n)).tobytes(), n
    assert np.array(inc[id(a)]).tobytes() == np.array(inc[id(b)]).tobytes()
    if kind in ("coupled", "uncoupled"):
        assert np.abs(np.array(inc[id(a)])).max() > 0

    def others():
        return dict(sp=isotropic_spectra(a).values, tr=spectral_transfer(a).transfer,
                    cg={n + k: getattr(coarse.flux_maps(a, [7], maps=False), k)[n] for n in coarse.available(a) for k in ("sums", "sumsq")},
                    q=dict(q=np.array(a.q), u=np.array(a.u)))
    before = others()
    shelltoshell.shell_to_shell(a, [0, 5, 64])
    after = others()
    for k in before:
        for n in before[k]:
            assert np.asarray(before[k][n]).tobytes() == np.asarray(after[k][n]).tobytes(), (k, n)


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_and_device_bytes():
    import niwqg_amd
    from niwqg_amd import shelltoshell, _lib
    from niwqg_amd.spectra import shell_count
    L = _lib.lib()
    nx = 64
    nb = shell_count(nx)
    out = np.zeros(4 * nb)

    def raw(h, mask, table, nb_arg=nb):
        t = np.ascontiguousarray(table, np.float64)
        return L.nq_shell_transfer(h, mask, 1, _lib._dptr(t), nb_arg, _lib._dptr(out))
    s = niwqg_amd.CoupledModel.Model(slab=2, **notebook_kwargs(nx, True))
    with pytest.raises(NotImplementedError, match="slab"):
        shelltoshell.shell_to_shell(s, [0, 4])
    ok = shelltoshell.bands(s, [0, 4])[0]
    hs = s._ctx.sim.ranks[0].h
    assert raw(hs, 1, ok) == -4 and len(L.nq_last_error(hs)) > 0
    a = make("coupled", 96)
    assert getattr(a, "_any_size", False)
    with pytest.raises(NotImplementedError, match="any-size"):
        shelltoshell.shell_to_shell(a, [0, 4])
    g, y = make("qg", nx), make("ybj", nx)
    with pytest.raises(ValueError, match="valid names: ke_qg, ens$"):
        shelltoshell.shell_to_shell(g, [0, 4], names=["ke_niw_adv"])
    assert raw(g._ctx.h, _lib.S2S_ADV, ok) == -1 and b"mask" in L.nq_last_error(g._ctx.h)
    assert raw(y._ctx.h, _lib.S2S_Q | _lib.S2S_ADV, ok) == -1
    assert raw(g._ctx.h, 0, ok) == -1 and raw(g._ctx.h, 8, ok) == -1
    k = make("coupled", nx)
    b0 = k._ctx.device_bytes()
    bad = ok.copy()
    bad[nx // 2] = 1e-300
    assert raw(k._ctx.h, 7, bad) == -1 and b"shell" in L.nq_last_error(k._ctx.h)
    bad = ok.copy()
    bad[2] = np.inf
    assert raw(k._ctx.h, 7, bad) == -1 and b"finite" in L.nq_last_error(k._ctx.h)
    assert raw(k._ctx.h, 7, ok, nb - 1) == -1 and b"shells" in L.nq_last_error(k._ctx.h)
    assert L.nq_shell_transfer(k._ctx.h, 7, 0, _lib._dptr(ok), nb, _lib._dptr(out)) == -1 and b"bands" in L.nq_last_error(k._ctx.h)
    assert L.nq_shell_transfer(k._ctx.h, 7, 65, _lib._dptr(np.zeros((65, nb))), nb, _lib._dptr(np.zeros(65 * 4 * nb))) == -1
    assert L.nq_shell_transfer(k._ctx.h, 7, 1, None, nb, _lib._dptr(out)) == -1
    assert k._ctx.device_bytes() == b0                     # every refusal came before the first allocation
    fresh = niwqg_amd.CoupledModel.Model(**notebook_kwargs(nx, True))
    with pytest.raises(RuntimeError, match="set_phi"):     # the tick's own precondition
        shelltoshell.shell_to_shell(fresh, [0, 4])
    # the planes of ONE band, allocated by the first call, counted and kept
    planes = (2 * nx * (nx // 2 + 1) + 4 * nx * nx) * 16
    shelltoshell.shell_to_shell(k, [0, 4])
    b1 = k._ctx.device_bytes()
    tables = 64 * nb * 8 * (1 + 4)
    assert planes + tables <= b1 - b0 <= 1.3 * planes + tables, (b1 - b0, planes, tables)
    shelltoshell.shell_to_shell(k, [0, 4, 9, 32])
    assert k._ctx.device_bytes() == b1
    k._ctx.close()
    assert make("coupled", nx)._ctx.device_bytes() == b0   # closed with the context: the next one starts where this one did


def test_refused_at_8192():
    """the row kernel of the 8192-point plan (128 registers per thread) spills: refused before any allocation"""
    import niwqg_amd
    from niwqg_amd import shelltoshell, _lib
    from niwqg_amd.spectra import shell_count
    nx = 8192
    m = niwqg_amd.CoupledModel.Model(**rough_kwargs(nx))
    b0 = m._ctx.device_bytes()
    with pytest.raises(NotImplementedError, match="8192"):
        shelltoshell.shell_to_shell(m, [0, 64])
    L = _lib.lib()
    g, out = shelltoshell.bands(m, [0, 64]), np.zeros(4 * shell_count(nx))
    assert L.nq_shell_transfer(m._ctx.h, 7, 1, _lib._dptr(g), shell_count(nx), _lib._dptr(out)) == -1
    assert b"section 7" in L.nq_last_error(m._ctx.h) and m._ctx.device_bytes() == b0
    m._ctx.close()
