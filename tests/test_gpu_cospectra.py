"""Isotropic co-spectra of the physical fields (niwqg_amd/cospectra.py, csrc/nq_cospec.hpp): the device
rows equal numpy's fft2 of the planes one ``averages`` sample returns for the same names, they close on the plane means, the tick's
sums and the enstrophy spectrum, they are symmetric in the order of the names, bit-reproducible, accumulate as sequential sums,
disturb nothing, agree on QGModel and on the any-size path, and the refusals are loud.

The bar for two routes to one number, per shell s of a row of the fields (a, b), A = fft2(a), B = fft2(b), M = nx ny, is the issue's

    |device - reference| <= 1e-12 sum_{shell s} |A||B| / M^2

and it is asserted as it stands on every RESOLVED shell, the outer partial shells included.  A transform's round-off is absolute
(about log2(M) 2^-53 / sqrt(M) of the plane's rms on every coefficient), not relative to the coefficient, so numpy's own reference
cannot hold 1e-12 of a shell whose wavenumbers carry less than 2e-5 of the plane's average energy: shell 0 of a mean-free field, the
shells the filter or three steps of hyperviscosity have emptied, the last shell of the (u, v) row (v has no Nyquist column, u no
Nyquist row: no wavenumber in common).  ``cospectra.transform_rounding`` is that bound, derived there; on a shell of average content
it is 4e-15 of the content and on the host test's broadband-plus-white fields at most 3 % of the issue's bar on every shell but
shell 0 of a mean-free field; two summation orders of numpy itself stay inside it and leave the issue's bar on the shells it is
there for (tests/test_cospectra_host.py).  A shell counts as resolved where that bound is below 5 % of the issue's bar; on the
others the bar is the issue's plus the same bound for the device's route (the packed plane a field shares with its partner has the
size of the peaks; the any-size path's chirp-z transforms have a larger growth factor).  How many shells of a row are not resolved is printed, and a state right after ``set_q`` /
``set_phi`` with the filter off may have only shell 0 and the last shell among them in the rows of q, q_psi, |phi|^2 (asserted).

Grids: 64 (eight rows per workgroup), 128 (four), 512 (one row, one wave), 1024 (two waves per row), 96 (the any-size path); 256,
2048, 4096, 8192, the two-pass tiles at 64 ... 512, another column split at 1024 and fields that vanish are in
tests/test_gpu_plan_ladder_analysis.py and the children of tests/test_gpu_plan_ladder.py, through ``check_lists``, ``check_rows`` and
``check_closure`` of this module.
States: tests/test_gpu_flow.py's ``make``: broadband q and phi plus a white part, so the Nyquist row and column and the outer
partial shells carry energy."""
import ctypes

import numpy as np
import pytest

from test_oracle_golden import notebook_kwargs, K0, U0
from test_gpu_flow import make, advance, device_values, KINDS, SIZES

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LISTS = (("q", "q_psi", "phi2"), ("q_psi", "ow", "gradphi2"), ("u", "v"), ("strain2",))


def transforms(planes):
    return {n: np.fft.fft2(p) for n, p in planes.items()}


def reference_rows(T, planes, a, b, nx, packed=True):
    """(reference row, bar, resolved) of the pair (a, b); a == b: the auto row.  bar: the issue's on the resolved shells (bool array),
    the issue's plus the round-off bound of the device's route on the others (packed=False: QGModel, whose q-hat and c-hat are
    not transformed at all)"""
    from niwqg_amd import cospectra, _lib
    M2 = float(nx) ** 4
    A, B = T[a], T[b]
    want = cospectra.bin_shells(A.real * B.real + A.imag * B.imag, nx) / M2
    bar = 1e-12 * cospectra.bin_shells(np.abs(A) * np.abs(B), nx) / M2
    # (the any-size path transforms by Bluestein's identity: three times the operations per axis, on twice the length)
    growth = None if _lib.has_fused_plan(nx) else cospectra.bluestein_growth(nx)
    resolved = cospectra.transform_rounding(A, B, planes[a], planes[b], nx, growth) <= 0.05 * bar
    # on the others the device's own route counts: a Kernel-family field shares its transform with its partner on the fused grids
    rounding = cospectra.transform_rounding(A, B, planes[a], planes[b], nx, growth, packed=packed and growth is None)
    return want, np.where(resolved, bar, bar + rounding), resolved


def check_rows(cs, T, planes, nx, tag, only_ends=False, packed=True):
    """only_ends: every shell but shell 0 and the last must be resolved (a broadband state nothing has damped yet)"""
    worst, worst_other, n_other = 0.0, 0.0, 0
    names = cs.names
    for i, a in enumerate(names):
        for b in names[i:]:
            got = cs.auto[a] if a == b else cs.co[(a, b)]
            want, bar, resolved = reference_rows(T, planes, a, b, nx, packed)
            ratio = np.abs(got - want) / bar
            worst = max(worst, float(ratio[resolved].max()) if resolved.any() else 0.0)      # (a constant field has no resolved co row)
            if not resolved.all():
                worst_other, n_other = max(worst_other, float(ratio[~resolved].max())), n_other + int((~resolved).sum())
            assert (ratio <= 1.0).all(), (tag, a, b, int(ratio.argmax()), float(ratio.max()), bool(resolved[ratio.argmax()]))
            assert not only_ends or resolved[1:-1].all(), (tag, a, b, np.flatnonzero(~resolved))
    print("%s %s: resolved shells, worst |device - reference| / (1e-12 sum_shell |A||B| / M^2) = %.3g; %d shells not resolved, worst %.3g "
          "of their bar" % (tag, "/".join(names), worst, n_other, worst_other))


def check_lists(m, nx, tag, lists=LISTS, only_ends=False):
    from niwqg_amd import cospectra
    union = sorted({n for names in lists for n in names})
    planes = device_values(m, union)                   # the specification of the values: one averages sample per name
    T = transforms(planes)
    for names in lists:
        cs = cospectra.cross_spectra(m, names)
        assert cs.names == tuple(names) and cs.n == 1 and len(cs.shell) == len(cs.auto[names[0]])
        check_rows(cs, T, planes, nx, tag, only_ends and names == LISTS[0])      # (u, v, the strain and the gradients fall off with k)
    return planes, T


# ---- 1. values -----------------------------------------------------------------------------------------------------------------------
VALUE_CASES = [(k, nx, "none") for k in KINDS for nx in SIZES] + [("coupled", nx, "filter") for nx in SIZES]


@pytest.mark.parametrize("kind, nx, mask", VALUE_CASES)
def test_rows_equal_the_reference(kind, nx, mask):
    from niwqg_amd import cospectra, flow
    m = make(kind, nx, mask)
    assert cospectra.available(m) == ["q", "q_psi", "phi2"] + list(flow.NAMES)
    check_lists(m, nx, "%s %d %s set" % (kind, nx, mask), only_ends=mask == "none")
    advance(m, 3, batched=True)                       # the rows are now the step's own inversion's
    check_lists(m, nx, "%s %d %s 3 steps" % (kind, nx, mask))


# ---- 2. closure ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, nx, mask", [("coupled", 64, "none"), ("uncoupled", 128, "none"), ("ybj", 512, "none"),
                                            ("coupled", 1024, "filter")])
def test_closure(kind, nx, mask):
    m = make(kind, nx, mask)
    advance(m, 2, batched=True)
    check_closure(m, kind, nx)


CLOSURE_LISTS = (("q_psi", "phi2", "ow"), ("strain2", "gradphi2"))


def check_closure(m, kind, nx, lists=CLOSURE_LISTS, host_transform=True):
    """host_transform=False (the largest grids): the bar of the last part from the shell sums of its partner, 2 x the enstrophy
    spectrum, and the downloaded q plane, instead of from numpy's transform of that plane.  That bar comes from a device output:
    it bounds two device routes to one number against each other (k_bin_shells on q-hat runs no row transform), not a route
    against numpy, and is for the sizes where a host transform is ruled out"""
    from niwqg_amd import averages, cospectra, spectra
    M = float(nx) * nx
    # the shells sum to the plane mean of the product: an averages product plane of one sample
    for names in lists:
        pairs = [(a, b) for i, a in enumerate(names) for b in names[i:]]
        A = averages.attach(m, names, pairs, every=0)
        A.sample()
        R = A.result()
        A.detach()
        cs = cospectra.cross_spectra(m, names)
        for a, b in pairs:
            co = cs.auto[a] if a == b else cs.co[(a, b)]
            want = R.sums["%s*%s" % (a, b)].mean()
            scale = np.sqrt((R.sums[a] ** 2).mean() * (R.sums[b] ** 2).mean())
            print("%s %d %s*%s: sum of the shells - plane mean = %.3g of the scale" % (kind, nx, a, b, abs(co.sum() - want) / scale))
            assert abs(co.sum() - want) <= 1e-12 * scale, (a, b, co.sum(), want)
            assert abs(co[0] - R.sums[a].mean() * R.sums[b].mean()) <= 1e-12 * scale, (a, b)
            assert abs(cs.covariance(a, b) - (want - R.sums[a].mean() * R.sums[b].mean())) <= 2e-12 * scale, (a, b)
    # the tick's raw sum [21] = sum ups q_psi, ups = |phi|^2 - its mean: M^2 sum_{s >= 1} co = M [21], at 1e-12 of sqrt([19] [20])
    cs = cospectra.cross_spectra(m, ("q_psi", "phi2"))
    s = m._ctx.diagnostic_sums()
    got = M * M * cs.co[("q_psi", "phi2")][1:].sum()
    print("%s %d tick [21]: %.3g of sqrt([19] [20])" % (kind, nx, abs(got - M * s[21]) / (M * np.sqrt(s[19] * s[20]))))
    assert abs(got - M * s[21]) <= 1e-12 * M * np.sqrt(s[19] * s[20])
    assert abs(M * M * cs.covariance("q_psi", "phi2") - M * s[21]) <= 1e-12 * M * np.sqrt(s[19] * s[20])
    # auto["q"] = 2 x the enstrophy spectrum, which comes from q-hat itself: per shell on the scale of the shell's own sum |A|^2
    cq = cospectra.cross_spectra(m, ("q",))
    ens = spectra.isotropic_spectra(m, ["ens"]).values["ens"]
    planes = device_values(m, ["q"])
    if host_transform:
        want, bar, resolved = reference_rows(transforms(planes), planes, "q", "q", nx)
    else:                                                 # reference_rows with sum_shell |A|^2 / M^2 = 2 ens in the place of numpy's
        S, q = 2.0 * ens, planes["q"]
        resolved = cospectra.shell_sum_rounding(S, S, q, q, nx) <= 0.05 * 1e-12 * S
        bar = np.where(resolved, 1e-12 * S, 1e-12 * S + cospectra.shell_sum_rounding(S, S, q, q, nx, packed=True))
    ratio = np.abs(cq.auto["q"] - 2.0 * ens) / bar
    print("%s %d auto[q] - 2 ens: worst %.3g of 1e-12 sum_shell |A|^2 / M^2 (%d shells not resolved: %.3g of their bar)"
          % (kind, nx, ratio[resolved].max(), (~resolved).sum(), ratio[~resolved].max() if not resolved.all() else 0.0))
    assert (ratio <= 1.0).all(), (int(ratio.argmax()), float(ratio.max()))


# ---- 3. symmetries -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, nx", [("coupled", 64), ("uncoupled", 128), ("coupled", 512), ("ybj", 1024)])
def test_symmetries(kind, nx):
    from niwqg_amd import cospectra
    m = make(kind, nx)
    advance(m, 2, batched=True)
    for names in (("q_psi", "phi2", "ow"), ("q", "phi2", "q_psi")):
        planes = device_values(m, names)
        T = transforms(planes)
        a, b, c = names
        one = cospectra.cross_spectra(m, names)
        again = cospectra.cross_spectra(m, names)
        assert np.array_equal(one.raw, again.raw)                    # two identical calls
        other = cospectra.cross_spectra(m, (c, a, b))                # another order: other partners in the packed transform
        single = cospectra.cross_spectra(m, (b,))
        for x, y in ((a, a), (b, b), (c, c), (a, b), (a, c), (b, c)):
            bar = reference_rows(T, planes, x, y, nx)[1]
            r1 = one.auto[x] if x == y else one.co[(x, y)]
            r2 = other.auto[x] if x == y else other.co[(y, x)]
            assert (np.abs(r1 - r2) <= bar).all(), (names, x, y)
        assert (np.abs(single.auto[b] - one.auto[b]) <= reference_rows(T, planes, b, b, nx)[1]).all()
        assert np.array_equal(single.raw[1:], np.zeros_like(single.raw[1:]))
        for x, y in ((a, b), (a, c), (b, c)):
            coh = one.coherence(x, y)
            ok = (one.auto[x] > 0) & (one.auto[y] > 0)
            assert ok.sum() >= len(ok) - 1 and not np.isnan(coh[ok]).any() and np.isnan(coh[~ok]).all()
            print("%s %d coherence(%s, %s): max |.| = %.15g" % (kind, nx, x, y, np.abs(coh[ok]).max()))
            assert (np.abs(coh[ok]) <= 1.0 + 1e-12).all(), (x, y, float(np.abs(coh[ok]).max()))
            assert abs(one.correlation(x, y)) <= 1.0 + 1e-12


# ---- 4. accumulator ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, nx, names", [("coupled", 128, ("q_psi", "phi2", "ow")), ("ybj", 64, ("q", "phi2")), ("qg", 64, ("q",))])
def test_accumulator(kind, nx, names):
    from niwqg_amd import cospectra, spectra
    a, b = make(kind, nx), make(kind, nx)                 # two identical runs: one accumulates, one is read state by state
    before = a._ctx.device_bytes()
    nb = spectra.shell_count(nx)
    own = 2 * 6 * nb * 8 + (0 if kind == "qg" else (6 * 8192 + 6) * 8)     # the tables; Kernel family: the range partials, the scales
    A = cospectra.Accumulator(a, names)
    total = None
    for i in range(3):
        x0 = a._ctx.device_bytes()
        A.add()
        assert a._ctx.device_bytes() - x0 == (own if i == 0 else 0)         # allocated by the first call, once
        r = cospectra.cross_spectra(b, names).raw
        total = r if total is None else total + r         # the sequential host sum
        advance(a, 2, batched=True)
        advance(b, 2, batched=True)
    R = A.result()
    assert R.n == 3 and R.names == tuple(names)
    assert np.array_equal(R.raw, total)
    M2 = float(nx) ** 4
    assert np.array_equal(R.auto[names[0]], total[0] * (1.0 / (3 * M2)))
    assert len(R.shell) == nb
    x1 = a._ctx.device_bytes()
    A.reset()
    assert A.n == 0
    with pytest.raises(RuntimeError, match="nothing added"):
        A.result()
    A.add()                                               # starts from zero again
    R1 = A.result()
    assert R1.n == 1 and np.array_equal(R1.raw, cospectra.cross_spectra(b, names).raw)
    assert a._ctx.device_bytes() == x1
    # a cross_spectra call on the same model takes the tables over
    A.add()
    cospectra.cross_spectra(a, names)
    with pytest.raises(RuntimeError, match="another call"):
        A.add()
    # a context counts its own bytes, so this says only that a fresh context starts where this one started (the tables are in
    # the list nq_destroy frees, as every allocation of alloc_all_or_none is); the first-add delta above is the test of the count
    a._ctx.close()
    b._ctx.close()
    assert make(kind, nx)._ctx.device_bytes() == before


# ---- 5. nothing is disturbed -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, nx", [("coupled", 128), ("uncoupled", 64)])
def test_calls_leave_the_run_alone(kind, nx):
    from niwqg_amd import cospectra, pdfs, transfer, _lib
    a, b = make(kind, nx, "filter"), make(kind, nx, "filter")
    for m in (a, b):
        m._ctx.take_budget_increments()
    for _ in range(4):
        a._ctx.step(1)
        b._ctx.step(1)
        cospectra.cross_spectra(a, ("q_psi", "ow", "gradphi2"))
        cospectra.cross_spectra(a, ("q", "phi2"))
    for fid in (_lib.F_QH, _lib.F_PHIH, _lib.F_PH) + ((_lib.F_QWH,) if kind == "coupled" else ()):
        assert a._ctx.field(fid).tobytes() == b._ctx.field(fid).tobytes(), fid
    assert a._ctx.take_budget_increments() == b._ctx.take_budget_increments()
    for m in (a, b):
        m._after_steps()
    # spectral_transfer and field_pdfs right after a call return what they return without it
    cospectra.cross_spectra(a, ("q_psi", "ow", "gradphi2"))
    ta, tb = transfer.spectral_transfer(a), transfer.spectral_transfer(b)
    for n in ta.transfer:
        assert np.array_equal(ta.transfer[n], tb.transfer[n]), n
    cospectra.cross_spectra(a, ("q_psi", "phi2", "u"))
    kw = dict(names=("q_psi", "phi2", "ow"), bins=64, joint=("q_psi", "phi2"), joint_bins=32)
    pa, pb = pdfs.field_pdfs(a, **kw), pdfs.field_pdfs(b, **kw)
    for n in kw["names"]:
        assert np.array_equal(pa.counts[n], pb.counts[n]) and np.array_equal(pa.edges[n], pb.edges[n]), n
    assert np.array_equal(pa.joint.counts, pb.joint.counts)
    a._ctx.step(2)
    b._ctx.step(2)
    assert a._ctx.field(_lib.F_QH).tobytes() == b._ctx.field(_lib.F_QH).tobytes()
    assert a._ctx.field(_lib.F_PHIH).tobytes() == b._ctx.field(_lib.F_PHIH).tobytes()


# ---- 6. QGModel ----------------------------------------------------------------------------------------------------------------------
def make_qg(nx, passive, seed=0):
    import niwqg_amd
    kw = notebook_kwargs(nx, False)
    for k in ("m", "N", "f", "nu4w", "nuw", "muw"):
        kw.pop(k)
    kw.update(mu=2e-8, nu=0.0, passive_scalar=passive)
    m = niwqg_amd.QGModel.Model(**kw)
    rng = np.random.default_rng(seed + nx)
    n = np.append(np.arange(0, nx // 2), np.arange(-(nx // 2), 0))
    kap = np.sqrt(n[None, :] ** 2.0 + n[:, None] ** 2.0)

    def noise():
        z = np.fft.ifft2(np.fft.fft2(rng.standard_normal((nx, nx))) * (np.exp(-(kap / 8.0) ** 2) + 0.05)).real
        return z - z.mean()
    q = noise()
    m.set_q(U0 * K0 * q / q.std())
    if passive:
        c = noise()
        m.set_c(2.0 + c / c.std())
    return m


@pytest.mark.parametrize("nx", [64, 256, 96])
@pytest.mark.parametrize("passive", [False, True])
def test_qgmodel(nx, passive):
    from niwqg_amd import cospectra
    m = make_qg(nx, passive)
    assert bool(getattr(m, "_any_size", False)) == (nx == 96)
    names = ("q", "c") if passive else ("q",)
    for stage in ("set", "3 steps"):
        planes = {n: np.array(getattr(m, n), np.float64) for n in names}
        T = transforms(planes)
        for lst in (names, names[::-1]):
            check_rows(cospectra.cross_spectra(m, lst), T, planes, nx, "qg %d %s" % (nx, stage), packed=False)
        advance(m, 3, batched=True)
    with pytest.raises(ValueError, match="valid names"):
        cospectra.cross_spectra(m, ("q", "phi2"))
    if nx == 96:                                          # the any-size path offers QGModel's flow names: the half-plane route on them
        from niwqg_amd import flow
        assert cospectra.available(m) == list(names) + [n for n in flow.NAMES if n != "gradphi2"]
        check_lists(m, nx, "qg 96 flow names", (("q", "u", "ow"), ("strain2", "v")))
    if nx != 96:                                          # the fused grids have no flow fields on QGModel
        with pytest.raises(ValueError, match="valid names: q"):
            cospectra.cross_spectra(m, ("q", "u"))
    if not passive:
        with pytest.raises(ValueError, match="valid names: q"):
            cospectra.cross_spectra(m, ("q", "c"))


# ---- 7. any-size ---------------------------------------------------------------------------------------------------------------------
def test_any_size_coupled():
    from niwqg_amd import cospectra
    nx = 96
    m = make("coupled", nx, "filter")
    assert getattr(m, "_any_size", False)
    advance(m, 2)
    check_lists(m, nx, "coupled 96")
    A = cospectra.Accumulator(m, ("q_psi", "phi2"))
    A.add()
    first = cospectra.cross_spectra(m, ("q_psi", "phi2")).raw
    advance(m, 1)
    A.add()
    R = A.result()
    assert R.n == 2 and np.array_equal(R.raw, first + cospectra.cross_spectra(m, ("q_psi", "phi2")).raw)


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals():
    import niwqg_amd
    from niwqg_amd import cospectra, _lib
    L = _lib.lib()
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    cnt = ctypes.c_longlong()

    def refused(state, call, rc, text=None, h=None):
        """the call returns rc (or raises) and leaves `state()` as it was"""
        before = state()
        if isinstance(rc, type):
            with pytest.raises(rc, match=text):
                call()
        else:
            assert call() == rc
            assert text is None or text in L.nq_last_error(h), L.nq_last_error(h)
        assert state() == before

    m = make("coupled", 64)
    advance(m, 1, batched=True)
    h = m._ctx.h
    nb = len(cospectra.cross_spectra(m, ("q", "phi2")).shell)
    out = np.zeros((6, nb))
    state = lambda: (m._ctx.field(_lib.F_QH).tobytes(), m._ctx.field(_lib.F_PHIH).tobytes(), m._ctx.field(_lib.F_QWH).tobytes(),
                     m._ctx.cospectra_read()[0], m._ctx.cospectra_read()[1].tobytes())
    s0 = state()
    for bad in (("q", "zeta"), ("q", "q_psi", "phi2", "ow"), ("q", "ow", "q"), ("c",), ()):
        refused(state, lambda: cospectra.cross_spectra(m, bad), ValueError)
        refused(state, lambda: cospectra.Accumulator(m, bad), ValueError)
    refused(state, lambda: L.nq_cospectra(h, 2, ints(_lib.PDF_Q, _lib.PDF_PHI2), nb + 1, 0, _lib._dptr(out)), -1, b"shells", h)
    refused(state, lambda: L.nq_cospectra(h, 2, ints(_lib.PDF_Q, _lib.FLOW_OW), nb, 1, None), -1, b"accumulate", h)
    refused(state, lambda: L.nq_cospectra(h, 2, None, nb, 0, None), -1)
    refused(state, lambda: L.nq_cospectra(h, 4, ints(0, 1, 2, 16), nb, 0, None), -1)
    refused(state, lambda: L.nq_cospectra(h, 2, ints(_lib.PDF_Q, _lib.PDF_Q), nb, 0, None), -1, b"twice", h)
    refused(state, lambda: L.nq_cospectra(h, 1, ints(_lib.PDF_C), nb, 0, None), -1)
    refused(state, lambda: L.nq_cospectra(h, 1, ints(23), nb, 0, None), -1)
    refused(state, lambda: L.nq_cospectra_read(h, None, _lib._dptr(out)), -1)
    assert state() == s0
    assert L.nq_cospectra(h, 2, ints(_lib.PDF_Q, _lib.PDF_PHI2), nb, 1, None) == 0        # the same list: adds
    n, sums = m._ctx.cospectra_read()
    assert n == 2 and np.array_equal(sums, 2.0 * np.frombuffer(s0[4]).reshape(6, nb))
    # a context that has not been asked yet: nothing to read, nothing to add to
    fresh = make("coupled", 64)
    fstate = lambda: (fresh._ctx.field(_lib.F_QH).tobytes(), fresh._ctx.field(_lib.F_PHIH).tobytes(), fresh._ctx.device_bytes())
    refused(fstate, lambda: L.nq_cospectra_read(fresh._ctx.h, ctypes.byref(cnt), _lib._dptr(out)), -1, b"no nq_cospectra call", fresh._ctx.h)
    refused(fstate, lambda: L.nq_cospectra(fresh._ctx.h, 1, ints(_lib.PDF_Q), nb, 1, None), -1, b"accumulate", fresh._ctx.h)
    # QGModel on a fused grid: no flow fields, and no c without its passive scalar
    g = make("qg", 64)
    gstate = lambda: (g._ctx.field(_lib.F_QH).tobytes(), g._ctx.field(_lib.F_PH).tobytes(), g._ctx.device_bytes())
    refused(gstate, lambda: L.nq_cospectra(g._ctx.h, 1, ints(_lib.FLOW_U), nb, 0, None), -1, b"QGModel", g._ctx.h)
    refused(gstate, lambda: L.nq_cospectra(g._ctx.h, 1, ints(_lib.PDF_C), nb, 0, None), -1)
    refused(gstate, lambda: cospectra.cross_spectra(g, ("q", "u")), ValueError, "valid names: q")
    # a slab context: -4 from the library, NotImplementedError from the module
    s = niwqg_amd.CoupledModel.Model(slab=2, **notebook_kwargs(64, True))
    s.set_q(np.array(m.q))
    s.set_phi(np.array(m.phi))
    hs = s._ctx.sim.ranks[0].h
    sstate = lambda: (np.array(s.qh).tobytes(), np.array(s.phih).tobytes())
    refused(sstate, lambda: cospectra.cross_spectra(s, ("q", "phi2")), NotImplementedError, "slab")
    refused(sstate, lambda: cospectra.Accumulator(s, ("q",)), NotImplementedError, "slab")
    refused(sstate, lambda: L.nq_cospectra(hs, 1, ints(_lib.PDF_Q), nb, 0, None), -4)
    assert len(L.nq_last_error(hs)) > 0
    refused(sstate, lambda: L.nq_cospectra_read(hs, ctypes.byref(cnt), _lib._dptr(out)), -4)
