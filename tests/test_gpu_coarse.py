"""Coarse-grained energy and enstrophy flux maps (niwqg_amd/coarse.py, csrc/nq_coarse.hpp): for the sharp
filter the plane mean of a device map closes on the spectral flux the device bins by another path (``spectral_transfer``), the
maps equal the numpy restatement ``coarse.reference``, the moments agree with the downloaded maps, scales and calls are
bit-reproducible, nothing disturbs the run, and the models and grids without the maps refuse.

Grids: 64 (eight rows per workgroup), 128 (four), 512 (one row, one wave), 1024 (two waves per row): the smallest shapes at which
the row plan changes; 2048 and 4096 once, identity only here; values at 256 and 2048, moments at 4096,
the two-pass tiles at 64 ... 512 and another column split at 1024 in tests/test_gpu_plan_ladder_analysis.py and the children of
tests/test_gpu_plan_ladder.py, through ``check_maps``, ``check_mean_closes`` and ``check_moments`` of this module.  States: those of test_gpu_flow.make, white part included (the Nyquist
lines carry energy), set and then advanced 3 steps, so quirks Q1 (UnCoupledModel's and YBJModel's stale gradients) and Q2 are live.

Bounds.  Identity: |mean - flux[B]| <= 1e-12 (mean |map| + sum_b |T_b|), the project's standing 1e-12 of two device routes to
one number.  Values: 1e-12 of the product of the factors' maxima (tau is a difference that cancels, so a map's own maximum is
not its rounding scale).  Mean of a map against numpy's: 1e-12 sum |map| / M; variance: 1e-12 sum map^2 / M, the same bound on
the second moment it is formed from."""
import time

import numpy as np
import pytest

from test_oracle_golden import notebook_kwargs
from test_gpu_at_size import rough_kwargs
import test_gpu_flow
from test_gpu_flow import make, advance

pytestmark = pytest.mark.gpu

# one more mask for test_gpu_flow.make: the 2/3 rule, which makes the context keep both copies of q-hat (dual_q)
test_gpu_flow.MASKS.setdefault("dealias", dict(use_filter=False, dealias=True))

SIZES = (64, 128, 512, 1024)
KINDS = ("coupled", "uncoupled", "ybj", "qg")
CASES = [(k, nx, "none") for k in KINDS for nx in SIZES] + [("coupled", nx, "filter") for nx in SIZES] + [("coupled", 128, "dealias")]


def cuts(nx, name):
    """the sharp cuts at which the identity is exact: every shell for ke_qg, 3 B < nx for the maps with a resolved triple product"""
    return sorted({1, 2, nx // 8, (nx - 1) // 3} | ({nx // 2 - 1} if name == "ke_qg" else set()))


def length(m):
    return 2 * np.pi / (8 * m.dk)                         # a Gaussian that passes the first few shells


@pytest.fixture(scope="module")
def cases():
    """(kind, nx, mask) -> the model after 3 steps, the tables [sharp cuts..., one Gaussian], the device result and the reference,
    formed once and only read afterwards"""
    cache = {}

    def get(kind, nx, mask):
        from niwqg_amd import coarse
        key = (kind, nx, mask)
        if key not in cache:
            m = make(kind, nx, mask)
            advance(m, 3, batched=True)
            shells = sorted({B for n in coarse.available(m) for B in cuts(nx, n)})
            tab = np.array([coarse.sharp(m, B) for B in shells] + [coarse.gaussian(m, length(m))])
            R = coarse.flux_maps(m, table=tab)
            cache[key] = dict(m=m, shells=shells, tab=tab, R=R, ref=coarse.reference(m, tab, coarse.available(m)))
        return cache[key]
    yield get
    for c in cache.values():
        c["m"]._ctx.close()


# ---- 1. the plane mean closes on the spectral flux -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind, nx, mask", CASES)
def test_mean_closes_on_the_spectral_flux(cases, kind, nx, mask):
    c = cases(kind, nx, mask)
    check_mean_closes(c["m"], c["R"], c["shells"], "%s %d %s" % (kind, nx, mask))


def check_mean_closes(m, R, shells, tag, cut_list=None):
    """R: flux_maps on the tables [sharp(B) for B in shells] + ...; the plane mean of every sharp map on the cuts of the name
    (cut_list: on these shells instead) against the spectral flux"""
    from niwqg_amd import coarse
    from niwqg_amd.transfer import spectral_transfer
    nx = m.nx
    assert list(R.names) == coarse.available(m)
    st = spectral_transfer(m)
    for name in R.names:
        T = st.transfer[name]
        for B in (cuts(nx, name) if cut_list is None else cut_list):
            i = shells.index(B)
            err, scale = abs(R.mean[name][i] - st.flux[name][B]), np.abs(R.maps[name][i]).mean() + np.abs(T).sum()
            print("%s %s B = %d: %.3g" % (tag, name, B, err / scale))
            assert scale > 0 and err <= 1e-12 * scale, (name, B, err, scale)


# ---- 2. the maps equal the reference -------------------------------------------------------------------------------------------
def factor_maxima(m, g):
    """max |u-bar, v-bar|, |q-bar|, |grad q-bar|, |phi-bar|, |grad phi-bar| of one table, from the public reads"""
    from niwqg_amd.spectra import shell_of
    nx = m.nx
    n = np.append(np.arange(0, nx // 2), np.arange(-(nx // 2), 0))
    G = g[shell_of(n[None, :], n[:, None])]
    k = np.fft.fftfreq(nx, 1.0 / nx) * m.dk
    ik, il = 1j * k[None, :], 1j * k[:, None]
    Fi = np.fft.ifft2
    ph = np.asarray(m.ph)
    P = np.fft.fft2(Fi(ph).real if ph.shape[1] == nx else np.fft.irfft2(ph, s=(nx, nx)))
    out = dict(uv=max(np.abs(Fi(-il * G * P).real).max(), np.abs(Fi(ik * G * P).real).max()))
    if getattr(m, "model_id", None) != 3:
        Q = np.fft.fft2(np.array(m.q))
        out.update(q=np.abs(Fi(G * Q).real).max(), gq=max(np.abs(Fi(ik * G * Q).real).max(), np.abs(Fi(il * G * Q).real).max()))
    if hasattr(m, "phih"):
        W = np.asarray(m.phih)
        out.update(w=np.abs(Fi(G * W)).max(), gw=max(np.abs(Fi(ik * G * W)).max(), np.abs(Fi(il * G * W)).max()))
    return out


def value_scale(name, f):
    return {"ke_qg": lambda: f["uv"] ** 2 * f["q"], "ens": lambda: f["uv"] * f["q"] * f["gq"],
            "ke_niw_adv": lambda: f["w"] * f["uv"] * f["gw"]}[name]()


@pytest.mark.parametrize("kind, nx, mask", CASES)
def test_maps_equal_the_reference(cases, kind, nx, mask):
    c = cases(kind, nx, mask)
    m, R = c["m"], c["R"]
    assert bool(m._ctx.dual_q) == (mask == "dealias")
    check_maps(m, R, c["tab"], c["ref"], "%s %d %s" % (kind, nx, mask))


def check_maps(m, R, tab, ref, tag):
    for i, g in enumerate(tab):
        f = factor_maxima(m, g)
        for name in R.names:
            err, scale = np.abs(R.maps[name][i] - ref[name][i]).max(), value_scale(name, f)
            print("%s %s table %d: max |device - reference| / scale = %.3g" % (tag, name, i, err / scale))
            assert scale > 0 and err <= 1e-12 * scale, (name, i, err, scale)


# ---- 3. the moments agree with the maps ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, nx, mask", [("coupled", nx, "none") for nx in SIZES] + [("qg", 64, "none"), ("ybj", 128, "none")])
def test_moments_agree_with_the_maps(cases, kind, nx, mask):
    from niwqg_amd import coarse
    c = cases(kind, nx, mask)
    m, R = c["m"], c["R"]
    check_moments(R, nx, len(c["tab"]))
    S = coarse.flux_maps(m, table=c["tab"], maps=False)
    assert S.maps is None
    for name in R.names:
        assert S.sums[name].tobytes() == R.sums[name].tobytes() and S.sumsq[name].tobytes() == R.sumsq[name].tobytes(), name


def check_moments(R, nx, ntab):
    """mean and variance of every map against numpy's on the downloaded map"""
    M = float(nx) * nx
    for name in R.names:
        for i in range(ntab):
            x = R.maps[name][i]
            a1, a2 = np.abs(x).sum() / M, (x * x).sum() / M
            assert abs(R.mean[name][i] - x.mean()) <= 1e-12 * a1, (name, i)
            assert abs(R.variance[name][i] - x.var()) <= 1e-12 * a2, (name, i)
            assert R.variance[name][i] > 0


# ---- 4. scales and calls -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, nx", [("coupled", 64), ("uncoupled", 512), ("qg", 128), ("ybj", 1024)])
def test_scales_and_calls_are_bit_identical(cases, kind, nx):
    from niwqg_amd import coarse
    c = cases(kind, nx, "none")
    m, R = c["m"], c["R"]
    again = coarse.flux_maps(m, table=c["tab"])
    for name in R.names:
        assert again.maps[name].tobytes() == R.maps[name].tobytes() and again.sums[name].tobytes() == R.sums[name].tobytes(), name
    for i in (0, len(c["tab"]) - 1):
        one = coarse.flux_maps(m, table=c["tab"][i])
        for name in R.names:
            assert one.maps[name][0].tobytes() == R.maps[name][i].tobytes(), (name, i)
            assert one.sums[name][0] == R.sums[name][i] and one.sumsq[name][0] == R.sumsq[name][i], (name, i)
    # a subset of the names is the same planes of the same kernel
    sub = coarse.flux_maps(m, table=c["tab"][:2], names=R.names[-1])
    assert sub.maps[R.names[-1]].tobytes() == R.maps[R.names[-1]][:2].tobytes()
    # the builders through the public arguments
    B = c["shells"][2]
    s = coarse.flux_maps(m, [B], maps=False)
    assert s.shell.tolist() == [B] and s.k_cut[0] == (B + 0.5) * m.dk and s.sums[R.names[0]][0] == R.sums[R.names[0]][2]
    g = coarse.flux_maps(m, [length(m)], kind="gaussian", maps=False)
    assert g.shell is None and g.ell[0] == length(m) and g.sums[R.names[0]][0] == R.sums[R.names[0]][-1]


# ---- 5. the run is left alone --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, mask", [("coupled", "filter"), ("coupled", "dealias"), ("uncoupled", "none"), ("ybj", "none"), ("qg", "none")])
def test_calls_leave_the_run_alone(kind, mask):
    from niwqg_amd import coarse, timespectra
    from niwqg_amd.spectra import isotropic_spectra
    from niwqg_amd.transfer import spectral_transfer
    a, b = make(kind, 128, mask), make(kind, 128, mask)
    A, Bt = timespectra.attach(a, every=1), timespectra.attach(b, every=1)
    for _ in range(6):
        advance(a, 1)
        advance(b, 1)
        coarse.flux_maps(a, [3, 40], maps=False)
    coarse.flux_maps(a, [5.0], kind="gaussian")
    for n in ("qh", "ph") + (("phih",) if kind != "qg" else ()):
        assert np.array(getattr(a, n)).tobytes() == np.array(getattr(b, n)).tobytes(), n
    ra, rb = A.result(), Bt.result()
    assert ra.n == rb.n == 6
    for k in ra.sums:
        assert ra.sums[k].tobytes() == rb.sums[k].tobytes(), k
    before = dict(sp=isotropic_spectra(a).values, tr=spectral_transfer(a).transfer, q=np.array(a.q), u=np.array(a.u))
    coarse.flux_maps(a, [7])
    after = dict(sp=isotropic_spectra(a).values, tr=spectral_transfer(a).transfer, q=np.array(a.q), u=np.array(a.u))
    for k in ("sp", "tr"):
        for n in before[k]:
            assert before[k][n].tobytes() == after[k][n].tobytes(), (k, n)
    assert before["q"].tobytes() == after["q"].tobytes() and before["u"].tobytes() == after["u"].tobytes()
    A.detach()
    Bt.detach()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_and_device_bytes():
    import niwqg_amd
    from niwqg_amd import coarse, _lib
    from niwqg_amd.spectra import shell_count
    L = _lib.lib()
    nx = 64
    nb = shell_count(nx)
    mom = np.zeros(6)

    def raw(h, mask, table, nb_arg=nb):
        t = np.ascontiguousarray(table, np.float64)
        return L.nq_coarse_flux(h, mask, 1, _lib._dptr(t), nb_arg, _lib._dptr(mom), None)
    s = niwqg_amd.CoupledModel.Model(slab=2, **notebook_kwargs(nx, True))
    with pytest.raises(NotImplementedError, match="slab"):
        coarse.flux_maps(s, [4])
    hs = s._ctx.sim.ranks[0].h
    assert raw(hs, 1, coarse.sharp(s, 4)) == -4 and len(L.nq_last_error(hs)) > 0
    a = make("coupled", 96)
    assert getattr(a, "_any_size", False)
    with pytest.raises(NotImplementedError, match="any-size"):
        coarse.flux_maps(a, [4])
    g, y = make("qg", nx), make("ybj", nx)
    with pytest.raises(ValueError, match="valid names: ke_qg, ens$"):
        coarse.flux_maps(g, [4], names=["ke_niw_adv"])
    ok = coarse.sharp(g, 4)
    assert raw(g._ctx.h, _lib.CG_NIW, ok) == -1 and b"mask" in L.nq_last_error(g._ctx.h)
    assert raw(y._ctx.h, _lib.CG_KE | _lib.CG_NIW, ok) == -1
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
    assert L.nq_coarse_flux(k._ctx.h, 7, 0, _lib._dptr(ok), nb, _lib._dptr(mom), None) == -1
    assert L.nq_coarse_flux(k._ctx.h, 7, 65, _lib._dptr(np.zeros((65, nb))), nb, _lib._dptr(mom), None) == -1
    assert k._ctx.device_bytes() == b0                     # every refusal came before the first allocation
    fresh = niwqg_amd.CoupledModel.Model(**notebook_kwargs(nx, True))
    with pytest.raises(RuntimeError, match="set_phi"):     # the tick's own precondition
        coarse.flux_maps(fresh, [4])
    # the scratch of the first call, counted and kept; the map planes come with the first call that asks for maps
    planes = (12 * nx * (nx // 2 + 1) + 6 * nx * nx) * 16
    coarse.flux_maps(k, [4], maps=False)
    b1 = k._ctx.device_bytes()
    assert planes <= b1 - b0 <= 1.3 * planes, (b1 - b0, planes)
    coarse.flux_maps(k, [4, 9], maps=False)
    assert k._ctx.device_bytes() == b1
    coarse.flux_maps(k, [4])
    b2 = k._ctx.device_bytes()
    assert b2 - b1 == 3 * nx * nx * 8
    coarse.flux_maps(k, [4, 9])
    assert k._ctx.device_bytes() == b2
    k._ctx.close()
    assert make("coupled", nx)._ctx.device_bytes() == b0   # closed with the context: the next one starts where this one did


# ---- 7. the larger plans -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [2048, 4096])
def test_identity_on_the_larger_plans(nx):
    """white noise in physical space (test_gpu_at_size's rough-field scaling, filter on), one cut with 3 B < nx, all three maps"""
    import niwqg_amd
    from niwqg_amd import coarse
    from niwqg_amd.transfer import spectral_transfer
    m = niwqg_amd.CoupledModel.Model(**rough_kwargs(nx))
    rng = np.random.default_rng(11)
    m.set_q(1e-5 * rng.standard_normal((nx, nx)))
    m.set_phi(0.05 * (rng.standard_normal((nx, nx)) + 1j * rng.standard_normal((nx, nx))))
    advance(m, 1, batched=True)
    B = nx // 8
    t0 = time.time()
    R = coarse.flux_maps(m, [B])
    print("%d: flux_maps with maps %.2f s" % (nx, time.time() - t0))
    st = spectral_transfer(m)
    for name in coarse.NAMES:
        err, scale = abs(R.mean[name][0] - st.flux[name][B]), np.abs(R.maps[name][0]).mean() + np.abs(st.transfer[name]).sum()
        print("%d %s B = %d: %.3g" % (nx, name, B, err / scale))
        assert scale > 0 and err <= 1e-12 * scale, (name, err, scale)
    m._ctx.close()


def test_refused_at_8192():
    """the 8192-point row plan gives a thread 128 registers, the maps need 7 values per point: refused before any allocation"""
    import niwqg_amd
    from niwqg_amd import coarse, _lib
    from niwqg_amd.spectra import shell_count
    nx = 8192
    m = niwqg_amd.CoupledModel.Model(**rough_kwargs(nx))
    b0 = m._ctx.device_bytes()
    with pytest.raises(NotImplementedError, match="8192"):
        coarse.flux_maps(m, [64])
    L = _lib.lib()
    g, mom = coarse.sharp(m, 64), np.zeros(6)
    assert L.nq_coarse_flux(m._ctx.h, 7, 1, _lib._dptr(g), shell_count(nx), _lib._dptr(mom), None) == -1
    assert b"section 7" in L.nq_last_error(m._ctx.h) and m._ctx.device_bytes() == b0
    m._ctx.close()
