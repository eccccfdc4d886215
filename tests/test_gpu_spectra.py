"""Isotropic spectra of the diagnostics tick (niwqg_amd/spectra.py, nq_diagnostics_binned): shell sums close on the tick's
raw sums and on the registry's scalars, agree per shell with a numpy restatement written here (the integer shell rule plus the
reference's expressions), are deterministic, and leave the simulation alone."""
import numpy as np
import pytest

from test_oracle_golden import notebook_kwargs, K0, U0

pytestmark = pytest.mark.gpu

KERNEL_ROWS = [0, 1, 2, 3] + list(range(6, 15)) + [24, 27, 28, 31]
QG_ROWS = list(range(6, 15))
QGC_ROWS = QG_ROWS + [16, 17, 18, 19]
MASKS = {"filter": dict(use_filter=True), "mask": dict(use_filter=False, dealias=True), "none": dict(use_filter=False),
         "dual": dict(use_filter=True, exact_qh=True)}


def np_shell(nx):
    n = np.append(np.arange(0, nx // 2), np.arange(-(nx // 2), 0)).astype(np.int64)
    r2 = 4 * (n[None, :] ** 2 + n[:, None] ** 2)
    s = np.sqrt(r2.astype(float)).astype(np.int64)
    s -= s * s > r2
    s += (s + 1) * (s + 1) <= r2
    return (s + 1) // 2


def make(kind, nx, mask="filter", tdiags=10 ** 9, seed=0, **extra):
    import niwqg_amd
    from niwqg_amd import InitialConditions as ic
    kw = notebook_kwargs(nx, False, tdiags=tdiags)
    kw.update(MASKS[mask])
    kw.update(extra)
    if kind in ("qg", "qgc"):
        for k in ("m", "N", "f", "nu4w", "nuw", "muw"):
            kw.pop(k)
        kw.pop("exact_qh", None)
        kw.update(mu=2e-8, nu=0.0, passive_scalar=(kind == "qgc"), nu4c=kw["nu4"], nuc=5.0, muc=1e-8)
        m = niwqg_amd.QGModel.Model(**kw)
    else:
        kw.update(nu4w=3e9 * (128.0 / nx) ** 4, muw=1e-7, mu=2e-8)
        cls = {"coupled": niwqg_amd.CoupledModel, "uncoupled": niwqg_amd.UnCoupledModel, "ybj": niwqg_amd.YBJModel}[kind]
        m = cls.Model(**kw)
    rng = np.random.default_rng(seed)
    sh = np_shell(nx)

    def noise(cplx):
        z = rng.standard_normal((nx, nx)) + (1j * rng.standard_normal((nx, nx)) if cplx else 0)
        z = np.fft.ifft2(np.fft.fft2(z) * np.exp(-(sh / 12.0) ** 2))
        return z if cplx else z.real
    q = ic.LambDipole(m, U=U0, R=2 * np.pi / K0)
    n = noise(False)
    m.set_q(q + 0.3 * q.std() * n / n.std())
    if kind == "qgc":
        c = noise(False)
        m.set_c(c / c.std())
    elif kind not in ("qg",):
        p = noise(True)
        m.set_phi(0.2 * (1 + 0.5j) / np.sqrt(2) + 0.05 * p / np.abs(p).std())
    return m


def steps(m, n):
    while m.tc < n:
        m._step_forward()


def rows_of(kind):
    return KERNEL_ROWS if kind in ("coupled", "uncoupled", "ybj") else (QGC_ROWS if kind == "qgc" else QG_ROWS)


def check_raw_closure(m, kind):
    S = m._ctx.diagnostic_sums_binned()
    s = m._ctx.diagnostic_sums()
    from niwqg_amd.spectra import shell_count
    assert S.shape == (32, shell_count(m.nx))
    rows = rows_of(kind)
    for r in range(32):
        if r in rows:
            assert abs(S[r].sum() - s[r]) <= 1e-11 * np.abs(S[r]).sum() + 1e-300, (r, S[r].sum(), s[r])
        else:
            assert not S[r].any(), r


CASES = [(k, msk) for k in ("coupled", "uncoupled", "ybj") for msk in MASKS] + [("qg", "filter"), ("qg", "none"),
                                                                               ("qgc", "filter"), ("qgc", "none")]


@pytest.mark.parametrize("nx", [64, 128, 512])
@pytest.mark.parametrize("kind,mask", CASES)
def test_raw_closure(kind, mask, nx):
    m = make(kind, nx, mask, tdiags=3)
    check_raw_closure(m, kind)                     # right after set_q / set_phi / set_c
    steps(m, 2)                                    # a tick at tc = 0 only
    check_raw_closure(m, kind)
    steps(m, 4)                                    # the tick at tc = 3 ran inside
    check_raw_closure(m, kind)


def tick_now(m):
    from niwqg_amd.Diagnostics import increment_diagnostics
    td = m.tdiags
    m.tdiags = 1
    try:
        increment_diagnostics(m)
    finally:
        m.tdiags = td
    return {name: float(np.ravel(d['value'])[-1]) for name, d in m.diagnostics.items() if 'value' in d}


def check_named(sp, scal, names):
    for name in names:
        v = sp.values[name]
        assert abs(v.sum() - scal[name]) <= 1e-11 * np.abs(v).sum() + 1e-300, (name, v.sum(), scal[name])


@pytest.mark.parametrize("kind,mask", [("coupled", "filter"), ("coupled", "dual"), ("uncoupled", "filter"), ("ybj", "none"),
                                       ("qg", "filter"), ("qgc", "filter"), ("qgc", "none")])
def test_named_closure(kind, mask):
    from niwqg_amd.spectra import isotropic_spectra, available
    m = make(kind, 128, mask)
    names = available(m)
    check_named(isotropic_spectra(m), tick_now(m), names)               # right after set_phi: every name
    steps(m, 7)
    if kind in ("uncoupled", "ybj"):                                     # quirk Q1: the scalars' stale gradient mean
        names = [n for n in names if n not in ("ep_phi", "chi_phi")]
    check_named(isotropic_spectra(m), tick_now(m), names)


def restated(m):
    """the named spectra from the host fields, in numpy: the reference's expressions, summed per shell"""
    nx, M2 = m.nx, float(m.nx) ** 4
    b = np_shell(nx).ravel()
    nb = int(b.max()) + 1
    k = np.fft.fftfreq(nx, 1.0 / nx) * m.dk
    kx, ly = k[None, :], k[:, None]
    wv2 = kx ** 2 + ly ** 2
    wv4 = wv2 ** 2

    def binned(x):
        return np.bincount(b, weights=np.ravel(x), minlength=nb)
    F = np.fft.fft2
    Q = F(m.q)
    P = F(np.fft.ifft2(m.ph).real if m.ph.shape[1] == nx else np.fft.irfft2(m.ph, s=(nx, nx)))     # the Kernel family's ph is full
    pq = (np.conj(P) * Q).real
    ybj = getattr(m, "model_id", None) == 3               # YBJModel: the reference's p stays zero, ep_psi keeps its nu4 term
    out = dict(ke_qg=binned(0.5 * wv2 * np.abs(P) ** 2) / M2, ens=binned(0.5 * np.abs(Q) ** 2) / M2,
               chi_q=-m.nu4 * binned(wv4 * np.abs(Q) ** 2) / M2,
               ep_psi=(m.nu4 * binned(wv4 * pq) + (0.0 if ybj else m.nu * binned(wv2 * pq) + m.mu * binned(pq))) / M2)
    if hasattr(m, "phih"):
        ph = m.phih
        a2 = np.abs(ph) ** 2
        out.update(ke_niw=binned(0.5 * a2) / M2, pe_niw=binned(0.25 * wv2 * a2) / M2 / m.kappa2,
                   ep_phi=(-m.nu4w * binned(wv4 * a2) - m.muw * binned(a2) - m.nuw * binned(wv2 * a2)) / M2,
                   chi_phi=(-0.5 * m.nu4w * binned(wv4 * wv2 * a2) - 0.5 * m.nuw * binned(wv4 * a2)
                            - 0.5 * m.muw * binned(wv2 * a2)) / M2 / m.kappa2)
        u, v = np.fft.ifft2(-1j * ly * P).real, np.fft.ifft2(1j * kx * P).real
        J = F(u * m.phix + v * m.phiy)
        R = 1j * F(m.phi * m.q_psi)
        lap = -wv2 * ph
        diss = -(m.nu4w * wv4 + m.nuw * wv2 + m.muw) * ph
        M2f = M2 * m.f
        out.update(gamma_a=0.5 * m.hslash * binned((np.conj(lap) * J).real) / M2f,
                   xi_r=binned((np.conj(diss) * J).imag) / M2f,
                   gamma_r=0.25 * m.hslash * binned((np.conj(lap) * R).real) / M2f,
                   xi_a=0.5 * binned((np.conj(diss) * R).imag) / M2f)
    if getattr(m, "passive_scalar", False):
        C = F(m.c)
        c2 = np.abs(C) ** 2
        c2[0, 0] = 0.0
        s16, s17, s18, s19 = binned(c2), binned(wv2 * c2), binned(wv4 * c2), binned(wv4 * wv2 * c2)
        out.update(C2=s16 / M2, gradC2=s17 / M2, ep_c=(-2 * m.nu4c * s18 - 2 * m.nu * s17 - 2 * m.muc * s16) / M2,
                   chi_c=(-2 * m.nu4c * s19 - 2 * m.nu * s18 - 2 * m.muc * s17) / M2)
    return out


@pytest.mark.parametrize("kind", ["coupled", "uncoupled", "ybj", "qg", "qgc"])
def test_against_numpy(kind):
    from niwqg_amd.spectra import isotropic_spectra, shell_modes
    m = make(kind, 128, "filter")
    steps(m, 20)
    sp = isotropic_spectra(m)
    assert np.array_equal(sp.modes, shell_modes(128)) and sp.modes.sum() == 128 ** 2
    assert np.allclose(sp.k, sp.shell * m.dk) and sp.k_iso_max == 64 * m.dk
    ref = restated(m)
    for name, v in sp.values.items():
        assert v.dtype == np.float64 and v.shape == sp.shell.shape
        err = np.abs(v - ref[name]).max() / np.abs(ref[name]).sum()
        assert err <= 1e-10, (name, err)


@pytest.mark.parametrize("kind", ["coupled", "qgc"])
def test_two_calls_are_bit_identical(kind):
    from niwqg_amd.spectra import isotropic_spectra
    m = make(kind, 512, "filter")
    steps(m, 3)
    a, b = isotropic_spectra(m), isotropic_spectra(m)
    for name in a.values:
        assert np.array_equal(a.values[name], b.values[name]), name


LEFTOVERS = {"coupled": ("phix", "phiy", "u", "v", "lapphi", "gamma1", "Ke", "Pw", "Kw", "phq", "uq"),
             "uncoupled": ("phix", "phiy", "u", "v", "lapphi", "gamma1", "Ke", "Pw", "Kw"),
             "ybj": ("phix", "phiy", "u", "v", "lapphi", "gamma1"),
             "qgc": ("u", "v", "Ke", "c", "lapc")}


def _run(kind, call, mask="filter"):
    from niwqg_amd.spectra import isotropic_spectra
    m = make(kind, 64, mask, tdiags=3)
    m.twrite = 5
    qs = []
    while m.tc < 30:
        m._step_forward()
        if call:
            isotropic_spectra(m)
        qs.append(np.array(m.q))
    out = {"q": np.array(qs)}
    out.update({"diag:" + n: np.array(d['value']) for n, d in m.diagnostics.items() if 'value' in d})
    if kind != "qgc":
        out["phi"] = np.array(m.phi)
    for name in LEFTOVERS[kind]:
        out[name] = np.array(getattr(m, name))
    return out


# scalars the package forms with floating-point atomics (k_reduce: ke_qg, pe_niw, the budgets Ke, Pw, Kw that start from
# them, and UnCoupled / YBJ's ep_phi, chi_phi through the gradient mean 4 kappa2 pe_niw of quirk Q1): their last bits differ
# between ANY two runs, with or without spectra (YBJModel's Pw is fixed at set_phi, before any call)
ATOMIC = {"diag:ke_qg", "diag:pe_niw", "diag:Ke", "diag:Pw", "diag:Kw", "Ke", "Pw", "Kw", "diag:ep_phi", "diag:chi_phi"}


@pytest.mark.parametrize("kind,mask", [("coupled", "filter"), ("coupled", "dual"), ("uncoupled", "filter"), ("uncoupled", "dual"),
                                       ("ybj", "filter"), ("ybj", "dual"), ("qgc", "filter")])
def test_spectra_leave_the_run_alone(kind, mask):
    """30 steps, ticks every 3, status lines every 5: a run that calls isotropic_spectra after every step against one that
    never does.  Bit-identical state, leftovers and diagnostics series; the atomically reduced scalars to rounding."""
    a, b = _run(kind, False, mask), _run(kind, True, mask)
    assert set(a) == set(b)
    for n in a:
        if n in ATOMIC and not (n in ("diag:ep_phi", "diag:chi_phi") and kind == "coupled"):
            assert np.allclose(a[n], b[n], rtol=1e-12, atol=0), n
        else:
            assert np.array_equal(a[n], b[n], equal_nan=True), n


def test_recording_inside_run_with_snapshots():
    from niwqg_amd.spectra import isotropic_spectra
    m = make("coupled", 64, "filter", tdiags=2)
    m.tmax = 6.5 * m.dt
    rec = [isotropic_spectra(m, names=["gamma_a", "ke_niw"]).values for _ in m.run_with_snapshots(tsnapint=2 * m.dt)]
    assert len(rec) == 3 and all(set(r) == {"gamma_a", "ke_niw"} for r in rec)
    assert m.tc == 7


def test_unavailable_names_and_phi_missing():
    import niwqg_amd
    from niwqg_amd.spectra import isotropic_spectra
    m = make("qg", 64)
    with pytest.raises(ValueError, match="valid names"):
        isotropic_spectra(m, names=["gamma_a"])
    c = niwqg_amd.CoupledModel.Model(**notebook_kwargs(64, True))
    with pytest.raises(RuntimeError, match="set_phi"):
        isotropic_spectra(c)


@pytest.mark.parametrize("P", [2, 4])
@pytest.mark.parametrize("kind,mask", [("coupled", "filter"), ("coupled", "dual"), ("uncoupled", "none"), ("ybj", "filter"),
                                       ("qgc", "filter")])
def test_slab_peers_equal_the_single_context(kind, mask, P):
    """slab=P peer ranks on one GPU: every rank bins its own columns, the ranks are summed in rank order"""
    from niwqg_amd.spectra import isotropic_spectra
    one, sl = make(kind, 128, mask, tdiags=3), make(kind, 128, mask, tdiags=3, slab=P)
    for m in (one, sl):
        steps(m, 5)
    a, b = isotropic_spectra(one), isotropic_spectra(sl)
    c = isotropic_spectra(sl)
    assert set(a.values) == set(b.values)
    for name in a.values:
        assert np.abs(a.values[name] - b.values[name]).max() <= 1e-12 * np.abs(a.values[name]).sum(), name
        assert np.array_equal(b.values[name], c.values[name]), name


GLOO_WORKER = """
import os, sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import torch.distributed as dist
from test_gpu_spectra import make, steps
from niwqg_amd.spectra import isotropic_spectra
m = make("coupled", 64, "filter", tdiags=3)
steps(m, 4)
sp = isotropic_spectra(m)
arr = np.array([sp.values[n] for n in sorted(sp.values)])
rank = dist.get_rank()
np.save(os.path.join(%r, "spec_%%d.npy" %% rank), arr)
print("spectra rank", rank, "done")
"""


def test_two_processes_over_gloo(tmp_path):
    """torch.distributed.run with two processes on the one GPU (callbacks + gloo): both ranks return the same array, and it
    equals the single-context spectra"""
    import os
    import subprocess
    import sys
    from conftest import free_port
    from niwqg_amd.spectra import isotropic_spectra
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "spectra_worker.py"
    script.write_text(GLOO_WORKER % (root, os.path.join(root, "tests"), str(tmp_path)))
    env = dict(os.environ, NIWQG_AMD_DIST_BACKEND="gloo")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                          "--master-addr", "127.0.0.1", "--master-port", str(free_port()), str(script)],
                         capture_output=True, text=True, timeout=600, env=env)
    if out.returncode != 0:
        print(out.stdout[-3000:])
        print(out.stderr[-6000:])
    assert out.returncode == 0
    a0, a1 = np.load(tmp_path / "spec_0.npy"), np.load(tmp_path / "spec_1.npy")
    assert np.array_equal(a0, a1)
    m = make("coupled", 64, "filter", tdiags=3, slab=False)
    steps(m, 4)
    sp = isotropic_spectra(m)
    ref = np.array([sp.values[n] for n in sorted(sp.values)])
    assert np.all(np.abs(a0 - ref).max(axis=1) <= 1e-12 * np.abs(ref).sum(axis=1))


@pytest.mark.parametrize("nx", [96, 100, 192])
@pytest.mark.parametrize("kind", ["coupled", "uncoupled", "ybj", "qg", "qgc"])
def test_any_size_closure_and_numpy(kind, nx):
    """grids without a fused plan: closure on the path's own scalars (as test_named_closure) and the numpy restatement"""
    from niwqg_amd.spectra import isotropic_spectra, available, shell_count
    m = make(kind, nx, "filter")
    assert getattr(m, "_any_size", False)
    names = available(m)
    if kind != "qgc":                  # (this path's Gamma_c needs the u, v a step leaves: its tick runs after a step there)
        check_named(isotropic_spectra(m), tick_now(m), names)
    steps(m, 6)
    sp = isotropic_spectra(m)
    assert sp.shell.shape == (shell_count(nx),) and sp.modes.sum() == nx * nx
    ref = restated(m)                  # before the tick below refreshes phix, phiy
    close = [n for n in names if not (kind in ("uncoupled", "ybj") and n in ("ep_phi", "chi_phi"))]
    check_named(sp, tick_now(m), close)
    for name, v in sp.values.items():
        err = np.abs(v - ref[name]).max() / np.abs(ref[name]).sum()
        assert err <= 1e-10, (name, err)
