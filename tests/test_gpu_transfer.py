"""Spectral transfer and flux spectra (niwqg_amd/transfer.py, nq_transfer_binned): per-shell agreement with a numpy
restatement of the definitions written here, the exact identities, the sign and normalisation against the model's own
dynamics, determinism, no side effects, slab ranks and the any-size path."""
import numpy as np
import pytest

from test_oracle_golden import notebook_kwargs
from test_gpu_spectra import make, steps, np_shell, MASKS, ATOMIC, LEFTOVERS

pytestmark = pytest.mark.gpu


def restated(m):
    """the transfer spectra from the host fields, in numpy.  F = fft2 on the full plane; u, v as the
    reference's jacobian_psi_q forms them (Kernel family: Re ifft2 of the full plane; QGModel: irfft2 of its half plane)."""
    nx, M2 = m.nx, float(m.nx) ** 4
    b = np_shell(nx).ravel()
    nb = int(b.max()) + 1
    k = np.fft.fftfreq(nx, 1.0 / nx) * m.dk
    kx, ly = k[None, :], k[:, None]

    def binned(x):
        return np.bincount(b, weights=np.ravel(x), minlength=nb)
    F = np.fft.fft2
    if m.ph.shape[1] == nx:
        P = F(np.fft.ifft2(m.ph).real)
        u, v = np.fft.ifft2(-1j * ly * P).real, np.fft.ifft2(1j * kx * P).real
    else:
        kh = np.fft.rfftfreq(nx, 1.0 / nx)[None, :] * m.dk
        P = F(np.fft.irfft2(m.ph, s=(nx, nx)))
        u, v = np.fft.irfft2(-1j * ly * m.ph, s=(nx, nx)), np.fft.irfft2(1j * kh * m.ph, s=(nx, nx))
    out = {}
    if getattr(m, "model_id", None) != 3:                 # YBJModel does not step q
        Q = F(m.q)
        Jq = 1j * kx * F(u * m.q) + 1j * ly * F(v * m.q)
        out.update(ke_qg=binned((np.conj(P) * Jq).real) / M2, ens=-binned((np.conj(Q) * Jq).real) / M2)
    if hasattr(m, "phih"):
        J = F(u * m.phix + v * m.phiy)
        R = 1j * F(m.phi * m.q_psi)
        out.update(ke_niw_adv=-binned((np.conj(m.phih) * J).real) / M2,
                   ke_niw_ref=-binned((np.conj(m.phih) * 0.5 * R).real) / M2)
    if getattr(m, "passive_scalar", False):
        C = F(m.c)
        Jc = 1j * kx * F(u * m.c) + 1j * ly * F(v * m.c)
        t = (np.conj(C) * Jc).real
        out.update(C2=-2 * binned(t) / M2, gradC2=-2 * binned((kx ** 2 + ly ** 2) * t) / M2)
    return out


CASES = [(k, msk) for k in ("coupled", "uncoupled", "ybj") for msk in ("filter", "none", "mask", "dual")] + \
        [(k, msk) for k in ("qg", "qgc") for msk in ("filter", "none")]


@pytest.mark.parametrize("kind,mask", CASES)
def test_against_numpy(kind, mask):
    from niwqg_amd.transfer import spectral_transfer, available
    from niwqg_amd.spectra import shell_modes
    m = make(kind, 128, mask)
    steps(m, 20)
    st = spectral_transfer(m)
    ref = restated(m)
    assert set(st.transfer) == set(available(m)) == set(ref)
    assert np.array_equal(st.modes, shell_modes(128)) and np.allclose(st.k_edge, (st.shell + 0.5) * m.dk)
    assert st.k_iso_max == 64 * m.dk
    for name, t in st.transfer.items():
        assert t.dtype == np.float64 and t.shape == st.shell.shape
        err = np.abs(t - ref[name]).max() / np.abs(ref[name]).sum()
        assert err <= 1e-10, (name, err)
        assert np.array_equal(st.flux[name], -np.cumsum(t))


@pytest.mark.parametrize("kind,mask", [(k, msk) for k in ("coupled", "uncoupled", "ybj") for msk in MASKS])
def test_refraction_transfer_sums_to_zero(kind, mask):
    """Re(conj(phi) i phi q_psi) = 0 at every point: the refractive transfer only moves wave energy between shells"""
    from niwqg_amd.transfer import spectral_transfer
    m = make(kind, 128, mask)
    steps(m, 10)
    t = spectral_transfer(m, names=["ke_niw_ref"]).transfer["ke_niw_ref"]
    assert np.abs(t).sum() > 0
    assert abs(t.sum()) <= 1e-12 * np.abs(t).sum(), (t.sum(), np.abs(t).sum())


@pytest.mark.parametrize("kind", ["coupled", "uncoupled", "qg", "qgc"])
def test_balanced_energy_transfer_sums_to_zero_with_the_filter(kind):
    """psi_x u q + psi_y v q = 0 at every point once the Nyquist content is filtered away"""
    from niwqg_amd.transfer import spectral_transfer
    m = make(kind, 128, "filter")
    steps(m, 10)
    t = spectral_transfer(m, names="ke_qg").transfer["ke_qg"]
    assert np.abs(t).sum() > 0
    assert abs(t.sum()) <= 1e-12 * np.abs(t).sum(), (t.sum(), np.abs(t).sum())


def make_inviscid(kind, nx, dt_scale, seed=1):
    """no filter, every viscosity and drag zero, a smooth state band-limited to shells <= nx/6; U != 0 (QGModel: beta too)"""
    import niwqg_amd
    kw = notebook_kwargs(nx, False)
    kw.update(nu4=0.0, nu=0.0, mu=0.0, nu4w=0.0, nuw=0.0, muw=0.0, dt=kw["dt"] * dt_scale)
    if kind in ("qg", "qgc"):
        for k in ("m", "N", "f", "nu4w", "nuw", "muw"):
            kw.pop(k)
        kw.update(beta=1e-11, passive_scalar=(kind == "qgc"), nu4c=0.0, nuc=0.0, muc=0.0)
        m = niwqg_amd.QGModel.Model(**kw)
    else:
        m = {"coupled": niwqg_amd.CoupledModel, "uncoupled": niwqg_amd.UnCoupledModel}[kind].Model(**kw)
    rng = np.random.default_rng(seed)
    sh = np_shell(nx)
    band = np.where(sh <= nx // 6, np.exp(-(sh / (nx / 16.0)) ** 2), 0.0)

    def smooth(cplx):
        z = rng.standard_normal((nx, nx)) + (1j * rng.standard_normal((nx, nx)) if cplx else 0)
        z = np.fft.ifft2(np.fft.fft2(z) * band)
        return z / np.abs(z).std() if cplx else z.real / z.real.std()
    m.set_q(1e-5 * smooth(False))
    if kind == "qgc":
        m.set_c(smooth(False))
    elif kind not in ("qg",):
        m.set_phi(0.1 * smooth(True))
    return m


@pytest.mark.parametrize("kind,name", [("coupled", "ens"), ("coupled", "ke_niw"), ("uncoupled", "ke_qg"), ("qg", "ke_qg"),
                                       ("qgc", "C2")])
def test_transfer_is_the_tendency_of_the_spectrum(kind, name):
    """(X(t + dt) - X(t)) / dt of isotropic_spectra against T_X(t), per shell, with dt and dt/2: the error is first order"""
    from niwqg_amd.spectra import isotropic_spectra
    from niwqg_amd.transfer import spectral_transfer
    errs = []
    for scale in (0.25, 0.125):
        m = make_inviscid(kind, 64, scale)
        X0 = isotropic_spectra(m, names=[name]).values[name]
        st = spectral_transfer(m)
        T = st.transfer["ke_niw_adv"] + st.transfer["ke_niw_ref"] if name == "ke_niw" else st.transfer[name]
        m._step_forward()
        X1 = isotropic_spectra(m, names=[name]).values[name]
        errs.append(np.linalg.norm((X1 - X0) / m.dt - T) / np.linalg.norm(T))
    assert errs[1] <= 0.05, errs
    assert 1.6 <= errs[0] / errs[1] <= 2.4, errs


@pytest.mark.parametrize("kind", ["coupled", "qgc"])
def test_two_calls_are_bit_identical(kind):
    from niwqg_amd.transfer import spectral_transfer
    m = make(kind, 512, "filter")
    steps(m, 3)
    a, b = spectral_transfer(m), spectral_transfer(m)
    for name in a.transfer:
        assert np.array_equal(a.transfer[name], b.transfer[name]), name


def _run(kind, call, mask="filter"):
    from niwqg_amd.transfer import spectral_transfer
    m = make(kind, 64, mask, tdiags=3)
    m.twrite = 5
    qs = []
    while m.tc < 30:
        m._step_forward()
        if call:
            spectral_transfer(m)
        qs.append(np.array(m.q))
    out = {"q": np.array(qs)}
    out.update({"diag:" + n: np.array(d['value']) for n, d in m.diagnostics.items() if 'value' in d})
    if kind != "qgc":
        out["phi"] = np.array(m.phi)
    for name in LEFTOVERS[kind]:
        out[name] = np.array(getattr(m, name))
    return out


@pytest.mark.parametrize("kind,mask", [("coupled", "filter"), ("coupled", "dual"), ("uncoupled", "filter"), ("uncoupled", "dual"),
                                       ("ybj", "filter"), ("qgc", "filter")])
def test_transfer_leaves_the_run_alone(kind, mask):
    """30 steps, ticks every 3, status lines every 5, with and without a spectral_transfer call after every step: bit-identical
    state, leftovers and diagnostics series; the atomically reduced scalars (test_gpu_spectra.ATOMIC) to rounding"""
    a, b = _run(kind, False, mask), _run(kind, True, mask)
    assert set(a) == set(b)
    for n in a:
        if n in ATOMIC and not (n in ("diag:ep_phi", "diag:chi_phi") and kind == "coupled"):
            assert np.allclose(a[n], b[n], rtol=1e-12, atol=0), n
        else:
            assert np.array_equal(a[n], b[n], equal_nan=True), n


def test_recording_inside_run_with_snapshots():
    from niwqg_amd.transfer import spectral_transfer
    m = make("coupled", 64, "filter", tdiags=2)
    m.tmax = 6.5 * m.dt
    rec = [spectral_transfer(m, names=["ens", "ke_niw_adv"]) for _ in m.run_with_snapshots(tsnapint=2 * m.dt)]
    assert len(rec) == 3 and all(set(r.transfer) == set(r.flux) == {"ens", "ke_niw_adv"} for r in rec)
    assert m.tc == 7


def test_unavailable_names_and_phi_missing():
    import niwqg_amd
    from niwqg_amd.transfer import spectral_transfer
    with pytest.raises(ValueError, match="valid names: ke_niw_adv, ke_niw_ref"):
        spectral_transfer(make("ybj", 64), names=["ke_qg"])
    with pytest.raises(ValueError, match="valid names: ke_qg, ens"):
        spectral_transfer(make("qg", 64), names=["C2"])
    c = niwqg_amd.CoupledModel.Model(**notebook_kwargs(64, True))
    with pytest.raises(RuntimeError, match="set_phi"):
        spectral_transfer(c)


@pytest.mark.parametrize("P", [2, 4])
@pytest.mark.parametrize("kind,mask", [("coupled", "filter"), ("coupled", "dual"), ("uncoupled", "none"), ("ybj", "filter"),
                                       ("qg", "none"), ("qgc", "filter")])
def test_slab_peers_equal_the_single_context(kind, mask, P):
    """slab=P peer ranks on one GPU: every rank bins its own columns, the ranks are summed in rank order"""
    from niwqg_amd.transfer import spectral_transfer
    one, sl = make(kind, 128, mask, tdiags=3), make(kind, 128, mask, tdiags=3, slab=P)
    for m in (one, sl):
        steps(m, 5)
    a, b = spectral_transfer(one), spectral_transfer(sl)
    c = spectral_transfer(sl)
    assert set(a.transfer) == set(b.transfer)
    for name in a.transfer:
        assert np.abs(a.transfer[name] - b.transfer[name]).max() <= 1e-12 * np.abs(a.transfer[name]).sum(), name
        assert np.array_equal(b.transfer[name], c.transfer[name]), name


GLOO_WORKER = """
import os, sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import torch.distributed as dist
from test_gpu_spectra import make, steps
from niwqg_amd.transfer import spectral_transfer
m = make("coupled", 64, "filter", tdiags=3)
steps(m, 4)
st = spectral_transfer(m)
arr = np.array([st.transfer[n] for n in sorted(st.transfer)])
rank = dist.get_rank()
np.save(os.path.join(%r, "transfer_%%d.npy" %% rank), arr)
print("transfer rank", rank, "done")
"""


def test_two_processes_over_gloo(tmp_path):
    """torch.distributed.run with two processes on the one GPU (callbacks + gloo): both ranks return the same array, and it
    equals the single-context transfer"""
    import os
    import subprocess
    import sys
    from conftest import free_port
    from niwqg_amd.transfer import spectral_transfer
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "transfer_worker.py"
    script.write_text(GLOO_WORKER % (root, os.path.join(root, "tests"), str(tmp_path)))
    env = dict(os.environ, NIWQG_AMD_DIST_BACKEND="gloo")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                          "--master-addr", "127.0.0.1", "--master-port", str(free_port()), str(script)],
                         capture_output=True, text=True, timeout=600, env=env)
    if out.returncode != 0:
        print(out.stdout[-3000:])
        print(out.stderr[-6000:])
    assert out.returncode == 0
    a0, a1 = np.load(tmp_path / "transfer_0.npy"), np.load(tmp_path / "transfer_1.npy")
    assert np.array_equal(a0, a1)
    m = make("coupled", 64, "filter", tdiags=3, slab=False)
    steps(m, 4)
    st = spectral_transfer(m)
    ref = np.array([st.transfer[n] for n in sorted(st.transfer)])
    assert np.all(np.abs(a0 - ref).max(axis=1) <= 1e-12 * np.abs(ref).sum(axis=1))


@pytest.mark.parametrize("nx", [96, 100, 192])
@pytest.mark.parametrize("kind", ["coupled", "uncoupled", "ybj", "qg", "qgc"])
def test_any_size_against_numpy(kind, nx):
    """grids without a fused plan: the path's own planes, binned by nq_any_bin, against the same restatement"""
    from niwqg_amd.transfer import spectral_transfer, available
    from niwqg_amd.spectra import shell_count
    m = make(kind, nx, "filter")
    assert getattr(m, "_any_size", False)
    steps(m, 6)
    ref = restated(m)
    st = spectral_transfer(m)
    assert st.shell.shape == (shell_count(nx),) and st.modes.sum() == nx * nx
    assert set(st.transfer) == set(available(m)) == set(ref)
    for name, t in st.transfer.items():
        err = np.abs(t - ref[name]).max() / np.abs(ref[name]).sum()
        assert err <= 1e-10, (name, err)
    again = spectral_transfer(m)
    for name in st.transfer:
        assert np.array_equal(st.transfer[name], again.transfer[name]), name
