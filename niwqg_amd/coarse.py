"""Coarse-grained energy and enstrophy flux maps, formed on the device.

    from niwqg_amd import coarse
    R = coarse.flux_maps(m, scales=[8, 32, 128])            # sharp cuts at shells 8, 32, 128
    R.maps["ens"][i], R.mean["ens"][i], R.variance["ens"][i], R.shell, R.k_cut

``transfer.spectral_transfer`` says where in WAVENUMBER the nonlinear terms move energy and enstrophy; these maps say where in
the DOMAIN the transfer across one scale happens.  G is a real isotropic filter given per shell (the shell rule of
``spectra.shell_of``), G(l, k) = g[shell], an overbar is F^-1[G .], and the planes are the ones the transfer bins: P = psi-hat,
Q = q-hat (dual-q models: the mean of the two copies), Fu = F[u q], Fv = F[v q], W = the CURRENT phi-hat and J = F[u phix + v phiy]
of the tick's first products pass (UnCoupledModel, YBJModel: with the stale gradients of quirk Q1, as ``transfer`` documents).

    u-bar, v-bar        Re F^-1[-il G P], Re F^-1[ik G P]
    q-bar and gradient  from G Q;    phi-bar and gradient from G W
    tau                 (F^-1[G Fu] - u-bar q-bar, F^-1[G Fv] - v-bar q-bar), the sub-filter PV flux

    ke_qg        tau . grad psi-bar = v-bar F^-1[G Fu] - u-bar F^-1[G Fv]                 CoupledModel, UnCoupledModel, QGModel
    ens          -tau . grad q-bar                                                        CoupledModel, UnCoupledModel, QGModel
    ke_niw_adv   Re(conj(phi-bar) (F^-1[G J] - u-bar phi-bar_x - v-bar phi-bar_y))         CoupledModel, UnCoupledModel, YBJModel

Positive means transfer towards scales smaller than the cut.  For the sharp filter at shell B the plane mean of a map is the
spectral flux through the cut, ``spectral_transfer(m).flux[name][B]``: ``ke_qg`` for every 1 <= B <= nx/2 - 1 (its resolved term
cancels at every point), ``ens`` and ``ke_niw_adv`` while 3 B < nx (the resolved triple product is then alias-free and has zero
mean).

Nyquist rule: every filter table is zero on the shells b >= nx/2, so row ny/2, column nx/2 and the passenger row of q-hat have
nothing in any filtered field.

Fused single-GPU grids up to 4096; slab-decomposed models, the any-size path and nx = 8192 raise ``NotImplementedError``
(DESIGN.md section 7).
"""
import numpy as np

from . import _lib
from .spectra import shell_count, shell_of, _is_qg

NAMES = ("ke_qg", "ens", "ke_niw_adv")
BITS = {"ke_qg": _lib.CG_KE, "ens": _lib.CG_ENS, "ke_niw_adv": _lib.CG_NIW}
KINDS = ("sharp", "gaussian")
MAX_SCALES = _lib.CG_MAX_SCALES
REFUSED_NX = 8192                   # csrc/nq_coarse.hpp: the row plan of that size has no registers for the maps


def available(m):
    """the maps flux_maps(m) can form for this model"""
    if _is_qg(m):
        return ["ke_qg", "ens"]
    if getattr(m, "model_id", None) == _lib.YBJ:
        return ["ke_niw_adv"]
    return list(NAMES)


def sharp(m, B):
    """the table of the sharp spectral filter at shell B: 1 on the shells b <= B, 0 beyond; 1 <= B <= nx/2 - 1"""
    nx = int(m.nx)
    if int(B) != B or not 1 <= int(B) <= nx // 2 - 1:
        raise ValueError("coarse.sharp: shell %r; valid: the integers 1 .. nx/2 - 1 = %d" % (B, nx // 2 - 1))
    g = np.zeros(shell_count(nx))
    g[:int(B) + 1] = 1.0
    return g


def gaussian(m, ell):
    """the table of the Gaussian filter of length ell: exp(-(b dk ell)^2 / 24) on the shells b < nx/2, 0 from nx/2 on"""
    nx = int(m.nx)
    ell = float(ell)
    if not (np.isfinite(ell) and ell > 0):
        raise ValueError("coarse.gaussian: length %r; valid: a finite length > 0" % (ell,))
    b = np.arange(shell_count(nx), dtype=np.float64)
    g = np.exp(-(b * float(m.dk) * ell) ** 2 / 24.0)
    g[nx // 2:] = 0.0
    return g


def check_table(nx, table):
    """(nscales, nb) float64 of a table argument; the contract of nq_coarse_flux on it"""
    nb = shell_count(nx)
    t = np.array(table, dtype=np.float64, ndmin=2)
    if t.ndim != 2 or t.shape[1] != nb or not 1 <= t.shape[0] <= MAX_SCALES:
        raise ValueError("coarse: table of shape %s; valid: (nscales, nb) with 1 <= nscales <= %d and nb = %d shells"
                         % (np.shape(table), MAX_SCALES, nb))
    if not np.isfinite(t).all():
        raise ValueError("coarse: a table entry is not finite; valid: finite values")
    if np.any(t[:, nx // 2:] != 0.0):
        raise ValueError("coarse: a table is not zero on a shell >= nx/2 = %d; valid: zero from that shell on (the Nyquist rule)" % (nx // 2))
    return np.ascontiguousarray(t)


def _names(m, names, what):
    valid = available(m)
    if names is None:
        return valid
    names = [names] if isinstance(names, str) else list(names)
    bad = [n for n in names if n not in valid]
    if bad or not names or len(set(names)) != len(names):
        raise ValueError("%s: names %r not available for %s (each once, at least one); valid names: %s"
                         % (what, bad or names, type(m).__module__, ", ".join(valid)))
    return [n for n in NAMES if n in names]            # bit order: the order of the device's planes


def _tables(m, scales, kind, table):
    """(tables (nscales, nb), shells or None, lengths or None)"""
    if table is not None:
        if scales is not None:
            raise ValueError("coarse.flux_maps: give scales or table=, not both; valid: one of them")
        return check_table(m.nx, table), None, None
    if kind not in KINDS:
        raise ValueError("coarse.flux_maps: kind %r; valid: %s" % (kind, ", ".join(KINDS)))
    scales = list(np.atleast_1d(scales)) if scales is not None else []
    if not 1 <= len(scales) <= MAX_SCALES:
        raise ValueError("coarse.flux_maps: %d scales; valid: 1 to %d per call" % (len(scales), MAX_SCALES))
    if kind == "sharp":
        return check_table(m.nx, [sharp(m, B) for B in scales]), np.array(scales, dtype=np.int64), None
    return check_table(m.nx, [gaussian(m, ell) for ell in scales]), None, np.array(scales, dtype=np.float64)


def refuse(m, what="coarse.flux_maps"):
    """NotImplementedError for the models and grids that have no coarse-grained maps yet"""
    if getattr(m, "_any_size", False):
        raise NotImplementedError("%s: the any-size path (nx = %d has no fused plan) has no coarse-grained maps yet "
                                  "(DESIGN.md section 7); use a power of two from 64 to 4096" % (what, m.nx))
    if not isinstance(m._ctx, _lib.Context):
        raise NotImplementedError("%s: slab-decomposed models have no coarse-grained maps yet (DESIGN.md section 7); use a "
                                  "single-GPU model" % what)
    if m.nx >= REFUSED_NX:
        raise NotImplementedError("%s: no coarse-grained maps at nx = %d yet: a device thread of that row plan has 128 registers "
                                  "and the maps need 7 values per point (DESIGN.md section 7)" % (what, m.nx))


class FluxMaps(object):
    """names; table (nscales, nb); shell and k_cut = (shell + 1/2) dk for sharp scales (else None); ell for gaussian ones (else
    None); mean, variance: {name: float64 (nscales,)} over the plane; sums, sumsq: the device's raw moments; maps: {name:
    float64 (nscales, ny, nx)} or None"""

    def __init__(self, names, table, shell, ell, dk, M, moments, maps):
        self.names = tuple(names)
        self.table = table
        self.shell = shell
        self.ell = ell
        self.dk = dk
        self.k_cut = None if shell is None else (shell + 0.5) * dk
        self.sums = {n: moments[:, NAMES.index(n), 0].copy() for n in names}
        self.sumsq = {n: moments[:, NAMES.index(n), 1].copy() for n in names}
        self.mean = {n: self.sums[n] / M for n in names}
        self.variance = {n: self.sumsq[n] / M - self.mean[n] ** 2 for n in names}
        self.maps = maps

    def __repr__(self):
        return "FluxMaps(names=%s, nscales=%d, maps=%s)" % (list(self.names), len(self.table), self.maps is not None)


def flux_maps(m, scales=None, names=None, kind="sharp", maps=True, table=None):
    """Coarse-grained flux maps of the model's current state.  scales: integer shells B (kind="sharp", 1 <= B <= nx/2 - 1) or
    lengths ell > 0 (kind="gaussian"); or table=: an explicit (nscales, nb) array, zero from shell nx/2 on.  names: a subset of
    available(m) (default: all).  maps=False: the moments only, nothing but 6 doubles per scale leaves the GPU.  Works after
    set_q / set_phi, between steps and inside run_with_snapshots; changes nothing a step can see."""
    names = _names(m, names, "coarse.flux_maps")
    tab, shell, ell = _tables(m, scales, kind, table)
    refuse(m)
    mom, planes = m._ctx.coarse_flux(sum(BITS[n] for n in names), tab, len(names) if maps else 0)
    out = None if planes is None else {n: planes[:, i] for i, n in enumerate(names)}
    return FluxMaps(names, tab, shell, ell, float(m.dk), float(m.nx) * m.nx, mom, out)


def _full(h, nx):
    """full plane of a half spectrum (ny, nx/2 + 1) of a real field, by Hermitian symmetry"""
    return np.fft.fft2(np.fft.irfft2(h, s=(nx, nx)))


def reference(m, table, names=None):
    """THE definitions in numpy, from the public reads ``m.ph``, ``m.q``, and for the wave map ``m.phih``, ``m.phix``,
    ``m.phiy``: {name: float64 (nscales, ny, nx)} for the tables (nscales, nb) (or one table (nb,)).  The specification of the
    device values, as ``flow.reference`` is of the flow fields'.  names: a subset of NAMES (default: those the attributes of m
    allow)."""
    nx = int(m.nx)
    tab = check_table(nx, table)
    if names is None:
        names = [n for n in NAMES if (n != "ke_niw_adv" and hasattr(m, "q")) or (n == "ke_niw_adv" and hasattr(m, "phih"))]
    names = [names] if isinstance(names, str) else list(names)
    bad = [n for n in names if n not in NAMES]
    if bad:
        raise ValueError("coarse.reference: names %r; valid: %s" % (bad, ", ".join(NAMES)))
    kk, ll = np.asarray(m.kk, np.float64), np.asarray(m.ll, np.float64)
    if kk.size != nx:                   # QGModel keeps kx = 0 .. nx/2
        kk = np.concatenate([kk, -kk[1:(nx + 1) // 2][::-1]])
    ik, il = 1j * kk[None, :], 1j * ll[:, None]
    n = np.append(np.arange(0, nx // 2), np.arange(-(nx // 2), 0))
    sh = shell_of(n[None, :], n[:, None])
    F, Fi = np.fft.fft2, np.fft.ifft2
    ph = np.asarray(m.ph)
    # u, v of the products F[u q], F[v q]: as the model's own jacobian_psi_q forms them.  QGModel's irfft2 of the half plane keeps
    # what row ny/2 of -il psi-hat holds, the full plane's real part drops it; no filtered field sees that row (the Nyquist rule)
    if ph.shape[1] == nx:
        P = F(Fi(ph).real)
        u, v = Fi(-il * P).real, Fi(ik * P).real
    else:
        P = _full(ph, nx)
        u, v = np.fft.irfft2(-il * ph, s=(nx, nx)), np.fft.irfft2(ik[:, :nx // 2 + 1] * ph, s=(nx, nx))
    need_q = bool(set(names) & {"ke_qg", "ens"})
    if need_q:
        q = np.array(m.q, np.float64)
        Q, Fu, Fv = F(q), F(u * q), F(v * q)
    if "ke_niw_adv" in names:
        W = np.asarray(m.phih)
        J = F(u * np.asarray(m.phix) + v * np.asarray(m.phiy))
    out = {k: np.empty((len(tab), nx, nx)) for k in names}
    for s, g in enumerate(tab):
        G = g[sh]
        ub, vb = Fi(-il * G * P).real, Fi(ik * G * P).real
        if need_q:
            fu, fv = Fi(G * Fu).real, Fi(G * Fv).real
        if "ke_qg" in names:
            out["ke_qg"][s] = vb * fu - ub * fv
        if "ens" in names:
            qb, qx, qy = Fi(G * Q).real, Fi(ik * G * Q).real, Fi(il * G * Q).real
            out["ens"][s] = qb * (ub * qx + vb * qy) - (fu * qx + fv * qy)
        if "ke_niw_adv" in names:
            wb, wx, wy, jb = Fi(G * W), Fi(ik * G * W), Fi(il * G * W), Fi(G * J)
            out["ke_niw_adv"][s] = (np.conj(wb) * (jb - ub * wx - vb * wy)).real
    return out
