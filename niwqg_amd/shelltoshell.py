"""Shell-to-shell (giver-receiver) transfers of enstrophy and wave kinetic energy, formed on the device.

    from niwqg_amd import shelltoshell
    R = shelltoshell.shell_to_shell(m, edges=[0, 1, 2, 4, 8, 16, 32, 64])
    R.rows["ens"]        # (nbands, nb): T(b | Q), donor band first
    R.matrix("ens")      # (nbands, nbands): [receiver band K, donor band Q]

``transfer.spectral_transfer`` says where in wavenumber the nonlinear terms move energy and enstrophy, ``coarse.flux_maps`` where
in the domain they cross a scale; neither says WHICH DONOR scales feed a receiving shell.  T(b | Q) is the transfer into shell b
with the ADVECTED field restricted to a donor band Q.  g_Q is a real table per shell (the shell rule of ``spectra.shell_of``, zero
on the shells >= nx/2: coarse's Nyquist rule), G_Q(l, k) = g_Q[shell], and the state is the one ``spectral_transfer(m)`` sees:
P = psi-hat, Q-hat = the q-hat the tick bins (dual-q models: the mean of the two copies), W = the CURRENT phi-hat, u, v and q_psi
those of the tick's products pass.  With F the transform on the full plane and M^2 = (nx ny)^2,

    q^Q = Re F^-1[G_Q Q-hat]        phi^Q = F^-1[G_Q W], gradients F^-1[ik G_Q W], F^-1[il G_Q W]  (CURRENT, on every model)
    Jq^Q = ik F[u q^Q] + il F[v q^Q]        J^Q = F[u phi^Q_x + v phi^Q_y]        R^Q = i F[phi^Q q_psi]

    ens         -sum_b Re(conj(Q-hat) Jq^Q) / M^2       CoupledModel, UnCoupledModel, QGModel
    ke_qg        sum_b Re(conj(P) Jq^Q) / M^2           CoupledModel, UnCoupledModel, QGModel
    ke_niw_adv  -sum_b Re(conj(W) J^Q) / M^2            CoupledModel, UnCoupledModel, YBJModel
    ke_niw_ref  -sum_b Re(conj(W) R^Q / 2) / M^2        CoupledModel, UnCoupledModel, YBJModel

in ``spectral_transfer``'s signs and normalisation; positive: shell b gains from band Q.  The band-to-band matrix is
M[K, Q] = sum_b g_K[b] T(b | Q).

Identities (numpy restatement on 64^2 .. 256^2, relative to sum |T(b | Q)|):

* closure: if sum_Q g_Q[b] = 1 on every shell below nx/2 and the state has nothing on the shells >= nx/2, then
  sum_Q T(b | Q) = spectral_transfer(m).transfer[name][b] for every name and shell (each J is linear in the filtered field).  For
  ``ke_niw_adv`` on UnCoupledModel and YBJModel only while the model's stored gradients are current, i.e. right after set_phi
  (quirk Q1 makes the tick's J stale after a step).
* ``ke_niw_ref`` is antisymmetric, M[K, Q] = -M[Q, K] with a zero diagonal, for ANY state: Re(i z q) is odd under z -> conj(z).
* ``ens`` and ``ke_niw_adv`` are antisymmetric while the top shell of u, v plus twice the top shell of the advected field is
  below nx (the triple product is then alias-free).
* ``ke_qg`` is the donor-resolved psi-weighted PV advection: it closes on T(b) but is NOT antisymmetric, because receiver (psi)
  and donor (q) are different fields.  The velocity-form kinetic-energy shell-to-shell transfer is not formed.

Fused single-GPU grids 64 .. 4096; slab-decomposed models, the any-size path and nx = 8192 raise ``NotImplementedError``
(DESIGN.md section 7).
"""
import numpy as np

from . import _lib
from .coarse import check_table as _check_table
from .spectra import shell_count, shell_of, _is_qg

NAMES = ("ke_qg", "ens", "ke_niw_adv", "ke_niw_ref")
BITS = {"ke_qg": _lib.S2S_Q, "ens": _lib.S2S_Q, "ke_niw_adv": _lib.S2S_ADV, "ke_niw_ref": _lib.S2S_REF}
# name -> (row of nq_shell_transfer, factor of the raw shell sum before the 1 / M^2): transfer.ROWS' first four
ROWS = dict(ke_qg=(0, 1.0), ens=(1, -1.0), ke_niw_adv=(2, -1.0), ke_niw_ref=(3, -0.5))
MAX_BANDS = _lib.S2S_MAX_BANDS
REFUSED_NX = 8192                   # csrc/nq_s2s.hpp: the row kernel of that size spills, even with one row per launch


def available(m):
    """the names shell_to_shell(m) can form for this model"""
    if _is_qg(m):
        return ["ke_qg", "ens"]
    if getattr(m, "model_id", None) == _lib.YBJ:
        return ["ke_niw_adv", "ke_niw_ref"]
    return list(NAMES)


def check_edges(nx, edges):
    """int64 array of band edges e_0 < ... < e_S <= nx/2, 1 <= S <= MAX_BANDS"""
    try:
        e = np.asarray(edges, dtype=np.float64).ravel()
    except (TypeError, ValueError):
        e = np.array([np.nan])
    ok = (np.ndim(edges) == 1 and 2 <= e.size <= MAX_BANDS + 1 and np.isfinite(e).all() and (e == np.round(e)).all()
          and e[0] >= 0 and e[-1] <= nx // 2 and (np.diff(e) > 0).all())
    if not ok:
        raise ValueError("shelltoshell: edges %r; valid: increasing integer shells 0 <= e_0 < ... < e_S <= nx/2 = %d with "
                         "1 <= S <= %d bands" % (edges, nx // 2, MAX_BANDS))
    return e.astype(np.int64)


def bands(m, edges):
    """the tables (nbands, nb) of the sharp bands with the given edges: band i is 1 on the shells e_i <= b < e_(i+1), 0 elsewhere"""
    nx = int(m.nx)
    e = check_edges(nx, edges)
    b = np.arange(shell_count(nx))
    return np.ascontiguousarray(((b[None, :] >= e[:-1, None]) & (b[None, :] < e[1:, None])).astype(np.float64))


def check_table(nx, table):
    """(nbands, nb) float64 of a table argument: coarse.check_table's contract (finite, zero from shell nx/2 on: the Nyquist
    rule), with the band count of nq_shell_transfer"""
    try:
        return _check_table(nx, table)
    except ValueError as e:
        raise ValueError(str(e).replace("coarse:", "shelltoshell:").replace("nscales", "nbands")) from None


def _names(m, names, what):
    valid = available(m)
    if names is None:
        return valid
    names = [names] if isinstance(names, str) else list(names)
    bad = [n for n in names if n not in valid]
    if bad or not names or len(set(names)) != len(names):
        raise ValueError("%s: names %r not available for %s (each once, at least one); valid names: %s"
                         % (what, bad or names, type(m).__module__, ", ".join(valid)))
    return [n for n in NAMES if n in names]


def _tables(m, edges, table, what):
    if (edges is None) == (table is None):
        raise ValueError("%s: give edges or table=, not both and not neither; valid: one of them" % what)
    if table is not None:
        return check_table(int(m.nx), table), None
    return bands(m, edges), check_edges(int(m.nx), edges)


def refuse(m, what="shelltoshell.shell_to_shell"):
    """NotImplementedError for the models and grids that have no shell-to-shell transfers yet"""
    if getattr(m, "_any_size", False):
        raise NotImplementedError("%s: the any-size path (nx = %d has no fused plan) has no shell-to-shell transfers yet "
                                  "(DESIGN.md section 7); use a power of two from 64 to 4096" % (what, m.nx))
    if not isinstance(m._ctx, _lib.Context):
        raise NotImplementedError("%s: slab-decomposed models have no shell-to-shell transfers yet (DESIGN.md section 7); use a "
                                  "single-GPU model" % what)
    if m.nx >= REFUSED_NX:
        raise NotImplementedError("%s: no shell-to-shell transfers at nx = %d yet: a device thread of that row plan has 128 "
                                  "registers and the row kernel spills (DESIGN.md section 7)" % (what, m.nx))


class ShellToShell(object):
    """names; table (nbands, nb); edges (nbands + 1 shells) and k_edges = edges * dk for sharp bands (else None); rows: {name:
    float64 (nbands, nb)}, T(b | Q) with the donor band first; raw: the device's (nbands, S2S_ROWS, nb) shell sums; matrix(name):
    (nbands, nbands), [receiver band K, donor band Q] = sum_b g_K[b] T(b | Q)"""

    def __init__(self, names, table, edges, dk, M2, raw):
        self.names = tuple(names)
        self.table = table
        self.edges = edges
        self.dk = dk
        self.k_edges = None if edges is None else edges * dk
        self.raw = raw
        self.rows = {n: ROWS[n][1] * raw[:, ROWS[n][0], :] / M2 for n in names}

    def matrix(self, name):
        return self.table @ self.rows[name].T

    def __repr__(self):
        return "ShellToShell(names=%s, nbands=%d)" % (list(self.names), len(self.table))


def shell_to_shell(m, edges=None, names=None, table=None):
    """Shell-to-shell transfers of the model's current state.  edges: increasing integer shells e_0 < ... < e_S <= nx/2, band i
    holds e_i <= b < e_(i+1); or table=: an explicit (nbands, nb) array, zero from shell nx/2 on (overlapping smooth bands are
    fine; closure needs them to sum to one below nx/2).  names: a subset of available(m) (default: all).  1 to 64 bands per
    call.  Works after set_q / set_phi, between steps and inside run_with_snapshots; changes nothing a step can see, and nothing
    but the (nbands, 4, nb) table leaves the GPU."""
    what = "shelltoshell.shell_to_shell"
    names = _names(m, names, what)
    tab, e = _tables(m, edges, table, what)
    refuse(m, what)
    mask = 0
    for n in names:
        mask |= BITS[n]
    raw = m._ctx.shell_transfer(mask, tab)
    return ShellToShell(names, tab, e, float(m.dk), (float(m.nx) * m.nx) ** 2, raw)


def reference(m, table, names=None):
    """THE definitions in numpy, from the public reads ``m.ph``, ``m.q``, ``m.phih`` and ``m.q_psi``: {name: float64 (nbands, nb)}
    for the tables (nbands, nb) (or one table (nb,)).  The specification of the device rows.  names: a subset of NAMES (default:
    those the attributes of m allow).  u, v are formed from psi-hat as ``coarse.reference`` forms them (QGModel's half plane:
    irfft2, which keeps row ny/2)."""
    nx = int(m.nx)
    tab = check_table(nx, table)
    if names is None:
        names = [n for n in NAMES if (n in ("ke_qg", "ens") and hasattr(m, "q")) or (n == "ke_niw_adv" and hasattr(m, "phih"))
                 or (n == "ke_niw_ref" and hasattr(m, "phih") and hasattr(m, "q_psi"))]
    names = [names] if isinstance(names, str) else list(names)
    bad = [n for n in names if n not in NAMES]
    if bad:
        raise ValueError("shelltoshell.reference: names %r; valid: %s" % (bad, ", ".join(NAMES)))
    kk, ll = np.asarray(m.kk, np.float64), np.asarray(m.ll, np.float64)
    if kk.size != nx:                   # QGModel keeps kx = 0 .. nx/2
        kk = np.concatenate([kk, -kk[1:(nx + 1) // 2][::-1]])
    ik, il = 1j * kk[None, :], 1j * ll[:, None]
    n = np.append(np.arange(0, nx // 2), np.arange(-(nx // 2), 0))
    sh = shell_of(n[None, :], n[:, None])
    nb, M2 = shell_count(nx), float(nx) ** 4
    F, Fi = np.fft.fft2, np.fft.ifft2
    ph = np.asarray(m.ph)
    if ph.shape[1] == nx:
        P = F(Fi(ph).real)
        u, v = Fi(-il * P).real, Fi(ik * P).real
    else:
        P = F(np.fft.irfft2(ph, s=(nx, nx)))
        u, v = np.fft.irfft2(-il * ph, s=(nx, nx)), np.fft.irfft2(ik[:, :nx // 2 + 1] * ph, s=(nx, nx))

    def binned(x):
        return np.bincount(sh.ravel(), weights=np.ravel(x), minlength=nb)
    need_q = bool(set(names) & {"ke_qg", "ens"})
    if need_q:
        Q = F(np.array(m.q, np.float64))
    if set(names) & {"ke_niw_adv", "ke_niw_ref"}:
        W = np.asarray(m.phih)
    if "ke_niw_ref" in names:
        zeta = np.array(m.q_psi, np.float64)
    out = {k: np.empty((len(tab), nb)) for k in names}
    for s, g in enumerate(tab):
        G = g[sh]
        if need_q:
            qQ = Fi(G * Q).real
            Jq = ik * F(u * qQ) + il * F(v * qQ)
            if "ke_qg" in names:
                out["ke_qg"][s] = binned((np.conj(P) * Jq).real) / M2
            if "ens" in names:
                out["ens"][s] = -binned((np.conj(Q) * Jq).real) / M2
        if "ke_niw_adv" in names:
            J = F(u * Fi(ik * G * W) + v * Fi(il * G * W))
            out["ke_niw_adv"][s] = -binned((np.conj(W) * J).real) / M2
        if "ke_niw_ref" in names:
            R = 1j * F(Fi(G * W) * zeta)
            out["ke_niw_ref"][s] = -0.5 * binned((np.conj(W) * R).real) / M2
    return out
