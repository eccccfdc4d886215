"""Spectral transfer and flux spectra, binned on the device.

``spectral_transfer(m)`` says where the nonlinear terms MOVE the quantities whose spectra ``isotropic_spectra`` returns: T_X(b)
is the rate of change of spectrum X in shell b caused by the nonlinear term alone, in the same normalisation as that spectrum,
and the flux through the outer edge of shell b, at k_edge = (b + 1/2) dk, is Pi_X(b) = -sum_{b' <= b} T_X(b').  With F the 2-D
transform on the full plane, M^2 = (nx ny)^2, P = F[psi], Q = F[q], C = F[c], Jq = ik F[u q] + il F[v q],
Jc = ik F[u c] + il F[v c], J = F[u phix + v phiy] and R = i F[phi q_psi] (the tick's wave planes; UnCoupled / YBJ with the
gradients quirk Q1 leaves), summed per shell:

  ke_qg       Re(conj(P) Jq) / M^2              CoupledModel, UnCoupledModel, QGModel
  ens        -Re(conj(Q) Jq) / M^2              CoupledModel, UnCoupledModel, QGModel
  ke_niw_adv -Re(conj(phih) J) / M^2            CoupledModel, UnCoupledModel, YBJModel
  ke_niw_ref -Re(conj(phih) R / 2) / M^2        CoupledModel, UnCoupledModel, YBJModel
  C2         -2 Re(conj(C) Jc) / M^2            QGModel with passive_scalar
  gradC2     -2 wv2 Re(conj(C) Jc) / M^2        QGModel with passive_scalar

YBJModel does not step q: it has no ke_qg or ens transfer.  The wave potential energy needs no rows of its own: its advective
and refractive transfers are isotropic_spectra's ``gamma_a`` and ``gamma_r`` (hslash / f = 1 / kappa2).  In CoupledModel,
``ke_qg`` is the psi-weighted advection of the TOTAL q; the rest of the balanced kinetic-energy tendency, the wave feedback
-Re(conj(P) d/dt F[q_w]), whose total is the tick's conversion terms, is not included.
"""
import numpy as np

from . import _lib
from .spectra import shell_count, shell_modes, _is_qg

KERNEL_NAMES = ("ke_qg", "ens", "ke_niw_adv", "ke_niw_ref")
YBJ_NAMES = ("ke_niw_adv", "ke_niw_ref")
QG_NAMES = ("ke_qg", "ens")
QG_SCALAR_NAMES = ("C2", "gradC2")

# name -> (row of nq_transfer_binned, factor of the raw shell sum before the 1 / M^2)
ROWS = dict(ke_qg=(0, 1.0), ens=(1, -1.0), ke_niw_adv=(2, -1.0), ke_niw_ref=(3, -0.5), C2=(4, -2.0), gradC2=(5, -2.0))


def available(m):
    """names of the transfer spectra spectral_transfer(m) can form for this model"""
    if _is_qg(m):
        return list(QG_NAMES + (QG_SCALAR_NAMES if m.passive_scalar else ()))
    if m.model_id == _lib.YBJ:
        return list(YBJ_NAMES)
    return list(KERNEL_NAMES)


def flux_of(transfer):
    """Pi(b) = -sum_{b' <= b} T(b'): the flux through the outer edge (b + 1/2) dk of shell b"""
    return -np.cumsum(transfer)


class SpectralTransfer(object):
    """shell (0..nb-1), k = shell * dk, k_edge = (shell + 1/2) * dk, dk, modes (full-plane wavenumbers per shell),
    k_iso_max = nx/2 * dk, transfer: {name: T (float64, length nb)} and flux: {name: Pi at k_edge}"""

    def __init__(self, shell, dk, modes, k_iso_max, transfer):
        self.shell = shell
        self.dk = dk
        self.k = shell * dk
        self.k_edge = (shell + 0.5) * dk
        self.modes = modes
        self.k_iso_max = k_iso_max
        self.transfer = transfer
        self.flux = {n: flux_of(t) for n, t in transfer.items()}

    def __repr__(self):
        return "SpectralTransfer(nb=%d, dk=%g, names=%s)" % (len(self.shell), self.dk, sorted(self.transfer))


def spectral_transfer(m, names=None):
    """Transfer spectra of the model's current state, binned on the device; names: a subset of available(m) (default: all).
    Works after set_q / set_phi / set_c, between steps and inside run_with_snapshots; changes nothing a step can see."""
    valid = available(m)
    if names is None:
        names = valid
    else:
        names = [names] if isinstance(names, str) else list(names)
        bad = [n for n in names if n not in valid]
        if bad:
            raise ValueError("spectral_transfer: %s not available for %s; valid names: %s"
                             % (", ".join(map(repr, bad)), type(m).__module__, ", ".join(valid)))
    nb = shell_count(m.nx)
    if getattr(m, "_any_size", False):            # grids without a fused plan: the path's own planes, binned by nq_any_bin
        values = m._transfer(names)
    else:                                         # fused contexts, single-GPU or slab-decomposed (the sum over ranks)
        S = m._ctx.transfer_sums_binned()
        assert S.shape == (_lib.TRANSFER_ROWS, nb), S.shape
        M2 = (float(m.nx) * m.ny) ** 2
        values = {n: ROWS[n][1] * S[ROWS[n][0]] / M2 for n in names}
    return SpectralTransfer(np.arange(nb, dtype=np.int64), float(m.dk), shell_modes(m.nx), 0.5 * m.nx * float(m.dk),
                            {n: values[n] for n in names})
