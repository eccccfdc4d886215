"""Isotropic spectra of the diagnostics tick, binned on the device.

``isotropic_spectra(m)`` resolves the registry's spectral scalars by wavenumber shell: the device adds the exact per-wavenumber
term of every tick sum into its isotropic shell (``nq_diagnostics_binned``), and the named spectra are the scalars' own
formulas (``Kernel._calc_*``, ``QGModel._calc_*``) applied shell by shell.  Summed over the shells, each spectrum is the scalar
the tick records, up to summation order.  Nothing but the (32, nb) shell sums leaves the GPU, and the call changes nothing a
later step or call can see.

Shells: the wavenumber (l, k) with integer indices i = kx / dk, j = ly / dk lies in shell b = the integer nearest
sqrt(i^2 + j^2), i.e. the unique b >= 0 with (2b - 1)^2 <= 4 (i^2 + j^2) < (2b + 1)^2 (b = 0 holds the mean only) -- integers
only, no ties.  An nx x nx grid has nb = round(nx / sqrt 2) + 1 shells; those with b <= nx/2 (k <= ``k_iso_max``) lie wholly
inside the square of resolved wavenumbers, the outer ones are cut by it.

One deliberate difference from the scalars: where UnCoupledModel / YBJModel form ``ep_phi`` and ``chi_phi`` with the mean of
phix, phiy as a status line last refreshed them (quirk Q1), the spectra use the current phi-hat.  Spectra describe the state.
"""
import functools

import numpy as np

from . import _lib

KERNEL_NAMES = ("ke_qg", "ens", "ke_niw", "pe_niw", "ep_phi", "ep_psi", "chi_q", "chi_phi", "gamma_r", "gamma_a", "xi_r", "xi_a")
QG_NAMES = ("ke_qg", "ens", "ep_psi", "chi_q")
QG_SCALAR_NAMES = ("C2", "gradC2", "ep_c", "chi_c")


def isqrt(v):
    """floor(sqrt(v)) of non-negative integers, elementwise, exactly"""
    v = np.asarray(v, dtype=np.int64)
    r = np.sqrt(v.astype(np.float64)).astype(np.int64)
    r -= (r * r > v)
    r += ((r + 1) * (r + 1) <= v)
    return r


def shell_of(i, j):
    """isotropic shell of the integer wavenumber indices (i, j): (isqrt(4 (i^2 + j^2)) + 1) // 2"""
    i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    return (isqrt(4 * (i * i + j * j)) + 1) // 2


def shell_count(nx):
    """number of shells of an nx x nx grid: the corner i = j = nx/2 lies in shell round(nx / sqrt 2)"""
    return int(shell_of(nx // 2, nx // 2)) + 1


@functools.lru_cache(maxsize=8)
def _modes(nx):
    n = np.append(np.arange(0, nx // 2), np.arange(-(nx // 2), 0))
    counts = np.zeros(shell_count(nx), dtype=np.int64)
    for r0 in range(0, nx, 512):                     # row blocks: bounded host memory at large nx
        counts += np.bincount(shell_of(n[None, :], n[r0:r0 + 512, None]).ravel(), minlength=len(counts))
    counts.setflags(write=False)
    return counts


def shell_modes(nx):
    """how many wavenumbers of the full nx x nx plane each shell holds (host integers; computed once per nx)"""
    return _modes(int(nx)).copy()


def _is_qg(m):
    from .QGModel import Model as QG
    return isinstance(m, QG)


def available(m):
    """names of the spectra isotropic_spectra(m) can form for this model"""
    if _is_qg(m):
        return list(QG_NAMES + (QG_SCALAR_NAMES if m.passive_scalar else ()))
    return list(KERNEL_NAMES)


class IsotropicSpectra(object):
    """shell (0..nb-1), k = shell * dk, dk, modes (full-plane wavenumbers per shell), k_iso_max = nx/2 * dk, and
    values: {name: float64 array of length nb}"""

    def __init__(self, shell, dk, modes, k_iso_max, values):
        self.shell = shell
        self.dk = dk
        self.k = shell * dk
        self.modes = modes
        self.k_iso_max = k_iso_max
        self.values = values

    def __repr__(self):
        return "IsotropicSpectra(nb=%d, dk=%g, names=%s)" % (len(self.shell), self.dk, sorted(self.values))


def _named(m, S, names):
    """the registry's formulas with every raw sum s[i] replaced by the shell sums S[i]"""
    M2 = (float(m.nx) * m.ny) ** 2
    out = {}
    if _is_qg(m):
        for name in names:
            if name == "ke_qg":
                out[name] = 0.5 * S[11] / M2
            elif name == "ens":
                out[name] = 0.5 * S[6] / M2
            elif name == "ep_psi":
                out[name] = (m.nu4 * S[12] + m.nu * S[13] + m.mu * S[14]) / M2
            elif name == "chi_q":
                out[name] = -m.nu4 * S[7] / M2
            elif name == "C2":
                out[name] = S[16] / M2
            elif name == "gradC2":
                out[name] = S[17] / M2
            elif name == "ep_c":              # nu, not nuc, multiplies gradC2 (QGModel._calc_ep_c)
                out[name] = -2 * m.nu4c * S[18] / M2 - 2 * m.nu * S[17] / M2 - 2 * m.muc * S[16] / M2
            elif name == "chi_c":
                out[name] = -2 * m.nu4c * S[19] / M2 - 2 * m.nu * S[18] / M2 - 2 * m.muc * S[17] / M2
        return out
    M2f = M2 * m.f
    grad2 = S[1] / M2                         # of the current phi-hat (the scalars may use stale gradients: quirk Q1)
    for name in names:
        if name == "ke_qg":
            out[name] = 0.5 * S[11] / M2
        elif name == "ens":
            out[name] = 0.5 * S[6] / M2
        elif name == "ke_niw":
            out[name] = 0.5 * S[0] / M2
        elif name == "pe_niw":
            out[name] = 0.25 * S[1] / M2 / m.kappa2
        elif name == "ep_phi":
            out[name] = (-m.nu4w * S[2] - m.muw * S[0]) / M2 - m.nuw * grad2
        elif name == "ep_psi":
            if m.model_id == _lib.YBJ:        # the reference's p stays zero there (YBJModel._calc_ep_psi)
                out[name] = m.nu4 * S[12] / M2
            else:
                out[name] = (m.nu4 * S[12] + m.nu * S[13] + m.mu * S[14]) / M2
        elif name == "chi_q":
            out[name] = -m.nu4 * S[7] / M2
        elif name == "chi_phi":
            out[name] = ((-0.5 * m.nuw * S[2] - 0.5 * m.nu4w * S[3]) / M2 - 0.5 * m.muw * grad2) / m.kappa2
        elif name == "gamma_r":
            out[name] = 0.25 * m.hslash * S[28] / M2f
        elif name == "gamma_a":
            out[name] = 0.5 * m.hslash * S[24] / M2f
        elif name == "xi_r":
            out[name] = S[27] / M2f
        elif name == "xi_a":
            out[name] = 0.5 * S[31] / M2f
    return out


def isotropic_spectra(m, names=None):
    """Isotropic spectra of the model's current state, binned on the device; names: a subset of available(m) (default: all).
    Works after set_q / set_phi / set_c, between steps and inside run_with_snapshots; changes nothing a step can see."""
    valid = available(m)
    if names is None:
        names = valid
    else:
        names = [names] if isinstance(names, str) else list(names)
        bad = [n for n in names if n not in valid]
        if bad:
            raise ValueError("isotropic_spectra: %s not available for %s; valid names: %s"
                             % (", ".join(map(repr, bad)), type(m).__module__, ", ".join(valid)))
    nb = shell_count(m.nx)
    if getattr(m, "_any_size", False):            # grids without a fused plan: the path's own planes, binned by nq_any_bin
        values = m._spectra(names)
    else:                                         # fused contexts, single-GPU or slab-decomposed (the sum over ranks)
        S = m._ctx.diagnostic_sums_binned()
        assert S.shape == (32, nb), S.shape
        values = _named(m, S, names)
    return IsotropicSpectra(np.arange(nb, dtype=np.int64), float(m.dk), shell_modes(m.nx), 0.5 * m.nx * float(m.dk),
                            {n: values[n] for n in names})
