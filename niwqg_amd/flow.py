"""Velocity, strain, Okubo-Weiss and wave-gradient fields for the PDFs and the averages.

    from niwqg_amd import pdfs, averages
    P = pdfs.field_pdfs(m, names=("q_psi", "ow", "gradphi2"), joint=("ow", "gradphi2"))
    A = averages.attach(m, fields=("strain2", "gradphi2"), products=(("strain2", "gradphi2"),), every=1)

``pdfs.field_pdfs``, ``pdfs.Accumulator`` and ``averages.attach`` take the names below wherever they take a name, mixed freely with
``q``, ``q_psi``, ``phi2`` (and ``phi`` for the averages), on CoupledModel, UnCoupledModel and YBJModel.  A flow name must be asked
for by name: ``pdfs.available`` and the default ``names=None`` are what they were.  A call that names one runs ONE row pass on the
device for all of its names (``k_x_flow_hist`` / ``k_x_flow_moments``): the joint table and the products see values of one pass,
and no physical plane is written or downloaded.

Definitions, with F^-1 the full-plane ``ifft2`` and the model's own ``m.ik``, ``m.il``, psi-hat = ``m.ph``, phi-hat = ``m.phih``:

    u, v       Re F^-1[-il psi-hat], Re F^-1[ik psi-hat]
    sn         normal strain u_x - v_y = 2 u_x,  u_x = Re F^-1[ik (-il psi-hat)]
    ss         shear strain v_x + u_y = 2 v_x - q_psi,  v_x = Re F^-1[ik ik psi-hat],  q_psi the value ``pdfs`` bins
    strain2    sn^2 + ss^2
    ow         strain2 - q_psi^2  (Okubo-Weiss)
    gradphi2   |F^-1[ik phi-hat]|^2 + |F^-1[il phi-hat]|^2, of the CURRENT phi-hat (not UnCoupledModel's stale pair)

Every value is of the last inversion, the state ``q_psi`` and ``phi2`` are binned from: ``set_phi`` after ``set_q`` leaves psi
wave-free until the first step (quirk Q2).

``ss`` is written with q_psi = psi_xx + psi_yy because a y-derivative is not available in mixed space without another column
pass.  It therefore equals psi_xx - psi_yy MINUS the plane mean of q_psi, which psi does not carry.  That mean is the mean of
the q that was set; it is zero for every packaged initial condition.

QGModel: on the any-size path the names without ``gradphi2`` are available with q_psi = q; on the fused grids none is
(DESIGN.md section 7), nor on slab-decomposed models (``NotImplementedError``).  At nx = 8192 every name runs in a launch of
its own: 1-D tables, means and second moments work, a joint table or a product of two different names in a call that has a
flow name raises ``NotImplementedError``.
"""
import numpy as np

from . import _lib

NAMES = ("u", "v", "sn", "ss", "strain2", "ow", "gradphi2")
ONE_VALUE_NX = 8192                 # csrc/nq_flow.hpp: flow_nv: from this fused size on a device thread holds one value
CODES = {"u": _lib.FLOW_U, "v": _lib.FLOW_V, "sn": _lib.FLOW_SN, "ss": _lib.FLOW_SS, "strain2": _lib.FLOW_STRAIN2,
         "ow": _lib.FLOW_OW, "gradphi2": _lib.FLOW_GRADPHI2}


def _is_qg(m):
    from .QGModel import Model as QG
    return isinstance(m, QG)


def available(m):
    """the flow names the PDFs and the averages take for this model, by name only"""
    if _is_qg(m):
        return [n for n in NAMES if n != "gradphi2"] if getattr(m, "_any_size", False) else []
    return list(NAMES)


def refuse(m, what, linked=False):
    """NotImplementedError for the models that have no flow fields yet; ``linked``: the call has a joint table or a product of
    two different names"""
    if _is_qg(m) and not getattr(m, "_any_size", False):
        raise NotImplementedError("%s: QGModel on the fused grids has no flow fields (u, v, strain, ow) yet: its plane route needs a "
                                  "spectral multiply into the download scratch (DESIGN.md section 7); the any-size path has them" % what)
    if not getattr(m, "_any_size", False) and not isinstance(m._ctx, _lib.Context):
        raise NotImplementedError("%s: slab-decomposed models have no flow fields yet (DESIGN.md section 7); use a single-GPU model" % what)
    if linked and not getattr(m, "_any_size", False) and m.nx >= ONE_VALUE_NX:
        raise NotImplementedError("%s: no joint table and no product of two different names with flow fields at nx = %d yet: a "
                                  "device thread of that row plan holds one value, so every name gets a launch of its own "
                                  "(DESIGN.md section 7); 1-D tables, means and second moments work" % (what, m.nx))


def _psi_hat(m):
    ph = np.asarray(m.ph)
    if ph.shape[1] == m.nx:
        return ph
    # QGModel keeps the half plane of a real psi: the full plane by Hermitian symmetry
    n = m.nx
    full = np.empty((n, n), complex)
    full[:, :n // 2 + 1] = ph
    full[:, n // 2 + 1:] = np.conj(np.roll(ph[::-1, 1:(n + 1) // 2], 1, axis=0))[:, ::-1]
    return full


def reference(m, names=NAMES):
    """THE definitions in numpy, from the public reads ``m.ph``, ``m.phih``, ``m.q_psi`` (QGModel: ``m.q``): a dict of (ny, nx)
    float64 planes.  The specification of the device values, as ``pdfs.bin_index`` and ``averages.accumulate`` are of theirs."""
    names = [names] if isinstance(names, str) else list(names)
    bad = [n for n in names if n not in NAMES]
    if bad:
        raise ValueError("flow.reference: names %r; valid: %s" % (bad, ", ".join(NAMES)))
    out, need = {}, set(names)
    n = m.nx
    kk, ll = np.asarray(m.kk, np.float64), np.asarray(m.ll, np.float64)
    if kk.size != n:                    # QGModel keeps kx = 0 .. nx/2
        kk = np.concatenate([kk, -kk[1:(n + 1) // 2][::-1]])
    ik, il = 1j * kk[None, :] * np.ones((n, 1)), 1j * ll[:, None] * np.ones((1, n))
    if need - {"gradphi2"}:
        ph = _psi_hat(m)
        uh = -il * ph
        if "u" in need:
            out["u"] = np.fft.ifft2(uh).real
        if "v" in need:
            out["v"] = np.fft.ifft2(ik * ph).real
        if need & {"sn", "ss", "strain2", "ow"}:
            q_psi = np.array(m.q if _is_qg(m) else m.q_psi, np.float64)
            sn = 2.0 * np.fft.ifft2(ik * uh).real
            ss = 2.0 * np.fft.ifft2(ik * (ik * ph)).real - q_psi
            strain2 = sn * sn + ss * ss
            out.update({k: v for k, v in (("sn", sn), ("ss", ss), ("strain2", strain2), ("ow", strain2 - q_psi * q_psi)) if k in need})
    if "gradphi2" in need:
        phih = np.asarray(m.phih)
        out["gradphi2"] = np.abs(np.fft.ifft2(ik * phih)) ** 2 + np.abs(np.fft.ifft2(il * phih)) ** 2
    return out
