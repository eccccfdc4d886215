"""ctypes binding of libniwqg_amd.so (C ABI: include/niwqg_amd.h).

The library is built in-tree by ``build()`` (hipcc, gfx950) and loaded from this directory.  There is
no CPU fallback: if the library is missing or no GPU is present, constructing a model raises.
"""
import ctypes
import glob
import os
import re
import subprocess

import numpy as np

from . import _abi, _etdrk4

try:                      # torch bundles its own libamdhip64.so.7; load it first so that our library
    import torch          # binds to the same HIP runtime instance (one runtime per process)
except Exception:         # pragma: no cover - torch is optional for single-GPU use
    torch = None

HERE = os.path.dirname(os.path.abspath(__file__))
# NIWQG_AMD_LIB: another build of the same sources (A/B experiments with compile-time knobs, tools/); default: the in-tree library
LIB_PATH = os.environ.get("NIWQG_AMD_LIB") or os.path.join(HERE, "libniwqg_amd.so")
SRC = os.path.join(HERE, "csrc", "nq_lib.hip")
HEADER = os.path.join(os.path.dirname(HERE), "include", "niwqg_amd.h")
HEADERS = sorted(glob.glob(os.path.join(HERE, "csrc", "*.hpp"))) + [HEADER]

# The header is the one statement of the C ABI: the entry points with their signatures, every NQ_X constant (here: X) and struct
# nq_params are read from it.  A new entry point is declared there and defined in the library; nothing here lists it.
PROTOTYPES, _CONSTANTS, _PARAMS_FIELDS = _abi.read(open(HEADER).read())
EXPORTS = [name for name, _, _ in PROTOTYPES]
globals().update({name[3:]: value for name, value in _CONSTANTS.items()})
COUPLED, UNCOUPLED, QG, YBJ = MODEL_COUPLED, MODEL_UNCOUPLED, MODEL_QG, MODEL_YBJ        # noqa: F821

FUSED_SIZES = (64, 128, 256, 512, 1024, 2048, 4096, 8192)       # grids the fused ETDRK4 kernels have a plan for (csrc: NQ_FOR_SIZES)


def has_fused_plan(nx):
    return nx in FUSED_SIZES


EXCHANGE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int)
ALLREDUCE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int)


# C spelling (const dropped) -> ctypes; a spelling the header starts to use and this table lacks fails lib() (TypeError)
_CTYPES = {"int": ctypes.c_int, "double": ctypes.c_double, "float": ctypes.c_float, "long long": ctypes.c_longlong,
           "unsigned long long": ctypes.c_ulonglong}


class Params(ctypes.Structure):
    _fields_ = [(name, _CTYPES[c_type]) for name, c_type in _PARAMS_FIELDS]


_CTYPES.update({c_type + "*": ctypes.POINTER(t) for c_type, t in list(_CTYPES.items())})
_CTYPES.update({"char*": ctypes.c_char_p, "nq_params*": ctypes.POINTER(Params), "nq_exchange_fn": EXCHANGE_FN, "nq_allreduce_fn": ALLREDUCE_FN})
for _opaque in ("void", "nq_ctx", "nq_any"):
    _CTYPES.update({_opaque + "*": ctypes.c_void_p, _opaque + "**": ctypes.POINTER(ctypes.c_void_p)})


def signature(prototype):
    """(argtypes, restype) of one prototype of the header"""
    def ctype(c_type, what):
        try:
            return _CTYPES[_abi.spelling(re.sub(r"\bconst\b", " ", c_type))]
        except KeyError:
            raise TypeError("%s: no ctypes type for %s of C type '%s' (niwqg_amd/_lib.py: _CTYPES)" % (name, what, c_type)) from None
    name, ret, params = prototype
    return [ctype(c_type, "parameter '%s'" % pname) for c_type, pname in params], ctype(ret, "the return value")


def needs_build():
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    return any(os.path.getmtime(p) > t for p in [SRC] + HEADERS)


def build(force=False, verbose=False):
    """Compile the HIP library for gfx950 (cross-compiles without a GPU)."""
    if not force and not needs_build():
        return LIB_PATH
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", "-Wno-unused-value",
           SRC, "-o", LIB_PATH]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return LIB_PATH


_lib = None


def lib():
    """Load (once) and type the shared library."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("niwqg_amd: %s is missing - run niwqg_amd._lib.build() (hipcc, gfx950); "
                           "there is no CPU fallback" % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH)
    for prototype in PROTOTYPES:
        try:
            fn = getattr(L, prototype[0])
        except AttributeError:
            raise RuntimeError("niwqg_amd: %s does not export %s, which %s declares (a stale build, or a library of other "
                               "sources)" % (LIB_PATH, prototype[0], HEADER)) from None
        fn.argtypes, fn.restype = signature(prototype)
    _lib = L
    return L


def _dptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _iptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def coeff_near_contour(L, h, eq, delta):
    """(l, k) index arrays (k global) of the entries of equation eq within delta of the ETDRK4 contour (nq_coeff_near_contour)"""
    cap = 1 << 16
    while True:
        li, ki = np.empty(cap, np.int32), np.empty(cap, np.int32)
        n = L.nq_coeff_near_contour(h, eq, float(delta), cap, _iptr(li), _iptr(ki))
        if n < 0:
            raise RuntimeError("nq_coeff_near_contour failed (%d): %s" % (n, L.nq_last_error(h).decode()))
        if n <= cap:
            return li[:n].astype(np.int64), ki[:n].astype(np.int64)
        cap = n


def coeff_patch(L, h, eq, li, ki, vals):
    li, ki = np.ascontiguousarray(li, np.int32), np.ascontiguousarray(ki, np.int32)
    vals = np.ascontiguousarray(vals, np.complex128)
    if vals.shape != (len(li), 4) or len(ki) != len(li):
        raise ValueError("coeff_patch: %d entries, values of shape %s" % (len(li), vals.shape))
    rc = L.nq_coeff_patch(h, eq, len(li), _iptr(li), _iptr(ki), _dptr(vals.view(np.float64)))
    if rc != 0:
        raise RuntimeError("nq_coeff_patch failed (%d): %s" % (rc, L.nq_last_error(h).decode()))


class Context:
    """Thin object wrapper over nq_ctx; all arrays in and out are numpy."""

    def __init__(self, model, nx, kk, ll, filtr, dt, U=0.0, f=1e-4, kappa2=1.0, nu=0.0, nu4=0.0, mu=0.0,
                 nuw=0.0, nu4w=0.0, muw=0.0, beta=0.0, budgets=True, device=0, dual_q=False, passive_scalar=False,
                 nu4c=0.0, nuc=0.0, muc=0.0):
        self.L = lib()
        self.model, self.nx = model, int(nx)
        self.nk = nx if model != QG else nx // 2 + 1
        self.dual_q = bool(dual_q) and model != QG
        p = Params(model=model, nx=nx, budgets=int(bool(budgets)), dual_q=int(self.dual_q), dt=dt, U=U, f=f, kappa2=kappa2,
                   nu=nu, nu4=nu4, mu=mu, nuw=nuw, nu4w=nu4w, muw=muw, beta=beta,
                   passive_scalar=int(bool(passive_scalar) and model == QG), nu4c=nu4c, nuc=nuc, muc=muc)
        kk = np.ascontiguousarray(kk, dtype=np.float64)
        ll = np.ascontiguousarray(ll, dtype=np.float64)
        filtr = np.ascontiguousarray(filtr, dtype=np.float64)
        if kk.shape != (self.nk,) or ll.shape != (nx,) or filtr.shape != (nx, self.nk):
            raise ValueError("kk %s, ll %s, filtr %s do not fit nx = %d (nk = %d)" % (kk.shape, ll.shape, filtr.shape, nx, self.nk))
        # roots of unity of the ETDRK4 contour mean, built exactly like the reference (Kernel.py:424-426)
        r = np.exp(2j * np.pi * (np.arange(1.0, 33.0) / 32.0))
        r = np.ascontiguousarray(r).view(np.float64)
        h = ctypes.c_void_p()
        rc = self.L.nq_create(ctypes.byref(p), _dptr(kk), _dptr(ll), _dptr(filtr), _dptr(r), device, ctypes.byref(h))
        if rc != 0:
            raise RuntimeError("nq_create failed (%d): %s" % (rc, self.L.nq_last_error(None).decode()))
        self.h = h
        self.budgets_enabled = bool(budgets)
        # the entries of Qh, f0, fab, fc next to the contour, recomputed as the reference computes them (_etdrk4.py)
        prm = dict(U=U, f=f, kappa2=kappa2, nu=nu, nu4=nu4, mu=mu, nuw=nuw, nu4w=nu4w, muw=muw, beta=beta, nu4c=nu4c, nuc=nuc, muc=muc)
        eqs = [0] + ([1] if model != QG else []) + ([2] if p.passive_scalar else [])
        self.contour_patched = _etdrk4.patch_near_contour(
            lambda eq, delta: coeff_near_contour(self.L, self.h, eq, delta), lambda eq, li, ki, v: coeff_patch(self.L, self.h, eq, li, ki, v),
            model, self.nx, kk, ll, filtr, dt, prm, eqs)

    def take_budget_increments(self):
        """Ke, Pw, Kw increments accumulated on the device since the last call (Kernel.py:390-392)."""
        return tuple(self.scalar(s) for s in (S_KE, S_PW, S_KW))

    def _chk(self, rc, what):
        if rc != 0:
            raise RuntimeError("%s failed (%d): %s" % (what, rc, self.L.nq_last_error(self.h).decode()))

    def close(self):
        if getattr(self, "h", None):
            self.L.nq_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- state
    @staticmethod
    def _shape(a, shape, what):
        """the C ABI takes plain pointers: a host array of the wrong size must never reach it"""
        if a.shape != tuple(shape):
            raise ValueError("%s: array of shape %s, expected %s" % (what, a.shape, tuple(shape)))

    def set_q(self, q):
        q = np.ascontiguousarray(q, dtype=np.float64)
        self._shape(q, (self.nx, self.nx), "set_q")
        self._chk(self.L.nq_set_q(self.h, _dptr(q)), "nq_set_q")

    def set_c(self, c):
        c = np.ascontiguousarray(c, dtype=np.float64)
        self._shape(c, (self.nx, self.nx), "set_c")
        self._chk(self.L.nq_set_c(self.h, _dptr(c)), "nq_set_c")

    def set_phi(self, phi):
        phi = np.ascontiguousarray(phi, dtype=np.complex128)
        self._shape(phi, (self.nx, self.nx), "set_phi")
        self._chk(self.L.nq_set_phi(self.h, _dptr(phi.view(np.float64))), "nq_set_phi")

    def invert(self):
        self._chk(self.L.nq_invert(self.h), "nq_invert")

    def refresh_grad_phi(self):
        self._chk(self.L.nq_refresh_grad_phi(self.h), "nq_refresh_grad_phi")

    def step(self, n=1):
        self._chk(self.L.nq_step(self.h, int(n)), "nq_step")

    def sync(self):
        self._chk(self.L.nq_sync(self.h), "nq_sync")

    def profile_stride(self, stride):
        """bracket only every stride-th launch of the enabled kernel class(es) (include/niwqg_amd.h: nq_profile_stride)"""
        self._chk(self.L.nq_profile_stride(self.h, int(stride)), "nq_profile_stride")

    def tick_snapshot(self):
        """keep qh, phih, qwh as the diagnostics tick sees them (include/niwqg_amd.h: nq_tick_snapshot)"""
        self._chk(self.L.nq_tick_snapshot(self.h), "nq_tick_snapshot")

    def request_stage4_max(self):
        """the last step of the next step() call also records max |u|, max |v| of its fourth stage (include/niwqg_amd.h)"""
        self._chk(self.L.nq_request_stage4_max(self.h), "nq_request_stage4_max")

    def status_cfl_max(self):
        """max(|u|, |v|) of the fourth stage of the last step (as requested before it) and |phi| of the new state: what the
        reference's status line takes its CFL from after a step without a tick (ref niwqg/Kernel.py:594, :660-662, :364-368)"""
        uv = np.zeros(2)
        self._chk(self.L.nq_get_stage4_max(self.h, _dptr(uv)), "nq_get_stage4_max")
        return float(np.max([uv[0], uv[1], self.scalar(S_MAX_PHI)]))      # (not max(): NaN anywhere must give NaN)

    # --- reads
    _REAL = (F_Q, F_P, F_U, F_V, F_QPSI, F_QW, F_C)
    _HALF = (F_QH, F_PH, F_QWH, F_QH_MINUS, F_CH, F_QH_STAGE4, F_QH_MINUS_STAGE4, F_QH_TICK, F_QH_MINUS_TICK, F_QWH_TICK)

    def field(self, fid):
        n, h = self.nx, self.nx // 2 + 1
        nd = self.L.nq_field_doubles(self.h, fid)           # the library states the size; shapes as in the header
        if nd < 0:
            raise RuntimeError("nq_get_field: unknown field id %d" % fid)
        if fid in self._REAL:
            out = np.empty((n, n), np.float64)
        elif fid in self._HALF:
            out = np.empty((n, h), np.complex128)
        else:
            out = np.empty((n, n), np.complex128)
        if out.view(np.float64).size != nd:
            raise RuntimeError("field %d: the library writes %d doubles, the binding allocated %d" % (fid, nd, out.view(np.float64).size))
        self._chk(self.L.nq_get_field(self.h, fid, _dptr(out.view(np.float64))), "nq_get_field(%d)" % fid)
        return out

    def stream_copy_gbs(self, nbytes=512 << 20, reps=5):
        """GB/s (read + written) of a plain 1r + 1w copy kernel on this device (nq_stream_copy_gbs)"""
        v = ctypes.c_double()
        self._chk(self.L.nq_stream_copy_gbs(self.h, int(nbytes), int(reps), ctypes.byref(v)), "nq_stream_copy_gbs")
        return v.value

    def qh_passenger(self):
        """anti-Hermitian part of the reference's qh on row ny/2, k = 0..nx/2 (include/niwqg_amd.h: nq_get_qh_passenger)"""
        out = np.zeros(self.nx // 2 + 1, np.complex128)
        self._chk(self.L.nq_get_qh_passenger(self.h, _dptr(out.view(np.float64))), "nq_get_qh_passenger")
        return out

    def scalar(self, sid):
        v = ctypes.c_double()
        self._chk(self.L.nq_get_scalar(self.h, sid, ctypes.byref(v)), "nq_get_scalar(%d)" % sid)
        return v.value

    def diagnostic_sums(self):
        """The 32 raw sums of one diagnostics tick (include/niwqg_amd.h: nq_diagnostics); nothing but these 256
        bytes leaves the GPU."""
        out = np.zeros(32)
        self._chk(self.L.nq_diagnostics(self.h, _dptr(out)), "nq_diagnostics")
        return out

    def diagnostic_sums_binned(self):
        """The tick's sums binned into isotropic shells, (32, nb) (include/niwqg_amd.h: nq_diagnostics_binned)"""
        nb = int(self.L.nq_spectrum_shells(self.h))
        out = np.zeros((32, nb))
        self._chk(self.L.nq_diagnostics_binned(self.h, nb, _dptr(out)), "nq_diagnostics_binned")
        return out

    def transfer_sums_binned(self):
        """Raw spectral-transfer shell sums, (TRANSFER_ROWS, nb) (include/niwqg_amd.h: nq_transfer_binned)"""
        nb = int(self.L.nq_spectrum_shells(self.h))
        out = np.zeros((TRANSFER_ROWS, nb))
        self._chk(self.L.nq_transfer_binned(self.h, nb, _dptr(out)), "nq_transfer_binned")
        return out

    def coarse_flux(self, mask, tables, nmaps):
        """(moments (nscales, 3, 2): sum and sum of squares per map, maps (nscales, nmaps, ny, nx) or None when nmaps = 0) of the
        coarse-grained flux maps selected by mask (CG_*) for the filter tables (nscales, nb) (include/niwqg_amd.h: nq_coarse_flux)"""
        tables = np.ascontiguousarray(tables, np.float64)
        self._shape(tables, (tables.shape[0], int(self.L.nq_spectrum_shells(self.h))), "coarse_flux")
        mom = np.zeros((tables.shape[0], 3, 2))
        maps = np.empty((tables.shape[0], nmaps, self.nx, self.nx)) if nmaps else None
        self._chk(self.L.nq_coarse_flux(self.h, int(mask), tables.shape[0], _dptr(tables), tables.shape[1], _dptr(mom),
                                        _dptr(maps) if nmaps else None), "nq_coarse_flux")
        return mom, maps

    def shell_transfer(self, mask, tables):
        """raw shell sums (nbands, S2S_ROWS, nb) of the shell-to-shell transfers selected by mask (S2S_*) for the donor-band tables
        (nbands, nb) (include/niwqg_amd.h: nq_shell_transfer)"""
        tables = np.ascontiguousarray(tables, np.float64)
        self._shape(tables, (tables.shape[0], int(self.L.nq_spectrum_shells(self.h))), "shell_transfer")
        out = np.zeros((tables.shape[0], S2S_ROWS, tables.shape[1]))              # noqa: F821
        self._chk(self.L.nq_shell_transfer(self.h, int(mask), tables.shape[0], _dptr(tables), tables.shape[1], _dptr(out)),
                  "nq_shell_transfer")
        return out

    def cospectra(self, codes, accumulate=False, download=True):
        """raw co-spectrum shell sums (COSPEC_ROWS, nb) of the listed fields (PDF_*, FLOW_*), added to the running sums on the
        device; download=False: nothing comes back and the host does not wait (include/niwqg_amd.h: nq_cospectra)"""
        nb = int(self.L.nq_spectrum_shells(self.h))
        c = (ctypes.c_int * max(1, len(codes)))(*codes)
        out = np.zeros((COSPEC_ROWS, nb)) if download else None                   # noqa: F821
        self._chk(self.L.nq_cospectra(self.h, len(codes), c, nb, int(bool(accumulate)), _dptr(out) if download else None), "nq_cospectra")
        return out

    def cospectra_read(self):
        """(calls in the running sums, the sums (COSPEC_ROWS, nb)) (include/niwqg_amd.h: nq_cospectra_read)"""
        n = ctypes.c_longlong()
        out = np.zeros((COSPEC_ROWS, int(self.L.nq_spectrum_shells(self.h))))     # noqa: F821
        self._chk(self.L.nq_cospectra_read(self.h, ctypes.byref(n), _dptr(out)), "nq_cospectra_read")
        return int(n.value), out

    def coeff(self, eq, which):
        n = self.nx
        w = n if eq == 1 else n // 2 + 1
        out = np.empty((n, w), np.complex128)
        self._chk(self.L.nq_get_coeff(self.h, eq, which, _dptr(out.view(np.float64))), "nq_get_coeff")
        return out

    # --- snapshots (niwqg_amd/Saving.py)
    def snapshot_begin(self, with_phi=True):
        self._chk(self.L.nq_snapshot_begin(self.h, int(bool(with_phi))), "nq_snapshot_begin")

    def snapshot_end(self, with_phi=True):
        n = self.nx
        q = np.empty((n, n), np.float64)
        phi = np.empty((n, n), np.complex128) if with_phi else None
        self._chk(self.L.nq_snapshot_end(self.h, _dptr(q), _dptr(phi.view(np.float64)) if with_phi else None), "nq_snapshot_end")
        return q, phi

    # --- FFT seam
    def _xf(self, fn, a, in_dtype, out_shape, out_dtype, in_shape=None):
        a = np.ascontiguousarray(a, dtype=in_dtype)
        self._shape(a, in_shape or (self.nx, self.nx), fn.__name__)
        out = np.empty(out_shape, out_dtype)
        self._chk(fn(self.h, _dptr(a.view(np.float64)), _dptr(out.view(np.float64))), fn.__name__)
        return out

    def fft2(self, a):
        return self._xf(self.L.nq_fft2, a, np.complex128, (self.nx, self.nx), np.complex128)

    def ifft2(self, a):
        return self._xf(self.L.nq_ifft2, a, np.complex128, (self.nx, self.nx), np.complex128)

    def rfft2(self, a):
        return self._xf(self.L.nq_rfft2, a, np.float64, (self.nx, self.nx // 2 + 1), np.complex128)

    def irfft2(self, a):
        return self._xf(self.L.nq_irfft2, a, np.complex128, (self.nx, self.nx), np.float64, in_shape=(self.nx, self.nx // 2 + 1))

    # --- Jacobians in the reference's layouts (assembled on the device)
    def jacobian_psi_q(self):
        """Kernel family: (ny, nx) with [0,0] = 0 (Kernel.py:471-486); QGModel: (ny, nx/2+1) (QGModel.py:469-481)"""
        out = np.empty((self.nx, self.nx if self.model != QG else self.nx // 2 + 1), np.complex128)
        self._chk(self.L.nq_jacobian_psi_q(self.h, _dptr(out.view(np.float64))), "nq_jacobian_psi_q")
        return out

    def jacobian_psi_c(self):
        """QGModel's passive scalar: ik*fft(u c) + il*fft(v c), (ny, nx/2+1) (QGModel.py:483-495), through the row kernel"""
        out = np.empty((self.nx, self.nx // 2 + 1), np.complex128)
        self._chk(self.L.nq_jacobian_psi_c(self.h, _dptr(out.view(np.float64))), "nq_jacobian_psi_c")
        return out

    def products_uq_vq(self):
        """fft(u q), fft(v q) on k = 0..nx/2"""
        n, h = self.nx, self.nx // 2 + 1
        out = np.empty((2, n, h), np.complex128)
        self._chk(self.L.nq_products_uq_vq(self.h, _dptr(out.view(np.float64))), "nq_products_uq_vq")
        return out[0], out[1]

    def jacobian_psi_phi(self):
        out = np.empty((self.nx, self.nx), np.complex128)
        self._chk(self.L.nq_jacobian_psi_phi(self.h, _dptr(out.view(np.float64))), "nq_jacobian_psi_phi")
        return out

    def refraction(self):
        """fft(phi * q_psi) from the row kernel (Kernel.py:332 without the -0.5j)"""
        out = np.empty((self.nx, self.nx), np.complex128)
        self._chk(self.L.nq_refraction(self.h, _dptr(out.view(np.float64))), "nq_refraction")
        return out

    def jacobian_phic_phi(self):
        out = np.empty((self.nx, self.nx), np.complex128)
        self._chk(self.L.nq_jacobian_phic_phi(self.h, _dptr(out.view(np.float64))), "nq_jacobian_phic_phi")
        return out

    # --- timing
    def timer_start(self):
        self._chk(self.L.nq_timer_start(self.h), "nq_timer_start")

    def timer_stop(self):
        ms = ctypes.c_float()
        self._chk(self.L.nq_timer_stop(self.h, ctypes.byref(ms)), "nq_timer_stop")
        return ms.value

    def event_record(self, slot):
        self._chk(self.L.nq_event_record(self.h, int(slot)), "nq_event_record")

    def event_elapsed(self, a, b):
        ms = ctypes.c_float()
        self._chk(self.L.nq_event_elapsed(self.h, int(a), int(b), ctypes.byref(ms)), "nq_event_elapsed")
        return ms.value

    KERNEL_CLASSES = {"x_products": 0, "x_wavepv": 1, "s_q": 2, "s_phi": 3, "s_invert": 4, "y_A": 5}
    RAY_KERNEL_CLASSES = {"pt_zeta": 6, "pt_rays": 7}       # ray mode's row pass and step: one at a time, profile_read()
    STRETCH_KERNEL_CLASSES = {"pt_tangent": 8}              # stretch mode's step (with or without the wave), likewise

    def profile_enable(self, kernel_class):
        self._chk(self.L.nq_profile_enable(self.h, int(kernel_class)), "nq_profile_enable")

    def profile_read(self):
        n, ms = ctypes.c_int(), ctypes.c_float()
        self._chk(self.L.nq_profile_read(self.h, ctypes.byref(n), ctypes.byref(ms)), "nq_profile_read")
        return n.value, ms.value

    def profile_read_all(self):
        """{class name: (launches, total ms)} after profile_enable(-2)"""
        n, ms = (ctypes.c_int * 6)(), (ctypes.c_float * 6)()
        self._chk(self.L.nq_profile_read_all(self.h, n, ms), "nq_profile_read_all")
        return {name: (n[k], ms[k]) for name, k in self.KERNEL_CLASSES.items()}

    def device_bytes(self):
        return int(self.L.nq_device_bytes(self.h))

    # ---- Lagrangian particles (include/niwqg_amd.h: nq_particles_*; niwqg_amd/particles.py) ----------------------------------
    def particles_attach(self, x, y, Lx, Ly, record_every, capacity, codes):
        x = np.ascontiguousarray(x, np.float64)
        y = np.ascontiguousarray(y, np.float64)
        c = (ctypes.c_int * max(1, len(codes)))(*codes)
        self._chk(self.L.nq_particles_attach(self.h, len(x), _dptr(x), _dptr(y), float(Lx), float(Ly), int(record_every),
                                             int(capacity), len(codes), c), "nq_particles_attach")

    def particles_wave(self, amplitude, f0, t0):
        """drifter mode: right after particles_attach"""
        self._chk(self.L.nq_particles_wave(self.h, float(amplitude), float(f0), float(t0)), "nq_particles_wave")

    def particles_clock(self, f0, t0):
        """the clock of the "uw" / "vw" values without drifter mode"""
        self._chk(self.L.nq_particles_clock(self.h, float(f0), float(t0)), "nq_particles_clock")

    def particles_rays(self, k, l, eta):
        """ray mode: right after particles_attach"""
        k = np.ascontiguousarray(k, np.float64)
        l = np.ascontiguousarray(l, np.float64)
        self._chk(self.L.nq_particles_rays(self.h, _dptr(k), _dptr(l), float(eta)), "nq_particles_rays")

    def particles_get_rays(self, n):
        k, l = np.empty(n), np.empty(n)
        self._chk(self.L.nq_particles_get_rays(self.h, _dptr(k), _dptr(l)), "nq_particles_get_rays")
        return k, l

    def particles_tangent(self, F0=None):
        """stretch mode: right after particles_attach; F0 (4, n) in the order f11, f12, f21, f22, or None: I"""
        if F0 is not None:
            F0 = np.ascontiguousarray(F0, np.float64)
        self._chk(self.L.nq_particles_tangent(self.h, None if F0 is None else _dptr(F0)), "nq_particles_tangent")

    def particles_get_tangent(self, n):
        F = np.empty((4, n))
        self._chk(self.L.nq_particles_get_tangent(self.h, _dptr(F)), "nq_particles_get_tangent")
        return F

    def particles_tangent_reset(self):
        self._chk(self.L.nq_particles_tangent_reset(self.h), "nq_particles_tangent_reset")

    def particles_tangent_step0(self):
        s = ctypes.c_longlong()
        self._chk(self.L.nq_particles_tangent_step0(self.h, ctypes.byref(s)), "nq_particles_tangent_step0")
        return int(s.value)

    def particles_detach(self):
        self._chk(self.L.nq_particles_detach(self.h), "nq_particles_detach")

    def particles_get(self, n):
        x, y = np.empty(n), np.empty(n)
        self._chk(self.L.nq_particles_get(self.h, _dptr(x), _dptr(y)), "nq_particles_get")
        return x, y

    def particles_sample(self, n, codes, ncols):
        out = np.empty((ncols, n))
        c = (ctypes.c_int * max(1, len(codes)))(*codes)
        self._chk(self.L.nq_particles_sample(self.h, len(codes), c, _dptr(out)), "nq_particles_sample")
        return out

    def particles_records(self, n):
        """(steps since attach (m,), records (m, columns, n)) of the records the ring holds, oldest first"""
        info = (ctypes.c_longlong * 4)()
        self._chk(self.L.nq_particles_records(self.h, info, None, None), "nq_particles_records")
        m, w = int(info[1]), int(info[2])
        steps = (ctypes.c_longlong * max(1, m))()
        out = np.empty((m, w, n))
        self._chk(self.L.nq_particles_records(self.h, info, steps, _dptr(out)), "nq_particles_records")
        return np.array(steps[:m], np.int64), out

    def particles_steps(self):
        """steps since attach"""
        info = (ctypes.c_longlong * 4)()
        self._chk(self.L.nq_particles_records(self.h, info, None, None), "nq_particles_records")
        return int(info[3])

    def particles_held(self, steps=False):
        """records the ring holds; steps=True: their steps since attach (m,), oldest first (nothing is downloaded)"""
        info = (ctypes.c_longlong * 4)()
        self._chk(self.L.nq_particles_records(self.h, info, None, None), "nq_particles_records")
        m = int(info[1])
        if not steps:
            return m
        out = (ctypes.c_longlong * max(1, m))()
        self._chk(self.L.nq_particles_records(self.h, info, out, None), "nq_particles_records")
        return np.array(out[:m], np.int64)

    # ---- Lagrangian spectra and dispersion (include/niwqg_amd.h: nq_lagr_*; niwqg_amd/lagrangian.py) ---------------------------
    def lagr_spectrum(self, code, T, F, window, demean, G, order, offsets, chunk):
        """(F, G) sums over each group, row p = FFT bin p"""
        w = np.ascontiguousarray(window, np.float64)
        out = np.empty((F, G))
        self._chk(self.L.nq_lagr_spectrum(self.h, int(code), int(T), int(F), _dptr(w), int(bool(demean)), int(G), _iptr(order), _iptr(offsets),
                                          int(chunk), _dptr(out)), "nq_lagr_spectrum")
        return out

    def lagr_dispersion(self, T, G, order, offsets, pairs):
        """((T, G, 6) sums over each group, (T, 5) sums over the pairs or None)"""
        out = np.empty((T, G, 6))
        npairs = 0 if pairs is None else len(pairs[0])
        outp = np.empty((T, 5)) if npairs else None
        self._chk(self.L.nq_lagr_dispersion(self.h, int(T), int(G), _iptr(order), _iptr(offsets), npairs, _iptr(pairs[0]) if npairs else None,
                                            _iptr(pairs[1]) if npairs else None, _dptr(out), _dptr(outp) if npairs else None),
                  "nq_lagr_dispersion")
        return out, outp

    def lagr_stretching(self, T, G, order, offsets):
        """(T, G, 4) sums over each group of ln sigma_1, its square, det F and its square"""
        out = np.empty((T, G, 4))
        self._chk(self.L.nq_lagr_stretching(self.h, int(T), int(G), _iptr(order), _iptr(offsets), _dptr(out)), "nq_lagr_stretching")
        return out

    # ---- PDFs of the physical fields (include/niwqg_amd.h: nq_field_hist; niwqg_amd/pdfs.py) --------------------------------
    def field_minmax(self, codes):
        """[(min, max)] of the listed fields (PDF_*), exact, from one device pass"""
        out = np.empty((len(codes), 2))
        c = (ctypes.c_int * len(codes))(*codes)
        self._chk(self.L.nq_field_minmax(self.h, len(codes), c, _dptr(out)), "nq_field_minmax")
        return [(float(a), float(b)) for a, b in out]

    def field_hist(self, codes, lo, hi, bins, joint=None, joint_bins=0, accumulate=False):
        """bin the listed fields on the device (nothing comes back: field_hist_read)"""
        c = (ctypes.c_int * len(codes))(*codes)
        lo, hi = np.ascontiguousarray(lo, np.float64), np.ascontiguousarray(hi, np.float64)
        ja, jb = joint if joint is not None else (-1, -1)
        self._chk(self.L.nq_field_hist(self.h, len(codes), c, _dptr(lo), _dptr(hi), int(bins), int(ja), int(jb), int(joint_bins),
                                       int(bool(accumulate))), "nq_field_hist")

    def field_hist_read(self, nfields, bins, joint_bins=0):
        """(counts (nfields, bins + 3) uint64 [bins, below, above, nan], joint (joint_bins^2 + 1,) uint64 or None)"""
        n1 = nfields * (bins + 3)
        out = np.zeros(n1 + (joint_bins * joint_bins + 1 if joint_bins else 0), np.uint64)
        self._chk(self.L.nq_field_hist_read(self.h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong))), "nq_field_hist_read")
        return out[:n1].reshape(nfields, bins + 3), (out[n1:] if joint_bins else None)

    # ---- stochastic forcing (include/niwqg_amd.h: nq_forcing_*; niwqg_amd/forcing.py) ------------------------------------------
    def forcing_attach(self, Aq, Aphi, seed, step0):
        Aq = None if Aq is None else np.ascontiguousarray(Aq, np.float64)
        Aphi = None if Aphi is None else np.ascontiguousarray(Aphi, np.float64)
        self._chk(self.L.nq_forcing_attach(self.h, None if Aq is None else _dptr(Aq), None if Aphi is None else _dptr(Aphi),
                                           int(seed), int(step0)), "nq_forcing_attach")

    def forcing_detach(self):
        self._chk(self.L.nq_forcing_detach(self.h), "nq_forcing_detach")

    def forcing_apply(self):
        self._chk(self.L.nq_forcing_apply(self.h), "nq_forcing_apply")

    def forcing_increment(self, stream, step):
        out = np.empty((self.nx, self.nx // 2 + 1 if stream == 0 else self.nx), np.complex128)
        self._chk(self.L.nq_forcing_increment(self.h, int(stream), int(step), _dptr(out.view(np.float64))), "nq_forcing_increment")
        return out

    def forcing_state(self):
        out = np.empty(3)
        self._chk(self.L.nq_forcing_state(self.h, _dptr(out)), "nq_forcing_state")
        return int(out[0]), float(out[1]), float(out[2])

    # ---- low-mode time series and their frequency spectra (include/niwqg_amd.h: nq_freq_*; niwqg_amd/frequency.py) ---------------
    def freq_attach(self, kmax, every, length, fields):
        f = (ctypes.c_int * len(fields))(*fields)
        self._chk(self.L.nq_freq_attach(self.h, int(kmax), int(every), int(length), len(fields), f), "nq_freq_attach")

    def freq_detach(self):
        self._chk(self.L.nq_freq_detach(self.h), "nq_freq_detach")

    def freq_info(self):
        out = (ctypes.c_longlong * 3)()
        self._chk(self.L.nq_freq_info(self.h, out), "nq_freq_info")
        return int(out[0]), int(out[1]), int(out[2])

    def freq_series(self, field, held, rows, cols):
        steps = (ctypes.c_longlong * max(held, 1))()
        out = np.empty((held, rows, cols), np.complex128)
        self._chk(self.L.nq_freq_series(self.h, int(field), steps, _dptr(out.view(np.float64))), "nq_freq_series")
        return np.array(steps[:held], np.int64), out

    def freq_spectrum(self, field, window, demean, dk, nb):
        w = np.ascontiguousarray(window, np.float64)
        out = np.empty((len(w), nb))
        self._chk(self.L.nq_freq_spectrum(self.h, int(field), _dptr(w), int(bool(demean)), float(dk), int(nb), _dptr(out)), "nq_freq_spectrum")
        return out

    # ---- time-mean and covariance maps (include/niwqg_amd.h: nq_avg_*; niwqg_amd/averages.py) ---------------------------------------
    def avg_attach(self, fields, pairs, every):
        f = (ctypes.c_int * len(fields))(*fields)
        flat = [i for p in pairs for i in p]
        pr = (ctypes.c_int * max(1, len(flat)))(*flat)
        self._chk(self.L.nq_avg_attach(self.h, len(fields), f, len(pairs), pr, int(every)), "nq_avg_attach")

    def avg_detach(self):
        self._chk(self.L.nq_avg_detach(self.h), "nq_avg_detach")

    def avg_sample(self):
        self._chk(self.L.nq_avg_sample(self.h), "nq_avg_sample")

    def avg_reset(self):
        self._chk(self.L.nq_avg_reset(self.h), "nq_avg_reset")

    def avg_info(self):
        """(samples in the sums, steps since attach, planes)"""
        out = (ctypes.c_longlong * 3)()
        self._chk(self.L.nq_avg_info(self.h, out), "nq_avg_info")
        return int(out[0]), int(out[1]), int(out[2])

    def avg_read(self, index, cplx=False):
        out = np.empty((self.nx, self.nx), np.complex128 if cplx else np.float64)
        self._chk(self.L.nq_avg_read(self.h, int(index), _dptr(out.view(np.float64))), "nq_avg_read")
        return out

    # ---- time-mean spectra, transfer and flux (include/niwqg_amd.h: nq_tspec_*; niwqg_amd/timespectra.py) ---------------------------
    def tspec_attach(self, mask, every):
        self._chk(self.L.nq_tspec_attach(self.h, int(mask), int(every)), "nq_tspec_attach")

    def tspec_detach(self):
        self._chk(self.L.nq_tspec_detach(self.h), "nq_tspec_detach")

    def tspec_sample(self):
        self._chk(self.L.nq_tspec_sample(self.h), "nq_tspec_sample")

    def tspec_reset(self):
        self._chk(self.L.nq_tspec_reset(self.h), "nq_tspec_reset")

    def tspec_info(self):
        """(samples in the sums, steps since attach, mask)"""
        out = (ctypes.c_longlong * 3)()
        self._chk(self.L.nq_tspec_info(self.h, out), "nq_tspec_info")
        return int(out[0]), int(out[1]), int(out[2])

    def tspec_read(self, which):
        """table `which` (TSPEC_S1 .. TSPEC_P2): (32, nb) for the spectra's two, (TRANSFER_ROWS, nb) for the others"""
        nb = int(self.L.nq_spectrum_shells(self.h))
        out = np.zeros((32 if which in (TSPEC_S1, TSPEC_S2) else TRANSFER_ROWS, nb))
        self._chk(self.L.nq_tspec_read(self.h, int(which), _dptr(out)), "nq_tspec_read")
        return out
