/* niwqg_amd -- C ABI of the MI355X-native ETDRK4 pseudo-spectral stepper.
 *
 * The reference (cesar-rocha/niwqg) is pure Python and has no FFI of its own; its drop-in boundary
 * is the Python class surface.  This header is the boundary a maintainer of
 * the reference would bind with ctypes (INTEGRATION.md shows the stub); every entry point names the
 * reference method it stands in for (file:line in the reference checkout).
 *
 * Conventions
 *   - plain pointers and sizes only; host buffers are caller-owned, device buffers context-owned;
 *   - one host thread per context, one HIP stream per context;
 *   - every function returns 0 on success or a negative error code; nq_last_error() gives text;
 *   - complex arrays are interleaved (re, im) doubles, i.e. numpy complex128;
 *   - all 2-D host arrays are C-contiguous in the reference's layouts: physical (ny, nx);
 *     Kernel-family spectral (ny, nx) index [l, k]; QGModel spectral (ny, nx/2+1).
 */
#ifndef NIWQG_AMD_H
#define NIWQG_AMD_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nq_ctx nq_ctx;

enum { NQ_MODEL_COUPLED = 0, NQ_MODEL_UNCOUPLED = 1, NQ_MODEL_QG = 2,
       NQ_MODEL_YBJ = 3 /* niwqg/YBJModel.py: steady psi, nq_step advances phi only (YBJModel.py:52-87); single rank */ };

/* field ids for nq_get_field.  Exact host shapes (C-contiguous; "cplx" = interleaved re,im doubles); nq_field_doubles()
 * returns the number of doubles written.  Spectra of REAL fields (qh, ph, qwh, ch) always come as the HALF spectrum
 * (ny, nx/2+1), k = 0..nx/2, for every model: the reference's Kernel-family (ny,nx) arrays follow from
 * X(l,k) = conj X(-l,-k) for k > nx/2 (niwqg_amd/Kernel.py: hermitian_full; with dual_q the k < 0 side of qh is
 * NQ_F_QH_MINUS instead; without it row ny/2 of qh additionally gets the passenger of nq_get_qh_passenger).  phih is a
 * genuine full plane. */
enum {
  NQ_F_Q = 0,      /* real (ny,nx)        q      = Re ifft(qh)                 Kernel.py:97/CoupledModel.py:97 */
  NQ_F_QH = 1,     /* cplx (ny,nx/2+1)    qh                                                                    */
  NQ_F_P = 2,      /* real (ny,nx)        p      streamfunction                CoupledModel.py:93               */
  NQ_F_PH = 3,     /* cplx (ny,nx/2+1)    ph                                                                    */
  NQ_F_PHI = 4,    /* cplx (ny,nx)        phi                                  Kernel.py:337                    */
  NQ_F_PHIH = 5,   /* cplx (ny,nx)        phih                                                                  */
  NQ_F_U = 6,      /* real (ny,nx)        u = Re ifft(-il ph)                  Kernel.py:481                    */
  NQ_F_V = 7,      /* real (ny,nx)        v = Re ifft( ik ph)                                                   */
  NQ_F_QPSI = 8,   /* real (ny,nx)        q_psi = q - qw (q without waves)     CoupledModel.py:145-152          */
  NQ_F_QW = 9,     /* real (ny,nx)        qw                                   (coupled model only)             */
  NQ_F_QWH = 10,   /* cplx (ny,nx/2+1)    qwh                                  CoupledModel.py:86-88            */
  NQ_F_PHIX = 11,  /* cplx (ny,nx)        phix (as last refreshed: quirk Q1)   Kernel.py:610                    */
  NQ_F_PHIY = 12,  /* cplx (ny,nx)        phiy                                                                  */
  NQ_F_QH_MINUS = 13,/* cplx half spectrum conj(qh(-l,-k)), k = 0..nx/2 (dual_q contexts only)                  */
  NQ_F_C = 14,       /* real (ny,nx)       c      passive scalar of QGModel     QGModel.py:403-404               */
  NQ_F_CH = 15,      /* cplx (ny,nx/2+1)   ch                                                                     */
  NQ_F_QH_STAGE4 = 16,/* cplx half spectrum qh at which the LAST step evaluated its fourth stage: the u, v that QGModel's
                         jacobian_psi_c sees at a diagnostics tick are still those (QGModel.py:375, :483-495, :727-731) */
  NQ_F_PHIH_STAGE4 = 17,      /* cplx (ny,nx) phih of that same stage (Kernel family): with NQ_F_QH_STAGE4 it determines the
                                 self.u, self.v a step leaves behind -- the reference's last jacobian_psi_q call of a step is
                                 the fourth stage's (Kernel.py:364-368 vs :381-387), not the new state's                     */
  NQ_F_QH_MINUS_STAGE4 = 18,  /* the second copy (NQ_F_QH_MINUS) of that stage, dual_q contexts                              */
  NQ_F_QH_TICK = 19,          /* qh, phih, the second copy of qh and qwh as the last nq_tick_snapshot kept them: what the      */
  NQ_F_PHIH_TICK = 20,        /* reference's tick-only leftovers (upsilon Kernel.py:618; phq, phw, uq, vq, uw, vw              */
  NQ_F_QH_MINUS_TICK = 21,    /* CoupledModel.py:99-113; YBJModel's lapphi) are rebuilt from between ticks                     */
  NQ_F_QWH_TICK = 22
};

/* scalar ids for nq_get_scalar */
enum {
  NQ_S_KE = 0, NQ_S_PW = 1, NQ_S_KW = 2,   /* INCREMENT of the budget accumulators Ke, Pw, Kw since the last
                                              read (reading resets it)             Kernel.py:390-392;
                                              QGModel with passive scalar: NQ_S_PW is the increment of cvar
                                              (QGModel.py:394)                                        */
  NQ_S_KE_QG = 3,                          /* _calc_ke_qg()                        Kernel.py:600-602 */
  NQ_S_KE_NIW = 4,                         /* _calc_ke_niw()                       Kernel.py:604-606 */
  NQ_S_PE_NIW = 5,                         /* _calc_pe_niw() (no side effect here) Kernel.py:608-611 */
  NQ_S_CFL = 6,                            /* max(|u|,|v|,|phi|): _calc_cfl() without the dt/dx factor
                                                                                   Kernel.py:660-662 */
  NQ_S_MAX_PHI = 7                         /* max |phi| alone (the status line's CFL combines it with the
                                              fourth stage's max |u|, |v|: nq_get_stage4_max)        */
};

typedef struct nq_params {
  int model;          /* NQ_MODEL_*                                                             */
  int nx;             /* grid is nx x nx (the reference ignores ny, Kernel.py:100-101)          */
  int budgets;        /* 1: accumulate Ke,Pw,Kw inside the step like Kernel.py:319-322,:390-392 */
  int dual_q;         /* 1: keep the second q-hat copy X-(l,k) = conj(qh(-l,-k)) (needed when filtr is not
                         mirror-symmetric, i.e. dealias=True, Kernel.py:277-281; also makes qh exact on row N/2) */
  double dt;
  double U;           /* uniform zonal flow                                                     */
  double f;           /* Coriolis                                                               */
  double kappa2;      /* (m f / N)^2                                                            */
  double nu, nu4, mu;       /* q equation   Kernel.py:417-418 / QGModel.py:426-428              */
  double nuw, nu4w, muw;    /* phi equation Kernel.py:440-442                                   */
  double beta;        /* QGModel only                                                           */
  int passive_scalar; /* QGModel only: 1 = also step the passive scalar c (QGModel.py:345-404)  */
  double nu4c, nuc, muc;    /* its linear operator -nu4c wv4 - nuc wv2 - muc (QGModel.py:446-454)      */
} nq_params;

/* Kernel.__init__ / QGModel.__init__ (Kernel.py:139-152): builds grid-dependent tables on the device.
 *   kk   : nk wavenumbers (nk = nx for the Kernel family, nx/2+1 for QG)   Kernel.py:242-244 / QGModel.py:249
 *   ll   : nx wavenumbers
 *   filtr: host (nx, nk) real plane, the reference's `filtr`                  Kernel.py:267-284
 *   contour: 32 complex roots of unity r_j used by the ETDRK4 contour mean    Kernel.py:424-426
 * The ETDRK4 coefficient planes (Kernel.py:417-454) are computed on the device.                      */
int nq_create(const nq_params* p, const double* kk, const double* ll, const double* filtr,
              const double* contour, int device, nq_ctx** out);
int nq_destroy(nq_ctx* ctx);
const char* nq_last_error(const nq_ctx* ctx);     /* ctx may be NULL: last global error */

/* Kernel.set_q (Kernel.py:520-535) / QGModel.set_q (QGModel.py:507-520) */
int nq_set_q(nq_ctx* ctx, const double* q_host);
/* QGModel.set_c (QGModel.py:522-534): real (ny,nx); call after nq_set_q */
int nq_set_c(nq_ctx* ctx, const double* c_host);
/* Kernel.set_phi (Kernel.py:538-551): phi_host is complex (ny,nx) */
int nq_set_phi(nq_ctx* ctx, const double* phi_host);
/* CoupledModel._invert + _calc_rel_vorticity (CoupledModel.py:75-97,:145-152), UnCoupledModel._invert
 * (UnCoupledModel.py:54-64), QGModel._invert (QGModel.py:497-505) on the current state */
int nq_invert(nq_ctx* ctx);
/* replay of the side effect of _calc_pe_niw on phix/phiy (Kernel.py:610, quirk Q1) */
int nq_refresh_grad_phi(nq_ctx* ctx);

/* nsteps x Kernel._step_etdrk4 (Kernel.py:307-397) / QGModel._step_etdrk4 (QGModel.py:328-407).
 * Asynchronous on the context's stream.                                                              */
int nq_step(nq_ctx* ctx, int nsteps);
/* After a step WITHOUT a diagnostics tick the reference's self.u, self.v are still those of the fourth jacobian_psi_q call
 * of _step_etdrk4 (Kernel.py:364-368), and its status line's CFL (Kernel.py:594, :660-662) is taken from them.
 * nq_request_stage4_max: the last step of the NEXT nq_step / nq_slab_step call also records max |u|, max |v| of that stage
 * over this rank's rows (two extra row passes in that one step, nothing otherwise); nq_get_stage4_max reads them
 * (out2 = max|u|, max|v|; -4 when the last step call recorded none).  Kernel family only (QGModel._calc_cfl recomputes
 * u, v from psi: QGModel.py:621-629; YBJModel's u, v are steady). */
int nq_request_stage4_max(nq_ctx* ctx);
int nq_get_stage4_max(nq_ctx* ctx, double* out2);
/* Keep this rank's qh (both copies), phih and qwh as they are NOW (device-to-device, asynchronous; four planes allocated by the
 * first call): the host classes call it at every diagnostics tick (Diagnostics.py:41-58), because some of the arrays a tick
 * leaves on the reference's instance are refreshed by nothing else (see NQ_F_QH_TICK).  Read back with nq_get_field
 * (NQ_F_*_TICK) or nq_download_spectral (which 9-12). */
int nq_tick_snapshot(nq_ctx* ctx);
int nq_sync(nq_ctx* ctx);

/* copy a field to the host in the reference's layout (blocking) */
int nq_get_field(nq_ctx* ctx, int field_id, double* host_out);
/* number of doubles nq_get_field(field_id) writes for this context (-1: unknown id or NULL ctx) */
long long nq_field_doubles(const nq_ctx* ctx, int field_id);
/* The reference's full-plane qh is not exactly Hermitian: on row l = ny/2 the il term of jacobian_psi_q
 * (Kernel.py:471-486; numpy's ll[ny/2] is not odd) adds an anti-Hermitian part A_k that every stage update carries
 * along (Kernel.py:327, :347, :364, :381) and that never reaches physical space.  The device evolves it as ONE extra row
 * beside the half spectrum; out_cplx receives A_k for this context's local half-spectrum columns (nx/2+1 complex values
 * on a single context, entries k = 0 and nx/2 zero; all zeros for QGModel, YBJModel and dual_q contexts):
 *     qh_ref[ny/2, k] = qh[ny/2, k] + A_k,     qh_ref[ny/2, nx-k] = conj(qh[ny/2, k]) - conj(A_k),   0 < k < nx/2.    */
int nq_get_qh_passenger(nq_ctx* ctx, double* out_cplx);
int nq_get_scalar(nq_ctx* ctx, int scalar_id, double* out);

/* Snapshots that do not stall the stepper (niwqg/Saving.py:59-86 saves t, q, phi every tsave_snapshots steps):
 * nq_snapshot_begin forms q (real (ny,nx)) and, with_phi != 0, phi (cplx (ny,nx)) of the CURRENT state in device buffers of
 * their own and starts their copy to pinned host memory on a second stream; further nq_step calls may be queued at once.
 * nq_snapshot_end waits for that copy only and writes the arrays to q_out / phi_out (either may be NULL).  One in flight. */
int nq_snapshot_begin(nq_ctx* ctx, int with_phi);
int nq_snapshot_end(nq_ctx* ctx, double* q_out, double* phi_out);

/* the FFT seam, Kernel.fft / Kernel.ifft (Kernel.py:562-566): complex (ny,nx) -> complex (ny,nx);
 * QGModel.fft / ifft (QGModel.py:551-552): real (ny,nx) <-> complex (ny,nx/2+1).                     */
int nq_fft2(nq_ctx* ctx, const double* in_cplx, double* out_cplx);
int nq_ifft2(nq_ctx* ctx, const double* in_cplx, double* out_cplx);
int nq_rfft2(nq_ctx* ctx, const double* in_real, double* out_cplx);
int nq_irfft2(nq_ctx* ctx, const double* in_cplx, double* out_real);

/* The three Jacobians, evaluated on the current device state, in the reference's own array layouts and with its
 * [0,0] conventions (assembled on the device; nothing left for the caller to multiply or expand):
 *   nq_jacobian_psi_q    Kernel.jacobian_psi_q (Kernel.py:471-486): ik*fft(u q) + il*fft(v q), [0,0] = 0
 *                          -> cplx (ny, nx)       = 2*ny*nx doubles          (Kernel family)
 *                        QGModel.jacobian_psi_q (QGModel.py:469-481): same, [0,0] kept
 *                          -> cplx (ny, nx/2+1)   = 2*ny*(nx/2+1) doubles    (NQ_MODEL_QG)
 *   nq_jacobian_psi_phi  Kernel.jacobian_psi_phi (Kernel.py:457-469): fft(u phix + v phiy), [0,0] = 0 (kept by a
 *                        NQ_MODEL_YBJ context, YBJModel.py:123-133)         -> cplx (ny, nx) = 2*ny*nx doubles
 *   nq_jacobian_phic_phi CoupledModel.jacobian_phic_phi (CoupledModel.py:59-73), [0,0] = 0; refreshes phix, phiy
 *                                                                           -> cplx (ny, nx) = 2*ny*nx doubles
 * nq_products_uq_vq has no reference counterpart: the two transforms fft(u q), fft(v q) themselves on k = 0..nx/2,
 *                        cplx (2, ny, nx/2+1) = 4*ny*(nx/2+1) doubles (tests; callers with their own flux forms). */
int nq_jacobian_psi_q(nq_ctx* ctx, double* out_cplx);
/* QGModel with its passive scalar: ik*fft(u c) + il*fft(v c), (ny, nx/2+1) cplx (QGModel.py:483-495), u, v of the current psi */
int nq_jacobian_psi_c(nq_ctx* ctx, double* out_cplx);
int nq_jacobian_psi_phi(nq_ctx* ctx, double* out_cplx);
int nq_jacobian_phic_phi(nq_ctx* ctx, double* out_cplx);
int nq_products_uq_vq(nq_ctx* ctx, double* out_cplx2);
/* fft(phi * q_psi), cplx (ny, nx) = 2*ny*nx doubles: the refraction source of Kernel.py:332 (before its -0.5j factor;
 * mean not removed), formed by the row kernel exactly as inside a step */
int nq_refraction(nq_ctx* ctx, double* out_cplx);

/* Diagnostics tick on the device: the raw sums from which every scalar of increment_diagnostics (Diagnostics.py:41-58;
 * the 21 kernel lambdas Kernel.py:718-868 and the 3 class lambdas CoupledModel.py:115-136) follows without any plane
 * leaving the GPU.  out: 32 doubles, M = nx*nx, H = Hermitian part on the two self-mirrored columns:
 *   [0..3]  sum wv2^n |phih|^2, n = 0..3      (ke_niw, pe_niw, ep_phi, chi_phi; Kernel.py:604-611, :629-652)
 *   [4,5]   phih[0,0]                         (cke_niw, pi; Kernel.py:701-706)
 *   [6]     sum |H qh|^2          -> ens      [7] sum wv4 |qh|^2 -> chi_q        [8]  sum |qh|^2/wv2  -> ke_qg_q
 *   [9]     sum |qwh|^2/wv2       -> ke_qg_w  [10] sum Re(conj(H qh) H qwh) (l'^2 + k'^2)/wv2^2, l' = 0 on row ny/2, k' = 0 on column nx/2 -> -ke_qg_qw
 *   [11]    sum wv2 |ph|^2        -> ke_qg    [12..14] sum {wv4, wv2, 1} Re(conj(H ph) H qh) -> ep_psi (Kernel.py:635-640)
 *   [15]    mean(q_psi)
 *   [16..23] physical sums: q^2, q_psi^2, q_psi^3, (q_psi-mean)^2, ups^2, ups q_psi, q_psi Re(phi), q_psi Im(phi),
 *            ups = |phi|^2 - mean|phi|^2     (conc_niw, skew, pi; Kernel.py:613-623, :701)
 *   [24..27] sum {Re, Im}(conj(lap_h) J), {Re, Im}(conj(diss_h) J),  J = F[u phix + v phiy]        (gamma2, xi1)
 *   [28..31] the same four with i F[phi q_psi] in place of J                                        (gamma1, xi2)
 * Sums over the half spectrum carry weight 2 on the interior columns.  QGModel: entries [6..15] only; with its passive
 * scalar also [16..19] sum w wv2^n |ch|^2, n = 0..3 (n = 0 without [0,0]; C2, gradC2, ep_c, chi_c of QGModel.py:595-604,
 * :724-726) and [20] sum w Re(conj(-wv2 ch)(ik F[u c] + il F[v c])) (Gamma_c, QGModel.py:727-731; u, v of the state at
 * which the last step evaluated its fourth stage, as the reference's are at a tick).                          */
int nq_diagnostics(nq_ctx* ctx, double* out32);

/* Isotropic spectra of the diagnostics tick: out[s * nb + b] = the sum, over the wavenumbers of shell b,
 * of the exact term nq_diagnostics adds into sum s (same expression, weights, Hermitian parts, dual copies, passenger row and
 * filter ratios), so that sum_b out[s * nb + b] = out32[s] up to summation order.  Shell of (l, k), i = kx/dk, j = ly/dk: the
 * unique b >= 0 with 2b - 1 <= 2 sqrt(i^2 + j^2) < 2b + 1 (integers: b = (isqrt(4 (i^2 + j^2)) + 1) / 2); shells b <= nx/2 lie
 * wholly inside the square, the outer ones are partial.  nb must be nq_spectrum_shells(ctx) = round(nx / sqrt 2) + 1.  Binned
 * rows: Kernel family [0..3], [6..14], [24], [27], [28], [31]; QGModel [6..14] and with its passive scalar [16..19]; every
 * other row is zero.  Deterministic (no floating-point atomics: one workgroup per shell); the products passes of the tick are
 * run again, nothing else a step or a later call reads is touched.  The first call allocates two real full planes (Kernel
 * family; counted by nq_device_bytes).  Single-rank contexts.                                                          */
int nq_spectrum_shells(const nq_ctx* ctx);
int nq_diagnostics_binned(nq_ctx* ctx, int nb, double* out);

/* Spectral transfer: out[r * nb + b] = the RAW shell sum of row r over the wavenumbers of shell b, on
 * the full plane of the reference (no signs, no 1/M^2; shells as nq_diagnostics_binned, nb = nq_spectrum_shells(ctx)).
 * With P = F[psi], Q = F[q] (the q-hat the tick bins: the mean of the two copies on dual_q contexts), Jq = ik F[u q] +
 * il F[v q], J = F[u phix + v phiy] and R = i F[phi q_psi] of the tick (phix, phiy as last refreshed: quirk Q1), C = F[c],
 * Jc = ik F[u c] + il F[v c], u, v, q_psi of the current state:
 *   [0] sum Re(conj(P) Jq)      [1] sum Re(conj(Q) Jq)          (CoupledModel, UnCoupledModel, QGModel; zero for YBJModel)
 *   [2] sum Re(conj(phih) J)    [3] sum Re(conj(phih) R)        (Kernel family)
 *   [4] sum Re(conj(C) Jc)      [5] sum wv2 Re(conj(C) Jc)      (QGModel with its passive scalar)
 * every other row is zero.  Deterministic (no floating-point atomics: one workgroup per shell).  The products passes the tick
 * runs (J, then R; the first also gives F[u q], F[v q] and F[u c], F[v c]) are run again into scratch planes; nothing else a
 * step or a later call reads is touched.  Slab contexts allocate their planes on the first call (counted by nq_device_bytes).
 * Single-rank contexts; nq_slab_transfer_binned below for slabs.                                                            */
#define NQ_TRANSFER_ROWS 6
int nq_transfer_binned(nq_ctx* ctx, int nb, double* out);

/* PDFs and joint PDFs of the physical fields: COUNTS of the values the tick's physical sums [16..23] see.
 * Fields: NQ_PDF_Q q, NQ_PDF_QPSI q_psi = q - q_w (= q without the wave feedback), NQ_PDF_PHI2 |phi|^2 of the last inversion's rows
 * (Kernel family; dual_q contexts: the mean of the two q-hat copies); QGModel: NQ_PDF_Q and, with its passive scalar, NQ_PDF_C of
 * the current spectra.  Bin rule (fp64, the same __device__ function everywhere): s = bins / (hi - lo) formed once on the host;
 * x != x -> NaN; x < lo -> below; x > hi -> above; else i = min((int) floor((x - lo) * s), bins - 1), so x == hi is in the last bin.
 *
 * nq_field_minmax: out[2 i], out[2 i + 1] = exact minimum and maximum of fields[i] (both NaN when any value is), one device pass.
 * nq_field_hist:   bins the listed fields (1 to 3, each once) over [lo[i], hi[i]] (finite, lo < hi) into `bins` (1..1024) bins
 *   each; joint_a, joint_b >= 0: also ONE table of joint_bins (1..128) bins per axis over the same ranges for that pair of the
 *   list (joint_a = joint_b = -1: none).  accumulate = 0 zeroes the device tables first; 1 adds to what they hold and needs the
 *   fields, ranges and bin counts of the call that zeroed them.  Nothing is copied to the host.
 * nq_field_hist_read: the tables of the last nq_field_hist configuration as 64-bit counts: per field of its list bins + 3
 *   (the bins, below, above, NaN), then, with a joint table, joint_bins^2 + 1: [index of b][index of a], then the points with
 *   either value out of range or NaN.
 * Integer counters only (32-bit in LDS per workgroup, 64-bit in global memory): bit-reproducible.  The Kernel family writes no
 * physical plane; QGModel goes through the scratch planes of nq_get_field.  The first call allocates the tables of the largest
 * configuration and the min/max partials, NQ_PDF_DEVICE_BYTES in all (counted by nq_device_bytes, freed with the context).
 * Reads the state, writes only these buffers.  Single-rank contexts (-4 on slab contexts).
 *
 * Flow fields, Kernel family only, one numbering for nq_field_minmax, nq_field_hist and nq_avg_attach:
 * NQ_FLOW_U u, NQ_FLOW_V v, NQ_FLOW_SN the normal strain 2 u_x, NQ_FLOW_SS the shear strain 2 v_x - q_psi, NQ_FLOW_STRAIN2 = sn^2 +
 * ss^2, NQ_FLOW_OW = strain2 - q_psi^2 (Okubo-Weiss), NQ_FLOW_GRADPHI2 = |phi_x|^2 + |phi_y|^2 of the current phi-hat; all of the
 * last inversion's rows, like NQ_PDF_QPSI.  They may be mixed with the three fields above; a list that names one runs ONE row
 * pass (k_x_flow_hist / k_x_flow_moments) for all of its fields, a list that names none runs the kernels it always ran.  A flow
 * field on a QGModel context is -1.  At nx = 8192 a device thread holds one value and every field of such a list runs in a launch
 * of its own: a joint table, or a product of two different fields in nq_avg_attach, is -1 there.                              */
enum { NQ_PDF_Q = 0, NQ_PDF_QPSI = 1, NQ_PDF_PHI2 = 2, NQ_PDF_C = 3 };
enum { NQ_FLOW_U = 16, NQ_FLOW_V = 17, NQ_FLOW_SN = 18, NQ_FLOW_SS = 19, NQ_FLOW_STRAIN2 = 20, NQ_FLOW_OW = 21, NQ_FLOW_GRADPHI2 = 22 };
#define NQ_PDF_MAX_BINS 1024
#define NQ_PDF_MAX_JOINT_BINS 128
#define NQ_PDF_DEVICE_BYTES ((3 * (NQ_PDF_MAX_BINS + 3) + NQ_PDF_MAX_JOINT_BINS * NQ_PDF_MAX_JOINT_BINS + 1) * 8 + 6 * 8192 * 8)
int nq_field_minmax(nq_ctx* ctx, int nfields, const int* fields, double* out);
int nq_field_hist(nq_ctx* ctx, int nfields, const int* fields, const double* lo, const double* hi, int bins, int joint_a,
                  int joint_b, int joint_bins, int accumulate);
int nq_field_hist_read(nq_ctx* ctx, unsigned long long* out);

/* Structure functions of the physical fields: raw plane SUMS of the moments of the x-increments
 * d_r a(x, y) = a((x + r) mod nx, y) - a(x, y), periodic, for each listed separation r (integers in [1, nx - 1], strictly
 * increasing, at most NQ_SF_MAX_SEPS).  fields: 1 to NQ_SF_MAX_FIELDS different ids out of those nq_field_hist takes for the model
 * (the same values: the rows of the last inversion) and, on the Kernel family, NQ_SF_PHI, the complex wave field phi itself.
 * NQ_SF_COLS = 9 columns per field and separation:
 *   a real field   [p - 1] = sum d^p, p = 1..6;        [6] = sum |d|,  [7] = sum |d|^3,  [8] = sum |d|^5
 *   NQ_SF_PHI      [p - 1] = sum |d phi|^p, p = 1..6;   [6] = sum Re d phi,  [7] = sum Im d phi,  [8] = 0
 * triples: ntriples (0 to NQ_SF_MAX_TRIPLES) x 3 INDICES into `fields`: one more column each, sum d_a d_b d_c; NQ_SF_PHI may only be
 * the last two entries together, (a, phi, phi) = sum d_a |d phi|^2.  A table row is one separation: 9 nfields + ntriples doubles.
 *
 * nq_structure: one state into the running table on the device; accumulate = 0 overwrites it, 1 adds to it and needs the fields,
 *   separations and triples of the call that started it.  Nothing is copied to the host.
 * nq_structure_read: *samples = states in the table, out = nsep x (9 nfields + ntriples) raw sums (divide by samples nx ny).
 * Deterministic: workgroup partials (one slot per workgroup and separation), then a second kernel adds the slots in a fixed order;
 * no floating-point atomics, so two calls on one state give the same bits.  The partials are allocated by the first call and grown
 * by the largest one, NQ_SF_PART_MAX_BYTES at most (counted by nq_device_bytes, freed with the context).  Reads the state, writes
 * only these buffers.  -1: bad arguments, a field the model lacks (any NQ_FLOW_* field or NQ_SF_PHI on a QGModel context), and at
 * nx = 8192 (one value per device thread, one launch per field) a triple of different fields; -4: slab contexts, nothing set yet,
 * no table yet; -5: an allocation failed.                                                                                     */
enum { NQ_SF_PHI = 32 };
#define NQ_SF_MAX_SEPS 64
#define NQ_SF_MAX_FIELDS 3
#define NQ_SF_MAX_TRIPLES 4
#define NQ_SF_COLS 9
#define NQ_SF_PART_MAX_BYTES (4096 * NQ_SF_MAX_SEPS * (NQ_SF_MAX_FIELDS * NQ_SF_COLS + NQ_SF_MAX_TRIPLES) * 8)
int nq_structure(nq_ctx* ctx, int nfields, const int* fields, int nsep, const int* seps, int ntriples,
                 const int* triples /* ntriples x 3 indices into fields */, int accumulate);
int nq_structure_read(nq_ctx* ctx, long long* samples, double* out /* nsep x (9 nfields + ntriples) raw sums */);

/* Structure functions at two-dimensional separations: the same columns and triples for the increments
 * d_r a(x, y) = a((x + r_x) mod nx, (y + r_y) mod ny) - a(x, y) at nvec (1 to NQ_SF2_MAX_VECS) lattice vectors, vecs = nvec x 2 ints
 * (r_x, r_y) in any order with r_x in [-(nx - 1), nx - 1], r_y in [0, ny - 1], not (0, 0), no vector twice and none beside its
 * own periodic image (r_x and r_x - nx).  A table row is one vector, in the caller's order.  proj (or NULL): nvec x 2 doubles
 * (c_x, c_y), finite; the increments of the real fields proj_a and proj_b (different indices into `fields`; -1, -1 with proj =
 * NULL) are rotated before anything is summed, d_L = c_x d_a + c_y d_b, d_T = -c_y d_a + c_x d_b: the columns and triples of
 * proj_a hold L, those of proj_b hold T.  The library takes (c_x, c_y) as given (the unit vector of (r_x dx, r_y dy) is the
 * caller's business) and needs no grid spacing.
 *
 * The Kernel family's values are first stored to physical planes of the context (at most NQ_SF_MAX_FIELDS real planes, or two and
 * a complex one; allocated by the first call, grown by the largest), so every combination of fields and triples works at every
 * fused size, nx = 8192 included.  The table, the planes and the owner of the running sums are this call's own: nq_structure's
 * table is not touched (the workgroup partials are shared, within NQ_SF_PART_MAX_BYTES).  Deterministic like nq_structure.
 * nq_structure2_read: *samples, out = nvec x (9 nfields + ntriples) raw sums.  Return codes as nq_structure's: -1 bad arguments
 * (a vector out of range, zero or listed twice; a projection on NQ_SF_PHI or on one field twice; a non-finite proj; a field the
 * model lacks); -4 slab contexts, nothing set yet, no table yet; -5 an allocation failed (the table, its sample count and the
 * planes are as they were: a buffer that grows is allocated before the old one is freed; the shared partials are freed first, as
 * nq_structure frees them, and are allocated again by the next call).                                                         */
#define NQ_SF2_MAX_VECS 256
int nq_structure2(nq_ctx* ctx, int nfields, const int* fields, int nvec, const int* vecs /* nvec x 2: r_x, r_y */,
                  const double* proj /* NULL or nvec x 2: c_x, c_y */, int proj_a, int proj_b, int ntriples,
                  const int* triples /* ntriples x 3 indices into fields */, int accumulate);
int nq_structure2_read(nq_ctx* ctx, long long* samples, double* out /* nvec x (9 nfields + ntriples) raw sums */);

/* PDFs of the field increments: COUNTS of the increments whose moments nq_structure and nq_structure2 sum,
 * per separation (or vector) and field.  fields, seps, vecs, proj, proj_a, proj_b: exactly as those two calls take them (no
 * triples).  A real field is binned signed; NQ_SF_PHI is binned as |d phi| = sqrt(Re^2 + Im^2).  With proj the pair is rotated first
 * (L in proj_a's table, T in proj_b's).  The bin rule is nq_field_hist's, with one range per (separation, field): lo, hi = n x
 * nfields doubles each (finite, lo < hi), s = bins / (hi - lo) formed once on the host; bins in [1, NQ_IPDF_MAX_BINS].
 *
 * nq_increment_range / nq_increment_range2: the range pass: out[(i nfields + f) 2] = sum d (NQ_SF_PHI: sum |d phi|), [.. + 1] = sum
 *   d^2 (sum |d phi|^2) of separation i and field f over the plane, from nq_structure's / nq_structure2's kernels into a table of this
 *   feature: the running tables, sample counts and configurations of those two calls are not touched (the workgroup partials are
 *   shared, within NQ_SF_PART_MAX_BYTES; nq_increment_range2 stores the Kernel family's values to the planes nq_structure2 uses).
 * nq_increment_hist / nq_increment_hist2: one state into the count table on the device; accumulate = 0 zeroes it first, 1 adds to
 *   it and needs the fields, separations or vectors, projection, ranges and bins of the call that zeroed it.  Nothing is copied
 *   to the host.  One table serves both calls.  On the fused grids the Kernel family's nq_increment_hist runs ONE row pass
 *   (k_x_flow_ipdf: the value rows in LDS, a table of 32-bit counters per separation in LDS, flushed to the 64-bit table with
 *   integer atomics); at nx = 8192 one launch per field, every combination of fields included.  QGModel and nq_increment_hist2
 *   go through physical planes (k_ipdf_plane).
 * nq_increment_hist_read: *samples = states in the table, out = n x nfields x (bins + 3) counts in the caller's field order: the
 *   bins, below, above, NaN.
 * Integer counters only: bit-reproducible.  The buffers are allocated by the first call, the count table is grown by the largest
 * one, NQ_IPDF_DEVICE_BYTES at most in all beside what nq_structure / nq_structure2 own (counted by nq_device_bytes, freed with the
 * context).  Reads the state, writes only these buffers.  -1: bad arguments, a field the model lacks, accumulate = 1 after
 * another configuration; -4: slab contexts, nothing set yet, no table yet; -5: an allocation failed, everything as it was.      */
#define NQ_IPDF_MAX_BINS NQ_PDF_MAX_BINS
#define NQ_IPDF_DEVICE_BYTES (NQ_SF2_MAX_VECS * (NQ_SF_MAX_FIELDS * (NQ_IPDF_MAX_BINS + 3) * 8 + NQ_SF_MAX_FIELDS * 3 * 8 + 16 + 16 + (NQ_SF_MAX_FIELDS * NQ_SF_COLS + NQ_SF_MAX_TRIPLES) * 8) + NQ_SF_MAX_SEPS * 4)
int nq_increment_range(nq_ctx* ctx, int nfields, const int* fields, int nsep, const int* seps, double* out /* nsep x nfields x 2 */);
int nq_increment_range2(nq_ctx* ctx, int nfields, const int* fields, int nvec, const int* vecs /* nvec x 2: r_x, r_y */,
                        const double* proj /* NULL or nvec x 2: c_x, c_y */, int proj_a, int proj_b, double* out /* nvec x nfields x 2 */);
int nq_increment_hist(nq_ctx* ctx, int nfields, const int* fields, int nsep, const int* seps, const double* lo /* nsep x nfields */,
                      const double* hi, int bins, int accumulate);
int nq_increment_hist2(nq_ctx* ctx, int nfields, const int* fields, int nvec, const int* vecs /* nvec x 2: r_x, r_y */,
                       const double* proj /* NULL or nvec x 2: c_x, c_y */, int proj_a, int proj_b, const double* lo /* nvec x nfields */,
                       const double* hi, int bins, int accumulate);
int nq_increment_hist_read(nq_ctx* ctx, long long* samples, unsigned long long* out /* n x nfields x (bins + 3) counts */);

/* Vortex census: the connected components of a thresholded field, labelled and summed on the device.
 * fields: 1 to 3 different REAL ids out of those nq_field_hist takes for the model (not NQ_SF_PHI); fields[crit] is the criterion a,
 * all of them are summed.  Point (y, x) is in the SET when a < t (NQ_VX_BELOW), a > t (NQ_VX_ABOVE) or |a| > t (NQ_VX_ABS_ABOVE) for
 * the finite threshold t; NaN is never in the set.  Components: those of the set under connectivity 4 or 8 on the doubly periodic
 * grid (column nx - 1 neighbours column 0, row ny - 1 row 0).  The LABEL of a component is the smallest linear index y nx + x of its
 * points, so the label plane does not depend on the order of execution.  Table: one row per component in ascending label order,
 * NQ_VX_COLS + nfields 64-bit integers:
 *   [0] label, (y0, x0) = divmod(label, nx)      [1] area in points       [2], [3] sum dx, sum dy
 *   [4], [5], [6] sum dx^2, sum dy^2, sum dx dy   [7], [8] bit patterns of the minimum and the maximum of a (doubles; -0 < +0)
 *   [9 + f] sum rint(a_f 2^s_f), half to even, a non-finite value counting 0
 * with dx = ((x - x0 + nx/2) mod nx) - nx/2 and dy likewise: the periodic offsets from the label's own point, in [-n/2, n/2) (a
 * component wider than half the domain gets what this formula gives).  s_f = 61 - ceil(log2(nx ny)) - e with max |a_f| = m 2^e, m in
 * [0.5, 1) over the finite values of the plane (s_f = 0 for a plane without a non-zero finite value): no sum over any subset of
 * the plane leaves int64, and a component's sum is sum a_f to within area 2^(-s_f - 1).  Integer sums: bit-reproducible.
 * capacity in [1, NQ_VX_MAX_CAPACITY]: the table holds the first min(total, capacity) components in label order; the points of
 * later ones are labelled, not summed.
 *
 * nq_vortex_range: out[4 f ..] = min, max, sum, sum of squares of field f over its finite values (+inf, -inf, 0, 0 without any),
 *   from workgroup partials added in a fixed order (deterministic); one small download.  It needs the small buffers only and
 *   keeps results of its own: the last census stays readable after it.
 * nq_vortex_census: every phase on the device, in stream order (range and scales, row runs, lock-free union-find across rows,
 *   flatten, rank, sums reduced per run within a wave and flushed with 64-bit integer atomics; csrc/nq_vortex.hpp).  Nothing is copied to the host, the host does not
 *   wait.
 * nq_vortex_read: info = {components found, rows in the table, points in the set, non-finite values met in the fields of the call,
 *   s_0, s_1, s_2}; table (or NULL): room for capacity rows, the first info[1] are written.
 * nq_vortex_labels: the ny x nx label plane of the last census, -1 outside the set.
 * nq_vortex_stats: out[4 f ..] = min, max, sum, sum of squares of field f of the last census, from its own range pass (what
 *   nq_vortex_range would have returned on that state); -4 before a census.
 * The Kernel family's values go through the physical planes nq_structure2 stores (grown by the largest call; a failure leaves the
 * old pool).  The label plane, the rank plane, the small buffers and the table are this feature's own: allocated by the first
 * call, grown all or none, counted by nq_device_bytes, freed with the context.  Reads the state, writes only these buffers and the
 * shared plane pool: the tables, sample counts and configurations of nq_structure2 and nq_increment_hist2 are not touched.
 * -1: bad arguments (a field the model lacks, a NQ_FLOW_* field on a QGModel context, a field listed twice, NQ_SF_PHI, a non-finite
 * threshold, connectivity other than 4 or 8, capacity out of range); -4: slab contexts, nothing set yet, a read before a census;
 * -5: an allocation failed, everything as it was.                                                                              */
enum { NQ_VX_BELOW = 0, NQ_VX_ABOVE = 1, NQ_VX_ABS_ABOVE = 2 };
#define NQ_VX_COLS 9
#define NQ_VX_MAX_CAPACITY 1048576
int nq_vortex_range(nq_ctx* ctx, int nfields, const int* fields, double* out /* nfields x 4: min, max, sum, sum of squares */);
int nq_vortex_census(nq_ctx* ctx, int nfields, const int* fields, int crit /* index into fields */, int mode, double threshold,
                     int connectivity /* 4 | 8 */, int capacity);
/* nq_vortex_census, synchronous, with device events between its phases (tools/vortices_cost.py): ms[0] the planes (the store
 * pass, or QGModel's transforms), then the range pass, the row pass, the merge, flatten + rank, the sums.  The census it leaves is
 * the one nq_vortex_census would have left. */
int nq_vortex_profile(nq_ctx* ctx, int nfields, const int* fields, int crit, int mode, double threshold, int connectivity,
                      int capacity, double* ms /* 6 */);
int nq_vortex_read(nq_ctx* ctx, long long* info /* 7 */, long long* table /* NULL or capacity x (NQ_VX_COLS + nfields) */);
int nq_vortex_labels(nq_ctx* ctx, int* out /* ny x nx labels, -1 outside the set */);
int nq_vortex_stats(nq_ctx* ctx, double* out /* nfields x 4: min, max, sum, sum of squares */);

/* Lagrangian particles, single-rank contexts only (slab contexts refuse every call with -4).
 * After every step of nq_step the library moves each particle one classical RK4 step through U_tot = (U + u, v), u = -d psi/dy,
 * v = d psi/dx of the ph the context holds, linear in time between U0 (start of the step) and U1 (after it):
 *   k1 = U0(x), k2 = (U0 + U1)/2 (x + dt/2 k1), k3 = (U0 + U1)/2 (x + dt/2 k2), k4 = U1(x + dt k3),
 *   x += dt/6 (k1 + 2 k2 + 2 k3 + k4);      (U0 + U1)/2 (x) is the mean of the two interpolated values.
 * U0 is formed again after nq_set_q, nq_set_phi, nq_set_c and nq_invert; YBJModel's psi is steady (U1 = U0).  Grid value [j, i]
 * sits at ((i + 1/2) Lx / nx, (j + 1/2) Ly / nx); values at a particle come from the periodic tensor-product cubic convolution
 * (Keys, a = -1/2) on the 4 x 4 nearest nodes; coordinates are reduced into [0, L) and node indices modulo nx, so no input
 * addresses outside a plane; a non-finite position gives NaN and stays NaN.  Positions are kept unwrapped.  No reductions, no
 * atomics: repeated runs are bit-identical; the particles write only buffers of their own, so every model output is the same as
 * without them.  Names of values (PT_*): 0 u, 1 v, 2 q, 3 phi (Kernel family only; two columns: real, imaginary part).
 *
 * attach: n >= 1 finite coordinates (host arrays); record_every r > 0 writes a record at attach (step 0) and after every r-th step
 * since, into a ring of `capacity` records of (2 + columns) x n doubles: x, y, then the named values of the state after that
 * step.  One set per context (-4 while one is attached).  Every allocation is counted by nq_device_bytes and freed by detach.
 * records: info[0] records written, [1] records held m = min(count, capacity), [2] doubles per particle and record, [3] steps
 * since attach; with steps / out non-null, the held records oldest first: steps[m] (steps since attach), out[m][2 + cols][n].
 * sample: out[cols][n], the named values at the current positions from the current state.                                    */
int nq_particles_attach(nq_ctx* ctx, int n, const double* x, const double* y, double Lx, double Ly, int record_every, int capacity,
                        int nnames, const int* names);
int nq_particles_detach(nq_ctx* ctx);
int nq_particles_get(nq_ctx* ctx, double* x, double* y);
int nq_particles_sample(nq_ctx* ctx, int nnames, const int* names, double* out);
int nq_particles_records(nq_ctx* ctx, long long* info4, long long* steps, double* out);

/* Drifter mode, Kernel family only: the particles move through the whole velocity,
 *   (U + u, v) + a (Re, Im)[phi(x, y, t) e^{-i f0 t}],
 * a > 0 the amplitude of the vertical mode at the drifters' depth, phi the back-rotated wave field.  The time of step s after
 * attach is t_s = t0 + s dt, s counted by the particles (not the accumulated float clock: they differ by rounding).  One step
 * from t = t_s, with Phi0 / Phi1 the physical phi of the state the step starts from and of the state after it (after the
 * forcing's re-emission), beside U0 / U1:
 *   k1 = U0(x) + a Phi0(x) e^{-i f0 t},   k2 = (U0 + U1)/2 (x + dt/2 k1) + a (Phi0 + Phi1)/2 (x + dt/2 k1) e^{-i f0 (t + dt/2)},
 *   k3 likewise at x + dt/2 k2,            k4 = U1(x + dt k3) + a Phi1(x + dt k3) e^{-i f0 (t + dt)},
 * k complex (x += Re, y += Im; U added to the real part), x += dt/6 (k1 + 2 k2 + 2 k3 + k4): the slow envelope linear in time,
 * the fast phase exact at the stage times (the three factors are formed on the host in double precision).  One stencil per stage
 * position serves the U and the phi gathers.  Phi0 is formed again after every call that forms U0 again (nq_set_phi included,
 * also where it leaves U0's source as it was).  YBJModel: U1 = U0, Phi0 / Phi1 are two planes.
 * wave: right after nq_particles_attach, before any step; -4 with no particles, on QGModel, after the first step or when the mode
 * is on already; -1 for a <= 0 or non-finite arguments; two (nx, nx) complex planes more, counted by nq_device_bytes and freed by
 * detach (-5: none of them stays).
 * Names NQ_PT_UW, NQ_PT_VW of attach and sample: a Re / Im [phi(x_p) e^{-i f0 t_s}] at the particle, one column each; without
 * drifter mode a = 1.  Their clock is f0 = nq_params.f, t0 = 0 until nq_particles_wave or nq_particles_clock (same refusals but
 * the amplitude's; no allocation) sets it; both write the "uw" / "vw" columns of the record taken at attach again.
 * NQ_LAGR_UVW, NQ_LAGR_UVT: nq_lagr_spectrum's composites uw + i vw and (u + uw) + i (v + vw) (all their columns recorded).    */
enum { NQ_PT_UW = 5, NQ_PT_VW = 6, NQ_LAGR_UVW = 7, NQ_LAGR_UVT = 8 };
int nq_particles_wave(nq_ctx* ctx, double amplitude, double f0, double t0);
int nq_particles_clock(nq_ctx* ctx, double f0, double t0);

/* Ray mode, Kernel family only: each particle is a near-inertial wave packet and also carries a wavevector
 * (k, l).  With eta = f / kappa^2 (hslash) and zeta = q_psi, the dispersion relation of the YBJ operator,
 *   omega = (U + u) k + v l + zeta / 2 + (eta / 2) (k^2 + l^2),
 * gives the rays as Hamilton's equations
 *   dx/dt = U + u + eta k,   dy/dt = v + eta l,   dk/dt = -(k u_x + l v_x) - zeta_x / 2,   dl/dt = -(k u_y + l v_y) - zeta_y / 2.
 * After every step of the model one classical RK4 step of the four, with the particles' time treatment: U0 / Z0 the (u, v) and zeta
 * planes of the state the step starts from, U1 / Z1 of the state after it, the fields linear in time between them (stages at t,
 * t + dt/2 twice, t + dt).  u, v, zeta come from the Keys interpolant and their gradients from ITS derivative (the same 16 nodes
 * contracted with w'(t) / dx along one axis): the discrete rays are Hamilton's equations of the interpolated omega exactly.
 * zeta is q_psi = q - q_w of the state the LAST INVERSION saw: on the host ifft2(-wv2 ph).real + mean(q).  nq_set_phi on
 * CoupledModel runs no inversion (quirk Q2): until the next one zeta stays what it was, the q_psi that matches the held ph, not
 * q minus the q_w of the new phi.  YBJModel: psi and q are steady, one zeta plane (formed again after nq_set_q).
 * rays: right after nq_particles_attach, before any step; -4 with no particles, on QGModel, on a slab context, after the first
 * step, or with ray or drifter mode on already (the two exclude each other: nq_particles_wave returns -4 once rays are on); -1
 * for null arrays or a non-finite k, l or eta; two arrays of n doubles and two (nx, nx) planes of doubles more (YBJModel: one),
 * counted by nq_device_bytes and freed by detach (-5: none of them stays, the particles are as they were).
 * get_rays: the wavevectors now (-4 without ray mode).
 * Names of attach and sample, one column each: NQ_PT_K, NQ_PT_L the wavevector; NQ_PT_ZETA zeta at the particle (any mode);
 * NQ_PT_OMEGA the omega above from the current state at the ray, U included.  Sampling K, L or OMEGA without ray mode: -1.  Attach
 * accepts them, for the mode is set after it: nq_particles_rays writes those columns of the record taken at attach again; records
 * taken without the mode hold NaN there.  nq_particles_attach takes up to 10 record names.  nq_lagr_spectrum does not take the
 * four (-1). */
enum { NQ_PT_K = 9, NQ_PT_L = 10, NQ_PT_ZETA = 11, NQ_PT_OMEGA = 12 };
int nq_particles_rays(nq_ctx* ctx, const double* k, const double* l, double eta);
int nq_particles_get_rays(nq_ctx* ctx, double* k, double* l);

/* Stretch mode, every model class (QGModel included: the mode needs the velocity plane only): each particle
 * also carries the deformation gradient F = d x(t) / d x0 of its trajectory, dF/dt = A F with A = [[u_x, u_y], [v_x, v_y]] at the
 * particle.  The six values (x, y, f11, f12, f21, f22) take one classical RK4 step after every step of the model, with the
 * particles' time treatment (stages at t, t + dt/2 twice, t + dt; the fields linear in time between U0 and U1; the F stages from
 * the stage values of F).  A comes from the derivative of the Keys interpolant on the 16 nodes that give (u, v), and a Runge-Kutta
 * step commutes with differentiation: F is the exact Jacobian of the discrete map the positions follow, not an approximation
 * beside it.  With drifter mode on (either order of the two calls) A gains the gradient of a phi e^{-i f0 t}: the compressible
 * case, det F != 1.  Ray mode and stretch mode exclude each other (the ray map lives in four dimensions).
 * tangent: right after nq_particles_attach, before any step.  F0 NULL: the identity; else [4][n] in the order f11, f12, f21, f22,
 * every value finite (-1 otherwise).  -4 with no particles, on a slab context, after the first step, when the mode is on already
 * or with ray mode on (nq_particles_rays returns -4 once the tangent is on).  Four arrays of n doubles more (32 B a particle, no
 * plane), counted by nq_device_bytes and freed by detach (-5: none of them stays, the particles are as they were).
 * get_tangent: F now, [4][n] (-4 without the mode).
 * tangent_reset: F = I now, so that a long run can renormalise before F overflows (overflow itself stays loud: inf, then NaN; no
 * clamp).  It writes no record.  tangent_step0: the particle step count (steps since attach) at which F was last the identity or
 * F0: 0, or the count at the last reset.
 * Names of attach and sample, one column each: NQ_PT_F11 .. NQ_PT_F22 the entries of F; NQ_PT_LNSIGMA the ln of the largest singular
 * value of F,  s = ((f11^2 + f12^2) + f21^2) + f22^2,  p = ((f11 - f22)^2 + (f12 + f21)^2) ((f11 + f22)^2 + (f21 - f12)^2)
 * (= s^2 - 4 det^2, without the cancellation near F = I),  ln sigma_1 = 1/2 ln(1/2 (s + sqrt p)), every product rounded on its
 * own; NQ_PT_DET f11 f22 - f12 f21.  Sampling them without the mode: -1.  Attach accepts them, for the mode is set after it:
 * nq_particles_tangent writes those columns of the record taken at attach again; records taken without the mode hold NaN there.
 * nq_lagr_spectrum does not take the six (-1).
 * nq_lagr_stretching: with the T held records and the group-sorted index list of nq_lagr_dispersion, out[T][G][4] = the sums over
 * run g of ln sigma_1, (ln sigma_1)^2, det F and (det F)^2, formed from the recorded f-columns (-1 unless all four are recorded)
 * by the summation of nq_lagr_dispersion: no floating-point atomics, two calls return the same bits.  A held record written before
 * the last reset is refused (-1; the text names the step count of the reset): call it once those records have left the ring.    */
enum { NQ_PT_F11 = 13, NQ_PT_F12 = 14, NQ_PT_F21 = 15, NQ_PT_F22 = 16, NQ_PT_LNSIGMA = 17, NQ_PT_DET = 18 };
int nq_particles_tangent(nq_ctx* ctx, const double* F0);
int nq_particles_get_tangent(nq_ctx* ctx, double* F);
int nq_particles_tangent_reset(nq_ctx* ctx);
int nq_particles_tangent_step0(nq_ctx* ctx, long long* step);
int nq_lagr_stretching(nq_ctx* ctx, int T, int G, const int* order, const int* offsets, double* out);

/* Lagrangian spectra and dispersion of the particle records, formed on the device, single-rank contexts
 * only (-4 on slab contexts, -4 with no particles attached; -1 with record_every = 0 or fewer than 2 held records).  With the
 * T held records (T must be their number), oldest first, and the particles taken in the order of a group-sorted index list --
 * `order` (n indices in [0, n)) in G <= 256 runs, run g being order[offsets[g] .. offsets[g + 1] - 1], offsets[0] = 0,
 * offsets[G] = n:
 * spectrum: name 0 u, 1 v, 2 q (real series), 3 phi (complex), 4 u + i v (both recorded); a real finite window w_n (T values),
 * demean: each particle's own time mean is subtracted first; X_p(i) = sum_n w_n x_n(i) e^{+2 pi i p n / nfft} (a series turning
 * as e^{-i omega t} appears at +omega), T <= nfft <= 8192 or nfft = 16384;
 *   out[p][g] = 1/2 sum_{i in run g} |X_p(i)|^2 / (nfft sum w^2),   (nfft, G), row p = FFT bin p.
 * The particles go through a (nfft, C) work plane C at a time: chunk = 0 takes C from (n, nfft) alone (the plane within 256 MiB),
 * chunk > 0 asks for that many (cut to the same bound); chunk partials are added in chunk order.
 * dispersion: with d = r_n(i) - r_0(i) of the unwrapped positions, out[n][g][6] = the sums over run g of dx, dy, dx^2, dy^2,
 * dx dy, (dx^2 + dy^2)^2; with npairs > 0 pairs (pi[q], pj[q]), indices in [0, n) and different, and s = r_n(pi) - r_n(pj),
 * out_pairs[n][5] = the sums of sx^2, sy^2, sx sy, |s|^2, |s|^4.
 * All sums are sums: the caller divides by the counts.  No floating-point atomics: two calls return the same bits.  The calls
 * wait for the context's stream first and write nothing the step or the particles read.  Work memory (and, for the spectrum, an
 * any-size engine for the transform along the record axis) is allocated by the first call, grows when a later call needs more,
 * is counted by nq_device_bytes and freed by nq_particles_detach; an allocation that fails is -5 and leaves none of it.          */
int nq_lagr_spectrum(nq_ctx* ctx, int name, int T, int nfft, const double* window, int demean, int G, const int* order, const int* offsets,
                     int chunk, double* out);
int nq_lagr_dispersion(nq_ctx* ctx, int T, int G, const int* order, const int* offsets, int npairs, const int* pi, const int* pj, double* out,
                       double* out_pairs);

/* Stochastic forcing of q and phi, single-rank contexts only (slab contexts refuse every call with -4).
 * After every step of nq_step (after the filtered ETDRK4 update, unfiltered) the library adds
 *   qh(l, k)   += sqrt(dt) Aq(l, k)   xi_q(l, k; s)      half spectrum (ny, nx/2+1), Hermitian: the forcing of q is a real field
 *   phih(l, k) += sqrt(dt) Aphi(l, k) xi_phi(l, k; s)    full plane (ny, nx), independent complex values
 * and then does what the end of a step does: phi, phiy from the new phih (when phi is forced; UnCoupledModel's frozen gradients,
 * quirk Q1, stay), the inversion of the new state, its spectral sums carried into slot 0 of the next step's budgets.  s starts at
 * step0 and counts forced steps (its low 32 bits enter the counter).  xi: Philox4x32-10, counter (l, k, s, stream) with stream
 * 0 for q and 1 for phi, key (seed & 0xffffffff, seed >> 32); from the output x0..x3: n = (x0 >> 5) 2^26 + (x1 >> 6),
 * u1 = 1 - n 2^-53, u2 = (x2 + 0.5) 2^-32, xi = sqrt(-ln u1) (cos 2 pi u2 + i sin 2 pi u2), E|xi|^2 = 1.  xi_q is zero on row
 * ny/2, column nx/2 and at (0, 0) whatever Aq holds; on column 0 row ny - l takes the conjugate of the value drawn at (l, 0),
 * 1 <= l < ny/2 (Aq must be equal on the two rows); a dual-q context adds the same increment to both copies of qh.
 * Amplitudes are finite and >= 0 (host arrays; NULL: that field is not forced; at least one).  QGModel takes q only, YBJModel
 * phi only (-1 otherwise).  The kernels run over the bounding box of A > 0 in (|l|, |k|) only.  Work, in fp64 on the device,
 * from per-workgroup partials summed in a fixed order (bit-reproducible), with psi-hat and phih BEFORE the increment D:
 *   work_q   += sum_full [ -Re(conj(psi-hat) D) + |D|^2 / (2 wv2) ] / M^2     (the change of ke_qg at fixed q_w)
 *   work_phi += sum      [  Re(conj(phih) D)    + |D|^2 / 2 ]       / M^2     (the change of ke_niw)
 * Ke, Pw, Kw stay the unforced rates.  Every allocation is counted by nq_device_bytes and freed by detach.
 * apply: one increment and re-inversion now, outside a step (advances s).  increment: the increment of step s of stream 0 / 1
 * as a host plane ((ny, nx/2+1) / (ny, nx) complex), the state untouched.  state: out3 = {s, work_q, work_phi}.              */
int nq_forcing_attach(nq_ctx* ctx, const double* Aq, const double* Aphi, unsigned long long seed, long long step0);
int nq_forcing_detach(nq_ctx* ctx);
int nq_forcing_apply(nq_ctx* ctx);
int nq_forcing_increment(nq_ctx* ctx, int stream, long long s, double* out_cplx);
int nq_forcing_state(nq_ctx* ctx, double* out3);

/* Low-mode time series recorded in the step and their frequency - wavenumber spectra, single-rank contexts
 * only (slab contexts refuse every call with -4).  A recorder keeps the block |i|, |j| <= kmax (1 <= kmax < nx/2) of the spectral
 * state in a device ring of `length` records, [field][record][row][col] complex128: rows j = 0..kmax, -kmax..-1 (fftfreq order);
 * columns the same for field 0 (phi-hat, full plane), i = 0..kmax for fields 1 (q-hat as the device holds it; the copy X+ of a
 * dual-q context) and 2 (psi-hat as the model's ph: on the Kernel family column 0 takes its Hermitian part in l).  CoupledModel
 * and UnCoupledModel take all three, QGModel 1 and 2, YBJModel 0 (-1 otherwise).  attach writes record 0 from the current state;
 * after that every `every`-th step of a step call since attach ends with one more record (after the forcing, one launch for all
 * fields, on the context's stream).  One recorder per context (-4 while one is attached).  Every allocation is counted by
 * nq_device_bytes and freed by detach; an allocation that fails is an error (-5) that leaves the context as it was.
 * info3 = {records written, records held, steps since attach}.  series: the held records, oldest first, steps (held) and
 * out_cplx (held x rows x cols complex); either may be NULL.
 * spectrum: with the T >= 2 held records x_n, a real finite window w_n (T values) and X_p = sum_n w_n x_n e^{+2 pi i p n / T}
 * (T ifft: a mode evolving as e^{-i omega t} appears at +omega), out (T, nb) with nb = shell(kmax, kmax) + 1, row p = FFT bin p:
 *   field 0:  1/2 sum_{block, shell b} |X_p|^2 / (M^2 T sum w^2),  M = nx ny
 *   field 1:  1/2 [sum_{col 0} |X_p|^2 + sum_{cols 1..kmax} (|X_p|^2 + |X_-p|^2)] / (M^2 T sum w^2)
 *   field 2:  as field 1 with kappa^2 = dk^2 (i^2 + j^2) inside the sums
 * demean: each mode's time mean is subtracted before the window.  Window, transform along the record axis (the any-length
 * column transform of the any-size engine) and binning run on the device; the binning is deterministic (no atomics).       */
int nq_freq_attach(nq_ctx* ctx, int kmax, int every, int length, int nfields, const int* fields);
int nq_freq_detach(nq_ctx* ctx);
int nq_freq_info(nq_ctx* ctx, long long* info3);
int nq_freq_series(nq_ctx* ctx, int field, long long* steps, double* out_cplx);
int nq_freq_spectrum(nq_ctx* ctx, int field, const double* window, int demean, double dk, int nb, double* out);

/* Time-mean and covariance maps of the physical fields, accumulated in the step, single-rank contexts only
 * (slab contexts refuse every call with -4).  The attachment keeps one running-sum plane per listed field and per listed product,
 * (ny, nx) float64 in physical order (NQ_AVG_PHI: complex128), zero at attach.  Fields: NQ_AVG_Q, NQ_AVG_QPSI, NQ_AVG_PHI2 (= |phi|^2)
 * and NQ_AVG_PHI on the Kernel family, NQ_AVG_Q and (with its passive scalar) NQ_AVG_C on QGModel, each at most once; the values
 * are those nq_field_hist bins (the rows of the last inversion; dual_q contexts: the mean of the two q-hat copies).  pairs: 2 x
 * nproducts field ids, unordered pairs of REAL fields of the list (a pair of one field: its second moment), each pair once; -1
 * otherwise.  A sample adds x to every field's plane and x y to every product's, in fp64, one thread per point (no atomics: two
 * runs are bit-identical; x y may be contracted into the add).  every >= 0: every `every`-th step of a step call since attach
 * ends with one sample, taken last (after the forcing, the particles and the recorder); 0: never.  attach takes no sample;
 * sample takes one now; reset zeroes the sums and the sample count, not the step count.  One set per context (-4 while one is
 * attached).  Every allocation is counted by nq_device_bytes and freed by detach; one that fails is an error (-5) that leaves
 * nothing attached.  info3 = {samples in the sums, steps since attach, planes}; read: plane `plane_index` (fields in the order of
 * the attach call, then the products) into out, nx ny doubles (NQ_AVG_PHI: 2 nx ny).  The Kernel family also takes the NQ_FLOW_*
 * fields above (at most three real fields in all, as ever).                                                                   */
enum { NQ_AVG_Q = 0, NQ_AVG_QPSI = 1, NQ_AVG_PHI2 = 2, NQ_AVG_C = 3, NQ_AVG_PHI = 4 };      /* the first four: NQ_PDF_* */
int nq_avg_attach(nq_ctx* ctx, int nfields, const int* fields, int nproducts, const int* pairs, int every);
int nq_avg_detach(nq_ctx* ctx);
int nq_avg_sample(nq_ctx* ctx);
int nq_avg_reset(nq_ctx* ctx);
int nq_avg_info(nq_ctx* ctx, long long* info3);
int nq_avg_read(nq_ctx* ctx, int plane_index, double* out);

/* Time-mean spectra, spectral transfer and flux, accumulated in the step, single-rank contexts only (slab
 * contexts refuse every call with -4).  what_mask: NQ_TSPEC_SPECTRA, NQ_TSPEC_TRANSFER or both (-1 otherwise).  A sample is what
 * nq_diagnostics_binned (NQ_TSPEC_SPECTRA) and nq_transfer_binned (NQ_TSPEC_TRANSFER) would return at that point, bit for bit: the
 * same passes on the same state (rows: the comments of those two calls above), left on the device -- nothing is downloaded and
 * the host does not wait.  With both, each of the tick's two products passes runs once per sample and serves the two tables.
 * Every raw element x of a sample goes S1 += x, S2 += x x; every transfer row also c[b] = sum_{b' <= b} x[b'], added in shell
 * order one after the other, then P1 += c, P2 += c c (the flux before its sign and factor).  fp64, in sample order, no atomics:
 * first moments are the sequential sums exactly, x x may be contracted into the add.  every >= 0: every `every`-th step of a step
 * call since attach ends with one sample, taken last (after the forcing, the particles, the recorder and the averages); 0: never.
 * attach takes no sample and allocates what the selected calls allocate on their first use (context-owned, kept at detach) and
 * the tables, (2 x 32 + 4 x NQ_TRANSFER_ROWS) x nb doubles, zero (freed by detach; one that fails is -5 and leaves nothing
 * attached); sample takes one now; reset zeroes the sums and the sample count, not the step count.  One set per context (-4
 * while one is attached).  info3 = {samples in the sums, steps since attach, what_mask}; read: table `which` into out, 32 x nb
 * doubles for NQ_TSPEC_S1 / _S2 (spectra), NQ_TRANSFER_ROWS x nb for NQ_TSPEC_T1 / _T2 (transfer) and NQ_TSPEC_P1 / _P2 (running
 * sums), nb = nq_spectrum_shells(ctx); the tables of a body that is not attached stay zero.                                    */
enum { NQ_TSPEC_SPECTRA = 1, NQ_TSPEC_TRANSFER = 2 };
enum { NQ_TSPEC_S1 = 0, NQ_TSPEC_S2 = 1, NQ_TSPEC_T1 = 2, NQ_TSPEC_T2 = 3, NQ_TSPEC_P1 = 4, NQ_TSPEC_P2 = 5 };
int nq_tspec_attach(nq_ctx* ctx, int what_mask, int every);
int nq_tspec_detach(nq_ctx* ctx);
int nq_tspec_sample(nq_ctx* ctx);
int nq_tspec_reset(nq_ctx* ctx);
int nq_tspec_info(nq_ctx* ctx, long long* info3);
int nq_tspec_read(nq_ctx* ctx, int which, double* out);

/* Coarse-grained (sub-filter) energy and enstrophy flux maps, formed on the device, single-rank fused
 * contexts only (slab contexts: -4).  G is a real isotropic filter given per shell, G(l, k) = g[b] with the shell rule of
 * nq_diagnostics_binned, an overbar is F^-1[G .].  The planes are those nq_transfer_binned bins: P = psi-hat, Q = the q-hat the
 * tick bins (dual_q contexts: the mean of the two copies), Fu = F[u q], Fv = F[v q], W = the CURRENT phi-hat, J = the J plane of
 * the tick's first products pass (UnCoupledModel, YBJModel: with the stale gradients of quirk Q1).  With u-bar = Re F^-1[-il G P],
 * v-bar = Re F^-1[ik G P], q-bar and its gradient from G Q, phi-bar and its gradient from G W:
 *   NQ_CG_KE   ke_qg       v-bar F^-1[G Fu] - u-bar F^-1[G Fv]                                    CoupledModel, UnCoupledModel, QGModel
 *   NQ_CG_ENS  ens         -(F^-1[G Fu] - u-bar q-bar) q-bar_x - (F^-1[G Fv] - v-bar q-bar) q-bar_y   the same three
 *   NQ_CG_NIW  ke_niw_adv  Re(conj(phi-bar) (F^-1[G J] - u-bar phi-bar_x - v-bar phi-bar_y))      CoupledModel, UnCoupledModel, YBJModel
 * Positive: transfer towards scales below the cut.  For the sharp filter at shell B (g = 1 on b <= B, else 0) the plane mean of a
 * map is the spectral flux through the cut, -sum_{b <= B} of the transfer nq_transfer_binned gives (ke_qg: every B < nx/2; ens,
 * ke_niw_adv: 3 B < nx, while the resolved triple product is alias-free).
 * NYQUIST RULE: every table is zero on the shells b >= nx/2 (-1 otherwise): row ny/2, column nx/2, the passenger row of q-hat and
 * the Hermitian-part rules of the self-mirrored column nx/2 then have nothing in any filtered plane.
 * g: nscales (1..NQ_CG_MAX_SCALES) tables of nb = nq_spectrum_shells(ctx) finite values.  moments[s][m][0..1]: the sum and the sum
 * of squares over the plane of map m (0 ke_qg, 1 ens, 2 ke_niw_adv) at scale s, zero for a map that was not selected, from
 * per-workgroup partials added in a fixed order (no floating-point atomics: two calls are bit-identical).  maps: NULL, or per
 * scale the selected maps in bit order, (ny, nx) doubles each.  A mask the model lacks, a wrong nb, a non-finite entry, a non-zero
 * entry from shell nx/2 on and nx = 8192 (no row plan that holds the maps in registers) are -1 before any launch.  The products
 * pass runs once per call and serves all scales.  The first call allocates the filtered planes (two copies, spectral and mixed
 * space, of up to six half-spectrum and three full planes), the first call with maps != NULL one plane per map of the model;
 * counted by nq_device_bytes, freed with the context; an allocation that fails is -5 and leaves the context as it was.  Reads
 * the state; writes only these buffers and the scratch planes nq_transfer_binned writes.                                       */
enum { NQ_CG_KE = 1, NQ_CG_ENS = 2, NQ_CG_NIW = 4 };
#define NQ_CG_MAX_SCALES 64
int nq_coarse_flux(nq_ctx* ctx, int what_mask, int nscales, const double* g /* nscales x nb */, int nb,
                   double* moments /* nscales x 3 x 2: sum, sum of squares per map; unselected: 0 */,
                   double* maps    /* NULL, or nscales x (selected maps, in bit order) x ny x nx */);

/* Shell-to-shell (giver-receiver) transfers, formed on the device, single-rank fused contexts only (slab
 * contexts: -4).  T(b | Q) is the transfer into receiver shell b with the ADVECTED field restricted to a donor band Q, a real
 * table g_Q per shell (shell rule and NYQUIST RULE of nq_coarse_flux: zero on the shells b >= nx/2, -1 otherwise),
 * G_Q(l, k) = g_Q[b].  The state is the one nq_transfer_binned sees: P = psi-hat, Q-hat = the q-hat the tick bins (dual_q contexts:
 * the mean of the two copies), W = the CURRENT phi-hat, u, v and q_psi those of the tick's products pass.  With
 * q^Q = Re F^-1[G_Q Q-hat], phi^Q = F^-1[G_Q W] and its CURRENT gradients F^-1[ik G_Q W], F^-1[il G_Q W] (also on UnCoupledModel
 * and YBJModel, whose tick uses the stale ones of quirk Q1):
 *   Jq^Q = ik F[u q^Q] + il F[v q^Q]      J^Q = F[u phi^Q_x + v phi^Q_y]      R^Q = i F[phi^Q q_psi]
 *   NQ_S2S_Q    rows [0] Re(conj P Jq^Q), [1] Re(conj Q-hat Jq^Q)     CoupledModel, UnCoupledModel, QGModel
 *   NQ_S2S_ADV  row  [2] Re(conj W J^Q)                               CoupledModel, UnCoupledModel, YBJModel
 *   NQ_S2S_REF  row  [3] Re(conj W R^Q)                               the same three
 * summed over the wavenumbers of shell b: raw sums, no signs and no 1/M^2, as nq_transfer_binned's rows [0..3], on which the sum
 * over bands closes when the tables sum to one below shell nx/2 and the state has nothing from that shell on (every J is linear
 * in the filtered field).  out[band][row][b]; rows that were not selected are zero.  No floating-point atomics and a fixed
 * summation order: two calls are bit-identical, and a band's rows do not depend on the other bands of the call.  A mask the model
 * lacks, nbands outside 1..NQ_S2S_MAX_BANDS, a wrong nb, a non-finite entry, a non-zero entry from shell nx/2 on and nx = 8192
 * (the row kernel of that plan does not fit its 128 registers) are -1 before any launch.  The first call allocates the filtered planes
 * of ONE band (two copies, spectral and mixed space, of one half-spectrum and two full planes), reused from band to band; counted by nq_device_bytes, freed with the context; an
 * allocation that fails is -5 and leaves the context as it was.  Reads the state; writes only these buffers, the products'
 * mixed-space planes (free between steps) and the scratch planes nq_transfer_binned writes.                                   */
#define NQ_S2S_ROWS 4
#define NQ_S2S_MAX_BANDS 64
enum { NQ_S2S_Q = 1, NQ_S2S_ADV = 2, NQ_S2S_REF = 4 };
int nq_shell_transfer(nq_ctx* ctx, int what_mask, int nbands, const double* g /* nbands x nb */, int nb,
                      double* out /* nbands x NQ_S2S_ROWS x nb */);

/* Isotropic co-spectra of the physical fields, formed on the device, single-rank fused contexts only (slab
 * contexts: -4).  fields: 1 to NQ_COSPEC_MAX_FIELDS different ids out of those nq_field_hist takes for the model (Kernel family:
 * NQ_PDF_Q, NQ_PDF_QPSI, NQ_PDF_PHI2 and the NQ_FLOW_* fields; QGModel: NQ_PDF_Q and, with its passive scalar, NQ_PDF_C), with
 * the values nq_field_hist bins: the rows of the last inversion (dual_q contexts: the mean of the two q-hat copies), the CURRENT
 * phi-hat for NQ_FLOW_GRADPHI2.  With F the unnormalised full-plane transform and A_i = F[field i], row i < 3 is
 * sum |A_i|^2 and rows 3, 4, 5 are sum Re(conj A_i A_j) of the pairs (0,1), (0,2), (1,2), each over the wavenumbers of shell b
 * (shell rule of nq_diagnostics_binned; every shell is kept): raw sums, no 1 / M^2; rows of fields the list does not have are
 * zero.  The quadrature part Im(conj A_i A_j) sums to zero over +-k for real fields and is not formed.  Summed over the shells,
 * row (i,j) / M^2 is the plane mean of field i times field j; shell 0 holds the product of the two means.
 * accumulate = 0 zeroes the running sums before this call's rows are added to them, accumulate = 1 adds (the same list as the
 * call that zeroed them, else -1); out: NULL (nothing is downloaded and the host does not wait) or NQ_COSPEC_ROWS x nb doubles,
 * the rows of THIS call.  nq_cospectra_read: the calls in the running sums and the sums (NQ_COSPEC_ROWS x nb; -1 before the first
 * call).  No floating-point atomics and a fixed summation order: two calls are bit-identical.  A null or bad list, a field twice
 * or one the model lacks, a wrong nb, and a list with an NQ_FLOW_* field at nx = 8192 (a thread of that row plan holds one value,
 * a packed pair needs two) are -1 before any launch.  The Kernel family runs the range pass of nq_field_minmax first and scales
 * every field by a power of two before the transforms (exact, taken out again in the bins; nothing of it reaches the host), so
 * fields of very different magnitudes do not share one transform's rounding.  The first call allocates the two tables
 * (2 x NQ_COSPEC_ROWS x nb doubles) and, in the Kernel family, the range pass's partials (6 x 8192 doubles) and six scales,
 * counted by nq_device_bytes, freed with the context; an allocation that fails is -5 and leaves the context as it was.  Reads the
 * state; writes only these tables, the products' mixed-space planes (free between steps) and the scratch planes
 * nq_transfer_binned writes.                                                                                                  */
#define NQ_COSPEC_MAX_FIELDS 3
#define NQ_COSPEC_ROWS 6           /* autos of the list in order, then pairs (0,1), (0,2), (1,2) */
int nq_cospectra(nq_ctx* ctx, int nfields, const int* fields /* NQ_PDF_*, NQ_FLOW_* */, int nb,
                 int accumulate /* 0: zero the device tables first, 1: add; needs the same list */,
                 double* out /* NULL, or rows x nb RAW sums of this call (no 1/M^2) */);
int nq_cospectra_read(nq_ctx* ctx, long long* samples, double* out /* rows x nb running sums */);

/* copy of one ETDRK4 coefficient plane (0:E 1:Eh 2:Q 3:f0 4:fab 5:fc) of equation eq (0: q, (nx, nx/2+1) complex;
 * 1: phi, (nx, nx) complex; 2: QGModel's passive scalar, (nx, nx/2+1)), without the filter folded in; values as the
 * reference's expch, expch_h, Qh, f0, fab, fc (Kernel.py:417-454, QGModel.py:426-461).                           */
int nq_get_coeff(nq_ctx* ctx, int eq, int which, double* out_cplx);

/* The reference evaluates Qh, f0, fab, fc as the mean of 32 points on the unit circle around c dt (Kernel.py:424-433).  Where
 * c dt lies within delta of minus one of those points, one term is a removable singularity evaluated by cancellation and the
 * reference's value is its libm's rounding error amplified by eps / distance^3: to be identical there, those entries have to
 * come from the same numpy expression.  nq_coeff_near_contour lists them for equation eq (as nq_get_coeff; on a slab context:
 * this rank's columns): up to cap (l, k) pairs, k a GLOBAL column index; returns how many there are (call again with a larger cap
 * if that exceeds cap), negative on error.  nq_coeff_patch replaces Qh, f0, fab, fc at n entries with vals (n x 4 complex128,
 * the reference's values WITHOUT the filter; the library folds its filter in) in every plane set of that equation, and
 * nq_get_coeff returns them from then on.  The host side calls both once, right after nq_create (niwqg_amd/_etdrk4.py).     */
int nq_coeff_near_contour(nq_ctx* ctx, int eq, double delta, int cap, int* l_out, int* k_out);
int nq_coeff_patch(nq_ctx* ctx, int eq, int n, const int* l, const int* k, const double* vals_cplx);

/* ---- the q update beside the wave-PV row kernel (single rank, CoupledModel) ----------
 * At 4096^2 the step runs the q update (memory-bound) on a second stream beside the wave-PV row kernel (bound by its
 * transforms), whose persistent grid leaves some CUs free for it.  NIWQG_AMD_OVERLAP_CUS is read once, by nq_create: unset =
 * the measured default, 0 = the serial step, n > 0 = free about n CUs (also honoured at 8192^2, where the default is the serial
 * step).  Results are bit-identical either way.  nq_overlap_grid is pure host arithmetic: the smallest persistent grid for nb
 * row blocks that needs no more rounds than `cus` workgroups would.  nq_overlap_default_cus: the default for an nx^2 grid
 * (0 = serial).  nq_overlap_info: out3 = {CUs left free, wave-PV grid, CUs of the device} of this context, all 0 when its
 * step is the serial one.                                                                                                 */
int nq_overlap_grid(int nb, int cus);
int nq_overlap_default_cus(int nx);
int nq_overlap_info(const nq_ctx* ctx, int* out3);

/* ---- grids of the persistent row kernels ------------------------------------------------------------------
 * The products and the wave-PV row kernels of 4096- and 8192-point rows are persistent: g workgroups walk nb row blocks in
 * ceil(nb / g) rounds, g from the CU count of the device.  NIWQG_AMD_NUM_CU=n (read by nq_create, 1 <= n <= the device's count,
 * anything else is refused) sizes those grids as if the device had n CUs; it masks no CU and exists so that tests can run
 * grids that do not divide their rows.  nq_row_grid_info: out6 = {CU count in use, CUs reserved on a slab link
 * (NIWQG_AMD_SLAB_RESERVE_CUS), products grid, products row blocks, wave-PV grid, wave-PV row blocks} of a launch over all
 * rows of this context, from the same arithmetic the launches use.                                                         */
int nq_row_grid_info(const nq_ctx* ctx, int* out6);

/* ---- 1-D slab decomposition over nranks GPUs (one process per GPU) -----------------
 * Rows of the mixed-space planes are split over ranks on the "x side" (row kernels), columns on the "y side"
 * (spectral kernels).  Arrays that cross together form an exchange group g = 0..3; each group has an x-side
 * and a y-side buffer of nq_group_elems() complex128 elements, both cut into nranks equal blocks, so that ONE
 * all_to_all_single(recv = other side, send = this side) moves the group.  Two ways to drive a step: nq_slab_step
 * (below: the library runs the phases AND issues the exchanges itself over the link the context was given -- the
 * product path), or phase by phase with nq_phase, where the CALLER owns the collectives (torch.distributed / RCCL) and
 * the library only runs the phases in between, on the stream it was given (stream == NULL: a private stream the
 * library creates -- then the caller must order its collectives against nq_stream()).
 *   buffers[2g], buffers[2g+1] : x-side and y-side device buffers of group g (may be NULL for empty groups)
 *   buffers[8]                 : 64 doubles for the per-step budget sums (summed over ranks by the caller)
 * buffers == NULL: the library allocates all of them itself (nq_group_buffers / nq_reduce_buffer give the pointers).   */
long long nq_group_elems(const nq_params* p, int nranks, int group);
int nq_create_slab(const nq_params* p, const double* kk, const double* ll, const double* filtr,
                   const double* contour, int device, int nranks, int rank, void* const* buffers, void* stream,
                   nq_ctx** out);
int nq_slab_info(const nq_ctx* ctx, int* info8);
int nq_group_buffers(nq_ctx* ctx, int group, void** x_side, void** y_side, long long* elems);
/* local column slab of qh (which 0: (ny, local half-spectrum columns)) or phih (which 1: (ny, nx/nranks)); download also
 * which 2: ph, 3: qwh, 4: the second copy of qh of a dual_q context, 5: ch of QGModel's passive scalar, 6: the q-hat the
 * last step's fourth stage was evaluated at (NQ_F_QH_STAGE4) (half-spectrum slabs like qh), 7: the phih of that stage (like
 * which 1), 8: the second copy of qh of that stage (like which 4), 9-12: nq_tick_snapshot's qh, phih, second copy of qh, qwh */
int nq_upload_spectral(nq_ctx* ctx, int which, const double* host);
int nq_download_spectral(nq_ctx* ctx, int which, double* host);
enum {
  NQ_PH_PRODUCTS = 0,      /* rows: nonlinear products (Kernel.py:471-486,:457-469,:332)   then exchange group 0 (x->y) */
  NQ_PH_UPDATE = 1,        /* spectral: N_q, N_phi, ETDRK4 stage update                    then group 1 (y->x) [+3]    */
  NQ_PH_WAVEPV = 2,        /* rows: wave-PV sources (CoupledModel.py:59-88)                then group 2 (x->y)         */
  NQ_PH_INVERT = 3,        /* spectral: psi inversion (CoupledModel.py:75-97)              then group 3 (y->x)         */
  NQ_PH_EMIT_PHI = 4,      /* after uploading phih (set_phi)                               then group 1 (y->x)         */
  NQ_PH_INVERT_NOW = 5,    /* inversion of the current qh (set_q)                          then group 3 (y->x)         */
  NQ_PH_BUDGET_SUMS = 6,   /* local budget sums of the finished step                       then all-reduce buffer 0    */
  NQ_PH_BUDGET_FINISH = 7  /* Ke, Pw, Kw increments from the reduced sums (Kernel.py:390-392)                          */
};
int nq_phase(nq_ctx* ctx, int phase, int stage);
int nq_reduce_buffer(nq_ctx* ctx, int which, void** device_ptr, int* count);
/* host copies of those blocks (which 0..3 as above, 4 / 5: the spectral / physical half of the diagnostic sums, 16 doubles
 * each): read, sum over ranks by any means, write back -- what an all-reduce callback does */
int nq_reduce_read(nq_ctx* ctx, int which, double* host_out);
int nq_reduce_write(nq_ctx* ctx, int which, const double* host_in);

/* ---- the slab step INSIDE the library: one host call per nsteps, exchanges issued by the library ------------------
 * nq_slab_step runs the phase sequence of nq_phase itself and moves the exchange groups over the link the context
 * was given, on its own exchange stream, chunk by chunk: every group is cut into nchunks row chunks; for an x->y group
 * the row kernel of chunk i+1 runs while chunk i is on the wire, for a y->x group the row kernel of chunk i starts as
 * soon as chunk i has arrived; the q update runs under the transfer of the phi group; the budget sums are all-reduced
 * once per step and not at all when budgets are off.  Links:
 *   nq_comm_init          RCCL: grouped ncclSend/ncclRecv per chunk + ncclAllReduce, communicator made from a
 *                         128-byte unique id (rank 0: nq_comm_unique_id; hand it to the others by any means, e.g.
 *                         torch.distributed broadcast).  librccl is taken from the process (dlopen), not linked.
 *   nq_slab_attach_peers  all nranks contexts live in THIS process on one device (the one-GPU test double): the same
 *                         choreography of streams and events, device-to-device copies instead of the wire.  The step is
 *                         then driven through the rank-0 context and advances all of them.
 *   nq_slab_set_callbacks the caller moves the data: exchange(user, group, to_y) and allreduce(user, which) are called
 *                         with the compute stream drained and must be complete on return (gloo / host staging).
 * nq_slab_put_rows + nq_slab_commit: Kernel.set_q / set_phi (Kernel.py:520-551) from this rank's ROWS of the physical
 * field (nloc rows of nx values, real / complex): row transform on the device (put_rows, local), then exchange, column
 * transform and the phases of the single-rank calls (commit, collective) -- no rank ever holds or transforms the whole plane.
 * nq_slab_get_rows: this rank's rows (nloc, nx) of a physical field (NQ_F_Q, _P, _U, _V, _QW, _C real; _PHI, _PHIX,
 * _PHIY complex) from the mixed-space rows the last step left on the x side (q_psi = q - qw: two calls).
 * nq_comm_probe: 0 when this process can resolve librccl (load only, no communicator) -- every rank calls it and the
 * ranks agree on the outcome BEFORE rank 0 asks for an id, so that nobody is left alone in a collective. */
typedef int (*nq_exchange_fn)(void* user, int group, int to_y);
typedef int (*nq_allreduce_fn)(void* user, int which);      /* which: as nq_reduce_read: 0..3, and 4 / 5 = the spectral /
                                                              * physical half of the diagnostic sums, 16 doubles each */
int nq_comm_probe(void);
int nq_comm_unique_id(void* out128);
int nq_comm_init(nq_ctx* ctx, const void* id128, int nranks, int rank);
int nq_slab_attach_peers(nq_ctx* const* ctxs, int nranks);
int nq_slab_set_callbacks(nq_ctx* ctx, nq_exchange_fn exchange, nq_allreduce_fn allreduce, void* user);
/* Measurement aid (bench.py --rank-of P): the context is ONE rank of its nranks-rank decomposition and runs alone -- every
 * stream, event, row chunk and kernel launch of a real rank, but only the rank's own block crosses (device copy) and nothing
 * is all-reduced.  The fields are not a simulation; what it gives is a rank's compute time without the exchange. */
int nq_slab_set_null_link(nq_ctx* ctx);
/* YBJModel on more than one rank has a fifth exchange group (4, y -> x, shaped like group 1: the stage results whose
 * gradients the next stage reads, YBJModel.py:52-87).  The library owns its buffers unless the caller hands over two
 * device buffers of nq_group_elems(p, nranks, 4) complex elements here (callback link: the caller moves them). */
int nq_slab_set_stage_buffers(nq_ctx* ctx, void* x_side, void* y_side);
int nq_slab_config(nq_ctx* ctx, int nchunks);               /* 1, 2, 4 or 8; reduced if the local rows do not divide */
int nq_slab_step(nq_ctx* ctx, int nsteps);
int nq_slab_put_rows(nq_ctx* ctx, int which /* 0: q, 1: phi, 2: c */, const double* rows);   /* local: rows -> x side */
int nq_slab_commit(nq_ctx* ctx, int which);   /* collective: the rest of set_q / set_phi (rank-0 context in peers mode);
                                                  which 2: Kernel._invert on the current state, nothing uploaded;
                                                  which 3: the rest of QGModel.set_c (QGModel.py:522-534) after put_rows(2) */
int nq_slab_get_rows(nq_ctx* ctx, int field_id, double* rows_out);
/* The whole-plane calls of the class API on a slab model (Kernel.fft, jacobian_psi_q, jacobian_psi_phi,
 * CoupledModel.jacobian_phic_phi): nq_slab_spectral (collective) runs the row kernel of the current state -- or takes
 * the rows last given to nq_slab_put_rows -- through exchange and column transform into a scratch column slab;
 * nq_slab_spectral_read (local) copies this rank's slab out: (nx, wh) complex for the half-spectrum results, (nx, wf)
 * otherwise (wh, wf: nq_slab_info).  what 0 / 1: F[u q] / F[v q] (half); 2: F[u phix + v phiy] (full, [0,0] as
 * computed); 3: F[i phi q_psi] (full); 4: F[Re i(phix* phiy - phiy* phix)] (half, coupled model); 5 / 6: forward
 * transform of the real / complex rows of nq_slab_put_rows(0 / 1) (half / full).  The model state is not touched. */
int nq_slab_spectral(nq_ctx* ctx, int what);
int nq_slab_spectral_read(nq_ctx* ctx, int half, double* out_cplx);
/* nq_diagnostics of a slab-decomposed simulation: the same 32 sums, every rank's part summed over the ranks (collective);
 * nq_slab_local_max: max|u|, max|v|, max|phi| over this rank's rows (the caller takes the max over ranks for the CFL) */
int nq_slab_diagnostics(nq_ctx* ctx, double* out32);
/* nq_diagnostics_binned of a slab-decomposed simulation (collective): every context bins its own columns (global k from its
 * first column), the products passes exchange as the tick's do, and the contexts of this process are summed in rank order:
 * peer ranks in one process give the whole (32, nb) array; with one rank per process the result is that rank's part, which
 * the caller gathers (all_gather) and sums in rank order, so that every rank holds the same array. */
int nq_slab_diagnostics_binned(nq_ctx* ctx, int nb, double* out);
/* nq_transfer_binned of a slab-decomposed simulation (collective): every context bins its own columns, the products passes
 * exchange as the tick's do, and the ranks are summed in rank order exactly as nq_slab_diagnostics_binned does
 * (NQ_TRANSFER_ROWS x nb doubles; with one rank per process the caller gathers and sums the parts in rank order). */
int nq_slab_transfer_binned(nq_ctx* ctx, int nb, double* out);
int nq_slab_local_max(nq_ctx* ctx, double* out3);
/* counters since the last reset: out[0] host calls of nq_slab_step, [1] steps, [2] exchange chunks issued, [3] bytes this
 * rank sent to OTHER ranks, [4] milliseconds the exchange stream spent in exchanges (HIP events; 0 unless timing was
 * switched on with reset = 2), [5] nchunks in use.  reset = 2 switches the per-exchange event timing ON and it stays on (two events
 * per exchange chunk and per all-reduce, at most 16384 timed pairs each -- later ones go untimed) until a call with reset = 1,
 * which zeroes the counters and switches it off again. */
int nq_slab_counters(nq_ctx* ctx, double* out6, int reset);
/* out2[0]: milliseconds the exchange stream spent in the all-reduces of the steps since timing was switched on
 * (nq_slab_counters with reset = 2), out2[1]: how many all-reduces that was.  Read before the call that resets. */
int nq_slab_allreduce_ms(nq_ctx* ctx, double* out2);

/* timing of the hot loop with HIP events on the context's stream */
int nq_timer_start(nq_ctx* ctx);
int nq_timer_stop(nq_ctx* ctx, float* elapsed_ms);
/* 16 event slots on the context's stream: record marks between asynchronous nq_step calls, read the time between
 * two marks afterwards (blocks until slot_b has passed) */
int nq_event_record(nq_ctx* ctx, int slot);
int nq_event_elapsed(nq_ctx* ctx, int slot_a, int slot_b, float* elapsed_ms);
/* Per-kernel timing with HIP events on the context's stream.  While enabled, every launch of the
 * selected kernel class inside nq_step is bracketed by an event pair (cost ~2 us per launch).
 * class: 0 x_products, 1 x_wavepv, 2 s_q, 3 s_phi, 4 s_invert, 5 y_A (all A sub-passes);
 * 6 the zeta row pass and 7 the ray step of ray mode (nq_particles_rays), 8 the step of stretch mode (nq_particles_tangent),
 * read with nq_profile_read           */
/* best of `reps` timed launches of a 1-read + 1-write stream copy of `bytes` bytes (16 B per lane, grid-stride), in GB/s
 * of bytes moved (read + written): the copy rate of THIS device, bench.py's second roofline denominator */
int nq_stream_copy_gbs(nq_ctx* ctx, long long bytes, int reps, double* gbs_out);
int nq_profile_enable(nq_ctx* ctx, int kernel_class);     /* -1 disables, -2 brackets every class */
/* bracket only every stride-th launch of the enabled class(es) (>= 1; 1 = every launch): keeps the cost of measuring a kernel
 * live inside a timed region below 1 % (an event pair costs the stream ~9 us) */
int nq_profile_stride(nq_ctx* ctx, int stride);
int nq_profile_read(nq_ctx* ctx, int* launches, float* total_ms);   /* synchronises, then resets */
int nq_profile_read_all(nq_ctx* ctx, int* launches6, float* total_ms6);   /* per class, after nq_profile_enable(-2) */
/* bytes of device memory held by the context */
long long nq_device_bytes(const nq_ctx* ctx);
/* stream handle (hipStream_t) so that callers can order their own work */
void* nq_stream(nq_ctx* ctx);

/* ---- the any-size engine: grids without a fused plan -----------------------------------------------------------------------
 * The reference takes any nx (niwqg/Kernel.py:100-103; numpy.fft transforms any length, :562-566; QGModel.py:93-96, :551-552).
 * The fused step above exists for powers of two in [64, 8192].  For every other even nx in [4, 8192] the model classes run the
 * reference's own sequence of whole-plane operations (niwqg_amd/_anysize.py) on device planes through these calls: 1-D transforms
 * of any length along either axis (Bluestein's chirp-z identity on the power-of-two row engine), element-wise operations,
 * deterministic reductions.  Planes are contiguous arrays of complex128 owned by the engine; everything is asynchronous on the
 * engine's stream except the calls that return data.  Same return codes as above; nq_any_last_error for the text. */
typedef struct nq_any nq_any;
enum {  /* nq_any_ew: d = ... element by element; s0, s1, s2 complex scalars (scalars6 = re, im of each; NULL: s0 = 1, s1 = s2 = 0) */
  NQ_EW_COPY = 0,      /* a                                   */
  NQ_EW_MUL = 1,       /* s0 a b                              */
  NQ_EW_MULCONJ = 2,   /* s0 conj(a) b                        */
  NQ_EW_AXPBY = 3,     /* s0 a + s1 b                         */
  NQ_EW_AXPBYPCZ = 4,  /* s0 a + s1 b + s2 c                  */
  NQ_EW_REAL = 5,      /* Re a (imaginary part zero): numpy's .real kept as a complex plane */
  NQ_EW_ABS2 = 6,      /* |a|^2                               */
  NQ_EW_SCALE = 7,     /* s0 a                                */
  NQ_EW_CONJ = 8,      /* conj(a)                             */
  NQ_EW_ADDS = 9,      /* a + s0                              */
  NQ_EW_IMAG = 10,     /* Im a (as a real value)              */
  NQ_EW_MULADD = 11,   /* s0 a b + s1 c                       */
  NQ_EW_FILL = 12      /* s0 (a is not read)                  */
};
enum {  /* nq_any_reduce: out2 = (re, im) */
  NQ_RD_SUM = 0, NQ_RD_SUMABS2 = 1, NQ_RD_DOT = 2 /* sum a b */, NQ_RD_DOTC = 3 /* sum conj(a) b */, NQ_RD_MAXABS = 4,
  NQ_RD_WSUMABS2 = 5 /* sum Re(b) |a|^2 */, NQ_RD_MAXABSRE = 6 /* max |Re a| */
};
int nq_any_create(int device, nq_any** out);
int nq_any_destroy(nq_any* eng);
const char* nq_any_last_error(const nq_any* eng);
int nq_any_sync(nq_any* eng);
long long nq_any_device_bytes(const nq_any* eng);
int nq_any_alloc(nq_any* eng, long long elems, void** plane);                 /* zero-filled */
int nq_any_free(nq_any* eng, void* plane, long long elems);
int nq_any_upload(nq_any* eng, void* plane, const double* host_cplx, long long elems);
int nq_any_download(nq_any* eng, const void* plane, double* host_cplx, long long elems);
/* numpy.fft.fft / ifft along one axis of a (rows, cols) plane (axis 1: the contiguous index); dst may be src.  Transform lengths:
 * 1 to 8192, and 16384; any other length returns non-zero with nq_any_last_error set */
int nq_any_fft(nq_any* eng, void* dst, const void* src, int rows, int cols, int axis, int inverse);
/* operands the op does not read may be NULL; d may alias any operand */
int nq_any_ew(nq_any* eng, int op, void* d, const void* a, const void* b, const void* c, long long elems, const double* scalars6);
int nq_any_reduce(nq_any* eng, int op, const void* a, const void* b, long long elems, double* out2);
/* (rows, n/2+1) -> (rows, n): full[l, n-k] = conj(half[-l, k]); project != 0 first takes the Hermitian part (in l) of columns 0
 * and n/2, which is all numpy.fft.irfft2 sees of them (QGModel.py:552) */
int nq_any_expand_half(nq_any* eng, void* full, const void* half, int rows, int n, int project);
int nq_any_take_cols(nq_any* eng, void* dst, const void* src, int rows, int src_cols, int dst_cols);
int nq_any_set_elem(nq_any* eng, void* plane, long long index, double re, double im);
/* isotropic shell sums of the REAL part of a complex plane: layout 0 a full (rows, rows) plane in fftfreq order, 1 an rfft half
 * plane (rows, rows/2 + 1); out: nb = round(rows / sqrt 2) + 1 doubles; the integer shell rule and the deterministic kernel of
 * nq_diagnostics_binned (no weights: the caller forms each element's term, half planes with their weight folded in).    */
int nq_any_bin(nq_any* eng, const void* plane, int rows, int cols, int layout, int nb, double* out);
/* PDFs on engine planes (nq_field_hist's bin rule and counting kernel): what 0 = Re of the plane, 1 = |a|^2, over `elems` complex
 * values.  nq_any_hist: out[bins + 3] = the bins (1..1024), below, above, NaN.  nq_any_hist2, the joint form: bins (1..128) per
 * axis, lo2 / hi2 the ranges of a and b, out[bins^2 + 1] = [index of b][index of a], then the points with either value out of
 * range or NaN.  nq_any_minmax: out2 = exact minimum and maximum (both NaN when any value is).  Synchronous, like nq_any_bin. */
int nq_any_hist(nq_any* eng, const void* plane, long long elems, int what, double lo, double hi, int bins, unsigned long long* out);
int nq_any_hist2(nq_any* eng, const void* plane_a, const void* plane_b, long long elems, int what_a, int what_b, const double* lo2,
                 const double* hi2, int bins, unsigned long long* out);
int nq_any_minmax(nq_any* eng, const void* plane, long long elems, int what, double* out2);
/* Structure functions on engine planes (nq_structure above: the same columns, the plane kernel of its QGModel route): (rows, cols)
 * complex planes, what[i] = 0: the real part of plane i, 2: its complex value (the NQ_SF_PHI columns; one plane at most);
 * increments along a row, separations in [1, cols - 1].  out: the raw sums of this one state, nsep x (9 nfields + ntriples). */
int nq_any_increments(nq_any* eng, int nfields, const void* const* planes, const int* what /* 0 Re, 2 complex */, int rows, int cols,
                      int nsep, const int* seps, int ntriples, const int* triples, double* out);
/* The same at two-dimensional separations (nq_structure2 above: vectors, projection and return codes; r_x in [-(cols - 1),
 * cols - 1], r_y in [0, rows - 1]).  out: the raw sums of this one state, nvec x (9 nfields + ntriples), in the caller's order. */
int nq_any_increments2(nq_any* eng, int nfields, const void* const* planes, const int* what /* 0 Re, 2 complex */, int rows, int cols,
                       int nvec, const int* vecs, const double* proj, int proj_a, int proj_b, int ntriples, const int* triples,
                       double* out);
/* PDFs of the increments on engine planes (nq_increment_hist2 above: vectors, projection, ranges, bin rule and return codes;
 * planes and what as nq_any_increments2 takes them).  out: the counts of this one state, nvec x nfields x (bins + 3).  An
 * x-separation r is the vector (r, 0).  Synchronous. */
int nq_any_increment_hist(nq_any* eng, int nfields, const void* const* planes, const int* what /* 0 Re, 2 complex */, int rows, int cols,
                          int nvec, const int* vecs, const double* proj, int proj_a, int proj_b, const double* lo, const double* hi,
                          int bins, unsigned long long* out);
/* Vortex census on engine planes (nq_vortex_census above: set, components, labels, table, capacity and return codes).  planes:
 * 1 to 3 different (rows, cols) complex planes whose REAL parts are the fields; rows, cols: even, from 4 to 16384, no power of two
 * or multiple of 64 needed.  info: the 7 entries of nq_vortex_read; table: room for capacity x (NQ_VX_COLS + nplanes), the first
 * info[1] rows are written; labels (or NULL): rows x cols.  Synchronous; its device buffers live for the call. */
int nq_any_components(nq_any* eng, int nplanes, const void* const* planes, int rows, int cols, int crit, int mode, double threshold,
                      int connectivity, int capacity, long long* info, long long* table, int* labels);
/* Lagrangian particles on engine planes (the RK4 step and interpolation of nq_particles_attach above): pos holds n complex
 * x + i y; U0, U1 and plane are (nx, nx) complex planes, velocity planes as u + i v; out[i] = plane at pos[i] (real and
 * imaginary parts interpolated each) */
int nq_any_particles_rk4(nq_any* eng, void* pos, int n, const void* U0, const void* U1, int nx, double Lx, double Ly, double U,
                         double dt);
int nq_any_interp(nq_any* eng, void* out, const void* plane, const void* pos, int n, int nx, double Lx, double Ly);
/* Drifter mode on engine planes (nq_particles_wave above): the step from time t with P0, P1 the (nx, nx) physical phi planes beside
 * U0, U1 (amplitude finite and > 0); out[i] = amplitude phi(pos[i]) e^{-i f0 t} */
int nq_any_particles_rk4_wave(nq_any* eng, void* pos, int n, const void* U0, const void* U1, const void* P0, const void* P1, int nx,
                              double Lx, double Ly, double U, double dt, double amplitude, double f0, double t);
int nq_any_interp_wave(nq_any* eng, void* out, const void* phi, const void* pos, int n, int nx, double Lx, double Ly, double amplitude,
                       double f0, double t);
/* Ray mode on engine planes (nq_particles_rays above): one step of the rays pos[i] = x + i y, wv[i] = k + i l; U0, U1 the velocity
 * planes u + i v and Z0, Z1 complex (nx, nx) planes with zeta in the real part (every engine plane is complex: a real layout
 * would cost the engine a conversion pass per step), of the state the step starts from and of the state after it (U0 == U1 or
 * Z0 == Z1: steady).  out[i] = omega at the rays from U, Z (imaginary part 0). */
int nq_any_particles_rk4_rays(nq_any* eng, void* pos, void* wv, int n, const void* U0, const void* U1, const void* Z0, const void* Z1,
                              int nx, double Lx, double Ly, double U, double eta, double dt);
int nq_any_interp_omega(nq_any* eng, void* out, const void* U, const void* Z, const void* pos, const void* wv, int n, int nx, double Lx,
                        double Ly, double Ub, double eta);
/* Stretch mode on engine planes (nq_particles_tangent above): one step of pos[i] = x + i y and of the columns of F, fa[i] = f11 + i f21
 * and fb[i] = f12 + i f22; U0, U1 the velocity planes u + i v (U0 == U1: steady); with the wave, P0, P1 the physical phi planes and
 * the step's start time t (amplitude finite and > 0): drifter mode's velocity and its gradient.  tangent_value: out[i] = ln sigma_1
 * (which 0) or det F (1) of (fa[i], fb[i]), imaginary part 0. */
int nq_any_particles_rk4_tangent(nq_any* eng, void* pos, void* fa, void* fb, int n, const void* U0, const void* U1, int nx, double Lx,
                                 double Ly, double U, double dt);
int nq_any_particles_rk4_wave_tangent(nq_any* eng, void* pos, void* fa, void* fb, int n, const void* U0, const void* U1, const void* P0,
                                      const void* P1, int nx, double Lx, double Ly, double U, double dt, double amplitude, double f0,
                                      double t);
int nq_any_tangent_value(nq_any* eng, void* out, const void* fa, const void* fb, int n, int which);
/* Stochastic forcing on engine planes (nq_forcing_attach above: the same generator, counters and Hermitian rule):
 * plane += sqrt_dt Re(amp_plane) xi(.; s).  layout 0: (rows, rows/2+1) half spectrum under the q rule; 1: full (rows, rows) plane,
 * independent values of `stream`; 2: full plane, the Hermitian extension of the q rule (columns k > rows/2 take the conjugate of
 * (-l, -k)).  work_in_plane (NULL: none; it may be `plane` itself, read before the increment D) and work_out2 go together:
 * work_out2 = {sum w Re(conj(work_in) D), sum w |D|^2} / M^2, w the half-spectrum weights on layout 0, else 1.               */
int nq_any_forcing(nq_any* eng, void* plane, const void* amp_plane, int rows, int cols, int layout, unsigned long long seed, long long s,
                   int stream, double sqrt_dt, const void* work_in_plane, double* work_out2);
/* The recorder on engine planes (nq_freq_attach above: the same kernels).  record: one record of nf planes into slot `slot` of their
 * rings, one launch; planes[f] is (rows, cols[f]); full[f] != 0: the block takes columns 0..kmax and -kmax..-1 of a full plane
 * (cols[f] == rows), else columns 0..kmax; rings[f]: [length][2 kmax + 1][2 kmax + 1 or kmax + 1] complex.  spectrum: the table of
 * the T records of one ring, the oldest in slot `first`; full / kappa: 1, 0 (phi), 0, 0 (q), 0, 1 (psi); out (T, nb).          */
int nq_any_freq_record(nq_any* eng, int nf, void* const* rings, const void* const* planes, const int* cols, const int* full, int rows, int kmax,
                       int length, int slot);
int nq_any_freq_spectrum(nq_any* eng, const void* ring, int rows, int kmax, int full, int kappa, int length, int first, int T,
                         const double* window, int demean, double dk, int nb, double* out);
/* Lagrangian spectra and dispersion on engine planes (nq_lagr_spectrum above: the same kernels and tables).  The any-size path
 * keeps one plane per record and name: re[r], im[r] are the device addresses of particle 0's real and imaginary part in record r,
 * oldest first (im NULL: a real series; for the value of a complex plane: its address, and that plus 8 bytes), stride the doubles
 * between particles (2 on a complex plane); pos[r]: the (1, n) plane x + i y of record r.  The work memory lives for the call.   */
int nq_any_lagr_spectrum(nq_any* eng, int n, int T, const void* const* re, const void* const* im, int stride, int nfft, const double* window,
                         int demean, int G, const int* order, const int* offsets, int chunk, double* out);
int nq_any_lagr_dispersion(nq_any* eng, int n, int T, const void* const* pos, int G, const int* order, const int* offsets, int npairs,
                           const int* pi, const int* pj, double* out, double* out_pairs);
/* nq_lagr_stretching on engine planes: f[r][4] = the device addresses of particle 0's f11, f12, f21, f22 in record r (T x 4
 * pointers, oldest first), stride the doubles between particles; out[T][G][4].                                               */
int nq_any_lagr_stretching(nq_any* eng, int n, int T, const void* const* f, int stride, int G, const int* order, const int* offsets,
                           double* out);
/* One sample of the averages on engine planes (nq_avg_attach above: the same rule, QGModel's kernel).  src[i]: complex planes of
 * `elems` values read as what[i] (0: Re, 1: |a|^2, 2: the complex value, at most once and in no product) and added to sums[i]
 * (elems doubles; what 2: elems complex); pairs: 2 x nproducts indices into src, psums[p] += the product.  Not synchronous.  */
int nq_any_moments(nq_any* eng, long long elems, int nfields, const void* const* src, const int* what, void* const* sums, int nproducts,
                   const int* pairs, void* const* psums);
/* E = exp(c dt), Eh = exp(c dt / 2), Q, f0, fab, fc of the linear operator c(l, k) on a (n, cols) plane, WITHOUT the filter
 * (Kernel.py:417-454, QGModel.py:426-466); eq 0: q of the Kernel family, 1: phi, 2: QGModel's q (beta term), 3: its passive
 * scalar.  The entries within delta of the contour are listed (near_*; at most cap) for the host to recompute exactly as the
 * reference does (niwqg_amd/_etdrk4.py) and hand back through nq_any_etdrk4_patch (vals: count x 4 complex: Qh, f0, fab, fc). */
int nq_any_etdrk4(nq_any* eng, int eq, const nq_params* p, const double* kk, const double* ll, const double* contour32, int n, int cols,
                  void* const* out6, double delta, int cap, int* near_count, int* near_l, int* near_k);
int nq_any_etdrk4_patch(nq_any* eng, void* const* out6, int cols, int count, const int* l, const int* k, const double* vals);

#ifdef __cplusplus
}
#endif
#endif
