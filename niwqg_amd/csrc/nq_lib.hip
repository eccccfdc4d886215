// niwqg_amd: context, precompute kernels and the C ABI (include/niwqg_amd.h).
// gfx950 only; build: hipcc --offload-arch=gfx950 -O3 -shared -fPIC nq_lib.hip -o libniwqg_amd.so
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/niwqg_amd.h"
#include "nq_step.hpp"
#include "nq_anysize.hpp"
#include "nq_particles.hpp"
#include "nq_hist.hpp"
#include "nq_avg.hpp"
#include "nq_flow.hpp"
#include "nq_sf.hpp"
#include "nq_sf2.hpp"
#include "nq_ipdf.hpp"
#include "nq_vortex.hpp"
#include "nq_forcing.hpp"

using namespace nq;

static thread_local std::string g_last_error;

#define NQ_FAIL(ctx, code, ...)                                  \
  do {                                                           \
    char buf_[512];                                              \
    snprintf(buf_, sizeof(buf_), __VA_ARGS__);                   \
    g_last_error = buf_;                                         \
    if (ctx) (ctx)->err = buf_;                                  \
    return (code);                                               \
  } while (0)

#define HIPCHK(ctx, call)                                                                          \
  do {                                                                                             \
    hipError_t e_ = (call);                                                                        \
    if (e_ != hipSuccess) NQ_FAIL(ctx, -5, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

#define NQ_SINGLE_RANK(c, what)                                                              \
  do {                                                                                       \
    if (!(c)) NQ_FAIL((nq_ctx*)nullptr, -1, what ": null context");                          \
    if ((c)->P != 1) NQ_FAIL(c, -4, what ": not available on a slab context (nranks > 1)");  \
  } while (0)

// ---------------------------------------------------------------------------------------------
struct EqState {           // ETDRK4 state of one equation
  cd* y[3] = {nullptr, nullptr, nullptr};   // rotating: y[cur] = y(t_n)
  int cur = 0;
  cd *fn0 = nullptr, *fna = nullptr;
  cd* coef[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // E, Eh, Q, f0, fab, fc (filter folded in)
};                                                                       // (rows 0..N/2 only when nq_ctx::cmirror is set)

// ---- step attachments: what rides on every step of a single-rank context -------------------------
// Device memory an attachment allocated after the context was built: att_alloc adds to it, att_release gives it all back.
struct DevMark { size_t n = 0; long long bytes = 0; };
struct DevOwned {
  std::vector<void*> mem;
  long long bytes = 0;                     // what nq_device_bytes counts for this attachment
  DevMark mark() const { return {mem.size(), bytes}; }
  // frees what was allocated since `to` (a default DevMark: everything); returns the bytes no longer counted
  long long rollback(DevMark to = DevMark()) {
    for (; mem.size() > to.n; mem.pop_back()) (void)hipFree(mem.back());
    const long long freed = bytes - to.bytes;
    bytes = to.bytes;
    return freed;
  }
  // frees one allocation of `nbytes` out of order (no mark may be outstanding); returns the bytes no longer counted
  long long release(void* p, long long nbytes) {
    for (size_t i = 0; i < mem.size(); ++i)
      if (mem[i] == p) {
        (void)hipFree(p);
        mem.erase(mem.begin() + i);
        bytes -= nbytes;
        return nbytes;
      }
    return 0;
  }
};
// Host bookkeeping of a ring of `cap` records, one after every `every`-th step (every == 0: never).
struct RecordRing {
  int cap = 0, every = 0;
  long long count = 0, steps = 0;          // records written, steps since attach
  std::vector<long long> ring_step;        // steps since attach of each slot
  void init(int cap_, int every_) { cap = cap_; every = every_; ring_step.assign((size_t)cap_, 0); }
  int slot() const { return (int)(count % cap); }                          // where the next record goes
  long long held() const { return count < cap ? count : cap; }
  int oldest(long long r) const { return (int)((count - held() + r) % cap); }   // slot of the r-th held record, oldest first
  void wrote() { ring_step[slot()] = steps; ++count; }
  bool tick() { ++steps; return every > 0 && steps % every == 0; }        // one step done: is a record due?
};
struct NqParticles : DevOwned {            // Lagrangian particles (section 5g)
  int n = 0;
  double *x = nullptr, *y = nullptr;       // unwrapped positions
  cd* uv[2] = {nullptr, nullptr};          // velocity planes (u, v) interleaved, ping-pong: uv[cur] is the current state's
  int cur = 0;
  bool u0 = false;                         // uv[cur] is the velocity of the state the next step starts from
  RecordRing rg;                           // records of (2 + ncol) x n doubles
  int ncol = 0;
  std::vector<int> names;                  // record columns (PT_*; PT_PHI takes two: real, imaginary part)
  double* ring = nullptr;
  double* qplane = nullptr;                // physical q (PT_Q), allocated when first needed
  cd* phiplane = nullptr;                  // physical phi (PT_PHI), idem
  double* samp = nullptr;                  // nq_particles_sample's output columns (4 x n), idem
  // drifter mode (section 5s): the particles also move through a phi e^{-i f0 t}
  bool wave = false;
  double wa = 1.0, wf0 = 0.0, wt0 = 0.0;   // amplitude; the clock of "uw" / "vw" and of the mode: t_s = wt0 + s dt
  cd* wphi[2] = {nullptr, nullptr};        // physical phi planes, ping-pong (YBJModel too: phi is not steady): wphi[wcur] is the current state's
  int wcur = 0;
  bool w0 = false;                         // wphi[wcur] is phi of the state the next step starts from
  // ray mode (section 5t): each particle carries a wavevector (k, l) through (U + u, v) and zeta = q_psi
  bool rays = false;
  double eta = 0.0;                        // f / kappa^2 (hslash)
  double *k = nullptr, *l = nullptr;
  double* zeta[2] = {nullptr, nullptr};    // q_psi planes beside uv[0], uv[1] (YBJModel: one, as uv): zeta[cur] is the current state's
  bool z0 = false;                         // zeta[cur] is q_psi of the state the next step starts from
  double* zplane = nullptr;                // q_psi for PT_ZETA without ray mode, allocated when first needed
  // stretch mode (section 5u): each particle carries the deformation gradient F of its trajectory, four arrays of n doubles
  bool tan = false;
  double* f[4] = {nullptr, nullptr, nullptr, nullptr};      // f11, f12, f21, f22
  long long tan_step0 = 0, tan_count0 = 0; // steps since attach, and records written, when F was last set (attach or reset)
  // Lagrangian spectra and dispersion (section 5r): work plane, window, series table, index lists and tables, allocated by the
  // first call and grown when a later call needs more; the transform of the record axis runs on an engine of its own
  enum { LG_WORK = 0, LG_WIN, LG_SER, LG_ORDER, LG_OFFS, LG_TAB, LG_PAIRS, LG_NBUF };
  void* lg[LG_NBUF] = {};
  size_t lg_have[LG_NBUF] = {};            // bytes
  nq_any* eng = nullptr;
  ~NqParticles() { if (eng) (void)nq_any_destroy(eng); }
};
struct NqForcing : DevOwned {              // stochastic forcing (section 5i)
  double *Aq = nullptr, *Aphi = nullptr;   // amplitude planes: (N, N/2+1) and (N, N), contiguous
  FcBox bq = {}, bphi = {};                // bounding boxes of A > 0 (nrows = 0: nothing to add)
  dim3 gq, gphi;                           // launch grids over the boxes
  int npq = 0, npphi = 0;                  // workgroups = work partials of each kernel
  double *partq = nullptr, *partphi = nullptr, *work = nullptr;   // partials [workgroups][2]; work_q, work_phi
  unsigned long long seed = 0;
  long long s = 0;                         // index of the next forced step
};
struct NqFreq : DevOwned {                 // low-mode recorder (section 5j)
  static constexpr int NF = 3;             // FQ_NFIELDS (nq_freq.hpp comes after the shell rule: checked where it is included)
  int K = 0, nf = 0;
  int field[NF] = {0, 0, 0}, ncols[NF] = {0, 0, 0};
  cd* ring[NF] = {nullptr, nullptr, nullptr};     // [record][row][col] of each attached field
  RecordRing rg;
  cd* work = nullptr;                      // (rg.cap, modes of the widest field): allocated by the first spectrum
  double *win = nullptr, *tab = nullptr;   // window (rg.cap), table (rg.cap, nb)
  nq_any* eng = nullptr;                   // the any-length transform of the record axis runs on an engine of its own
  ~NqFreq() { if (eng) (void)nq_any_destroy(eng); }
};

struct NqAvg : DevOwned {                  // time-mean and covariance maps (section 5l)
  int nf = 0, np = 0;
  int field[AVG_SLOTS + 1] = {0, 0, 0, 0};          // public ids, in the order of the attach call: the planes nq_avg_read counts
  void* plane[AVG_SLOTS + 1 + AVG_MAX_PRODUCTS] = {};       // fields first (phi: a complex plane), then the products
  AvgArgs args = {};
  bool flow = false;                       // a flow field is listed: the samples run k_x_flow_moments with `sel` (section 5m)
  FlowSel sel = {};
  RecordRing rg;                           // cap = 1: only tick() and the two counters are used (count = samples in the sums)
};
#include "nq_tspec.hpp"                    // NqTspec and its kernel: time-mean spectra, transfer and flux (section 5n)
static_assert(TSPEC_TR_ROWS == NQ_TRANSFER_ROWS, "rows of nq_transfer_binned");

struct nq_ctx {
  nq_params p;
  int N = 0, S1 = 0, S2 = 0, nk = 0;
  int CLy = CL;          // columns per workgroup of the y-side kernels: CL, or CLS with single-pass columns (S1 = N, S2 = 1)
  int small_qg = 0;      // QGModel on a small grid: columns per workgroup of the array-parallel spectral kernel k_c_qg (0 = off)
  int WhG = 0;           // global half-spectrum width N/2+1
  int Wh = 0, Ph = 0;    // valid local half-spectrum columns and their pitch (== WhG, N/2+8 when P == 1)
  bool own_stream = true;
  bool kernel_family = true;
  // c(l, k), the filter and the contour patches depend on l through l^2 only: rows l and N - l of every ETDRK4 coefficient plane
  // are bit-identical (unless the filter is not mirror-symmetric in l: the 2/3 mask).  cmirror = 1: the planes hold rows 0..N/2
  // and the spectral kernels index them through crow() -- half the coefficient memory, and, with the B-sub-pass workgroups of
  // mirrored residues launched back to back (pair_order), the second read of a line is served on chip.  NIWQG_AMD_COEF_MIRROR=0
  // keeps all N rows (A/B measurements).
  int cmirror = 0, crows = 0;
  // k_s_phi forms the phi-hat results of stages 0 and 1 again where a later stage needs them (phi_stage_update) and w.y[(cur+1)%3]
  // is not allocated.  NIWQG_AMD_PHI_STAGE_STORE=1 stores them and reads them back (A/B measurements, the bit-identity test).
  int phi_stage_store = 0;
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipEvent_t marks[16] = {};               // nq_event_record / nq_event_elapsed
  std::string err;
  long long bytes = 0;
  std::vector<void*> allocs;
  // tables
  cd* tw = nullptr;
  int num_cu = 256;
  cd *twx_half = nullptr;   // stage table of the N/2-point plan (k_x_products_eo / k_x_wavepv_eo: 8192-point rows)
  cd *twx = nullptr, *twx1 = nullptr;   // per-stage twiddle tables of the two row-kernel plans (WgFft::tw_off layout)
  double *kk = nullptr, *ll = nullptr, *filt_h = nullptr, *filt_f = nullptr;
  cd* contour = nullptr;
  // equations
  EqState q, w;
  // dual-copy q equation (dealias=True, or exact full-plane qh on request): second copy + unfolded filters
  bool dual = false;
  EqState q2;
  // the anti-Hermitian passenger on row l = N/2 of the reference's full-plane qh (k_s_q): one row per array, coefficient
  // pointers at row N/2 of the q planes; off in dual mode (the second copy carries it) and for QGModel
  bool pass = false;
  EqState qp;
  cd* coefu[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // q coefficients without the filter
  struct CoefPatch { int n = 0; int* l = nullptr; int* k = nullptr; cd* v = nullptr; } patch[3];   // nq_coeff_patch, per public eq
  double* filt_m = nullptr;                                                 // filter at (-l, -k)
  // half-spectrum aux spectra
  cd *qwh = nullptr, *ph = nullptr;
  // inside a slab step the A sub-passes read / write the rank's own block on the X side directly and the exchanges skip its
  // device copy (ArrayListR; NIWQG_AMD_SLAB_OWN_REDIRECT=0 keeps the copy): set by nq_slab_step while it issues steps
  bool redir_now = false;
  // nq_tick_snapshot: qh (both copies), phih, qwh as the last diagnostics tick saw them (allocated by the first call)
  cd *tick_qh = nullptr, *tick_q2 = nullptr, *tick_w = nullptr, *tick_qwh = nullptr;
  // slab decomposition; P == 1: one rank owns everything
  int P = 1, rank = 0;
  int Nloc = 0;          // local rows on the X side
  int row0 = 0, nrows = 0;   // row window of the next row-kernel launch (a chunk of the local rows; whole slab by default)
  int Wf = 0, kf0 = 0;   // full-width planes: local columns, first global column
  int Wl = 0, kh0 = 0;   // half-spectrum planes: columns per rank, first global column of this rank
  // exchange groups: G[0] X->Y {Muq,Mvq,Mw}, G[1] Y->X {Mphi,Mphiy}, G[2] X->Y {Ma,Mb},
  // G[3] Y->X {Mu,Mp,Mq,Mqw}; Gs = stale copy of G[1]'s X side (UnCoupled's frozen phix/phiy, quirk Q1)
  // G[4] (YBJModel on more than one rank): Gs with a y side of its own, the second G1-shaped group of do_step_ybj
  struct Group {
    cd *bx = nullptr, *by = nullptr;
    int pitch = 0;
    size_t elems = 0;
  } G[5];
  cd *Gs = nullptr, *Gs_y = nullptr;
  MArr mUq, mVq, mW, mPhi, mPhiy, mGx, mGy, mA, mB, mU, mP, mQ, mQw;
  // scratch for the generic transforms / downloads
  cd *scr_f0 = nullptr, *scr_f1 = nullptr, *scr_h0 = nullptr, *scr_h1 = nullptr;
  double* scr_r = nullptr;
  // in-step budget integrals (ref Kernel.py:319-322, :390-392)
  bool bud = false;
  int nww = 0, nwq = 0;                           // workgroups of the two kernels that emit partial sums
  double *partW = nullptr, *partQ = nullptr;      // [4 stages][workgroups][NQ_PARTW | 3]; partW: + 2 (BudgetW.w00)
  double *part0W = nullptr, *part0Q = nullptr;    // partials of set_phi / set_q / nq_invert
  double *diag_part = nullptr, *diag_out = nullptr;   // diagnostics tick: workgroup partials, 32 reduced sums
  double *spec_out = nullptr, *spec_r = nullptr;     // isotropic spectra of the tick: 32 x nb shell sums, two real planes
  double* tr_out = nullptr;                          // spectral transfer: NQ_TRANSFER_ROWS x nb shell sums
  // PDFs of the physical fields (nq_field_hist): 64-bit tables of the largest configuration and the min/max partials,
  // allocated by the first call; the configuration of the last binning call (what nq_field_hist_read copies out)
  unsigned long long* hist_tab = nullptr;
  double* hist_part = nullptr;
  struct HistCfg { int nf = 0, fields[4] = {0, 0, 0, 0}, slot[4] = {0, 0, 0, 0}, bins = 0, jbins = 0, ja = -1, jb = -1; double lo[4] = {}, hi[4] = {}; } hist_cfg;
  // structure functions (nq_structure): the running table of raw sums and the workgroup partials, sized by the largest call so
  // far; the configuration of the call that zeroed the table (what accumulate = 1 must repeat and nq_structure_read copies out)
  double *sf_tab = nullptr, *sf_part = nullptr;
  int* sf_seps = nullptr;                         // the separations of the call on the device, from sf_seps_host
  int sf_seps_host[SF_MAX_SEPS] = {};
  void* sf_part_raw = nullptr;
  size_t sf_part_count = 0;
  struct SfCfg { int nf = 0, fields[SF_MAX_FIELDS] = {}, nsep = 0, seps[SF_MAX_SEPS] = {}, ntri = 0, tri[3 * SF_MAX_TRIPLES] = {}; long long samples = 0; } sf_cfg;
  // structure functions at two-dimensional separations (nq_structure2): a running table, vectors and projection of their own, the
  // physical planes the store pass writes (one pool: the real planes, then the complex one), and the call that zeroed the table
  double *sf2_tab = nullptr, *sf2_proj = nullptr;
  Sf2Vec* sf2_vecs = nullptr;
  Sf2Vec sf2_vecs_host[SF2_MAX_VECS] = {};
  double sf2_proj_host[2 * SF2_MAX_VECS] = {};
  void* sf2_planes = nullptr;
  size_t sf2_planes_count = 0;                    // doubles
  struct Sf2Cfg {
    int nf = 0, fields[SF_MAX_FIELDS] = {}, nvec = 0, vecs[2 * SF2_MAX_VECS] = {}, pa = -1, pb = -1, ntri = 0, tri[3 * SF_MAX_TRIPLES] = {};
    bool has_proj = false;
    double proj[2 * SF2_MAX_VECS] = {};
    long long samples = 0;
  } sf2_cfg;
  // PDFs of the increments (nq_increment_hist, nq_increment_hist2, nq_increment_range*; csrc/nq_ipdf.hpp): the 64-bit count table
  // (grown by the largest call), the ranges, the separations or vectors and the projection on the device with their staging copies,
  // the table of the range pass's sums, and the call that zeroed the count table (one table for both kinds of call)
  void* ipdf_tab = nullptr;
  size_t ipdf_tab_bytes = 0;
  double *ipdf_rng = nullptr, *ipdf_proj = nullptr, *ipdf_sums = nullptr;
  int* ipdf_seps = nullptr;
  Sf2Vec* ipdf_vecs = nullptr;
  int ipdf_seps_host[SF_MAX_SEPS] = {};
  Sf2Vec ipdf_vecs_host[SF2_MAX_VECS] = {};
  double ipdf_proj_host[2 * SF2_MAX_VECS] = {}, ipdf_rng_host[3 * SF_MAX_FIELDS * SF2_MAX_VECS] = {};
  struct IpdfCfg {
    int kind = 0, nf = 0, fields[SF_MAX_FIELDS] = {}, n = 0, vecs[2 * SF2_MAX_VECS] = {}, pa = -1, pb = -1, bins = 0;   // kind 1: separations (in vecs[0..n)), 2: vectors
    bool has_proj = false;
    double proj[2 * SF2_MAX_VECS] = {}, lo[SF_MAX_FIELDS * SF2_MAX_VECS] = {}, hi[SF_MAX_FIELDS * SF2_MAX_VECS] = {};
    long long samples = 0;
  } ipdf_cfg;
  // vortex census (nq_vortex_*; csrc/nq_vortex.hpp): the label and rank planes, the small buffers (range partials, scales, info,
  // per-row counts) and the table, grown by the largest capacity; the call nq_vortex_read and nq_vortex_labels answer for
  void *vx_planes = nullptr, *vx_small = nullptr, *vx_tab = nullptr;
  size_t vx_planes_bytes = 0, vx_small_bytes = 0, vx_tab_bytes = 0;
  struct VxCfg { int nf = 0, cap = 0; bool census = false; } vx_cfg;
  cd *tr_h = nullptr, *tr_f = nullptr;               // its planes on slab contexts (two half, one full-width; P == 1: scr_*)
  double *carryW = nullptr, *carryQ = nullptr;    // spectral sums of the state at the start of the next step
  double *gradS1 = nullptr, *acc = nullptr;       // stale-aware sum wv2|phih_grad|^2 ; Ke,Pw,Kw increments
  double* bsums = nullptr;                        // [4 stages][11] reduced sums of one step
  int prof_class = -1;
  int prof_stride = 1;          // nq_profile_stride: every prof_stride-th launch of the enabled class is bracketed
  unsigned long long prof_seen = 0;
  std::vector<hipEvent_t> prof_ev;               // pairs
  std::vector<int> prof_cls;                     // kernel class of each pair
  size_t prof_used = 0;
  bool have_q = false, have_phi = false, stepped = false;
  // max |u|, max |v| of the FOURTH stage (what the reference's status line uses after a step without a tick: Kernel.py:594 with
  // the self.u, self.v of :364-368): recorded by the last step of a call when asked for (nq_request_stage4_max)
  bool want_uv4 = false, uv4_now = false, have_uv4 = false;
  double* uv4 = nullptr;
  // snapshots (ref niwqg/Saving.py:59-86): physical q, phi in buffers of their own, copied out on a second stream
  double* snap_q = nullptr;
  cd* snap_phi = nullptr;
  double* snap_hq = nullptr;       // pinned host
  cd* snap_hphi = nullptr;
  hipStream_t snap_stream = nullptr;
  hipEvent_t ev_snap = nullptr;
  bool snap_busy = false;
  // single-rank CoupledModel: the q update (memory-bound) runs on a second stream beside the wave-PV row kernel
  // (transform-engine bound), whose persistent grid shrinks to `overlap_grid` workgroups and so leaves
  // `overlap_cus` = num_cu - overlap_grid CUs free for it (0 = off: the serial step); DESIGN.md section 8
  hipStream_t stream2 = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  int overlap_cus = 0, overlap_grid = 0;
  // ---- slab step inside the library: how the exchange groups cross between the ranks
  int link = 0;                        // LINK_*: 0 none, 1 peers in this process, 2 RCCL, 3 caller's callbacks, 4 nothing on the wire (nq_slab_set_null_link)
  std::vector<nq_ctx*> peers;          // LINK_PEERS: every rank's context (index = rank), the same list on all of them
  void* comm = nullptr;                // LINK_RCCL: ncclComm_t
  nq_exchange_fn xcb = nullptr;        // LINK_CALLBACK
  nq_allreduce_fn rcb = nullptr;
  void* cb_user = nullptr;
  int nchunk = 1;                      // row chunks per exchange (producer / consumer row kernels run chunk by chunk)
  int reserve_cus = 0;                 // CUs the persistent row kernels leave free (RCCL's copy kernels need somewhere to run:
                                       // a row-kernel workgroup owns the whole register file of its CU)
  hipStream_t mstream = nullptr;       // exchanges run here, beside the compute stream
  hipEvent_t ev_prod[8] = {}, ev_arr[5][8] = {}, ev_col = nullptr, ev_done = nullptr, ev_red = nullptr;
  bool arr_pending[5] = {false, false, false, false, false};   // group g is arriving chunk by chunk (ev_arr[g][*] recorded)
  long long n_exch = 0, n_calls = 0, n_steps = 0;       // counters since nq_slab_counters(reset)
  double bytes_sent = 0.0;
  std::vector<hipEvent_t> xev;         // timing pairs around every exchange chunk on mstream (when counting)
  size_t xev_used = 0;
  std::vector<hipEvent_t> rev;         // the same around every all-reduce
  size_t rev_used = 0;
  bool xtime = false;
  bool alloc_plain = false;            // dev_alloc: no skew (exchange-group buffers: whole rows, read by the row kernels)
  int spec_kind = -1;                  // what the scratch column slab of nq_slab_spectral holds: 1 half-spectrum, 0 full width
  bool ybj = false;
  bool passive = false;  // QGModel with its passive scalar: state cq, spectrum emitted through the qw slots of G3 / G0
  EqState cq;
  MArr mUc, mVc;      // niwqg.YBJModel: UnCoupled layouts, only phi is stepped (stage graph in do_step_ybj)
  NqParticles* pt = nullptr;          // Lagrangian particles (nq_particles_attach): null when none
  double pt_L[2] = {0.0, 0.0};       // their domain, Lx and Ly
  NqForcing* fc = nullptr;            // stochastic forcing (nq_forcing_attach): null when none
  NqFreq* fq = nullptr;               // low-mode time-series recorder (nq_freq_attach): null when none
  NqAvg* av = nullptr;                // time-mean and covariance maps (nq_avg_attach): null when none
  NqTspec* ts = nullptr;              // time-mean spectra, transfer and flux (nq_tspec_attach): null when none
  // coarse-grained flux maps (nq_coarse_flux): the filtered planes in spectral (s*) and mixed space (m*),
  // half-spectrum {G P, -il G P, G Q, il G Q, G Fu, G Fv} and full {G W, il G W, G J}, the tables, the workgroup partials, the
  // moments and the map planes; allocated by the first call (the map planes: the first that asks for maps), context-owned
  struct Coarse {
    cd *sh[6] = {}, *mh[6] = {}, *sf[3] = {}, *mf[3] = {};
    double *g = nullptr, *part = nullptr, *mom = nullptr, *map[3] = {};
    bool ready = false, have_maps = false;
  } cg;
  // shell-to-shell transfers (nq_shell_transfer): the filtered planes of one band in spectral (s*) and mixed
  // space (m*), half-spectrum G Q and full {G W, il G W}, the tables and the rows; allocated by the first call, context-owned
  struct S2s {
    cd *sq = nullptr, *mq = nullptr, *sf[2] = {}, *mf[2] = {};
    double *g = nullptr, *out = nullptr;
    bool ready = false;
  } ss;
  // co-spectra of the physical fields (nq_cospectra): this call's rows, the running sums, the list the sums
  // were started with and the calls in them; allocated by the first call, context-owned
  struct Cospec {
    double *cur = nullptr, *sum = nullptr;
    double *part = nullptr, *scl = nullptr;     // Kernel family: workgroup partials of the range pass, the scales of the call
    int nf = 0, fields[3] = {0, 0, 0};
    long long samples = 0;
  } cs;
};

// Device arrays start at staggered offsets inside their allocations.  hipMalloc hands out large blocks at addresses that
// differ by multiples of 2 MiB (the 256 MiB planes: by exact multiples of their size), so element idx of every state,
// tendency and coefficient plane a spectral kernel touches in one go would sit in the same DRAM channel and bank; a few
// KB of skew per array spreads them (tools/rw_mix_bench.hip: +12-24 % for kernels with 4-8 streams).
static size_t alloc_stagger_bytes() {
  static long v = -1;
  if (v < 0) {
    const char* e = getenv("NIWQG_AMD_ALLOC_STAGGER");
    v = e ? atol(e) : 4352;
    if (v < 0 || v % 256) v = 0;
  }
  return (size_t)v;
}
template <typename Tp>
static int dev_alloc(nq_ctx* c, Tp** out, size_t count) {
  void* p = nullptr;
  const size_t skew = c->alloc_plain ? 0 : (c->allocs.size() % 16) * alloc_stagger_bytes();
  HIPCHK(c, hipMalloc(&p, count * sizeof(Tp) + skew));
  HIPCHK(c, hipMemsetAsync(p, 0, count * sizeof(Tp) + skew, c->stream));
  c->allocs.push_back(p);
  c->bytes += (long long)(count * sizeof(Tp));
  *out = reinterpret_cast<Tp*>(static_cast<char*>(p) + skew);
  return 0;
}
#define ALLOC(c, ptr, count)                    \
  do {                                          \
    int rc_ = dev_alloc((c), &(ptr), (count));  \
    if (rc_) return rc_;                        \
  } while (0)

// ---- the lifecycle the step attachments share -----------------------------------------------
// `count` zero-filled elements owned by attachment `o` of context c, counted in both byte totals
template <typename Tp>
static int att_alloc(nq_ctx* c, DevOwned* o, Tp** out, size_t count, const char* what) {
  const size_t bytes = count * sizeof(Tp);
  void* p = nullptr;
  if (hipMalloc(&p, bytes) != hipSuccess) {
    (void)hipGetLastError();
    NQ_FAIL(c, -5, "%s: cannot allocate %zu bytes of device memory", what, bytes);
  }
  o->mem.push_back(p);
  o->bytes += (long long)bytes;
  c->bytes += (long long)bytes;
  HIPCHK(c, hipMemsetAsync(p, 0, bytes, c->stream));
  *out = static_cast<Tp*>(p);
  return 0;
}
// detach: the stream drains, the memory goes back, the slot (c->pt, c->fc, c->fq, c->av, c->ts) is null again
template <typename A>
static void att_release(nq_ctx* c, A*& slot) {
  if (!slot) return;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  c->bytes -= slot->rollback();
  delete slot;
  slot = nullptr;
}
// a failed attach: nothing stays attached, the first error's text is the one reported
template <typename A>
static int att_fail(nq_ctx* c, A*& slot, int rc) {
  const std::string e = c->err;
  att_release(c, slot);
  NQ_FAIL(c, rc, "%s", e.c_str());
}
// nq_step's two hooks, defined below the last attachment (the recorder, which needs the any-size engine): the one place
// that fixes the order the attachments see a step in.  niwqg_amd/_anysize.py's _step_etdrk4 mirrors it on the any-size path.
static void attachments_before_step(nq_ctx* c);
static int attachments_after_step(nq_ctx* c);
// particles: U0 is formed again from the state the next step starts from
// -- and, in drifter mode (section 5s), Phi0 from its phi.  Phi0 has a flag of its own: sampling "u" forms U0 alone, and
// nq_set_phi on CoupledModel changes phi's x-side array while quirk Q2 leaves U0's source as it was.  Every call that may change
// either between two steps clears both -- and the flag of ray mode's zeta plane (section 5t), for the same reason as Phi0's.
static void pt_mark_stale(nq_ctx* c) {
  if (c && c->pt) c->pt->u0 = c->pt->w0 = c->pt->z0 = false;
}

// ---------------------------------------------------------------------------------------------
// ETDRK4 coefficient planes on the device (ref Kernel.py:417-454, QGModel.py:426-443).
// eq 0: q (Kernel family), 1: phi, 2: q (QGModel, with beta), 3: QGModel's passive scalar.  One thread per element.
__device__ __forceinline__ cd cexp_d(cd z) {
  double s, c;
  sincos(z.y, &s, &c);
  const double e = exp(z.x);
  return cmake(e * c, e * s);
}
__device__ __forceinline__ cd cdiv(cd a, cd b) {
  const double d = b.x * b.x + b.y * b.y;
  return cmake((a.x * b.x + a.y * b.y) / d, (a.y * b.x - a.x * b.y) / d);
}

// the linear operator c(l, k) of equation eq (ref Kernel.py:417-418, :440-442, QGModel.py:426-428, :452-453)
__device__ __forceinline__ cd linear_operator(int eq, const nq_params& p, double kx, double ly) {
  const double wv2 = kx * kx + ly * ly, wv4 = wv2 * wv2;
  if (eq == 0) return cmake(-p.nu4 * wv4 - p.nu * wv2 - p.mu, -kx * p.U);
  if (eq == 1) return cmake(-p.nu4w * wv4 - p.nuw * wv2 - p.muw, -kx * p.U - 0.5 * p.f * (wv2 / p.kappa2));
  if (eq == 3) return cmake(-p.nu4c * wv4 - p.nuc * wv2 - p.muc, 0.0);      // QGModel's passive scalar: no mean flow, no beta
  const double wv2i = (wv2 != 0.0) ? 1.0 / wv2 : 0.0;
  return cmake(-p.nu4 * wv4 - p.nu * wv2 - p.mu, -kx * p.U + p.beta * kx * wv2i);
}

__global__ void k_etdrk4_coeffs(int eq, int N, int width, int pitch, int k0, nq_params p, const double* __restrict__ kk,
                                const double* __restrict__ ll, const double* __restrict__ filt,
                                const cd* __restrict__ contour, cd* E, cd* Eh, cd* Q, cd* f0, cd* fab, cd* fc) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  const int l = blockIdx.y;
  if (k >= width) return;
  const cd c = linear_operator(eq, p, kk[k0 + k], ll[l]);
  const cd ch = cscale(c, p.dt);
  cd sQ = cmake(0, 0), s0 = cmake(0, 0), sab = cmake(0, 0), sc = cmake(0, 0);
  for (int m = 0; m < 32; ++m) {
    const cd LR = cadd(ch, contour[m]);
    const cd LR2 = cmul(LR, LR), LR3 = cmul(LR2, LR);
    const cd eLR = cexp_d(LR), eh = cexp_d(cscale(LR, 0.5));
    sQ = cadd(sQ, cdiv(cmake(eh.x - 1.0, eh.y), LR));
    // (-4 - LR + e^LR (4 - 3 LR + LR^2)) / LR^3
    cd t = cmul(eLR, cmake(4.0 - 3.0 * LR.x + LR2.x, -3.0 * LR.y + LR2.y));
    s0 = cadd(s0, cdiv(cmake(-4.0 - LR.x + t.x, -LR.y + t.y), LR3));
    // (2 + LR + e^LR (-2 + LR)) / LR^3
    t = cmul(eLR, cmake(-2.0 + LR.x, LR.y));
    sab = cadd(sab, cdiv(cmake(2.0 + LR.x + t.x, LR.y + t.y), LR3));
    // (-4 - 3 LR - LR^2 + e^LR (4 - LR)) / LR^3
    t = cmul(eLR, cmake(4.0 - LR.x, -LR.y));
    sc = cadd(sc, cdiv(cmake(-4.0 - 3.0 * LR.x - LR2.x + t.x, -3.0 * LR.y - LR2.y + t.y), LR3));
  }
  const size_t idx = (size_t)l * pitch + k;
  const double fl = filt ? filt[idx] : 1.0;
  const double s = p.dt / 32.0 * fl;
  E[idx] = cscale(cexp_d(ch), fl);
  Eh[idx] = cscale(cexp_d(cscale(ch, 0.5)), fl);
  Q[idx] = cscale(sQ, s);
  f0[idx] = cscale(s0, s);
  fab[idx] = cscale(sab, s);
  fc[idx] = cscale(sc, s);
}

// Entries whose c dt lies within delta of MINUS a contour point: there one of the 32 terms of the contour mean is the
// removable singularity (e^z - 1 - z - ...) / z^3 at |z| < delta, evaluated by cancellation, and what the reference holds in Qh,
// f0, fab, fc at such an entry is its own libm's rounding error amplified by eps / |z|^3 -- a function of numpy's exp, not of
// the mathematics.  The host recomputes exactly these entries with the reference's numpy expression (niwqg_amd/_etdrk4.py) and
// hands them back through nq_coeff_patch; everywhere else the two evaluations agree to ~1e-13.
__global__ void k_coeff_flag(int eq, int N, int width, int k0, nq_params p, const double* __restrict__ kk,
                             const double* __restrict__ ll, const cd* __restrict__ contour, double delta2, int cap,
                             int* __restrict__ count, int* __restrict__ lo, int* __restrict__ ko) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x, l = blockIdx.y;
  if (k >= width) return;
  const cd ch = cscale(linear_operator(eq, p, kk[k0 + k], ll[l]), p.dt);
  double dmin = 1e300;
  for (int m = 0; m < 32; ++m) {
    const cd LR = cadd(ch, contour[m]);
    dmin = fmin(dmin, LR.x * LR.x + LR.y * LR.y);
  }
  if (!(dmin >= delta2)) {        // also catches NaN
    const int at = atomicAdd(count, 1);
    if (at < cap) { lo[at] = l; ko[at] = k0 + k; }
  }
}
// v: n x 4 values (Qh, f0, fab, fc of the reference, no filter); k is a global column
// mrows = N when the planes hold rows 0..N/2 only (row N - l shares the storage of row l: nq_ctx::cmirror), else 0
__global__ void k_coeff_patch(int n, const int* __restrict__ li, const int* __restrict__ ki, const cd* __restrict__ v, int width,
                              int pitch, int k0, const double* __restrict__ filt, cd* Q, cd* f0, cd* fab, cd* fc, int mrows) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int k = ki[i] - k0;
  if (k < 0 || k >= width) return;
  const double fl = filt ? filt[(size_t)li[i] * pitch + k] : 1.0;
  const int lr = (mrows && li[i] > mrows / 2) ? mrows - li[i] : li[i];
  const size_t idx = (size_t)lr * pitch + k;
  Q[idx] = cscale(v[4 * i], fl);
  f0[idx] = cscale(v[4 * i + 1], fl);
  fab[idx] = cscale(v[4 * i + 2], fl);
  fc[idx] = cscale(v[4 * i + 3], fl);
}

// small helper kernels -------------------------------------------------------------------------
// out = mult(l,k) * in on a spectral plane; mode 0: copy, 1: -i*l, 2: i*k, 3: -wv2i (psi from q, no wave part)
__global__ void k_spec_mul(const cd* __restrict__ in, cd* __restrict__ out, int width, int pitch, int mode,
                           const double* __restrict__ kk, const double* __restrict__ ll, int N, int kernel_family) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x, l = blockIdx.y;
  if (k >= width) return;
  const size_t idx = (size_t)l * pitch + k;
  const cd v = in[idx];
  const double kx = kk[k], ly = ll[l];
  cd o = v;
  if (mode == 1) {
    const double lz = (kernel_family && l == N / 2 && width != N) ? 0.0 : ly;
    o = cmake(lz * v.y, -lz * v.x);
  } else if (mode == 2) {
    o = cmake(-kx * v.y, kx * v.x);
  } else if (mode == 3) {
    const double wv2 = kx * kx + ly * ly;
    const double wv2i = (wv2 != 0.0) ? 1.0 / wv2 : 0.0;
    o = cmake(-wv2i * v.x, -wv2i * v.y);
  }
  out[idx] = o;
}

// out = a on the self-mirrored columns, (a + b)/2 on the interior columns (dual-copy q-hat -> Hermitian part); the planes are
// column slabs whose first column is global column k0 (0 on one rank)
__global__ void k_avg_interior(const cd* __restrict__ a, const cd* __restrict__ b, cd* __restrict__ out, int width,
                               int pitch, int N, int k0) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x, l = blockIdx.y;
  if (k >= width) return;
  const size_t idx = (size_t)l * pitch + k;
  cd v = a[idx];
  if (k0 + k > 0 && k0 + k < N / 2) {
    const cd w = b[idx];
    v = cmake(0.5 * (v.x + w.x), 0.5 * (v.y + w.y));
  }
  out[idx] = v;
}

// a *= -i, contiguous array
__global__ void k_mul_minus_i(cd* __restrict__ a, size_t n) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i < n) a[i] = cmul_mi(a[i]);
}

__global__ void k_axpy1(double* y, const double* x, double a) { y[0] += a * x[0]; }

// out = a - b on a half-spectrum plane (q_psi = q - qw, ref CoupledModel.py:145-152)
__global__ void k_sub_half(const cd* __restrict__ a, const cd* __restrict__ b, cd* __restrict__ out, int width, int pitch) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x, l = blockIdx.y;
  if (k >= width) return;
  const size_t idx = (size_t)l * pitch + k;
  out[idx] = csub(a[idx], b[idx]);
}

// Half spectra of REAL fields -> the reference's array layouts.  a(l,k) = f(l,k) for k <= N/2 and conj f(-l,-k) beyond
// (what numpy.fft.fft2 of the real field holds there); out has `wout` columns (N: Kernel family, N/2+1: QGModel).
//   mode 0: out = a1                               (ref CoupledModel.py:71: fft of a real field)
//   mode 1: out = i kk[k] a1 + i ll[l] a2          (ref Kernel.py:484 / QGModel.py:481: ik*fft(u q) + il*fft(v q))
__global__ void k_expand_half(const cd* __restrict__ f1, const cd* __restrict__ f2, cd* __restrict__ out, int N,
                              int pitch_h, int wout, int mode, const double* __restrict__ kk,
                              const double* __restrict__ ll) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x, l = blockIdx.y;
  if (k >= wout) return;
  cd a, b = cmake(0, 0);
  if (k <= N / 2) {
    const size_t at = (size_t)l * pitch_h + k;
    a = f1[at];
    if (mode == 1) b = f2[at];
  } else {
    const size_t at = (size_t)((N - l) % N) * pitch_h + (N - k);
    a = cconj(f1[at]);
    if (mode == 1) b = cconj(f2[at]);
  }
  if (mode == 1) {
    const double kx = kk[k], ly = ll[l];
    a = cmake(-(kx * a.y + ly * b.y), kx * a.x + ly * b.x);
  }
  out[(size_t)l * wout + k] = a;
}

// reductions: sum over a real/complex plane of a pointwise expression; result in out[0..] via atomics
// kind 0: sum |a|^2 (complex plane, width N)       -> out[0]
// kind 1: sum weight_k * wv2 * |a|^2 (half spectrum psi -> 2*ke_qg*M^2), skipping [0,0]
// kind 2: sum wv2 * |a|^2 (full complex plane)
// kind 3: max |a| over complex plane (out[0] as max via atomicMax on bits, values >= 0).  NaN propagates (nan_max): a NaN
//         with either sign bit orders above +inf as an unsigned bit pattern, so the atomicMax keeps it too
__global__ void k_reduce(const cd* __restrict__ a, int width, int pitch, int N, int kind, const double* __restrict__ kk,
                         const double* __restrict__ ll, double* out, double* __restrict__ part = nullptr) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x, l = blockIdx.y;
  double v = 0.0;
  if (k < width) {
    cd z = a[(size_t)l * pitch + k];
    if (kind == 4 && (k == 0 || k == N / 2)) {     // Kernel family: ph = fft of the REAL p, i.e. the Hermitian part (in l) of the
      const cd zm = a[(size_t)((N - l) % N) * pitch + k];   // two self-mirrored columns (they differ under the 2/3 mask's dual copies)
      z = cmake(0.5 * (z.x + zm.x), 0.5 * (z.y - zm.y));
    }
    const double m2 = z.x * z.x + z.y * z.y;
    if (kind == 0) v = m2;
    else if (kind == 1 || kind == 4) {
      const double w = (k == 0 || k == N / 2) ? 1.0 : 2.0;
      v = (l == 0 && k == 0) ? 0.0 : w * (kk[k] * kk[k] + ll[l] * ll[l]) * m2;
    } else if (kind == 2) v = (kk[k] * kk[k] + ll[l] * ll[l]) * m2;
    else v = sqrt(m2);
  }
  __shared__ double sh[256];
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int s = blockDim.x / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) sh[threadIdx.x] = (kind == 3) ? nan_max(sh[threadIdx.x], sh[threadIdx.x + s]) : sh[threadIdx.x] + sh[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (kind == 3) atomicMax(reinterpret_cast<unsigned long long*>(out), (unsigned long long)__double_as_longlong(sh[0]));
    else if (part) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = sh[0];      // one slot per workgroup, added up by k_sum_slots
    else atomicAdd(out, sh[0]);
  }
}
// out[0] = sum of part[0..n) in a fixed order (one workgroup).  The sums of k_reduce go through it: an atomicAdd per workgroup adds
// in the order the workgroups happen to finish, and the energies then differ in the last bit from one call to the next -- and
// between a run and the same run in other units (tests/test_gpu_magnitudes.py).
__global__ void k_sum_slots(const double* __restrict__ part, int n, double* out) {
  double v = 0.0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) v += part[i];
  __shared__ double sh[256];
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int s = blockDim.x / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = sh[0];
}
// max |a| of a real plane into out[0] (atomicMax on bits as kind 3 of k_reduce: NaN propagates)
__global__ void k_reduce_real_max(const double* __restrict__ a, size_t n, double* out) {
  double v = 0.0;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) v = nan_max(v, fabs(a[i]));
  __shared__ double sh[256];
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int s = blockDim.x / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) sh[threadIdx.x] = nan_max(sh[threadIdx.x], sh[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) atomicMax(reinterpret_cast<unsigned long long*>(out), (unsigned long long)__double_as_longlong(sh[0]));
}

// diagnostics tick: spectral sums -----------------------------------------------------------------
// Deterministic: every block writes its partial sums (part[block][NQ]); k_reduce_partials adds them.
template <int NQ>
__device__ void diag_block_store(double (&v)[NQ], double* __restrict__ part) {
  __shared__ double sh[4][NQ];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    double x = v[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
    if (lane == 0) sh[wave][i] = x;
  }
  __syncthreads();
  if (threadIdx.x < NQ) part[(size_t)blockIdx.x * NQ + threadIdx.x] = sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x];
}
// phih (local columns [k0, k0+width) of the full plane): S_n = sum wv2^n |phih|^2, n = 0..3   (256 threads)
__global__ void k_diag_phi(const cd* __restrict__ phih, int N, int width, int pitch, int k0,
                           const double* __restrict__ kk, const double* __restrict__ ll, double* __restrict__ part) {
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  const size_t total = (size_t)N * width;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int l = (int)(i / width), k = (int)(i - (size_t)l * width);
    const cd z = phih[(size_t)l * pitch + k];
    const double kx = kk[k0 + k], ly = ll[l];
    const double wv2 = kx * kx + ly * ly, m2 = z.x * z.x + z.y * z.y;
    v[0] += m2;
    v[1] += wv2 * m2;
    v[2] += wv2 * wv2 * m2;
    v[3] += wv2 * wv2 * wv2 * m2;
  }
  diag_block_store<4>(v, part);
}
// half spectra qh, qwh (may be null), ph; nine sums (see nq_diagnostics).  On the two self-mirrored columns the sums
// that stand for means of REAL fields use the Hermitian part H(l) = (X(l) + conj X(-l))/2 (what `.real` keeps).
// qp, qm (dual-copy contexts, else null): the two copies X+ = qh(l,k), X- = conj qh(-l,-k) that `qh` is the mean of.  The two
// spec_var-type sums (chi_q, ke_qg_q: ref Kernel.py:644, CoupledModel.py:115-136 take |.|^2 over the reference's FULL plane,
// which is not Hermitian under the 2/3 mask) then see |X+|^2 + |X-|^2 on the interior columns, not 2 |mean|^2.  filt_p, filt_m
// (idem): the filter at (l,k) and at (-l,-k).  The stored qwh is the Hermitian part fs * qw of the reference's filtr * qw, fs =
// (filt_p + filt_m)/2; ke_qg_w = spec_var over the full plane (CoupledModel.py:108) needs (filt_p^2 + filt_m^2)/2 |qw|^2 instead.
__global__ void k_diag_q(const cd* __restrict__ qh, const cd* __restrict__ qwh, const cd* __restrict__ ph, int N,
                         int width, int pitch, int k0, const double* __restrict__ kk, const double* __restrict__ ll,
                         double* __restrict__ part, const cd* __restrict__ qp, const cd* __restrict__ qm_,
                         const double* __restrict__ filt_p, const double* __restrict__ filt_m, const cd* __restrict__ passenger) {
  double v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  const size_t total = (size_t)N * width;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int l = (int)(i / width), kl = (int)(i - (size_t)l * width), k = k0 + kl;      // kl: local column, k: global
    const size_t idx = (size_t)l * pitch + kl;
    const cd q = qh[idx], w = qwh ? qwh[idx] : cmake(0, 0), p = ph[idx];
    cd hq = q, hw = w, hp = p;
    double wt = 2.0;
    if (k == 0 || k == N / 2) {
      wt = 1.0;
      const size_t im = (size_t)((N - l) % N) * pitch + kl;
      const cd qm = qh[im], wm = qwh ? qwh[im] : cmake(0, 0), pm = ph[im];
      hq = cmake(0.5 * (q.x + qm.x), 0.5 * (q.y - qm.y));
      hw = cmake(0.5 * (w.x + wm.x), 0.5 * (w.y - wm.y));
      hp = cmake(0.5 * (p.x + pm.x), 0.5 * (p.y - pm.y));
    }
    const double kx = kk[k], ly = ll[l];
    const double wv2 = kx * kx + ly * ly, wv4 = wv2 * wv2, wv2i = (wv2 != 0.0) ? 1.0 / wv2 : 0.0;
    double q2 = q.x * q.x + q.y * q.y;
    if (qp != nullptr && wt == 2.0) {
      const cd a = qp[idx], b = qm_[idx];
      q2 = 0.5 * (a.x * a.x + a.y * a.y + b.x * b.x + b.y * b.y);
    }
    if (passenger != nullptr && l == N / 2 && wt == 2.0) {       // the reference's full-plane qh carries an anti-Hermitian part A on
      const cd a = passenger[kl];                                  // this row: |qh(l,k)|^2 + |qh(l,-k)|^2 = 2 |H|^2 + 2 |A|^2 (spec_var sees it)
      q2 += a.x * a.x + a.y * a.y;
    }
    v[0] += wt * (hq.x * hq.x + hq.y * hq.y);                     // sum |H q|^2            -> ens
    v[1] += wt * wv4 * q2;                                        // sum wv4 |q|^2          -> chi_q
    v[2] += wt * wv2i * q2;                                       // sum |q|^2 / wv2        -> ke_qg_q
    double w2 = w.x * w.x + w.y * w.y;
    if (filt_p != nullptr) {
      const double fp = filt_p[idx], fm = filt_m[idx], fs = 0.5 * (fp + fm);
      if (fs > 0.0) {                      // as ratios: fs * fs underflows in the far corner of the exponential filter (exact_qh)
        const double a = fp / fs, b = fm / fs;
        w2 *= (wt == 2.0) ? 0.5 * (a * a + b * b) : a * a;
      }
    }
    v[3] += wt * wv2i * w2;                                       // sum |qw|^2 / wv2       -> ke_qg_w
    // -> ke_qg_qw = mean(uq uw + vq vw) of PHYSICAL fields (CoupledModel.py:110-112): u = Re ifft(-il psi) has nothing from the
    // Nyquist row, v = Re ifft(ik psi) nothing from the Nyquist column (Hermitian psi: the two partners cancel), and qwh has no
    // anti-Hermitian part for q-hat's to pair with.  Without a filter those two lines carry energy (2 of 460 random draws, 8e-6).
    const double w2eff = ((l == N / 2) ? 0.0 : ly * ly) + ((k == N / 2) ? 0.0 : kx * kx);
    v[4] += wt * wv2i * wv2i * w2eff * (hq.x * hw.x + hq.y * hw.y);
    // -> ke_qg.  Dual-copy (2/3 mask) contexts: the reference's ph = fft of the REAL p is the Hermitian part, and there the two
    // self-mirrored columns of the stored psi-hat are not Hermitian in l.  (QGModel's ph = -wv2i qh is summed as it is.)
    const cd pk = (qp != nullptr) ? hp : p;
    v[5] += (l == 0 && k == 0) ? 0.0 : wt * wv2 * (pk.x * pk.x + pk.y * pk.y);
    const double pq = hp.x * hq.x + hp.y * hq.y;                  // Re(conj(psi) q)
    v[6] += wt * wv4 * pq;                                        // -> mean(q lap2 psi)
    v[7] += wt * wv2 * pq;                                        // -> -mean(psi lap q)
    v[8] += wt * pq;                                              // -> mean(psi q)
  }
  diag_block_store<9>(v, part);
}

// passive scalar of QGModel: S_n = sum w wv2^n |c-hat|^2, n = 0..3, over the half spectrum (w = 1 on the self-mirrored columns,
// 2 elsewhere; n = 0 without the [0,0] entry, like spec_var): C2, gradC2, mean(lap c ^2), -mean(lap^2 c lap c)
__global__ void k_diag_c(const cd* __restrict__ ch, int N, int width, int pitch, int k0, const double* __restrict__ kk,
                         const double* __restrict__ ll, double* __restrict__ part) {
  // n = 0, 1 are spec_var sums of c-hat as it is (C2, gradC2); n = 2, 3 stand for physical-space means of lap c, which only
  // sees the Hermitian part (in l) of the two self-mirrored columns -- what irfft2 keeps
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  const size_t total = (size_t)N * width;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int l = (int)(i / width), kl = (int)(i - (size_t)l * width), k = k0 + kl;
    const cd z = ch[(size_t)l * pitch + kl];
    cd h = z;
    double wt = 2.0;
    if (k == 0 || k == N / 2) {
      wt = 1.0;
      const cd zm = ch[(size_t)((N - l) % N) * pitch + kl];
      h = cmake(0.5 * (z.x + zm.x), 0.5 * (z.y - zm.y));
    }
    const double kx = kk[k], ly = ll[l], wv2 = kx * kx + ly * ly;
    const double m2 = wt * (z.x * z.x + z.y * z.y), m2h = wt * (h.x * h.x + h.y * h.y);
    v[0] += (l == 0 && k == 0) ? 0.0 : m2;
    v[1] += wv2 * m2;
    v[2] += wv2 * wv2 * m2h;
    v[3] += wv2 * wv2 * wv2 * m2h;
  }
  diag_block_store<4>(v, part);
}

// isotropic spectra of the diagnostics tick (nq_diagnostics_binned) ------------------------------
// Shell of the wavenumber with integer indices (i, j): the unique b >= 0 with 2b - 1 <= 2 sqrt(i^2 + j^2) < 2b + 1, i.e.
// b = (isqrt(4 (i^2 + j^2)) + 1) / 2 -- integers only, no ties.  Only the sign-free i^2, j^2 enter, so the k = N/2 column
// of the half spectrum (+N/2) and of the full plane (-N/2) fall into the same shell.
__host__ __device__ inline long long nq_isqrt(long long v) {          // floor(sqrt(v)), v >= 0 (exact: v < 2^52 here)
  long long r = (long long)sqrt((double)v);
  while (r * r > v) --r;
  while ((r + 1) * (r + 1) <= v) ++r;
  return r;
}
__host__ __device__ inline int nq_shell_of(long long i, long long j) { return (int)((nq_isqrt(4 * (i * i + j * j)) + 1) / 2); }
// shells of an N x N grid: the corner i = j = N/2 lies in shell round(N / sqrt 2)
inline int nq_shell_count(int N) { return nq_shell_of(N / 2, N / 2) + 1; }
// the i >= 0 of row j that lie in shell b: [*lo, *hi] (empty when *lo > *hi)
__device__ inline void shell_run(int b, int j, int* lo, int* hi) {
  const long long j2 = 4LL * j * j, ub = (2LL * b + 1) * (2LL * b + 1) - j2;       // 4 i^2 < ub
  const long long lb = (b == 0) ? 0 : (2LL * b - 1) * (2LL * b - 1) - j2;           // 4 i^2 >= lb
  if (ub <= 0) { *lo = 1; *hi = 0; return; }
  *hi = (int)nq_isqrt((ub - 1) / 4);
  *lo = (lb <= 0) ? 0 : (int)nq_isqrt((lb + 3) / 4 - 1) + 1;                          // smallest i with i^2 >= ceil(lb / 4)
}
// Shell-stationary binning: workgroup b owns shell b and walks the rows |j| <= b, one row per thread; in a row the k of the
// shell are one run (half spectrum: k = i) or two (full plane: k = i and k = N - i), cut to the local columns [k0, k0 + width)
// (a slab rank's; the whole plane: 0, N/2 + 1 or N).  Every thread adds its rows in a fixed order, the workgroup reduces in a
// fixed tree: no atomics, bit-identical results from call to call.  Term::NQ sums per element, t(l, kg, kl, v) ADDS the
// terms of the element at row l, global column kg, local column kl = kg - k0 to v; out[q * nb + b] (q < Term::NQ).  256 threads.
template <class Term>
__global__ void __launch_bounds__(256) k_bin_shells(Term t, int N, int nb, int full, int k0, int width, double* __restrict__ out) {
  constexpr int NQ = Term::NQ;
  const int b = blockIdx.x;
  double v[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) v[q] = 0.0;
  const int j0 = (b < N / 2) ? -b : -N / 2, j1 = (b < N / 2 - 1) ? b : N / 2 - 1;
  for (int j = j0 + (int)threadIdx.x; j <= j1; j += blockDim.x) {
    int lo, hi;
    shell_run(b, j, &lo, &hi);
    const int l = (j < 0) ? j + N : j;
    int a = (lo > k0) ? lo : k0, e = (hi < N / 2) ? hi : N / 2;
    if (e > k0 + width - 1) e = k0 + width - 1;
    for (int i = a; i <= e; ++i) t(l, i, i - k0, v);                          // k = i (the half spectrum's only run)
    if (full) {                                                                // k = N - i: negative kx, i in [1, N/2 - 1]
      a = (lo > 1) ? lo : 1;
      if (a < N - k0 - width + 1) a = N - k0 - width + 1;
      e = (hi < N / 2 - 1) ? hi : N / 2 - 1;
      if (e > N - k0) e = N - k0;
      for (int i = a; i <= e; ++i) t(l, N - i, N - i - k0, v);
    }
  }
  __shared__ double sh[4][NQ];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    double x = v[q];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
    if (lane == 0) sh[wave][q] = x;
  }
  __syncthreads();
  if (threadIdx.x < NQ) out[(size_t)threadIdx.x * nb + b] = sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x];
}
// per-element terms of k_diag_phi: [0..3] wv2^n |phih|^2 (full plane)
struct BinPhi {
  static constexpr int NQ = 4;
  const cd* phih;
  int pitch;
  const double *kk, *ll;
  __device__ void operator()(int l, int k, int kl, double* v) const {
    const cd z = phih[(size_t)l * pitch + kl];
    const double kx = kk[k], ly = ll[l];
    const double wv2 = kx * kx + ly * ly, m2 = z.x * z.x + z.y * z.y;
    v[0] += m2;
    v[1] += wv2 * m2;
    v[2] += wv2 * wv2 * m2;
    v[3] += wv2 * wv2 * wv2 * m2;
  }
};
// per-element terms of k_diag_q: [6..14] (half spectrum; weights, Hermitian parts, dual copies, filter ratios and the passenger
// row exactly as there)
struct BinQ {
  static constexpr int NQ = 9;
  const cd *qh, *qwh, *ph;
  int N, pitch;
  const double *kk, *ll;
  const cd *qp, *qm_;
  const double *filt_p, *filt_m;
  const cd* passenger;
  __device__ void operator()(int l, int k, int kl, double* v) const {
    const size_t idx = (size_t)l * pitch + kl;
    const cd q = qh[idx], w = qwh ? qwh[idx] : cmake(0, 0), p = ph[idx];
    cd hq = q, hw = w, hp = p;
    double wt = 2.0;
    if (k == 0 || k == N / 2) {
      wt = 1.0;
      const size_t im = (size_t)((N - l) % N) * pitch + kl;
      const cd qm = qh[im], wm = qwh ? qwh[im] : cmake(0, 0), pm = ph[im];
      hq = cmake(0.5 * (q.x + qm.x), 0.5 * (q.y - qm.y));
      hw = cmake(0.5 * (w.x + wm.x), 0.5 * (w.y - wm.y));
      hp = cmake(0.5 * (p.x + pm.x), 0.5 * (p.y - pm.y));
    }
    const double kx = kk[k], ly = ll[l];
    const double wv2 = kx * kx + ly * ly, wv4 = wv2 * wv2, wv2i = (wv2 != 0.0) ? 1.0 / wv2 : 0.0;
    double q2 = q.x * q.x + q.y * q.y;
    if (qp != nullptr && wt == 2.0) {
      const cd a = qp[idx], b = qm_[idx];
      q2 = 0.5 * (a.x * a.x + a.y * a.y + b.x * b.x + b.y * b.y);
    }
    if (passenger != nullptr && l == N / 2 && wt == 2.0) {
      const cd a = passenger[kl];
      q2 += a.x * a.x + a.y * a.y;
    }
    v[0] += wt * (hq.x * hq.x + hq.y * hq.y);
    v[1] += wt * wv4 * q2;
    v[2] += wt * wv2i * q2;
    double w2 = w.x * w.x + w.y * w.y;
    if (filt_p != nullptr) {
      const double fp = filt_p[idx], fm = filt_m[idx], fs = 0.5 * (fp + fm);
      if (fs > 0.0) {
        const double a = fp / fs, b = fm / fs;
        w2 *= (wt == 2.0) ? 0.5 * (a * a + b * b) : a * a;
      }
    }
    v[3] += wt * wv2i * w2;
    const double w2eff = ((l == N / 2) ? 0.0 : ly * ly) + ((k == N / 2) ? 0.0 : kx * kx);
    v[4] += wt * wv2i * wv2i * w2eff * (hq.x * hw.x + hq.y * hw.y);
    const cd pk = (qp != nullptr) ? hp : p;
    v[5] += (l == 0 && k == 0) ? 0.0 : wt * wv2 * (pk.x * pk.x + pk.y * pk.y);
    const double pq = hp.x * hq.x + hp.y * hq.y;
    v[6] += wt * wv4 * pq;
    v[7] += wt * wv2 * pq;
    v[8] += wt * pq;
  }
};
// per-element terms of k_diag_c: [16..19] w wv2^n |c-hat|^2 (half spectrum)
struct BinC {
  static constexpr int NQ = 4;
  const cd* ch;
  int N, pitch;
  const double *kk, *ll;
  __device__ void operator()(int l, int k, int kl, double* v) const {
    const cd z = ch[(size_t)l * pitch + kl];
    cd h = z;
    double wt = 2.0;
    if (k == 0 || k == N / 2) {
      wt = 1.0;
      const cd zm = ch[(size_t)((N - l) % N) * pitch + kl];
      h = cmake(0.5 * (z.x + zm.x), 0.5 * (z.y - zm.y));
    }
    const double kx = kk[k], ly = ll[l], wv2 = kx * kx + ly * ly;
    const double m2 = wt * (z.x * z.x + z.y * z.y), m2h = wt * (h.x * h.x + h.y * h.y);
    v[0] += (l == 0 && k == 0) ? 0.0 : m2;
    v[1] += wv2 * m2;
    v[2] += wv2 * wv2 * m2h;
    v[3] += wv2 * wv2 * wv2 * m2h;
  }
};
// k_s_project_bin's two real planes of per-element terms, in the places of [24..27] / [28..31]: Re-lap -> +0, Im-diss -> +3
// (+1, +2, the Im-lap and Re-diss projections, are not binned and stay zero)
struct BinProj {
  static constexpr int NQ = 4;
  const double *rlap, *rdiss;
  int pitch;
  __device__ void operator()(int l, int k, int kl, double* v) const {
    (void)k;
    const size_t idx = (size_t)l * pitch + kl;
    v[0] += rlap[idx];
    v[3] += rdiss[idx];
  }
};

// spectral transfer (nq_transfer_binned) ---------------------------------------------------------
// Re(conj X * (i kx a + i ly b)) of one half-spectrum element, with a = F[u s], b = F[v s] of a real field s: the co-spectrum of
// X with the Jacobian J(psi, s) over the FULL plane, weight 2 on the interior columns standing for (l, k) and (-l, -k).  On the
// two self-mirrored columns every factor is replaced by its Hermitian part (what the real fields' transforms hold) and the
// weight is 1.  On the column k = N/2 and the row l = N/2 the full plane holds kx (ly) with ONE sign for an element and its
// mirror, so their kx (ly) terms cancel in pairs inside the shell: those wavenumbers enter as 0.
__device__ inline cd herm_part(cd x, cd xm) { return cmake(0.5 * (x.x + xm.x), 0.5 * (x.y - xm.y)); }
struct HalfJac {
  const cd *fu, *fv;
  int N, pitch;
  const double *kk, *ll;
  // *wt: the element's weight; *x: X at the element (Hermitian part on the self-mirrored columns); returns (Re J, Im J)
  __device__ cd at(const cd* X, int l, int k, int kl, double* wt, cd* x) const {
    const size_t idx = (size_t)l * pitch + kl;
    cd a = fu[idx], b = fv[idx];
    *x = X[idx];
    *wt = 2.0;
    if (k == 0 || k == N / 2) {
      *wt = 1.0;
      const size_t im = (size_t)((N - l) % N) * pitch + kl;
      a = herm_part(a, fu[im]);
      b = herm_part(b, fv[im]);
      *x = herm_part(*x, X[im]);
    }
    const double kx = (k == N / 2) ? 0.0 : kk[k], ly = (l == N / 2) ? 0.0 : ll[l];
    return cmake(-(kx * a.y + ly * b.y), kx * a.x + ly * b.x);
  }
};
// rows [0] Re(conj psi-hat Jq), [1] Re(conj q-hat Jq) with Jq = i k F[u q] + i l F[v q] (half spectrum; qh: the q-hat the tick
// bins, i.e. the mean of the two copies on dual-copy contexts; the passenger row never reaches physical space and is not in it)
struct BinTrQ {
  static constexpr int NQ = 2;
  HalfJac j;
  const cd *ph, *qh;
  __device__ void operator()(int l, int k, int kl, double* v) const {
    double wt;
    cd p, q;
    const cd J = j.at(ph, l, k, kl, &wt, &p);
    j.at(qh, l, k, kl, &wt, &q);
    v[0] += wt * (p.x * J.x + p.y * J.y);
    v[1] += wt * (q.x * J.x + q.y * J.y);
  }
};
// rows [4] Re(conj c-hat Jc), [5] wv2 Re(conj c-hat Jc) with Jc = i k F[u c] + i l F[v c] (QGModel's passive scalar)
struct BinTrC {
  static constexpr int NQ = 2;
  HalfJac j;
  const cd* ch;
  __device__ void operator()(int l, int k, int kl, double* v) const {
    double wt;
    cd c;
    const cd J = j.at(ch, l, k, kl, &wt, &c);
    const double kx = j.kk[k], ly = j.ll[l], t = wt * (c.x * J.x + c.y * J.y);
    v[0] += t;
    v[1] += (kx * kx + ly * ly) * t;
  }
};
// rows [2] / [3]: Re(conj phi-hat a) of a full plane a (the J plane F[u phix + v phiy], then the R plane i F[phi q_psi])
struct BinTrW {
  static constexpr int NQ = 1;
  const cd *phih, *a;
  int pitch;
  __device__ void operator()(int l, int k, int kl, double* v) const {
    (void)k;
    const size_t idx = (size_t)l * pitch + kl;
    const cd z = phih[idx], w = a[idx];
    v[0] += z.x * w.x + z.y * w.y;
  }
};

// budget bookkeeping ----------------------------------------------------------------------------
struct BudgetAcc {
  int model, nww, nwq, nqs;     // nqs: doubles per workgroup in partQ (6 with QGModel's passive scalar)
  double nu4c, muc;
  const double *partW, *partQ;
  double *carryW, *carryQ, *gradS1, *acc;
  double dt, f, hslash, kappa2, nu, nu4, mu, nuw, nu4w, muw, M;
};

__device__ double block_total(const double* __restrict__ part, int n, int stride, double* sh) {
  double x = 0.0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) x += part[(size_t)i * stride];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = x;
  __syncthreads();
  double tot = 0.0;
  for (int w = 0; w < (int)(blockDim.x >> 6); ++w) tot += sh[w];
  return tot;
}

// sums workgroup partials of one emitter into dst[0..nq)
__global__ void k_reduce_partials(const double* __restrict__ part, int nwg, int stride, int nq, double* dst) {
  __shared__ double sh[16];
  for (int q = 0; q < nq; ++q) {
    const double t = block_total(part + q, nwg, stride, sh);
    if (threadIdx.x == 0) dst[q] = t;
  }
}

// Stage sums: one workgroup per (stage, quantity); quantity 0-2: partQ, 3-8: partW (S0..S3, SG, SX), 9-10 unused.
// sums[stage][11]
__global__ void k_budget_sums(BudgetAcc b, double* __restrict__ sums) {
  __shared__ double sh[16];
  const int s = blockIdx.x / 11, q = blockIdx.x % 11;
  double t = 0.0;
  if (q < 3) t = block_total(b.partQ + (size_t)s * b.nwq * b.nqs + q, b.nwq, b.nqs, sh);
  else if (b.model == NQ_MODEL_QG) {
    if (b.nqs == 6 && q < 6) t = block_total(b.partQ + (size_t)s * b.nwq * 6 + q, b.nwq, 6, sh);   // |c|^2 sums
  } else {
    if (q < 3 + NQ_PARTW) t = block_total(b.partW + (size_t)s * b.nww * NQ_PARTW + (q - 3), b.nww, NQ_PARTW, sh);
  }
  if (threadIdx.x == 0) sums[s * 11 + q] = t;
}

// One ETDRK4 step's worth of budget rates -> Ke, Pw, Kw increments (ref Kernel.py:319-322, :390-392;
// QGModel.py:355-407).  Slot s of the spectral sums = state at the start of stage s.
__device__ void budget_accumulate_body(const BudgetAcc& b, const double* __restrict__ sums) {
  double sw[5][4], sj[4][2], sq[5][3];
  const bool qg = b.model == NQ_MODEL_QG;
  for (int s = 0; s < 4; ++s) {
    for (int q = 0; q < 3; ++q) sq[qg ? s : s + 1][q] = sums[s * 11 + q];
    for (int q = 0; q < 4; ++q) sw[s + 1][q] = sums[s * 11 + 3 + q];
    for (int q = 0; q < 2; ++q) sj[s][q] = sums[s * 11 + 7 + q];
  }
  const double M2 = b.M * b.M;
  if (!qg) {
    for (int q = 0; q < 3; ++q) sq[0][q] = b.carryQ[q];
    for (int q = 0; q < 4; ++q) sw[0][q] = b.carryW[q];
  }
  double K = 0.0, Pw = 0.0, A = 0.0;
  const double wgt[4] = {1.0, 2.0, 2.0, 1.0};
  for (int s = 0; s < 4; ++s) {
    const double ep_psi = (b.nu4 * sq[s][0] + b.nu * sq[s][1] + b.mu * sq[s][2]) / M2;
    double k = ep_psi, p = 0.0, a = 0.0;
    if (!qg) {
      const double lap2 = sw[s][2] / M2, glap2 = sw[s][3] / M2, phi2 = sw[s][0] / M2;
      const double grad2 = ((b.model == NQ_MODEL_COUPLED) ? sw[s][1] : b.gradS1[0]) / M2;
      // sj[s] = {sum Re(conj(lap_h) W), sum Im(conj(diss_h) W)} with W the whole phi tendency (k_s_phi)
      const double g12 = -0.5 * b.hslash * (sj[s][0] / M2) / b.f;      // gamma1 + gamma2
      const double x12 = -(sj[s][1] / M2) / b.f;                        // xi1 + xi2
      const double chi = (-0.5 * b.nu4w * glap2 - 0.5 * b.nuw * lap2 - 0.5 * b.muw * grad2) / b.kappa2;
      a = -b.nu4w * lap2 - b.nuw * grad2 - b.muw * phi2;
      k = -g12 + x12 + ep_psi;
      p = g12 + chi;
    }
    K += wgt[s] * k;
    Pw += wgt[s] * p;
    A += wgt[s] * a;
  }
  if (qg && b.nqs == 6) {
    // cvar += dt (c1 + 2 c2 + 2 c3 + c4) / 6 with c_s = ep_c after the stage-s update (ref QGModel.py:350-394, :595-598;
    // the reference multiplies gradC2 by nu, not nuc)
    for (int s = 0; s < 4; ++s) {
      const double* sc = sums + s * 11 + 3;
      Pw += wgt[s] * (-2.0 * b.nu4c * sc[2] - 2.0 * b.nu * sc[1] - 2.0 * b.muc * sc[0]) / M2;
    }
  }
  b.acc[0] += b.dt * K / 6.0;
  b.acc[1] += b.dt * Pw / 6.0;
  b.acc[2] += b.dt * A / 6.0;
  if (!qg) {
    for (int q = 0; q < 3; ++q) b.carryQ[q] = sq[4][q];
    for (int q = 0; q < 4; ++q) b.carryW[q] = sw[4][q];
  }
}
__global__ void k_budget_accumulate(BudgetAcc b, const double* __restrict__ sums) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  budget_accumulate_body(b, sums);
}
// Both in ONE launch of one workgroup, for grids whose kernels emit few partial sums (<= 256 workgroups; at 1024 partials one
// workgroup reading them all is slower than the 44 of k_budget_sums): on the small grids a step is a chain of dependent
// 5-15 us kernels and each of the two budget launches costs 4.6 us of it.
__global__ void __launch_bounds__(1024) k_budget_small(BudgetAcc b, double* __restrict__ sums) {
  __shared__ double ss[44];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  for (int i = wave; i < 44; i += nwaves) {          // every wave sums its own quantities: no workgroup barrier inside
    const int s = i / 11, q = i % 11;
    const double* part = nullptr;
    int n = 0, stride = 0;
    if (q < 3) {
      part = b.partQ + (size_t)s * b.nwq * b.nqs + q; n = b.nwq; stride = b.nqs;
    } else if (b.model == NQ_MODEL_QG) {
      if (b.nqs == 6 && q < 6) { part = b.partQ + (size_t)s * b.nwq * 6 + q; n = b.nwq; stride = 6; }
    } else if (q < 3 + NQ_PARTW) {
      part = b.partW + (size_t)s * b.nww * NQ_PARTW + (q - 3); n = b.nww; stride = NQ_PARTW;
    }
    double x = 0.0;
    for (int k = lane; k < n; k += 64) x += part[(size_t)k * stride];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
    if (lane == 0) {
      ss[i] = x;
      sums[i] = x;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) budget_accumulate_body(b, ss);
}

// ---------------------------------------------------------------------------------------------
// size dispatch
#define NQ_FOR_SIZES(M) M(64, 8, 8) M(128, 8, 16) M(256, 16, 16) M(512, 16, 32) M(1024, 32, 32) M(2048, 32, 64) M(4096, 64, 64) M(8192, 64, 128)

static bool plan_for(int N, int* S1, int* S2) {
#define CASE_(n, a, b) if (N == n) { *S1 = a; *S2 = b; return true; }
  NQ_FOR_SIZES(CASE_)
#undef CASE_
  return false;
}
// The three visitors below are the only places where a run-time size becomes a template argument: f is a generic lambda
// that reads the value from its argument's type (constexpr int N = decltype(n)::value).  A site that has kernels for
// some sizes only says so with `if constexpr` on N inside the lambda: the discarded branch instantiates nothing.
// false: the size is not in the table and f was not called.
template <int V>
struct Int { static constexpr int value = V; };
// row length: f(Int<n>) for the n of NQ_FOR_SIZES
template <class F>
static bool with_row_size(int N, F&& f) {
  switch (N) {
#define CASE_(n, a, b) case n: f(Int<n>{}); return true;
    NQ_FOR_SIZES(CASE_)
#undef CASE_
  }
  return false;
}
// y plan: f(Int<S1>, Int<CLy>); S1 = one radix of the two-pass transform (tiles of CL columns) or, with single-pass
// columns, N itself (tiles of CLS columns for N >= 128)
template <class F>
static bool with_col_plan(const nq_ctx* c, F&& f) {
#define CALL_(s, clx) case s: f(Int<s>{}, Int<clx>{}); return true;
  if (c->CLy == CL) {
    switch (c->S1) { CALL_(8, CL) CALL_(16, CL) CALL_(32, CL) CALL_(64, CL) }
  } else {
    switch (c->S1) { CALL_(128, CLS) CALL_(256, CLS) CALL_(512, CLS) }
  }
#undef CALL_
  return false;
}
// radix of the A sub-pass: f(Int<S2>)
template <class F>
static bool with_a_radix(int S2, F&& f) {
  switch (S2) {
#define CASE_(s) case s: f(Int<s>{}); return true;
    CASE_(8) CASE_(16) CASE_(32) CASE_(64) CASE_(128)
#undef CASE_
  }
  return false;
}
// grid of a row kernel that takes XPlan::C rows per workgroup, the last one possibly partly filled
template <class X>
static dim3 rows_grid(int rows) { return dim3((rows + X::C - 1) / X::C); }

// per-kernel event profiling ---------------------------------------------------------------------
enum { PK_PRODUCTS = 0, PK_WAVEPV = 1, PK_SQ = 2, PK_SPHI = 3, PK_INVERT = 4, PK_A = 5,
       PK_PT_ZETA = 6, PK_PT_RAYS = 7,     // ray mode's two kernels (section 5t): read one class at a time (nq_profile_read)
       PK_PT_TANGENT = 8 };                // stretch mode's step (section 5u), with or without the wave
struct ProfScope {
  nq_ctx* c;
  bool on;
  ProfScope(nq_ctx* c_, int cls) : c(c_), on(c_->prof_class == cls || c_->prof_class == -2) {   // -2: every class
    if (!on) return;
    if (c->prof_stride > 1 && (c->prof_seen++ % c->prof_stride) != 0) { on = false; return; }    // nq_profile_stride: a sample
    if (c->prof_used + 2 > c->prof_ev.size()) {
      for (int i = 0; i < 2; ++i) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) { on = false; return; }
        c->prof_ev.push_back(e);
      }
    }
    if (c->prof_cls.size() < c->prof_ev.size() / 2) c->prof_cls.resize(c->prof_ev.size() / 2);
    c->prof_cls[c->prof_used / 2] = cls;
    (void)hipEventRecord(c->prof_ev[c->prof_used], c->stream);
  }
  ~ProfScope() {
    if (!on) return;
    (void)hipEventRecord(c->prof_ev[c->prof_used + 1], c->stream);
    c->prof_used += 2;
  }
};

// generic launches -----------------------------------------------------------------------------
static void launch_x_c2c(nq_ctx* c, bool inv, const cd* in, cd* out, int pin, int pout, double scale, int mul_ik = 0) {
  with_row_size(c->N, [&](auto n) {
    constexpr int N = decltype(n)::value;
    typedef XPlan<N> X;
    const dim3 grid = rows_grid<X>(c->N), block(X::THREADS);
    if (inv) hipLaunchKernelGGL((k_x_c2c<N, true>), grid, block, X::LDS_BYTES, c->stream, in, out, pin, pout, c->N, scale, c->tw, c->kk, mul_ik);
    else hipLaunchKernelGGL((k_x_c2c<N, false>), grid, block, X::LDS_BYTES, c->stream, in, out, pin, pout, c->N, scale, c->tw, c->kk, mul_ik);
  });
}
static void launch_x_r2c(nq_ctx* c, const double* in, cd* out) {
  with_row_size(c->N, [&](auto n) {
    constexpr int N = decltype(n)::value;
    typedef XPlan<N> X;
    hipLaunchKernelGGL((k_x_r2c<N>), rows_grid<X>(c->N), dim3(X::THREADS), X::LDS_BYTES, c->stream, in, out, c->N, c->Ph, c->N, c->tw);
  });
}
static void launch_x_c2r(nq_ctx* c, const cd* in, double* out, double scale) {
  with_row_size(c->N, [&](auto n) {
    constexpr int N = decltype(n)::value;
    typedef XPlan<N> X;
    hipLaunchKernelGGL((k_x_c2r<N>), rows_grid<X>(c->N), dim3(X::THREADS), X::LDS_BYTES, c->stream, in, out, c->Ph, c->N, c->N, scale, c->tw);
  });
}

template <typename AL>
static void launch_A_list(nq_ctx* c, bool inv, const AL& al, int n, int maxw) {
  if (c->S2 == 1) return;                  // single-pass columns: the B sub-pass is the whole y transform
  ProfScope ps(c, PK_A);
  with_a_radix(c->S2, [&](auto s2) {
    constexpr int S = decltype(s2)::value;
    typedef YPlan<S> Y;
    const dim3 grid((maxw + CL - 1) / CL, c->S1, n), block(Y::THREADS);
    if (inv) hipLaunchKernelGGL((k_y_A<S, true, AL>), grid, block, Y::LDS_BYTES, c->stream, al, c->S1, c->tw, 1);
    else hipLaunchKernelGGL((k_y_A<S, false, AL>), grid, block, Y::LDS_BYTES, c->stream, al, c->S1, c->tw, 1);
  });
}
// A sub-pass on plain arrays (generic path, P == 1): half-spectrum or full-plane geometry
static void launch_A(nq_ctx* c, bool inv, std::initializer_list<cd*> arrs, bool half) {
  ArrayList al;
  int n = 0, maxw = 0;
  for (cd* a : arrs) {
    al.ptr[n] = a;
    al.width[n] = half ? c->Wh : c->N;
    al.pitch[n] = half ? c->Ph : c->N;
    maxw = al.width[n] > maxw ? al.width[n] : maxw;
    ++n;
  }
  for (int i = n; i < 6; ++i) { al.ptr[i] = nullptr; al.width[i] = 0; al.pitch[i] = 0; }
  launch_A_list(c, inv, al, n, maxw);
}
// local valid width of a mixed-space array on the Y side
static int y_width(const nq_ctx* c, const MArr& m) {
  if (m.W == c->Wf) return c->Wf;
  const int left = c->WhG - c->kh0;
  return left < 0 ? 0 : (left < c->Wl ? left : c->Wl);
}
// A sub-pass on the Y side of exchange-group arrays
static void launch_A_m(nq_ctx* c, bool inv, std::initializer_list<const MArr*> arrs) {
  ArrayListR al;
  int n = 0, maxw = 0;
  for (const MArr* m : arrs) {
    al.ptr[n] = m->ys;
    al.alt[n] = m->xs;
    al.width[n] = y_width(c, *m);
    al.pitch[n] = m->pitch;
    maxw = al.width[n] > maxw ? al.width[n] : maxw;
    ++n;
  }
  for (int i = n; i < 6; ++i) { al.ptr[i] = al.alt[i] = nullptr; al.width[i] = 0; al.pitch[i] = 0; }
  al.own0 = c->rank * c->Nloc;
  al.own1 = al.own0 + c->Nloc;
  if (maxw <= 0) return;
  if (c->redir_now) launch_A_list(c, inv, al, n, maxw);                               // (see ArrayListR)
  else launch_A_list(c, inv, static_cast<const ArrayList&>(al), n, maxw);
}
static void launch_B_p(nq_ctx* c, bool inv, const cd* in, int pin, cd* out, int pout, int width, double scale) {
  with_col_plan(c, [&](auto s1, auto cly) {
    constexpr int S = decltype(s1)::value, CLX = decltype(cly)::value;
    typedef YPlanT<S, CLX> Y;
    const dim3 grid((width + CLX - 1) / CLX, c->S2), block(Y::THREADS);
    if (inv) hipLaunchKernelGGL((k_y_B<S, true, CLX>), grid, block, Y::LDS_BYTES, c->stream, in, out, width, pin, pout, c->S2, scale, c->tw, 1);
    else hipLaunchKernelGGL((k_y_B<S, false, CLX>), grid, block, Y::LDS_BYTES, c->stream, in, out, width, pin, pout, c->S2, scale, c->tw, 1);
  });
}
static void launch_B(nq_ctx* c, bool inv, const cd* in, cd* out, bool half, double scale) {
  const int width = half ? c->Wh : c->N, pitch = half ? c->Ph : c->N;
  launch_B_p(c, inv, in, pitch, out, pitch, width, scale);
}

// whole 2-D transforms on device arrays (generic path, P == 1) -------------------------------------
// complex physical (N,N) -> spectral (N,N), unnormalised; `tmp` is a full-plane scratch
static void fwd2d_full(nq_ctx* c, const cd* phys, cd* spec, cd* tmp) {
  launch_x_c2c(c, false, phys, tmp, c->N, c->N, 1.0);
  launch_A(c, false, {tmp}, false);
  launch_B(c, false, tmp, spec, false, 1.0);
}
static void inv2d_full(nq_ctx* c, const cd* spec, cd* phys, cd* tmp) {
  launch_B(c, true, spec, tmp, false, 1.0 / ((double)c->N * c->N));
  launch_A(c, true, {tmp}, false);
  launch_x_c2c(c, true, tmp, phys, c->N, c->N, 1.0);
}
// real physical -> half spectrum
static void fwd2d_half(nq_ctx* c, const double* phys, cd* spec, cd* tmp_h) {
  launch_x_r2c(c, phys, tmp_h);
  launch_A(c, false, {tmp_h}, true);
  launch_B(c, false, tmp_h, spec, true, 1.0);
}
static void inv2d_half(nq_ctx* c, const cd* spec, double* phys, cd* tmp_h) {
  launch_B(c, true, spec, tmp_h, true, 1.0 / ((double)c->N * c->N));
  launch_A(c, true, {tmp_h}, true);
  launch_x_c2r(c, tmp_h, phys, 1.0);
}

// column-slab geometry of the spectral kernels
static YGeom geom_half(const nq_ctx* c) {
  YGeom g;
  g.k0 = c->kh0;
  const int left = c->WhG - c->kh0;
  g.width = left < 0 ? 0 : (left < c->Wl ? left : c->Wl);
  g.pitch_s = c->Ph;
  g.S2 = c->S2;
  g.kernel_family = c->kernel_family ? 1 : 0;
  g.cmirror = c->cmirror;
  return g;
}
static YGeom geom_full(const nq_ctx* c) {
  YGeom g;
  g.k0 = c->kf0;
  g.width = c->Wf;
  g.pitch_s = c->Wf;
  g.S2 = c->S2;
  g.kernel_family = 1;
  g.cmirror = c->cmirror;
  return g;
}

// fused-stage launches ----------------------------------------------------------------------------
// X-side view of a mixed-space array that starts at local row c->row0: a row kernel launched on such views with
// c->nrows rows processes one CHUNK of the slab (the slab driver overlaps the exchange of chunk i with the kernel of
// chunk i+1); everything a row kernel addresses is relative to the row, so the kernels themselves do not change
static MArr rw(const nq_ctx* c, const MArr& m) {
  MArr r = m;
  if (r.xs) r.xs += (size_t)c->row0 * m.pitch;
  return r;
}
// Grid and row blocks of a row kernel over `nrows` rows of an N-point grid: the one place that sizes them, for the launches
// below and for nq_row_grid_info.  A persistent grid never exceeds its row blocks (grid <= nb): every workgroup owns the block
// blockIdx.x, which the 4096-point kernels request before their loop without a guard.
enum { RG_PRODUCTS = 0, RG_WAVEPV = 1 };
struct RowGrid { int grid, nb; };
template <int N>
static RowGrid row_grid(const nq_ctx* c, int which, int nrows) {
  RowGrid g;
  if (which == RG_WAVEPV) {
    if constexpr (N == 8192) {
      const int ncu = (c->stream2 ? c->overlap_grid : c->num_cu) - c->reserve_cus, nb = nrows, grid = nb < ncu ? nb : ncu;
      g.grid = grid;
      g.nb = nb;
    } else if constexpr (N == 4096) {
      typedef XPlan<4096> X;
      int grid = (c->stream2 ? c->overlap_grid : c->num_cu) - c->reserve_cus;      // one persistent workgroup per CU
      const int nb = nrows / X::C;
      if (grid > nb) grid = nb;
      g.grid = grid;
      g.nb = nb;
    } else {                                          // not persistent: one workgroup per row block
      g.grid = g.nb = nrows / XPlan1<N>::C;
    }
    return g;
  }
  const int ncu = c->num_cu - c->reserve_cus;
  if constexpr (N == 8192) {
    const int nb = nrows, grid = nb < ncu ? nb : ncu;
    g.grid = grid;
    g.nb = nb;
  } else {
    typedef XPlan<N> X;
    const int nb = nrows / X::C;
    // one workgroup fits per CU (LDS) and does not spill: persistent; 8192-point rows spill and do better with dynamic dispatch
    const int grid = (X::LDS_BYTES > 80 * 1024 && X::THREADS <= 512 && nb > ncu) ? ncu : nb;
    g.grid = grid;
    g.nb = nb;
  }
  return g;
}
template <bool SLAB>
static void launch_wavepv_t(nq_ctx* c) {
  const MArr mPhi = rw(c, c->mPhi), mPhiy = rw(c, c->mPhiy), mA = rw(c, c->mA), mB = rw(c, c->mB);
  with_row_size(c->N, [&](auto n) {
    constexpr int N = decltype(n)::value;
    const RowGrid g = row_grid<N>(c, RG_WAVEPV, c->nrows);
    if constexpr (N == 8192) {                        // even / odd samples as two 4096-point problems (no spills)
      typedef XPlan<4096> X;
      const size_t ldsb = X::LDS_BYTES + (size_t)4096 * sizeof(cd);           // + the 64 KB of thread-private park slots
      hipLaunchKernelGGL((k_x_wavepv_eo<8192, SLAB>), dim3(g.grid), dim3(X::THREADS), ldsb, c->stream, mPhi, mPhiy, mA, mB, c->twx_half, c->tw, c->kk, g.nb);
    } else if constexpr (N == 4096) {                 // long rows: two transforms in flight, no spills
      typedef XPlan<4096> X;
      const size_t ldsb = X::LDS_BYTES + X::F::LDS_ELEMS * sizeof(cd);
      hipLaunchKernelGGL((k_x_wavepv2<4096, SLAB>), dim3(g.grid), dim3(X::THREADS), ldsb, c->stream, mPhi, mPhiy, mA, mB, c->twx, c->kk, g.nb);
    } else {
      typedef XPlan1<N> X;
      hipLaunchKernelGGL((k_x_wavepv<N, SLAB>), dim3(g.grid), dim3(X::THREADS), X::LDS_BYTES, c->stream, mPhi, mPhiy, mA, mB, c->twx1, c->kk);
    }
  });
}
// one rank: the row kernels address their rows without the block arithmetic of the slab layout (XRowT<false>)
static void launch_wavepv(nq_ctx* c) {
  ProfScope ps(c, PK_WAVEPV);
  if (c->P > 1) launch_wavepv_t<true>(c);
  else launch_wavepv_t<false>(c);
}
template <int MODE, bool SLAB>
static void launch_products_t(nq_ctx* c, double cj, double cr, bool fresh_grad) {
  const int vz = c->kernel_family ? 1 : 0;
  const MArr mU = rw(c, c->mU), mP = rw(c, c->mP), mQ = rw(c, c->mQ), mQw = rw(c, c->mQw), mPhi = rw(c, c->mPhi);
  const MArr mUq = rw(c, c->mUq), mVq = rw(c, c->mVq), mW = rw(c, c->mW), mPhiy = rw(c, c->mPhiy);
  const MArr mGx = rw(c, c->mGx), mGy = rw(c, c->mGy), mUc = rw(c, c->mUc), mVc = rw(c, c->mVc);
  const MArr& gx = (MODE == MODE_QGC) ? mUc : ((MODE == MODE_UNCOUPLED && !fresh_grad) ? mGx : mPhi);
  const MArr& gy = (MODE == MODE_QGC) ? mVc : ((MODE == MODE_UNCOUPLED && !fresh_grad) ? mGy : mPhiy);
  with_row_size(c->N, [&](auto n) {
    constexpr int N = decltype(n)::value;
    const RowGrid g = row_grid<N>(c, RG_PRODUCTS, c->nrows);
    if constexpr (N == 8192) {
      // rows too long for the register budget as one transform: even / odd samples as two 4096-point problems
      // (their stage table, c->twx_half, exists on every 8192 context)
      typedef XPlan<4096> X;
      const size_t ldsb = X::LDS_BYTES + (size_t)4096 * sizeof(cd);             // + the 64 KB of thread-private park slots
      hipLaunchKernelGGL((k_x_products_eo<8192, MODE, SLAB>), dim3(g.grid), dim3(X::THREADS), ldsb, c->stream, mU, mP, mQ, mQw, mPhi, gx, gy, mUq, mVq, mW, c->twx_half, c->tw, c->kk, vz, cj, cr, g.nb);
    } else {
      typedef XPlan<N> X;
      hipLaunchKernelGGL((k_x_products<N, MODE, SLAB>), dim3(g.grid), dim3(X::THREADS), X::LDS_BYTES, c->stream, mU, mP, mQ, mQw, mPhi, gx, gy, mUq, mVq, mW, c->twx, c->kk, vz, cj, cr, g.nb);
    }
  });
}
template <int MODE>
static void launch_products_m(nq_ctx* c, double cj, double cr, bool fresh_grad) {
  if (c->P > 1) launch_products_t<MODE, true>(c, cj, cr, fresh_grad);
  else launch_products_t<MODE, false>(c, cj, cr, fresh_grad);
}
// Mw <- cj * (u phix + v phiy) + i cr * phi q_psi; a step uses the phi tendency itself: cj = -1, cr = -1/2
// fresh_grad (UnCoupled layouts only): phix, phiy from the rows of Mphi, Mphiy instead of the frozen copy
static void launch_products(nq_ctx* c, double cj = -1.0, double cr = -0.5, bool fresh_grad = false) {
  ProfScope ps(c, PK_PRODUCTS);
  if (c->p.model == NQ_MODEL_COUPLED) launch_products_m<MODE_COUPLED>(c, cj, cr, false);
  else if (c->p.model == NQ_MODEL_UNCOUPLED) launch_products_m<MODE_UNCOUPLED>(c, cj, cr, fresh_grad);
  else if (c->passive) launch_products_m<MODE_QGC>(c, cj, cr, false);
  else launch_products_m<MODE_QG>(c, cj, cr, false);
}

static EtdArrays etd_arrays(EqState& e, int stage, int* out_slot) {
  // slots: cur = y(t_n); a = (cur+1)%3 holds the stage-0 result; b = (cur+2)%3 scratch
  const int cur = e.cur, a = (cur + 1) % 3, b = (cur + 2) % 3;
  EtdArrays ea;
  ea.y_in = (stage == 2) ? e.y[a] : e.y[cur];
  const int out = (stage == 0) ? a : (stage == 3 ? cur : b);
  ea.y_out = e.y[out];
  ea.fn0 = e.fn0;
  ea.fna = e.fna;
  ea.E = e.coef[0];
  ea.Eh = e.coef[1];
  ea.Q = e.coef[2];
  ea.f0 = e.coef[3];
  ea.fab = e.coef[4];
  ea.fc = e.coef[5];
  *out_slot = out;
  return ea;
}

// huq, hvq: the products' arrays, when they are not Muq, Mvq (the passive scalar's equation)
static void launch_sq(nq_ctx* c, const EtdArrays& ea, int stage, const MArr* huq_ = nullptr, const MArr* hvq_ = nullptr) {
  ProfScope ps(c, PK_SQ);
  const MArr& huq = huq_ ? *huq_ : c->mUq;
  const MArr& hvq = hvq_ ? *hvq_ : c->mVq;
  DualQ dq;
  EtdArrays eap = ea;
  memset(&dq, 0, sizeof(dq));
  if (c->dual) {
    int slot = 0;
    dq.minus = etd_arrays(c->q2, stage, &slot);
    dq.filt_p = c->filt_h;
    dq.filt_m = c->filt_m;
    eap.E = dq.minus.E = c->coefu[0];
    eap.Eh = dq.minus.Eh = c->coefu[1];
    eap.Q = dq.minus.Q = c->coefu[2];
    eap.f0 = dq.minus.f0 = c->coefu[3];
    eap.fab = dq.minus.fab = c->coefu[4];
    eap.fc = dq.minus.fc = c->coefu[5];
  }
  const YGeom g = geom_half(c);
  if (g.width <= 0) return;
  EtdArrays ep;
  memset(&ep, 0, sizeof(ep));
  if (c->pass && huq_ == nullptr) {        // the q equation itself, not the passive scalar's
    int slot = 0;
    ep = etd_arrays(c->qp, stage, &slot);
  }
  with_col_plan(c, [&](auto s1, auto cly) {
    constexpr int S = decltype(s1)::value, CLX = decltype(cly)::value;
    typedef YPlanT<S, CLX> Y;
    const dim3 grid((g.width + CLX - 1) / CLX, c->S2), block(Y::THREADS);
    if (c->dual) hipLaunchKernelGGL((k_s_q<S, true, CLX>), grid, block, Y::LDS_BYTES, c->stream, huq, hvq, eap, stage, g, c->kk, c->ll, c->tw, 1, dq, ep);
    else hipLaunchKernelGGL((k_s_q<S, false, CLX>), grid, block, Y::LDS_BYTES, c->stream, huq, hvq, eap, stage, g, c->kk, c->ll, c->tw, 1, dq, ep);
  });
}
static BudgetW budget_w(nq_ctx* c, double* part, const cd* y_start) {
  BudgetW bw;
  bw.part = c->bud ? part : nullptr;
  bw.y_start = y_start;
  bw.nu4w = c->p.nu4w;
  bw.nuw = c->p.nuw;
  bw.muw = c->p.muw;
  bw.part_prev = nullptr;
  bw.w00 = nullptr;
  return bw;
}
// ophi, ophiy: where phi and phiy of the stage result go, when not to Mphi, Mphiy (do_step_ybj)
// ea_: etd_arrays(c->w, stage) and y_start as the stored data flow has them; without phi_stage_store the kernel forms the
// results of stages 0 and 1 again from y(t_n) and the stored tendencies, and their planes are neither written nor read
static void launch_sphi(nq_ctx* c, const EtdArrays& ea_, int stage, const cd* y_start, const MArr* ophi_ = nullptr,
                        const MArr* ophiy_ = nullptr) {
  ProfScope ps(c, PK_SPHI);
  const MArr& ophi = ophi_ ? *ophi_ : c->mPhi;
  const MArr& ophiy = ophiy_ ? *ophiy_ : c->mPhiy;
  EtdArrays ea = ea_;
  PhiFlow pf;
  pf.y_n = c->w.y[c->w.cur];
  pf.store = c->phi_stage_store;
  if (!pf.store) {
    if (stage < 2) ea.y_out = nullptr;
    if (stage == 2) ea.y_in = nullptr;
    if (stage == 1 || stage == 2) y_start = nullptr;
  }
  BudgetW bw = budget_w(c, c->partW + (size_t)stage * c->nww * NQ_PARTW, y_start);
  if (bw.part && !pf.store) {
    // SG, SX of stage 1 come from the stage-2 launch.  Every reader of partW (k_budget_sums, k_budget_small, and through
    // bsums the slab all-reduce and the host's increments) runs after stage 3 of the step that wrote it, in every step.
    if (stage == 2) bw.part_prev = c->partW + (size_t)(stage - 1) * c->nww * NQ_PARTW;
    bw.w00 = c->partW + (size_t)4 * c->nww * NQ_PARTW;
  }
  const cd* jpass = c->ybj ? nullptr : c->mUq.ys + c->mUq.W;     // YBJModel.jacobian_psi_phi keeps [0,0] (YBJModel.py:123-133)
  const cd* jown = (jpass && c->redir_now) ? c->mUq.xs + c->mUq.W : jpass;     // the own block was not copied across (ArrayListR)
  const int own0 = c->redir_now ? c->rank * c->Nloc : 0, own1 = c->redir_now ? own0 + c->Nloc : 0;
  with_col_plan(c, [&](auto s1, auto cly) {
    constexpr int S = decltype(s1)::value, CLX = decltype(cly)::value;
    typedef YPlanT<S, CLX> Y;
    auto launch = [&](auto st) {
      hipLaunchKernelGGL((k_s_phi<S, CLX, decltype(st)::value>), dim3(c->Wf / CLX, c->S2), dim3(Y::THREADS), Y::LDS_BYTES, c->stream, c->mW, jpass, jown, own0, own1, c->mUq.pitch, ea, geom_full(c), ophi, ophiy, 1.0 / ((double)c->N * c->N), c->kk, c->ll, c->tw, 1, bw, pf);
    };
    switch (stage) {
      case 0: launch(Int<0>{}); break;
      case 1: launch(Int<1>{}); break;
      case 2: launch(Int<2>{}); break;
      default: launch(Int<3>{}); break;
    }
  });
}
static void launch_emit_phi(nq_ctx* c, const cd* phih) {
  BudgetW bw = budget_w(c, c->part0W, phih);
  with_col_plan(c, [&](auto s1, auto cly) {
    constexpr int S = decltype(s1)::value, CLX = decltype(cly)::value;
    typedef YPlanT<S, CLX> Y;
    hipLaunchKernelGGL((k_s_emit_phi<S, CLX>), dim3(c->Wf / CLX, c->S2), dim3(Y::THREADS), Y::LDS_BYTES, c->stream, phih, geom_full(c), c->mPhi, c->mPhiy, 1.0 / ((double)c->N * c->N), c->kk, c->ll, c->tw, 1, bw);
  });
}
// c_hat: the passive scalar's spectrum (contexts that have one; nullptr otherwise)
static void launch_invert(nq_ctx* c, const cd* qh, bool store_aux, double* part, const cd* q_bud, const cd* c_hat = nullptr) {
  ProfScope ps(c, PK_INVERT);
  // the second copy lives in the same rotating slot as qh
  const cd* qh_minus = nullptr;
  if (c->dual)
    for (int i = 0; i < 3; ++i)
      if (c->q.y[i] == qh) qh_minus = c->q2.y[i];
  const YGeom g = geom_half(c);
  if (g.width <= 0) return;
  with_col_plan(c, [&](auto s1, auto cly) {
    constexpr int S = decltype(s1)::value, CLX = decltype(cly)::value;
    typedef YPlanT<S, CLX> Y;
    auto launch = [&](auto mode) {
      hipLaunchKernelGGL((k_s_invert<S, decltype(mode)::value, CLX>), dim3((g.width + CLX - 1) / CLX, c->S2), dim3(Y::THREADS), Y::LDS_BYTES, c->stream, c->mA, c->mB, qh, c->filt_h, c->mU, c->mP, c->mQ, c->mQw, store_aux ? c->qwh : nullptr, store_aux ? c->ph : nullptr, g, 1.0 / ((double)c->N * c->N), c->p.f, c->kk, c->ll, c->tw, 1, c->bud ? part : nullptr, q_bud, qh_minus, c->dual ? c->filt_m : nullptr, c_hat);
    };
    if (c->passive) launch(Int<MODE_QGC>{});
    else if (c->p.model == NQ_MODEL_COUPLED) launch(Int<MODE_COUPLED>{});
    else launch(Int<MODE_UNCOUPLED>{});
  });
}

// QGModel, small grid: N_q, the stage update, the inversion and its three inverse y transforms in one launch
static void launch_cqg(nq_ctx* c, const EtdArrays& ea, int stage, bool store_aux, double* part, const cd* q_bud) {
  ProfScope ps(c, PK_SQ);
  with_row_size(c->N, [&](auto n) {
    constexpr int N = decltype(n)::value;
    if constexpr (N == 128 || N == 256 || N == 512) {
      constexpr int CW = N == 128 ? 4 : 2;           // columns per workgroup
      typedef SmallColPlan<N, CW> Y;
      hipLaunchKernelGGL((k_c_qg<N, CW>), dim3((c->Wh + CW - 1) / CW), dim3(Y::THREADS), Y::LDS_BYTES, c->stream, c->mUq, c->mVq, ea, stage,
                         geom_half(c), c->mU, c->mP, c->mQ, store_aux ? c->ph : nullptr, 1.0 / ((double)c->N * c->N), c->kk, c->ll, c->tw,
                         c->bud ? part : nullptr, q_bud);
    }
  });
}

static BudgetAcc budget_acc(nq_ctx* c) {
  BudgetAcc b;
  b.model = c->p.model;
  b.nww = c->nww; b.nwq = c->nwq; b.nqs = c->passive ? 6 : 3;
  b.nu4c = c->p.nu4c; b.muc = c->p.muc;
  b.partW = c->partW; b.partQ = c->partQ;
  b.carryW = c->carryW; b.carryQ = c->carryQ; b.gradS1 = c->gradS1; b.acc = c->acc;
  b.dt = c->p.dt; b.f = c->p.f; b.kappa2 = c->p.kappa2; b.hslash = c->p.f / c->p.kappa2;
  b.nu = c->p.nu; b.nu4 = c->p.nu4; b.mu = c->p.mu; b.nuw = c->p.nuw; b.nu4w = c->p.nu4w; b.muw = c->p.muw;
  b.M = (double)c->N * c->N;
  return b;
}

// a new qh from physical space (set_q) is Hermitian: the passenger row starts from zero
static int reset_passenger(nq_ctx* c) {
  if (c->pass) HIPCHK(c, hipMemsetAsync(c->qp.y[c->qp.cur], 0, sizeof(cd) * (size_t)c->Ph, c->stream));
  return 0;
}

// ---- phases of one ETDRK4 stage --------------------------------------------------------------------
// Between two phases the named exchange group has to cross from one side to the other: with P == 1 both
// sides are the same buffer and nq_step simply runs the phases back to back; with P > 1 the caller does
//      nq_phase(PRODUCTS) -> all_to_all(G0) -> nq_phase(UPDATE) -> all_to_all(G1) [-> all_to_all(G3)]
//      -> nq_phase(WAVEPV) -> all_to_all(G2) -> nq_phase(INVERT) -> all_to_all(G3)         (Coupled)
// (UnCoupled / QG have no WAVEPV/INVERT: UPDATE also emits G3.)
static const cd* stage_qh_out(nq_ctx* c, int stage) {
  const int cur = c->q.cur;
  return c->q.y[(stage == 0) ? (cur + 1) % 3 : (stage == 3 ? cur : (cur + 2) % 3)];
}
// join: recorded by another stream once qh is complete (do_step_overlap); the forward columns of a, b do not read qh
static void phase_invert_y(nq_ctx* c, const cd* qh, bool store_aux, double* part, const cd* q_bud, const cd* c_hat = nullptr,
                           hipEvent_t join = nullptr) {
  if (c->p.model == NQ_MODEL_COUPLED) launch_A_m(c, false, {&c->mA, &c->mB});
  if (join) (void)hipStreamWaitEvent(c->stream, join, 0);
  launch_invert(c, qh, store_aux, part, q_bud, c_hat);
  if (c->p.model == NQ_MODEL_COUPLED || c->passive) launch_A_m(c, true, {&c->mU, &c->mP, &c->mQ, &c->mQw});
  else launch_A_m(c, true, {&c->mU, &c->mP, &c->mQ});
}
static void phase_products(nq_ctx* c, int stage) { (void)stage; launch_products(c); }
static void phase_update(nq_ctx* c, int s) {
  const bool waves = c->p.model != NQ_MODEL_QG;
  int qslot = 0, wslot = 0;
  if (waves) launch_A_m(c, false, {&c->mW});
  if (c->passive) launch_A_m(c, false, {&c->mUq, &c->mVq, &c->mUc, &c->mVc});
  else launch_A_m(c, false, {&c->mUq, &c->mVq});
  EtdArrays eq = etd_arrays(c->q, s, &qslot);
  if (c->small_qg) {          // QGModel.py:355,:401: ep_psi of stages 0..2 with the start-of-step q
    launch_cqg(c, eq, s, s == 3, c->partQ + (size_t)s * c->nwq * 3, s < 3 ? c->q.y[c->q.cur] : nullptr);
    return;
  }
  launch_sq(c, eq, s);
  int cslot = 0;
  if (c->passive) {           // same update with the scalar's operator and its own products (ref QGModel.py:345-392)
    EtdArrays ec = etd_arrays(c->cq, s, &cslot);
    launch_sq(c, ec, s, &c->mUc, &c->mVc);
  }
  if (waves) {
    // phih at the start of this stage: y(t_n), stage-0 result, stage-1 result, stage-2 result
    const int cur = c->w.cur;
    const cd* y_start = (s == 0) ? c->w.y[cur] : (s == 1 ? c->w.y[(cur + 1) % 3] : c->w.y[(cur + 2) % 3]);
    EtdArrays ew = etd_arrays(c->w, s, &wslot);
    launch_sphi(c, ew, s, y_start);
    launch_A_m(c, true, {&c->mPhi, &c->mPhiy});
  }
  if (c->p.model != NQ_MODEL_COUPLED) {
    // no wave feedback on psi: the inversion needs no row pass, it runs here on the spectral side
    // QGModel evaluates ep_psi after each stage's inversion with the start-of-step q (QGModel.py:355,:401)
    const cd* q_bud = (!c->kernel_family && s < 3) ? c->q.y[c->q.cur] : nullptr;
    const int nqs = c->passive ? 6 : 3;
    phase_invert_y(c, c->q.y[qslot], s == 3, c->partQ + (size_t)s * c->nwq * nqs, q_bud, c->passive ? c->cq.y[cslot] : nullptr);
  }
}
static void phase_wavepv(nq_ctx* c) { launch_wavepv(c); }
static void phase_invert(nq_ctx* c, int s, hipEvent_t join = nullptr) {      // Coupled only
  phase_invert_y(c, stage_qh_out(c, s), s == 3, c->partQ + (size_t)s * c->nwq * 3, nullptr, nullptr, join);
}
static void phase_budget_sums(nq_ctx* c) {
  if (c->bud) hipLaunchKernelGGL(k_budget_sums, dim3(44), dim3(1024), 0, c->stream, budget_acc(c), c->bsums);
}
static void phase_budget_finish(nq_ctx* c) {
  if (c->bud) hipLaunchKernelGGL(k_budget_accumulate, dim3(1), dim3(64), 0, c->stream, budget_acc(c), (const double*)c->bsums);
}

// inversion of the CURRENT state outside a step (set_q, nq_invert); P == 1 only.  Its spectral sums become
// the next step's slot 0.
static void do_invert_now(nq_ctx* c) {
  if (c->p.model == NQ_MODEL_COUPLED) launch_wavepv(c);
  phase_invert_y(c, c->q.y[c->q.cur], true, c->part0Q, nullptr, c->passive ? c->cq.y[c->cq.cur] : nullptr);
  if (c->bud && c->kernel_family)
    hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(1024), 0, c->stream, c->part0Q, c->nwq, 3, 3, c->carryQ);
}

// physical rows <-> the x side of a mixed-space array, one row kernel each.  SLAB: this rank's c->Nloc rows in the slab
// layout; otherwise the c->N rows of a one-rank context.  false: no row plan, nothing launched.
template <bool SLAB>
static bool launch_get_real(nq_ctx* c, const MArr& src, double* out, int mode, int zero_nyq) {
  const int rows = SLAB ? c->Nloc : c->N;
  return with_row_size(c->N, [&](auto n) {
    constexpr int N = decltype(n)::value;
    typedef XPlan<N> X;
    hipLaunchKernelGGL((k_x_get_real<N, SLAB>), rows_grid<X>(rows), dim3(X::THREADS), X::LDS_BYTES, c->stream, src, out, rows, c->tw, c->kk, mode, zero_nyq);
  });
}
static bool launch_get_cplx(nq_ctx* c, const MArr& src, cd* out, int mul_ik) {
  return with_row_size(c->N, [&](auto n) {
    constexpr int N = decltype(n)::value;
    typedef XPlan<N> X;
    hipLaunchKernelGGL((k_x_get_cplx<N, true>), rows_grid<X>(c->Nloc), dim3(X::THREADS), X::LDS_BYTES, c->stream, src, out, c->Nloc, c->tw, c->kk, mul_ik);
  });
}
static bool launch_put_real(nq_ctx* c, const double* in, const MArr& dst) {
  return with_row_size(c->N, [&](auto n) {
    constexpr int N = decltype(n)::value;
    typedef XPlan<N> X;
    hipLaunchKernelGGL((k_x_put_real<N, true>), rows_grid<X>(c->Nloc), dim3(X::THREADS), X::LDS_BYTES, c->stream, in, dst, c->Nloc, c->tw);
  });
}
static bool launch_put_cplx(nq_ctx* c, const cd* in, const MArr& dst) {
  return with_row_size(c->N, [&](auto n) {
    constexpr int N = decltype(n)::value;
    typedef XPlan<N> X;
    hipLaunchKernelGGL((k_x_put_cplx<N, true>), rows_grid<X>(c->Nloc), dim3(X::THREADS), X::LDS_BYTES, c->stream, in, dst, c->Nloc, c->tw);
  });
}
// max |u|, max |v| over this rank's rows of Mu, Mp (x side) into out2[0], out2[1], which the caller has zeroed; scr: Nloc * N doubles
static bool launch_uv_max(nq_ctx* c, double* scr, double* out2) {
  const size_t n = (size_t)c->Nloc * c->N;
  for (int which = 0; which < 2; ++which) {
    if (!launch_get_real<true>(c, which == 0 ? c->mU : c->mP, scr, which, (which == 1 && c->kernel_family) ? 1 : 0)) return false;
    hipLaunchKernelGGL(k_reduce_real_max, dim3(1024), dim3(256), 0, c->stream, (const double*)scr, n, out2 + which);
  }
  return true;
}

// max |u|, max |v| over this rank's rows of the fields the LAST inversion emitted (Mu, Mp on the x side): during a step, right
// after stage index 2, these are the u, v of the reference's fourth jacobian_psi_q call (Kernel.py:364-368, :481-482)
static int stage4_uv_max(nq_ctx* c) {
  if (!c->uv4) ALLOC(c, c->uv4, (size_t)2);
  if (!c->scr_f0) ALLOC(c, c->scr_f0, (size_t)c->Nloc * c->N);
  HIPCHK(c, hipMemsetAsync(c->uv4, 0, sizeof(double) * 2, c->stream));
  if (!launch_uv_max(c, reinterpret_cast<double*>(c->scr_f0), c->uv4)) NQ_FAIL(c, -2, "no row plan of length %d", c->N);
  c->have_uv4 = true;
  return 0;
}

// niwqg.YBJModel._step_etdrk4 (YBJModel.py:52-87): psi, u, v, q are steady; phix, phiy are refreshed from the current
// phih before every stage, but the refraction factor phi only after the step.  Two G1-shaped buffers do it without a
// copy: A = G[1] holds phi, phiy of the start-of-step state (products read phi from it in all four stages, and the
// gradients in stage 0); B = Gs receives the stage results 0..2 and feeds the gradients of stages 1..3; the final
// state goes back to A, so B is left with the gradients of the stage-2 result -- exactly the stale phix, phiy the
// reference leaves behind (they matter to the next diagnostics tick only).
static void do_step_ybj(nq_ctx* c) {
  for (int s = 0; s < 4; ++s) {
    launch_products(c, -1.0, -0.5, s == 0);
    launch_A_m(c, false, {&c->mW});
    int wslot = 0;
    const int cur = c->w.cur;
    const cd* y_start = (s == 0) ? c->w.y[cur] : (s == 1 ? c->w.y[(cur + 1) % 3] : c->w.y[(cur + 2) % 3]);
    EtdArrays ew = etd_arrays(c->w, s, &wslot);
    if (s < 3) {
      launch_sphi(c, ew, s, y_start, &c->mGx, &c->mGy);
      launch_A_m(c, true, {&c->mGx, &c->mGy});
    } else {
      launch_sphi(c, ew, s, y_start);
      launch_A_m(c, true, {&c->mPhi, &c->mPhiy});
    }
  }
}

// A persistent row kernel walks nb row blocks with g workgroups in ceil(nb / g) rounds, and the last round is as long as
// the others however few blocks it holds.  Of all grids that fit into `cus` CUs this is the SMALLEST one that needs no more
// rounds than `cus` itself would: the row kernel loses nothing against `cus`, the CUs it gives up go to the other stream,
// and the idle share of its last round, rounds * g / nb - 1, is below rounds / nb (nb = 4096: 171 -> 171 in 24 rounds,
// 0.2 %; 160 -> 158 in 26 rounds, 0.3 %).
#define NQ_OVERLAP_CUS_DEFAULT 128     /* 4096^2: wave-PV grid 128 = 32 full rounds; from the sweep in DESIGN.md section 8 */
int nq_overlap_grid(int nb, int cus) {
  if (nb < 1 || cus < 1) return 0;
  if (cus >= nb) return nb;
  const int rounds = (nb + cus - 1) / cus;
  return (nb + rounds - 1) / rounds;
}

int nq_overlap_default_cus(int nx) { return nx == 4096 ? NQ_OVERLAP_CUS_DEFAULT : 0; }
int nq_row_grid_info(const nq_ctx* c, int* out6) {
  if (!c || !out6) return -1;
  out6[0] = c->num_cu;
  out6[1] = c->reserve_cus;
  with_row_size(c->N, [&](auto n) {
    constexpr int N = decltype(n)::value;
    const RowGrid p = row_grid<N>(c, RG_PRODUCTS, c->Nloc), w = row_grid<N>(c, RG_WAVEPV, c->Nloc);
    out6[2] = p.grid;
    out6[3] = p.nb;
    out6[4] = w.grid;
    out6[5] = w.nb;
  });
  return 0;
}
int nq_overlap_info(const nq_ctx* c, int* out3) {
  if (!c || !out3) return -1;
  out3[0] = c->stream2 ? c->overlap_cus : 0;
  out3[1] = c->stream2 ? c->overlap_grid : 0;
  out3[2] = c->stream2 ? c->num_cu : 0;
  return 0;
}

// CoupledModel, one rank: same kernels as do_step, but the q update waits until the wave-PV row kernel starts and
// runs beside it on a second stream.  The wave-PV kernel is bound by its row transforms and uses a persistent grid of
// overlap_grid workgroups; the spectral q kernels need 34 KB of LDS, which only the CUs it left free can give.
// The fork is recorded after the inverse columns of phi, phiy and the wait is queued on stream2 BEFORE the host reaches
// launch_wavepv, so both branches become ready at the same moment: beside k_s_phi or k_y_A (memory-bound as well) the
// q branch would gain nothing.
// The join sits as late as the data allow: k_s_invert is the first reader of the new qh, the forward columns of a, b before it
// touch neither qh nor uq, vq, and whichever branch ends first no longer leaves its CUs idle until the other one is done.
// Invariant of the join: the main stream waits for ev_join before k_s_invert of the SAME stage, so after every stage
// and when do_step_overlap returns, all work of stream2 is ordered before whatever the main stream runs next.  Every reader
// of the state (set_q / set_phi, the getters, diagnostics, nq_tick_snapshot, the particles' sampling before and after a
// step, stage4_uv_max after stage 2, the next step's fork) is issued on the main stream and needs no second wait.
static void do_step_overlap(nq_ctx* c) {
  hipStream_t main_stream = c->stream;
  for (int s = 0; s < 4; ++s) {
    phase_products(c, s);
    int qslot = 0, wslot = 0;
    launch_A_m(c, false, {&c->mW});
    const int cur = c->w.cur;
    const cd* y_start = (s == 0) ? c->w.y[cur] : (s == 1 ? c->w.y[(cur + 1) % 3] : c->w.y[(cur + 2) % 3]);
    EtdArrays ew = etd_arrays(c->w, s, &wslot);
    launch_sphi(c, ew, s, y_start);
    launch_A_m(c, true, {&c->mPhi, &c->mPhiy});
    (void)hipEventRecord(c->ev_fork, main_stream);
    c->stream = c->stream2;                                   // every launch helper uses c->stream
    (void)hipStreamWaitEvent(c->stream2, c->ev_fork, 0);
    launch_A_m(c, false, {&c->mUq, &c->mVq});
    EtdArrays eq = etd_arrays(c->q, s, &qslot);
    launch_sq(c, eq, s);
    (void)hipEventRecord(c->ev_join, c->stream2);
    c->stream = main_stream;
    phase_wavepv(c);
    phase_invert(c, s, c->ev_join);                           // joins between the forward columns of a, b and k_s_invert
    if (s == 2 && c->uv4_now) (void)stage4_uv_max(c);
  }
  phase_budget_sums(c);
  phase_budget_finish(c);
}

static void do_step(nq_ctx* c) {      // P == 1
  if (c->ybj) return do_step_ybj(c);
  if (c->stream2) return do_step_overlap(c);       // nq_create made stream2 only where this step applies
  for (int s = 0; s < 4; ++s) {
    phase_products(c, s);
    phase_update(c, s);
    if (c->p.model == NQ_MODEL_COUPLED) {
      phase_wavepv(c);
      phase_invert(c, s);
    }
    if (s == 2 && c->uv4_now) (void)stage4_uv_max(c);
  }
  if (c->bud && c->nww <= 256 && c->nwq <= 256) {            // few partials (grids <= 512): sums and accumulation in one launch
    hipLaunchKernelGGL(k_budget_small, dim3(1), dim3(1024), 0, c->stream, budget_acc(c), c->bsums);
    return;
  }
  phase_budget_sums(c);
  phase_budget_finish(c);
}


// ==================================================================================================================
// The slab step inside the library (include/niwqg_amd.h: nq_slab_step)
// ==================================================================================================================
enum { LINK_NONE = 0, LINK_PEERS = 1, LINK_RCCL = 2, LINK_CALLBACK = 3, LINK_NULL = 4 };

// Iterating the contexts of a group makes each context's device current before its loop body runs: with peers on DIFFERENT
// devices of one process (nq_slab_attach_peers, round 4) every launch, event record and copy has to be issued with the owner's
// device current.  On one device it is a thread-local no-op.
struct EachCtx {
  std::vector<nq_ctx*>& g;
  struct It {
    nq_ctx** p;
    nq_ctx* operator*() const {
      (void)hipSetDevice((*p)->device);
      return *p;
    }
    It& operator++() { ++p; return *this; }
    bool operator!=(const It& o) const { return p != o.p; }
  };
  It begin() const { return It{g.data()}; }
  It end() const { return It{g.data() + g.size()}; }
};
static inline EachCtx each(std::vector<nq_ctx*>& g) { return EachCtx{g}; }


// RCCL, taken from the process at run time (torch ships its own librccl and has usually loaded it already)
struct NcclId { char internal[128]; };
struct RcclApi {
  void* handle = nullptr;
  int (*GetUniqueId)(NcclId*) = nullptr;
  int (*CommInitRank)(void**, int, NcclId, int) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  int (*Send)(const void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*Recv)(void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
};
static RcclApi g_rccl;
static const int kNcclDouble = 8, kNcclSum = 0;
static bool rccl_load(std::string* err) {
  if (g_rccl.handle) return true;
  const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
  void* h = nullptr;
  // NIWQG_AMD_RCCL_LIB: an explicit library instead (tests/mock_rccl: rank THREADS on one GPU)
  const char* forced = getenv("NIWQG_AMD_RCCL_LIB");
  if (forced && *forced && !(h = dlopen(forced, RTLD_NOW | RTLD_LOCAL))) {
    const char* e = dlerror();                  // ONE call: dlerror() clears its state, a second call returns NULL
    *err = std::string("NIWQG_AMD_RCCL_LIB: ") + (e ? e : "?");
    return false;
  }
  for (const char* n : names)
    if (!h && (h = dlopen(n, RTLD_NOW | RTLD_NOLOAD))) break;          // the copy the process already uses, if any
  for (const char* n : names) {
    if (h) break;
    h = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
  }
  if (!h) {
    const char* e = dlerror();
    *err = std::string("librccl not found: ") + (e ? e : "?");
    return false;
  }
#define SYM_(field, name)                                                  \
  g_rccl.field = reinterpret_cast<decltype(g_rccl.field)>(dlsym(h, name)); \
  if (!g_rccl.field) {                                                     \
    *err = std::string("librccl lacks ") + name;                           \
    return false;                                                          \
  }
  SYM_(GetUniqueId, "ncclGetUniqueId") SYM_(CommInitRank, "ncclCommInitRank") SYM_(CommDestroy, "ncclCommDestroy")
  SYM_(GroupStart, "ncclGroupStart") SYM_(GroupEnd, "ncclGroupEnd") SYM_(Send, "ncclSend") SYM_(Recv, "ncclRecv")
  SYM_(AllReduce, "ncclAllReduce") SYM_(GetErrorString, "ncclGetErrorString")
#undef SYM_
  g_rccl.handle = h;
  return true;
}
#define NCCLCHK(ctx, call)                                                                                       \
  do {                                                                                                           \
    int r_ = (call);                                                                                             \
    if (r_ != 0) NQ_FAIL(ctx, -6, "%s failed: %s", #call, g_rccl.GetErrorString ? g_rccl.GetErrorString(r_) : "?"); \
  } while (0)

static int slab_link_setup(nq_ctx* c) {        // exchange stream and events, once
  if (c->mstream) return 0;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamCreateWithFlags(&c->mstream, hipStreamNonBlocking));
  for (int i = 0; i < 8; ++i) HIPCHK(c, hipEventCreateWithFlags(&c->ev_prod[i], hipEventDisableTiming));
  for (int g = 0; g < 5; ++g)
    for (int i = 0; i < 8; ++i) HIPCHK(c, hipEventCreateWithFlags(&c->ev_arr[g][i], hipEventDisableTiming));
  HIPCHK(c, hipEventCreateWithFlags(&c->ev_col, hipEventDisableTiming));
  HIPCHK(c, hipEventCreateWithFlags(&c->ev_done, hipEventDisableTiming));
  HIPCHK(c, hipEventCreateWithFlags(&c->ev_red, hipEventDisableTiming));
  return 0;
}
// the contexts one call drives: every rank of the process in peers mode, otherwise this rank alone
static int slab_group(nq_ctx* c, std::vector<nq_ctx*>* g) {
  if (c->link == LINK_NONE) {
    if (c->P != 1) NQ_FAIL(c, -4, "slab context without a link: call nq_comm_init, nq_slab_attach_peers or nq_slab_set_callbacks first");
    c->peers.assign(1, c);                       // one rank: its own blocks cross by device copies
    c->link = LINK_PEERS;
  }
  if (c->link == LINK_PEERS) {
    if (c->rank != 0) NQ_FAIL(c, -4, "peers mode: drive the group through its rank-0 context");
    *g = c->peers;
  } else {
    g->assign(1, c);
  }
  for (nq_ctx* x : *g) {
    int rc = slab_link_setup(x);
    if (rc) return rc;
  }
  return 0;
}
static int effective_chunks(const nq_ctx* c) {
  if (c->link == LINK_CALLBACK) return 1;
  int rows_per_wg = 1;
  with_row_size(c->N, [&](auto n) {
    constexpr int N = decltype(n)::value;
    rows_per_wg = XPlan<N>::C > XPlan1<N>::C ? XPlan<N>::C : XPlan1<N>::C;
  });
  int n = c->nchunk < 1 ? 1 : (c->nchunk > 8 ? 8 : c->nchunk);
  while (n > 1 && (c->Nloc % (n * rows_per_wg) != 0)) n >>= 1;
  return n;
}
struct XTimer {                                  // optional HIP-event pair around one exchange chunk (or one all-reduce) on the exchange stream
  nq_ctx* c;
  bool on;
  std::vector<hipEvent_t>& ev;
  size_t& used;
  hipStream_t xs;
  explicit XTimer(nq_ctx* c_, bool reduce = false, hipStream_t xs_ = nullptr)
      : c(c_), on(c_->xtime), ev(reduce ? c_->rev : c_->xev), used(reduce ? c_->rev_used : c_->xev_used), xs(xs_ ? xs_ : c_->mstream) {
    if (!on) return;
    if (used + 2 > ev.size()) {
      // the pool only shrinks in nq_slab_counters(reset): a caller that leaves timing on for a long run() gets the first
      // 16384 exchanges / all-reduces timed and the rest untimed instead of an event pool that grows without bound
      if (ev.size() >= 2 * 16384) { on = false; return; }
      for (int i = 0; i < 2; ++i) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) { on = false; return; }
        ev.push_back(e);
      }
    }
    (void)hipEventRecord(ev[used], xs);
  }
  ~XTimer() {
    if (!on) return;
    (void)hipEventRecord(ev[used + 1], xs);
    used += 2;
  }
};

// Chunk i of nch of exchange group g, for every rank of grp.  to_y: x side -> y side (the producers' row kernels recorded
// ev_prod[i]); else y side -> x side (the column kernels recorded ev_col).  Both buffers of a group are cut into P blocks of
// Nloc rows; chunk i is the same row range inside every block.
// An exchange that nothing can run under -- one chunk, and not group 1, whose transfer the q update hides -- gains nothing from the
// second stream and pays two event hand-offs between the streams (~25-35 us per exchange on one GPU, 0.3-0.4 ms of a 2.2 ms rank
// step at 4096^2 / P = 8: profiles/r04_rank_of_P_measurements.txt): it is issued on the compute stream itself.
// NIWQG_AMD_SLAB_INLINE=0 keeps every exchange on the exchange stream.
static bool inline_exchange(const nq_ctx* c, int g, int nch) {
  static int on = -1;
  if (on < 0) {
    const char* e = getenv("NIWQG_AMD_SLAB_INLINE");
    on = (e && atoi(e) == 0) ? 0 : 1;
  }
  return on && nch == 1 && g != 1 && c->link != LINK_CALLBACK;
}
static int issue_chunk(std::vector<nq_ctx*>& grp, int g, bool to_y, int i, int nch) {
  nq_ctx* c0 = grp[0];
  if (c0->G[g].elems == 0) return 0;
  const size_t blk = (size_t)c0->Nloc * c0->G[g].pitch, cblk = blk / nch, off = (size_t)i * cblk;
  const bool inl = inline_exchange(c0, g, nch);
  for (nq_ctx* c : each(grp)) {
    cd* send = to_y ? c->G[g].bx : c->G[g].by;
    cd* recv = to_y ? c->G[g].by : c->G[g].bx;
    hipEvent_t mine = to_y ? c->ev_prod[i] : c->ev_col;
    if (c->link == LINK_CALLBACK) {
      if (i == 0) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (!c->xcb) NQ_FAIL(c, -4, "no exchange callback");
        const int rc = c->xcb(c->cb_user, g, to_y ? 1 : 0);
        if (rc) NQ_FAIL(c, -6, "exchange callback failed (%d)", rc);
        c->n_exch += 1;
        c->bytes_sent += (double)blk * 16.0 * (c->P - 1);
      }
      continue;
    }
    const hipStream_t xs = inl ? c->stream : c->mstream;       // the stream this exchange runs on
    if (!inl) HIPCHK(c, hipStreamWaitEvent(xs, mine, 0));
    {
      XTimer xt(c, false, xs);
      if (c->link == LINK_PEERS) {
        for (nq_ctx* s : grp)
          if (!(inl && s == c)) HIPCHK(c, hipStreamWaitEvent(xs, to_y ? s->ev_prod[i] : s->ev_col, 0));
        for (nq_ctx* s : grp) {
          if (s == c && c->redir_now) continue;  // the own block: the A sub-passes use it where it is (ArrayListR)
          const cd* src = (to_y ? s->G[g].bx : s->G[g].by) + (size_t)c->rank * blk + off;
          HIPCHK(c, hipMemcpyAsync(recv + (size_t)s->rank * blk + off, src, cblk * sizeof(cd), hipMemcpyDeviceToDevice, xs));
        }
      } else if (c->link == LINK_NULL) {         // one rank of P measured alone: only its own block crosses (device copy)
        if (!c->redir_now)
          HIPCHK(c, hipMemcpyAsync(recv + (size_t)c->rank * blk + off, send + (size_t)c->rank * blk + off, cblk * sizeof(cd), hipMemcpyDeviceToDevice, xs));
      } else {                                   // RCCL: one grouped send/recv pair per peer, the own block by a device copy
        NCCLCHK(c, g_rccl.GroupStart());
        for (int p = 0; p < c->P; ++p) {
          if (p == c->rank) continue;
          NCCLCHK(c, g_rccl.Send(send + (size_t)p * blk + off, 2 * cblk, kNcclDouble, p, c->comm, xs));
          NCCLCHK(c, g_rccl.Recv(recv + (size_t)p * blk + off, 2 * cblk, kNcclDouble, p, c->comm, xs));
        }
        NCCLCHK(c, g_rccl.GroupEnd());
        if (!c->redir_now)
          HIPCHK(c, hipMemcpyAsync(recv + (size_t)c->rank * blk + off, send + (size_t)c->rank * blk + off, cblk * sizeof(cd), hipMemcpyDeviceToDevice, xs));
      }
    }
    c->n_exch += 1;
    if (c->link != LINK_NULL) c->bytes_sent += (double)cblk * 16.0 * (c->P - 1);
    if (to_y) {
      if (i == nch - 1) HIPCHK(c, hipEventRecord(c->ev_done, xs));
    } else {
      HIPCHK(c, hipEventRecord(c->ev_arr[g][i], xs));
      c->arr_pending[g] = true;
    }
  }
  return 0;
}
static int wait_arrival(nq_ctx* c, int g, int i, int nch_now) {
  // the group was sent with the step's chunking; a caller that uses fewer chunks waits for all the chunks it covers
  if (!c->arr_pending[g] || c->link == LINK_CALLBACK) return 0;
  const int sent = effective_chunks(c);
  const int per = sent / nch_now > 0 ? sent / nch_now : 1;
  for (int k = i * per; k < (i + 1) * per && k < sent; ++k) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_arr[g][k], 0));
  return 0;
}
static void set_window(nq_ctx* c, int i, int nch) {
  c->nrows = c->Nloc / nch;
  c->row0 = i * c->nrows;
}
#define SLABTRY(call)          \
  do {                         \
    int rc__ = (call);         \
    if (rc__) return rc__;     \
  } while (0)

// whole group g at once, complete on the compute streams when this returns to the caller's next launch
static int exchange_now(std::vector<nq_ctx*>& grp, int g, bool to_y) {
  if (grp.size() == 1 && grp[0]->P == 1 && grp[0]->G[g].bx == grp[0]->G[g].by) return 0;      // one rank, one buffer
  for (nq_ctx* c : each(grp)) HIPCHK(c, hipEventRecord(to_y ? c->ev_prod[0] : c->ev_col, c->stream));
  const int sent = effective_chunks(grp[0]);
  if (to_y) {
    SLABTRY(issue_chunk(grp, g, true, 0, 1));
    for (nq_ctx* c : each(grp))
      if (c->link != LINK_CALLBACK) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_done, 0));
  } else {
    // arrival events are per chunk of the step's chunking: send it that way so that later waits find every event recorded
    for (int i = 0; i < sent; ++i) SLABTRY(issue_chunk(grp, g, false, i, sent));
    for (nq_ctx* c : each(grp))
      for (int i = 0; i < sent; ++i) SLABTRY(wait_arrival(c, g, i, sent));
  }
  return 0;
}

struct PeerBufs { double* p[8]; };
__global__ void k_peer_allreduce(PeerBufs b, int P, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  for (int r = 0; r < P; ++r) s += b.p[r][i];
  for (int r = 0; r < P; ++r) b.p[r][i] = s;
}
// sum over ranks of n doubles at offset `lo` of each rank's reduction block (bsums), or of its 32 diagnostic sums (which = 4)
static double* red_ptr(nq_ctx* c, int which, int* n) {
  switch (which) {
    case 0: *n = 44; return c->bsums;
    case 1: *n = 4; return c->carryW;
    case 2: *n = 3; return c->carryQ;
    case 3: *n = 1; return c->gradS1;
    case 4: *n = 16; return c->diag_out;           // diagnostics tick, spectral half
    case 5: *n = 16; return c->diag_out ? c->diag_out + 16 : nullptr;   // physical half
    default: *n = 0; return nullptr;
  }
}
static int slab_allreduce(std::vector<nq_ctx*>& grp, int which) {
  if (grp.size() == 1 && grp[0]->P == 1) return 0;      // one rank: its sums are the sums (as exchange_now)
  nq_ctx* c0 = grp[0];
  int n = 0;
  if (!red_ptr(c0, which, &n)) NQ_FAIL(c0, -1, "slab_allreduce: which = %d", which);
  if (c0->link == LINK_CALLBACK) {
    for (nq_ctx* c : each(grp)) {
      HIPCHK(c, hipStreamSynchronize(c->stream));
      if (!c->rcb) NQ_FAIL(c, -4, "no all-reduce callback");
      const int rc = c->rcb(c->cb_user, which);
      if (rc) NQ_FAIL(c, -6, "all-reduce callback failed (%d)", rc);
    }
    return 0;
  }
  if (c0->link == LINK_NULL) return 0;           // one rank of P measured alone: its partial sums stay partial
  if (c0->link == LINK_PEERS) {
    if (grp.size() == 1) return 0;
    PeerBufs pb;
    for (size_t r = 0; r < grp.size(); ++r) {
      pb.p[r] = red_ptr(grp[r], which, &n);
      HIPCHK(grp[r], hipSetDevice(grp[r]->device));
      HIPCHK(grp[r], hipEventRecord(grp[r]->ev_red, grp[r]->stream));
    }
    HIPCHK(c0, hipSetDevice(c0->device));       // the reduction runs on rank 0's device and reads / writes the peers' sums in place
    for (size_t r = 0; r < grp.size(); ++r) HIPCHK(c0, hipStreamWaitEvent(c0->mstream, grp[r]->ev_red, 0));
    {
      XTimer xt(c0, true);
      hipLaunchKernelGGL(k_peer_allreduce, dim3(1), dim3(64), 0, c0->mstream, pb, (int)grp.size(), n);
    }
    HIPCHK(c0, hipEventRecord(c0->ev_done, c0->mstream));
    for (nq_ctx* c : each(grp)) HIPCHK(c, hipStreamWaitEvent(c->stream, c0->ev_done, 0));
    return 0;
  }
  for (nq_ctx* c : each(grp)) {                        // RCCL
    double* p = red_ptr(c, which, &n);
    HIPCHK(c, hipEventRecord(c->ev_red, c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->mstream, c->ev_red, 0));
    {
      XTimer xt(c, true);
      NCCLCHK(c, g_rccl.AllReduce(p, p, (size_t)n, kNcclDouble, kNcclSum, c->comm, c->mstream));
    }
    HIPCHK(c, hipEventRecord(c->ev_done, c->mstream));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_done, 0));
  }
  return 0;
}

// UPDATE split in two for the coupled model: the phi half produces exchange group 1, the q half runs under its transfer
static void phase_update_phi(nq_ctx* c, int s) {
  int wslot = 0;
  launch_A_m(c, false, {&c->mW});
  const int cur = c->w.cur;
  const cd* y_start = (s == 0) ? c->w.y[cur] : (s == 1 ? c->w.y[(cur + 1) % 3] : c->w.y[(cur + 2) % 3]);
  EtdArrays ew = etd_arrays(c->w, s, &wslot);
  launch_sphi(c, ew, s, y_start);
  launch_A_m(c, true, {&c->mPhi, &c->mPhiy});
}
static void phase_update_q(nq_ctx* c, int s) {
  int qslot = 0;
  launch_A_m(c, false, {&c->mUq, &c->mVq});
  EtdArrays eq = etd_arrays(c->q, s, &qslot);
  launch_sq(c, eq, s);
}

// YBJModel's stage graph (do_step_ybj) on slabs: only the wave products cross x -> y (group 0); the stage results 0..2
// come back in group 4 (gradients for the next stage), the new state in group 1
static int slab_step_ybj(std::vector<nq_ctx*>& grp) {
  nq_ctx* c0 = grp[0];
  const int nch = effective_chunks(c0);
  for (int s = 0; s < 4; ++s) {
    for (int i = 0; i < nch; ++i) {
      for (nq_ctx* c : each(grp)) {
        SLABTRY(wait_arrival(c, 3, i, nch));
        SLABTRY(wait_arrival(c, 1, i, nch));
        SLABTRY(wait_arrival(c, 4, i, nch));
        set_window(c, i, nch);
        launch_products(c, -1.0, -0.5, s == 0);
        HIPCHK(c, hipEventRecord(c->ev_prod[i], c->stream));
      }
      SLABTRY(issue_chunk(grp, 0, true, i, nch));
    }
    for (nq_ctx* c : each(grp)) {
      set_window(c, 0, 1);
      if (c->link != LINK_CALLBACK) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_done, 0));
      launch_A_m(c, false, {&c->mW});
      int wslot = 0;
      const int cur = c->w.cur;
      const cd* y_start = (s == 0) ? c->w.y[cur] : (s == 1 ? c->w.y[(cur + 1) % 3] : c->w.y[(cur + 2) % 3]);
      EtdArrays ew = etd_arrays(c->w, s, &wslot);
      if (s < 3) {
        launch_sphi(c, ew, s, y_start, &c->mGx, &c->mGy);
        launch_A_m(c, true, {&c->mGx, &c->mGy});
      } else {
        launch_sphi(c, ew, s, y_start);
        launch_A_m(c, true, {&c->mPhi, &c->mPhiy});
      }
      HIPCHK(c, hipEventRecord(c->ev_col, c->stream));
    }
    for (int i = 0; i < nch; ++i) SLABTRY(issue_chunk(grp, s < 3 ? 4 : 1, false, i, nch));
  }
  for (nq_ctx* c : each(grp)) c->n_steps += 1;
  return 0;
}

static int slab_step_once(std::vector<nq_ctx*>& grp) {
  nq_ctx* c0 = grp[0];
  if (c0->ybj) return slab_step_ybj(grp);
  const bool coupled = c0->p.model == NQ_MODEL_COUPLED, waves = c0->kernel_family;
  const int nch = effective_chunks(c0);
  for (int s = 0; s < 4; ++s) {
    if (s == 3 && c0->uv4_now)
      for (nq_ctx* c : each(grp)) {                   // the fourth stage's u, v have just arrived on the x side (group 3)
        for (int i = 0; i < nch; ++i) SLABTRY(wait_arrival(c, 3, i, nch));
        set_window(c, 0, 1);
        SLABTRY(stage4_uv_max(c));
      }
    // rows: nonlinear products, chunk by chunk; chunk i leaves as soon as it is done
    for (int i = 0; i < nch; ++i) {
      for (nq_ctx* c : each(grp)) {
        SLABTRY(wait_arrival(c, 3, i, nch));
        if (waves) SLABTRY(wait_arrival(c, 1, i, nch));
        set_window(c, i, nch);
        phase_products(c, s);
        HIPCHK(c, hipEventRecord(c->ev_prod[i], c->stream));
      }
      SLABTRY(issue_chunk(grp, 0, true, i, nch));
    }
    for (nq_ctx* c : each(grp)) {
      set_window(c, 0, 1);
      if (c->link != LINK_CALLBACK) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_done, 0));
    }
    if (coupled) {
      for (nq_ctx* c : each(grp)) {
        phase_update_phi(c, s);
        HIPCHK(c, hipEventRecord(c->ev_col, c->stream));
      }
      for (int i = 0; i < nch; ++i) SLABTRY(issue_chunk(grp, 1, false, i, nch));
      for (nq_ctx* c : each(grp)) phase_update_q(c, s);                    // under the transfer of group 1
      for (int i = 0; i < nch; ++i) {
        for (nq_ctx* c : each(grp)) {
          SLABTRY(wait_arrival(c, 1, i, nch));
          set_window(c, i, nch);
          phase_wavepv(c);
          HIPCHK(c, hipEventRecord(c->ev_prod[i], c->stream));
        }
        SLABTRY(issue_chunk(grp, 2, true, i, nch));
      }
      for (nq_ctx* c : each(grp)) {
        set_window(c, 0, 1);
        if (c->link != LINK_CALLBACK) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_done, 0));
        phase_invert(c, s);
        HIPCHK(c, hipEventRecord(c->ev_col, c->stream));
      }
      for (int i = 0; i < nch; ++i) SLABTRY(issue_chunk(grp, 3, false, i, nch));
    } else {
      for (nq_ctx* c : each(grp)) {
        phase_update(c, s);                                            // includes the (spectral) inversion
        HIPCHK(c, hipEventRecord(c->ev_col, c->stream));
      }
      if (waves)
        for (int i = 0; i < nch; ++i) SLABTRY(issue_chunk(grp, 1, false, i, nch));
      for (int i = 0; i < nch; ++i) SLABTRY(issue_chunk(grp, 3, false, i, nch));
    }
  }
  if (c0->bud) {
    for (nq_ctx* c : each(grp)) phase_budget_sums(c);
    SLABTRY(slab_allreduce(grp, 0));
    for (nq_ctx* c : each(grp)) phase_budget_finish(c);
  }
  for (nq_ctx* c : each(grp)) c->n_steps += 1;
  return 0;
}
// every arrival of the last step has to be on the compute stream before anybody else (a read, a set_q, a sync) touches the x side
static int slab_settle(std::vector<nq_ctx*>& grp) {
  for (nq_ctx* c : each(grp)) {
    const int sent = effective_chunks(c);
    for (int g = 0; g < 5; ++g)
      if (c->arr_pending[g]) {
        for (int i = 0; i < sent; ++i) SLABTRY(wait_arrival(c, g, i, sent));
        c->arr_pending[g] = false;
      }
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------
// diagnostics tick launches
static void launch_project(nq_ctx* c, double* part) {
  with_col_plan(c, [&](auto s1, auto cly) {
    constexpr int S = decltype(s1)::value, CLX = decltype(cly)::value;
    typedef YPlanT<S, CLX> Y;
    hipLaunchKernelGGL((k_s_project<S, CLX>), dim3(c->Wf / CLX, c->S2), dim3(Y::THREADS), Y::LDS_BYTES, c->stream, c->mW,
                       (const cd*)c->w.y[c->w.cur], geom_full(c), c->kk, c->ll, c->tw, 1, c->p.nu4w, c->p.nuw, c->p.muw, part);
  });
}
// the passive scalar's Gamma_c projection: B-fft of Muc, Mvc against c-hat; one partial per workgroup, their count returned
static int launch_project_c(nq_ctx* x, const cd* ch, double* part) {
  const YGeom g = geom_half(x);
  if (g.width <= 0) return 0;
  with_col_plan(x, [&](auto s1, auto cly) {
    constexpr int S = decltype(s1)::value, CLX = decltype(cly)::value;
    typedef YPlanT<S, CLX> Y;
    hipLaunchKernelGGL((k_s_project_c<S, CLX>), dim3((g.width + CLX - 1) / CLX, x->S2), dim3(Y::THREADS), Y::LDS_BYTES, x->stream, x->mUc, x->mVc, ch, g, x->kk, x->ll, x->tw, 1, part);
  });
  return ((g.width + x->CLy - 1) / x->CLy) * x->S2;
}
// the tick's two products passes: which = 0 leaves J = u phix + v phiy in Mw (c_J = 1, c_R = 0), which = 1 i phi q_psi (0, 1)
static void launch_products_pass(nq_ctx* x, int which) { launch_products(x, which == 0 ? 1.0 : 0.0, which == 0 ? 0.0 : 1.0); }
// Physical space sees the mean of the two copies of q-hat: formed in a scratch plane (scr_f1 on one rank, where scr_h1 is a
// plane of the transfer; a lazily allocated scr_h1 on a slab rank) that *qh then names.  One copy: *qh is left alone.
static int mean_qh(nq_ctx* x, const cd** qh) {
  if (!x->dual) return 0;
  if (x->P > 1 && !x->scr_h1) ALLOC(x, x->scr_h1, (size_t)x->N * x->Ph);
  cd* mean = x->P > 1 ? x->scr_h1 : x->scr_f1;
  if (x->Wh > 0) hipLaunchKernelGGL(k_avg_interior, dim3((x->Wh + 63) / 64, x->N), dim3(64), 0, x->stream, *qh, (const cd*)x->q2.y[x->q2.cur], mean, x->Wh, x->Ph, x->N, x->kh0);
  *qh = mean;
  return 0;
}
// out <- the sum, in rank order on the host, of the `count` doubles every context of the group holds at x->*sums: the first
// rank's are copied (a -0.0 shell sum of a single rank stays -0.0), the others added
static int sum_ranks_on_host(std::vector<nq_ctx*>& grp, double* nq_ctx::*sums, size_t count, double* out) {
  std::vector<double> part(grp.size() > 1 ? count : 0);
  for (nq_ctx* x : each(grp)) {
    double* dst = x == grp[0] ? out : part.data();
    HIPCHK(x, hipGetLastError());
    HIPCHK(x, hipMemcpyAsync(dst, x->*sums, sizeof(double) * count, hipMemcpyDeviceToHost, x->stream));
    SLABTRY(nq_sync(x));
    if (dst != out)
      for (size_t i = 0; i < count; ++i) out[i] += part[i];
  }
  return 0;
}
static void launch_project_bin(nq_ctx* c, double* rlap, double* rdiss) {
  with_col_plan(c, [&](auto s1, auto cly) {
    constexpr int S = decltype(s1)::value, CLX = decltype(cly)::value;
    typedef YPlanT<S, CLX> Y;
    hipLaunchKernelGGL((k_s_project_bin<S, CLX>), dim3(c->Wf / CLX, c->S2), dim3(Y::THREADS), Y::LDS_BYTES, c->stream, c->mW,
                       (const cd*)c->w.y[c->w.cur], geom_full(c), c->kk, c->ll, c->tw, 1, c->p.nu4w, c->p.nuw, c->p.muw, rlap, rdiss, c->Wf);
  });
}
template <int MODE, bool SLAB>
static void launch_xdiag_t(nq_ctx* c, double qbar, double abar, double* part) {
  with_row_size(c->N, [&](auto n) {
    constexpr int N = decltype(n)::value;
    typedef XPlan<N> X;
    hipLaunchKernelGGL((k_x_diag<N, MODE, SLAB>), dim3(c->Nloc / X::C), dim3(X::THREADS), X::LDS_BYTES, c->stream, c->mQ, c->mQw, c->mPhi, c->twx, c->kk, qbar, abar, part);
  });
}
template <int MODE>
static void launch_xdiag_m(nq_ctx* c, double qbar, double abar, double* part) {
  if (c->P > 1) launch_xdiag_t<MODE, true>(c, qbar, abar, part);
  else launch_xdiag_t<MODE, false>(c, qbar, abar, part);
}
static int xdiag_blocks(const nq_ctx* c) {
  int nb = 0;
  with_row_size(c->N, [&](auto n) { nb = c->Nloc / XPlan<decltype(n)::value>::C; });
  return nb;
}

// PDFs of the physical fields (csrc/nq_hist.hpp): the tick's row pass with the binning (or the min/max) in place of the sums
template <int MODE, bool SLAB, bool MINMAX>
static void launch_xhist_t(nq_ctx* c, const HistArgs& h, double* part) {
  const int words = MINMAX ? 0 : hist_words(h.bins, h.jbins);
  with_row_size(c->N, [&](auto n) {
    constexpr int N = decltype(n)::value;
    typedef XPlan<N> X;
    hipLaunchKernelGGL((k_x_hist<N, MODE, SLAB, MINMAX>), dim3(c->Nloc / X::C), dim3(X::THREADS), hist_lds_bytes<N>(words), c->stream, c->mQ, c->mQw, c->mPhi, c->twx, c->kk, h, part);
  });
}
template <bool MINMAX>
static void launch_xhist(nq_ctx* c, const HistArgs& h, double* part) {
  if (c->p.model == NQ_MODEL_COUPLED) launch_xhist_t<MODE_COUPLED, false, MINMAX>(c, h, part);
  else launch_xhist_t<MODE_UNCOUPLED, false, MINMAX>(c, h, part);
}
// time-mean and covariance maps (csrc/nq_avg.hpp): the same row pass with the read-add-write of the sum planes after it
template <int MODE>
static void launch_xmoments_t(nq_ctx* c, const AvgArgs& a) {
  with_row_size(c->N, [&](auto n) {
    constexpr int N = decltype(n)::value;
    typedef XPlan<N> X;
    hipLaunchKernelGGL((k_x_moments<N, MODE, false>), dim3(c->Nloc / X::C), dim3(X::THREADS), X::LDS_BYTES, c->stream, c->mQ, c->mQw, c->mPhi, c->twx, c->kk, a);
  });
}
static void launch_xmoments(nq_ctx* c, const AvgArgs& a) {
  if (c->p.model == NQ_MODEL_COUPLED) launch_xmoments_t<MODE_COUPLED>(c, a);
  else launch_xmoments_t<MODE_UNCOUPLED>(c, a);
}
// the same two on the selected values of x_flow_values (csrc/nq_flow.hpp)
template <int MODE, bool MINMAX>
static void launch_xflow_hist_t(nq_ctx* c, const FlowSel& sel, const HistArgs& h, double* part) {
  const int words = MINMAX ? 0 : hist_words(h.bins, h.jbins);
  with_row_size(c->N, [&](auto n) {
    constexpr int N = decltype(n)::value;
    typedef XPlan<N> X;
    hipLaunchKernelGGL((k_x_flow_hist<N, MODE, false, MINMAX>), dim3(c->Nloc / X::C), dim3(X::THREADS), hist_lds_bytes<N>(words), c->stream, c->mQ, c->mQw, c->mU, c->mP, c->mPhi, c->mPhiy, c->twx, c->kk, sel, h, part);
  });
}
template <bool MINMAX>
static void launch_xflow_hist(nq_ctx* c, const FlowSel& sel, const HistArgs& h, double* part) {
  if (c->p.model == NQ_MODEL_COUPLED) launch_xflow_hist_t<MODE_COUPLED, MINMAX>(c, sel, h, part);
  else launch_xflow_hist_t<MODE_UNCOUPLED, MINMAX>(c, sel, h, part);
}
template <int MODE>
static void launch_xflow_moments_t(nq_ctx* c, const FlowSel& sel, const AvgArgs& a) {
  with_row_size(c->N, [&](auto n) {
    constexpr int N = decltype(n)::value;
    typedef XPlan<N> X;
    hipLaunchKernelGGL((k_x_flow_moments<N, MODE, false>), dim3(c->Nloc / X::C), dim3(X::THREADS), X::LDS_BYTES, c->stream, c->mQ, c->mQw, c->mU, c->mP, c->mPhi, c->mPhiy, c->twx, c->kk, sel, a);
  });
}
static void launch_xflow_moments(nq_ctx* c, const FlowSel& sel, const AvgArgs& a) {
  if (c->p.model == NQ_MODEL_COUPLED) launch_xflow_moments_t<MODE_COUPLED>(c, sel, a);
  else launch_xflow_moments_t<MODE_UNCOUPLED>(c, sel, a);
}
// structure functions (csrc/nq_sf.hpp): the same row pass with the increments out of LDS rows after it
template <int MODE>
static void launch_xflow_sf_t(nq_ctx* c, const FlowSel& sel, const SfArgs& a) {
  with_row_size(c->N, [&](auto n) {
    constexpr int N = decltype(n)::value;
    typedef XPlan<N> X;
    hipLaunchKernelGGL((k_x_flow_sf<N, MODE, false>), dim3(c->Nloc / X::C), dim3(X::THREADS), sf_lds_bytes<N>(a.nreal, a.phi), c->stream, c->mQ, c->mQw, c->mU, c->mP, c->mPhi, c->mPhiy, c->twx, c->kk, sel, a);
  });
}
static void launch_xflow_sf(nq_ctx* c, const FlowSel& sel, const SfArgs& a) {
  if (c->p.model == NQ_MODEL_COUPLED) launch_xflow_sf_t<MODE_COUPLED>(c, sel, a);
  else launch_xflow_sf_t<MODE_UNCOUPLED>(c, sel, a);
}
// structure functions at two-dimensional separations (csrc/nq_sf2.hpp): the same row pass with plain stores to physical planes
template <int MODE>
static void launch_xflow_store_t(nq_ctx* c, const FlowSel& sel, const Sf2Store& st) {
  with_row_size(c->N, [&](auto n) {
    constexpr int N = decltype(n)::value;
    typedef XPlan<N> X;
    hipLaunchKernelGGL((k_x_flow_store<N, MODE>), dim3(c->Nloc / X::C), dim3(X::THREADS), X::LDS_BYTES, c->stream, c->mQ, c->mQw, c->mU, c->mP, c->mPhi, c->mPhiy, c->twx, c->kk, sel, st);
  });
}
static void launch_xflow_store(nq_ctx* c, const FlowSel& sel, const Sf2Store& st) {
  if (c->p.model == NQ_MODEL_COUPLED) launch_xflow_store_t<MODE_COUPLED>(c, sel, st);
  else launch_xflow_store_t<MODE_UNCOUPLED>(c, sel, st);
}
// PDFs of the increments (csrc/nq_ipdf.hpp): the same row pass with the value rows and a table of counters per separation in LDS
template <int MODE>
static void launch_xflow_ipdf_t(nq_ctx* c, const FlowSel& sel, const IpdfArgs& a) {
  with_row_size(c->N, [&](auto n) {
    constexpr int N = decltype(n)::value;
    typedef XPlan<N> X;
    hipLaunchKernelGGL((k_x_flow_ipdf<N, MODE>), dim3(c->Nloc / X::C), dim3(X::THREADS), ipdf_lds_bytes<N>(a.nreal, a.phi, a.bins), c->stream, c->mQ, c->mQw, c->mU, c->mP, c->mPhi, c->mPhiy, c->twx, c->kk, sel, a);
  });
}
static void launch_xflow_ipdf(nq_ctx* c, const FlowSel& sel, const IpdfArgs& a) {
  if (c->p.model == NQ_MODEL_COUPLED) launch_xflow_ipdf_t<MODE_COUPLED>(c, sel, a);
  else launch_xflow_ipdf_t<MODE_UNCOUPLED>(c, sel, a);
}
// which kernel serves rows of `cols` elements of these fields: the row route (points per thread, threads, LDS bytes) or the global
// one.  The row route runs workgroups of up to 1024 threads with 1, 2, 4 or 8 points each; where the base values and the running
// sums of that layout pass 128 registers (three field slots at 4096 columns, two real fields at 8192) it runs 512 threads with
// twice the points (csrc/nq_sf2.hpp: sf2_tmax).  Past 4096 columns phi beside a real field and three real fields go the global way
// (at 8192 columns their rows exceed the LDS).
struct Sf2Route {
  bool lds;
  int pts, threads, nc;
  size_t lds_bytes;
};
static Sf2Route sf2_route(int cols, int nreal, int phi) {
  Sf2Route r = {};
  const int nf = nreal + phi;
  r.nc = nf == 1 ? sf_ncols<1>() : (nf == 2 ? sf_ncols<2>() : sf_ncols<3>());
  r.pts = 1;
  while (r.pts < 8 && (size_t)r.pts * SF2_MAX_THREADS < (size_t)cols) r.pts *= 2;
  r.lds = (size_t)r.pts * SF2_MAX_THREADS >= (size_t)cols;
  if (nf == 3 && r.pts == 4) r.pts = 8;                  // 512 threads
  else if (nf == 2 && !phi && r.pts == 8) r.pts = 16;    // 512 threads
  else if (r.pts == 8 && nf > 1) r.lds = false;
  r.threads = ((cols + r.pts - 1) / r.pts + 63) / 64 * 64;
  r.lds_bytes = ((size_t)(nreal + 2 * phi) * cols + 2 * (size_t)(r.threads / 64) * r.nc) * sizeof(double);
  if (r.lds_bytes > SF2_LDS_LIMIT) r.lds = false;
  if (!r.lds) {
    r.threads = SF2_GLOBAL_THREADS;
    r.lds_bytes = 0;
  }
  return r;
}
// workgroups of a call: one per row while the partials (blocks x vectors x columns) stay within NQ_SF_PART_MAX_BYTES
static int sf2_grid(int rows, int nvec, int nc) {
  const size_t most = (size_t)NQ_SF_PART_MAX_BYTES / ((size_t)nvec * nc * sizeof(double));
  return (size_t)rows < most ? rows : (int)most;
}
template <int NREAL, int PHI>
static void sf2_launch_fields(hipStream_t s, int nblk, const Sf2Route& r, const SfPlanes& pl, const Sf2Args& a) {
  constexpr int NF = NREAL + PHI;
  const dim3 g(nblk), b(r.threads);
  if (!r.lds) hipLaunchKernelGGL((k_sf_plane2_global<NREAL, PHI>), g, b, 0, s, pl, a);
  else if (r.pts == 1) hipLaunchKernelGGL((k_sf_plane2<1, NREAL, PHI>), g, b, r.lds_bytes, s, pl, a);
  else if (r.pts == 2) hipLaunchKernelGGL((k_sf_plane2<2, NREAL, PHI>), g, b, r.lds_bytes, s, pl, a);
  else if (r.pts == 4) {
    if constexpr (NF < 3) hipLaunchKernelGGL((k_sf_plane2<4, NREAL, PHI>), g, b, r.lds_bytes, s, pl, a);
  } else if (r.pts == 8) {
    if constexpr (NF != 2) hipLaunchKernelGGL((k_sf_plane2<8, NREAL, PHI>), g, b, r.lds_bytes, s, pl, a);
  } else {
    if constexpr (NREAL == 2 && PHI == 0) hipLaunchKernelGGL((k_sf_plane2<16, NREAL, PHI>), g, b, r.lds_bytes, s, pl, a);
  }
}
static_assert(sf2_lds_bytes<3, 0>(4096, 512) <= SF2_LDS_LIMIT && sf2_lds_bytes<2, 1>(4096, 512) <= SF2_LDS_LIMIT && sf2_lds_bytes<2, 0>(8192, 512) <= SF2_LDS_LIMIT &&
              sf2_lds_bytes<0, 1>(8192, 1024) <= SF2_LDS_LIMIT && sf2_lds_bytes<3, 0>(8192, 512) > SF2_LDS_LIMIT && sf2_lds_bytes<1, 1>(8192, 512) > SF2_LDS_LIMIT,
              "which rows take the row route (DESIGN.md section 5w)");
static_assert(sf2_tmax<8, 3, 0>() == 512 && sf2_tmax<8, 2, 1>() == 512 && sf2_tmax<16, 2, 0>() == 512 && sf2_tmax<8, 1, 0>() == 1024 && sf2_tmax<4, 2, 0>() == 1024,
              "sf2_route's thread counts are the kernels' launch bounds");
static void sf2_launch(hipStream_t s, int nblk, const Sf2Route& r, const SfPlanes& pl, const Sf2Args& a) {
  switch (a.nreal * 2 + a.phi) {
    case 2: sf2_launch_fields<1, 0>(s, nblk, r, pl, a); break;
    case 4: sf2_launch_fields<2, 0>(s, nblk, r, pl, a); break;
    case 6: sf2_launch_fields<3, 0>(s, nblk, r, pl, a); break;
    case 1: sf2_launch_fields<0, 1>(s, nblk, r, pl, a); break;
    case 3: sf2_launch_fields<1, 1>(s, nblk, r, pl, a); break;
    default: sf2_launch_fields<2, 1>(s, nblk, r, pl, a);
  }
}
static int hist_plane_grid(size_t n) { return (int)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024); }

// 1 read + 1 write stream copy, 16 B per lane: the rate a copy kernel reaches on THIS device, the second denominator of
// bench.py's roofline fractions.  Three shapes are timed and the best is reported (tools/copy_shape_bench.hip
// swept them, 4.4-6.5 TB/s): plain grid-stride; grid-stride with U loads then U stores in flight, non-temporal both ways (what
// MI355X_MICROARCH.md's 6.29 TB/s float4 copy is); the same at twice the depth.  Buffers live only for the call.
template <int U, bool NT>
__global__ void __launch_bounds__(256) k_stream_copy(const double2* __restrict__ src, double2* __restrict__ dst, size_t n) {
  const size_t step = (size_t)gridDim.x * blockDim.x;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + (U - 1) * step < n; i += U * step) {
    double2 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (NT) {
        v[u].x = __builtin_nontemporal_load(&src[i + u * step].x);
        v[u].y = __builtin_nontemporal_load(&src[i + u * step].y);
      } else {
        v[u] = src[i + u * step];
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (NT) {
        __builtin_nontemporal_store(v[u].x, &dst[i + u * step].x);
        __builtin_nontemporal_store(v[u].y, &dst[i + u * step].y);
      } else {
        dst[i + u * step] = v[u];
      }
    }
  }
  for (; i < n; i += step) dst[i] = src[i];
}
#include "nq_coarse.hpp"                   // the kernels of nq_coarse_flux (section 5o); after the shell rule above
static_assert(CG_KE == NQ_CG_KE && CG_ENS == NQ_CG_ENS && CG_NIW == NQ_CG_NIW, "map bits of nq_coarse_flux");
#include "nq_s2s.hpp"                      // the kernels of nq_shell_transfer (section 5p)
static_assert(S2S_Q == NQ_S2S_Q && S2S_ADV == NQ_S2S_ADV && S2S_REF == NQ_S2S_REF, "row bits of nq_shell_transfer");
template <int MODE>
static void launch_x_band(nq_ctx* c, const BandRows& r) {
  const int nblocks = xdiag_blocks(c);
  with_row_size(c->N, [&](auto n) {
    constexpr int NN = decltype(n)::value;
    if constexpr (NN < 8192) {                         // refused by nq_shell_transfer: that row plan spills
      typedef XPlan<NN> X;
      hipLaunchKernelGGL((k_x_band<NN, MODE>), dim3(nblocks), dim3(X::THREADS), X::LDS_BYTES, c->stream, r, c->twx, c->kk);
    }
  });
}

#include "nq_cospec.hpp"                   // the kernels of nq_cospectra (section 5q)
static_assert(COSPEC_FIELDS == NQ_COSPEC_MAX_FIELDS && COSPEC_ROWS == NQ_COSPEC_ROWS, "rows of nq_cospectra");
template <int MODE, bool FLOW>
static void launch_x_cross(nq_ctx* c, const FlowSel& sel, const double* scl, const MArr& oAB, const MArr& oC) {
  const int nblocks = xdiag_blocks(c);
  with_row_size(c->N, [&](auto n) {
    constexpr int NN = decltype(n)::value;
    if constexpr (!FLOW || flow_nv<NN>() == COSPEC_FIELDS) {      // refused by nq_cospectra: one value per thread
      typedef XPlan<NN> X;
      hipLaunchKernelGGL((k_x_cross<NN, MODE, false, FLOW>), dim3(nblocks), dim3(X::THREADS), X::LDS_BYTES, c->stream, c->mQ, c->mQw, c->mU,
                         c->mP, c->mPhi, c->mPhiy, c->twx, c->kk, sel, scl, oAB, oC);
    }
  });
}

extern "C" {

const char* nq_last_error(const nq_ctx* ctx) { return ctx ? ctx->err.c_str() : g_last_error.c_str(); }

// ---- slab geometry (shared by nq_group_elems and the constructor) -----------------------------------
struct SlabGeom {
  int N, P, Nloc, Wf, Wl, WhG, Ph;
  bool waves, coupled, bud, passive;
  int npitch[4];                 // row pitch of the four exchange groups
  int off[4][4];                 // column offset of each array inside its group's row
};
static int round8(int x) { return (x + 7) / 8 * 8; }
static SlabGeom slab_geom(const nq_params* p, int P) {
  SlabGeom g;
  g.N = p->nx;
  g.P = P;
  g.Nloc = g.N / P;
  g.Wf = g.N / P;
  g.WhG = g.N / 2 + 1;
  g.Wl = (g.WhG + P - 1) / P;
  g.Ph = (P == 1) ? g.N / 2 + 8 : round8(g.Wl);
  g.waves = p->model != NQ_MODEL_QG;
  g.coupled = p->model == NQ_MODEL_COUPLED;
  g.bud = p->budgets != 0;
  g.passive = p->model == NQ_MODEL_QG && p->passive_scalar != 0;
  const int hs = g.Ph;                          // segment stride of a half-spectrum array inside a row
  memset(g.off, 0, sizeof(g.off));
  // G0: Muq, Mvq, [Mw | Muc, Mvc]
  g.off[0][0] = 0; g.off[0][1] = hs; g.off[0][2] = 2 * hs; g.off[0][3] = 3 * hs;
  g.npitch[0] = 2 * hs + (g.waves ? g.Wf : 0) + (g.passive ? 2 * hs : 0);
  // G1: Mphi, Mphiy
  for (int i = 0; i < 4; ++i) g.off[1][i] = i * g.Wf;
  g.npitch[1] = g.waves ? 2 * g.Wf : 0;
  // G2: Ma, Mb
  g.off[2][0] = 0; g.off[2][1] = hs;
  g.npitch[2] = g.coupled ? 2 * hs : 0;
  // G3: Mu, Mp, Mq, [Mqw]
  for (int i = 0; i < 4; ++i) g.off[3][i] = i * hs;
  g.npitch[3] = ((g.coupled || g.passive) ? 4 : 3) * hs;
  return g;
}

long long nq_group_elems(const nq_params* p, int nranks, int group) {
  if (!p || group < 0 || group > 4 || nranks < 1 || p->nx % nranks) return -1;
  const SlabGeom g = slab_geom(p, nranks);
  if (group == 4) return (p->model == NQ_MODEL_YBJ && nranks > 1) ? (long long)g.N * g.npitch[1] : 0;
  return (long long)g.N * g.npitch[group];       // one side: P blocks of Nloc rows = N rows of `pitch`
}

static MArr make_marr(const SlabGeom& g, cd* bx, cd* by, int group, int idx, bool half) {
  MArr m;
  m.xs = bx ? bx + g.off[group][idx] : nullptr;
  m.ys = by ? by + g.off[group][idx] : nullptr;
  m.pitch = g.npitch[group];
  m.W = half ? (g.P == 1 ? g.WhG : g.Wl) : g.Wf;
  m.blk = (long long)g.Nloc * g.npitch[group];
  m.shift = -1;
  m.magic = 0;
  if (g.P == 1) m.shift = 30;                    // a single block: kx / W == 0
  else if ((m.W & (m.W - 1)) == 0) {
    int sh = 0;
    while ((1 << sh) < m.W) ++sh;
    m.shift = sh;
  } else {
    m.magic = (unsigned)(((1u << 24) + m.W - 1) / m.W);
  }
  return m;
}

static int create_impl(const nq_params* p_in, const double* kk, const double* ll, const double* filtr,
                       const double* contour, int device, int P, int rank, void* const* ext, void* ext_stream,
                       nq_ctx** out) {
  if (!p_in || !kk || !ll || !filtr || !contour || !out) NQ_FAIL((nq_ctx*)nullptr, -1, "nq_create: null argument");
  // YBJModel = UnCoupled layouts and kernels with its own stage graph; its step accumulates no budgets
  nq_params pp = *p_in;
  const bool ybj = pp.model == NQ_MODEL_YBJ;
  if (ybj) {
    pp.model = NQ_MODEL_UNCOUPLED;
    pp.budgets = 0;
  }
  const nq_params* p = &pp;
  int S1, S2;
  if (!plan_for(p->nx, &S1, &S2)) NQ_FAIL((nq_ctx*)nullptr, -2, "nq_create: nx=%d unsupported (power of two in [64, 8192])", p->nx);
  if (const char* e = getenv("NIWQG_AMD_Y_SPLIT")) {       // "S1,S2": another split of the two-pass y transform (measurements)
    int a = 0, b = 0;
    if (sscanf(e, "%d,%d", &a, &b) == 2 && a * b == p->nx && (a == 8 || a == 16 || a == 32 || a == 64) &&
        (b == 8 || b == 16 || b == 32 || b == 64 || b == 128)) {
      S1 = a;
      S2 = b;
    } else {
      NQ_FAIL((nq_ctx*)nullptr, -2, "NIWQG_AMD_Y_SPLIT=%s: S1 in {8,16,32,64}, S2 in {8..128}, S1*S2 = nx", e);
    }
  }
  if (p->model < 0 || p->model > 2) NQ_FAIL((nq_ctx*)nullptr, -2, "nq_create: unknown model %d", p->model);
  if (P < 1 || rank < 0 || rank >= P || (P & (P - 1)) || p->nx / P < CL)
    NQ_FAIL((nq_ctx*)nullptr, -2, "nq_create: %d ranks unsupported for nx=%d (power of two, at least %d columns per rank)", P, p->nx, CL);
  if (P > 1) {
    // the row kernels find the block of a half-spectrum column with kx / Wl = (kx * ceil(2^24 / Wl)) >> 24 (MArr::magic, Wl is not
    // a power of two): checked here for every column this grid has, not trusted (exact while kx * Wl < 2^24)
    const int whg = p->nx / 2 + 1, wl = (whg + P - 1) / P;
    if (wl & (wl - 1)) {
      const unsigned magic = (unsigned)(((1u << 24) + wl - 1) / wl);
      for (int kx = 0; kx < whg; ++kx)
        if ((int)(((unsigned)kx * magic) >> 24) != kx / wl)
          NQ_FAIL((nq_ctx*)nullptr, -2, "nq_create: %d ranks unsupported for nx=%d (block index of column %d)", P, p->nx, kx);
    }
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) NQ_FAIL((nq_ctx*)nullptr, -3, "nq_create: no HIP device available");
  if (device < 0 || device >= ndev) NQ_FAIL((nq_ctx*)nullptr, -3, "nq_create: device %d out of range (%d devices)", device, ndev);
  nq_ctx* c = new nq_ctx();
  const SlabGeom sg = slab_geom(p, P);
  c->p = *p;
  c->ybj = ybj;
  c->passive = sg.passive;
  c->N = p->nx;
  c->S1 = S1;
  c->S2 = S2;
  c->CLy = CL;
  {
    // Small grids on one rank: SINGLE-PASS columns (a tile of whole columns per workgroup, no A sub-pass).  A step of these
    // grids is a chain of dependent 5-microsecond kernels: what counts is how many there are.  NIWQG_AMD_SINGLE_PASS=0 keeps
    // the two-pass tiles (A/B measurements; slab contexts always use them).
    const char* e = getenv("NIWQG_AMD_SINGLE_PASS");
    if (P == 1 && p->nx <= 512 && !(e && atoi(e) == 0)) {
      if (getenv("NIWQG_AMD_Y_SPLIT")) {          // the knob would be silently overridden here: refuse instead
        delete c;
        NQ_FAIL((nq_ctx*)nullptr, -2, "NIWQG_AMD_Y_SPLIT has no effect on a single-rank grid <= 512 (single-pass columns); set NIWQG_AMD_SINGLE_PASS=0 with it");
      }
      c->S1 = p->nx;
      c->S2 = 1;
      c->CLy = p->nx >= 128 ? CLS : CL;
      // QGModel without its passive scalar: k_s_q + k_s_invert of a stage as ONE array-parallel kernel (k_c_qg); one wave per
      // array and column tile (NIWQG_AMD_SMALL_QG=0: the separate kernels)
      const char* e2 = getenv("NIWQG_AMD_SMALL_QG");
      if (p->model == NQ_MODEL_QG && !p->passive_scalar && p->nx >= 128 && !(e2 && atoi(e2) == 0))
        c->small_qg = p->nx == 128 ? 4 : 2;
    }
  }
  c->P = P;
  c->rank = rank;
  c->Nloc = sg.Nloc;
  c->row0 = 0;
  c->nrows = sg.Nloc;
  c->Wf = sg.Wf;
  c->kf0 = rank * sg.Wf;
  c->Wl = (P == 1) ? sg.WhG : sg.Wl;
  c->kh0 = (P == 1) ? 0 : rank * sg.Wl;
  c->WhG = sg.WhG;
  {
    const int left = sg.WhG - c->kh0;
    c->Wh = left < 0 ? 0 : (left < c->Wl ? left : c->Wl);      // valid local half-spectrum columns
  }
  c->Ph = sg.Ph;
  c->kernel_family = p->model != NQ_MODEL_QG;
  c->nk = c->kernel_family ? c->N : c->WhG;
  c->device = device;
  const int N = c->N;
  const size_t full = (size_t)N * c->Wf, half = (size_t)N * c->Ph;     // local spectral planes
#define FAILC(rc)        \
  do {                   \
    g_last_error = c->err; \
    nq_destroy(c);       \
    return (rc);         \
  } while (0)
#define TRY(call)              \
  do {                         \
    int rc__ = (call);         \
    if (rc__) FAILC(rc__);     \
  } while (0)
  auto setup = [&]() -> int {
    HIPCHK(c, hipSetDevice(device));
    {
      int ncu = 0;
      if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && ncu > 0) c->num_cu = ncu;
    }
    if (const char* e = getenv("NIWQG_AMD_NUM_CU")) {      // the CU count the row grids are sized by (tests: grids that do not divide their rows)
      char* end = nullptr;
      const long v = strtol(e, &end, 10);
      if (end == e || *end || v < 1 || v > c->num_cu)
        NQ_FAIL(c, -2, "NIWQG_AMD_NUM_CU=%s: an integer in 1..%d (the CUs of the device); it sizes grids, it masks nothing", e, c->num_cu);
      c->num_cu = (int)v;
    }
    if (ext_stream) {
      c->stream = reinterpret_cast<hipStream_t>(ext_stream);
      c->own_stream = false;
    } else {
      HIPCHK(c, hipStreamCreate(&c->stream));
    }
    HIPCHK(c, hipEventCreate(&c->ev0));
    HIPCHK(c, hipEventCreate(&c->ev1));
    // twiddles, long-double accurate
    std::vector<double> twh(2 * (size_t)N);
    for (int m = 0; m < N; ++m) {
      const long double a = -2.0L * 3.14159265358979323846264338327950288L * (long double)m / (long double)N;
      twh[2 * m] = (double)cosl(a);
      twh[2 * m + 1] = (double)sinl(a);
    }
    ALLOC(c, c->tw, (size_t)N);
    HIPCHK(c, hipMemcpyAsync(c->tw, twh.data(), sizeof(double) * 2 * N, hipMemcpyHostToDevice, c->stream));
    // stage tables for the fused row kernels: [stage >= 1][w^1 | w^4 | w^8][jr < NS]
    for (int which = 0; which < 2; ++which) {
      const int PP = which == 0 ? XPlan<8>::pts(N) : XPlan1<8>::pts(N);
      std::vector<double> st;
      for (int sidx = 1; sidx < plan_stages(N, PP); ++sidx) {
        const int R = plan_radix(N, PP, sidx), NS = plan_ns(N, PP, sidx);
        for (int pw = 1; pw <= 8; pw *= (pw == 1 ? 4 : 2)) {          // powers 1, 4, 8 as far as the radix needs
          if ((pw == 4 && plan_tw_rows(N, PP, R) < 2) || (pw == 8 && plan_tw_rows(N, PP, R) < 3)) continue;
          for (int jr = 0; jr < NS; ++jr) {
            const long long m = ((long long)pw * jr * (N / (NS * R))) % N;
            st.push_back(twh[2 * m]);
            st.push_back(twh[2 * m + 1]);
          }
        }
      }
      cd*& dst = which == 0 ? c->twx : c->twx1;
      ALLOC(c, dst, st.size() / 2 + 1);
      HIPCHK(c, hipMemcpyAsync(dst, st.data(), sizeof(double) * st.size(), hipMemcpyHostToDevice, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    if (N == 8192) {
      // k_x_products_eo: stage table of the 4096-point plan (its own twiddles: exp(-2 pi i m / 4096) = twh[2m])
      const int Mh = N / 2, PP = XPlan<8>::pts(Mh);
      std::vector<double> st;
      for (int sidx = 1; sidx < plan_stages(Mh, PP); ++sidx) {
        const int R = plan_radix(Mh, PP, sidx), NS = plan_ns(Mh, PP, sidx);
        for (int pw = 1; pw <= 8; pw *= (pw == 1 ? 4 : 2)) {
          if ((pw == 4 && plan_tw_rows(Mh, PP, R) < 2) || (pw == 8 && plan_tw_rows(Mh, PP, R) < 3)) continue;
          for (int jr = 0; jr < NS; ++jr) {
            const long long m = ((long long)pw * jr * (Mh / (NS * R))) % Mh;
            st.push_back(twh[2 * (2 * m)]);
            st.push_back(twh[2 * (2 * m) + 1]);
          }
        }
      }
      ALLOC(c, c->twx_half, st.size() / 2 + 1);
      HIPCHK(c, hipMemcpyAsync(c->twx_half, st.data(), sizeof(double) * st.size(), hipMemcpyHostToDevice, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    ALLOC(c, c->kk, (size_t)N);
    ALLOC(c, c->ll, (size_t)N);
    HIPCHK(c, hipMemcpyAsync(c->kk, kk, sizeof(double) * c->nk, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->ll, ll, sizeof(double) * N, hipMemcpyHostToDevice, c->stream));
    ALLOC(c, c->contour, (size_t)32);
    HIPCHK(c, hipMemcpyAsync(c->contour, contour, sizeof(double) * 64, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // filter planes, local columns: half-spectrum copy (pitch Ph) and, for the Kernel family, full-width copy
    ALLOC(c, c->filt_h, half);
    if (c->Wh > 0)
      HIPCHK(c, hipMemcpy2DAsync(c->filt_h, sizeof(double) * c->Ph, filtr + c->kh0, sizeof(double) * c->nk, sizeof(double) * c->Wh, N, hipMemcpyHostToDevice, c->stream));
    if (c->kernel_family) {
      ALLOC(c, c->filt_f, full);
      HIPCHK(c, hipMemcpy2DAsync(c->filt_f, sizeof(double) * c->Wf, filtr + c->kf0, sizeof(double) * c->nk, sizeof(double) * c->Wf, N, hipMemcpyHostToDevice, c->stream));
    }
    {
      // is the filter mirror-symmetric in l on this rank's columns?  (the exponential filter and "none" are; the 2/3 mask is not)
      const char* e = getenv("NIWQG_AMD_COEF_MIRROR");
      bool sym = !(e && atoi(e) == 0) && N >= 4;
      for (int l = 1; sym && l < N / 2; ++l)
        for (int k = 0; k < c->nk; ++k)
          if (filtr[(size_t)l * c->nk + k] != filtr[(size_t)(N - l) * c->nk + k]) { sym = false; break; }
      c->cmirror = sym ? 1 : 0;
      c->crows = sym ? N / 2 + 1 : N;
    }
    const size_t half_c = (size_t)c->crows * c->Ph, full_c = (size_t)c->crows * c->Wf;
    // equations
    for (int i = 0; i < 3; ++i) ALLOC(c, c->q.y[i], half);
    ALLOC(c, c->q.fn0, half);
    ALLOC(c, c->q.fna, half);
    for (int i = 0; i < 6; ++i) ALLOC(c, c->q.coef[i], half_c);
    dim3 blk(64), grdh((c->Wh + 63) / 64, c->crows), grdf((c->Wf + 63) / 64, c->crows);
    if (c->Wh > 0)
      hipLaunchKernelGGL(k_etdrk4_coeffs, grdh, blk, 0, c->stream, c->kernel_family ? 0 : 2, N, c->Wh, c->Ph, c->kh0, c->p, c->kk, c->ll, c->filt_h, c->contour, c->q.coef[0], c->q.coef[1], c->q.coef[2], c->q.coef[3], c->q.coef[4], c->q.coef[5]);
    if (sg.passive) {
      for (int i = 0; i < 3; ++i) ALLOC(c, c->cq.y[i], half);
      ALLOC(c, c->cq.fn0, half);
      ALLOC(c, c->cq.fna, half);
      for (int i = 0; i < 6; ++i) ALLOC(c, c->cq.coef[i], half_c);
      if (c->Wh > 0)
        hipLaunchKernelGGL(k_etdrk4_coeffs, grdh, blk, 0, c->stream, 3, N, c->Wh, c->Ph, c->kh0, c->p, c->kk, c->ll, c->filt_h, c->contour, c->cq.coef[0], c->cq.coef[1], c->cq.coef[2], c->cq.coef[3], c->cq.coef[4], c->cq.coef[5]);
    }
    c->dual = c->kernel_family && p->dual_q != 0;
    if (c->dual) {
      for (int i = 0; i < 3; ++i) ALLOC(c, c->q2.y[i], half);
      ALLOC(c, c->q2.fn0, half);
      ALLOC(c, c->q2.fna, half);
      for (int i = 0; i < 6; ++i) ALLOC(c, c->coefu[i], half_c);
      if (c->Wh > 0)
        hipLaunchKernelGGL(k_etdrk4_coeffs, grdh, blk, 0, c->stream, 0, N, c->Wh, c->Ph, c->kh0, c->p, c->kk, c->ll, (const double*)nullptr, c->contour, c->coefu[0], c->coefu[1], c->coefu[2], c->coefu[3], c->coefu[4], c->coefu[5]);
      std::vector<double> fm((size_t)N * c->Ph, 0.0);
      for (int l = 0; l < N; ++l)
        for (int k = 0; k < c->Wh; ++k) fm[(size_t)l * c->Ph + k] = filtr[(size_t)((N - l) % N) * c->nk + (N - (c->kh0 + k)) % N];
      ALLOC(c, c->filt_m, half);
      HIPCHK(c, hipMemcpyAsync(c->filt_m, fm.data(), sizeof(double) * half, hipMemcpyHostToDevice, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    c->pass = c->kernel_family && !c->dual && !ybj;
    if (c->pass) {
      for (int i = 0; i < 3; ++i) ALLOC(c, c->qp.y[i], (size_t)c->Ph);
      ALLOC(c, c->qp.fn0, (size_t)c->Ph);
      ALLOC(c, c->qp.fna, (size_t)c->Ph);
      for (int i = 0; i < 6; ++i) c->qp.coef[i] = c->q.coef[i] + (size_t)(N / 2) * c->Ph;     // row N/2 of the q planes
    }
    ALLOC(c, c->ph, half);
    ALLOC(c, c->qwh, half);
    if (P == 1) {                                   // scratch of the generic (single-rank) transform paths
      ALLOC(c, c->scr_h0, half);
      ALLOC(c, c->scr_h1, half);
      ALLOC(c, c->scr_r, (size_t)N * N);
      ALLOC(c, c->scr_f0, (size_t)N * N);
      ALLOC(c, c->scr_f1, (size_t)N * N);
    } else {
      ALLOC(c, c->scr_h0, (size_t)64);              // reduction scratch only
    }
    if (c->kernel_family) {
      {
        const char* e = getenv("NIWQG_AMD_PHI_STAGE_STORE");
        c->phi_stage_store = (e && atoi(e) != 0) ? 1 : 0;
      }
      // slot (cur+1)%3 held the stage-0 result of phi-hat: nothing but k_s_phi's stored data flow touches it (cur never moves)
      for (int i = 0; i < 3; ++i)
        if (i != 1 || c->phi_stage_store) ALLOC(c, c->w.y[i], full);
      ALLOC(c, c->w.fn0, full);
      ALLOC(c, c->w.fna, full);
      for (int i = 0; i < 6; ++i) ALLOC(c, c->w.coef[i], full_c);
      hipLaunchKernelGGL(k_etdrk4_coeffs, grdf, blk, 0, c->stream, 1, N, c->Wf, c->Wf, c->kf0, c->p, c->kk, c->ll, c->filt_f, c->contour, c->w.coef[0], c->w.coef[1], c->w.coef[2], c->w.coef[3], c->w.coef[4], c->w.coef[5]);
    }
    c->bud = p->budgets != 0;
    // exchange groups: one buffer per side (the same buffer when P == 1); external (torch) buffers when given
    for (int gi = 0; gi < 4; ++gi) {
      c->G[gi].pitch = sg.npitch[gi];
      c->G[gi].elems = (size_t)N * sg.npitch[gi];
      if (c->G[gi].elems == 0) continue;
      if (ext && ext[2 * gi] && ext[2 * gi + 1]) {
        c->G[gi].bx = reinterpret_cast<cd*>(ext[2 * gi]);
        c->G[gi].by = reinterpret_cast<cd*>(ext[2 * gi + 1]);
        HIPCHK(c, hipMemsetAsync(c->G[gi].bx, 0, c->G[gi].elems * sizeof(cd), c->stream));
        HIPCHK(c, hipMemsetAsync(c->G[gi].by, 0, c->G[gi].elems * sizeof(cd), c->stream));
      } else {
        c->alloc_plain = true;
        ALLOC(c, c->G[gi].bx, c->G[gi].elems);
        if (P == 1) c->G[gi].by = c->G[gi].bx;
        else ALLOC(c, c->G[gi].by, c->G[gi].elems);
        c->alloc_plain = false;
      }
    }
    c->mUq = make_marr(sg, c->G[0].bx, c->G[0].by, 0, 0, true);
    c->mVq = make_marr(sg, c->G[0].bx, c->G[0].by, 0, 1, true);
    c->mW = make_marr(sg, c->G[0].bx, c->G[0].by, 0, 2, false);
    c->mPhi = make_marr(sg, c->G[1].bx, c->G[1].by, 1, 0, false);
    c->mPhiy = make_marr(sg, c->G[1].bx, c->G[1].by, 1, 1, false);
    c->mA = make_marr(sg, c->G[2].bx, c->G[2].by, 2, 0, true);
    c->mB = make_marr(sg, c->G[2].bx, c->G[2].by, 2, 1, true);
    c->mU = make_marr(sg, c->G[3].bx, c->G[3].by, 3, 0, true);
    c->mP = make_marr(sg, c->G[3].bx, c->G[3].by, 3, 1, true);
    c->mQ = make_marr(sg, c->G[3].bx, c->G[3].by, 3, 2, true);
    c->mQw = make_marr(sg, c->G[3].bx, c->G[3].by, 3, 3, true);
    if (sg.passive) {
      c->mUc = make_marr(sg, c->G[0].bx, c->G[0].by, 0, 2, true);
      c->mVc = make_marr(sg, c->G[0].bx, c->G[0].by, 0, 3, true);
    }
    if (P == 1 && p->model == NQ_MODEL_COUPLED && !c->dual && (N == 4096 || N == 8192)) {
      // NIWQG_AMD_OVERLAP_CUS: unset = the measured default (4096^2 only), 0 = the serial step,
      // n > 0 = leave about n CUs to the q branch (the wave-PV grid is nq_overlap_grid of the rest, which may free a few more)
      const char* e = getenv("NIWQG_AMD_OVERLAP_CUS");
      const int want = e ? atoi(e) : nq_overlap_default_cus(N);
      if (want > 0 && want < c->num_cu) {
        const int nb = N == 4096 ? N / XPlan<4096>::C : N;
        c->overlap_grid = nq_overlap_grid(nb, c->num_cu - want);
        c->overlap_cus = c->num_cu - c->overlap_grid;
        HIPCHK(c, hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
      }
    }
    c->mGx = c->mPhi;
    c->mGy = c->mPhiy;
    if (c->p.model == NQ_MODEL_UNCOUPLED) {        // frozen copy of the X side of G1 (quirk Q1)
      ALLOC(c, c->Gs, c->G[1].elems);
      cd* gsy = c->Gs;
      if (ybj && P > 1) {                          // its stage results cross y -> x in a group of their own
        ALLOC(c, c->Gs_y, c->G[1].elems);
        gsy = c->Gs_y;
        c->G[4].bx = c->Gs;
        c->G[4].by = c->Gs_y;
        c->G[4].pitch = c->G[1].pitch;
        c->G[4].elems = c->G[1].elems;
      }
      c->mGx = make_marr(sg, c->Gs, gsy, 1, 0, false);
      c->mGy = make_marr(sg, c->Gs, gsy, 1, 1, false);
    }
    if (c->bud) {
      c->nww = (c->Wf / c->CLy) * c->S2;
      c->nwq = ((c->Wh + c->CLy - 1) / c->CLy) * c->S2;
      if (c->small_qg && (c->Wh + c->small_qg - 1) / c->small_qg > c->nwq) c->nwq = (c->Wh + c->small_qg - 1) / c->small_qg;
      if (c->nwq < 1) c->nwq = 1;
      ALLOC(c, c->partQ, (size_t)4 * c->nwq * (sg.passive ? 6 : 3));
      ALLOC(c, c->part0Q, (size_t)c->nwq * (sg.passive ? 6 : 3));
      ALLOC(c, c->acc, (size_t)4);
      // everything that has to be summed over ranks lives in one 64-double block (external when the caller
      // does the all-reduce): [0,44) stage sums of a step, [44,48) carried phi sums, [48,51) carried q sums,
      // [51] frozen gradient sum
      if (ext && ext[8]) {
        c->bsums = reinterpret_cast<double*>(ext[8]);
        HIPCHK(c, hipMemsetAsync(c->bsums, 0, 64 * sizeof(double), c->stream));
      } else {
        ALLOC(c, c->bsums, (size_t)64);
      }
      c->carryW = c->bsums + 44;
      c->carryQ = c->bsums + 48;
      c->gradS1 = c->bsums + 51;
      if (c->kernel_family) {
        ALLOC(c, c->partW, (size_t)4 * c->nww * NQ_PARTW + 2);       // + BudgetW.w00
        ALLOC(c, c->part0W, (size_t)c->nww * NQ_PARTW);
      }
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return 0;
  };
  TRY(setup());
  *out = c;
  return 0;
}

int nq_create(const nq_params* p, const double* kk, const double* ll, const double* filtr, const double* contour,
              int device, nq_ctx** out) {
  return create_impl(p, kk, ll, filtr, contour, device, 1, 0, nullptr, nullptr, out);
}

int nq_create_slab(const nq_params* p, const double* kk, const double* ll, const double* filtr, const double* contour,
                   int device, int nranks, int rank, void* const* buffers, void* stream, nq_ctx** out) {
  return create_impl(p, kk, ll, filtr, contour, device, nranks, rank, buffers, stream, out);
}

int nq_destroy(nq_ctx* c) {
  if (!c) return 0;
  hipSetDevice(c->device);
  if (c->stream) hipStreamSynchronize(c->stream);
  att_release(c, c->pt);
  att_release(c, c->fc);
  att_release(c, c->fq);
  att_release(c, c->av);
  att_release(c, c->ts);
  for (void* p : c->allocs) hipFree(p);
  for (auto& pt : c->patch) { (void)hipFree(pt.l); (void)hipFree(pt.k); (void)hipFree(pt.v); }
  for (hipEvent_t e : c->prof_ev) hipEventDestroy(e);
  for (hipEvent_t e : c->marks)
    if (e) hipEventDestroy(e);
  if (c->ev0) hipEventDestroy(c->ev0);
  if (c->ev1) hipEventDestroy(c->ev1);
  if (c->snap_stream) {
    hipStreamSynchronize(c->snap_stream);
    hipStreamDestroy(c->snap_stream);
  }
  if (c->ev_snap) hipEventDestroy(c->ev_snap);
  if (c->snap_hq) hipHostFree(c->snap_hq);
  if (c->snap_hphi) hipHostFree(c->snap_hphi);
  if (c->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(c->comm);
  if (c->mstream) hipStreamSynchronize(c->mstream);
  for (hipEvent_t e : c->ev_prod)
    if (e) hipEventDestroy(e);
  for (auto& row : c->ev_arr)
    for (hipEvent_t e : row)
      if (e) hipEventDestroy(e);
  for (hipEvent_t e : {c->ev_col, c->ev_done, c->ev_red})
    if (e) hipEventDestroy(e);
  for (hipEvent_t e : c->xev) hipEventDestroy(e);
  if (c->mstream) hipStreamDestroy(c->mstream);
  if (c->stream2) {
    hipStreamSynchronize(c->stream2);
    hipStreamDestroy(c->stream2);
  }
  if (c->ev_fork) hipEventDestroy(c->ev_fork);
  if (c->ev_join) hipEventDestroy(c->ev_join);
  if (c->stream && c->own_stream) hipStreamDestroy(c->stream);
  delete c;
  return 0;
}

void* nq_stream(nq_ctx* c) { return c ? (void*)c->stream : nullptr; }
long long nq_device_bytes(const nq_ctx* c) { return c ? c->bytes : 0; }

int nq_sync(nq_ctx* c) {
  if (!c) return -1;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  // ... and the exchange stream: the last y -> x group of a slab step is only waited for by the NEXT row kernel, so the
  // library's communicator can still have sends / receives queued when the compute stream is idle.  A caller that syncs
  // and then runs a collective of its own (torch.distributed) must never find two communicators active on the device.
  if (c->mstream) HIPCHK(c, hipStreamSynchronize(c->mstream));
  HIPCHK(c, hipGetLastError());
  return 0;
}

int nq_stream_copy_gbs(nq_ctx* c, long long bytes, int reps, double* gbs_out) {
  if (!c || !gbs_out || bytes < (1 << 20) || reps < 1) return -1;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = (size_t)bytes / sizeof(double2);
  double2 *a = nullptr, *b = nullptr;
  HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&a), n * sizeof(double2)));
  if (hipMalloc(reinterpret_cast<void**>(&b), n * sizeof(double2)) != hipSuccess) {
    (void)hipFree(a);
    NQ_FAIL(c, -5, "nq_stream_copy_gbs: out of device memory");
  }
  (void)hipMemsetAsync(a, 1, n * sizeof(double2), c->stream);
  (void)hipMemsetAsync(b, 0, n * sizeof(double2), c->stream);
  auto launch = [&](int shape) {
    const double2* src = a;
    switch (shape) {
      case 0: hipLaunchKernelGGL((k_stream_copy<1, false>), dim3(c->num_cu * 8), dim3(256), 0, c->stream, src, b, n); break;
      case 1: hipLaunchKernelGGL((k_stream_copy<4, true>), dim3(c->num_cu * 8), dim3(256), 0, c->stream, src, b, n); break;
      case 2: hipLaunchKernelGGL((k_stream_copy<4, true>), dim3(c->num_cu * 16), dim3(256), 0, c->stream, src, b, n); break;
      default: hipLaunchKernelGGL((k_stream_copy<8, true>), dim3(c->num_cu * 8), dim3(256), 0, c->stream, src, b, n); break;
    }
  };
  launch(0);                                                                                            // untimed warm-up
  double best = 0.0;
  int rc = 0;
  for (int shape = 0; shape < 4 && rc == 0; ++shape)
    for (int r = 0; r < reps && rc == 0; ++r) {
      if (hipEventRecord(c->ev0, c->stream) != hipSuccess) { rc = -5; break; }
      launch(shape);
      float ms = 0.f;
      if (hipEventRecord(c->ev1, c->stream) != hipSuccess || hipEventSynchronize(c->ev1) != hipSuccess ||
          hipEventElapsedTime(&ms, c->ev0, c->ev1) != hipSuccess) { rc = -5; break; }
      const double g = 2.0 * (double)(n * sizeof(double2)) / (ms * 1e-3) / 1e9;
      best = g > best ? g : best;
    }
  (void)hipStreamSynchronize(c->stream);
  (void)hipFree(a);
  (void)hipFree(b);
  if (rc) NQ_FAIL(c, rc, "nq_stream_copy_gbs: event timing failed");
  *gbs_out = best;
  return 0;
}

int nq_profile_enable(nq_ctx* c, int kernel_class) {
  if (!c) return -1;
  c->prof_class = kernel_class;
  c->prof_used = 0;
  c->prof_seen = 0;
  return 0;
}
// Bracket only every stride-th launch of the enabled class(es): an event pair costs the stream about 9 microseconds, 2 % of a
// 4096^2 step when all 20 A sub-passes of a step are bracketed and 10 % of a rank's step on eight slab ranks.  A stride coprime
// with the launch pattern of a step (5 A sub-passes per stage, 20 per step: 7) samples every position equally often.
int nq_profile_stride(nq_ctx* c, int stride) {
  if (!c || stride < 1) return -1;
  c->prof_stride = stride;
  c->prof_seen = 0;
  return 0;
}
int nq_profile_read(nq_ctx* c, int* launches, float* total_ms) {
  if (!c || !launches || !total_ms) return -1;
  int rc = nq_sync(c);
  if (rc) return rc;
  float tot = 0.f;
  for (size_t i = 0; i + 1 < c->prof_used; i += 2) {
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->prof_ev[i], c->prof_ev[i + 1]));
    tot += ms;
  }
  *launches = (int)(c->prof_used / 2);
  *total_ms = tot;
  c->prof_used = 0;
  return 0;
}

int nq_profile_read_all(nq_ctx* c, int* launches6, float* total_ms6) {
  if (!c || !launches6 || !total_ms6) return -1;
  int rc = nq_sync(c);
  if (rc) return rc;
  for (int k = 0; k < 6; ++k) {
    launches6[k] = 0;
    total_ms6[k] = 0.f;
  }
  for (size_t i = 0; i + 1 < c->prof_used; i += 2) {
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->prof_ev[i], c->prof_ev[i + 1]));
    const int k = c->prof_cls[i / 2];
    if (k >= 0 && k < 6) {
      launches6[k] += 1;
      total_ms6[k] += ms;
    }
  }
  c->prof_used = 0;
  return 0;
}

int nq_timer_start(nq_ctx* c) {
  if (!c) return -1;
  HIPCHK(c, hipEventRecord(c->ev0, c->stream));
  return 0;
}
int nq_timer_stop(nq_ctx* c, float* ms) {
  if (!c || !ms) return -1;
  HIPCHK(c, hipEventRecord(c->ev1, c->stream));
  HIPCHK(c, hipEventSynchronize(c->ev1));
  HIPCHK(c, hipEventElapsedTime(ms, c->ev0, c->ev1));
  return 0;
}

int nq_event_record(nq_ctx* c, int slot) {
  if (!c) return -1;
  if (slot < 0 || slot >= 16) NQ_FAIL(c, -1, "nq_event_record: slot %d (0..15)", slot);
  HIPCHK(c, hipSetDevice(c->device));
  if (!c->marks[slot]) HIPCHK(c, hipEventCreate(&c->marks[slot]));
  HIPCHK(c, hipEventRecord(c->marks[slot], c->stream));
  return 0;
}
int nq_event_elapsed(nq_ctx* c, int slot_a, int slot_b, float* ms) {
  if (!c || !ms) return -1;
  if (slot_a < 0 || slot_a >= 16 || slot_b < 0 || slot_b >= 16 || !c->marks[slot_a] || !c->marks[slot_b])
    NQ_FAIL(c, -1, "nq_event_elapsed: slots %d, %d not recorded", slot_a, slot_b);
  HIPCHK(c, hipEventSynchronize(c->marks[slot_b]));
  HIPCHK(c, hipEventElapsedTime(ms, c->marks[slot_a], c->marks[slot_b]));
  return 0;
}

int nq_set_q(nq_ctx* c, const double* q_host) {
  if (!c || !q_host) return -1;
  NQ_SINGLE_RANK(c, "nq_set_q");
  pt_mark_stale(c);
  const size_t full = (size_t)c->N * c->N;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(c->scr_r, q_host, sizeof(double) * full, hipMemcpyHostToDevice, c->stream));
  fwd2d_half(c, c->scr_r, c->q.y[c->q.cur], c->scr_h0);
  if (c->dual) HIPCHK(c, hipMemcpyAsync(c->q2.y[c->q2.cur], c->q.y[c->q.cur], sizeof(cd) * (size_t)c->N * c->Ph, hipMemcpyDeviceToDevice, c->stream));
  { int rc = reset_passenger(c); if (rc) return rc; }
  do_invert_now(c);
  c->have_q = true;
  return nq_sync(c);
}

int nq_set_c(nq_ctx* c, const double* c_host) {
  if (!c || !c_host) return -1;
  NQ_SINGLE_RANK(c, "nq_set_c");
  pt_mark_stale(c);
  if (!c->passive) NQ_FAIL(c, -4, "nq_set_c: this context has no passive scalar");
  const size_t full = (size_t)c->N * c->N;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(c->scr_r, c_host, sizeof(double) * full, hipMemcpyHostToDevice, c->stream));
  fwd2d_half(c, c->scr_r, c->cq.y[c->cq.cur], c->scr_h0);
  do_invert_now(c);                 // re-emits u, psi, q and the scalar's mixed-space rows
  return nq_sync(c);
}

int nq_set_phi(nq_ctx* c, const double* phi_host) {
  if (!c || !phi_host) return -1;
  NQ_SINGLE_RANK(c, "nq_set_phi");
  pt_mark_stale(c);
  if (!c->kernel_family) NQ_FAIL(c, -4, "nq_set_phi: QGModel has no wave field");
  const size_t full = (size_t)c->N * c->N;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(c->scr_f0, phi_host, sizeof(cd) * full, hipMemcpyHostToDevice, c->stream));
  fwd2d_full(c, c->scr_f0, c->w.y[c->w.cur], c->scr_f1);
  launch_emit_phi(c, c->w.y[c->w.cur]);
  launch_A_m(c, true, {&c->mPhi, &c->mPhiy});
  if (c->bud) hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(1024), 0, c->stream, c->part0W, c->nww, NQ_PARTW, 4, c->carryW);
  c->have_phi = true;
  int rc = nq_refresh_grad_phi(c);
  if (rc) return rc;
  return nq_sync(c);
}

int nq_invert(nq_ctx* c) {
  if (!c) return -1;
  NQ_SINGLE_RANK(c, "nq_invert");
  pt_mark_stale(c);
  HIPCHK(c, hipSetDevice(c->device));
  do_invert_now(c);
  return nq_sync(c);
}

int nq_refresh_grad_phi(nq_ctx* c) {
  if (!c) return -1;
  HIPCHK(c, hipSetDevice(c->device));
  if (c->p.model == NQ_MODEL_UNCOUPLED) {
    // freeze the X side of group 1 (phi, phiy rows as the row kernels see them)
    HIPCHK(c, hipMemcpyAsync(c->Gs, c->G[1].bx, sizeof(cd) * c->G[1].elems, hipMemcpyDeviceToDevice, c->stream));
    if (c->bud) HIPCHK(c, hipMemcpyAsync(c->gradS1, c->carryW + 1, sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  }
  return 0;
}

int nq_step(nq_ctx* c, int nsteps) {
  if (!c) return -1;
  NQ_SINGLE_RANK(c, "nq_step");
  if (nsteps < 0) NQ_FAIL(c, -1, "nq_step: nsteps < 0");
  HIPCHK(c, hipSetDevice(c->device));
  for (int i = 0; i < nsteps; ++i) {
    c->uv4_now = c->want_uv4 && i == nsteps - 1 && c->kernel_family && !c->ybj;
    attachments_before_step(c);
    do_step(c);
    const int rc = attachments_after_step(c);
    if (rc) return rc;
  }
  if (nsteps > 0) {
    c->stepped = true;
    c->have_uv4 = c->uv4_now;
    c->want_uv4 = c->uv4_now = false;
  }
  HIPCHK(c, hipGetLastError());
  return 0;
}
// The last step of the NEXT nq_step / nq_slab_step call also records max |u|, max |v| of its fourth stage over this rank's rows
// (two extra row passes in that one step); nq_get_stage4_max reads them (-4 when the last call recorded none).
int nq_request_stage4_max(nq_ctx* c) {
  if (!c) return -1;
  c->want_uv4 = true;
  return 0;
}
int nq_get_stage4_max(nq_ctx* c, double* out2) {
  if (!c || !out2) return -1;
  if (!c->have_uv4 || !c->uv4) NQ_FAIL(c, -4, "nq_get_stage4_max: the last step call was not asked to record the fourth stage's maxima");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(out2, c->uv4, sizeof(double) * 2, hipMemcpyDeviceToHost, c->stream));
  return nq_sync(c);
}

// ---- Lagrangian particles ------------------------------------------------------------------------
// Between calls, Mu and Mp on the x side hold the column-transformed -il psi and psi of the ph the context holds: every step
// ends with the inversion of its final state (store_aux), set_q / set_c / nq_invert run do_invert_now, the QGModel scalar tick
// re-runs do_invert_now after its stale inversion, YBJModel's step writes neither, and a dual-q context inverts the mean of its
// two copies exactly where ph takes it.  So a velocity plane is ONE row kernel (k_x_get_uv) away at any point between steps.
enum { PT_U = 0, PT_V = 1, PT_Q = 2, PT_PHI = 3, PT_UW = NQ_PT_UW, PT_VW = NQ_PT_VW, PT_K = NQ_PT_K, PT_L = NQ_PT_L, PT_ZETA = NQ_PT_ZETA,
       PT_OMEGA = NQ_PT_OMEGA, PT_F11 = NQ_PT_F11, PT_F22 = NQ_PT_F22, PT_LNSIGMA = NQ_PT_LNSIGMA, PT_DET = NQ_PT_DET };
static bool pt_name_of_rays(int name) { return name == PT_K || name == PT_L || name == PT_OMEGA; }   // values only ray mode has
static bool pt_name_of_tangent(int name) { return name >= PT_F11 && name <= PT_DET; }                // values only stretch mode has
static bool pt_name_ok(int name) {
  return (name >= PT_U && name <= PT_PHI) || name == PT_UW || name == PT_VW || name == PT_ZETA || pt_name_of_rays(name) ||
         pt_name_of_tangent(name);
}
static bool pt_name_needs_phi(int name) { return name == PT_PHI || name == PT_UW || name == PT_VW; }
// q_psi comes from the Kernel family's row pass, and ray mode is the Kernel family's
static bool pt_name_needs_waves(int name) { return name == PT_ZETA || pt_name_of_rays(name); }
static PtGrid pt_grid(const nq_ctx* c) {
  PtGrid g;
  g.n = c->N;
  g.Lx = c->pt_L[0];
  g.Ly = c->pt_L[1];
  g.dx = g.Lx / c->N;
  g.dy = g.Ly / c->N;
  return g;
}
static int pt_blocks(int n) { return (n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096; }

// the velocity plane of the current ph from Mu, Mp (one row kernel)
static void pt_form_uv(nq_ctx* c, cd* out) {
  with_row_size(c->N, [&](auto n) {
    constexpr int N = decltype(n)::value;
    typedef XPlan<N> X;
    constexpr bool one = N >= 8192;
    for (int comp = 0; comp < (one ? 2 : 1); ++comp)
      hipLaunchKernelGGL((k_x_get_uv<N, false, one>), rows_grid<X>(c->N), dim3(X::THREADS), X::LDS_BYTES, c->stream, c->mU, c->mP, out, c->N, c->tw, c->kk, c->kernel_family ? 1 : 0, comp);
  });
}
// the physical phi of the current phi-hat from Mphi on the x side (one row pass), as nq_get_field(NQ_F_PHI) forms it
static void pt_form_phi(nq_ctx* c, cd* out) { launch_x_c2c(c, true, c->mPhi.xs, out, c->mPhi.pitch, c->N, 1.0); }
// q_psi of the state the last inversion saw, from Mq (and Mqw on CoupledModel) on the x side: one row kernel (Kernel family)
static void pt_form_zeta(nq_ctx* c, double* out) {
  ProfScope ps(c, PK_PT_ZETA);
  with_row_size(c->N, [&](auto n) {
    constexpr int N = decltype(n)::value;
    typedef XPlan<N> X;
    if (c->p.model == NQ_MODEL_COUPLED)
      hipLaunchKernelGGL((k_x_get_zeta<N, MODE_COUPLED>), dim3(c->Nloc / X::C), dim3(X::THREADS), X::LDS_BYTES, c->stream, c->mQ, c->mQw, c->twx, c->kk, out);
    else
      hipLaunchKernelGGL((k_x_get_zeta<N, MODE_UNCOUPLED>), dim3(c->Nloc / X::C), dim3(X::THREADS), X::LDS_BYTES, c->stream, c->mQ, c->mQw, c->twx, c->kk, out);
  });
}
static void pt_before_step(nq_ctx* c) {
  NqParticles* P = c->pt;
  if (!P->u0) {
    pt_form_uv(c, P->uv[P->cur]);
    P->u0 = true;
  }
  if (P->rays && !P->z0) {
    pt_form_zeta(c, P->zeta[P->cur]);
    P->z0 = true;
  }
  if (P->wave && !P->w0) {
    pt_form_phi(c, P->wphi[P->wcur]);
    P->w0 = true;
  }
}
// e^{-i f0 t} = (c, s), formed on the host in double precision
static void pt_phase(double f0, double t, double* co, double* si) {
  *co = std::cos(f0 * t);
  *si = -std::sin(f0 * t);
}
// the time of step s after attach, counted by the particles: t_s = t0 + s dt (not the accumulated float clock)
static double pt_time(const nq_ctx* c) { return c->pt->wt0 + (double)c->pt->rg.steps * c->p.dt; }
// sample column `name` into o0 (and o1: phi's imaginary part) from the current state; planes allocated on first use
static int pt_sample_into(nq_ctx* c, int name, double* o0, double* o1) {
  NqParticles* P = c->pt;
  const PtGrid g = pt_grid(c);
  const int nb = pt_blocks(P->n);
  if (name == PT_U || name == PT_V) {
    pt_before_step(c);
    hipLaunchKernelGGL(k_pt_sample<cd>, dim3(nb), dim3(256), 0, c->stream, (const cd*)P->uv[P->cur], (const double*)P->x, (const double*)P->y, P->n, g, name == PT_U ? o0 : nullptr, name == PT_V ? o0 : nullptr);
  } else if (name == PT_Q) {
    if (!P->qplane) { int rc = att_alloc(c, P, &P->qplane, (size_t)c->N * c->N, "particles"); if (rc) return rc; }
    // Mq holds the q the last inversion saw (the mean of the two copies on dual-q contexts): m.q
    if (!launch_get_real<false>(c, c->mQ, P->qplane, 0, 0)) NQ_FAIL(c, -2, "no row plan of length %d", c->N);
    hipLaunchKernelGGL(k_pt_sample<double>, dim3(nb), dim3(256), 0, c->stream, (const double*)P->qplane, (const double*)P->x, (const double*)P->y, P->n, g, o0, nullptr);
  } else if (name == PT_PHI) {
    if (!c->kernel_family) NQ_FAIL(c, -4, "particles: QGModel has no wave field (phi)");
    if (!P->phiplane) { int rc = att_alloc(c, P, &P->phiplane, (size_t)c->N * c->N, "particles"); if (rc) return rc; }
    launch_x_c2c(c, true, c->mPhi.xs, P->phiplane, c->mPhi.pitch, c->N, 1.0);         // as nq_get_field(NQ_F_PHI)
    hipLaunchKernelGGL(k_pt_sample<cd>, dim3(nb), dim3(256), 0, c->stream, (const cd*)P->phiplane, (const double*)P->x, (const double*)P->y, P->n, g, o0, o1);
  } else if (name == PT_UW || name == PT_VW) {
    if (!c->kernel_family) NQ_FAIL(c, -4, "particles: QGModel has no wave field (phi)");
    const cd* phi;
    if (P->wave) {                            // drifter mode holds the current phi already
      pt_before_step(c);
      phi = P->wphi[P->wcur];
    } else {
      if (!P->phiplane) { int rc = att_alloc(c, P, &P->phiplane, (size_t)c->N * c->N, "particles"); if (rc) return rc; }
      pt_form_phi(c, P->phiplane);
      phi = P->phiplane;
    }
    double co, si;
    pt_phase(P->wf0, pt_time(c), &co, &si);
    hipLaunchKernelGGL(k_pt_sample_w, dim3(nb), dim3(256), 0, c->stream, phi, (const double*)P->x, (const double*)P->y, P->n, g, P->wa, co, si, name == PT_UW ? o0 : nullptr, name == PT_VW ? o0 : nullptr);
  } else if (name == PT_ZETA) {
    if (!c->kernel_family) NQ_FAIL(c, -4, "particles: zeta is formed by the row pass of the Kernel family");
    const double* z;
    if (P->rays) {                            // ray mode holds the current zeta already
      pt_before_step(c);
      z = P->zeta[P->cur];
    } else {
      if (!P->zplane) { int rc = att_alloc(c, P, &P->zplane, (size_t)c->N * c->N, "particles"); if (rc) return rc; }
      pt_form_zeta(c, P->zplane);
      z = P->zplane;
    }
    hipLaunchKernelGGL(k_pt_sample<double>, dim3(nb), dim3(256), 0, c->stream, z, (const double*)P->x, (const double*)P->y, P->n, g, o0, nullptr);
  } else if (pt_name_of_rays(name)) {
    if (!P->rays) {                           // a column recorded without the mode (nq_particles_sample refuses): NaN, every bit set
      HIPCHK(c, hipMemsetAsync(o0, 0xff, sizeof(double) * (size_t)P->n, c->stream));
    } else if (name == PT_OMEGA) {
      pt_before_step(c);
      hipLaunchKernelGGL(k_pt_omega, dim3(nb), dim3(256), 0, c->stream, (const cd*)P->uv[P->cur], (const double*)P->zeta[P->cur], (const double*)P->x,
                         (const double*)P->y, (const double*)P->k, (const double*)P->l, P->n, g, c->p.U, P->eta, o0);
    } else {
      HIPCHK(c, hipMemcpyAsync(o0, name == PT_K ? P->k : P->l, sizeof(double) * (size_t)P->n, hipMemcpyDeviceToDevice, c->stream));
    }
  } else if (pt_name_of_tangent(name)) {
    if (!P->tan) {                            // a column recorded without the mode (nq_particles_sample refuses): NaN, every bit set
      HIPCHK(c, hipMemsetAsync(o0, 0xff, sizeof(double) * (size_t)P->n, c->stream));
    } else if (name == PT_LNSIGMA || name == PT_DET) {
      hipLaunchKernelGGL(k_pt_tan_value, dim3(nb), dim3(256), 0, c->stream, (const double*)P->f[0], (const double*)P->f[1], (const double*)P->f[2],
                         (const double*)P->f[3], 1, P->n, name == PT_LNSIGMA ? 0 : 1, o0, 1);
    } else {
      HIPCHK(c, hipMemcpyAsync(o0, P->f[name - PT_F11], sizeof(double) * (size_t)P->n, hipMemcpyDeviceToDevice, c->stream));
    }
  } else {
    NQ_FAIL(c, -1, "particles: unknown sample name %d", name);
  }
  HIPCHK(c, hipGetLastError());
  return 0;
}
static int pt_record(nq_ctx* c) {
  NqParticles* P = c->pt;
  const size_t n = (size_t)P->n;
  double* r = P->ring + (size_t)P->rg.slot() * (2 + P->ncol) * n;
  HIPCHK(c, hipMemcpyAsync(r, P->x, sizeof(double) * n, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(r + n, P->y, sizeof(double) * n, hipMemcpyDeviceToDevice, c->stream));
  int col = 2;
  for (int name : P->names) {
    const int rc = pt_sample_into(c, name, r + col * n, name == PT_PHI ? r + (col + 1) * n : nullptr);
    if (rc) return rc;
    col += name == PT_PHI ? 2 : 1;
  }
  P->rg.wrote();
  return 0;
}
static int pt_after_step(nq_ctx* c) {
  NqParticles* P = c->pt;
  const PtGrid g = pt_grid(c);
  const cd* U0 = P->uv[P->cur];
  const cd* U1 = U0;                       // YBJModel: psi is steady, U1 = U0 (formed again only after set_q)
  if (!c->ybj) {
    pt_form_uv(c, P->uv[P->cur ^ 1]);
    U1 = P->uv[P->cur ^ 1];
  }
  if (P->wave) {                           // Phi1 beside U1; the phases at t_s, t_s + dt/2, t_s + dt
    pt_form_phi(c, P->wphi[P->wcur ^ 1]);
    const double t = pt_time(c), dt = c->p.dt;
    PtWave wv;
    wv.a = P->wa;
    pt_phase(P->wf0, t, &wv.c[0], &wv.s[0]);
    pt_phase(P->wf0, t + 0.5 * dt, &wv.c[1], &wv.s[1]);
    pt_phase(P->wf0, t + dt, &wv.c[2], &wv.s[2]);
    if (P->tan) {
      ProfScope ps(c, PK_PT_TANGENT);
      hipLaunchKernelGGL(k_pt_rk4_wt, dim3(pt_blocks(P->n)), dim3(256), 0, c->stream, P->x, P->y, P->f[0], P->f[1], P->f[2], P->f[3], P->n, U0, U1,
                         (const cd*)P->wphi[P->wcur], (const cd*)P->wphi[P->wcur ^ 1], g, c->p.U, dt, wv);
    } else {
      hipLaunchKernelGGL(k_pt_rk4_w, dim3(pt_blocks(P->n)), dim3(256), 0, c->stream, P->x, P->y, P->n, U0, U1, (const cd*)P->wphi[P->wcur],
                         (const cd*)P->wphi[P->wcur ^ 1], g, c->p.U, dt, wv);
    }
    P->wcur ^= 1;
  } else if (P->rays) {                    // zeta1 beside U1 (YBJModel: q is steady as psi is, one plane)
    if (!c->ybj) pt_form_zeta(c, P->zeta[P->cur ^ 1]);
    ProfScope ps(c, PK_PT_RAYS);
    hipLaunchKernelGGL(k_pt_rk4_r, dim3(pt_blocks(P->n)), dim3(256), 0, c->stream, P->x, P->y, P->k, P->l, P->n, U0, U1, (const double*)P->zeta[P->cur],
                       (const double*)P->zeta[c->ybj ? P->cur : P->cur ^ 1], g, c->p.U, P->eta, c->p.dt);
  } else if (P->tan) {
    ProfScope ps(c, PK_PT_TANGENT);
    hipLaunchKernelGGL(k_pt_rk4_t, dim3(pt_blocks(P->n)), dim3(256), 0, c->stream, P->x, P->y, P->f[0], P->f[1], P->f[2], P->f[3], P->n, U0, U1, g,
                       c->p.U, c->p.dt);
  } else {
    hipLaunchKernelGGL(k_pt_rk4, dim3(pt_blocks(P->n)), dim3(256), 0, c->stream, P->x, P->y, P->n, U0, U1, g, c->p.U, c->p.dt);
  }
  HIPCHK(c, hipGetLastError());
  if (!c->ybj) P->cur ^= 1;
  return P->rg.tick() ? pt_record(c) : 0;
}

int nq_particles_attach(nq_ctx* c, int n, const double* x, const double* y, double Lx, double Ly, int record_every, int capacity,
                        int nnames, const int* names) {
  NQ_SINGLE_RANK(c, "nq_particles_attach");
  if (c->pt) NQ_FAIL(c, -4, "nq_particles_attach: particles are attached already (nq_particles_detach first)");
  if (n < 1 || !x || !y) NQ_FAIL(c, -1, "nq_particles_attach: n = %d (>= 1) and both coordinate arrays", n);
  if (!(Lx > 0.0) || !(Ly > 0.0) || !std::isfinite(Lx) || !std::isfinite(Ly)) NQ_FAIL(c, -1, "nq_particles_attach: domain %g x %g", Lx, Ly);
  if (record_every < 0 || (record_every > 0 && capacity < 1)) NQ_FAIL(c, -1, "nq_particles_attach: record_every = %d, capacity = %d", record_every, capacity);
  if (nnames < 0 || nnames > 10 || (nnames > 0 && !names)) NQ_FAIL(c, -1, "nq_particles_attach: %d record names", nnames);
  int ncol = 0;
  for (int i = 0; i < nnames; ++i) {
    if (!pt_name_ok(names[i])) NQ_FAIL(c, -1, "nq_particles_attach: record name %d", names[i]);
    if (pt_name_needs_phi(names[i]) && !c->kernel_family) NQ_FAIL(c, -1, "nq_particles_attach: QGModel has no wave field (phi)");
    if (pt_name_needs_waves(names[i]) && !c->kernel_family) NQ_FAIL(c, -1, "nq_particles_attach: record name %d is the Kernel family's (zeta, rays)", names[i]);
    ncol += names[i] == PT_PHI ? 2 : 1;
  }
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(x[i]) || !std::isfinite(y[i])) NQ_FAIL(c, -1, "nq_particles_attach: particle %d has a non-finite coordinate", i);
  HIPCHK(c, hipSetDevice(c->device));
  c->pt_L[0] = Lx;
  c->pt_L[1] = Ly;
  c->pt = new NqParticles();
  NqParticles* P = c->pt;
  P->n = n;
  P->rg.init(record_every > 0 ? capacity : 0, record_every);
  P->ncol = ncol;
  P->names.assign(names, names + nnames);
  P->wf0 = c->p.f;                         // the clock of "uw" / "vw" until nq_particles_clock / nq_particles_wave set it
  const size_t plane = (size_t)c->N * c->N;
  const char* what = "nq_particles_attach";
  int rc = att_alloc(c, P, &P->x, (size_t)n, what);
  if (!rc) rc = att_alloc(c, P, &P->y, (size_t)n, what);
  if (!rc) rc = att_alloc(c, P, &P->uv[0], plane, what);
  if (!rc && !c->ybj) rc = att_alloc(c, P, &P->uv[1], plane, what);
  if (!rc && c->ybj) P->uv[1] = P->uv[0];
  if (!rc && P->rg.cap > 0) rc = att_alloc(c, P, &P->ring, (size_t)P->rg.cap * (2 + ncol) * n, what);
  if (rc) return att_fail(c, c->pt, rc);
  // (hipMemcpy from pageable memory returns once the source is consumed)
  HIPCHK(c, hipMemcpyAsync(P->x, x, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(P->y, y, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
  if (P->rg.every > 0) {
    rc = pt_record(c);
    if (rc) return att_fail(c, c->pt, rc);
  }
  return nq_sync(c);
}
// the "uw" / "vw" columns of the record written at attach, again with the clock (and amplitude) just set; rays: the "k", "l"
// and "omega" columns instead, with the mode just set; which == 2: the columns of stretch mode
static int pt_rewrite_wave_columns(nq_ctx* c, int which = 0) {
  NqParticles* P = c->pt;
  if (P->rg.every <= 0 || P->rg.count != 1) return 0;
  const size_t n = (size_t)P->n;
  double* r = P->ring + (size_t)P->rg.oldest(0) * (2 + P->ncol) * n;
  int col = 2;
  for (int name : P->names) {
    if (which == 2 ? pt_name_of_tangent(name) : which == 1 ? pt_name_of_rays(name) : (name == PT_UW || name == PT_VW)) {
      const int rc = pt_sample_into(c, name, r + col * n, nullptr);
      if (rc) return rc;
    }
    col += name == PT_PHI ? 2 : 1;
  }
  return 0;
}
static int pt_set_clock(nq_ctx* c, const char* what, double f0, double t0) {
  if (!c->pt) NQ_FAIL(c, -4, "%s: no particles attached", what);
  if (!c->kernel_family) NQ_FAIL(c, -4, "%s: QGModel has no wave field (phi)", what);
  if (!std::isfinite(f0) || !std::isfinite(t0)) NQ_FAIL(c, -1, "%s: f0 = %g, t0 = %g", what, f0, t0);
  if (c->pt->rg.steps > 0) NQ_FAIL(c, -4, "%s: the particles have moved already (call it right after nq_particles_attach)", what);
  c->pt->wf0 = f0;
  c->pt->wt0 = t0;
  return 0;
}
int nq_particles_clock(nq_ctx* c, double f0, double t0) {
  NQ_SINGLE_RANK(c, "nq_particles_clock");
  int rc = pt_set_clock(c, "nq_particles_clock", f0, t0);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  rc = pt_rewrite_wave_columns(c);
  if (rc) return rc;
  return nq_sync(c);
}
int nq_particles_wave(nq_ctx* c, double amplitude, double f0, double t0) {
  NQ_SINGLE_RANK(c, "nq_particles_wave");
  NqParticles* P = c->pt;
  if (!P) NQ_FAIL(c, -4, "nq_particles_wave: no particles attached");
  if (!c->kernel_family) NQ_FAIL(c, -4, "nq_particles_wave: QGModel has no wave field (phi)");
  if (!(amplitude > 0.0) || !std::isfinite(amplitude)) NQ_FAIL(c, -1, "nq_particles_wave: amplitude = %g (finite, > 0)", amplitude);
  if (P->wave) NQ_FAIL(c, -4, "nq_particles_wave: drifter mode is on already");
  if (P->rays) NQ_FAIL(c, -4, "nq_particles_wave: ray mode is on (the two modes exclude each other)");
  int rc = pt_set_clock(c, "nq_particles_wave", f0, t0);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t plane = (size_t)c->N * c->N;
  const DevMark before = P->mark();
  rc = att_alloc(c, P, &P->wphi[0], plane, "nq_particles_wave");
  if (!rc) rc = att_alloc(c, P, &P->wphi[1], plane, "nq_particles_wave");
  if (rc) {                                // the particles stay as they were
    c->bytes -= P->rollback(before);
    P->wphi[0] = P->wphi[1] = nullptr;
    return rc;
  }
  P->wa = amplitude;
  P->wave = true;
  P->w0 = false;
  rc = pt_rewrite_wave_columns(c);
  if (rc) return rc;
  return nq_sync(c);
}
// ray mode
int nq_particles_rays(nq_ctx* c, const double* k, const double* l, double eta) {
  NQ_SINGLE_RANK(c, "nq_particles_rays");
  NqParticles* P = c->pt;
  if (!P) NQ_FAIL(c, -4, "nq_particles_rays: no particles attached");
  if (!c->kernel_family) NQ_FAIL(c, -4, "nq_particles_rays: QGModel has no near-inertial waves");
  if (P->rays) NQ_FAIL(c, -4, "nq_particles_rays: ray mode is on already");
  if (P->wave) NQ_FAIL(c, -4, "nq_particles_rays: drifter mode is on (the two modes exclude each other)");
  if (P->tan) NQ_FAIL(c, -4, "nq_particles_rays: stretch mode is on (the ray map lives in four dimensions; the two modes exclude each other)");
  if (P->rg.steps > 0) NQ_FAIL(c, -4, "nq_particles_rays: the particles have moved already (call it right after nq_particles_attach)");
  if (!k || !l) NQ_FAIL(c, -1, "nq_particles_rays: both wavevector arrays");
  if (!std::isfinite(eta)) NQ_FAIL(c, -1, "nq_particles_rays: eta = %g", eta);
  for (int i = 0; i < P->n; ++i)
    if (!std::isfinite(k[i]) || !std::isfinite(l[i])) NQ_FAIL(c, -1, "nq_particles_rays: ray %d has a non-finite wavevector", i);
  HIPCHK(c, hipSetDevice(c->device));
  const size_t plane = (size_t)c->N * c->N, n = (size_t)P->n;
  const DevMark before = P->mark();
  const char* what = "nq_particles_rays";
  int rc = att_alloc(c, P, &P->k, n, what);
  if (!rc) rc = att_alloc(c, P, &P->l, n, what);
  if (!rc) rc = att_alloc(c, P, &P->zeta[0], plane, what);
  if (!rc && !c->ybj) rc = att_alloc(c, P, &P->zeta[1], plane, what);
  if (rc) {                                // the particles stay as they were
    c->bytes -= P->rollback(before);
    P->k = P->l = P->zeta[0] = P->zeta[1] = nullptr;
    return rc;
  }
  if (c->ybj) P->zeta[1] = P->zeta[0];
  HIPCHK(c, hipMemcpyAsync(P->k, k, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(P->l, l, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
  P->eta = eta;
  P->rays = true;
  P->z0 = false;
  rc = pt_rewrite_wave_columns(c, 1);
  if (rc) return rc;
  return nq_sync(c);
}
int nq_particles_get_rays(nq_ctx* c, double* k, double* l) {
  NQ_SINGLE_RANK(c, "nq_particles_get_rays");
  if (!c->pt) NQ_FAIL(c, -4, "nq_particles_get_rays: no particles attached");
  if (!c->pt->rays) NQ_FAIL(c, -4, "nq_particles_get_rays: ray mode is off");
  if (!k || !l) return -1;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(k, c->pt->k, sizeof(double) * c->pt->n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(l, c->pt->l, sizeof(double) * c->pt->n, hipMemcpyDeviceToHost, c->stream));
  return nq_sync(c);
}
// stretch mode
int nq_particles_tangent(nq_ctx* c, const double* F0) {
  NQ_SINGLE_RANK(c, "nq_particles_tangent");
  NqParticles* P = c->pt;
  if (!P) NQ_FAIL(c, -4, "nq_particles_tangent: no particles attached");
  if (P->tan) NQ_FAIL(c, -4, "nq_particles_tangent: stretch mode is on already");
  if (P->rays) NQ_FAIL(c, -4, "nq_particles_tangent: ray mode is on (the ray map lives in four dimensions; the two modes exclude each other)");
  if (P->rg.steps > 0) NQ_FAIL(c, -4, "nq_particles_tangent: the particles have moved already (call it right after nq_particles_attach)");
  const size_t n = (size_t)P->n;
  if (F0)
    for (size_t i = 0; i < 4 * n; ++i)
      if (!std::isfinite(F0[i])) NQ_FAIL(c, -1, "nq_particles_tangent: F0 is not finite at entry %zu of particle %zu", i / n, i % n);
  HIPCHK(c, hipSetDevice(c->device));
  const DevMark before = P->mark();
  int rc = 0;
  for (int k = 0; k < 4 && !rc; ++k) rc = att_alloc(c, P, &P->f[k], n, "nq_particles_tangent");
  if (rc) {                                // the particles stay as they were
    c->bytes -= P->rollback(before);
    P->f[0] = P->f[1] = P->f[2] = P->f[3] = nullptr;
    return rc;
  }
  if (F0) {
    for (int k = 0; k < 4; ++k) HIPCHK(c, hipMemcpyAsync(P->f[k], F0 + (size_t)k * n, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
  } else {
    hipLaunchKernelGGL(k_pt_tan_identity, dim3(pt_blocks(P->n)), dim3(256), 0, c->stream, P->f[0], P->f[1], P->f[2], P->f[3], P->n);
    HIPCHK(c, hipGetLastError());
  }
  P->tan = true;
  P->tan_step0 = 0;
  P->tan_count0 = 0;
  rc = pt_rewrite_wave_columns(c, 2);
  if (rc) return rc;
  return nq_sync(c);
}
int nq_particles_get_tangent(nq_ctx* c, double* F) {
  NQ_SINGLE_RANK(c, "nq_particles_get_tangent");
  if (!c->pt) NQ_FAIL(c, -4, "nq_particles_get_tangent: no particles attached");
  if (!c->pt->tan) NQ_FAIL(c, -4, "nq_particles_get_tangent: stretch mode is off");
  if (!F) return -1;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = (size_t)c->pt->n;
  for (int k = 0; k < 4; ++k) HIPCHK(c, hipMemcpyAsync(F + (size_t)k * n, c->pt->f[k], sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
  return nq_sync(c);
}
int nq_particles_tangent_reset(nq_ctx* c) {
  NQ_SINGLE_RANK(c, "nq_particles_tangent_reset");
  NqParticles* P = c->pt;
  if (!P) NQ_FAIL(c, -4, "nq_particles_tangent_reset: no particles attached");
  if (!P->tan) NQ_FAIL(c, -4, "nq_particles_tangent_reset: stretch mode is off");
  HIPCHK(c, hipSetDevice(c->device));
  hipLaunchKernelGGL(k_pt_tan_identity, dim3(pt_blocks(P->n)), dim3(256), 0, c->stream, P->f[0], P->f[1], P->f[2], P->f[3], P->n);
  HIPCHK(c, hipGetLastError());
  P->tan_step0 = P->rg.steps;
  P->tan_count0 = P->rg.count;
  return nq_sync(c);
}
int nq_particles_tangent_step0(nq_ctx* c, long long* step) {
  NQ_SINGLE_RANK(c, "nq_particles_tangent_step0");
  if (!c->pt) NQ_FAIL(c, -4, "nq_particles_tangent_step0: no particles attached");
  if (!c->pt->tan) NQ_FAIL(c, -4, "nq_particles_tangent_step0: stretch mode is off");
  if (!step) return -1;
  *step = c->pt->tan_step0;
  return 0;
}
int nq_particles_detach(nq_ctx* c) {
  NQ_SINGLE_RANK(c, "nq_particles_detach");
  if (!c->pt) NQ_FAIL(c, -4, "nq_particles_detach: no particles attached");
  att_release(c, c->pt);
  return 0;
}
int nq_particles_get(nq_ctx* c, double* x, double* y) {
  NQ_SINGLE_RANK(c, "nq_particles_get");
  if (!c->pt) NQ_FAIL(c, -4, "nq_particles_get: no particles attached");
  if (!x || !y) return -1;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(x, c->pt->x, sizeof(double) * c->pt->n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(y, c->pt->y, sizeof(double) * c->pt->n, hipMemcpyDeviceToHost, c->stream));
  return nq_sync(c);
}
int nq_particles_sample(nq_ctx* c, int nnames, const int* names, double* out) {
  NQ_SINGLE_RANK(c, "nq_particles_sample");
  NqParticles* P = c->pt;
  if (!P) NQ_FAIL(c, -4, "nq_particles_sample: no particles attached");
  if (nnames < 0 || (nnames > 0 && (!names || !out))) return -1;
  for (int i = 0; i < nnames; ++i) {
    if (!pt_name_ok(names[i])) NQ_FAIL(c, -1, "nq_particles_sample: name %d", names[i]);
    if (pt_name_needs_phi(names[i]) && !c->kernel_family) NQ_FAIL(c, -1, "nq_particles_sample: QGModel has no wave field (phi)");
    if (pt_name_needs_waves(names[i]) && !c->kernel_family) NQ_FAIL(c, -1, "nq_particles_sample: name %d is the Kernel family's (zeta, rays)", names[i]);
    if (pt_name_of_rays(names[i]) && !P->rays) NQ_FAIL(c, -1, "nq_particles_sample: name %d needs ray mode (nq_particles_rays)", names[i]);
    if (pt_name_of_tangent(names[i]) && !P->tan) NQ_FAIL(c, -1, "nq_particles_sample: name %d needs stretch mode (nq_particles_tangent)", names[i]);
  }
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = (size_t)P->n;
  if (!P->samp) { int rc = att_alloc(c, P, &P->samp, 2 * n, "nq_particles_sample"); if (rc) return rc; }
  size_t col = 0;
  for (int i = 0; i < nnames; ++i) {
    const int w = names[i] == PT_PHI ? 2 : 1;
    int rc = pt_sample_into(c, names[i], P->samp, w == 2 ? P->samp + n : nullptr);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(out + col * n, P->samp, sizeof(double) * w * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));          // (samp is reused by the next name)
    col += w;
  }
  return nq_sync(c);
}
int nq_particles_records(nq_ctx* c, long long* info, long long* steps, double* out) {
  NQ_SINGLE_RANK(c, "nq_particles_records");
  NqParticles* P = c->pt;
  if (!P) NQ_FAIL(c, -4, "nq_particles_records: no particles attached");
  if (!info) return -1;
  const long long m = P->rg.held();
  info[0] = P->rg.count;
  info[1] = m;
  info[2] = 2 + P->ncol;
  info[3] = P->rg.steps;
  if (!steps && !out) return 0;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t rec = (size_t)(2 + P->ncol) * P->n;
  for (long long r = 0; r < m; ++r) {
    const int slot = P->rg.oldest(r);
    if (steps) steps[r] = P->rg.ring_step[slot];
    if (out) HIPCHK(c, hipMemcpyAsync(out + (size_t)r * rec, P->ring + (size_t)slot * rec, sizeof(double) * rec, hipMemcpyDeviceToHost, c->stream));
  }
  return nq_sync(c);
}

// ---- stochastic forcing (kernels and the generator: nq_forcing.hpp) --------------------------------
// bounding box of A > 0 on a (N, cols) host plane: cols = N/2+1 (half: k itself) or N (full: |k| as |l|)
static FcBox fc_box(const double* A, int N, int cols) {
  int L = -1, K = -1;
  for (int l = 0; l < N; ++l)
    for (int k = 0; k < cols; ++k)
      if (A[(size_t)l * cols + k] > 0.0) {
        const int al = l <= N / 2 ? l : N - l, ak = (cols == N && k > N / 2) ? N - k : k;
        if (al > L) L = al;
        if (ak > K) K = ak;
      }
  FcBox b = {N, L, K, 0, 0};
  if (L < 0) return b;
  b.nrows = 2 * L + 1 < N ? 2 * L + 1 : N;
  b.ncols = cols == N ? (2 * K + 1 < N ? 2 * K + 1 : N) : K + 1;
  return b;
}
static dim3 fc_grid(const FcBox& b) { return dim3((b.ncols + 63) / 64, (b.nrows + 3) / 4); }

// one increment of step index s into the state, its work into F->work, then the end of a step: phi, phiy from the new phih
// (when phi was forced), the inversion of the new state with its spectral sums carried into the next step's slot 0
static int fc_apply(nq_ctx* c) {
  NqForcing* F = c->fc;
  const double sdt = sqrt(c->p.dt);
  const uint32_t s = (uint32_t)((unsigned long long)F->s & 0xffffffffull);
  const bool fq = F->Aq && F->bq.nrows > 0, fw = F->Aphi && F->bphi.nrows > 0;
  if (fq)
    hipLaunchKernelGGL(k_force_half<double>, F->gq, dim3(64, 4), 0, c->stream, c->q.y[c->q.cur], c->dual ? c->q2.y[c->q2.cur] : (cd*)nullptr, c->Ph,
                       (const double*)F->Aq, F->bq, sdt, s, F->seed, (const cd*)c->ph, c->Ph, (const double*)c->kk, (const double*)c->ll, F->partq, (cd*)nullptr);
  if (fw)
    hipLaunchKernelGGL((k_force_full<double, false>), F->gphi, dim3(64, 4), 0, c->stream, c->w.y[c->w.cur], (const double*)F->Aphi, F->bphi, sdt, s, 1u,
                       F->seed, (const cd*)c->w.y[c->w.cur], (const double*)nullptr, (const double*)nullptr, F->partphi, (cd*)nullptr);
  if (fq || fw)
    hipLaunchKernelGGL(k_force_accum, dim3(1), dim3(256), 0, c->stream, (const double*)F->partq, fq ? F->npq : 0, (const double*)F->partphi, fw ? F->npphi : 0,
                       1.0 / ((double)c->N * c->N * (double)c->N * c->N), F->work, (double*)nullptr);
  if (F->Aphi) {                          // as nq_set_phi, without its refresh of UnCoupledModel's frozen gradients (quirk Q1)
    launch_emit_phi(c, c->w.y[c->w.cur]);
    launch_A_m(c, true, {&c->mPhi, &c->mPhiy});
    if (c->bud) hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(1024), 0, c->stream, c->part0W, c->nww, NQ_PARTW, 4, c->carryW);
  }
  if (!c->ybj) do_invert_now(c);          // (YBJModel: psi is steady)
  ++F->s;
  HIPCHK(c, hipGetLastError());
  return 0;
}

int nq_forcing_attach(nq_ctx* c, const double* Aq, const double* Aphi, unsigned long long seed, long long step0) {
  NQ_SINGLE_RANK(c, "nq_forcing_attach");
  if (c->fc) NQ_FAIL(c, -4, "nq_forcing_attach: a forcing is attached already (nq_forcing_detach first)");
  if (!Aq && !Aphi) NQ_FAIL(c, -1, "nq_forcing_attach: no amplitude plane");
  if (Aq && c->ybj) NQ_FAIL(c, -1, "nq_forcing_attach: YBJModel's psi is steady (phi forcing only)");
  if (Aphi && !c->kernel_family) NQ_FAIL(c, -1, "nq_forcing_attach: QGModel has no wave field (q forcing only)");
  if (step0 < 0) NQ_FAIL(c, -1, "nq_forcing_attach: step0 = %lld", step0);
  const int N = c->N, Wh = N / 2 + 1;
  if (Aq) {
    for (size_t i = 0; i < (size_t)N * Wh; ++i)
      if (!std::isfinite(Aq[i]) || Aq[i] < 0.0) NQ_FAIL(c, -1, "nq_forcing_attach: the q amplitude is not finite and >= 0 at element %zu", i);
    for (int l = 1; l < N / 2; ++l)          // the increment is a real field's: column 0 mirrors in l
      if (Aq[(size_t)l * Wh] != Aq[(size_t)(N - l) * Wh]) NQ_FAIL(c, -1, "nq_forcing_attach: the q amplitude differs between rows %d and %d of column 0", l, N - l);
  }
  if (Aphi)
    for (size_t i = 0; i < (size_t)N * N; ++i)
      if (!std::isfinite(Aphi[i]) || Aphi[i] < 0.0) NQ_FAIL(c, -1, "nq_forcing_attach: the phi amplitude is not finite and >= 0 at element %zu", i);
  HIPCHK(c, hipSetDevice(c->device));
  c->fc = new NqForcing();
  NqForcing* F = c->fc;
  F->seed = seed;
  F->s = step0;
  const char* what = "nq_forcing_attach";
  int rc = att_alloc(c, F, &F->work, 2, what);
  if (!rc && Aq) {
    F->bq = fc_box(Aq, N, Wh);
    F->gq = fc_grid(F->bq);
    F->npq = (int)(F->gq.x * F->gq.y);
    rc = att_alloc(c, F, &F->Aq, (size_t)N * Wh, what);
    if (!rc && F->npq > 0) rc = att_alloc(c, F, &F->partq, (size_t)2 * F->npq, what);
  }
  if (!rc && Aphi) {
    F->bphi = fc_box(Aphi, N, N);
    F->gphi = fc_grid(F->bphi);
    F->npphi = (int)(F->gphi.x * F->gphi.y);
    rc = att_alloc(c, F, &F->Aphi, (size_t)N * N, what);
    if (!rc && F->npphi > 0) rc = att_alloc(c, F, &F->partphi, (size_t)2 * F->npphi, what);
  }
  if (rc) return att_fail(c, c->fc, rc);
  if (Aq) HIPCHK(c, hipMemcpyAsync(F->Aq, Aq, sizeof(double) * (size_t)N * Wh, hipMemcpyHostToDevice, c->stream));
  if (Aphi) HIPCHK(c, hipMemcpyAsync(F->Aphi, Aphi, sizeof(double) * (size_t)N * N, hipMemcpyHostToDevice, c->stream));
  return nq_sync(c);
}
int nq_forcing_detach(nq_ctx* c) {
  NQ_SINGLE_RANK(c, "nq_forcing_detach");
  if (!c->fc) NQ_FAIL(c, -4, "nq_forcing_detach: no forcing attached");
  att_release(c, c->fc);
  return 0;
}
int nq_forcing_apply(nq_ctx* c) {
  NQ_SINGLE_RANK(c, "nq_forcing_apply");
  if (!c->fc) NQ_FAIL(c, -4, "nq_forcing_apply: no forcing attached");
  pt_mark_stale(c);
  HIPCHK(c, hipSetDevice(c->device));
  const int rc = fc_apply(c);
  if (rc) return rc;
  return nq_sync(c);
}
int nq_forcing_increment(nq_ctx* c, int stream, long long s, double* out) {
  NQ_SINGLE_RANK(c, "nq_forcing_increment");
  NqForcing* F = c->fc;
  if (!F) NQ_FAIL(c, -4, "nq_forcing_increment: no forcing attached");
  if (!out || s < 0) return -1;
  if (stream != 0 && stream != 1) NQ_FAIL(c, -1, "nq_forcing_increment: stream %d (0: q, 1: phi)", stream);
  if (!(stream == 0 ? F->Aq : F->Aphi)) NQ_FAIL(c, -4, "nq_forcing_increment: %s is not forced", stream == 0 ? "q" : "phi");
  HIPCHK(c, hipSetDevice(c->device));
  const int N = c->N;
  const size_t n = (size_t)N * (stream == 0 ? N / 2 + 1 : N);
  void* tmp = nullptr;
  HIPCHK(c, hipMalloc(&tmp, sizeof(cd) * n));
  const double sdt = sqrt(c->p.dt);
  const uint32_t s32 = (uint32_t)((unsigned long long)s & 0xffffffffull);
  hipError_t er = hipMemsetAsync(tmp, 0, sizeof(cd) * n, c->stream);
  if (stream == 0 && F->bq.nrows > 0)
    hipLaunchKernelGGL(k_force_half<double>, F->gq, dim3(64, 4), 0, c->stream, (cd*)nullptr, (cd*)nullptr, c->Ph, (const double*)F->Aq, F->bq, sdt, s32, F->seed,
                       (const cd*)nullptr, 0, (const double*)nullptr, (const double*)nullptr, (double*)nullptr, reinterpret_cast<cd*>(tmp));
  if (stream == 1 && F->bphi.nrows > 0)
    hipLaunchKernelGGL((k_force_full<double, false>), F->gphi, dim3(64, 4), 0, c->stream, (cd*)nullptr, (const double*)F->Aphi, F->bphi, sdt, s32, 1u, F->seed,
                       (const cd*)nullptr, (const double*)nullptr, (const double*)nullptr, (double*)nullptr, reinterpret_cast<cd*>(tmp));
  if (er == hipSuccess) er = hipGetLastError();
  if (er == hipSuccess) er = hipMemcpyAsync(out, tmp, sizeof(cd) * n, hipMemcpyDeviceToHost, c->stream);
  const int rc = nq_sync(c);
  (void)hipFree(tmp);
  if (er != hipSuccess) NQ_FAIL(c, -5, "nq_forcing_increment: %s", hipGetErrorString(er));
  return rc;
}
int nq_forcing_state(nq_ctx* c, double* out3) {
  NQ_SINGLE_RANK(c, "nq_forcing_state");
  NqForcing* F = c->fc;
  if (!F) NQ_FAIL(c, -4, "nq_forcing_state: no forcing attached");
  if (!out3) return -1;
  HIPCHK(c, hipSetDevice(c->device));
  out3[0] = (double)F->s;
  HIPCHK(c, hipMemcpyAsync(out3 + 1, F->work, sizeof(double) * 2, hipMemcpyDeviceToHost, c->stream));
  return nq_sync(c);
}

// ---- slab decomposition API ------------------------------------------------------------------------
int nq_slab_info(const nq_ctx* c, int* info) {
  // info[0..7] = nranks, rank, local rows, full-plane local columns, first full column,
  //              half-spectrum local (valid) columns, first half-spectrum column, half-spectrum pitch
  if (!c || !info) return -1;
  info[0] = c->P; info[1] = c->rank; info[2] = c->Nloc; info[3] = c->Wf; info[4] = c->kf0;
  info[5] = c->Wh; info[6] = c->kh0; info[7] = c->Ph;
  return 0;
}

int nq_group_buffers(nq_ctx* c, int group, void** x_side, void** y_side, long long* elems) {
  if (!c || group < 0 || group > 3) return -1;
  if (x_side) *x_side = c->G[group].bx;
  if (y_side) *y_side = c->G[group].by;
  if (elems) *elems = (long long)c->G[group].elems;
  return 0;
}

// local column slab of a spectral state plane: which 0 = qh (half spectrum, (ny, local valid columns)),
// 1 = phih (full plane, (ny, local columns)); host arrays are contiguous
int nq_upload_spectral(nq_ctx* c, int which, const double* host) {
  if (!c || !host) return -1;
  HIPCHK(c, hipSetDevice(c->device));
  if (which == 0) {
    if (c->Wh > 0) HIPCHK(c, hipMemcpy2DAsync(c->q.y[c->q.cur], sizeof(cd) * c->Ph, host, sizeof(cd) * c->Wh, sizeof(cd) * c->Wh, c->N, hipMemcpyHostToDevice, c->stream));
    if (c->dual) HIPCHK(c, hipMemcpyAsync(c->q2.y[c->q2.cur], c->q.y[c->q.cur], sizeof(cd) * (size_t)c->N * c->Ph, hipMemcpyDeviceToDevice, c->stream));
    { int rc = reset_passenger(c); if (rc) return rc; }
  } else if (which == 1) {
    if (!c->kernel_family) NQ_FAIL(c, -4, "no wave field in QGModel");
    HIPCHK(c, hipMemcpyAsync(c->w.y[c->w.cur], host, sizeof(cd) * (size_t)c->N * c->Wf, hipMemcpyHostToDevice, c->stream));
  } else NQ_FAIL(c, -1, "nq_upload_spectral: which = %d", which);
  return nq_sync(c);
}
int nq_download_spectral(nq_ctx* c, int which, double* host) {
  if (!c || !host) return -1;
  HIPCHK(c, hipSetDevice(c->device));
  if (which == 0 || (which >= 2 && which <= 6) || which == 8) {   // half-spectrum planes: qh, ph, qwh, second copy of qh, ch, stage-4 qh (both copies)
    if (which == 3 && c->p.model != NQ_MODEL_COUPLED) NQ_FAIL(c, -4, "qwh exists only in the coupled model");
    if ((which == 4 || which == 8) && !c->dual) NQ_FAIL(c, -4, "no second copy of qh in this context (dual_q)");
    if (which == 5 && !c->passive) NQ_FAIL(c, -4, "no passive scalar in this context");
    const cd* src = which == 0 ? c->q.y[c->q.cur] : (which == 2 ? c->ph : (which == 3 ? c->qwh : (which == 4 ? c->q2.y[c->q2.cur] : (which == 5 ? c->cq.y[c->cq.cur] : (which == 8 ? c->q2.y[(c->q2.cur + 2) % 3] : c->q.y[(c->q.cur + 2) % 3])))));
    if (c->Wh > 0) HIPCHK(c, hipMemcpy2DAsync(host, sizeof(cd) * c->Wh, src, sizeof(cd) * c->Ph, sizeof(cd) * c->Wh, c->N, hipMemcpyDeviceToHost, c->stream));
  } else if (which == 1 || which == 7) {
    if (!c->kernel_family) NQ_FAIL(c, -4, "no wave field in QGModel");
    const cd* src = which == 1 ? c->w.y[c->w.cur] : c->w.y[(c->w.cur + 2) % 3];
    HIPCHK(c, hipMemcpyAsync(host, src, sizeof(cd) * (size_t)c->N * c->Wf, hipMemcpyDeviceToHost, c->stream));
  } else if (which == 9 || which == 11 || which == 12) {      // nq_tick_snapshot: qh, its second copy, qwh
    const cd* src = which == 9 ? c->tick_qh : (which == 11 ? c->tick_q2 : c->tick_qwh);
    if (!src) NQ_FAIL(c, -4, "nq_download_spectral: which = %d: no nq_tick_snapshot yet (or no such plane in this context)", which);
    if (c->Wh > 0) HIPCHK(c, hipMemcpy2DAsync(host, sizeof(cd) * c->Wh, src, sizeof(cd) * c->Ph, sizeof(cd) * c->Wh, c->N, hipMemcpyDeviceToHost, c->stream));
  } else if (which == 10) {                                   // ... and phih
    if (!c->tick_w) NQ_FAIL(c, -4, "nq_download_spectral: which = 10: no nq_tick_snapshot yet (or no wave field)");
    HIPCHK(c, hipMemcpyAsync(host, c->tick_w, sizeof(cd) * (size_t)c->N * c->Wf, hipMemcpyDeviceToHost, c->stream));
  } else NQ_FAIL(c, -1, "nq_download_spectral: which = %d", which);
  return nq_sync(c);
}
// What only a diagnostics tick refreshes in the reference (upsilon: Kernel.py:618; phq, phw, uq, vq, uw, vw: CoupledModel.py:
// 99-113; YBJModel's lapphi: Kernel.py:685 through the tick's _calc_energy_conversion) stays the TICK's until the next one, however
// many steps follow.  The host classes rebuild those arrays on demand; this keeps the spectra they derive from: device-to-device
// copies of this rank's qh (both copies), phih and qwh on the context's stream (planes allocated by the first call).
int nq_tick_snapshot(nq_ctx* c) {
  if (!c) return -1;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t full = (size_t)c->N * c->Wf, half = (size_t)c->N * c->Ph;
  if (!c->tick_qh) {
    ALLOC(c, c->tick_qh, half);
    if (c->dual) ALLOC(c, c->tick_q2, half);
    if (c->kernel_family) ALLOC(c, c->tick_w, full);
    if (c->qwh) ALLOC(c, c->tick_qwh, half);
  }
  HIPCHK(c, hipMemcpyAsync(c->tick_qh, c->q.y[c->q.cur], sizeof(cd) * half, hipMemcpyDeviceToDevice, c->stream));
  if (c->tick_q2) HIPCHK(c, hipMemcpyAsync(c->tick_q2, c->q2.y[c->q2.cur], sizeof(cd) * half, hipMemcpyDeviceToDevice, c->stream));
  if (c->tick_w) HIPCHK(c, hipMemcpyAsync(c->tick_w, c->w.y[c->w.cur], sizeof(cd) * full, hipMemcpyDeviceToDevice, c->stream));
  if (c->tick_qwh) HIPCHK(c, hipMemcpyAsync(c->tick_qwh, c->qwh, sizeof(cd) * half, hipMemcpyDeviceToDevice, c->stream));
  return 0;
}

// One phase of the distributed step (see "phases of one ETDRK4 stage").  Asynchronous on the stream.
//   NQ_PH_PRODUCTS(stage)  row kernel: reads G3.x, G1.x, writes G0.x             then exchange G0 (x -> y)
//   NQ_PH_UPDATE(stage)    y passes + stage updates: reads G0.y, writes G1.y (and G3.y unless Coupled)
//                                                                                  then exchange G1 (y -> x) [, G3]
//   NQ_PH_WAVEPV           Coupled row kernel: reads G1.x, writes G2.x            then exchange G2 (x -> y)
//   NQ_PH_INVERT(stage)    Coupled inversion: reads G2.y, writes G3.y             then exchange G3 (y -> x)
//   NQ_PH_EMIT_PHI         after nq_upload_spectral(phih): writes G1.y            then exchange G1 (y -> x)
//   NQ_PH_INVERT_NOW       inversion of the current qh (set_q): Coupled: run NQ_PH_WAVEPV + exchange G2 first
//   NQ_PH_BUDGET_SUMS      local sums of one step -> nq_budget_sums buffer        then all-reduce (sum) it
//   NQ_PH_BUDGET_FINISH    RK-weighted accumulation from the (reduced) sums
int nq_phase(nq_ctx* c, int phase, int stage) {
  if (!c) return -1;
  if (c->ybj) NQ_FAIL(c, -4, "nq_phase: YBJModel has a stage graph of its own (nq_step, nq_slab_step)");
  if (stage < 0 || stage > 3) NQ_FAIL(c, -1, "nq_phase: stage %d", stage);
  HIPCHK(c, hipSetDevice(c->device));
  switch (phase) {
    case NQ_PH_PRODUCTS: phase_products(c, stage); break;
    case NQ_PH_UPDATE: phase_update(c, stage); break;
    case NQ_PH_WAVEPV: phase_wavepv(c); break;
    case NQ_PH_INVERT: phase_invert(c, stage); break;
    case NQ_PH_EMIT_PHI:
      if (!c->kernel_family) NQ_FAIL(c, -4, "no wave field in QGModel");
      launch_emit_phi(c, c->w.y[c->w.cur]);
      launch_A_m(c, true, {&c->mPhi, &c->mPhiy});
      // local part of the carried sums; the caller all-reduces them (nq_reduce_buffer)
      if (c->bud) hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(1024), 0, c->stream, c->part0W, c->nww, NQ_PARTW, 4, c->carryW);
      break;
    case NQ_PH_INVERT_NOW:
      phase_invert_y(c, c->q.y[c->q.cur], true, c->part0Q, nullptr);
      if (c->bud && c->kernel_family)
        hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(1024), 0, c->stream, c->part0Q, c->nwq, 3, 3, c->carryQ);
      break;
    case NQ_PH_BUDGET_SUMS: phase_budget_sums(c); break;
    case NQ_PH_BUDGET_FINISH: phase_budget_finish(c); break;
    default: NQ_FAIL(c, -1, "nq_phase: unknown phase %d", phase);
  }
  HIPCHK(c, hipGetLastError());
  return 0;
}

// The 64-double block that has to be summed over ranks at three points (see nq_phase): elements [0,44) after
// NQ_PH_BUDGET_SUMS, [44,48) after NQ_PH_EMIT_PHI, [48,51) after NQ_PH_INVERT_NOW.  It is buffers[8] of
// nq_create_slab when that was given.
int nq_reduce_buffer(nq_ctx* c, int which, void** ptr, int* count) {
  if (!c || !ptr || !count) return -1;
  if (!c->bud) NQ_FAIL(c, -4, "budgets are disabled in this context");
  switch (which) {
    case 0: *ptr = c->bsums; *count = 44; break;
    case 1: *ptr = c->carryW; *count = 4; break;
    case 2: *ptr = c->carryQ; *count = 3; break;
    case 3: *ptr = c->gradS1; *count = 1; break;
    case 4: *ptr = c->diag_out; *count = 16; break;
    case 5: *ptr = c->diag_out ? c->diag_out + 16 : nullptr; *count = 16; break;
    default: NQ_FAIL(c, -1, "nq_reduce_buffer: which = %d", which);
  }
  return 0;
}


// ---- the slab step inside the library: API ------------------------------------------------------------------------
int nq_comm_probe(void) {           // load-only: can this process resolve librccl at all?  (no communicator, no GPU work)
  std::string err;
  if (!rccl_load(&err)) NQ_FAIL((nq_ctx*)nullptr, -6, "nq_comm_probe: %s", err.c_str());
  return 0;
}
int nq_comm_unique_id(void* out128) {
  if (!out128) return -1;
  std::string err;
  if (!rccl_load(&err)) NQ_FAIL((nq_ctx*)nullptr, -6, "nq_comm_unique_id: %s", err.c_str());
  NcclId id;
  NCCLCHK((nq_ctx*)nullptr, g_rccl.GetUniqueId(&id));
  memcpy(out128, &id, sizeof(id));
  return 0;
}
int nq_comm_init(nq_ctx* c, const void* id128, int nranks, int rank) {
  if (!c || !id128) return -1;
  if (nranks != c->P || rank != c->rank) NQ_FAIL(c, -1, "nq_comm_init: rank %d of %d given to a context created as rank %d of %d", rank, nranks, c->rank, c->P);
  if (c->link != LINK_NONE) NQ_FAIL(c, -4, "nq_comm_init: the context already has a link");
  std::string err;
  if (!rccl_load(&err)) NQ_FAIL(c, -6, "nq_comm_init: %s", err.c_str());
  HIPCHK(c, hipSetDevice(c->device));
  NcclId id;
  memcpy(&id, id128, sizeof(id));
  NCCLCHK(c, g_rccl.CommInitRank(&c->comm, nranks, id, rank));
  c->link = LINK_RCCL;
  if (nranks > 1) {
    // RCCL's send/recv kernels run BESIDE the chunked row kernels, and a persistent row-kernel workgroup (512 threads x
    // ~250 VGPRs) fills its CU's register file, so they compete for whole CUs.  NIWQG_AMD_SLAB_RESERVE_CUS=R keeps R CUs
    // out of the row kernels' persistent grids.  Off by default: with 256 or 512 rows per chunk a grid of 256-R
    // workgroups needs an extra round of rows, which costs what the overlap gains -- to be settled
    // by measurement on a multi-GPU node.
    const char* e = getenv("NIWQG_AMD_SLAB_RESERVE_CUS");
    c->reserve_cus = e ? atoi(e) : 0;
    if (c->reserve_cus < 0 || c->reserve_cus >= c->num_cu) c->reserve_cus = 0;
  }
  return slab_link_setup(c);
}
int nq_slab_attach_peers(nq_ctx* const* ctxs, int nranks) {
  if (!ctxs || nranks < 1 || nranks > 8) NQ_FAIL((nq_ctx*)nullptr, -1, "nq_slab_attach_peers: 1..8 contexts");
  std::vector<nq_ctx*> all(ctxs, ctxs + nranks);
  for (int r = 0; r < nranks; ++r) {
    nq_ctx* c = all[r];
    if (!c || c->P != nranks || c->rank != r || c->link != LINK_NONE)
      NQ_FAIL(c, -1, "nq_slab_attach_peers: context %d is not rank %d of %d (or already linked)", r, r, nranks);
  }
  // peers on different devices of this process: the blocks then cross by peer copies (SDMA over xGMI, no CU involved) and the
  // all-reduce kernel reads the peers' buffers directly -- both need peer access, enabled here in both directions
  for (nq_ctx* a : all)
    for (nq_ctx* b : all) {
      if (a->device == b->device) continue;
      int can = 0;
      HIPCHK(a, hipDeviceCanAccessPeer(&can, a->device, b->device));
      if (!can) NQ_FAIL(a, -3, "nq_slab_attach_peers: device %d cannot access device %d", a->device, b->device);
      HIPCHK(a, hipSetDevice(a->device));
      const hipError_t e = hipDeviceEnablePeerAccess(b->device, 0);
      if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) NQ_FAIL(a, -5, "hipDeviceEnablePeerAccess(%d -> %d): %s", a->device, b->device, hipGetErrorString(e));
      (void)hipGetLastError();
    }
  for (nq_ctx* c : all) {
    c->peers = all;
    c->link = LINK_PEERS;
    int rc = slab_link_setup(c);
    if (rc) return rc;
  }
  return 0;
}
// Measurement aid (bench.py --rank-of P): this context is ONE rank of its P-rank decomposition and runs alone.  Streams, events,
// chunking and every kernel launch are those of a real rank; on the wire only the rank's own block moves (the device copy the RCCL
// link makes as well), the other P-1 blocks of every group keep whatever they held, and nothing is all-reduced.  The fields are
// therefore NOT a simulation -- what is measured is a rank's compute and launch structure without the exchange.
int nq_slab_set_null_link(nq_ctx* c) {
  if (!c) return -1;
  if (c->link != LINK_NONE) NQ_FAIL(c, -4, "nq_slab_set_null_link: the context already has a link");
  const char* e = getenv("NIWQG_AMD_SLAB_RESERVE_CUS");
  c->reserve_cus = e ? atoi(e) : 0;
  if (c->reserve_cus < 0 || c->reserve_cus >= c->num_cu) c->reserve_cus = 0;
  c->link = LINK_NULL;
  return slab_link_setup(c);
}
int nq_slab_set_callbacks(nq_ctx* c, nq_exchange_fn exchange, nq_allreduce_fn allreduce, void* user) {
  if (!c || !exchange || !allreduce) return -1;
  if (c->link != LINK_NONE && c->link != LINK_CALLBACK) NQ_FAIL(c, -4, "nq_slab_set_callbacks: the context already has a link");
  c->xcb = exchange;
  c->rcb = allreduce;
  c->cb_user = user;
  c->link = LINK_CALLBACK;
  return slab_link_setup(c);
}
// caller-owned buffers for exchange group 4 (as ext_buffers of nq_create_slab for groups 0..3), before the first step
int nq_slab_set_stage_buffers(nq_ctx* c, void* bx, void* by) {
  if (!c || !bx || !by) return -1;
  if (!c->ybj || c->P == 1) NQ_FAIL(c, -4, "nq_slab_set_stage_buffers: only YBJModel on more than one rank has exchange group 4");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const SlabGeom sg = slab_geom(&c->p, c->P);
  c->Gs = c->G[4].bx = reinterpret_cast<cd*>(bx);
  c->Gs_y = c->G[4].by = reinterpret_cast<cd*>(by);
  HIPCHK(c, hipMemsetAsync(c->Gs, 0, c->G[4].elems * sizeof(cd), c->stream));
  HIPCHK(c, hipMemsetAsync(c->Gs_y, 0, c->G[4].elems * sizeof(cd), c->stream));
  c->mGx = make_marr(sg, c->Gs, c->Gs_y, 1, 0, false);
  c->mGy = make_marr(sg, c->Gs, c->Gs_y, 1, 1, false);
  return nq_sync(c);
}
int nq_slab_config(nq_ctx* c, int nchunks) {
  if (!c) return -1;
  if (nchunks != 1 && nchunks != 2 && nchunks != 4 && nchunks != 8) NQ_FAIL(c, -1, "nq_slab_config: nchunks = %d (1, 2, 4 or 8)", nchunks);
  std::vector<nq_ctx*> grp = c->link == LINK_PEERS ? c->peers : std::vector<nq_ctx*>(1, c);
  int rc = slab_settle(grp);
  if (rc) return rc;
  for (nq_ctx* x : each(grp)) x->nchunk = nchunks;
  return 0;
}
int nq_slab_step(nq_ctx* c, int nsteps) {
  if (!c) return -1;
  if (nsteps < 0) NQ_FAIL(c, -1, "nq_slab_step: nsteps < 0");
  std::vector<nq_ctx*> grp;
  SLABTRY(slab_group(c, &grp));
  for (nq_ctx* x : each(grp)) HIPCHK(x, hipSetDevice(x->device));
  c->n_calls += 1;
  // inside the step every exchange has an A sub-pass next to it on the Y side: the rank's own block is used where it lies
  // (ArrayListR) instead of being copied across -- not with caller-moved buffers (the callback moves the own block too) and not
  // on plans without an A sub-pass (single-pass columns)
  static int redirect_on = -1;
  if (redirect_on < 0) {
    const char* e = getenv("NIWQG_AMD_SLAB_OWN_REDIRECT");
    redirect_on = (e && atoi(e) == 0) ? 0 : 1;
  }
  const bool redir = redirect_on && c->link != LINK_CALLBACK && c->link != LINK_NONE && c->S2 > 1 && c->P > 1;
  for (nq_ctx* x : each(grp)) x->redir_now = redir;
  int step_rc = 0;
  for (int i = 0; i < nsteps && step_rc == 0; ++i) {
    const bool now = c->want_uv4 && i == nsteps - 1 && c->kernel_family && !c->ybj;
    for (nq_ctx* x : each(grp)) x->uv4_now = now;
    step_rc = slab_step_once(grp);
  }
  for (nq_ctx* x : each(grp)) x->redir_now = false;
  if (step_rc) return step_rc;
  if (nsteps > 0)
    for (nq_ctx* x : each(grp)) {
      x->stepped = true;
      x->have_uv4 = x->uv4_now;
      x->want_uv4 = x->uv4_now = false;
    }
  SLABTRY(slab_settle(grp));
  for (nq_ctx* x : each(grp)) HIPCHK(x, hipGetLastError());
  return 0;
}

// rows of a physical field -> the x side of the carrier array of exchange group 0 (q: the uq slot, phi: the W slot)
static int rows_scratch(nq_ctx* c, cd** out) {
  if (!c->scr_f0) ALLOC(c, c->scr_f0, (size_t)c->Nloc * c->N);
  *out = c->scr_f0;
  return 0;
}
int nq_slab_put_rows(nq_ctx* c, int which, const double* rows) {
  if (!c || !rows) return -1;
  if (which == 1 && !c->kernel_family) NQ_FAIL(c, -4, "no wave field in QGModel");
  HIPCHK(c, hipSetDevice(c->device));
  cd* scr = nullptr;
  SLABTRY(rows_scratch(c, &scr));
  const size_t n = (size_t)c->Nloc * c->N;
  if (which == 2 && !c->passive) NQ_FAIL(c, -4, "nq_slab_put_rows: this context has no passive scalar");
  if (which == 0 || which == 2) {
    HIPCHK(c, hipMemcpyAsync(scr, rows, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    if (!launch_put_real(c, (const double*)scr, c->mUq)) NQ_FAIL(c, -2, "no row plan of length %d", c->N);
  } else if (which == 1) {
    HIPCHK(c, hipMemcpyAsync(scr, rows, sizeof(cd) * n, hipMemcpyHostToDevice, c->stream));
    if (!launch_put_cplx(c, (const cd*)scr, c->mW)) NQ_FAIL(c, -2, "no row plan of length %d", c->N);
  } else NQ_FAIL(c, -1, "nq_slab_put_rows: which = %d", which);
  HIPCHK(c, hipGetLastError());
  return nq_sync(c);                            // the host rows may be released
}
// collective half of set_q / set_phi: exchange the carrier, finish the transform on the column slabs, then the phases of
// Kernel.set_q (Kernel.py:520-535: inversion with the current phi, quirk Q2) / Kernel.set_phi (:538-551)
int nq_slab_commit(nq_ctx* c, int which) {
  if (!c) return -1;
  std::vector<nq_ctx*> grp;
  SLABTRY(slab_group(c, &grp));
  for (nq_ctx* x : each(grp)) HIPCHK(x, hipSetDevice(x->device));
  SLABTRY(slab_settle(grp));
  nq_ctx* c0 = grp[0];
  if (which == 0) {
    SLABTRY(exchange_now(grp, 0, true));
    for (nq_ctx* x : each(grp)) {
      launch_A_m(x, false, {&x->mUq});
      if (x->Wh > 0) launch_B_p(x, false, x->mUq.ys, x->mUq.pitch, x->q.y[x->q.cur], x->Ph, x->Wh, 1.0);
      if (x->dual)      // q is real: both copies of the dual-copy equation start from the same half spectrum
        HIPCHK(x, hipMemcpyAsync(x->q2.y[x->q2.cur], x->q.y[x->q.cur], sizeof(cd) * (size_t)x->N * x->Ph, hipMemcpyDeviceToDevice, x->stream));
      SLABTRY(reset_passenger(x));
    }
    if (c0->p.model == NQ_MODEL_COUPLED) {
      for (nq_ctx* x : each(grp)) phase_wavepv(x);
      SLABTRY(exchange_now(grp, 2, true));
    }
    for (nq_ctx* x : each(grp)) {
      phase_invert_y(x, x->q.y[x->q.cur], true, x->part0Q, nullptr, x->passive ? x->cq.y[x->cq.cur] : nullptr);
      if (x->bud && x->kernel_family)
        hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(1024), 0, x->stream, x->part0Q, x->nwq, 3, 3, x->carryQ);
      x->have_q = true;
    }
    SLABTRY(exchange_now(grp, 3, false));
    if (c0->bud && c0->kernel_family) SLABTRY(slab_allreduce(grp, 2));
  } else if (which == 1) {
    if (!c0->kernel_family) NQ_FAIL(c, -4, "no wave field in QGModel");
    SLABTRY(exchange_now(grp, 0, true));
    for (nq_ctx* x : each(grp)) {
      launch_A_m(x, false, {&x->mW});
      launch_B_p(x, false, x->mW.ys, x->mW.pitch, x->w.y[x->w.cur], x->Wf, x->Wf, 1.0);
      launch_emit_phi(x, x->w.y[x->w.cur]);
      launch_A_m(x, true, {&x->mPhi, &x->mPhiy});
      if (x->bud) hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(1024), 0, x->stream, x->part0W, x->nww, NQ_PARTW, 4, x->carryW);
      x->have_phi = true;
    }
    SLABTRY(exchange_now(grp, 1, false));
    if (c0->bud) SLABTRY(slab_allreduce(grp, 1));
    for (nq_ctx* x : each(grp)) SLABTRY(nq_refresh_grad_phi(x));
  } else if (which == 2 || which == 3) {        // Kernel._invert on the current state (CoupledModel.py:75-97 / UnCoupledModel.py:54-64)
    if (which == 3) {                           // QGModel.set_c (QGModel.py:476-480): the scalar's spectrum first
      if (!c0->passive) NQ_FAIL(c, -4, "nq_slab_commit: this context has no passive scalar");
      SLABTRY(exchange_now(grp, 0, true));
      for (nq_ctx* x : each(grp)) {
        launch_A_m(x, false, {&x->mUq});
        if (x->Wh > 0) launch_B_p(x, false, x->mUq.ys, x->mUq.pitch, x->cq.y[x->cq.cur], x->Ph, x->Wh, 1.0);
      }
    }
    if (c0->p.model == NQ_MODEL_COUPLED) {
      for (nq_ctx* x : each(grp)) phase_wavepv(x);
      SLABTRY(exchange_now(grp, 2, true));
    }
    for (nq_ctx* x : each(grp)) {
      phase_invert_y(x, x->q.y[x->q.cur], true, x->part0Q, nullptr, x->passive ? x->cq.y[x->cq.cur] : nullptr);
      if (x->bud && x->kernel_family)
        hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(1024), 0, x->stream, x->part0Q, x->nwq, 3, 3, x->carryQ);
    }
    SLABTRY(exchange_now(grp, 3, false));
    if (c0->bud && c0->kernel_family) SLABTRY(slab_allreduce(grp, 2));
  } else NQ_FAIL(c, -1, "nq_slab_commit: which = %d", which);
  SLABTRY(slab_settle(grp));
  for (nq_ctx* x : each(grp)) {
    HIPCHK(x, hipGetLastError());
    SLABTRY(nq_sync(x));
  }
  return 0;
}
// this rank's rows of a physical field, from the mixed-space rows of the last inversion / emission on the x side
int nq_slab_get_rows(nq_ctx* c, int id, double* out) {
  if (!c || !out) return -1;
  HIPCHK(c, hipSetDevice(c->device));
  cd* scr = nullptr;
  SLABTRY(rows_scratch(c, &scr));
  const size_t n = (size_t)c->Nloc * c->N;
  const MArr* src = nullptr;
  int mode = 0, zero_nyq = 0, mul_ik = 0;
  bool real = true;
  switch (id) {
    case NQ_F_Q: src = &c->mQ; break;
    case NQ_F_P: src = &c->mP; break;
    case NQ_F_U: src = &c->mU; break;
    case NQ_F_V: src = &c->mP; mode = 1; zero_nyq = c->kernel_family ? 1 : 0; break;
    case NQ_F_QW:
      if (c->p.model != NQ_MODEL_COUPLED) NQ_FAIL(c, -4, "qw exists only in the coupled model");
      src = &c->mQw;
      break;
    case NQ_F_C:
      if (!c->passive) NQ_FAIL(c, -4, "no passive scalar in this context");
      src = &c->mQw;                            // the scalar rides in the qw slot of group 3
      break;
    case NQ_F_PHI: src = &c->mPhi; real = false; break;
    case NQ_F_PHIX: src = &c->mGx; real = false; mul_ik = 1; break;
    case NQ_F_PHIY: src = &c->mGy; real = false; break;
    default: NQ_FAIL(c, -1, "nq_slab_get_rows: field id %d", id);
  }
  if (!real && !c->kernel_family) NQ_FAIL(c, -4, "no wave field in QGModel");
  if (!(real ? launch_get_real<true>(c, *src, reinterpret_cast<double*>(scr), mode, zero_nyq) : launch_get_cplx(c, *src, scr, mul_ik)))
    NQ_FAIL(c, -2, "no row plan of length %d", c->N);
  HIPCHK(c, hipMemcpyAsync(out, scr, (real ? sizeof(double) : sizeof(cd)) * n, hipMemcpyDeviceToHost, c->stream));
  return nq_sync(c);
}

// Spectra the whole-plane calls of the class API need on a slab model (fft seam, the three Jacobians): the row kernel of
// the current state (or the rows uploaded by nq_slab_put_rows), exchange, column transform into a scratch column slab.
//   what 0 / 1: F[u q] / F[v q]                 half-spectrum slab (Kernel.py:471-486, QGModel.py:469-481)
//        2:     F[u phix + v phiy]              full-width slab, [0,0] as computed (Kernel.py:457-469)
//        3:     F[i phi q_psi]                  full-width slab (the refraction source, Kernel.py:332)
//        4:     F[Re i(phix* phiy - phiy* phix)] half-spectrum slab (CoupledModel.py:59-73)
//        5 / 6: forward transform of the real / complex rows last given to nq_slab_put_rows(0 / 1)
// Groups 0 and 2 are dead between steps, so the state is left alone.
int nq_slab_spectral(nq_ctx* c, int what) {
  if (!c) return -1;
  if (what < 0 || what > 6) NQ_FAIL(c, -1, "nq_slab_spectral: what = %d", what);
  std::vector<nq_ctx*> grp;
  SLABTRY(slab_group(c, &grp));
  for (nq_ctx* x : each(grp)) HIPCHK(x, hipSetDevice(x->device));
  SLABTRY(slab_settle(grp));
  nq_ctx* c0 = grp[0];
  const bool full = what == 2 || what == 3 || what == 6;
  if (full && !c0->kernel_family) NQ_FAIL(c, -4, "nq_slab_spectral: no wave field in QGModel");
  if (what == 4 && (c0->p.model != NQ_MODEL_COUPLED || c0->ybj)) NQ_FAIL(c, -4, "jacobian_phic_phi exists only in the coupled model");
  if (what <= 3 && !c0->have_q) NQ_FAIL(c, -4, "nq_slab_spectral: set_q has not been called");
  if ((what == 2 || what == 3 || what == 4) && !c0->have_phi) NQ_FAIL(c, -4, "nq_slab_spectral: set_phi has not been called");
  for (nq_ctx* x : each(grp)) {
    if (!x->scr_f1) {
      const size_t w = (size_t)(x->Wf > x->Ph ? x->Wf : x->Ph);
      ALLOC(x, x->scr_f1, (size_t)x->N * w);
    }
    set_window(x, 0, 1);
    if (what <= 1) launch_products(x);
    else if (what == 2) launch_products(x, 1.0, 0.0);
    else if (what == 3) launch_products(x, 0.0, 1.0);
    else if (what == 4) launch_wavepv(x);
  }
  SLABTRY(exchange_now(grp, what == 4 ? 2 : 0, true));
  for (nq_ctx* x : each(grp)) {
    const MArr& m = (what == 0 || what == 5) ? x->mUq : (what == 1 ? x->mVq : (what == 4 ? x->mB : x->mW));
    launch_A_m(x, false, {&m});
    if (full) launch_B_p(x, false, m.ys, m.pitch, x->scr_f1, x->Wf, x->Wf, 1.0);
    else if (x->Wh > 0) launch_B_p(x, false, m.ys, m.pitch, x->scr_f1, x->Ph, x->Wh, 1.0);
    HIPCHK(x, hipGetLastError());
    x->spec_kind = full ? 0 : 1;
  }
  for (nq_ctx* x : each(grp)) SLABTRY(nq_sync(x));
  return 0;
}
// this rank's column slab of the last nq_slab_spectral: (nx, wh) for the half-spectrum results, (nx, wf) for the others
int nq_slab_spectral_read(nq_ctx* c, int half, double* out) {
  if (!c || !out) return -1;
  if (c->spec_kind < 0) NQ_FAIL(c, -4, "nq_slab_spectral_read: nothing computed yet");
  if (c->spec_kind != (half ? 1 : 0)) NQ_FAIL(c, -1, "nq_slab_spectral_read: the last nq_slab_spectral result is a %s slab", c->spec_kind ? "half-spectrum" : "full-width");
  HIPCHK(c, hipSetDevice(c->device));
  const int w = half ? c->Wh : c->Wf, pitch = half ? c->Ph : c->Wf;
  if (w > 0) HIPCHK(c, hipMemcpy2DAsync(out, sizeof(cd) * w, c->scr_f1, sizeof(cd) * pitch, sizeof(cd) * w, c->N, hipMemcpyDeviceToHost, c->stream));
  return nq_sync(c);
}
// max |u|, max |v|, max |phi| over THIS rank's rows (the caller takes the max over ranks: Kernel._calc_cfl, Kernel.py:660-662)
int nq_slab_local_max(nq_ctx* c, double* out3) {
  if (!c || !out3) return -1;
  HIPCHK(c, hipSetDevice(c->device));
  cd* scr = nullptr;
  SLABTRY(rows_scratch(c, &scr));
  if (!c->diag_out) {
    ALLOC(c, c->diag_out, (size_t)40);
  }
  double* d = c->diag_out + 34;
  HIPCHK(c, hipMemsetAsync(d, 0, sizeof(double) * 3, c->stream));
  if (!launch_uv_max(c, reinterpret_cast<double*>(scr), d)) NQ_FAIL(c, -2, "no row plan of length %d", c->N);
  if (c->kernel_family) {
    launch_get_cplx(c, c->mPhi, scr, 0);
    hipLaunchKernelGGL(k_reduce, dim3((c->N + 255) / 256, c->Nloc), dim3(256), 0, c->stream, (const cd*)scr, c->N, c->N, c->N, 3, c->kk, c->ll, d + 2);
  }
  HIPCHK(c, hipMemcpyAsync(out3, d, sizeof(double) * 3, hipMemcpyDeviceToHost, c->stream));
  return nq_sync(c);
}
int nq_slab_counters(nq_ctx* c, double* out, int reset) {
  if (!c || !out) return -1;
  SLABTRY(nq_sync(c));
  if (c->mstream) HIPCHK(c, hipStreamSynchronize(c->mstream));
  float tot = 0.f;
  for (size_t i = 0; i + 1 < c->xev_used; i += 2) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, c->xev[i], c->xev[i + 1]) == hipSuccess) tot += ms;
  }
  out[0] = (double)c->n_calls;
  out[1] = (double)c->n_steps;
  out[2] = (double)c->n_exch;
  out[3] = c->bytes_sent;
  out[4] = (double)tot;
  out[5] = (double)effective_chunks(c);
  if (reset) {
    c->n_calls = c->n_steps = c->n_exch = 0;
    c->bytes_sent = 0.0;
    c->xev_used = 0;
    c->rev_used = 0;
    c->xtime = reset == 2;
  }
  return 0;
}
// milliseconds the exchange stream spent in all-reduces since timing was switched on (nq_slab_counters(reset = 2)), and
// how many were timed; read BEFORE the nq_slab_counters call that resets
int nq_slab_allreduce_ms(nq_ctx* c, double* out2) {
  if (!c || !out2) return -1;
  SLABTRY(nq_sync(c));
  float tot = 0.f;
  for (size_t i = 0; i + 1 < c->rev_used; i += 2) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, c->rev[i], c->rev[i + 1]) == hipSuccess) tot += ms;
  }
  out2[0] = (double)tot;
  out2[1] = (double)(c->rev_used / 2);
  return 0;
}


// ---- snapshots without stalling the stepper (ref niwqg/Saving.py:59-86: t, q, phi every tsave_snapshots steps) ---------
// nq_snapshot_begin: q = Re ifft(qh) (and phi = ifft(phih)) of the CURRENT state into device buffers of their own, on the
// context's stream; a second stream copies them to pinned host memory as soon as they are formed.  The caller may queue
// further steps at once.  nq_snapshot_end waits for that copy only and hands the arrays over.
int nq_snapshot_begin(nq_ctx* c, int with_phi) {
  NQ_SINGLE_RANK(c, "nq_snapshot_begin");
  if (with_phi && !c->kernel_family) NQ_FAIL(c, -4, "no wave field in QGModel");
  if (c->snap_busy) NQ_FAIL(c, -4, "nq_snapshot_begin: the previous snapshot has not been collected (nq_snapshot_end)");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t full = (size_t)c->N * c->N;
  // every resource is guarded by its own pointer: a call that failed half-way (a 4096^2 snapshot pins 128 + 256 MB of
  // host memory) leaves the rest to be made by the next call instead of running on null buffers
  if (!c->snap_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->snap_stream, hipStreamNonBlocking));
  if (!c->ev_snap) HIPCHK(c, hipEventCreateWithFlags(&c->ev_snap, hipEventDisableTiming));
  if (!c->snap_q) ALLOC(c, c->snap_q, full);
  if (!c->snap_hq) HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&c->snap_hq), sizeof(double) * full, hipHostMallocDefault));
  if (with_phi) {
    if (!c->snap_phi) ALLOC(c, c->snap_phi, full);
    if (!c->snap_hphi) HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&c->snap_hphi), sizeof(cd) * full, hipHostMallocDefault));
  }
  const cd* qh = c->q.y[c->q.cur];
  SLABTRY(mean_qh(c, &qh));
  inv2d_half(c, qh, c->snap_q, c->scr_h0);
  if (with_phi) launch_x_c2c(c, true, c->mPhi.xs, c->snap_phi, c->mPhi.pitch, c->N, 1.0);
  HIPCHK(c, hipEventRecord(c->ev_snap, c->stream));
  HIPCHK(c, hipStreamWaitEvent(c->snap_stream, c->ev_snap, 0));
  HIPCHK(c, hipMemcpyAsync(c->snap_hq, c->snap_q, sizeof(double) * full, hipMemcpyDeviceToHost, c->snap_stream));
  if (with_phi) HIPCHK(c, hipMemcpyAsync(c->snap_hphi, c->snap_phi, sizeof(cd) * full, hipMemcpyDeviceToHost, c->snap_stream));
  c->snap_busy = true;
  HIPCHK(c, hipGetLastError());
  return 0;
}
int nq_snapshot_end(nq_ctx* c, double* q_out, double* phi_out) {
  NQ_SINGLE_RANK(c, "nq_snapshot_end");
  if (!c->snap_busy) NQ_FAIL(c, -4, "nq_snapshot_end: no snapshot in flight");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->snap_stream));
  const size_t full = (size_t)c->N * c->N;
  if (q_out) memcpy(q_out, c->snap_hq, sizeof(double) * full);
  if (phi_out) {
    if (!c->snap_hphi) NQ_FAIL(c, -4, "nq_snapshot_end: the snapshot was taken without phi");
    memcpy(phi_out, c->snap_hphi, sizeof(cd) * full);
  }
  c->snap_busy = false;
  return 0;
}

// host copies of the blocks that are summed over ranks (nq_reduce_buffer): what a callback link reduces
int nq_reduce_read(nq_ctx* c, int which, double* host_out) {
  if (!c || !host_out) return -1;
  int n = 0;
  double* p = red_ptr(c, which, &n);
  if (!p) NQ_FAIL(c, -1, "nq_reduce_read: block %d does not exist (yet)", which);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(host_out, p, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
  return nq_sync(c);
}
int nq_reduce_write(nq_ctx* c, int which, const double* host_in) {
  if (!c || !host_in) return -1;
  int n = 0;
  double* p = red_ptr(c, which, &n);
  if (!p) NQ_FAIL(c, -1, "nq_reduce_write: block %d does not exist (yet)", which);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(p, host_in, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
  return nq_sync(c);
}

// ---- FFT seam ----------------------------------------------------------------------------------
int nq_fft2(nq_ctx* c, const double* in, double* out) {
  if (!c || !in || !out) return -1;
  NQ_SINGLE_RANK(c, "nq_fft2");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t full = (size_t)c->N * c->N;
  HIPCHK(c, hipMemcpyAsync(c->scr_f0, in, sizeof(cd) * full, hipMemcpyHostToDevice, c->stream));
  fwd2d_full(c, c->scr_f0, c->scr_f0, c->scr_f1);
  HIPCHK(c, hipMemcpyAsync(out, c->scr_f0, sizeof(cd) * full, hipMemcpyDeviceToHost, c->stream));
  return nq_sync(c);
}
int nq_ifft2(nq_ctx* c, const double* in, double* out) {
  if (!c || !in || !out) return -1;
  NQ_SINGLE_RANK(c, "nq_ifft2");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t full = (size_t)c->N * c->N;
  HIPCHK(c, hipMemcpyAsync(c->scr_f0, in, sizeof(cd) * full, hipMemcpyHostToDevice, c->stream));
  inv2d_full(c, c->scr_f0, c->scr_f0, c->scr_f1);
  HIPCHK(c, hipMemcpyAsync(out, c->scr_f0, sizeof(cd) * full, hipMemcpyDeviceToHost, c->stream));
  return nq_sync(c);
}
int nq_rfft2(nq_ctx* c, const double* in, double* out) {
  if (!c || !in || !out) return -1;
  NQ_SINGLE_RANK(c, "nq_rfft2");
  HIPCHK(c, hipSetDevice(c->device));
  const int N = c->N;
  HIPCHK(c, hipMemcpyAsync(c->scr_r, in, sizeof(double) * (size_t)N * N, hipMemcpyHostToDevice, c->stream));
  fwd2d_half(c, c->scr_r, c->scr_h1, c->scr_h0);
  HIPCHK(c, hipMemcpy2DAsync(out, sizeof(cd) * c->Wh, c->scr_h1, sizeof(cd) * c->Ph, sizeof(cd) * c->Wh, N, hipMemcpyDeviceToHost, c->stream));
  return nq_sync(c);
}
int nq_irfft2(nq_ctx* c, const double* in, double* out) {
  if (!c || !in || !out) return -1;
  NQ_SINGLE_RANK(c, "nq_irfft2");
  HIPCHK(c, hipSetDevice(c->device));
  const int N = c->N;
  HIPCHK(c, hipMemcpy2DAsync(c->scr_h1, sizeof(cd) * c->Ph, in, sizeof(cd) * c->Wh, sizeof(cd) * c->Wh, N, hipMemcpyHostToDevice, c->stream));
  inv2d_half(c, c->scr_h1, c->scr_r, c->scr_h0);
  HIPCHK(c, hipMemcpyAsync(out, c->scr_r, sizeof(double) * (size_t)N * N, hipMemcpyDeviceToHost, c->stream));
  return nq_sync(c);
}

// ---- downloads ---------------------------------------------------------------------------------
static int get_half_spec(nq_ctx* c, const cd* dev, double* host) {
  HIPCHK(c, hipMemcpy2DAsync(host, sizeof(cd) * c->Wh, dev, sizeof(cd) * c->Ph, sizeof(cd) * c->Wh, c->N, hipMemcpyDeviceToHost, c->stream));
  return nq_sync(c);
}
static int get_real_from_half(nq_ctx* c, const cd* spec, int mul_mode, double* host) {
  const size_t full = (size_t)c->N * c->N;
  const cd* src = spec;
  if (mul_mode) {
    hipLaunchKernelGGL(k_spec_mul, dim3((c->Wh + 63) / 64, c->N), dim3(64), 0, c->stream, spec, c->scr_h1, c->Wh, c->Ph, mul_mode, c->kk, c->ll, c->N, c->kernel_family ? 1 : 0);
    src = c->scr_h1;
  }
  inv2d_half(c, src, c->scr_r, c->scr_h0);
  HIPCHK(c, hipMemcpyAsync(host, c->scr_r, sizeof(double) * full, hipMemcpyDeviceToHost, c->stream));
  return nq_sync(c);
}

int nq_get_field(nq_ctx* c, int id, double* host) {
  if (!c || !host) return -1;
  NQ_SINGLE_RANK(c, "nq_get_field");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t full = (size_t)c->N * c->N;
  const cd* qh = c->q.y[c->q.cur];
  const bool waves = c->kernel_family;
  switch (id) {
    case NQ_F_QH: return get_half_spec(c, qh, host);
    case NQ_F_QH_MINUS:
      if (!c->dual) NQ_FAIL(c, -4, "NQ_F_QH_MINUS needs a dual_q context");
      return get_half_spec(c, c->q2.y[c->q2.cur], host);
    case NQ_F_PH: return get_half_spec(c, c->ph, host);
    case NQ_F_CH:
      if (!c->passive) NQ_FAIL(c, -4, "no passive scalar in this context");
      return get_half_spec(c, c->cq.y[c->cq.cur], host);
    case NQ_F_QH_STAGE4: return get_half_spec(c, c->q.y[(c->q.cur + 2) % 3], host);
    case NQ_F_QH_MINUS_STAGE4:
      if (!c->dual) NQ_FAIL(c, -4, "NQ_F_QH_MINUS_STAGE4 needs a dual_q context");
      return get_half_spec(c, c->q2.y[(c->q2.cur + 2) % 3], host);
    case NQ_F_PHIH_STAGE4:
      if (!waves) NQ_FAIL(c, -4, "no wave field in QGModel");
      HIPCHK(c, hipMemcpyAsync(host, c->w.y[(c->w.cur + 2) % 3], sizeof(cd) * full, hipMemcpyDeviceToHost, c->stream));
      return nq_sync(c);
    case NQ_F_QH_TICK: case NQ_F_QH_MINUS_TICK: case NQ_F_QWH_TICK: {
      const cd* src = id == NQ_F_QH_TICK ? c->tick_qh : (id == NQ_F_QH_MINUS_TICK ? c->tick_q2 : c->tick_qwh);
      if (!src) NQ_FAIL(c, -4, "field %d: no nq_tick_snapshot yet (or no such plane in this context)", id);
      return get_half_spec(c, src, host);
    }
    case NQ_F_PHIH_TICK:
      if (!c->tick_w) NQ_FAIL(c, -4, "NQ_F_PHIH_TICK: no nq_tick_snapshot yet (or no wave field)");
      HIPCHK(c, hipMemcpyAsync(host, c->tick_w, sizeof(cd) * full, hipMemcpyDeviceToHost, c->stream));
      return nq_sync(c);
    case NQ_F_C:
      if (!c->passive) NQ_FAIL(c, -4, "no passive scalar in this context");
      return get_real_from_half(c, c->cq.y[c->cq.cur], 0, host);
    case NQ_F_QWH:
      if (c->p.model != NQ_MODEL_COUPLED) NQ_FAIL(c, -4, "qwh exists only in the coupled model");
      return get_half_spec(c, c->qwh, host);
    case NQ_F_Q:
      SLABTRY(mean_qh(c, &qh));
      return get_real_from_half(c, qh, 0, host);
    case NQ_F_QPSI: {
      const cd* src = qh;
      SLABTRY(mean_qh(c, &src));
      if (c->p.model == NQ_MODEL_COUPLED && !c->ybj) {
        hipLaunchKernelGGL(k_sub_half, dim3((c->Wh + 63) / 64, c->N), dim3(64), 0, c->stream, src, (const cd*)c->qwh, c->scr_f1, c->Wh, c->Ph);
        src = c->scr_f1;
      }
      return get_real_from_half(c, src, 0, host);
    }
    case NQ_F_P: return get_real_from_half(c, c->ph, 0, host);
    case NQ_F_U: return get_real_from_half(c, c->ph, 1, host);
    case NQ_F_V: {
      // v = Re ifft(ik psi): psi must be Hermitian-projected on the Nyquist column first;
      // equivalently its k = N/2 column does not contribute for the Kernel family.
      hipLaunchKernelGGL(k_spec_mul, dim3((c->Wh + 63) / 64, c->N), dim3(64), 0, c->stream, c->ph, c->scr_h1, c->Wh, c->Ph, 2, c->kk, c->ll, c->N, 1);
      if (c->kernel_family) HIPCHK(c, hipMemset2DAsync(c->scr_h1 + c->N / 2, sizeof(cd) * c->Ph, 0, sizeof(cd), c->N, c->stream));
      inv2d_half(c, c->scr_h1, c->scr_r, c->scr_h0);
      HIPCHK(c, hipMemcpyAsync(host, c->scr_r, sizeof(double) * full, hipMemcpyDeviceToHost, c->stream));
      return nq_sync(c);
    }
    case NQ_F_QW:
      if (c->p.model != NQ_MODEL_COUPLED) NQ_FAIL(c, -4, "qw exists only in the coupled model");
      return get_real_from_half(c, c->qwh, 0, host);
    case NQ_F_PHIH:
      if (!waves) NQ_FAIL(c, -4, "no wave field in QGModel");
      HIPCHK(c, hipMemcpyAsync(host, c->w.y[c->w.cur], sizeof(cd) * full, hipMemcpyDeviceToHost, c->stream));
      return nq_sync(c);
    case NQ_F_PHI:
      if (!waves) NQ_FAIL(c, -4, "no wave field in QGModel");
      launch_x_c2c(c, true, c->mPhi.xs, c->scr_f0, c->mPhi.pitch, c->N, 1.0);
      HIPCHK(c, hipMemcpyAsync(host, c->scr_f0, sizeof(cd) * full, hipMemcpyDeviceToHost, c->stream));
      return nq_sync(c);
    case NQ_F_PHIX:
    case NQ_F_PHIY: {
      if (!waves) NQ_FAIL(c, -4, "no wave field in QGModel");
      const bool unc = c->p.model == NQ_MODEL_UNCOUPLED;
      (void)unc;
      const MArr& src = (id == NQ_F_PHIX) ? c->mGx : c->mGy;       // == mPhi/mPhiy unless UnCoupled
      launch_x_c2c(c, true, src.xs, c->scr_f0, src.pitch, c->N, 1.0, id == NQ_F_PHIX ? 1 : 0);
      HIPCHK(c, hipMemcpyAsync(host, c->scr_f0, sizeof(cd) * full, hipMemcpyDeviceToHost, c->stream));
      return nq_sync(c);
    }
    default: NQ_FAIL(c, -1, "nq_get_field: unknown field id %d", id);
  }
}

// the anti-Hermitian passenger of qh on row l = N/2 (k_s_q): this context's local half-spectrum columns, zeros where there is none
int nq_get_qh_passenger(nq_ctx* c, double* out_cplx) {
  if (!c || !out_cplx) return -1;
  HIPCHK(c, hipSetDevice(c->device));
  memset(out_cplx, 0, sizeof(cd) * (size_t)(c->Wh > 0 ? c->Wh : 0));
  if (c->pass && c->Wh > 0) {
    HIPCHK(c, hipMemcpyAsync(out_cplx, c->qp.y[c->qp.cur], sizeof(cd) * (size_t)c->Wh, hipMemcpyDeviceToHost, c->stream));
    return nq_sync(c);
  }
  return 0;
}

int nq_get_scalar(nq_ctx* c, int id, double* out) {
  if (!c || !out) return -1;
  HIPCHK(c, hipSetDevice(c->device));
  const int N = c->N;
  const double M = (double)N * N;
  // scratch of the reductions: d[0..1] the results, d[2 ..] one partial-sum slot per workgroup of k_reduce, at most
  // ceil(N / 256) * N doubles.  scr_h0 holds N * Ph complex entries (2 N (N/2 + 1) doubles) on a single rank; the 64-entry
  // allocation of a slab rank is never reached, the sums sit behind NQ_SINGLE_RANK below
  double* d = reinterpret_cast<double*>(c->scr_h0);
  double h[2] = {0, 0};
  HIPCHK(c, hipMemsetAsync(d, 0, sizeof(double) * 2, c->stream));
  if (id == NQ_S_KE || id == NQ_S_PW || id == NQ_S_KW) {
    // increment accumulated by nq_step since the last read; reading resets it
    if (!c->bud) NQ_FAIL(c, -4, "budgets are disabled in this context");
    HIPCHK(c, hipMemcpyAsync(h, c->acc + id, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemsetAsync(c->acc + id, 0, sizeof(double), c->stream));
    int rc = nq_sync(c);
    *out = h[0];
    return rc;
  }
  NQ_SINGLE_RANK(c, "nq_get_scalar (ids other than the budget increments)");
  if (id == NQ_S_KE_QG) {
    hipLaunchKernelGGL(k_reduce, dim3((c->Wh + 255) / 256, N), dim3(256), 0, c->stream, c->ph, c->Wh, c->Ph, N, c->kernel_family ? 4 : 1, c->kk, c->ll, d, d + 2);
    hipLaunchKernelGGL(k_sum_slots, dim3(1), dim3(256), 0, c->stream, d + 2, ((c->Wh + 255) / 256) * N, d);
    HIPCHK(c, hipMemcpyAsync(h, d, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    int rc = nq_sync(c);
    *out = 0.5 * h[0] / (M * M);
    return rc;
  }
  if (!c->kernel_family && id == NQ_S_CFL) {
    const size_t full = (size_t)N * N;
    for (int which = 0; which < 2; ++which) {        // QGModel._calc_cfl: literal irfft2 (QGModel.py:621-629)
      hipLaunchKernelGGL(k_spec_mul, dim3((c->Wh + 63) / 64, N), dim3(64), 0, c->stream, c->ph, c->scr_h1, c->Wh, c->Ph, which == 0 ? 1 : 2, c->kk, c->ll, N, 0);
      inv2d_half(c, c->scr_h1, c->scr_r, c->scr_f1);
      hipLaunchKernelGGL(k_reduce_real_max, dim3(1024), dim3(256), 0, c->stream, c->scr_r, full, d);
    }
    HIPCHK(c, hipMemcpyAsync(h, d, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    int rc = nq_sync(c);
    *out = h[0];
    return rc;
  }
  if (!c->kernel_family) NQ_FAIL(c, -4, "scalar %d needs the wave field", id);
  const cd* phih = c->w.y[c->w.cur];
  if (id == NQ_S_KE_NIW || id == NQ_S_PE_NIW) {
    hipLaunchKernelGGL(k_reduce, dim3((N + 255) / 256, N), dim3(256), 0, c->stream, phih, N, N, N, id == NQ_S_KE_NIW ? 0 : 2, c->kk, c->ll, d, d + 2);
    hipLaunchKernelGGL(k_sum_slots, dim3(1), dim3(256), 0, c->stream, d + 2, ((N + 255) / 256) * N, d);
    HIPCHK(c, hipMemcpyAsync(h, d, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    int rc = nq_sync(c);
    *out = (id == NQ_S_KE_NIW) ? 0.5 * h[0] / (M * M) : 0.25 * h[0] / (M * M) / c->p.kappa2;
    return rc;
  }
  if (id == NQ_S_CFL || id == NQ_S_MAX_PHI) {
    // max(|u|, |v|, |phi|) on the device (the caller multiplies by dt/dx): ref Kernel.py:660-662; NQ_S_MAX_PHI: max |phi| alone
    const size_t full = (size_t)N * N;
    for (int which = 0; which < (id == NQ_S_CFL ? 2 : 0); ++which) {
      hipLaunchKernelGGL(k_spec_mul, dim3((c->Wh + 63) / 64, N), dim3(64), 0, c->stream, c->ph, c->scr_h1, c->Wh, c->Ph, which == 0 ? 1 : 2, c->kk, c->ll, N, 1);
      if (which == 1 && c->kernel_family) HIPCHK(c, hipMemset2DAsync(c->scr_h1 + N / 2, sizeof(cd) * c->Ph, 0, sizeof(cd), N, c->stream));
      inv2d_half(c, c->scr_h1, c->scr_r, c->scr_f1);
      hipLaunchKernelGGL(k_reduce_real_max, dim3(1024), dim3(256), 0, c->stream, c->scr_r, full, d);
    }
    launch_x_c2c(c, true, c->mPhi.xs, c->scr_f0, c->mPhi.pitch, N, 1.0);
    hipLaunchKernelGGL(k_reduce, dim3((N + 255) / 256, N), dim3(256), 0, c->stream, c->scr_f0, N, N, N, 3, c->kk, c->ll, d);
    HIPCHK(c, hipMemcpyAsync(h, d, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    int rc = nq_sync(c);
    *out = h[0];
    return rc;
  }
  NQ_FAIL(c, -1, "nq_get_scalar: id %d not available", id);
}

// overwrite the entries nq_coeff_patch recorded for public equation eq in one set of coefficient planes
static void apply_coeff_patch(nq_ctx* c, int eq, int width, int pitch, int k0, const double* filt, cd* const* coef, bool mirrored) {
  const nq_ctx::CoefPatch& pt = c->patch[eq];
  if (pt.n == 0 || width == 0) return;
  hipLaunchKernelGGL(k_coeff_patch, dim3((pt.n + 255) / 256), dim3(256), 0, c->stream, pt.n, pt.l, pt.k, pt.v, width, pitch, k0, filt,
                     coef[2], coef[3], coef[4], coef[5], mirrored ? c->N : 0);
}

int nq_get_coeff(nq_ctx* c, int eq, int which, double* out) {
  if (!c || !out || which < 0 || which > 5 || eq < 0 || eq > 2) return -1;
  NQ_SINGLE_RANK(c, "nq_get_coeff");
  if (eq == 1 && !c->kernel_family) NQ_FAIL(c, -4, "no phi equation in QGModel");
  if (eq == 2 && !c->passive) NQ_FAIL(c, -4, "no passive scalar in this context");
  HIPCHK(c, hipSetDevice(c->device));
  const int N = c->N;
  const bool half = eq != 1;
  const int width = half ? c->Wh : N, pitch = half ? c->Ph : N;
  const size_t cnt = (size_t)N * pitch;
  cd* tmp[6];
  void* blockp = nullptr;                               // one allocation: nothing to leak when it fails
  HIPCHK(c, hipMalloc(&blockp, 6 * cnt * sizeof(cd)));
  for (int i = 0; i < 6; ++i) tmp[i] = reinterpret_cast<cd*>(blockp) + (size_t)i * cnt;
  const int e = eq == 2 ? 3 : (half ? (c->kernel_family ? 0 : 2) : 1);
  hipLaunchKernelGGL(k_etdrk4_coeffs, dim3((width + 63) / 64, N), dim3(64), 0, c->stream, e, N, width, pitch, 0, c->p, c->kk, c->ll, (const double*)nullptr, c->contour, tmp[0], tmp[1], tmp[2], tmp[3], tmp[4], tmp[5]);
  apply_coeff_patch(c, eq, width, pitch, 0, nullptr, tmp, false);
  hipError_t er = hipMemcpy2DAsync(out, sizeof(cd) * width, tmp[which], sizeof(cd) * pitch, sizeof(cd) * width, N, hipMemcpyDeviceToHost, c->stream);
  int rc = nq_sync(c);
  (void)hipFree(blockp);
  if (er != hipSuccess) NQ_FAIL(c, -5, "nq_get_coeff: copy failed");
  return rc;
}

// public eq (0: q, 1: phi, 2: QGModel's passive scalar) -> k_etdrk4_coeffs' operator code, local width and first column
static int coeff_eq(nq_ctx* c, int eq, const char* what, int* code, int* width, int* k0) {
  if (!c) NQ_FAIL((nq_ctx*)nullptr, -1, "%s: null context", what);
  if (eq < 0 || eq > 2) NQ_FAIL(c, -1, "%s: eq %d (0: q, 1: phi, 2: passive scalar)", what, eq);
  if (eq == 1 && !c->kernel_family) NQ_FAIL(c, -4, "%s: no phi equation in QGModel", what);
  if (eq == 2 && !c->passive) NQ_FAIL(c, -4, "%s: no passive scalar in this context", what);
  *code = eq == 2 ? 3 : (eq == 1 ? 1 : (c->kernel_family ? 0 : 2));
  *width = eq == 1 ? c->Wf : c->Wh;
  *k0 = eq == 1 ? c->kf0 : c->kh0;
  return 0;
}

int nq_coeff_near_contour(nq_ctx* c, int eq, double delta, int cap, int* l_out, int* k_out) {
  int code, width, k0;
  if (int rc = coeff_eq(c, eq, "nq_coeff_near_contour", &code, &width, &k0)) return rc;
  if (!(delta >= 0.0) || cap < 0 || (cap > 0 && (!l_out || !k_out))) NQ_FAIL(c, -1, "nq_coeff_near_contour: bad delta / cap / outputs");
  HIPCHK(c, hipSetDevice(c->device));
  if (width == 0) return 0;
  int* d = nullptr;                                     // [count | l (cap) | k (cap)]
  HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&d), sizeof(int) * (1 + 2 * (size_t)cap)));
  hipError_t er = hipMemsetAsync(d, 0, sizeof(int), c->stream);
  hipLaunchKernelGGL(k_coeff_flag, dim3((width + 63) / 64, c->N), dim3(64), 0, c->stream, code, c->N, width, k0, c->p, c->kk, c->ll,
                     c->contour, delta * delta, cap, d, d + 1, d + 1 + cap);
  int n = 0;
  if (er == hipSuccess) er = hipMemcpyAsync(&n, d, sizeof(int), hipMemcpyDeviceToHost, c->stream);
  if (er == hipSuccess) er = hipStreamSynchronize(c->stream);
  const int got = n < cap ? n : cap;
  if (er == hipSuccess && got > 0) er = hipMemcpy(l_out, d + 1, sizeof(int) * got, hipMemcpyDeviceToHost);
  if (er == hipSuccess && got > 0) er = hipMemcpy(k_out, d + 1 + cap, sizeof(int) * got, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (er != hipSuccess) NQ_FAIL(c, -5, "nq_coeff_near_contour: %s", hipGetErrorString(er));
  return n;
}

int nq_coeff_patch(nq_ctx* c, int eq, int n, const int* l, const int* k, const double* vals) {
  int code, width, k0;
  if (int rc = coeff_eq(c, eq, "nq_coeff_patch", &code, &width, &k0)) return rc;
  if (n < 0 || (n > 0 && (!l || !k || !vals))) NQ_FAIL(c, -1, "nq_coeff_patch: bad arguments");
  for (int i = 0; i < n; ++i)
    if (l[i] < 0 || l[i] >= c->N || k[i] < k0 || k[i] >= k0 + width)
      NQ_FAIL(c, -1, "nq_coeff_patch: entry %d = (l %d, k %d) outside this context's columns [%d, %d)", i, l[i], k[i], k0, k0 + width);
  HIPCHK(c, hipSetDevice(c->device));
  nq_ctx::CoefPatch& pt = c->patch[eq];
  HIPCHK(c, hipStreamSynchronize(c->stream));           // a previous patch may still be read by a queued kernel
  (void)hipFree(pt.l); (void)hipFree(pt.k); (void)hipFree(pt.v);
  pt = nq_ctx::CoefPatch();
  if (n == 0) return 0;
  HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&pt.l), sizeof(int) * n));
  HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&pt.k), sizeof(int) * n));
  HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&pt.v), sizeof(cd) * 4 * (size_t)n));
  HIPCHK(c, hipMemcpy(pt.l, l, sizeof(int) * n, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(pt.k, k, sizeof(int) * n, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(pt.v, vals, sizeof(cd) * 4 * (size_t)n, hipMemcpyHostToDevice));
  pt.n = n;
  if (eq == 0) {
    apply_coeff_patch(c, 0, c->Wh, c->Ph, c->kh0, c->filt_h, c->q.coef, c->cmirror != 0);
    if (c->dual) apply_coeff_patch(c, 0, c->Wh, c->Ph, c->kh0, nullptr, c->coefu, c->cmirror != 0);
  } else if (eq == 1) {
    apply_coeff_patch(c, 1, c->Wf, c->Wf, c->kf0, c->filt_f, c->w.coef, c->cmirror != 0);
  } else {
    apply_coeff_patch(c, 2, c->Wh, c->Ph, c->kh0, c->filt_h, c->cq.coef, c->cmirror != 0);
  }
  return nq_sync(c);
}

// ---- the three Jacobians of the public API, in the reference's own array layouts ------------------------------
// F[u q], F[v q] of the current state as two half-spectrum planes in scr_h0, scr_h1
static void products_to_scratch(nq_ctx* c) {
  launch_products(c);
  launch_A_m(c, false, {&c->mUq, &c->mVq});
  launch_B_p(c, false, c->mUq.ys, c->mUq.pitch, c->scr_h0, c->Ph, c->Wh, 1.0);
  launch_B_p(c, false, c->mVq.ys, c->mVq.pitch, c->scr_h1, c->Ph, c->Wh, 1.0);
}
// Kernel.jacobian_psi_q (ref Kernel.py:471-486): ik*fft(u q) + il*fft(v q) as the full (ny, nx) plane, [0,0] = 0;
// QGModel.jacobian_psi_q (ref QGModel.py:469-481): the same on (ny, nx/2+1), [0,0] kept.
int nq_jacobian_psi_q(nq_ctx* c, double* out_cplx) {
  NQ_SINGLE_RANK(c, "nq_jacobian_psi_q");
  if (!out_cplx) NQ_FAIL(c, -1, "nq_jacobian_psi_q: null output");
  HIPCHK(c, hipSetDevice(c->device));
  products_to_scratch(c);
  const int N = c->N, wout = c->kernel_family ? N : c->WhG;
  hipLaunchKernelGGL(k_expand_half, dim3((wout + 63) / 64, N), dim3(64), 0, c->stream, (const cd*)c->scr_h0, (const cd*)c->scr_h1, c->scr_f0, N, c->Ph, wout, 1, c->kk, c->ll);
  if (c->kernel_family) HIPCHK(c, hipMemsetAsync(c->scr_f0, 0, sizeof(cd), c->stream));
  HIPCHK(c, hipMemcpyAsync(out_cplx, c->scr_f0, sizeof(cd) * (size_t)N * wout, hipMemcpyDeviceToHost, c->stream));
  return nq_sync(c);
}
// QGModel.jacobian_psi_c (ref QGModel.py:483-495): ik*fft(u c) + il*fft(v c) on (ny, nx/2+1), with u, v of the current psi;
// formed by the row kernel exactly as inside a step (the scalar rides paired with q, its products leave as a second pair)
int nq_jacobian_psi_c(nq_ctx* c, double* out_cplx) {
  NQ_SINGLE_RANK(c, "nq_jacobian_psi_c");
  if (!out_cplx) NQ_FAIL(c, -1, "nq_jacobian_psi_c: null output");
  if (!c->passive) NQ_FAIL(c, -4, "nq_jacobian_psi_c: this context has no passive scalar");
  HIPCHK(c, hipSetDevice(c->device));
  launch_products(c);
  launch_A_m(c, false, {&c->mUc, &c->mVc});
  launch_B_p(c, false, c->mUc.ys, c->mUc.pitch, c->scr_h0, c->Ph, c->Wh, 1.0);
  launch_B_p(c, false, c->mVc.ys, c->mVc.pitch, c->scr_h1, c->Ph, c->Wh, 1.0);
  const int N = c->N, wout = c->WhG;
  hipLaunchKernelGGL(k_expand_half, dim3((wout + 63) / 64, N), dim3(64), 0, c->stream, (const cd*)c->scr_h0, (const cd*)c->scr_h1, c->scr_f0, N, c->Ph, wout, 1, c->kk, c->ll);
  HIPCHK(c, hipMemcpyAsync(out_cplx, c->scr_f0, sizeof(cd) * (size_t)N * wout, hipMemcpyDeviceToHost, c->stream));
  return nq_sync(c);
}
// the two transforms themselves, (2, ny, nx/2+1): fft(u q) then fft(v q) restricted to k = 0..nx/2 (no reference
// counterpart: exported for tests and for callers that assemble their own flux forms)
int nq_products_uq_vq(nq_ctx* c, double* out_cplx) {
  NQ_SINGLE_RANK(c, "nq_products_uq_vq");
  if (!out_cplx) NQ_FAIL(c, -1, "nq_products_uq_vq: null output");
  HIPCHK(c, hipSetDevice(c->device));
  products_to_scratch(c);
  int rc = get_half_spec(c, c->scr_h0, out_cplx);
  if (rc) return rc;
  return get_half_spec(c, c->scr_h1, out_cplx + 2 * (size_t)c->N * c->Wh);
}
// Kernel.jacobian_psi_phi (ref Kernel.py:457-469): fft(u phix + v phiy), (ny, nx), [0,0] = 0.  YBJModel's own version
// (ref YBJModel.py:123-133) keeps [0,0], and so does a YBJ context.
int nq_jacobian_psi_phi(nq_ctx* c, double* out_cplx) {
  NQ_SINGLE_RANK(c, "nq_jacobian_psi_phi");
  if (!out_cplx) NQ_FAIL(c, -1, "nq_jacobian_psi_phi: null output");
  if (!c->kernel_family) NQ_FAIL(c, -4, "no wave field in QGModel");
  HIPCHK(c, hipSetDevice(c->device));
  launch_products(c, 1.0, 0.0);                       // the Jacobian part alone
  launch_A_m(c, false, {&c->mW});
  launch_B_p(c, false, c->mW.ys, c->mW.pitch, c->scr_f0, c->N, c->N, 1.0);
  if (!c->ybj) HIPCHK(c, hipMemsetAsync(c->scr_f0, 0, sizeof(cd), c->stream));
  HIPCHK(c, hipMemcpyAsync(out_cplx, c->scr_f0, sizeof(cd) * (size_t)c->N * c->N, hipMemcpyDeviceToHost, c->stream));
  return nq_sync(c);
}
// ---- diagnostics tick on the device (ref Diagnostics.py:41-58, Kernel.py:613-706, :718-868, CoupledModel.py:99-136) --
// One body per tick call (this one, tick_binned and tick_transfer below), written for a group of contexts: a slab entry
// hands over slab_group's contexts, a single-rank entry a group of just its own.  For that group of one exchange_now and
// slab_allreduce return at once and slab_settle finds nothing pending, so a plain context gets no exchange stream and its
// link stays LINK_NONE.  fn: the public function that was called, for the messages.
static int tick_need_phi(std::vector<nq_ctx*>& grp, const char* fn) {
  for (nq_ctx* x : grp)
    if (x->kernel_family && !x->have_phi) NQ_FAIL(x, -4, "%s: set_phi has not been called", fn);
  return 0;
}
// the 32 sums of include/niwqg_amd.h, every rank's part summed over the ranks (two all-reduces: the spectral half gives the
// two means the physical half is centred with)
static int tick_scalar(std::vector<nq_ctx*>& grp, double* out) {
  SLABTRY(slab_settle(grp));
  nq_ctx* c0 = grp[0];
  const int N = c0->N, NB = 1024;
  const double M = (double)N * N;
  const bool waves = c0->kernel_family, coupled = c0->p.model == NQ_MODEL_COUPLED;
  // spectral sums: [0,4) S0..S3, [4,6) phih[0,0], [6,15) the nine half-spectrum sums, [15] Re(qh - qwh)[0,0]
  for (nq_ctx* x : each(grp)) {
    const int nxb = xdiag_blocks(x), nww = (x->Wf / x->CLy) * x->S2;
    if (!x->diag_part) {
      size_t need = (size_t)NB * 9;
      if ((size_t)nxb * 8 > need) need = (size_t)nxb * 8;
      if ((size_t)nww * 4 > need) need = (size_t)nww * 4;
      ALLOC(x, x->diag_part, need);
      ALLOC(x, x->diag_out, (size_t)40);
    }
    double* d = x->diag_out;
    HIPCHK(x, hipMemsetAsync(d, 0, sizeof(double) * 40, x->stream));
    const cd* qh = x->q.y[x->q.cur];
    SLABTRY(mean_qh(x, &qh));
    if (waves) {
      const cd* phih = x->w.y[x->w.cur];
      hipLaunchKernelGGL(k_diag_phi, dim3(NB), dim3(256), 0, x->stream, phih, N, x->Wf, x->Wf, x->kf0, x->kk, x->ll, x->diag_part);
      hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(1024), 0, x->stream, x->diag_part, NB, 4, 4, d);
      if (x->kf0 == 0) HIPCHK(x, hipMemcpyAsync(d + 4, phih, sizeof(cd), hipMemcpyDeviceToDevice, x->stream));
    }
    if (x->Wh > 0) {
      hipLaunchKernelGGL(k_diag_q, dim3(NB), dim3(256), 0, x->stream, qh, (const cd*)(coupled ? x->qwh : nullptr), (const cd*)x->ph, N, x->Wh, x->Ph, x->kh0, x->kk, x->ll, x->diag_part,
                         (const cd*)(x->dual ? x->q.y[x->q.cur] : nullptr), (const cd*)(x->dual ? x->q2.y[x->q2.cur] : nullptr),
                         (const double*)(x->dual ? x->filt_h : nullptr), (const double*)(x->dual ? x->filt_m : nullptr),
                         (const cd*)(x->pass ? x->qp.y[x->qp.cur] : nullptr));
      hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(1024), 0, x->stream, x->diag_part, NB, 9, 9, d + 6);
    }
    if (x->kh0 == 0) {                              // [15] <- Re(qh - qwh)[0,0] (the owner of column 0 contributes it)
      HIPCHK(x, hipMemcpyAsync(d + 15, qh, sizeof(double), hipMemcpyDeviceToDevice, x->stream));
      if (coupled) {
        HIPCHK(x, hipMemcpyAsync(d + 32, x->qwh, sizeof(double), hipMemcpyDeviceToDevice, x->stream));
        hipLaunchKernelGGL(k_axpy1, dim3(1), dim3(1), 0, x->stream, d + 15, d + 32, -1.0);
      }
    }
  }
  SLABTRY(slab_allreduce(grp, 4));
  double h[16];
  HIPCHK(c0, hipSetDevice(c0->device));
  HIPCHK(c0, hipMemcpyAsync(h, c0->diag_out, sizeof(double) * 16, hipMemcpyDeviceToHost, c0->stream));
  SLABTRY(nq_sync(c0));
  for (int i = 0; i < 15; ++i) out[i] = h[i];
  for (int i = 15; i < 32; ++i) out[i] = 0.0;
  const double qbar = h[15] / M, abar = h[0] / (M * M);
  out[15] = qbar;
  if (!waves && c0->passive) {
    // QGModel's passive scalar (ref QGModel.py:724-737, :595-604): [16..19] the four |c-hat|^2 sums, [20] the Gamma_c projection
    for (nq_ctx* x : each(grp)) {
      const cd* ch = x->cq.y[x->cq.cur];
      if (x->Wh > 0) {
        hipLaunchKernelGGL(k_diag_c, dim3(NB), dim3(256), 0, x->stream, ch, N, x->Wh, x->Ph, x->kh0, x->kk, x->ll, x->diag_part);
        hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(1024), 0, x->stream, x->diag_part, NB, 4, 4, x->diag_out + 16);
      }
      // jacobian_psi_c with the u, v the reference still holds at a tick: those of the state at which the last step evaluated
      // its fourth stage (QGModel.py:375 vs :396); before any step, those of the current state
      const cd* qh4 = x->stepped ? x->q.y[(x->q.cur + 2) % 3] : x->q.y[x->q.cur];
      phase_invert_y(x, qh4, false, x->part0Q, nullptr, ch);
    }
    SLABTRY(exchange_now(grp, 3, false));
    for (nq_ctx* x : each(grp)) launch_products(x);
    SLABTRY(exchange_now(grp, 0, true));
    for (nq_ctx* x : each(grp)) {
      launch_A_m(x, false, {&x->mUc, &x->mVc});
      const int nwc = launch_project_c(x, x->cq.y[x->cq.cur], x->diag_part);
      if (nwc > 0) hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(1024), 0, x->stream, x->diag_part, nwc, 1, 1, x->diag_out + 20);
    }
    for (nq_ctx* x : each(grp))                           // the mixed-space rows of the CURRENT state again, for the next step
      phase_invert_y(x, x->q.y[x->q.cur], true, x->part0Q, nullptr, x->cq.y[x->cq.cur]);
    SLABTRY(exchange_now(grp, 3, false));
    SLABTRY(slab_allreduce(grp, 5));
    HIPCHK(c0, hipSetDevice(c0->device));
    HIPCHK(c0, hipMemcpyAsync(out + 16, c0->diag_out + 16, sizeof(double) * 5, hipMemcpyDeviceToHost, c0->stream));
    SLABTRY(slab_settle(grp));
    for (nq_ctx* x : each(grp)) SLABTRY(nq_sync(x));
    return 0;
  }
  if (!waves) return 0;
  // physical-space statistics: [16,24)
  for (nq_ctx* x : each(grp)) {
    if (coupled) launch_xdiag_m<MODE_COUPLED>(x, qbar, abar, x->diag_part);
    else launch_xdiag_m<MODE_UNCOUPLED>(x, qbar, abar, x->diag_part);
    hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(1024), 0, x->stream, x->diag_part, xdiag_blocks(x), 8, 8, x->diag_out + 16);
  }
  // projections of F[u phix + v phiy] ([24,28)) and of i F[phi q_psi] ([28,32)) on lap_h and diss_h; u, v, q_psi are
  // those of the last inversion, phix / phiy as last refreshed (UnCoupled: quirk Q1), like ref Kernel.py:680-700
  for (int which = 0; which < 2; ++which) {
    for (nq_ctx* x : each(grp)) launch_products_pass(x, which);
    SLABTRY(exchange_now(grp, 0, true));
    for (nq_ctx* x : each(grp)) {
      const int nww = (x->Wf / x->CLy) * x->S2;
      launch_A_m(x, false, {&x->mW});
      launch_project(x, x->diag_part);
      hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(1024), 0, x->stream, x->diag_part, nww, 4, 4, x->diag_out + 24 + 4 * which);
    }
  }
  SLABTRY(slab_allreduce(grp, 5));
  HIPCHK(c0, hipSetDevice(c0->device));
  HIPCHK(c0, hipMemcpyAsync(out + 16, c0->diag_out + 16, sizeof(double) * 16, hipMemcpyDeviceToHost, c0->stream));
  for (nq_ctx* x : each(grp)) SLABTRY(nq_sync(x));
  return 0;
}
int nq_diagnostics(nq_ctx* c, double* out) {
  NQ_SINGLE_RANK(c, "nq_diagnostics");
  if (!out) NQ_FAIL(c, -1, "nq_diagnostics: null output");
  std::vector<nq_ctx*> grp(1, c);
  SLABTRY(tick_need_phi(grp, "nq_diagnostics"));
  return tick_scalar(grp, out);
}
// the tick of a slab-decomposed simulation.  Collective.  It runs before set_phi too: a slab model's set_q reads ke_qg from
// these sums (slab.py: scalar), as Kernel.set_q does before the wave field exists.
int nq_slab_diagnostics(nq_ctx* c, double* out) {
  if (!c || !out) return -1;
  std::vector<nq_ctx*> grp;
  SLABTRY(slab_group(c, &grp));
  return tick_scalar(grp, out);
}

// ---- PDFs and joint PDFs of the physical fields (csrc/nq_hist.hpp) -----------------------------------
// slot of a public field id in the tables and the kernels: Kernel family q, q_psi, |phi|^2 -> 0, 1, 2; QGModel q, c -> 0, 1
static int hist_slot(const nq_ctx* c, int field) {
  if (c->kernel_family) return (field >= NQ_PDF_Q && field <= NQ_PDF_PHI2) ? field : -1;
  if (field == NQ_PDF_Q) return 0;
  return (field == NQ_PDF_C && c->passive) ? 1 : -1;
}
// flow fields (csrc/nq_flow.hpp): Kernel family only, one numbering for the PDFs and the averages
static_assert(NQ_FLOW_U == FLOW_U && NQ_FLOW_V == FLOW_V && NQ_FLOW_SN == FLOW_SN && NQ_FLOW_SS == FLOW_SS && NQ_FLOW_STRAIN2 == FLOW_STRAIN2 &&
              NQ_FLOW_OW == FLOW_OW && NQ_FLOW_GRADPHI2 == FLOW_GRADPHI2 && NQ_PDF_Q == FLOW_Q && NQ_PDF_QPSI == FLOW_QPSI && NQ_PDF_PHI2 == FLOW_PHI2,
              "public field ids and the kernel's value codes");
static bool is_flow(int field) { return field >= FLOW_FIRST && field <= FLOW_LAST; }
static bool any_flow(int nfields, const int* fields) {
  for (int i = 0; i < nfields; ++i)
    if (is_flow(fields[i])) return true;
  return false;
}
// A list of old fields keeps hist_slot's fixed slots and the old kernels.  A list that names a flow field goes through
// k_x_flow_hist for ALL of its fields: slot i is the i-th field of the list, and the selection says what each slot holds.
static FlowSel flow_sel_none(const nq_ctx* c) {
  FlowSel sel = {{FLOW_NONE, FLOW_NONE, FLOW_NONE}, 0, c->ph + (size_t)(c->N / 2) * c->Ph + c->N / 2, c->ll};
  return sel;
}
// values one launch holds per point (csrc/nq_flow.hpp: flow_nv): a call that selects more is issued as one launch per value
static int flow_nv_of(const nq_ctx* c) { return c->N >= 8192 ? 1 : HIST_SLOTS; }
// the range pass (part[block][2 i], [2 i + 1] = minimum and maximum of fields[i]) or the counting pass (`h` is the call's: slot i
// = field i) of a list that names a flow field
static void flow_hist_launch(nq_ctx* c, bool minmax, const FlowSel& sel, const HistArgs& h, double* part) {
  if (minmax) launch_xflow_hist<true>(c, sel, h, part);
  else launch_xflow_hist<false>(c, sel, h, part);
}
static void flow_hist(nq_ctx* c, bool minmax, int nfields, const int* fields, const HistArgs& h, double* part) {
  if (nfields <= flow_nv_of(c)) {
    FlowSel sel = flow_sel_none(c);
    for (int i = 0; i < nfields; ++i) sel.code[i] = fields[i];
    flow_hist_launch(c, minmax, sel, h, part);
    return;
  }
  for (int i = 0; i < nfields; ++i) {               // one value per launch, in the launch's slot 0 (no joint table: refused before)
    FlowSel sel = flow_sel_none(c);
    sel.code[0] = fields[i];
    HistArgs g = {};
    if (!minmax) {
      g.bins = h.bins;
      g.mask = 1;
      g.lo[0] = h.lo[i];
      g.hi[0] = h.hi[i];
      g.s[0] = h.s[i];
      g.tab = h.tab + (size_t)i * (h.bins + 3);
    }
    flow_hist_launch(c, minmax, sel, g, minmax ? part + 2 * i : nullptr);
  }
}
// one sample of the averages of an attachment that names a flow field (`a`, `sel`: slot s = its s-th real field)
static void flow_moments(nq_ctx* c, const FlowSel& sel, const AvgArgs& a) {
  int nreal = 0;
  for (int i = 0; i < HIST_SLOTS; ++i) nreal += sel.code[i] != FLOW_NONE;
  if (nreal <= flow_nv_of(c)) {
    launch_xflow_moments(c, sel, a);
    return;
  }
  for (int f = 0; f < nreal; ++f) {                 // one value per launch: its sum and its own second moment (mixed products: refused)
    FlowSel s = flow_sel_none(c);
    s.code[0] = sel.code[f];
    AvgArgs g = {};
    if (a.mask & (1 << f)) {
      g.mask = 1;
      g.sum[0] = a.sum[f];
    }
    for (int p = 0; p < a.np; ++p)
      if (a.pa[p] == f && a.pb[p] == f) g.prod[g.np++] = a.prod[p];       // pa = pb = 0
    if (f == 0 && (a.mask & (1 << AVG_PHI))) {
      g.mask |= 1 << AVG_PHI;
      g.sum_phi = a.sum_phi;
      s.phi = 1;
    }
    launch_xflow_moments(c, s, g);
  }
}
static int hist_check_fields(nq_ctx* c, const char* what, int nfields, const int* fields) {
  NQ_SINGLE_RANK(c, "nq_field_hist");
  if (!fields || nfields < 1 || nfields > HIST_SLOTS) NQ_FAIL(c, -1, "%s: %d fields (1 to %d)", what, nfields, HIST_SLOTS);
  for (int i = 0; i < nfields; ++i) {
    if (is_flow(fields[i]) && !c->kernel_family)
      NQ_FAIL(c, -1, "%s: flow field %d (NQ_FLOW_*) on a QGModel context: its plane route has no velocity or strain values yet (DESIGN.md section 7)", what, fields[i]);
    if (!is_flow(fields[i]) && hist_slot(c, fields[i]) < 0)
      NQ_FAIL(c, -1, "%s: field %d is not available here (Kernel family: NQ_PDF_Q, NQ_PDF_QPSI, NQ_PDF_PHI2 and the NQ_FLOW_* fields; QGModel: NQ_PDF_Q, with its passive scalar NQ_PDF_C)", what, fields[i]);
    for (int k = 0; k < i; ++k)
      if (fields[k] == fields[i]) NQ_FAIL(c, -1, "%s: field %d listed twice", what, fields[i]);
  }
  if (c->kernel_family && !c->have_phi) NQ_FAIL(c, -4, "%s: set_phi has not been called", what);
  return 0;
}
static int hist_alloc(nq_ctx* c) {
  if (!c->hist_tab) {
    ALLOC(c, c->hist_tab, (size_t)HIST_MAX_WORDS);
    ALLOC(c, c->hist_part, (size_t)6 * HIST_PART_BLOCKS);
  }
  return 0;
}
// QGModel: q (and c) of the current state as real planes, by the transforms nq_get_field uses (scratch planes of the downloads)
static void hist_qg_planes(nq_ctx* c, int mask, const double** a, const double** b) {
  *a = *b = nullptr;
  if (mask & 1) {
    inv2d_half(c, c->q.y[c->q.cur], c->scr_r, c->scr_h0);
    *a = c->scr_r;
  }
  if (mask & 2) {
    inv2d_half(c, c->cq.y[c->cq.cur], reinterpret_cast<double*>(c->scr_f0), c->scr_h0);
    *b = reinterpret_cast<const double*>(c->scr_f0);
  }
}

int nq_field_minmax(nq_ctx* c, int nfields, const int* fields, double* out) {
  {
    const int rc = hist_check_fields(c, "nq_field_minmax", nfields, fields);
    if (rc) return rc;
  }
  if (!out) NQ_FAIL(c, -1, "nq_field_minmax: null output");
  HIPCHK(c, hipSetDevice(c->device));
  {
    const int rc = hist_alloc(c);
    if (rc) return rc;
  }
  int nblk, per;
  const bool flow = any_flow(nfields, fields);
  if (c->kernel_family) {
    HistArgs h = {};
    nblk = xdiag_blocks(c);
    per = 6;
    if (flow) flow_hist(c, true, nfields, fields, h, c->hist_part);
    else launch_xhist<true>(c, h, c->hist_part);
  } else {
    int mask = 0;
    for (int i = 0; i < nfields; ++i) mask |= 1 << hist_slot(c, fields[i]);
    const double *a, *b;
    hist_qg_planes(c, mask, &a, &b);
    const size_t n = (size_t)c->N * c->N;
    nblk = hist_plane_grid(n);
    per = 4;
    hipLaunchKernelGGL(k_minmax_plane, dim3(nblk), dim3(256), 0, c->stream, a, b, n, 1, 0, 0, c->hist_part);
  }
  HIPCHK(c, hipGetLastError());
  std::vector<double> part((size_t)nblk * per);
  HIPCHK(c, hipMemcpyAsync(part.data(), c->hist_part, sizeof(double) * part.size(), hipMemcpyDeviceToHost, c->stream));
  {
    const int rc = nq_sync(c);
    if (rc) return rc;
  }
  for (int i = 0; i < nfields; ++i) {
    const int s = flow ? i : hist_slot(c, fields[i]);
    double lo = part[2 * s], hi = part[2 * s + 1];
    for (int k = 1; k < nblk; ++k) {                    // NaN in any workgroup's slot stays (min and max: order is irrelevant)
      const double a = part[(size_t)k * per + 2 * s], b = part[(size_t)k * per + 2 * s + 1];
      lo = (lo != lo || lo < a) ? lo : a;
      hi = (hi != hi || hi > b) ? hi : b;
    }
    out[2 * i] = lo;
    out[2 * i + 1] = hi;
  }
  return 0;
}

int nq_field_hist(nq_ctx* c, int nfields, const int* fields, const double* lo, const double* hi, int bins, int joint_a,
                  int joint_b, int joint_bins, int accumulate) {
  {
    const int rc = hist_check_fields(c, "nq_field_hist", nfields, fields);
    if (rc) return rc;
  }
  if (!lo || !hi) NQ_FAIL(c, -1, "nq_field_hist: null ranges");
  if (bins < 1 || bins > HIST_MAX_BINS) NQ_FAIL(c, -1, "nq_field_hist: bins = %d (1 to %d: the LDS tables of a workgroup)", bins, HIST_MAX_BINS);
  const bool joint = joint_a >= 0 || joint_b >= 0;
  int ja = -1, jb = -1;
  if (joint) {
    if (joint_bins < 1 || joint_bins > HIST_MAX_JBINS)
      NQ_FAIL(c, -1, "nq_field_hist: joint_bins = %d (1 to %d: the LDS tables of a workgroup)", joint_bins, HIST_MAX_JBINS);
    for (int i = 0; i < nfields; ++i) {
      if (fields[i] == joint_a) ja = i;
      if (fields[i] == joint_b) jb = i;
    }
    if (ja < 0 || jb < 0 || ja == jb) NQ_FAIL(c, -1, "nq_field_hist: the joint pair (%d, %d) is not two different fields of the list", joint_a, joint_b);
  }
  for (int i = 0; i < nfields; ++i)
    if (!std::isfinite(lo[i]) || !std::isfinite(hi[i]) || !(lo[i] < hi[i]))
      NQ_FAIL(c, -1, "nq_field_hist: range [%g, %g] of field %d (finite, lo < hi)", lo[i], hi[i], fields[i]);
  const bool flow = any_flow(nfields, fields);
  if (flow && joint && nfields > flow_nv_of(c))
    NQ_FAIL(c, -1, "nq_field_hist: a joint table with flow fields (NQ_FLOW_*) at nx = %d: a thread of that row plan holds one value, the pair needs two (DESIGN.md section 7)", c->N);
  nq_ctx::HistCfg cfg;
  cfg.nf = nfields;
  cfg.bins = bins;
  cfg.jbins = joint ? joint_bins : 0;
  cfg.ja = ja;
  cfg.jb = jb;
  for (int i = 0; i < nfields; ++i) {
    cfg.fields[i] = fields[i];
    cfg.slot[i] = flow ? i : hist_slot(c, fields[i]);
    cfg.lo[i] = lo[i];
    cfg.hi[i] = hi[i];
  }
  if (accumulate) {
    const nq_ctx::HistCfg& o = c->hist_cfg;
    bool same = c->hist_tab && o.nf == cfg.nf && o.bins == cfg.bins && o.jbins == cfg.jbins && o.ja == cfg.ja && o.jb == cfg.jb;
    for (int i = 0; same && i < nfields; ++i) same = o.fields[i] == cfg.fields[i] && o.lo[i] == cfg.lo[i] && o.hi[i] == cfg.hi[i];
    if (!same) NQ_FAIL(c, -1, "nq_field_hist: accumulate = 1 needs the fields, ranges and bin counts of the call that zeroed the tables");
  }
  HIPCHK(c, hipSetDevice(c->device));
  {
    const int rc = hist_alloc(c);
    if (rc) return rc;
  }
  HistArgs h = {};
  h.bins = bins;
  h.jbins = cfg.jbins;
  h.tab = c->hist_tab;
  for (int i = 0; i < nfields; ++i) {
    const int s = cfg.slot[i];
    h.mask |= 1 << s;
    h.lo[s] = lo[i];
    h.hi[s] = hi[i];
    h.s[s] = (double)bins / (hi[i] - lo[i]);
  }
  if (joint) {
    h.ja = cfg.slot[ja];
    h.jb = cfg.slot[jb];
    h.js[0] = (double)joint_bins / (hi[ja] - lo[ja]);
    h.js[1] = (double)joint_bins / (hi[jb] - lo[jb]);
  }
  const int words = hist_words(h.bins, h.jbins);
  if (!accumulate) HIPCHK(c, hipMemsetAsync(c->hist_tab, 0, sizeof(unsigned long long) * words, c->stream));
  if (c->kernel_family) {
    if (flow) flow_hist(c, false, nfields, fields, h, nullptr);
    else launch_xhist<false>(c, h, nullptr);
  } else {
    const double *a, *b;
    hist_qg_planes(c, h.mask, &a, &b);
    const size_t n = (size_t)c->N * c->N;
    hipLaunchKernelGGL(k_hist_plane, dim3(hist_plane_grid(n)), dim3(256), sizeof(unsigned) * words, c->stream, a, b, n, 1, 0, 0, h);
  }
  HIPCHK(c, hipGetLastError());
  c->hist_cfg = cfg;
  return 0;
}

int nq_field_hist_read(nq_ctx* c, unsigned long long* out) {
  NQ_SINGLE_RANK(c, "nq_field_hist_read");
  if (!out) NQ_FAIL(c, -1, "nq_field_hist_read: null output");
  const nq_ctx::HistCfg& g = c->hist_cfg;
  if (!c->hist_tab || g.nf == 0) NQ_FAIL(c, -4, "nq_field_hist_read: no nq_field_hist call yet");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t per = (size_t)g.bins + 3;
  for (int i = 0; i < g.nf; ++i)
    HIPCHK(c, hipMemcpyAsync(out + i * per, c->hist_tab + g.slot[i] * per, sizeof(unsigned long long) * per, hipMemcpyDeviceToHost, c->stream));
  if (g.jbins)
    HIPCHK(c, hipMemcpyAsync(out + g.nf * per, c->hist_tab + HIST_SLOTS * per, sizeof(unsigned long long) * ((size_t)g.jbins * g.jbins + 1), hipMemcpyDeviceToHost, c->stream));
  return nq_sync(c);
}

// ---- structure functions of the physical fields (csrc/nq_sf.hpp) ------------------------------------------
static_assert(SF_COLS == NQ_SF_COLS && SF_MAX_SEPS == NQ_SF_MAX_SEPS && SF_MAX_FIELDS == NQ_SF_MAX_FIELDS && SF_MAX_TRIPLES == NQ_SF_MAX_TRIPLES,
              "limits of nq_structure");
static_assert(NQ_SF_PHI > FLOW_LAST && NQ_SF_PHI != NQ_PDF_C && NQ_SF_PHI != NQ_AVG_PHI, "NQ_SF_PHI is no other field's id");
// The call in the kernels' canonical order (csrc/nq_sf.hpp): canon[i] = slot of the call's field i (real fields first, in the
// call's order, then the complex one); a: nsep, seps, nreal, phi and the triples in slots.  nullptr, or what is wrong.
static const char* sf_plan(int n, int nfields, const bool* cplx, int nsep, const int* seps, int ntriples, const int* triples, SfArgs* a, int* canon) {
  static char msg[256];
  if (nfields < 1 || nfields > SF_MAX_FIELDS) return "1 to 3 fields (the value registers and the LDS rows of the row pass)";
  if (!seps || nsep < 1 || nsep > SF_MAX_SEPS) return "1 to 64 separations";
  if (ntriples < 0 || ntriples > SF_MAX_TRIPLES || (ntriples && !triples)) return "0 to 4 triples";
  *a = SfArgs();
  for (int i = 0; i < nfields; ++i) {
    if (cplx[i]) {
      if (a->phi) return "the complex field listed twice";
      a->phi = 1;
    } else {
      canon[i] = a->nreal++;
    }
  }
  for (int i = 0; i < nfields; ++i)
    if (cplx[i]) canon[i] = a->nreal;
  a->nsep = nsep;
  for (int s = 0; s < nsep; ++s) {
    if (seps[s] < 1 || seps[s] > n - 1 || (s && seps[s] <= seps[s - 1])) {
      snprintf(msg, sizeof(msg), "separation %d at position %d (integers in [1, %d], strictly increasing)", seps[s], s, n - 1);
      return msg;
    }
  }
  a->ntri = ntriples;
  for (int k = 0; k < ntriples; ++k) {
    const int* t = triples + 3 * k;
    for (int i = 0; i < 3; ++i)
      if (t[i] < 0 || t[i] >= nfields) return "a triple holds three indices into the field list";
    if (cplx[t[0]] || cplx[t[1]] != cplx[t[2]]) return "the complex field enters a triple only as its last two entries together: (a, phi, phi) = <d a |d phi|^2>";
    for (int o = 0; o < k; ++o)
      if (triples[3 * o] == t[0] && triples[3 * o + 1] == t[1] && triples[3 * o + 2] == t[2]) return "a triple listed twice";
    a->ta[k] = canon[t[0]];
    a->tb[k] = cplx[t[1]] ? -1 : canon[t[1]];
    a->tc[k] = cplx[t[2]] ? -1 : canon[t[2]];
  }
  return nullptr;
}
// where the columns of a partial slot of NF field slots land in a table row of the call: field i at 9 i, triple k at 9 nfields + k
static SfMap sf_map(int NF, int nfields, const int* canon, int ntriples) {
  SfMap m;
  for (int i = 0; i < sf_ncols<SF_MAX_FIELDS>(); ++i) m.col[i] = -1;
  for (int i = 0; i < nfields; ++i)
    for (int k = 0; k < SF_COLS; ++k) m.col[canon[i] * SF_COLS + k] = i * SF_COLS + k;
  for (int k = 0; k < ntriples; ++k) m.col[NF * SF_COLS + k] = nfields * SF_COLS + k;
  return m;
}
static int sf_plane_grid(int rows) { return rows < 1024 ? rows : 1024; }
// the partials of a call: `count` doubles, allocated on first use and grown by the largest call (NQ_SF_PART_MAX_BYTES bounds it)
static int sf_reserve_part(nq_ctx* c, size_t count, const char* fn);
static int sf_reserve(nq_ctx* c) {
  if (!c->sf_tab) {
    ALLOC(c, c->sf_tab, (size_t)SF_MAX_SEPS * sf_ncols<SF_MAX_FIELDS>());
    ALLOC(c, c->sf_seps, (size_t)SF_MAX_SEPS);
  }
  return 0;
}
// the partials alone: nq_structure2 shares them (its table is its own)
static int sf_reserve_part(nq_ctx* c, size_t count, const char* fn) {
  if (count <= c->sf_part_count) return 0;
  if (c->sf_part_raw) {
    const int rc = nq_sync(c);                           // a launch of the last call may still write them
    if (rc) return rc;
    for (size_t i = 0; i < c->allocs.size(); ++i)
      if (c->allocs[i] == c->sf_part_raw) {
        c->allocs.erase(c->allocs.begin() + i);
        break;
      }
    (void)hipFree(c->sf_part_raw);
    c->bytes -= (long long)(c->sf_part_count * sizeof(double));
    c->sf_part_raw = nullptr;
    c->sf_part = nullptr;
    c->sf_part_count = 0;
  }
  void* p = nullptr;
  if (hipMalloc(&p, count * sizeof(double)) != hipSuccess) {
    (void)hipGetLastError();
    NQ_FAIL(c, -5, "%s: cannot allocate %zu bytes of device memory for the workgroup partials", fn, count * sizeof(double));
  }
  c->allocs.push_back(p);
  c->bytes += (long long)(count * sizeof(double));
  c->sf_part_raw = p;
  c->sf_part = static_cast<double*>(p);
  c->sf_part_count = count;
  return 0;
}

// The launches of one call: the sums of the current state into `tab` (nsep rows of 9 nfields + ntriples; on top of it with
// `accumulate`), through the shared partials.  dseps / hseps: the separations on the device and their staging copy.  The caller has
// checked the call (sf_plan: a, canon) and owns `tab`: nq_structure's running table, or the range pass of nq_increment_range.
static int sf_sums_into(nq_ctx* c, const char* fn, int nfields, const int* fields, const bool* cplx, SfArgs a, const int* canon, int nsep,
                        const int* seps, int ntriples, const int* triples, int accumulate, double* tab, int* dseps, int* hseps) {
  const bool one = c->kernel_family && flow_nv_of(c) == 1;        // one value per thread: a launch per field
  const int nout = nfields * SF_COLS + ntriples;
  const int NF = one ? 1 : SF_MAX_FIELDS, nc = one ? sf_ncols<1>() : sf_ncols<SF_MAX_FIELDS>();
  const int nblk = c->kernel_family ? xdiag_blocks(c) : sf_plane_grid(c->N);
  {
    const int rc = sf_reserve_part(c, (size_t)nblk * nsep * nc, fn);
    if (rc) return rc;
  }
  a.part = c->sf_part;
  a.seps = dseps;
  for (int s = 0; s < nsep; ++s) hseps[s] = seps[s];
  HIPCHK(c, hipMemcpyAsync(dseps, hseps, sizeof(int) * nsep, hipMemcpyHostToDevice, c->stream));
  const int tgrid = (nsep * nc + SF_TOTAL_ENTRIES - 1) / SF_TOTAL_ENTRIES;
  if (!c->kernel_family) {
    SfPlanes pl = {};
    int mask = 0;
    for (int i = 0; i < nfields; ++i) mask |= 1 << hist_slot(c, fields[i]);
    const double* qc[2];
    hist_qg_planes(c, mask, &qc[0], &qc[1]);
    for (int i = 0; i < nfields; ++i) {
      pl.p[canon[i]] = qc[hist_slot(c, fields[i])];
      pl.stride[canon[i]] = 1;
    }
    pl.rows = pl.cols = c->N;
    hipLaunchKernelGGL(k_sf_plane, dim3(nblk), dim3(SF_PLANE_THREADS), 0, c->stream, pl, a);
    hipLaunchKernelGGL(k_sf_total, dim3(tgrid), dim3(SF_TOTAL_RUNS * SF_TOTAL_ENTRIES), 0, c->stream, (const double*)c->sf_part, nblk, nsep, nc, sf_map(NF, nfields, canon, ntriples), nout, accumulate, tab);
  } else if (!one) {
    FlowSel sel = flow_sel_none(c);
    for (int i = 0; i < nfields; ++i)
      if (!cplx[i]) sel.code[canon[i]] = fields[i];
    sel.phi = a.phi;
    launch_xflow_sf(c, sel, a);
    hipLaunchKernelGGL(k_sf_total, dim3(tgrid), dim3(SF_TOTAL_RUNS * SF_TOTAL_ENTRIES), 0, c->stream, (const double*)c->sf_part, nblk, nsep, nc, sf_map(NF, nfields, canon, ntriples), nout, accumulate, tab);
  } else {
    for (int i = 0; i < nfields; ++i) {                 // one field per launch, in the launch's slot 0, into its own columns
      FlowSel sel = flow_sel_none(c);
      SfArgs g = a;
      g.nreal = cplx[i] ? 0 : 1;
      g.phi = cplx[i] ? 1 : 0;
      g.ntri = 0;
      if (!cplx[i]) sel.code[0] = fields[i];
      sel.phi = g.phi;
      SfMap m;
      for (int k = 0; k < sf_ncols<SF_MAX_FIELDS>(); ++k) m.col[k] = k < SF_COLS ? i * SF_COLS + k : -1;
      for (int k = 0; k < ntriples; ++k)
        if (triples[3 * k] == i) {                       // (i, i, i): refused above otherwise
          g.ta[g.ntri] = g.tb[g.ntri] = g.tc[g.ntri] = 0;
          m.col[SF_COLS + g.ntri++] = nfields * SF_COLS + k;
        }
      launch_xflow_sf(c, sel, g);
      hipLaunchKernelGGL(k_sf_total, dim3(tgrid), dim3(SF_TOTAL_RUNS * SF_TOTAL_ENTRIES), 0, c->stream, (const double*)c->sf_part, nblk, nsep, nc, m, nout, accumulate, tab);
    }
  }
  HIPCHK(c, hipGetLastError());
  return 0;
}

int nq_structure(nq_ctx* c, int nfields, const int* fields, int nsep, const int* seps, int ntriples, const int* triples, int accumulate) {
  NQ_SINGLE_RANK(c, "nq_structure");
  if (!fields || nfields < 1 || nfields > SF_MAX_FIELDS) NQ_FAIL(c, -1, "nq_structure: %d fields (1 to %d)", nfields, SF_MAX_FIELDS);
  bool cplx[SF_MAX_FIELDS] = {};
  for (int i = 0; i < nfields; ++i) {
    cplx[i] = fields[i] == NQ_SF_PHI;
    if ((cplx[i] || is_flow(fields[i])) && !c->kernel_family)
      NQ_FAIL(c, -1, "nq_structure: field %d (NQ_FLOW_*, NQ_SF_PHI) on a QGModel context: its plane route has q and its passive scalar only (DESIGN.md section 7)", fields[i]);
    if (!cplx[i] && !is_flow(fields[i]) && hist_slot(c, fields[i]) < 0)
      NQ_FAIL(c, -1, "nq_structure: field %d is not available here (Kernel family: NQ_PDF_Q, NQ_PDF_QPSI, NQ_PDF_PHI2, the NQ_FLOW_* fields and NQ_SF_PHI; QGModel: NQ_PDF_Q, with its passive scalar NQ_PDF_C)", fields[i]);
    for (int k = 0; k < i; ++k)
      if (fields[k] == fields[i]) NQ_FAIL(c, -1, "nq_structure: field %d listed twice", fields[i]);
  }
  if (c->kernel_family ? !c->have_phi : !c->have_q) NQ_FAIL(c, -4, "nq_structure: %s has not been called", c->kernel_family ? "set_phi" : "set_q");
  SfArgs a;
  int canon[SF_MAX_FIELDS] = {};
  if (const char* bad = sf_plan(c->N, nfields, cplx, nsep, seps, ntriples, triples, &a, canon)) NQ_FAIL(c, -1, "nq_structure: %s", bad);
  const bool one = c->kernel_family && flow_nv_of(c) == 1;        // one value per thread: a launch per field
  if (one && a.phi && nfields > 1)
    NQ_FAIL(c, -1, "nq_structure: NQ_SF_PHI beside a real field at nx = %d: a thread of that row plan holds one value, so every field runs in a launch of its own (DESIGN.md section 7); NQ_SF_PHI alone works", c->N);
  if (one)
    for (int k = 0; k < ntriples; ++k)
      if (triples[3 * k] != triples[3 * k + 1] || triples[3 * k] != triples[3 * k + 2])
        NQ_FAIL(c, -1, "nq_structure: a triple of different fields at nx = %d: a thread of that row plan holds one value, so every field runs in a launch of its own (DESIGN.md section 7); single fields and (a, a, a) work", c->N);
  nq_ctx::SfCfg cfg;
  cfg.nf = nfields;
  cfg.nsep = nsep;
  cfg.ntri = ntriples;
  for (int i = 0; i < nfields; ++i) cfg.fields[i] = fields[i];
  for (int s = 0; s < nsep; ++s) cfg.seps[s] = seps[s];
  for (int k = 0; k < 3 * ntriples; ++k) cfg.tri[k] = triples[k];
  if (accumulate) {
    const nq_ctx::SfCfg& o = c->sf_cfg;
    bool same = c->sf_tab && o.samples > 0 && o.nf == cfg.nf && o.nsep == cfg.nsep && o.ntri == cfg.ntri;
    for (int i = 0; same && i < nfields; ++i) same = o.fields[i] == cfg.fields[i];
    for (int s = 0; same && s < nsep; ++s) same = o.seps[s] == cfg.seps[s];
    for (int k = 0; same && k < 3 * ntriples; ++k) same = o.tri[k] == cfg.tri[k];
    if (!same) NQ_FAIL(c, -1, "nq_structure: accumulate = 1 needs the fields, separations and triples of the call that zeroed the table");
    cfg.samples = o.samples;
  }
  HIPCHK(c, hipSetDevice(c->device));
  {
    int rc = sf_reserve(c);
    if (!rc) rc = sf_sums_into(c, "nq_structure", nfields, fields, cplx, a, canon, nsep, seps, ntriples, triples, accumulate, c->sf_tab, c->sf_seps, c->sf_seps_host);
    if (rc) return rc;
  }
  ++cfg.samples;
  c->sf_cfg = cfg;
  return 0;
}

int nq_structure_read(nq_ctx* c, long long* samples, double* out) {
  NQ_SINGLE_RANK(c, "nq_structure_read");
  if (!samples || !out) NQ_FAIL(c, -1, "nq_structure_read: null output");
  const nq_ctx::SfCfg& g = c->sf_cfg;
  if (!c->sf_tab || g.nf == 0) NQ_FAIL(c, -4, "nq_structure_read: no nq_structure call yet");
  HIPCHK(c, hipSetDevice(c->device));
  *samples = g.samples;
  HIPCHK(c, hipMemcpyAsync(out, c->sf_tab, sizeof(double) * g.nsep * (g.nf * SF_COLS + g.ntri), hipMemcpyDeviceToHost, c->stream));
  return nq_sync(c);
}

// ---- structure functions at two-dimensional separations (csrc/nq_sf2.hpp) -----------------------------------
static_assert(SF2_MAX_VECS == NQ_SF2_MAX_VECS, "limits of nq_structure2");
static_assert((size_t)64 * NQ_SF2_MAX_VECS * sf_ncols<SF_MAX_FIELDS>() * sizeof(double) <= NQ_SF_PART_MAX_BYTES, "64 workgroups of the longest list fit the partials");
// The call in the kernels' terms: fields and triples through sf_plan (canon, nreal, phi, the triples in slots); the vectors checked,
// r_x brought to [0, cols), sorted by (r_y, r_x) into `sorted` with their position in the caller's list; the rotated pair in slots.
// nullptr, or what is wrong.
static const char* sf2_plan(int rows, int cols, int nfields, const bool* cplx, int nvec, const int* vecs, const double* proj, int pa, int pb,
                            int ntriples, const int* triples, Sf2Args* a, int* canon, Sf2Vec* sorted) {
  static char msg[256];
  static const int one = 1;
  SfArgs x;
  if (const char* bad = sf_plan(cols, nfields, cplx, 1, &one, ntriples, triples, &x, canon)) return bad;
  *a = Sf2Args();
  a->nreal = x.nreal;
  a->phi = x.phi;
  a->ntri = x.ntri;
  for (int k = 0; k < x.ntri; ++k) a->tri |= sf2_tri_pack(k, x.ta[k], x.tb[k], x.tc[k]);
  if (!vecs || nvec < 1 || nvec > SF2_MAX_VECS) return "1 to 256 vectors";
  for (int i = 0; i < nvec; ++i) {
    const int rx = vecs[2 * i], ry = vecs[2 * i + 1];
    if (rx <= -cols || rx >= cols || ry < 0 || ry >= rows || (rx == 0 && ry == 0)) {
      snprintf(msg, sizeof(msg), "vector (%d, %d) at position %d (r_x in [%d, %d], r_y in [0, %d], not (0, 0))", rx, ry, i, -(cols - 1), cols - 1, rows - 1);
      return msg;
    }
    sorted[i].rx = rx < 0 ? rx + cols : rx;
    sorted[i].ry = ry;
    sorted[i].slot = i;
    sorted[i].pad = 0;
  }
  std::sort(sorted, sorted + nvec, [](const Sf2Vec& p, const Sf2Vec& q) { return p.ry != q.ry ? p.ry < q.ry : (p.rx != q.rx ? p.rx < q.rx : p.slot < q.slot); });
  for (int i = 1; i < nvec; ++i)
    if (sorted[i].rx == sorted[i - 1].rx && sorted[i].ry == sorted[i - 1].ry) {
      snprintf(msg, sizeof(msg), "the vectors at positions %d and %d are one vector (or one and its periodic image r_x - nx)", sorted[i - 1].slot, sorted[i].slot);
      return msg;
    }
  a->nvec = nvec;
  a->pa = a->pb = -1;
  if (!proj) {
    if (pa != -1 || pb != -1) return "proj_a, proj_b without proj (NULL goes with -1, -1)";
  } else {
    if (pa < 0 || pa >= nfields || pb < 0 || pb >= nfields) return "proj_a, proj_b are indices into the field list";
    if (pa == pb) return "the projection names one field twice";
    if (cplx[pa] || cplx[pb]) return "the projection rotates two real fields, not the complex one";
    for (int i = 0; i < 2 * nvec; ++i)
      if (!std::isfinite(proj[i])) return "proj holds a non-finite value";
    a->pa = canon[pa];
    a->pb = canon[pb];
  }
  return nullptr;
}
// `bytes` of device memory in *raw (counted, owned by the context), grown by the largest call; a failure leaves the old buffer
static int sf2_grow(nq_ctx* c, void** raw, size_t* have, size_t bytes, const char* what, const char* fn = "nq_structure2") {
  if (bytes <= *have) return 0;
  void* p = nullptr;
  if (hipMalloc(&p, bytes) != hipSuccess) {
    (void)hipGetLastError();
    NQ_FAIL(c, -5, "%s: cannot allocate %zu bytes of device memory for %s", fn, bytes, what);
  }
  if (*raw) {
    const int rc = nq_sync(c);                           // a launch of the last call may still use it
    if (rc) {
      (void)hipFree(p);
      return rc;
    }
    for (size_t i = 0; i < c->allocs.size(); ++i)
      if (c->allocs[i] == *raw) {
        c->allocs.erase(c->allocs.begin() + i);
        break;
      }
    (void)hipFree(*raw);
    c->bytes -= (long long)*have;
  }
  c->allocs.push_back(p);
  c->bytes += (long long)bytes;
  *raw = p;
  *have = bytes;
  return 0;
}
static int alloc_all_or_none(nq_ctx* c, std::vector<std::pair<void**, size_t>>& want, const char* fn);

// The physical planes of a call's fields in the kernels' canonical slots: QGModel's scratch planes (an inverse transform each), or,
// on the Kernel family, the context's pool, filled by the store pass (grown by the largest call; a failure leaves the old pool)
static int sf2_planes_of(nq_ctx* c, const char* fn, int nfields, const int* fields, const bool* cplx, const int* canon, int nreal, int phi, SfPlanes* out) {
  const int N = c->N;
  const size_t plane = (size_t)N * N;
  if (c->kernel_family) {
    const int rc = sf2_grow(c, &c->sf2_planes, &c->sf2_planes_count, (size_t)(nreal + 2 * phi) * plane * sizeof(double), "the physical planes", fn);
    if (rc) return rc;
  }
  SfPlanes pl = {};
  pl.rows = pl.cols = N;
  if (!c->kernel_family) {
    int mask = 0;
    for (int i = 0; i < nfields; ++i) mask |= 1 << hist_slot(c, fields[i]);
    const double* qc[2];
    hist_qg_planes(c, mask, &qc[0], &qc[1]);
    for (int i = 0; i < nfields; ++i) {
      pl.p[canon[i]] = qc[hist_slot(c, fields[i])];
      pl.stride[canon[i]] = 1;
    }
  } else {
    double* pool = static_cast<double*>(c->sf2_planes);
    for (int i = 0; i < nfields; ++i) {                 // the real planes in slot order, then the complex one
      pl.p[canon[i]] = pool + (size_t)canon[i] * plane;
      pl.stride[canon[i]] = cplx[i] ? 2 : 1;
    }
    if (nfields <= flow_nv_of(c)) {
      FlowSel sel = flow_sel_none(c);
      Sf2Store st = {};
      for (int i = 0; i < nfields; ++i) {
        if (cplx[i]) {
          sel.phi = 1;
          st.phi = reinterpret_cast<cd*>(pool + (size_t)canon[i] * plane);
        } else {
          sel.code[canon[i]] = fields[i];
          st.re[canon[i]] = pool + (size_t)canon[i] * plane;
        }
      }
      launch_xflow_store(c, sel, st);
    } else {
      for (int i = 0; i < nfields; ++i) {               // one value per launch, in the launch's slot 0, into that field's plane
        FlowSel sel = flow_sel_none(c);
        Sf2Store st = {};
        if (cplx[i]) {
          sel.phi = 1;
          st.phi = reinterpret_cast<cd*>(pool + (size_t)canon[i] * plane);
        } else {
          sel.code[0] = fields[i];
          st.re[0] = pool + (size_t)canon[i] * plane;
        }
        launch_xflow_store(c, sel, st);
      }
    }
  }
  *out = pl;
  return 0;
}
// The launches of one call: the sums of the current state into `tab` (nvec rows; on top of it with `accumulate`) through the shared
// partials.  dvecs, dproj / hvecs, hproj: the sorted vectors and the projection on the device and their staging copies.  The caller
// has checked the call (sf2_plan: a, canon, sorted) and owns `tab`: nq_structure2's running table, or nq_increment_range2's.
static int sf2_sums_into(nq_ctx* c, const char* fn, int nfields, const int* fields, const bool* cplx, Sf2Args a, const int* canon, const Sf2Vec* sorted,
                         int nvec, const double* proj, int ntriples, int accumulate, double* tab, Sf2Vec* dvecs, Sf2Vec* hvecs, double* dproj, double* hproj) {
  const int N = c->N, nout = nfields * SF_COLS + ntriples;
  const Sf2Route route = sf2_route(N, a.nreal, a.phi);
  const int nblk = sf2_grid(N, nvec, route.nc);
  {
    const int rc = sf_reserve_part(c, (size_t)nblk * nvec * route.nc, fn);
    if (rc) return rc;
  }
  a.part = c->sf_part;
  a.vecs = dvecs;
  a.proj = proj ? dproj : nullptr;
  for (int i = 0; i < nvec; ++i) hvecs[i] = sorted[i];
  HIPCHK(c, hipMemcpyAsync(dvecs, hvecs, sizeof(Sf2Vec) * nvec, hipMemcpyHostToDevice, c->stream));
  if (proj) {
    for (int i = 0; i < 2 * nvec; ++i) hproj[i] = proj[i];
    HIPCHK(c, hipMemcpyAsync(dproj, hproj, sizeof(double) * 2 * nvec, hipMemcpyHostToDevice, c->stream));
  }
  SfPlanes pl = {};
  {
    const int rc = sf2_planes_of(c, fn, nfields, fields, cplx, canon, a.nreal, a.phi, &pl);
    if (rc) return rc;
  }
  sf2_launch(c->stream, nblk, route, pl, a);
  const int tgrid = (nvec * route.nc + SF_TOTAL_ENTRIES - 1) / SF_TOTAL_ENTRIES;
  hipLaunchKernelGGL(k_sf_total, dim3(tgrid), dim3(SF_TOTAL_RUNS * SF_TOTAL_ENTRIES), 0, c->stream, (const double*)c->sf_part, nblk, nvec, route.nc,
                     sf_map(route.nc == sf_ncols<1>() ? 1 : (route.nc == sf_ncols<2>() ? 2 : 3), nfields, canon, ntriples), nout, accumulate, tab);
  HIPCHK(c, hipGetLastError());
  return 0;
}

int nq_structure2(nq_ctx* c, int nfields, const int* fields, int nvec, const int* vecs, const double* proj, int proj_a, int proj_b,
                  int ntriples, const int* triples, int accumulate) {
  NQ_SINGLE_RANK(c, "nq_structure2");
  if (!fields || nfields < 1 || nfields > SF_MAX_FIELDS) NQ_FAIL(c, -1, "nq_structure2: %d fields (1 to %d)", nfields, SF_MAX_FIELDS);
  bool cplx[SF_MAX_FIELDS] = {};
  for (int i = 0; i < nfields; ++i) {
    cplx[i] = fields[i] == NQ_SF_PHI;
    if ((cplx[i] || is_flow(fields[i])) && !c->kernel_family)
      NQ_FAIL(c, -1, "nq_structure2: field %d (NQ_FLOW_*, NQ_SF_PHI) on a QGModel context: its plane route has q and its passive scalar only (DESIGN.md section 7)", fields[i]);
    if (!cplx[i] && !is_flow(fields[i]) && hist_slot(c, fields[i]) < 0)
      NQ_FAIL(c, -1, "nq_structure2: field %d is not available here (Kernel family: NQ_PDF_Q, NQ_PDF_QPSI, NQ_PDF_PHI2, the NQ_FLOW_* fields and NQ_SF_PHI; QGModel: NQ_PDF_Q, with its passive scalar NQ_PDF_C)", fields[i]);
    for (int k = 0; k < i; ++k)
      if (fields[k] == fields[i]) NQ_FAIL(c, -1, "nq_structure2: field %d listed twice", fields[i]);
  }
  if (c->kernel_family ? !c->have_phi : !c->have_q) NQ_FAIL(c, -4, "nq_structure2: %s has not been called", c->kernel_family ? "set_phi" : "set_q");
  const int N = c->N;
  Sf2Args a;
  int canon[SF_MAX_FIELDS] = {};
  Sf2Vec sorted[SF2_MAX_VECS];
  if (const char* bad = sf2_plan(N, N, nfields, cplx, nvec, vecs, proj, proj_a, proj_b, ntriples, triples, &a, canon, sorted)) NQ_FAIL(c, -1, "nq_structure2: %s", bad);
  nq_ctx::Sf2Cfg cfg;
  cfg.nf = nfields;
  cfg.nvec = nvec;
  cfg.ntri = ntriples;
  cfg.pa = proj_a;
  cfg.pb = proj_b;
  cfg.has_proj = proj != nullptr;
  for (int i = 0; i < nfields; ++i) cfg.fields[i] = fields[i];
  for (int i = 0; i < 2 * nvec; ++i) cfg.vecs[i] = vecs[i];
  for (int i = 0; proj && i < 2 * nvec; ++i) cfg.proj[i] = proj[i];
  for (int k = 0; k < 3 * ntriples; ++k) cfg.tri[k] = triples[k];
  if (accumulate) {
    const nq_ctx::Sf2Cfg& o = c->sf2_cfg;
    bool same = c->sf2_tab && o.samples > 0 && o.nf == cfg.nf && o.nvec == cfg.nvec && o.ntri == cfg.ntri && o.pa == cfg.pa && o.pb == cfg.pb && o.has_proj == cfg.has_proj;
    for (int i = 0; same && i < nfields; ++i) same = o.fields[i] == cfg.fields[i];
    for (int i = 0; same && i < 2 * nvec; ++i) same = o.vecs[i] == cfg.vecs[i] && (!proj || memcmp(&o.proj[i], &cfg.proj[i], sizeof(double)) == 0);
    for (int k = 0; same && k < 3 * ntriples; ++k) same = o.tri[k] == cfg.tri[k];
    if (!same) NQ_FAIL(c, -1, "nq_structure2: accumulate = 1 needs the fields, vectors, projection and triples of the call that zeroed the table");
    cfg.samples = o.samples;
  }
  HIPCHK(c, hipSetDevice(c->device));
  if (!c->sf2_tab) {
    std::vector<std::pair<void**, size_t>> want;
    want.push_back({(void**)&c->sf2_tab, sizeof(double) * SF2_MAX_VECS * sf_ncols<SF_MAX_FIELDS>()});
    want.push_back({(void**)&c->sf2_vecs, sizeof(Sf2Vec) * SF2_MAX_VECS});
    want.push_back({(void**)&c->sf2_proj, sizeof(double) * 2 * SF2_MAX_VECS});
    const int rc = alloc_all_or_none(c, want, "nq_structure2");
    if (rc) return rc;
  }
  {
    const int rc = sf2_sums_into(c, "nq_structure2", nfields, fields, cplx, a, canon, sorted, nvec, proj, ntriples, accumulate, c->sf2_tab, c->sf2_vecs,
                                 c->sf2_vecs_host, c->sf2_proj, c->sf2_proj_host);
    if (rc) return rc;
  }
  ++cfg.samples;
  c->sf2_cfg = cfg;
  return 0;
}

int nq_structure2_read(nq_ctx* c, long long* samples, double* out) {
  NQ_SINGLE_RANK(c, "nq_structure2_read");
  if (!samples || !out) NQ_FAIL(c, -1, "nq_structure2_read: null output");
  const nq_ctx::Sf2Cfg& g = c->sf2_cfg;
  if (!c->sf2_tab || g.nf == 0) NQ_FAIL(c, -4, "nq_structure2_read: no nq_structure2 call yet");
  HIPCHK(c, hipSetDevice(c->device));
  *samples = g.samples;
  HIPCHK(c, hipMemcpyAsync(out, c->sf2_tab, sizeof(double) * g.nvec * (g.nf * SF_COLS + g.ntri), hipMemcpyDeviceToHost, c->stream));
  return nq_sync(c);
}

// ---- PDFs of the increments (csrc/nq_ipdf.hpp) ---------------------------------------------------------------
static_assert(IPDF_MAX_BINS == NQ_IPDF_MAX_BINS, "limits of nq_increment_hist");
constexpr size_t IPDF_SMALL_BYTES = sizeof(double) * 3 * SF_MAX_FIELDS * SF2_MAX_VECS + sizeof(double) * 2 * SF2_MAX_VECS + sizeof(Sf2Vec) * SF2_MAX_VECS +
                                    sizeof(double) * SF2_MAX_VECS * sf_ncols<SF_MAX_FIELDS>() + sizeof(int) * SF_MAX_SEPS;
static_assert(sizeof(unsigned long long) * SF2_MAX_VECS * SF_MAX_FIELDS * (IPDF_MAX_BINS + 3) + IPDF_SMALL_BYTES <= (size_t)NQ_IPDF_DEVICE_BYTES,
              "the largest count table and the small buffers are what the header declares");
constexpr int IPDF_PLANE_GRID = 512;              // workgroups of k_ipdf_plane: each flushes one table per vector
// the fields of a call: nq_structure's checks; cplx[i]: field i is NQ_SF_PHI
static int ipdf_check_fields(nq_ctx* c, const char* fn, int nfields, const int* fields, bool* cplx) {
  if (!fields || nfields < 1 || nfields > SF_MAX_FIELDS) NQ_FAIL(c, -1, "%s: %d fields (1 to %d)", fn, nfields, SF_MAX_FIELDS);
  for (int i = 0; i < nfields; ++i) {
    cplx[i] = fields[i] == NQ_SF_PHI;
    if ((cplx[i] || is_flow(fields[i])) && !c->kernel_family)
      NQ_FAIL(c, -1, "%s: field %d (NQ_FLOW_*, NQ_SF_PHI) on a QGModel context: its plane route has q and its passive scalar only (DESIGN.md section 7)", fn, fields[i]);
    if (!cplx[i] && !is_flow(fields[i]) && hist_slot(c, fields[i]) < 0)
      NQ_FAIL(c, -1, "%s: field %d is not available here (Kernel family: NQ_PDF_Q, NQ_PDF_QPSI, NQ_PDF_PHI2, the NQ_FLOW_* fields and NQ_SF_PHI; QGModel: NQ_PDF_Q, with its passive scalar NQ_PDF_C)", fn, fields[i]);
    for (int k = 0; k < i; ++k)
      if (fields[k] == fields[i]) NQ_FAIL(c, -1, "%s: field %d listed twice", fn, fields[i]);
  }
  if (c->kernel_family ? !c->have_phi : !c->have_q) NQ_FAIL(c, -4, "%s: %s has not been called", fn, c->kernel_family ? "set_phi" : "set_q");
  return 0;
}
// bins and the n x nfields ranges of a call; nullptr, or what is wrong
static const char* ipdf_check_ranges(int n, int nfields, const double* lo, const double* hi, int bins) {
  static char msg[256];
  if (bins < 1 || bins > IPDF_MAX_BINS) {
    snprintf(msg, sizeof(msg), "bins = %d (1 to %d: the LDS tables of a workgroup)", bins, IPDF_MAX_BINS);
    return msg;
  }
  if (!lo || !hi) return "null ranges";
  for (int i = 0; i < n * nfields; ++i)
    if (!std::isfinite(lo[i]) || !std::isfinite(hi[i]) || !(lo[i] < hi[i])) {
      snprintf(msg, sizeof(msg), "range [%g, %g] of row %d, field %d (finite, lo < hi)", lo[i], hi[i], i / nfields, i % nfields);
      return msg;
    }
  return nullptr;
}
// the small buffers: all of them or none
static int ipdf_reserve(nq_ctx* c, const char* fn) {
  if (c->ipdf_rng) return 0;
  std::vector<std::pair<void**, size_t>> want;
  want.push_back({(void**)&c->ipdf_rng, sizeof(double) * 3 * SF_MAX_FIELDS * SF2_MAX_VECS});
  want.push_back({(void**)&c->ipdf_proj, sizeof(double) * 2 * SF2_MAX_VECS});
  want.push_back({(void**)&c->ipdf_vecs, sizeof(Sf2Vec) * SF2_MAX_VECS});
  want.push_back({(void**)&c->ipdf_sums, sizeof(double) * SF2_MAX_VECS * sf_ncols<SF_MAX_FIELDS>()});
  want.push_back({(void**)&c->ipdf_seps, sizeof(int) * SF_MAX_SEPS});
  return alloc_all_or_none(c, want, fn);
}
// columns 0 and 1 of every field of the range pass's table -> out
static int ipdf_range_out(nq_ctx* c, int n, int nfields, double* out) {
  const int nout = nfields * SF_COLS;
  std::vector<double> host((size_t)n * nout);
  HIPCHK(c, hipMemcpyAsync(host.data(), c->ipdf_sums, sizeof(double) * host.size(), hipMemcpyDeviceToHost, c->stream));
  const int rc = nq_sync(c);
  if (rc) return rc;
  for (int i = 0; i < n; ++i)
    for (int f = 0; f < nfields; ++f) {
      out[((size_t)i * nfields + f) * 2] = host[(size_t)i * nout + f * SF_COLS];
      out[((size_t)i * nfields + f) * 2 + 1] = host[(size_t)i * nout + f * SF_COLS + 1];
    }
  return 0;
}

int nq_increment_range(nq_ctx* c, int nfields, const int* fields, int nsep, const int* seps, double* out) {
  static const char* fn = "nq_increment_range";
  NQ_SINGLE_RANK(c, "nq_increment_range");
  bool cplx[SF_MAX_FIELDS] = {};
  {
    const int rc = ipdf_check_fields(c, fn, nfields, fields, cplx);
    if (rc) return rc;
  }
  if (!out) NQ_FAIL(c, -1, "%s: null output", fn);
  SfArgs a;
  int canon[SF_MAX_FIELDS] = {};
  if (const char* bad = sf_plan(c->N, nfields, cplx, nsep, seps, 0, nullptr, &a, canon)) NQ_FAIL(c, -1, "%s: %s", fn, bad);
  HIPCHK(c, hipSetDevice(c->device));
  {
    int rc = ipdf_reserve(c, fn);
    if (!rc) rc = sf_sums_into(c, fn, nfields, fields, cplx, a, canon, nsep, seps, 0, nullptr, 0, c->ipdf_sums, c->ipdf_seps, c->ipdf_seps_host);
    if (rc) return rc;
  }
  return ipdf_range_out(c, nsep, nfields, out);
}

int nq_increment_range2(nq_ctx* c, int nfields, const int* fields, int nvec, const int* vecs, const double* proj, int proj_a, int proj_b, double* out) {
  static const char* fn = "nq_increment_range2";
  NQ_SINGLE_RANK(c, "nq_increment_range2");
  bool cplx[SF_MAX_FIELDS] = {};
  {
    const int rc = ipdf_check_fields(c, fn, nfields, fields, cplx);
    if (rc) return rc;
  }
  if (!out) NQ_FAIL(c, -1, "%s: null output", fn);
  Sf2Args a;
  int canon[SF_MAX_FIELDS] = {};
  Sf2Vec sorted[SF2_MAX_VECS];
  if (const char* bad = sf2_plan(c->N, c->N, nfields, cplx, nvec, vecs, proj, proj_a, proj_b, 0, nullptr, &a, canon, sorted)) NQ_FAIL(c, -1, "%s: %s", fn, bad);
  HIPCHK(c, hipSetDevice(c->device));
  {
    int rc = ipdf_reserve(c, fn);
    if (!rc) rc = sf2_sums_into(c, fn, nfields, fields, cplx, a, canon, sorted, nvec, proj, 0, 0, c->ipdf_sums, c->ipdf_vecs, c->ipdf_vecs_host, c->ipdf_proj, c->ipdf_proj_host);
    if (rc) return rc;
  }
  return ipdf_range_out(c, nvec, nfields, out);
}

// What the two counting calls share once the call is checked: accumulate = 1 against the call that zeroed the table, the buffers
// (the count table grown to this call), the table zeroed without `accumulate`, the ranges on the device.  cfg: this call, samples
// filled in.  g: bins, nfields, rng and tab filled in.
static int ipdf_begin(nq_ctx* c, const char* fn, nq_ctx::IpdfCfg& cfg, const double* lo, const double* hi, int accumulate, IpdfArgs* g) {
  const int cells = cfg.n * cfg.nf;
  for (int i = 0; i < cells; ++i) {
    cfg.lo[i] = lo[i];
    cfg.hi[i] = hi[i];
  }
  if (accumulate) {
    const nq_ctx::IpdfCfg& o = c->ipdf_cfg;
    bool same = c->ipdf_tab && o.samples > 0 && o.kind == cfg.kind && o.nf == cfg.nf && o.n == cfg.n && o.bins == cfg.bins && o.pa == cfg.pa && o.pb == cfg.pb &&
                o.has_proj == cfg.has_proj;
    for (int i = 0; same && i < cfg.nf; ++i) same = o.fields[i] == cfg.fields[i];
    for (int i = 0; same && i < (cfg.kind == 1 ? 1 : 2) * cfg.n; ++i) same = o.vecs[i] == cfg.vecs[i];
    for (int i = 0; same && cfg.has_proj && i < 2 * cfg.n; ++i) same = memcmp(&o.proj[i], &cfg.proj[i], sizeof(double)) == 0;
    for (int i = 0; same && i < cells; ++i) same = memcmp(&o.lo[i], &cfg.lo[i], sizeof(double)) == 0 && memcmp(&o.hi[i], &cfg.hi[i], sizeof(double)) == 0;
    if (!same) NQ_FAIL(c, -1, "%s: accumulate = 1 needs the fields, separations or vectors, projection, ranges and bins of the call that zeroed the table", fn);
    cfg.samples = o.samples;
  }
  HIPCHK(c, hipSetDevice(c->device));
  const size_t bytes = sizeof(unsigned long long) * cells * (cfg.bins + 3);
  {
    int rc = ipdf_reserve(c, fn);
    if (!rc) rc = sf2_grow(c, &c->ipdf_tab, &c->ipdf_tab_bytes, bytes, "the count table", fn);
    if (rc) return rc;
  }
  if (!accumulate) HIPCHK(c, hipMemsetAsync(c->ipdf_tab, 0, bytes, c->stream));
  for (int i = 0; i < cells; ++i) {
    c->ipdf_rng_host[3 * i] = lo[i];
    c->ipdf_rng_host[3 * i + 1] = hi[i];
    c->ipdf_rng_host[3 * i + 2] = (double)cfg.bins / (hi[i] - lo[i]);
  }
  HIPCHK(c, hipMemcpyAsync(c->ipdf_rng, c->ipdf_rng_host, sizeof(double) * 3 * cells, hipMemcpyHostToDevice, c->stream));
  g->bins = cfg.bins;
  g->nfields = cfg.nf;
  g->rng = c->ipdf_rng;
  g->tab = static_cast<unsigned long long*>(c->ipdf_tab);
  return 0;
}
static void ipdf_plane_launch(hipStream_t s, const SfPlanes& pl, const IpdfArgs& g) {
  const int grid = pl.rows < IPDF_PLANE_GRID ? pl.rows : IPDF_PLANE_GRID;
  hipLaunchKernelGGL(k_ipdf_plane, dim3(grid), dim3(IPDF_PLANE_THREADS), 2 * sizeof(unsigned) * ipdf_words(g.nreal + g.phi, g.bins), s, pl, g);
}
// the vectors of a call on the device, from the context's staging copy
static int ipdf_put_vecs(nq_ctx* c, const Sf2Vec* v, int n, const double* proj) {
  for (int i = 0; i < n; ++i) c->ipdf_vecs_host[i] = v[i];
  HIPCHK(c, hipMemcpyAsync(c->ipdf_vecs, c->ipdf_vecs_host, sizeof(Sf2Vec) * n, hipMemcpyHostToDevice, c->stream));
  if (proj) {
    for (int i = 0; i < 2 * n; ++i) c->ipdf_proj_host[i] = proj[i];
    HIPCHK(c, hipMemcpyAsync(c->ipdf_proj, c->ipdf_proj_host, sizeof(double) * 2 * n, hipMemcpyHostToDevice, c->stream));
  }
  return 0;
}

int nq_increment_hist(nq_ctx* c, int nfields, const int* fields, int nsep, const int* seps, const double* lo, const double* hi, int bins, int accumulate) {
  static const char* fn = "nq_increment_hist";
  NQ_SINGLE_RANK(c, "nq_increment_hist");
  bool cplx[SF_MAX_FIELDS] = {};
  {
    const int rc = ipdf_check_fields(c, fn, nfields, fields, cplx);
    if (rc) return rc;
  }
  SfArgs a;
  int canon[SF_MAX_FIELDS] = {};
  if (const char* bad = sf_plan(c->N, nfields, cplx, nsep, seps, 0, nullptr, &a, canon)) NQ_FAIL(c, -1, "%s: %s", fn, bad);
  if (const char* bad = ipdf_check_ranges(nsep, nfields, lo, hi, bins)) NQ_FAIL(c, -1, "%s: %s", fn, bad);
  nq_ctx::IpdfCfg cfg;
  cfg.kind = 1;
  cfg.nf = nfields;
  cfg.n = nsep;
  cfg.bins = bins;
  for (int i = 0; i < nfields; ++i) cfg.fields[i] = fields[i];
  for (int s = 0; s < nsep; ++s) cfg.vecs[s] = seps[s];
  IpdfArgs g = {};
  {
    const int rc = ipdf_begin(c, fn, cfg, lo, hi, accumulate, &g);
    if (rc) return rc;
  }
  g.nsep = nsep;
  g.nreal = a.nreal;
  g.phi = a.phi;
  g.pa = g.pb = -1;
  for (int i = 0; i < nfields; ++i) g.out[canon[i]] = i;
  if (!c->kernel_family) {                              // planes: the separations as the vectors (r, 0)
    Sf2Vec v[SF_MAX_SEPS];
    for (int s = 0; s < nsep; ++s) v[s] = Sf2Vec{seps[s], 0, s, 0};
    {
      const int rc = ipdf_put_vecs(c, v, nsep, nullptr);
      if (rc) return rc;
    }
    g.vecs = c->ipdf_vecs;
    SfPlanes pl = {};
    {
      const int rc = sf2_planes_of(c, fn, nfields, fields, cplx, canon, a.nreal, a.phi, &pl);
      if (rc) return rc;
    }
    ipdf_plane_launch(c->stream, pl, g);
  } else {
    for (int s = 0; s < nsep; ++s) c->ipdf_seps_host[s] = seps[s];
    HIPCHK(c, hipMemcpyAsync(c->ipdf_seps, c->ipdf_seps_host, sizeof(int) * nsep, hipMemcpyHostToDevice, c->stream));
    g.seps = c->ipdf_seps;
    if (nfields <= flow_nv_of(c)) {
      FlowSel sel = flow_sel_none(c);
      for (int i = 0; i < nfields; ++i)
        if (!cplx[i]) sel.code[canon[i]] = fields[i];
      sel.phi = a.phi;
      launch_xflow_ipdf(c, sel, g);
    } else {
      for (int i = 0; i < nfields; ++i) {               // one field per launch, in the launch's slot 0, into its own part of the table
        FlowSel sel = flow_sel_none(c);
        IpdfArgs k = g;
        k.nreal = cplx[i] ? 0 : 1;
        k.phi = cplx[i] ? 1 : 0;
        k.out[0] = i;
        if (!cplx[i]) sel.code[0] = fields[i];
        sel.phi = k.phi;
        launch_xflow_ipdf(c, sel, k);
      }
    }
  }
  HIPCHK(c, hipGetLastError());
  ++cfg.samples;
  c->ipdf_cfg = cfg;
  return 0;
}

int nq_increment_hist2(nq_ctx* c, int nfields, const int* fields, int nvec, const int* vecs, const double* proj, int proj_a, int proj_b, const double* lo,
                       const double* hi, int bins, int accumulate) {
  static const char* fn = "nq_increment_hist2";
  NQ_SINGLE_RANK(c, "nq_increment_hist2");
  bool cplx[SF_MAX_FIELDS] = {};
  {
    const int rc = ipdf_check_fields(c, fn, nfields, fields, cplx);
    if (rc) return rc;
  }
  Sf2Args a;
  int canon[SF_MAX_FIELDS] = {};
  Sf2Vec sorted[SF2_MAX_VECS];
  if (const char* bad = sf2_plan(c->N, c->N, nfields, cplx, nvec, vecs, proj, proj_a, proj_b, 0, nullptr, &a, canon, sorted)) NQ_FAIL(c, -1, "%s: %s", fn, bad);
  if (const char* bad = ipdf_check_ranges(nvec, nfields, lo, hi, bins)) NQ_FAIL(c, -1, "%s: %s", fn, bad);
  nq_ctx::IpdfCfg cfg;
  cfg.kind = 2;
  cfg.nf = nfields;
  cfg.n = nvec;
  cfg.bins = bins;
  cfg.pa = proj_a;
  cfg.pb = proj_b;
  cfg.has_proj = proj != nullptr;
  for (int i = 0; i < nfields; ++i) cfg.fields[i] = fields[i];
  for (int i = 0; i < 2 * nvec; ++i) cfg.vecs[i] = vecs[i];
  for (int i = 0; proj && i < 2 * nvec; ++i) cfg.proj[i] = proj[i];
  IpdfArgs g = {};
  {
    int rc = ipdf_begin(c, fn, cfg, lo, hi, accumulate, &g);
    if (!rc) rc = ipdf_put_vecs(c, sorted, nvec, proj);
    if (rc) return rc;
  }
  g.nsep = nvec;
  g.vecs = c->ipdf_vecs;
  g.proj = proj ? c->ipdf_proj : nullptr;
  g.nreal = a.nreal;
  g.phi = a.phi;
  g.pa = a.pa;
  g.pb = a.pb;
  for (int i = 0; i < nfields; ++i) g.out[canon[i]] = i;
  SfPlanes pl = {};
  {
    const int rc = sf2_planes_of(c, fn, nfields, fields, cplx, canon, a.nreal, a.phi, &pl);
    if (rc) return rc;
  }
  ipdf_plane_launch(c->stream, pl, g);
  HIPCHK(c, hipGetLastError());
  ++cfg.samples;
  c->ipdf_cfg = cfg;
  return 0;
}

int nq_increment_hist_read(nq_ctx* c, long long* samples, unsigned long long* out) {
  NQ_SINGLE_RANK(c, "nq_increment_hist_read");
  if (!samples || !out) NQ_FAIL(c, -1, "nq_increment_hist_read: null output");
  const nq_ctx::IpdfCfg& g = c->ipdf_cfg;
  if (!c->ipdf_tab || g.nf == 0) NQ_FAIL(c, -4, "nq_increment_hist_read: no nq_increment_hist or nq_increment_hist2 call yet");
  HIPCHK(c, hipSetDevice(c->device));
  *samples = g.samples;
  HIPCHK(c, hipMemcpyAsync(out, c->ipdf_tab, sizeof(unsigned long long) * g.n * g.nf * (g.bins + 3), hipMemcpyDeviceToHost, c->stream));
  return nq_sync(c);
}

// ---- vortex census (csrc/nq_vortex.hpp) --------------------------------------------------------------------
static_assert(VX_BELOW == NQ_VX_BELOW && VX_ABOVE == NQ_VX_ABOVE && VX_ABS_ABOVE == NQ_VX_ABS_ABOVE && VX_BASE_COLS == NQ_VX_COLS &&
              VX_MAX_FIELDS == SF_MAX_FIELDS && VX_INFO == 7, "public constants of nq_vortex_census and the kernels'");
// the device buffers of a census on planes of (rows, cols): two int32 planes, the small buffers, the table
struct VxBufs {
  int *L, *R, *rowroots, *rowset, *rowoff;
  double* part;
  VxRange* rng;
  long long* info;
  unsigned long long* tab;
};
static size_t vx_planes_bytes(int rows, int cols) { return 2 * sizeof(int) * (size_t)rows * cols; }
static size_t vx_small_bytes(int rows) {
  return sizeof(double) * VX_RANGE_GRID * VX_MAX_FIELDS * VX_RANGE_COLS + sizeof(VxRange) + sizeof(long long) * VX_INFO + 3 * sizeof(int) * (size_t)rows;
}
static size_t vx_tab_bytes(int cap) { return sizeof(unsigned long long) * (size_t)cap * (VX_BASE_COLS + VX_MAX_FIELDS); }
static VxBufs vx_bufs(void* planes, void* small, void* tab, int rows, int cols) {
  VxBufs b;
  b.L = static_cast<int*>(planes);
  b.R = b.L + (size_t)rows * cols;
  b.part = static_cast<double*>(small);
  b.rng = reinterpret_cast<VxRange*>(b.part + VX_RANGE_GRID * VX_MAX_FIELDS * VX_RANGE_COLS);
  b.info = reinterpret_cast<long long*>(b.rng + 1);
  b.rowroots = reinterpret_cast<int*>(b.info + VX_INFO);
  b.rowset = b.rowroots + rows;
  b.rowoff = b.rowset + rows;
  b.tab = static_cast<unsigned long long*>(tab);
  return b;
}
static_assert(sizeof(VxRange) % 8 == 0, "the small buffers stay 8-byte aligned");
static const char* vx_check_call(int crit, int nfields, int mode, double threshold, int connectivity, int capacity) {
  if (crit < 0 || crit >= nfields) return "crit is an index into the field list";
  if (mode != NQ_VX_BELOW && mode != NQ_VX_ABOVE && mode != NQ_VX_ABS_ABOVE) return "mode is NQ_VX_BELOW, NQ_VX_ABOVE or NQ_VX_ABS_ABOVE";
  if (!std::isfinite(threshold)) return "the threshold is not finite";
  if (connectivity != 4 && connectivity != 8) return "connectivity is 4 or 8";
  if (capacity < 1 || capacity > NQ_VX_MAX_CAPACITY) return "capacity outside [1, NQ_VX_MAX_CAPACITY]";
  return nullptr;
}
// the range pass: min, max, sums and scales of every plane of the call into b.rng, the non-finite count and the scales into b.info
static void vx_range_launch(hipStream_t s, const VxPlanes& pl, const VxBufs& b) {
  const int nblk = pl.rows < VX_RANGE_GRID ? pl.rows : VX_RANGE_GRID;
  int lg = 0;
  while (((size_t)1 << lg) < (size_t)pl.rows * pl.cols) ++lg;
  hipLaunchKernelGGL(k_vx_range, dim3(nblk), dim3(VX_THREADS), 0, s, pl, b.part);
  hipLaunchKernelGGL(k_vx_scale, dim3(1), dim3(64 * VX_RANGE_COLS), 0, s, (const double*)b.part, nblk, pl.nf, lg, b.rng, b.info);
}
// every phase of one census, in stream order; nothing is copied, the host does not wait
// (ev, for nq_vortex_profile: VX_PHASES + 1 events, ev[0] recorded by the caller; ev[k + 1] closes phase k: range, rows, merge,
// flatten + prefix + rank, sums + finish)
constexpr int VX_PHASES = 5;
static void vx_census_launch(hipStream_t s, const VxPlanes& pl, int mode, double thr, int conn, int cap, const VxBufs& b, hipEvent_t* ev = nullptr) {
  const int ncols = VX_BASE_COLS + pl.nf, rows = pl.rows, cols = pl.cols;
  vx_range_launch(s, pl, b);
  if (ev) (void)hipEventRecord(ev[1], s);
  hipLaunchKernelGGL(k_vx_rows, dim3(rows), dim3(VX_THREADS), 0, s, pl, mode, thr, b.L);
  if (ev) (void)hipEventRecord(ev[2], s);
  hipLaunchKernelGGL(k_vx_merge, dim3(rows), dim3(VX_THREADS), 0, s, rows, cols, conn, b.L);
  if (ev) (void)hipEventRecord(ev[3], s);
  hipLaunchKernelGGL(k_vx_flatten, dim3(rows), dim3(VX_THREADS), 0, s, cols, b.L, b.rowroots, b.rowset);
  hipLaunchKernelGGL(k_vx_prefix, dim3(1), dim3(VX_THREADS), 0, s, rows, cap, (const int*)b.rowroots, (const int*)b.rowset, b.rowoff, b.info);
  hipLaunchKernelGGL(k_vx_rank, dim3(rows), dim3(VX_THREADS), 0, s, cols, cap, ncols, (const int*)b.L, (const int*)b.rowoff, b.R, b.tab);
  if (ev) (void)hipEventRecord(ev[4], s);
  hipLaunchKernelGGL(k_vx_sums, dim3(rows), dim3(VX_THREADS), 0, s, pl, cap, ncols, (const int*)b.L, (const int*)b.R, (const VxRange*)b.rng, b.tab);
  const int fin = (cap + VX_THREADS - 1) / VX_THREADS;
  hipLaunchKernelGGL(k_vx_finish, dim3(fin < 1024 ? fin : 1024), dim3(VX_THREADS), 0, s, ncols, (const long long*)b.info, b.tab);
  if (ev) (void)hipEventRecord(ev[5], s);
}
// the fields of a call (real fields only) and the state: nq_structure2's checks without NQ_SF_PHI
static int vx_check_fields(nq_ctx* c, const char* fn, int nfields, const int* fields) {
  if (!fields || nfields < 1 || nfields > VX_MAX_FIELDS) NQ_FAIL(c, -1, "%s: %d fields (1 to %d)", fn, nfields, VX_MAX_FIELDS);
  for (int i = 0; i < nfields; ++i) {
    if (fields[i] == NQ_SF_PHI) NQ_FAIL(c, -1, "%s: NQ_SF_PHI is complex: a census thresholds and sums real fields (NQ_PDF_PHI2 is |phi|^2; DESIGN.md section 7)", fn);
    if (is_flow(fields[i]) && !c->kernel_family)
      NQ_FAIL(c, -1, "%s: field %d (NQ_FLOW_*) on a QGModel context: its plane route has q and its passive scalar only (DESIGN.md section 7)", fn, fields[i]);
    if (!is_flow(fields[i]) && hist_slot(c, fields[i]) < 0)
      NQ_FAIL(c, -1, "%s: field %d is not available here (Kernel family: NQ_PDF_Q, NQ_PDF_QPSI, NQ_PDF_PHI2 and the NQ_FLOW_* fields; QGModel: NQ_PDF_Q, with its passive scalar NQ_PDF_C)", fn, fields[i]);
    for (int k = 0; k < i; ++k)
      if (fields[k] == fields[i]) NQ_FAIL(c, -1, "%s: field %d listed twice", fn, fields[i]);
  }
  if (c->kernel_family ? !c->have_phi : !c->have_q) NQ_FAIL(c, -4, "%s: %s has not been called", fn, c->kernel_family ? "set_phi" : "set_q");
  return 0;
}
// the feature's own buffers for this capacity: all of what is missing or too small, or none of it and -5 (the old buffers stay)
// (cap = 0, a range call: the small buffers only.  The context's small buffers are two sets: the census's, then the range call's,
// so that a range call leaves the scales and counts of the last census alone.)
static int vx_reserve(nq_ctx* c, const char* fn, int cap) {
  void** slot[3] = {&c->vx_planes, &c->vx_small, &c->vx_tab};
  size_t* have[3] = {&c->vx_planes_bytes, &c->vx_small_bytes, &c->vx_tab_bytes};
  const size_t need[3] = {cap ? vx_planes_bytes(c->N, c->N) : 0, 2 * vx_small_bytes(c->N), cap ? vx_tab_bytes(cap) : 0};
  void* fresh[3] = {nullptr, nullptr, nullptr};
  for (int i = 0; i < 3; ++i) {
    if (need[i] <= *have[i]) continue;
    if (hipMalloc(&fresh[i], need[i]) != hipSuccess) {
      (void)hipGetLastError();
      for (int k = 0; k < i; ++k)
        if (fresh[k]) (void)hipFree(fresh[k]);
      NQ_FAIL(c, -5, "%s: cannot allocate %zu bytes of device memory", fn, need[i]);
    }
  }
  for (int i = 0; i < 3; ++i) {
    if (!fresh[i]) continue;
    if (*slot[i]) {
      const int rc = nq_sync(c);                          // a launch of the last call may still use it
      if (rc) {
        for (int k = i; k < 3; ++k)
          if (fresh[k]) (void)hipFree(fresh[k]);
        return rc;
      }
      for (size_t k = 0; k < c->allocs.size(); ++k)
        if (c->allocs[k] == *slot[i]) {
          c->allocs.erase(c->allocs.begin() + k);
          break;
        }
      (void)hipFree(*slot[i]);
      c->bytes -= (long long)*have[i];
      c->vx_cfg = nq_ctx::VxCfg();                        // what the old buffer held is gone
    }
    c->allocs.push_back(fresh[i]);
    c->bytes += (long long)need[i];
    *slot[i] = fresh[i];
    *have[i] = need[i];
  }
  return 0;
}
static int vx_planes_for(nq_ctx* c, const char* fn, int nfields, const int* fields, int crit, VxPlanes* out) {
  const bool cplx[SF_MAX_FIELDS] = {};
  const int canon[SF_MAX_FIELDS] = {0, 1, 2};
  SfPlanes sp = {};
  const int rc = sf2_planes_of(c, fn, nfields, fields, cplx, canon, nfields, 0, &sp);
  if (rc) return rc;
  VxPlanes pl = {};
  for (int i = 0; i < nfields; ++i) {
    pl.p[i] = sp.p[i];
    pl.stride[i] = sp.stride[i];
  }
  pl.nf = nfields;
  pl.crit = crit;
  pl.rows = sp.rows;
  pl.cols = sp.cols;
  *out = pl;
  return 0;
}

int nq_vortex_range(nq_ctx* c, int nfields, const int* fields, double* out) {
  static const char* fn = "nq_vortex_range";
  NQ_SINGLE_RANK(c, "nq_vortex_range");
  {
    const int rc = vx_check_fields(c, fn, nfields, fields);
    if (rc) return rc;
  }
  if (!out) NQ_FAIL(c, -1, "%s: null output", fn);
  HIPCHK(c, hipSetDevice(c->device));
  {
    const int rc = vx_reserve(c, fn, 0);
    if (rc) return rc;
  }
  VxPlanes pl;
  {
    const int rc = vx_planes_for(c, fn, nfields, fields, 0, &pl);
    if (rc) return rc;
  }
  VxBufs b = vx_bufs(c->vx_small, static_cast<char*>(c->vx_small) + vx_small_bytes(c->N), nullptr, 0, 0);   // the second set
  b.L = b.R = nullptr;                                    // a range call has no planes, table or per-row counts
  b.rowroots = b.rowset = b.rowoff = nullptr;
  vx_range_launch(c->stream, pl, b);
  HIPCHK(c, hipGetLastError());
  VxRange r;
  HIPCHK(c, hipMemcpyAsync(&r, b.rng, sizeof(r), hipMemcpyDeviceToHost, c->stream));
  {
    const int rc = nq_sync(c);
    if (rc) return rc;
  }
  for (int f = 0; f < nfields; ++f)
    for (int k = 0; k < 4; ++k) out[4 * f + k] = r.v[f][k];
  return 0;
}

static int vx_census(nq_ctx* c, const char* fn, int nfields, const int* fields, int crit, int mode, double threshold, int connectivity, int capacity, double* ms);
int nq_vortex_census(nq_ctx* c, int nfields, const int* fields, int crit, int mode, double threshold, int connectivity, int capacity) {
  NQ_SINGLE_RANK(c, "nq_vortex_census");
  return vx_census(c, "nq_vortex_census", nfields, fields, crit, mode, threshold, connectivity, capacity, nullptr);
}
// the same census, synchronous, with device events between its phases: ms[0] the planes (store pass or QGModel's transforms), then
// range, rows, merge, flatten + rank, sums
int nq_vortex_profile(nq_ctx* c, int nfields, const int* fields, int crit, int mode, double threshold, int connectivity, int capacity, double* ms) {
  NQ_SINGLE_RANK(c, "nq_vortex_profile");
  if (!ms) NQ_FAIL(c, -1, "nq_vortex_profile: null output");
  return vx_census(c, "nq_vortex_profile", nfields, fields, crit, mode, threshold, connectivity, capacity, ms);
}
static int vx_census(nq_ctx* c, const char* fn, int nfields, const int* fields, int crit, int mode, double threshold, int connectivity, int capacity, double* ms) {
  {
    const int rc = vx_check_fields(c, fn, nfields, fields);
    if (rc) return rc;
  }
  if (const char* bad = vx_check_call(crit, nfields, mode, threshold, connectivity, capacity)) NQ_FAIL(c, -1, "%s: %s", fn, bad);
  HIPCHK(c, hipSetDevice(c->device));
  {
    const int rc = vx_reserve(c, fn, capacity);
    if (rc) return rc;
  }
  hipEvent_t ev[VX_PHASES + 2] = {};
  int made = 0, rc = 0;
  if (ms) {
    while (made < VX_PHASES + 2 && hipEventCreate(&ev[made]) == hipSuccess) ++made;
    if (made < VX_PHASES + 2 || hipEventRecord(ev[0], c->stream) != hipSuccess) {
      (void)hipGetLastError();
      rc = -5;
    }
  }
  VxPlanes pl;
  if (!rc) rc = vx_planes_for(c, fn, nfields, fields, crit, &pl);
  if (!rc) {
    if (ms) (void)hipEventRecord(ev[1], c->stream);
    c->vx_cfg.census = false;
    vx_census_launch(c->stream, pl, mode, threshold, connectivity, capacity, vx_bufs(c->vx_planes, c->vx_small, c->vx_tab, c->N, c->N), ms ? ev + 1 : nullptr);
    if (hipGetLastError() != hipSuccess) rc = -5;
  }
  if (!rc) {
    c->vx_cfg.nf = nfields;
    c->vx_cfg.cap = capacity;
    c->vx_cfg.census = true;
    if (ms) rc = nq_sync(c);
  }
  if (ms) {
    for (int i = 0; !rc && i <= VX_PHASES; ++i) {
      float t = 0.f;
      if (hipEventElapsedTime(&t, ev[i], ev[i + 1]) != hipSuccess) rc = -5;
      ms[i] = t;
    }
    for (int i = 0; i < made; ++i) (void)hipEventDestroy(ev[i]);
  }
  if (rc == -5 && c->err.empty()) NQ_FAIL(c, -5, "%s: a launch or an event failed", fn);
  return rc;
}

int nq_vortex_stats(nq_ctx* c, double* out) {
  NQ_SINGLE_RANK(c, "nq_vortex_stats");
  if (!out) NQ_FAIL(c, -1, "nq_vortex_stats: null output");
  if (!c->vx_cfg.census) NQ_FAIL(c, -4, "nq_vortex_stats: no nq_vortex_census call yet");
  HIPCHK(c, hipSetDevice(c->device));
  VxRange r;
  HIPCHK(c, hipMemcpyAsync(&r, vx_bufs(c->vx_planes, c->vx_small, c->vx_tab, c->N, c->N).rng, sizeof(r), hipMemcpyDeviceToHost, c->stream));
  {
    const int rc = nq_sync(c);
    if (rc) return rc;
  }
  for (int f = 0; f < c->vx_cfg.nf; ++f)
    for (int k = 0; k < 4; ++k) out[4 * f + k] = r.v[f][k];
  return 0;
}

int nq_vortex_read(nq_ctx* c, long long* info, long long* table) {
  NQ_SINGLE_RANK(c, "nq_vortex_read");
  if (!info) NQ_FAIL(c, -1, "nq_vortex_read: null info");
  if (!c->vx_cfg.census) NQ_FAIL(c, -4, "nq_vortex_read: no nq_vortex_census call yet");
  HIPCHK(c, hipSetDevice(c->device));
  const VxBufs b = vx_bufs(c->vx_planes, c->vx_small, c->vx_tab, c->N, c->N);
  HIPCHK(c, hipMemcpyAsync(info, b.info, sizeof(long long) * VX_INFO, hipMemcpyDeviceToHost, c->stream));
  {
    const int rc = nq_sync(c);
    if (rc) return rc;
  }
  if (table && info[1] > 0) {
    HIPCHK(c, hipMemcpyAsync(table, b.tab, sizeof(long long) * (size_t)info[1] * (VX_BASE_COLS + c->vx_cfg.nf), hipMemcpyDeviceToHost, c->stream));
    return nq_sync(c);
  }
  return 0;
}

int nq_vortex_labels(nq_ctx* c, int* out) {
  NQ_SINGLE_RANK(c, "nq_vortex_labels");
  if (!out) NQ_FAIL(c, -1, "nq_vortex_labels: null output");
  if (!c->vx_cfg.census) NQ_FAIL(c, -4, "nq_vortex_labels: no nq_vortex_census call yet");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(out, c->vx_planes, sizeof(int) * (size_t)c->N * c->N, hipMemcpyDeviceToHost, c->stream));
  return nq_sync(c);
}

// ---- isotropic spectra of the diagnostics tick ----------------------------------------------------
int nq_spectrum_shells(const nq_ctx* c) { return c ? nq_shell_count(c->N) : -1; }

// out[s * nb + b]: the terms nq_diagnostics adds into sum s, summed over the wavenumbers of shell b.  Binned: the Kernel family's
// [0..3], [6..14], [24], [27], [28], [31]; QGModel's [6..14] and, with its passive scalar, [16..19]; every other row is zero.
// The same passes as the tick (the two products passes included, so its side effects are the tick's), the binning kernels in
// place of the workgroup sums.
// this context's local columns: allocate, zero, and bin the spectral rows ([0..3], [6..14], [16..19]) into spec_out
// (*qh_binned, when asked for: the q-hat that was binned -- on dual-copy contexts the mean in the scratch plane)
static int bin_local_spectral(nq_ctx* x, int nb, const cd** qh_binned = nullptr) {
  const int N = x->N;
  const bool waves = x->kernel_family;
  if (!x->spec_out) ALLOC(x, x->spec_out, (size_t)32 * nb);
  if (waves && !x->spec_r) ALLOC(x, x->spec_r, (size_t)2 * N * x->Wf);
  double* d = x->spec_out;
  HIPCHK(x, hipMemsetAsync(d, 0, sizeof(double) * 32 * nb, x->stream));
  const cd* qh = x->q.y[x->q.cur];
  SLABTRY(mean_qh(x, &qh));                           // as the tick
  if (qh_binned) *qh_binned = qh;
  if (waves && x->Wf > 0) {
    const BinPhi t{(const cd*)x->w.y[x->w.cur], x->Wf, x->kk, x->ll};
    hipLaunchKernelGGL(k_bin_shells<BinPhi>, dim3(nb), dim3(256), 0, x->stream, t, N, nb, 1, x->kf0, x->Wf, d);
  }
  if (x->Wh > 0) {
    const BinQ t{qh, (const cd*)(x->p.model == NQ_MODEL_COUPLED ? x->qwh : nullptr), (const cd*)x->ph, N, x->Ph, x->kk, x->ll,
                 (const cd*)(x->dual ? x->q.y[x->q.cur] : nullptr), (const cd*)(x->dual ? x->q2.y[x->q2.cur] : nullptr),
                 (const double*)(x->dual ? x->filt_h : nullptr), (const double*)(x->dual ? x->filt_m : nullptr),
                 (const cd*)(x->pass ? x->qp.y[x->qp.cur] : nullptr)};
    hipLaunchKernelGGL(k_bin_shells<BinQ>, dim3(nb), dim3(256), 0, x->stream, t, N, nb, 0, x->kh0, x->Wh, d + (size_t)6 * nb);
    if (!waves && x->passive) {
      const BinC tc{(const cd*)x->cq.y[x->cq.cur], N, x->Ph, x->kk, x->ll};
      hipLaunchKernelGGL(k_bin_shells<BinC>, dim3(nb), dim3(256), 0, x->stream, tc, N, nb, 0, x->kh0, x->Wh, d + (size_t)16 * nb);
    }
  }
  return 0;
}
// after the products pass `which` (0: J, 1: i F[phi q_psi]) and its A sub-pass: rows 24 + 4 which .. 27 + 4 which
static void bin_local_project(nq_ctx* x, int nb, int which) {
  double *rl = x->spec_r, *rd = x->spec_r + (size_t)x->N * x->Wf;
  launch_project_bin(x, rl, rd);
  const BinProj t{rl, rd, x->Wf};
  hipLaunchKernelGGL(k_bin_shells<BinProj>, dim3(nb), dim3(256), 0, x->stream, t, x->N, nb, 1, x->kf0, x->Wf, x->spec_out + (size_t)(24 + 4 * which) * nb);
}

// every context bins its own columns, the products passes exchange as the tick's do (the device part: nothing is downloaded and
// the host does not wait; every context's spec_out is complete in stream order), and the contexts are summed in rank order on the host
static int tick_binned_device(std::vector<nq_ctx*>& grp, const char* fn, int nb) {
  SLABTRY(tick_need_phi(grp, fn));
  SLABTRY(slab_settle(grp));
  for (nq_ctx* x : each(grp)) SLABTRY(bin_local_spectral(x, nb));
  if (grp[0]->kernel_family) {
    // [24], [27] from F[u phix + v phiy], [28], [31] from i F[phi q_psi]: the tick's two products passes
    for (int which = 0; which < 2; ++which) {
      for (nq_ctx* x : each(grp)) launch_products_pass(x, which);
      SLABTRY(exchange_now(grp, 0, true));
      for (nq_ctx* x : each(grp)) {
        launch_A_m(x, false, {&x->mW});
        if (x->Wf > 0) bin_local_project(x, nb, which);
      }
    }
  }
  return 0;
}
static int tick_binned(std::vector<nq_ctx*>& grp, const char* fn, int nb, double* out) {
  SLABTRY(tick_binned_device(grp, fn, nb));
  return sum_ranks_on_host(grp, &nq_ctx::spec_out, (size_t)32 * nb, out);
}
int nq_diagnostics_binned(nq_ctx* c, int nb, double* out) {
  NQ_SINGLE_RANK(c, "nq_diagnostics_binned");
  if (!out) NQ_FAIL(c, -1, "nq_diagnostics_binned: null output");
  if (nb != nq_shell_count(c->N)) NQ_FAIL(c, -1, "nq_diagnostics_binned: nb = %d, the grid has %d shells", nb, nq_shell_count(c->N));
  std::vector<nq_ctx*> grp(1, c);
  return tick_binned(grp, "nq_diagnostics_binned", nb, out);
}
// the same on a slab-decomposed simulation (collective, like nq_slab_diagnostics): the contexts of this process are summed
// (peers: all ranks -- the whole result; one rank per process: that rank's part, which the caller gathers and sums in rank order)
int nq_slab_diagnostics_binned(nq_ctx* c, int nb, double* out) {
  if (!c || !out) return -1;
  if (nb != nq_shell_count(c->N)) NQ_FAIL(c, -1, "nq_slab_diagnostics_binned: nb = %d, the grid has %d shells", nb, nq_shell_count(c->N));
  std::vector<nq_ctx*> grp;
  SLABTRY(slab_group(c, &grp));
  return tick_binned(grp, "nq_slab_diagnostics_binned", nb, out);
}

// ---- spectral transfer -----------------------------------------------------------------------------
// The tick's two products passes again: the first (c_J = 1, c_R = 0) gives F[u q], F[v q] (F[u c], F[v c] with QGModel's passive
// scalar) and the J plane, the second (0, 1) the R plane.  Each is B-transformed into a scratch plane and binned against the
// state's spectrum by k_bin_shells (BinTrQ, BinTrC, BinTrW).  Planes: scr_h0, scr_h1, scr_f0 on one rank (scr_f1: the mean of the
// two q copies), tr_h, tr_f (scr_h1: the mean) on slab ranks, allocated on the first call.
struct TrPlanes {
  cd *h0, *h1, *f;
  const cd* qh;
};
// qh_mean: the q-hat a caller has formed already (tick_both_device: what bin_local_spectral binned); null: formed here
static int transfer_begin(nq_ctx* x, int nb, TrPlanes* t, const cd* qh_mean = nullptr) {
  const int N = x->N;
  if (!x->tr_out) ALLOC(x, x->tr_out, (size_t)NQ_TRANSFER_ROWS * nb);
  HIPCHK(x, hipMemsetAsync(x->tr_out, 0, sizeof(double) * NQ_TRANSFER_ROWS * nb, x->stream));
  if (x->P == 1) {
    t->h0 = x->scr_h0;
    t->h1 = x->scr_h1;
    t->f = x->scr_f0;
  } else {
    if (!x->ybj && !x->tr_h) ALLOC(x, x->tr_h, (size_t)2 * N * x->Ph);
    if (x->kernel_family && !x->tr_f) ALLOC(x, x->tr_f, (size_t)N * x->Wf);
    t->h0 = x->tr_h;
    t->h1 = x->tr_h ? x->tr_h + (size_t)N * x->Ph : nullptr;
    t->f = x->tr_f;
  }
  t->qh = qh_mean ? qh_mean : x->q.y[x->q.cur];
  if (!x->ybj && !qh_mean) SLABTRY(mean_qh(x, &t->qh));           // the q-hat the tick bins
  return 0;
}
// after the products pass `which` (0: J and the balanced / scalar products, 1: R) and its exchange: A sub-pass (transfer_A),
// then B into the scratch planes and the bins into tr_out (transfer_B_bin); Mw stays as the A sub-pass left it
static void transfer_A(nq_ctx* x, int which) {
  const bool waves = x->kernel_family, balanced = !x->ybj, passive = !waves && x->passive;
  if (which != 0) launch_A_m(x, false, {&x->mW});
  else if (waves && balanced) launch_A_m(x, false, {&x->mUq, &x->mVq, &x->mW});
  else if (waves) launch_A_m(x, false, {&x->mW});
  else if (passive) launch_A_m(x, false, {&x->mUq, &x->mVq, &x->mUc, &x->mVc});
  else launch_A_m(x, false, {&x->mUq, &x->mVq});
}
static void transfer_B_bin(nq_ctx* x, int nb, int which, const TrPlanes& t) {
  const int N = x->N;
  const bool waves = x->kernel_family, balanced = !x->ybj, passive = !waves && x->passive;
  double* d = x->tr_out;
  if (which == 0) {
    if (balanced && x->Wh > 0) {
      launch_B_p(x, false, x->mUq.ys, x->mUq.pitch, t.h0, x->Ph, x->Wh, 1.0);
      launch_B_p(x, false, x->mVq.ys, x->mVq.pitch, t.h1, x->Ph, x->Wh, 1.0);
      const BinTrQ bq{HalfJac{t.h0, t.h1, N, x->Ph, x->kk, x->ll}, (const cd*)x->ph, t.qh};
      hipLaunchKernelGGL(k_bin_shells<BinTrQ>, dim3(nb), dim3(256), 0, x->stream, bq, N, nb, 0, x->kh0, x->Wh, d);
    }
    if (passive && x->Wh > 0) {
      launch_B_p(x, false, x->mUc.ys, x->mUc.pitch, t.h0, x->Ph, x->Wh, 1.0);
      launch_B_p(x, false, x->mVc.ys, x->mVc.pitch, t.h1, x->Ph, x->Wh, 1.0);
      const BinTrC bc{HalfJac{t.h0, t.h1, N, x->Ph, x->kk, x->ll}, (const cd*)x->cq.y[x->cq.cur]};
      hipLaunchKernelGGL(k_bin_shells<BinTrC>, dim3(nb), dim3(256), 0, x->stream, bc, N, nb, 0, x->kh0, x->Wh, d + (size_t)4 * nb);
    }
  }
  if (waves && x->Wf > 0) {
    launch_B_p(x, false, x->mW.ys, x->mW.pitch, t.f, x->Wf, x->Wf, 1.0);
    const BinTrW bw{(const cd*)x->w.y[x->w.cur], t.f, x->Wf};
    hipLaunchKernelGGL(k_bin_shells<BinTrW>, dim3(nb), dim3(256), 0, x->stream, bw, N, nb, 1, x->kf0, x->Wf, d + (size_t)(2 + which) * nb);
  }
}
static void transfer_bin_pass(nq_ctx* x, int nb, int which, const TrPlanes& t) {
  transfer_A(x, which);
  transfer_B_bin(x, nb, which, t);
}

// the device part: every context's tr_out is complete in stream order, nothing is downloaded and the host does not wait
static int tick_transfer_device(std::vector<nq_ctx*>& grp, const char* fn, int nb) {
  SLABTRY(tick_need_phi(grp, fn));
  SLABTRY(slab_settle(grp));
  std::vector<TrPlanes> t(grp.size());
  for (size_t r = 0; r < grp.size(); ++r) {
    HIPCHK(grp[r], hipSetDevice(grp[r]->device));
    SLABTRY(transfer_begin(grp[r], nb, &t[r]));
  }
  for (int which = 0; which < (grp[0]->kernel_family ? 2 : 1); ++which) {
    for (nq_ctx* x : each(grp)) {
      set_window(x, 0, 1);
      launch_products_pass(x, which);
    }
    SLABTRY(exchange_now(grp, 0, true));
    for (size_t r = 0; r < grp.size(); ++r) {
      HIPCHK(grp[r], hipSetDevice(grp[r]->device));
      transfer_bin_pass(grp[r], nb, which, t[r]);
    }
  }
  return 0;
}
static int tick_transfer(std::vector<nq_ctx*>& grp, const char* fn, int nb, double* out) {
  SLABTRY(tick_transfer_device(grp, fn, nb));
  return sum_ranks_on_host(grp, &nq_ctx::tr_out, (size_t)NQ_TRANSFER_ROWS * nb, out);
}
// Both tables of one single-rank context from ONE run of each products pass (the samples of nq_tspec_attach with both bodies;
// DESIGN.md section 5n).  spec_out and tr_out end up bit for bit what the two calls above leave there one after the other:
// the window is the whole slab either way on one rank, the mean of the two q-hat copies is formed once and serves both, the A
// sub-pass over the transfer's list transforms Mw exactly as the one over Mw alone does (one workgroup column per array), and
// k_s_project_bin only reads Mw, so the B pass finds it as the A sub-pass left it.
static int tick_both_device(nq_ctx* x, const char* fn, int nb) {
  std::vector<nq_ctx*> grp(1, x);
  SLABTRY(tick_need_phi(grp, fn));
  SLABTRY(slab_settle(grp));
  const cd* qh = nullptr;
  SLABTRY(bin_local_spectral(x, nb, &qh));
  TrPlanes t;
  SLABTRY(transfer_begin(x, nb, &t, x->dual ? qh : nullptr));
  const bool waves = x->kernel_family;
  for (int which = 0; which < (waves ? 2 : 1); ++which) {
    set_window(x, 0, 1);
    launch_products_pass(x, which);
    SLABTRY(exchange_now(grp, 0, true));
    transfer_A(x, which);
    if (waves && x->Wf > 0) bin_local_project(x, nb, which);
    transfer_B_bin(x, nb, which, t);
  }
  return 0;
}
int nq_transfer_binned(nq_ctx* c, int nb, double* out) {
  NQ_SINGLE_RANK(c, "nq_transfer_binned");
  if (!out) NQ_FAIL(c, -1, "nq_transfer_binned: null output");
  if (nb != nq_shell_count(c->N)) NQ_FAIL(c, -1, "nq_transfer_binned: nb = %d, the grid has %d shells", nb, nq_shell_count(c->N));
  std::vector<nq_ctx*> grp(1, c);
  return tick_transfer(grp, "nq_transfer_binned", nb, out);
}
// collective, as nq_slab_diagnostics_binned: every context bins its own columns, the contexts of this process summed in rank order
int nq_slab_transfer_binned(nq_ctx* c, int nb, double* out) {
  if (!c || !out) return -1;
  if (nb != nq_shell_count(c->N)) NQ_FAIL(c, -1, "nq_slab_transfer_binned: nb = %d, the grid has %d shells", nb, nq_shell_count(c->N));
  std::vector<nq_ctx*> grp;
  SLABTRY(slab_group(c, &grp));
  return tick_transfer(grp, "nq_slab_transfer_binned", nb, out);
}

// ---- coarse-grained flux maps ---------------------------------------------------------------------------
// The tick's first products pass again, B-transformed into the scratch planes as the transfer does; then per filter scale
// k_s_coarse into the context's own spectral planes, the inverse column passes into its own mixed-space planes, k_x_coarse.
static int coarse_model_mask(const nq_ctx* c) { return !c->kernel_family ? (CG_KE | CG_ENS) : c->ybj ? CG_NIW : (CG_KE | CG_ENS | CG_NIW); }
// every buffer of `want`, zeroed, owned by the context and counted by nq_device_bytes -- or none of them and -5
static int alloc_all_or_none(nq_ctx* c, std::vector<std::pair<void**, size_t>>& want, const char* fn) {
  size_t got = 0, total = 0;
  for (; got < want.size(); ++got) {
    if (hipMalloc(want[got].first, want[got].second) != hipSuccess) break;
    total += want[got].second;
  }
  if (got < want.size()) {
    (void)hipGetLastError();
    const size_t bytes = want[got].second;
    for (size_t i = 0; i <= got && i < want.size(); ++i) {
      if (i < got) (void)hipFree(*want[i].first);
      *want[i].first = nullptr;
    }
    NQ_FAIL(c, -5, "%s: cannot allocate %zu bytes of device memory", fn, bytes);
  }
  for (auto& w : want) {
    HIPCHK(c, hipMemsetAsync(*w.first, 0, w.second, c->stream));
    c->allocs.push_back(*w.first);
  }
  c->bytes += (long long)total;
  return 0;
}
// the planes of the first call (and the map planes of the first call that asks for maps): all of them or none
static int coarse_reserve(nq_ctx* c, int nb, bool maps) {
  nq_ctx::Coarse& k = c->cg;
  const size_t N = (size_t)c->N, half = N * c->Ph * sizeof(cd), full = N * N * sizeof(cd);
  std::vector<std::pair<void**, size_t>> want;
  if (!k.ready) {
    for (int i = 0; i < (c->ybj ? 2 : 6); ++i) {
      want.push_back({(void**)&k.sh[i], half});
      want.push_back({(void**)&k.mh[i], half});
    }
    for (int i = 0; i < (c->kernel_family ? 3 : 0); ++i) {
      want.push_back({(void**)&k.sf[i], full});
      want.push_back({(void**)&k.mf[i], full});
    }
    want.push_back({(void**)&k.g, sizeof(double) * NQ_CG_MAX_SCALES * nb});
    want.push_back({(void**)&k.part, sizeof(double) * 6 * N});
    want.push_back({(void**)&k.mom, sizeof(double) * 6 * NQ_CG_MAX_SCALES});
  }
  if (maps && !k.have_maps)
    for (int m = 0; m < 3; ++m)
      if (coarse_model_mask(c) & (1 << m)) want.push_back({(void**)&k.map[m], sizeof(double) * N * N});
  SLABTRY(alloc_all_or_none(c, want, "nq_coarse_flux"));
  k.ready = true;
  if (maps) k.have_maps = true;
  return 0;
}
static MArr coarse_rows_of(cd* p, int pitch) {
  MArr m;
  m.xs = m.ys = p;
  m.pitch = pitch;
  m.W = pitch;
  m.shift = 30;
  m.magic = 0;
  m.blk = 0;
  return m;
}
static void coarse_columns_inverse(nq_ctx* c, cd* const* spec, cd* const* mixed, int n, bool half_planes) {
  ArrayList al;
  const int width = half_planes ? c->Wh : c->N, pitch = half_planes ? c->Ph : c->N;
  for (int i = 0; i < 6; ++i) {
    al.ptr[i] = i < n ? mixed[i] : nullptr;
    al.width[i] = i < n ? width : 0;
    al.pitch[i] = i < n ? pitch : 0;
  }
  for (int i = 0; i < n; ++i) launch_B_p(c, true, spec[i], pitch, mixed[i], pitch, width, 1.0 / ((double)c->N * c->N));
  launch_A_list(c, true, al, n, width);
}
int nq_coarse_flux(nq_ctx* c, int what_mask, int nscales, const double* g, int nb, double* moments, double* maps) {
  NQ_SINGLE_RANK(c, "nq_coarse_flux");
  const int N = c->N, have = coarse_model_mask(c);
  if (what_mask <= 0 || (what_mask & ~have))
    NQ_FAIL(c, -1, "nq_coarse_flux: map mask %d; this model has mask %d (NQ_CG_KE 1, NQ_CG_ENS 2, NQ_CG_NIW 4)", what_mask, have);
  if (nscales < 1 || nscales > NQ_CG_MAX_SCALES) NQ_FAIL(c, -1, "nq_coarse_flux: %d scales; 1 to %d per call", nscales, NQ_CG_MAX_SCALES);
  if (!g || !moments) NQ_FAIL(c, -1, "nq_coarse_flux: null table or null moments");
  if (nb != nq_shell_count(N)) NQ_FAIL(c, -1, "nq_coarse_flux: nb = %d, the grid has %d shells", nb, nq_shell_count(N));
  for (int s = 0; s < nscales; ++s)
    for (int b = 0; b < nb; ++b) {
      const double x = g[(size_t)s * nb + b];
      if (!std::isfinite(x)) NQ_FAIL(c, -1, "nq_coarse_flux: table %d is not finite on shell %d", s, b);
      if (b >= N / 2 && x != 0.0) NQ_FAIL(c, -1, "nq_coarse_flux: table %d is %g on shell %d; every table is zero from shell nx/2 = %d on", s, x, b, N / 2);
    }
  if (N >= 8192)
    NQ_FAIL(c, -1, "nq_coarse_flux: no coarse-grained maps at nx = %d: a thread of that row plan has 128 registers, the maps need 7 values per point (DESIGN.md section 7)", N);
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<nq_ctx*> grp(1, c);
  SLABTRY(tick_need_phi(grp, "nq_coarse_flux"));
  SLABTRY(slab_settle(grp));
  SLABTRY(coarse_reserve(c, nb, maps != nullptr));
  nq_ctx::Coarse& k = c->cg;
  const bool waves = c->kernel_family, balanced = !c->ybj;
  const bool need_q = (what_mask & (CG_KE | CG_ENS)) != 0, need_w = (what_mask & CG_NIW) != 0;
  const cd* qh = c->q.y[c->q.cur];
  if (balanced && (what_mask & CG_ENS)) SLABTRY(mean_qh(c, &qh));                 // the q-hat the tick bins
  // the products pass, once for all scales: F[u q], F[v q] into scr_h0, scr_h1, J into scr_f0 (nq_transfer_binned's planes)
  set_window(c, 0, 1);
  launch_products_pass(c, 0);
  SLABTRY(exchange_now(grp, 0, true));
  transfer_A(c, 0);
  if (need_q) {
    launch_B_p(c, false, c->mUq.ys, c->mUq.pitch, c->scr_h0, c->Ph, c->Wh, 1.0);
    launch_B_p(c, false, c->mVq.ys, c->mVq.pitch, c->scr_h1, c->Ph, c->Wh, 1.0);
  }
  if (need_w) launch_B_p(c, false, c->mW.ys, c->mW.pitch, c->scr_f0, c->Wf, c->Wf, 1.0);
  HIPCHK(c, hipMemcpyAsync(k.g, g, sizeof(double) * (size_t)nscales * nb, hipMemcpyHostToDevice, c->stream));
  const int nblocks = xdiag_blocks(c);
  const size_t plane = (size_t)N * N;
  size_t out_plane = 0;
  for (int s = 0; s < nscales; ++s) {
    CoarseSpec sp;
    sp.P = c->ph; sp.Q = qh; sp.Fu = c->scr_h0; sp.Fv = c->scr_h1;
    sp.W = waves ? c->w.y[c->w.cur] : nullptr; sp.J = c->scr_f0;
    sp.gp = k.sh[0]; sp.up = k.sh[1]; sp.gq = k.sh[2]; sp.qy = k.sh[3]; sp.fu = k.sh[4]; sp.fv = k.sh[5];
    sp.gw = k.sf[0]; sp.wy = k.sf[1]; sp.gj = k.sf[2];
    sp.g = k.g + (size_t)s * nb; sp.ll = c->ll; sp.N = N; sp.ph = c->Ph; sp.what = what_mask;
    const int cols = need_w ? N : N / 2 + 1;
    hipLaunchKernelGGL(k_s_coarse, dim3((cols + 255) / 256, N), dim3(256), 0, c->stream, sp);
    // the filtered half planes in use: G P, -il G P always; G Q, il G Q for ens; G Fu, G Fv for ke_qg and ens
    coarse_columns_inverse(c, k.sh, k.mh, 2, true);
    if (what_mask & CG_ENS) coarse_columns_inverse(c, k.sh + 2, k.mh + 2, 2, true);
    if (need_q) coarse_columns_inverse(c, k.sh + 4, k.mh + 4, 2, true);
    if (need_w) coarse_columns_inverse(c, k.sf, k.mf, 3, false);
    CoarseRows r;
    r.gp = coarse_rows_of(k.mh[0], c->Ph); r.up = coarse_rows_of(k.mh[1], c->Ph);
    r.gq = coarse_rows_of(k.mh[2], c->Ph); r.qy = coarse_rows_of(k.mh[3], c->Ph);
    r.fu = coarse_rows_of(k.mh[4], c->Ph); r.fv = coarse_rows_of(k.mh[5], c->Ph);
    r.gw = k.mf[0]; r.wy = k.mf[1]; r.gj = k.mf[2];
    r.what = what_mask;
    for (int m = 0; m < 3; ++m) r.map[m] = (maps && (what_mask & (1 << m))) ? k.map[m] : nullptr;
    r.part = k.part;
    with_row_size(N, [&](auto n) {
      constexpr int NN = decltype(n)::value;
      if constexpr (NN < 8192) {
        typedef XPlan<NN> X;
        if (waves) hipLaunchKernelGGL((k_x_coarse<NN, true>), dim3(nblocks), dim3(X::THREADS), X::LDS_BYTES, c->stream, r, c->twx, c->kk);
        else hipLaunchKernelGGL((k_x_coarse<NN, false>), dim3(nblocks), dim3(X::THREADS), X::LDS_BYTES, c->stream, r, c->twx, c->kk);
      }
    });
    hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(256), 0, c->stream, (const double*)k.part, nblocks, 6, 6, k.mom + 6 * (size_t)s);
    HIPCHK(c, hipGetLastError());
    if (maps)
      for (int m = 0; m < 3; ++m)
        if (what_mask & (1 << m)) HIPCHK(c, hipMemcpyAsync(maps + plane * out_plane++, k.map[m], sizeof(double) * plane, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipMemcpyAsync(moments, k.mom, sizeof(double) * 6 * (size_t)nscales, hipMemcpyDeviceToHost, c->stream));
  return nq_sync(c);
}

// ---- shell-to-shell transfers -----------------------------------------------------------------------------
// Per donor band: k_s_band into the context's own spectral planes, the inverse column passes into its own mixed-space planes,
// k_x_band into Muq, Mvq, Mw (once for Jq^Q and J^Q, once for R^Q: the tick's two passes), then the forward column passes and
// the bins of nq_transfer_binned into the band's rows.  u, v and q_psi come from the last inversion's rows, as in the tick.
static int s2s_model_mask(const nq_ctx* c) { return !c->kernel_family ? S2S_Q : c->ybj ? (S2S_ADV | S2S_REF) : (S2S_Q | S2S_ADV | S2S_REF); }
static int s2s_reserve(nq_ctx* c, int nb) {
  nq_ctx::S2s& k = c->ss;
  if (k.ready) return 0;
  const size_t N = (size_t)c->N, half = N * c->Ph * sizeof(cd), full = N * N * sizeof(cd);
  std::vector<std::pair<void**, size_t>> want;
  if (!c->ybj) {
    want.push_back({(void**)&k.sq, half});
    want.push_back({(void**)&k.mq, half});
  }
  for (int i = 0; i < (c->kernel_family ? 2 : 0); ++i) {
    want.push_back({(void**)&k.sf[i], full});
    want.push_back({(void**)&k.mf[i], full});
  }
  want.push_back({(void**)&k.g, sizeof(double) * NQ_S2S_MAX_BANDS * nb});
  want.push_back({(void**)&k.out, sizeof(double) * NQ_S2S_MAX_BANDS * NQ_S2S_ROWS * nb});
  SLABTRY(alloc_all_or_none(c, want, "nq_shell_transfer"));
  k.ready = true;
  return 0;
}
int nq_shell_transfer(nq_ctx* c, int what_mask, int nbands, const double* g, int nb, double* out) {
  NQ_SINGLE_RANK(c, "nq_shell_transfer");
  const int N = c->N, have = s2s_model_mask(c);
  if (what_mask <= 0 || (what_mask & ~have))
    NQ_FAIL(c, -1, "nq_shell_transfer: row mask %d; this model has mask %d (NQ_S2S_Q 1, NQ_S2S_ADV 2, NQ_S2S_REF 4)", what_mask, have);
  if (nbands < 1 || nbands > NQ_S2S_MAX_BANDS) NQ_FAIL(c, -1, "nq_shell_transfer: %d bands; 1 to %d per call", nbands, NQ_S2S_MAX_BANDS);
  if (!g || !out) NQ_FAIL(c, -1, "nq_shell_transfer: null table or null output");
  if (nb != nq_shell_count(N)) NQ_FAIL(c, -1, "nq_shell_transfer: nb = %d, the grid has %d shells", nb, nq_shell_count(N));
  for (int s = 0; s < nbands; ++s)
    for (int b = 0; b < nb; ++b) {
      const double x = g[(size_t)s * nb + b];
      if (!std::isfinite(x)) NQ_FAIL(c, -1, "nq_shell_transfer: table %d is not finite on shell %d", s, b);
      if (b >= N / 2 && x != 0.0) NQ_FAIL(c, -1, "nq_shell_transfer: table %d is %g on shell %d; every table is zero from shell nx/2 = %d on", s, x, b, N / 2);
    }
  if (N >= 8192)
    NQ_FAIL(c, -1, "nq_shell_transfer: no shell-to-shell transfers at nx = %d: a thread of that row plan has 128 registers and spills even with one row per launch (DESIGN.md section 7)", N);
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<nq_ctx*> grp(1, c);
  SLABTRY(tick_need_phi(grp, "nq_shell_transfer"));
  SLABTRY(slab_settle(grp));
  SLABTRY(s2s_reserve(c, nb));
  nq_ctx::S2s& k = c->ss;
  const bool waves = c->kernel_family;
  const bool need_q = (what_mask & S2S_Q) != 0, need_w = (what_mask & (S2S_ADV | S2S_REF)) != 0;
  const cd* qh = c->q.y[c->q.cur];
  if (need_q) SLABTRY(mean_qh(c, &qh));                                           // the q-hat the tick bins
  const size_t rows = (size_t)NQ_S2S_ROWS * nb;
  HIPCHK(c, hipMemcpyAsync(k.g, g, sizeof(double) * (size_t)nbands * nb, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(k.out, 0, sizeof(double) * (size_t)nbands * rows, c->stream));
  for (int s = 0; s < nbands; ++s) {
    BandSpec sp;
    sp.Q = qh; sp.W = waves ? c->w.y[c->w.cur] : nullptr;
    sp.gq = k.sq; sp.gw = k.sf[0]; sp.wy = k.sf[1];
    sp.g = k.g + (size_t)s * nb; sp.ll = c->ll; sp.N = N; sp.ph = c->Ph; sp.what = what_mask;
    const int cols = need_w ? N : N / 2 + 1;
    hipLaunchKernelGGL(k_s_band, dim3((cols + 255) / 256, N), dim3(256), 0, c->stream, sp);
    if (need_q) coarse_columns_inverse(c, &k.sq, &k.mq, 1, true);
    if (need_w) coarse_columns_inverse(c, k.sf, k.mf, (what_mask & S2S_ADV) ? 2 : 1, false);
    BandRows r;
    r.mU = c->mU; r.mP = c->mP; r.mQ = c->mQ; r.mQw = c->mQw;
    r.gq = coarse_rows_of(k.mq, c->Ph);
    r.gw = k.mf[0]; r.wy = k.mf[1];
    r.oUq = c->mUq; r.oVq = c->mVq; r.oW = c->mW;
    r.v_zero_nyq = waves ? 1 : 0;
    double* d = k.out + (size_t)s * rows;
    for (int which = 0; which < 2; ++which) {          // 0: Jq^Q and J^Q, 1: R^Q -- Mw holds one of the two wave planes at a time
      r.what = what_mask & (which == 0 ? (S2S_Q | S2S_ADV) : S2S_REF);
      if (!r.what) continue;
      if (c->p.model == NQ_MODEL_COUPLED) launch_x_band<MODE_COUPLED>(c, r);
      else if (c->p.model == NQ_MODEL_UNCOUPLED) launch_x_band<MODE_UNCOUPLED>(c, r);
      else launch_x_band<MODE_QG>(c, r);
      const bool bq = (r.what & S2S_Q) != 0, bw = (r.what & (S2S_ADV | S2S_REF)) != 0;
      if (bq && bw) launch_A_m(c, false, {&c->mUq, &c->mVq, &c->mW});
      else if (bq) launch_A_m(c, false, {&c->mUq, &c->mVq});
      else launch_A_m(c, false, {&c->mW});
      if (bq) {
        launch_B_p(c, false, c->mUq.ys, c->mUq.pitch, c->scr_h0, c->Ph, c->Wh, 1.0);
        launch_B_p(c, false, c->mVq.ys, c->mVq.pitch, c->scr_h1, c->Ph, c->Wh, 1.0);
        const BinTrQ t{HalfJac{c->scr_h0, c->scr_h1, N, c->Ph, c->kk, c->ll}, (const cd*)c->ph, qh};
        hipLaunchKernelGGL(k_bin_shells<BinTrQ>, dim3(nb), dim3(256), 0, c->stream, t, N, nb, 0, c->kh0, c->Wh, d);
      }
      if (bw) {
        launch_B_p(c, false, c->mW.ys, c->mW.pitch, c->scr_f0, c->Wf, c->Wf, 1.0);
        const BinTrW t{(const cd*)c->w.y[c->w.cur], c->scr_f0, c->Wf};
        hipLaunchKernelGGL(k_bin_shells<BinTrW>, dim3(nb), dim3(256), 0, c->stream, t, N, nb, 1, c->kf0, c->Wf, d + (size_t)(2 + which) * nb);
      }
    }
    HIPCHK(c, hipGetLastError());
  }
  HIPCHK(c, hipMemcpyAsync(out, k.out, sizeof(double) * (size_t)nbands * rows, hipMemcpyDeviceToHost, c->stream));
  return nq_sync(c);
}

// ---- isotropic co-spectra of the physical fields -----------------------------------------------------------
// Kernel family: k_x_cross packs the row values of the list (what nq_field_hist bins) as a + i b and c + i 0 and transforms them
// forward into Mw and scr_f1; the column passes finish the first plane in scr_f0 and the third field's in Mw, BinCross bins them.
// QGModel: q-hat and c-hat are the state and BinQC bins them as they are.
static int cospec_reserve(nq_ctx* c, int nb) {
  if (c->cs.cur) return 0;
  std::vector<std::pair<void**, size_t>> want;
  want.push_back({(void**)&c->cs.cur, sizeof(double) * NQ_COSPEC_ROWS * nb});
  want.push_back({(void**)&c->cs.sum, sizeof(double) * NQ_COSPEC_ROWS * nb});
  if (c->kernel_family) {                               // the range pass's workgroup partials and the scales formed from them
    want.push_back({(void**)&c->cs.part, sizeof(double) * 6 * HIST_PART_BLOCKS});
    want.push_back({(void**)&c->cs.scl, sizeof(double) * 2 * NQ_COSPEC_MAX_FIELDS});
  }
  return alloc_all_or_none(c, want, "nq_cospectra");
}
int nq_cospectra(nq_ctx* c, int nfields, const int* fields, int nb, int accumulate, double* out) {
  NQ_SINGLE_RANK(c, "nq_cospectra");
  {
    const int rc = hist_check_fields(c, "nq_cospectra", nfields, fields);
    if (rc) return rc;
  }
  const int N = c->N;
  if (nb != nq_shell_count(N)) NQ_FAIL(c, -1, "nq_cospectra: nb = %d, the grid has %d shells", nb, nq_shell_count(N));
  const bool flow = any_flow(nfields, fields);
  if (flow && flow_nv_of(c) < NQ_COSPEC_MAX_FIELDS)
    NQ_FAIL(c, -1, "nq_cospectra: flow fields (NQ_FLOW_*) at nx = %d: a thread of that row plan holds one value, a packed pair needs two (DESIGN.md section 7)", N);
  nq_ctx::Cospec& k = c->cs;
  if (accumulate) {
    bool same = k.cur && k.samples > 0 && k.nf == nfields;
    for (int i = 0; same && i < nfields; ++i) same = k.fields[i] == fields[i];
    if (!same) NQ_FAIL(c, -1, "nq_cospectra: accumulate = 1 needs the field list of the call that zeroed the tables");
  }
  HIPCHK(c, hipSetDevice(c->device));
  SLABTRY(cospec_reserve(c, nb));
  const size_t count = (size_t)NQ_COSPEC_ROWS * nb;
  if (c->kernel_family) {
    FlowSel sel = flow_sel_none(c);
    for (int i = 0; i < nfields; ++i) sel.code[i] = fields[i];
    // the third field's rows go to scr_f1 (Muq and Mvq are no home for a full row: k_x_products keeps the Jacobian's passenger sums
    // in their padding column Muq.W, zero on the rows it does not write, and k_s_phi adds all of them up)
    const MArr oC = coarse_rows_of(c->scr_f1, N);
    const bool third = nfields == NQ_COSPEC_MAX_FIELDS, coupled = c->p.model == NQ_MODEL_COUPLED;
    // the PDFs' range pass (the old names' kernel has fixed slots q, q_psi, phi2; the flow kernel's slot i is field i), then the
    // scales: all on the device
    CrossSlots sl = {{-1, -1, -1}};
    for (int i = 0; i < nfields; ++i) sl.slot[i] = flow ? i : hist_slot(c, fields[i]);
    const HistArgs none = {};
    if (flow) flow_hist(c, true, nfields, fields, none, k.part);
    else launch_xhist<true>(c, none, k.part);
    hipLaunchKernelGGL(k_cospec_scale, dim3(1), dim3(256), 0, c->stream, (const double*)k.part, xdiag_blocks(c), 6, sl, k.scl);
    if (flow) {
      if (coupled) launch_x_cross<MODE_COUPLED, true>(c, sel, k.scl, c->mW, oC);
      else launch_x_cross<MODE_UNCOUPLED, true>(c, sel, k.scl, c->mW, oC);
    } else {
      if (coupled) launch_x_cross<MODE_COUPLED, false>(c, sel, k.scl, c->mW, oC);
      else launch_x_cross<MODE_UNCOUPLED, false>(c, sel, k.scl, c->mW, oC);
    }
    launch_A_m(c, false, {&c->mW});
    if (third) launch_A(c, false, {c->scr_f1}, false);
    launch_B_p(c, false, c->mW.ys, c->mW.pitch, c->scr_f0, N, N, 1.0);
    if (third) launch_B_p(c, false, c->scr_f1, N, c->mW.ys, c->mW.pitch, N, 1.0);       // Mw is free again: the third plane ends there
    const BinCross t{(const cd*)c->scr_f0, (const cd*)(third ? c->mW.ys : nullptr), (const double*)k.scl, N, c->mW.pitch, nfields == 1};
    hipLaunchKernelGGL(k_bin_shells<BinCross>, dim3(nb), dim3(256), 0, c->stream, t, N, nb, 1, 0, N, k.cur);
  } else {
    BinQC t{{nullptr, nullptr, nullptr}, N, c->Ph};
    for (int i = 0; i < nfields; ++i) t.f[i] = fields[i] == NQ_PDF_Q ? c->q.y[c->q.cur] : c->cq.y[c->cq.cur];
    hipLaunchKernelGGL(k_bin_shells<BinQC>, dim3(nb), dim3(256), 0, c->stream, t, N, nb, 0, 0, c->Wh, k.cur);
  }
  if (!accumulate) HIPCHK(c, hipMemsetAsync(k.sum, 0, sizeof(double) * count, c->stream));
  hipLaunchKernelGGL(k_cospec_add, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, c->stream, (const double*)k.cur, k.sum, (int)count);
  HIPCHK(c, hipGetLastError());
  if (!accumulate) {
    k.nf = nfields;
    for (int i = 0; i < nfields; ++i) k.fields[i] = fields[i];
    k.samples = 0;
  }
  ++k.samples;
  if (!out) return 0;
  HIPCHK(c, hipMemcpyAsync(out, k.cur, sizeof(double) * count, hipMemcpyDeviceToHost, c->stream));
  return nq_sync(c);
}
int nq_cospectra_read(nq_ctx* c, long long* samples, double* out) {
  NQ_SINGLE_RANK(c, "nq_cospectra_read");
  if (!samples || !out) NQ_FAIL(c, -1, "nq_cospectra_read: null output");
  if (!c->cs.cur || c->cs.samples == 0) NQ_FAIL(c, -1, "nq_cospectra_read: no nq_cospectra call yet");
  HIPCHK(c, hipSetDevice(c->device));
  *samples = c->cs.samples;
  HIPCHK(c, hipMemcpyAsync(out, c->cs.sum, sizeof(double) * NQ_COSPEC_ROWS * nq_shell_count(c->N), hipMemcpyDeviceToHost, c->stream));
  return nq_sync(c);
}

// fft(phi * q_psi), (ny, nx): the refraction source of ref Kernel.py:332, :350, :367, :385 before its -0.5j factor,
// formed by the row kernel exactly as inside a step (mean NOT removed)
int nq_refraction(nq_ctx* c, double* out_cplx) {
  NQ_SINGLE_RANK(c, "nq_refraction");
  if (!out_cplx) NQ_FAIL(c, -1, "nq_refraction: null output");
  if (!c->kernel_family) NQ_FAIL(c, -4, "no wave field in QGModel");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t full = (size_t)c->N * c->N;
  launch_products(c, 0.0, 1.0);                       // W = i phi q_psi
  launch_A_m(c, false, {&c->mW});
  launch_B_p(c, false, c->mW.ys, c->mW.pitch, c->scr_f0, c->N, c->N, 1.0);
  hipLaunchKernelGGL(k_mul_minus_i, dim3((unsigned)((full + 255) / 256)), dim3(256), 0, c->stream, c->scr_f0, full);
  HIPCHK(c, hipMemcpyAsync(out_cplx, c->scr_f0, sizeof(cd) * full, hipMemcpyDeviceToHost, c->stream));
  return nq_sync(c);
}

// CoupledModel.jacobian_phic_phi (ref CoupledModel.py:59-73): fft(Re i(phix* phiy - phiy* phix)), (ny, nx), [0,0] = 0
int nq_jacobian_phic_phi(nq_ctx* c, double* out_cplx) {
  NQ_SINGLE_RANK(c, "nq_jacobian_phic_phi");
  if (!out_cplx) NQ_FAIL(c, -1, "nq_jacobian_phic_phi: null output");
  if (c->p.model != NQ_MODEL_COUPLED || c->ybj) NQ_FAIL(c, -4, "jacobian_phic_phi exists only in the coupled model");
  HIPCHK(c, hipSetDevice(c->device));
  const int N = c->N;
  launch_wavepv(c);
  launch_A_m(c, false, {&c->mB});
  launch_B_p(c, false, c->mB.ys, c->mB.pitch, c->scr_h0, c->Ph, c->Wh, 1.0);
  hipLaunchKernelGGL(k_expand_half, dim3((N + 63) / 64, N), dim3(64), 0, c->stream, (const cd*)c->scr_h0, (const cd*)nullptr, c->scr_f0, N, c->Ph, N, 0, c->kk, c->ll);
  HIPCHK(c, hipMemsetAsync(c->scr_f0, 0, sizeof(cd), c->stream));
  HIPCHK(c, hipMemcpyAsync(out_cplx, c->scr_f0, sizeof(cd) * (size_t)N * N, hipMemcpyDeviceToHost, c->stream));
  return nq_sync(c);
}

// number of DOUBLES nq_get_field(field_id) writes for this context (-1: unknown id)
long long nq_field_doubles(const nq_ctx* c, int id) {
  if (!c) return -1;
  const long long n = c->N, h = c->N / 2 + 1;
  switch (id) {
    case NQ_F_Q: case NQ_F_P: case NQ_F_U: case NQ_F_V: case NQ_F_QPSI: case NQ_F_QW: case NQ_F_C: return n * n;
    case NQ_F_QH: case NQ_F_PH: case NQ_F_QWH: case NQ_F_QH_MINUS: case NQ_F_CH: case NQ_F_QH_STAGE4: case NQ_F_QH_MINUS_STAGE4:
    case NQ_F_QH_TICK: case NQ_F_QH_MINUS_TICK: case NQ_F_QWH_TICK: return 2 * n * h;
    case NQ_F_PHI: case NQ_F_PHIH: case NQ_F_PHIX: case NQ_F_PHIY: case NQ_F_PHIH_STAGE4: case NQ_F_PHIH_TICK: return 2 * n * n;
    default: return -1;
  }
}

}  // extern "C"

// ==================================================================================================================
// The any-size engine (include/niwqg_amd.h: nq_any_*; csrc/nq_anysize.hpp; niwqg_amd/_anysize.py)
// ==================================================================================================================
#define ANYCHK(e, call)                                                                                      \
  do {                                                                                                       \
    hipError_t e_ = (call);                                                                                  \
    if (e_ != hipSuccess) {                                                                                  \
      char b_[384];                                                                                          \
      snprintf(b_, sizeof(b_), "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__);   \
      g_last_error = b_;                                                                                     \
      if (e) (e)->err = b_;                                                                                  \
      return -5;                                                                                             \
    }                                                                                                        \
  } while (0)
#define ANYFAIL(e, code, ...)                      \
  do {                                             \
    char b_[384];                                  \
    snprintf(b_, sizeof(b_), __VA_ARGS__);         \
    g_last_error = b_;                             \
    if (e) (e)->err = b_;                          \
    return (code);                                 \
  } while (0)

template <bool INV>
static int any_rows_fft(nq_any* e, const nq_any::Plan& pl, int nlines, double scale) {
  if (pl.M == 16384) {
    // four-step transform of rows of 128 x 128 points (csrc/nq_anysize.hpp: k_any_btranspose); result back in e->tmp
    const int A = 128, B = 128;
    typedef XPlan<128> X;
    const dim3 tg(A / 16, B / 16, nlines), tb(256);
    const int rows128 = nlines * 128;
    hipLaunchKernelGGL(k_any_btranspose, tg, tb, 0, e->stream, (const cd*)e->tmp, e->tmp2, B, A, (const cd*)nullptr, 0, 0);
    hipLaunchKernelGGL((k_x_c2c<128, INV>), rows_grid<X>(rows128), dim3(X::THREADS), X::LDS_BYTES, e->stream, (const cd*)e->tmp2, e->tmp2, 128, 128,
                       rows128, 1.0, (const cd*)pl.tw_small, (const double*)nullptr, 0);
    hipLaunchKernelGGL(k_any_btranspose, tg, tb, 0, e->stream, (const cd*)e->tmp2, e->tmp, A, B, (const cd*)pl.tw, 1, INV ? 1 : 0);
    hipLaunchKernelGGL((k_x_c2c<128, INV>), rows_grid<X>(rows128), dim3(X::THREADS), X::LDS_BYTES, e->stream, (const cd*)e->tmp, e->tmp, 128, 128,
                       rows128, scale, (const cd*)pl.tw_small, (const double*)nullptr, 0);
    hipLaunchKernelGGL(k_any_btranspose, tg, tb, 0, e->stream, (const cd*)e->tmp, e->tmp2, B, A, (const cd*)nullptr, 0, 0);
    std::swap(e->tmp, e->tmp2);
    std::swap(e->tmp_elems, e->tmp2_elems);
    return 0;
  }
  const bool ok = with_row_size(pl.M, [&](auto m) {
    constexpr int M = decltype(m)::value;
    typedef XPlan<M> X;
    hipLaunchKernelGGL((k_x_c2c<M, INV>), rows_grid<X>(nlines), dim3(X::THREADS), X::LDS_BYTES, e->stream,
                       (const cd*)e->tmp, e->tmp, pl.M, pl.M, nlines, scale, (const cd*)pl.tw, (const double*)nullptr, 0);
  });
  if (!ok) ANYFAIL(e, -2, "any-size engine: no row plan of length %d", pl.M);
  return 0;
}
// the fused Bluestein row kernel on `nlines` contiguous rows of `n` values (pitch n), in place or src -> dst
static int any_bluestein_rows(nq_any* e, const nq_any::Plan& pl, const cd* src, cd* dst, int nlines, int n, int inverse) {
  const double scale = (inverse ? 1.0 / (double)n : 1.0) / (double)pl.M;
  const bool ok = with_row_size(pl.M, [&](auto m) {
    constexpr int M = decltype(m)::value;
    typedef XPlan<M> X;
    hipLaunchKernelGGL((k_any_bluestein_rows<M>), rows_grid<X>(nlines), dim3(X::THREADS), X::LDS_BYTES, e->stream, src, dst, nlines, n, n,
                       (const cd*)pl.chirp, (const cd*)pl.bhat, (const cd*)pl.tw, inverse ? 1 : 0, scale);
  });
  if (!ok) ANYFAIL(e, -2, "any-size engine: no fused row plan of length %d", pl.M);
  return 0;
}
template <int R>
static int any_split_rows(nq_any* e, const nq_any::Plan& pl, const cd* src, cd* dst, int nlines, int n, int inverse) {
  const double scale = inverse ? 1.0 / (double)n : 1.0;
  bool ok = false;
  with_row_size(pl.M, [&](auto m) {
    constexpr int M = decltype(m)::value;
    if constexpr (M <= 2048) {                       // the split kernels exist for these lengths only
      typedef XPlan<M> X;
      hipLaunchKernelGGL((k_any_split_rows<M, R>), rows_grid<X>(nlines), dim3(X::THREADS), X::LDS_BYTES, e->stream, src, dst, nlines, n,
                         (const cd*)pl.chirp, (const cd*)pl.tw, inverse ? 1 : 0, scale);
      ok = true;
    }
  });
  if (!ok) ANYFAIL(e, -2, "any-size engine: no split row plan of length %d x %d", R, pl.M);
  return 0;
}
// device temporaries of one call: freed when the call returns, on the error paths too
struct AnyScratch {
  std::vector<void*> held;
  ~AnyScratch() {
    for (void* q : held) (void)hipFree(q);
  }
  template <typename T>
  hipError_t get(T** out, size_t count) {
    void* q = nullptr;
    const hipError_t r = hipMalloc(&q, count * sizeof(T));
    if (r == hipSuccess) held.push_back(q);
    *out = static_cast<T*>(q);
    return r;
  }
};
static int any_buf(nq_any* e, cd** buf, size_t* have, size_t elems) {
  if (*have >= elems) return 0;
  if (*buf) {
    ANYCHK(e, hipStreamSynchronize(e->stream));
    ANYCHK(e, hipFree(*buf));
    *buf = nullptr;
    *have = 0;
  }
  ANYCHK(e, hipMalloc(reinterpret_cast<void**>(buf), elems * sizeof(cd)));
  *have = elems;
  return 0;
}
static int any_tmp(nq_any* e, size_t elems, bool four_step = false) {
  int rc = any_buf(e, &e->tmp, &e->tmp_elems, elems);
  if (rc == 0 && four_step) rc = any_buf(e, &e->tmp2, &e->tmp2_elems, elems);
  return rc;
}
static void any_plan_free(nq_any::Plan& p) {
  for (nq::cd** q : {&p.chirp, &p.bhat, &p.tw, &p.tw_small})
    if (*q) {
      (void)hipFree(*q);
      *q = nullptr;
    }
}
static int any_plan_build(nq_any* e, int n, nq_any::Plan& pl);
// Bluestein plan for transforms of length n: chirp w[j] = exp(-i pi j^2 / n) (angle reduced exactly: j^2 mod 2n), the transform of
// conj(w) laid out circularly on M >= 2n - 1 points, and the twiddle table of the M-point row engine.  A plan that fails half
// way frees what it allocated (after the work queued on e->stream that may still read its host vectors or e->tmp is done).
static int any_plan(nq_any* e, int n, const nq_any::Plan** out) {
  for (const nq_any::Plan& p : e->plans)
    if (p.n == n) { *out = &p; return 0; }
  const bool pow2 = n >= 64 && (n & (n - 1)) == 0;
  if (n < 2 || (pow2 ? n > 16384 : n > 8192)) ANYFAIL(e, -2, "any-size engine: transform length %d (any n in [1, 8192], or 16384)", n);
  nq_any::Plan pl;
  const int rc = any_plan_build(e, n, pl);
  if (rc) {
    (void)hipStreamSynchronize(e->stream);
    any_plan_free(pl);
    return rc;
  }
  e->plans.push_back(pl);
  *out = &e->plans.back();
  return 0;
}
static int any_plan_build(nq_any* e, int n, nq_any::Plan& pl) {
  const bool pow2 = n >= 64 && (n & (n - 1)) == 0;
  pl.n = n;
  pl.direct = pow2;
  pl.M = 64;
  static int use_split = -1;
  if (use_split < 0) {
    const char* ev = getenv("NIWQG_AMD_ANY_SPLIT");              // 0: Bluestein for 3 m and 5 m as well (A/B measurements)
    use_split = (ev && atoi(ev) == 0) ? 0 : 1;
  }
  for (int R : {3, 5}) {
    const int m = n / R;
    if (use_split && !pow2 && n % R == 0 && m >= 64 && m <= 2048 && (m & (m - 1)) == 0) {
      pl.split = R;
      pl.M = m;
      break;
    }
  }
  if (pow2) pl.M = n;
  else if (!pl.split)
    while (pl.M < 2 * n - 1) pl.M *= 2;
  const int M = pl.M;
  const long double pi = 3.14159265358979323846264338327950288L;
  std::vector<double> tw(2 * (size_t)M);
  for (int m = 0; m < M; ++m) {
    const long double a = -2.0L * pi * (long double)m / (long double)M;
    tw[2 * m] = (double)cosl(a);
    tw[2 * m + 1] = (double)sinl(a);
  }
  ANYCHK(e, hipMalloc(reinterpret_cast<void**>(&pl.tw), sizeof(cd) * M));
  ANYCHK(e, hipMemcpy(pl.tw, tw.data(), sizeof(cd) * M, hipMemcpyHostToDevice));
  if (M == 16384) {
    std::vector<double> ts(2 * 128);
    for (int m = 0; m < 128; ++m) {
      const long double a = -2.0L * pi * (long double)m / 128.0L;
      ts[2 * m] = (double)cosl(a);
      ts[2 * m + 1] = (double)sinl(a);
    }
    ANYCHK(e, hipMalloc(reinterpret_cast<void**>(&pl.tw_small), sizeof(cd) * 128));
    ANYCHK(e, hipMemcpy(pl.tw_small, ts.data(), sizeof(cd) * 128, hipMemcpyHostToDevice));
  }
  if (pl.split) {
    // chirp slot: exp(-2 pi i q / n), q < n -- the twiddles of the radix-R combination
    std::vector<double> wn(2 * (size_t)n);
    for (int q = 0; q < n; ++q) {
      const long double a = -2.0L * pi * (long double)q / (long double)n;
      wn[2 * q] = (double)cosl(a);
      wn[2 * q + 1] = (double)sinl(a);
    }
    ANYCHK(e, hipMalloc(reinterpret_cast<void**>(&pl.chirp), sizeof(cd) * n));
    ANYCHK(e, hipMemcpy(pl.chirp, wn.data(), sizeof(cd) * n, hipMemcpyHostToDevice));
  } else if (!pl.direct) {
    std::vector<double> w(2 * (size_t)n), b(2 * (size_t)M, 0.0);
    for (int j = 0; j < n; ++j) {
      const long long r = ((long long)j * j) % (2LL * n);
      const long double a = pi * (long double)r / (long double)n;
      w[2 * j] = (double)cosl(a);
      w[2 * j + 1] = (double)(-sinl(a));
      // conj(w[j]) at +j and -j (circular)
      b[2 * j] = (double)cosl(a);
      b[2 * j + 1] = (double)sinl(a);
      if (j > 0) {
        b[2 * (size_t)(M - j)] = (double)cosl(a);
        b[2 * (size_t)(M - j) + 1] = (double)sinl(a);
      }
    }
    ANYCHK(e, hipMalloc(reinterpret_cast<void**>(&pl.chirp), sizeof(cd) * n));
    ANYCHK(e, hipMalloc(reinterpret_cast<void**>(&pl.bhat), sizeof(cd) * M));
    ANYCHK(e, hipMemcpy(pl.chirp, w.data(), sizeof(cd) * n, hipMemcpyHostToDevice));
    int rc = any_tmp(e, (size_t)M, M == 16384);
    if (rc) return rc;
    // e->tmp may still be read by transforms queued before this call: the upload goes in stream order (the synchronisation
    // below keeps b alive until it is done)
    ANYCHK(e, hipMemcpyAsync(e->tmp, b.data(), sizeof(cd) * M, hipMemcpyHostToDevice, e->stream));
    rc = any_rows_fft<false>(e, pl, 1, 1.0);
    if (rc) return rc;
    ANYCHK(e, hipMemcpyAsync(pl.bhat, e->tmp, sizeof(cd) * M, hipMemcpyDeviceToDevice, e->stream));
    ANYCHK(e, hipStreamSynchronize(e->stream));
    ANYCHK(e, hipGetLastError());
  }
  return 0;
}

extern "C" {

int nq_any_create(int device, nq_any** out) {
  if (!out) return -1;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) NQ_FAIL((nq_ctx*)nullptr, -3, "nq_any_create: no HIP device available");
  if (device < 0 || device >= ndev) NQ_FAIL((nq_ctx*)nullptr, -3, "nq_any_create: device %d out of range (%d devices)", device, ndev);
  nq_any* e = new nq_any();
  e->device = device;
  e->plans.reserve(16);
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess ||
      hipMalloc(reinterpret_cast<void**>(&e->part), sizeof(double) * 2 * 1024) != hipSuccess ||
      hipMalloc(reinterpret_cast<void**>(&e->red), sizeof(double) * 2) != hipSuccess) {
    delete e;
    NQ_FAIL((nq_ctx*)nullptr, -5, "nq_any_create: stream / scratch allocation failed");
  }
  *out = e;
  return 0;
}
int nq_any_destroy(nq_any* e) {
  if (!e) return -1;
  (void)hipSetDevice(e->device);
  (void)hipStreamSynchronize(e->stream);
  for (void* p : e->allocs) (void)hipFree(p);
  for (nq_any::Plan& p : e->plans) {
    if (p.chirp) (void)hipFree(p.chirp);
    if (p.bhat) (void)hipFree(p.bhat);
    if (p.tw_small) (void)hipFree(p.tw_small);
    (void)hipFree(p.tw);
  }
  if (e->tmp) (void)hipFree(e->tmp);
  if (e->tmp2) (void)hipFree(e->tmp2);
  (void)hipFree(e->part);
  (void)hipFree(e->red);
  (void)hipStreamDestroy(e->stream);
  delete e;
  return 0;
}
const char* nq_any_last_error(const nq_any* e) { return e ? e->err.c_str() : g_last_error.c_str(); }
int nq_any_sync(nq_any* e) {
  if (!e) return -1;
  ANYCHK(e, hipSetDevice(e->device));
  ANYCHK(e, hipStreamSynchronize(e->stream));
  ANYCHK(e, hipGetLastError());
  return 0;
}
long long nq_any_device_bytes(const nq_any* e) { return e ? e->bytes + (long long)((e->tmp_elems + e->tmp2_elems) * sizeof(cd)) : 0; }
int nq_any_alloc(nq_any* e, long long elems, void** plane) {
  if (!e || !plane || elems <= 0) return -1;
  ANYCHK(e, hipSetDevice(e->device));
  void* p = nullptr;
  ANYCHK(e, hipMalloc(&p, (size_t)elems * sizeof(cd)));
  ANYCHK(e, hipMemsetAsync(p, 0, (size_t)elems * sizeof(cd), e->stream));
  e->allocs.push_back(p);
  e->bytes += elems * (long long)sizeof(cd);
  *plane = p;
  return 0;
}
int nq_any_free(nq_any* e, void* plane, long long elems) {
  if (!e || !plane) return -1;
  ANYCHK(e, hipSetDevice(e->device));
  for (size_t i = 0; i < e->allocs.size(); ++i)
    if (e->allocs[i] == plane) {
      ANYCHK(e, hipStreamSynchronize(e->stream));
      ANYCHK(e, hipFree(plane));
      e->allocs.erase(e->allocs.begin() + i);
      e->bytes -= elems * (long long)sizeof(cd);
      return 0;
    }
  ANYFAIL(e, -1, "nq_any_free: not a plane of this engine");
}
int nq_any_upload(nq_any* e, void* plane, const double* host_cplx, long long elems) {
  if (!e || !plane || !host_cplx || elems <= 0) return -1;
  ANYCHK(e, hipSetDevice(e->device));
  ANYCHK(e, hipMemcpyAsync(plane, host_cplx, (size_t)elems * sizeof(cd), hipMemcpyHostToDevice, e->stream));
  return nq_any_sync(e);
}
int nq_any_download(nq_any* e, const void* plane, double* host_cplx, long long elems) {
  if (!e || !plane || !host_cplx || elems <= 0) return -1;
  ANYCHK(e, hipSetDevice(e->device));
  ANYCHK(e, hipMemcpyAsync(host_cplx, plane, (size_t)elems * sizeof(cd), hipMemcpyDeviceToHost, e->stream));
  return nq_any_sync(e);
}
// dst <- 1-D transforms of src along `axis` (1: along the contiguous index, length cols; 0: length rows), numpy.fft conventions
// (forward unnormalised, inverse scaled by 1/n; length 1 is the identity); dst may be src
int nq_any_fft(nq_any* e, void* dst, const void* src, int rows, int cols, int axis, int inverse) {
  if (!e || !dst || !src || rows < 1 || cols < 1 || (axis != 0 && axis != 1)) return -1;
  ANYCHK(e, hipSetDevice(e->device));
  const int n = axis == 1 ? cols : rows, nlines = axis == 1 ? rows : cols;
  if (n == 1) {
    if (dst != src) ANYCHK(e, hipMemcpyAsync(dst, src, (size_t)rows * cols * sizeof(cd), hipMemcpyDeviceToDevice, e->stream));
    return 0;
  }
  const nq_any::Plan* pl = nullptr;
  int rc = any_plan(e, n, &pl);
  if (rc) return rc;
  cd* srcp = reinterpret_cast<cd*>(const_cast<void*>(src));
  static int fused = -1;
  if (fused < 0) {
    const char* ev = getenv("NIWQG_AMD_ANY_FUSED");             // 0: the unfused five-launch form (A/B measurements)
    fused = (ev && atoi(ev) == 0) ? 0 : 1;
  }
  auto line_kernel = [&](const cd* a, cd* b, int nl, int len) -> int {
    if (pl->split == 3) return any_split_rows<3>(e, *pl, a, b, nl, len, inverse);
    if (pl->split == 5) return any_split_rows<5>(e, *pl, a, b, nl, len, inverse);
    return any_bluestein_rows(e, *pl, a, b, nl, len, inverse);
  };
  if ((fused || pl->split) && !pl->direct && pl->M <= 8192) {
    // one kernel per line (k_any_bluestein_rows / k_any_split_rows); columns through a transpose of the plane
    if (axis == 1) {
      if (pl->split && srcp == reinterpret_cast<cd*>(dst)) {      // the split kernel writes X[k + m s] while other threads still read x[R j + r]: not in place
        rc = any_tmp(e, (size_t)rows * cols);
        if (rc) return rc;
        rc = line_kernel(srcp, e->tmp, rows, cols);
        if (rc) return rc;
        ANYCHK(e, hipMemcpyAsync(dst, e->tmp, (size_t)rows * cols * sizeof(cd), hipMemcpyDeviceToDevice, e->stream));
      } else {
        rc = line_kernel(srcp, reinterpret_cast<cd*>(dst), rows, cols);
        if (rc) return rc;
      }
    } else {
      rc = any_tmp(e, (size_t)rows * cols);
      if (rc) return rc;
      hipLaunchKernelGGL(k_any_btranspose, dim3((cols + 15) / 16, (rows + 15) / 16, 1), dim3(256), 0, e->stream, (const cd*)srcp, e->tmp, rows, cols,
                         (const cd*)nullptr, 0, 0);
      if (pl->split) {                                           // (not in place, see above: tmp -> tmp2)
        rc = any_buf(e, &e->tmp2, &e->tmp2_elems, (size_t)rows * cols);
        if (rc) return rc;
        rc = line_kernel(e->tmp, e->tmp2, cols, rows);
        if (rc) return rc;
        hipLaunchKernelGGL(k_any_btranspose, dim3((rows + 15) / 16, (cols + 15) / 16, 1), dim3(256), 0, e->stream, (const cd*)e->tmp2, reinterpret_cast<cd*>(dst), cols, rows,
                           (const cd*)nullptr, 0, 0);
        ANYCHK(e, hipGetLastError());
        return 0;
      }
      rc = line_kernel(e->tmp, e->tmp, cols, rows);
      if (rc) return rc;
      hipLaunchKernelGGL(k_any_btranspose, dim3((rows + 15) / 16, (cols + 15) / 16, 1), dim3(256), 0, e->stream, (const cd*)e->tmp, reinterpret_cast<cd*>(dst), cols, rows,
                         (const cd*)nullptr, 0, 0);
    }
    ANYCHK(e, hipGetLastError());
    return 0;
  }
  rc = any_tmp(e, (size_t)nlines * pl->M, pl->M == 16384);
  if (rc) return rc;
  const dim3 gp((pl->M + 15) / 16, (nlines + 15) / 16), gu((n + 15) / 16, (nlines + 15) / 16);
  if (pl->direct) {          // a power of two the row engine takes (four-step for 16384): no chirp, the inverse by its own kernel
    hipLaunchKernelGGL((k_any_lines<true>), gp, dim3(256), 0, e->stream, srcp, e->tmp, rows, cols, axis, pl->M, (const cd*)nullptr, 0, 1.0);
    rc = inverse ? any_rows_fft<true>(e, *pl, nlines, 1.0 / (double)n) : any_rows_fft<false>(e, *pl, nlines, 1.0);
    if (rc) return rc;
    hipLaunchKernelGGL((k_any_lines<false>), gu, dim3(256), 0, e->stream, reinterpret_cast<cd*>(dst), e->tmp, rows, cols, axis, pl->M, (const cd*)nullptr, 0, 1.0);
    ANYCHK(e, hipGetLastError());
    return 0;
  }
  hipLaunchKernelGGL((k_any_lines<true>), gp, dim3(256), 0, e->stream, srcp, e->tmp, rows, cols, axis, pl->M,
                     (const cd*)pl->chirp, inverse ? 1 : 0, 1.0);
  rc = any_rows_fft<false>(e, *pl, nlines, 1.0);
  if (rc) return rc;
  hipLaunchKernelGGL(k_any_mul_rows, dim3(2048), dim3(256), 0, e->stream, e->tmp, (const cd*)pl->bhat, nlines, pl->M);
  rc = any_rows_fft<true>(e, *pl, nlines, 1.0 / (double)pl->M);
  if (rc) return rc;
  hipLaunchKernelGGL((k_any_lines<false>), gu, dim3(256), 0, e->stream, reinterpret_cast<cd*>(dst), e->tmp, rows, cols, axis, pl->M,
                     (const cd*)pl->chirp, inverse ? 1 : 0, inverse ? 1.0 / (double)n : 1.0);
  ANYCHK(e, hipGetLastError());
  return 0;
}
// d <- op(a, b, c; scalars) element by element over `elems` complex values (NQ_EW_* in the header); operands the op does not use
// may be NULL; d may alias an operand
int nq_any_ew(nq_any* e, int op, void* d, const void* a, const void* b, const void* c, long long elems, const double* scalars6) {
  if (!e || !d || !a || elems <= 0 || op < 0 || op > EW_FILL) return -1;
  const bool need_b = (op == EW_MUL || op == EW_MULCONJ || op == EW_AXPBY || op == EW_AXPBYPCZ || op == EW_MULADD);
  const bool need_c = (op == EW_AXPBYPCZ || op == EW_MULADD);
  if ((need_b && !b) || (need_c && !c)) ANYFAIL(e, -1, "nq_any_ew: op %d needs more operands", op);
  ANYCHK(e, hipSetDevice(e->device));
  EwScalars sc;
  for (int i = 0; i < 6; ++i) sc.s[i] = scalars6 ? scalars6[i] : (i == 0 ? 1.0 : 0.0);
  const size_t n = (size_t)elems;
  const int grid = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
  hipLaunchKernelGGL(k_any_ew, dim3(grid), dim3(256), 0, e->stream, op, reinterpret_cast<cd*>(d), reinterpret_cast<const cd*>(a),
                     reinterpret_cast<const cd*>(b), reinterpret_cast<const cd*>(c), n, sc);
  ANYCHK(e, hipGetLastError());
  return 0;
}
// out2 <- reduction over `elems` complex values (NQ_RD_*): deterministic (fixed grid, partials added in order)
int nq_any_reduce(nq_any* e, int op, const void* a, const void* b, long long elems, double* out2) {
  if (!e || !a || !out2 || elems <= 0 || op < 0 || op > RD_MAXABSRE) return -1;
  if ((op == RD_DOT || op == RD_DOTC || op == RD_WSUMABS2) && !b) ANYFAIL(e, -1, "nq_any_reduce: op %d needs two operands", op);
  ANYCHK(e, hipSetDevice(e->device));
  const size_t n = (size_t)elems;
  const int grid = (int)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);
  hipLaunchKernelGGL(k_any_reduce1, dim3(grid), dim3(256), 0, e->stream, op, reinterpret_cast<const cd*>(a), reinterpret_cast<const cd*>(b), n, e->part);
  hipLaunchKernelGGL(k_any_reduce2, dim3(1), dim3(256), 0, e->stream, op, (const double*)e->part, grid, e->red);
  ANYCHK(e, hipMemcpyAsync(out2, e->red, sizeof(double) * 2, hipMemcpyDeviceToHost, e->stream));
  return nq_any_sync(e);
}
// (rows, n/2+1) half spectrum -> (rows, n) Hermitian extension; project: Hermitian part (in l) of the two self-mirrored columns first
int nq_any_expand_half(nq_any* e, void* full, const void* half, int rows, int n, int project) {
  if (!e || !full || !half || rows < 1 || n < 2 || (n & 1)) return -1;
  ANYCHK(e, hipSetDevice(e->device));
  hipLaunchKernelGGL(k_any_expand_half, dim3((n + 63) / 64, rows), dim3(64), 0, e->stream, reinterpret_cast<const cd*>(half), reinterpret_cast<cd*>(full), rows, n, project);
  ANYCHK(e, hipGetLastError());
  return 0;
}
// the first dcols columns of a (rows, scols) plane as a (rows, dcols) plane
int nq_any_take_cols(nq_any* e, void* dst, const void* src, int rows, int scols, int dcols) {
  if (!e || !dst || !src || rows < 1 || dcols < 1 || dcols > scols) return -1;
  ANYCHK(e, hipSetDevice(e->device));
  hipLaunchKernelGGL(k_any_take_cols, dim3((dcols + 63) / 64, rows), dim3(64), 0, e->stream, reinterpret_cast<const cd*>(src), reinterpret_cast<cd*>(dst), rows, scols, dcols);
  ANYCHK(e, hipGetLastError());
  return 0;
}
// isotropic shell sums of Re(plane): layout 0 a full (rows, rows) plane in fftfreq order, 1 an rfft half plane (rows, rows/2+1);
// out: nb = round(rows / sqrt 2) + 1 doubles, the shell rule of nq_diagnostics_binned, deterministic (no atomics)
int nq_any_bin(nq_any* e, const void* plane, int rows, int cols, int layout, int nb, double* out) {
  if (!e || !plane || !out || rows < 2 || (rows & 1)) return -1;
  if (layout != 0 && layout != 1) ANYFAIL(e, -1, "nq_any_bin: layout %d (0: full plane, 1: half plane)", layout);
  if (cols != (layout == 0 ? rows : rows / 2 + 1)) ANYFAIL(e, -1, "nq_any_bin: %d columns for a %s plane of %d rows", cols, layout == 0 ? "full" : "half", rows);
  if (nb != nq_shell_count(rows)) ANYFAIL(e, -1, "nq_any_bin: nb = %d, the grid has %d shells", nb, nq_shell_count(rows));
  ANYCHK(e, hipSetDevice(e->device));
  double* d = nullptr;
  AnyScratch tmp;
  ANYCHK(e, tmp.get(&d, (size_t)nb));
  const AnyBinRe t{reinterpret_cast<const cd*>(plane), cols};
  hipLaunchKernelGGL(k_bin_shells<AnyBinRe>, dim3(nb), dim3(256), 0, e->stream, t, rows, nb, layout == 0 ? 1 : 0, 0, cols, d);
  ANYCHK(e, hipGetLastError());
  ANYCHK(e, hipMemcpyAsync(out, d, sizeof(double) * nb, hipMemcpyDeviceToHost, e->stream));
  return nq_any_sync(e);
}
// PDFs on engine planes: counts of Re(plane) (what = 0) or |plane|^2 (what = 1) over `elems` complex values,
// the bin rule and the kernels of nq_field_hist; out: bins + 3 counts (bins, below, above, NaN)
static int any_hist_range(nq_any* e, const char* what, double lo, double hi) {
  if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo < hi)) ANYFAIL(e, -1, "%s: range [%g, %g] (finite, lo < hi)", what, lo, hi);
  return 0;
}
int nq_any_hist(nq_any* e, const void* plane, long long elems, int what, double lo, double hi, int bins, unsigned long long* out) {
  if (!e || !plane || !out || elems <= 0) return -1;
  if (what != 0 && what != 1) ANYFAIL(e, -1, "nq_any_hist: what = %d (0: Re, 1: |a|^2)", what);
  if (bins < 1 || bins > HIST_MAX_BINS) ANYFAIL(e, -1, "nq_any_hist: bins = %d (1 to %d: the LDS tables of a workgroup)", bins, HIST_MAX_BINS);
  {
    const int rc = any_hist_range(e, "nq_any_hist", lo, hi);
    if (rc) return rc;
  }
  ANYCHK(e, hipSetDevice(e->device));
  HistArgs h = {};
  h.bins = bins;
  h.mask = 1;
  h.lo[0] = lo;
  h.hi[0] = hi;
  h.s[0] = (double)bins / (hi - lo);
  const int words = hist_words(bins, 0);
  AnyScratch tmp;
  ANYCHK(e, tmp.get(&h.tab, (size_t)words));
  ANYCHK(e, hipMemsetAsync(h.tab, 0, sizeof(unsigned long long) * words, e->stream));
  const size_t n = (size_t)elems;
  hipLaunchKernelGGL(k_hist_plane, dim3(hist_plane_grid(n)), dim3(256), sizeof(unsigned) * words, e->stream,
                     reinterpret_cast<const double*>(plane), (const double*)nullptr, n, 2, what, 0, h);
  ANYCHK(e, hipGetLastError());
  ANYCHK(e, hipMemcpyAsync(out, h.tab, sizeof(unsigned long long) * (bins + 3), hipMemcpyDeviceToHost, e->stream));
  return nq_any_sync(e);
}
// the joint form: out[ib * bins + ia] over the pair (what_a of plane_a, what_b of plane_b), then out[bins^2] = the points
// with either value out of its range or NaN; lo2 / hi2: the two ranges
int nq_any_hist2(nq_any* e, const void* plane_a, const void* plane_b, long long elems, int what_a, int what_b, const double* lo2,
                 const double* hi2, int bins, unsigned long long* out) {
  if (!e || !plane_a || !plane_b || !lo2 || !hi2 || !out || elems <= 0) return -1;
  if ((what_a != 0 && what_a != 1) || (what_b != 0 && what_b != 1)) ANYFAIL(e, -1, "nq_any_hist2: what = %d, %d (0: Re, 1: |a|^2)", what_a, what_b);
  if (bins < 1 || bins > HIST_MAX_JBINS) ANYFAIL(e, -1, "nq_any_hist2: bins = %d (1 to %d per axis: the LDS tables of a workgroup)", bins, HIST_MAX_JBINS);
  for (int i = 0; i < 2; ++i) {
    const int rc = any_hist_range(e, "nq_any_hist2", lo2[i], hi2[i]);
    if (rc) return rc;
  }
  ANYCHK(e, hipSetDevice(e->device));
  HistArgs h = {};
  h.bins = 1;                       // (the 1-D tables are not counted: mask = 0)
  h.jbins = bins;
  h.ja = 0;
  h.jb = 1;
  for (int i = 0; i < 2; ++i) {
    h.lo[i] = lo2[i];
    h.hi[i] = hi2[i];
    h.js[i] = (double)bins / (hi2[i] - lo2[i]);
  }
  const int words = hist_words(h.bins, h.jbins), j0 = HIST_SLOTS * (h.bins + 3);
  AnyScratch tmp;
  ANYCHK(e, tmp.get(&h.tab, (size_t)words));
  ANYCHK(e, hipMemsetAsync(h.tab, 0, sizeof(unsigned long long) * words, e->stream));
  const size_t n = (size_t)elems;
  hipLaunchKernelGGL(k_hist_plane, dim3(hist_plane_grid(n)), dim3(256), sizeof(unsigned) * words, e->stream,
                     reinterpret_cast<const double*>(plane_a), reinterpret_cast<const double*>(plane_b), n, 2, what_a, what_b, h);
  ANYCHK(e, hipGetLastError());
  ANYCHK(e, hipMemcpyAsync(out, h.tab + j0, sizeof(unsigned long long) * ((size_t)bins * bins + 1), hipMemcpyDeviceToHost, e->stream));
  return nq_any_sync(e);
}
// out2 = exact minimum and maximum of Re(plane) or |plane|^2; NaN (both) when any value is NaN
int nq_any_minmax(nq_any* e, const void* plane, long long elems, int what, double* out2) {
  if (!e || !plane || !out2 || elems <= 0) return -1;
  if (what != 0 && what != 1) ANYFAIL(e, -1, "nq_any_minmax: what = %d (0: Re, 1: |a|^2)", what);
  ANYCHK(e, hipSetDevice(e->device));
  const size_t n = (size_t)elems;
  const int grid = hist_plane_grid(n);
  double* part = nullptr;
  AnyScratch tmp;
  ANYCHK(e, tmp.get(&part, (size_t)4 * grid));
  hipLaunchKernelGGL(k_minmax_plane, dim3(grid), dim3(256), 0, e->stream, reinterpret_cast<const double*>(plane), (const double*)nullptr, n, 2, what, 0, part);
  ANYCHK(e, hipGetLastError());
  std::vector<double> host((size_t)4 * grid);
  ANYCHK(e, hipMemcpyAsync(host.data(), part, sizeof(double) * host.size(), hipMemcpyDeviceToHost, e->stream));
  {
    const int rc = nq_any_sync(e);
    if (rc) return rc;
  }
  double lo = host[0], hi = host[1];
  for (int k = 1; k < grid; ++k) {
    const double a = host[(size_t)4 * k], b = host[(size_t)4 * k + 1];
    lo = (lo != lo || lo < a) ? lo : a;
    hi = (hi != hi || hi > b) ? hi : b;
  }
  out2[0] = lo;
  out2[1] = hi;
  return 0;
}
// Structure functions on engine planes: the raw sums of nq_structure for one state, from (rows, cols) complex
// planes; what[i] = 0: the real part of plane i, 2: its complex value (the phi columns; one plane at most); k_sf_plane and
// k_sf_total of the fused QGModel route.  out: nsep x (9 nfields + ntriples).  Synchronous, like nq_any_hist.
int nq_any_increments(nq_any* e, int nfields, const void* const* planes, const int* what, int rows, int cols, int nsep, const int* seps,
                      int ntriples, const int* triples, double* out) {
  if (!e || !planes || !what || !out || rows < 1 || cols < 2) return -1;
  if (nfields < 1 || nfields > SF_MAX_FIELDS) ANYFAIL(e, -1, "nq_any_increments: %d fields (1 to %d)", nfields, SF_MAX_FIELDS);
  bool cplx[SF_MAX_FIELDS] = {};
  for (int i = 0; i < nfields; ++i) {
    if (!planes[i]) ANYFAIL(e, -1, "nq_any_increments: plane %d is null", i);
    if (what[i] != 0 && what[i] != 2) ANYFAIL(e, -1, "nq_any_increments: what[%d] = %d (0: Re, 2: complex)", i, what[i]);
    cplx[i] = what[i] == 2;
  }
  SfArgs a;
  int canon[SF_MAX_FIELDS] = {};
  if (const char* bad = sf_plan(cols, nfields, cplx, nsep, seps, ntriples, triples, &a, canon)) ANYFAIL(e, -1, "nq_any_increments: %s", bad);
  ANYCHK(e, hipSetDevice(e->device));
  constexpr int nc = sf_ncols<SF_MAX_FIELDS>();
  const int nblk = sf_plane_grid(rows), nout = nfields * SF_COLS + ntriples;
  double* tab = nullptr;
  AnyScratch tmp;
  ANYCHK(e, tmp.get(&a.part, (size_t)nblk * nsep * nc));
  ANYCHK(e, tmp.get(&tab, (size_t)nsep * nout));
  int* dseps = nullptr;
  ANYCHK(e, tmp.get(&dseps, (size_t)nsep));
  ANYCHK(e, hipMemcpyAsync(dseps, seps, sizeof(int) * nsep, hipMemcpyHostToDevice, e->stream));
  a.seps = dseps;
  SfPlanes pl = {};
  for (int i = 0; i < nfields; ++i) {
    pl.p[canon[i]] = reinterpret_cast<const double*>(planes[i]);
    pl.stride[canon[i]] = 2;
  }
  pl.rows = rows;
  pl.cols = cols;
  hipLaunchKernelGGL(k_sf_plane, dim3(nblk), dim3(SF_PLANE_THREADS), 0, e->stream, pl, a);
  hipLaunchKernelGGL(k_sf_total, dim3((nsep * nc + SF_TOTAL_ENTRIES - 1) / SF_TOTAL_ENTRIES), dim3(SF_TOTAL_RUNS * SF_TOTAL_ENTRIES), 0, e->stream, (const double*)a.part, nblk, nsep, nc, sf_map(SF_MAX_FIELDS, nfields, canon, ntriples), nout, 0, tab);
  ANYCHK(e, hipGetLastError());
  ANYCHK(e, hipMemcpyAsync(out, tab, sizeof(double) * nsep * nout, hipMemcpyDeviceToHost, e->stream));
  return nq_any_sync(e);
}
// The same at two-dimensional separations: nq_structure2's plane kernels on engine planes
int nq_any_increments2(nq_any* e, int nfields, const void* const* planes, const int* what, int rows, int cols, int nvec, const int* vecs,
                       const double* proj, int proj_a, int proj_b, int ntriples, const int* triples, double* out) {
  if (!e || !planes || !what || !out || rows < 1 || cols < 2) return -1;
  if (nfields < 1 || nfields > SF_MAX_FIELDS) ANYFAIL(e, -1, "nq_any_increments2: %d fields (1 to %d)", nfields, SF_MAX_FIELDS);
  bool cplx[SF_MAX_FIELDS] = {};
  for (int i = 0; i < nfields; ++i) {
    if (!planes[i]) ANYFAIL(e, -1, "nq_any_increments2: plane %d is null", i);
    if (what[i] != 0 && what[i] != 2) ANYFAIL(e, -1, "nq_any_increments2: what[%d] = %d (0: Re, 2: complex)", i, what[i]);
    cplx[i] = what[i] == 2;
  }
  Sf2Args a;
  int canon[SF_MAX_FIELDS] = {};
  Sf2Vec sorted[SF2_MAX_VECS];
  if (const char* bad = sf2_plan(rows, cols, nfields, cplx, nvec, vecs, proj, proj_a, proj_b, ntriples, triples, &a, canon, sorted))
    ANYFAIL(e, -1, "nq_any_increments2: %s", bad);
  ANYCHK(e, hipSetDevice(e->device));
  const Sf2Route route = sf2_route(cols, a.nreal, a.phi);
  const int nblk = sf2_grid(rows, nvec, route.nc), nout = nfields * SF_COLS + ntriples;
  double *tab = nullptr, *dproj = nullptr;
  Sf2Vec* dvecs = nullptr;
  AnyScratch tmp;
  ANYCHK(e, tmp.get(&a.part, (size_t)nblk * nvec * route.nc));
  ANYCHK(e, tmp.get(&tab, (size_t)nvec * nout));
  ANYCHK(e, tmp.get(&dvecs, (size_t)nvec));
  ANYCHK(e, hipMemcpyAsync(dvecs, sorted, sizeof(Sf2Vec) * nvec, hipMemcpyHostToDevice, e->stream));
  a.vecs = dvecs;
  if (proj) {
    ANYCHK(e, tmp.get(&dproj, (size_t)2 * nvec));
    ANYCHK(e, hipMemcpyAsync(dproj, proj, sizeof(double) * 2 * nvec, hipMemcpyHostToDevice, e->stream));
    a.proj = dproj;
  }
  SfPlanes pl = {};
  for (int i = 0; i < nfields; ++i) {
    pl.p[canon[i]] = reinterpret_cast<const double*>(planes[i]);
    pl.stride[canon[i]] = 2;
  }
  pl.rows = rows;
  pl.cols = cols;
  sf2_launch(e->stream, nblk, route, pl, a);
  hipLaunchKernelGGL(k_sf_total, dim3((nvec * route.nc + SF_TOTAL_ENTRIES - 1) / SF_TOTAL_ENTRIES), dim3(SF_TOTAL_RUNS * SF_TOTAL_ENTRIES), 0, e->stream, (const double*)a.part,
                     nblk, nvec, route.nc, sf_map(route.nc == sf_ncols<1>() ? 1 : (route.nc == sf_ncols<2>() ? 2 : 3), nfields, canon, ntriples), nout, 0, tab);
  ANYCHK(e, hipGetLastError());
  ANYCHK(e, hipMemcpyAsync(out, tab, sizeof(double) * nvec * nout, hipMemcpyDeviceToHost, e->stream));
  return nq_any_sync(e);
}
// PDFs of the increments on engine planes: nq_increment_hist2's plane kernel, the counts of one state
int nq_any_increment_hist(nq_any* e, int nfields, const void* const* planes, const int* what, int rows, int cols, int nvec, const int* vecs,
                          const double* proj, int proj_a, int proj_b, const double* lo, const double* hi, int bins, unsigned long long* out) {
  if (!e || !planes || !what || !out || rows < 1 || cols < 2) return -1;
  if (nfields < 1 || nfields > SF_MAX_FIELDS) ANYFAIL(e, -1, "nq_any_increment_hist: %d fields (1 to %d)", nfields, SF_MAX_FIELDS);
  bool cplx[SF_MAX_FIELDS] = {};
  for (int i = 0; i < nfields; ++i) {
    if (!planes[i]) ANYFAIL(e, -1, "nq_any_increment_hist: plane %d is null", i);
    if (what[i] != 0 && what[i] != 2) ANYFAIL(e, -1, "nq_any_increment_hist: what[%d] = %d (0: Re, 2: complex)", i, what[i]);
    cplx[i] = what[i] == 2;
  }
  Sf2Args a;
  int canon[SF_MAX_FIELDS] = {};
  Sf2Vec sorted[SF2_MAX_VECS];
  if (const char* bad = sf2_plan(rows, cols, nfields, cplx, nvec, vecs, proj, proj_a, proj_b, 0, nullptr, &a, canon, sorted))
    ANYFAIL(e, -1, "nq_any_increment_hist: %s", bad);
  if (const char* bad = ipdf_check_ranges(nvec, nfields, lo, hi, bins)) ANYFAIL(e, -1, "nq_any_increment_hist: %s", bad);
  ANYCHK(e, hipSetDevice(e->device));
  const int cells = nvec * nfields;
  const size_t words = (size_t)cells * (bins + 3);
  std::vector<double> rng((size_t)3 * cells);
  for (int i = 0; i < cells; ++i) {
    rng[3 * i] = lo[i];
    rng[3 * i + 1] = hi[i];
    rng[3 * i + 2] = (double)bins / (hi[i] - lo[i]);
  }
  IpdfArgs g = {};
  unsigned long long* tab = nullptr;
  double *drng = nullptr, *dproj = nullptr;
  Sf2Vec* dvecs = nullptr;
  AnyScratch tmp;
  ANYCHK(e, tmp.get(&tab, words));
  ANYCHK(e, tmp.get(&drng, rng.size()));
  ANYCHK(e, tmp.get(&dvecs, (size_t)nvec));
  ANYCHK(e, hipMemsetAsync(tab, 0, sizeof(unsigned long long) * words, e->stream));
  ANYCHK(e, hipMemcpyAsync(drng, rng.data(), sizeof(double) * rng.size(), hipMemcpyHostToDevice, e->stream));
  ANYCHK(e, hipMemcpyAsync(dvecs, sorted, sizeof(Sf2Vec) * nvec, hipMemcpyHostToDevice, e->stream));
  if (proj) {
    ANYCHK(e, tmp.get(&dproj, (size_t)2 * nvec));
    ANYCHK(e, hipMemcpyAsync(dproj, proj, sizeof(double) * 2 * nvec, hipMemcpyHostToDevice, e->stream));
  }
  g.nsep = nvec;
  g.vecs = dvecs;
  g.proj = dproj;
  g.pa = a.pa;
  g.pb = a.pb;
  g.nreal = a.nreal;
  g.phi = a.phi;
  g.nfields = nfields;
  g.bins = bins;
  g.rng = drng;
  g.tab = tab;
  SfPlanes pl = {};
  for (int i = 0; i < nfields; ++i) {
    g.out[canon[i]] = i;
    pl.p[canon[i]] = reinterpret_cast<const double*>(planes[i]);
    pl.stride[canon[i]] = 2;
  }
  pl.rows = rows;
  pl.cols = cols;
  ipdf_plane_launch(e->stream, pl, g);
  ANYCHK(e, hipGetLastError());
  ANYCHK(e, hipMemcpyAsync(out, tab, sizeof(unsigned long long) * words, hipMemcpyDeviceToHost, e->stream));
  return nq_any_sync(e);
}
// Vortex census on engine planes: nq_vortex_census's kernels on complex planes whose real parts are the fields
int nq_any_components(nq_any* e, int nplanes, const void* const* planes, int rows, int cols, int crit, int mode, double threshold, int connectivity,
                      int capacity, long long* info, long long* table, int* labels) {
  if (!e || !planes || !info || !table) return -1;
  if (nplanes < 1 || nplanes > VX_MAX_FIELDS) ANYFAIL(e, -1, "nq_any_components: %d planes (1 to %d)", nplanes, VX_MAX_FIELDS);
  if (rows < 4 || cols < 4 || (rows & 1) || (cols & 1) || rows > VX_MAX_DIM || cols > VX_MAX_DIM)
    ANYFAIL(e, -1, "nq_any_components: planes of %d x %d (even sizes from 4 to %d)", rows, cols, VX_MAX_DIM);
  for (int i = 0; i < nplanes; ++i) {
    if (!planes[i]) ANYFAIL(e, -1, "nq_any_components: plane %d is null", i);
    for (int k = 0; k < i; ++k)
      if (planes[k] == planes[i]) ANYFAIL(e, -1, "nq_any_components: plane %d listed twice", i);
  }
  if (const char* bad = vx_check_call(crit, nplanes, mode, threshold, connectivity, capacity)) ANYFAIL(e, -1, "nq_any_components: %s", bad);
  ANYCHK(e, hipSetDevice(e->device));
  AnyScratch tmp;
  char *dplanes = nullptr, *dsmall = nullptr, *dtab = nullptr;
  ANYCHK(e, tmp.get(&dplanes, vx_planes_bytes(rows, cols)));
  ANYCHK(e, tmp.get(&dsmall, vx_small_bytes(rows)));
  ANYCHK(e, tmp.get(&dtab, vx_tab_bytes(capacity)));
  const VxBufs b = vx_bufs(dplanes, dsmall, dtab, rows, cols);
  VxPlanes pl = {};
  for (int i = 0; i < nplanes; ++i) {
    pl.p[i] = reinterpret_cast<const double*>(planes[i]);
    pl.stride[i] = 2;
  }
  pl.nf = nplanes;
  pl.crit = crit;
  pl.rows = rows;
  pl.cols = cols;
  vx_census_launch(e->stream, pl, mode, threshold, connectivity, capacity, b);
  ANYCHK(e, hipGetLastError());
  ANYCHK(e, hipMemcpyAsync(info, b.info, sizeof(long long) * VX_INFO, hipMemcpyDeviceToHost, e->stream));
  if (labels) ANYCHK(e, hipMemcpyAsync(labels, b.L, sizeof(int) * (size_t)rows * cols, hipMemcpyDeviceToHost, e->stream));
  {
    const int rc = nq_any_sync(e);
    if (rc) return rc;
  }
  if (info[1] > 0) {
    ANYCHK(e, hipMemcpyAsync(table, b.tab, sizeof(long long) * (size_t)info[1] * (VX_BASE_COLS + nplanes), hipMemcpyDeviceToHost, e->stream));
    return nq_any_sync(e);
  }
  return 0;
}
int nq_any_set_elem(nq_any* e, void* plane, long long index, double re, double im) {
  if (!e || !plane || index < 0) return -1;
  ANYCHK(e, hipSetDevice(e->device));
  hipLaunchKernelGGL(k_any_set_elem, dim3(1), dim3(1), 0, e->stream, reinterpret_cast<cd*>(plane), (size_t)index, re, im);
  ANYCHK(e, hipGetLastError());
  return 0;
}
// Lagrangian particles on the any-size path: the fused contexts' RK4 step and interpolation on engine
// planes; pos: n complex x + i y (unwrapped), U0 / U1 / plane: (nx, nx) complex planes (velocity planes: u + i v)
int nq_any_particles_rk4(nq_any* e, void* pos, int n, const void* U0, const void* U1, int nx, double Lx, double Ly, double Ub,
                         double dt) {
  if (!e || !pos || !U0 || !U1 || n < 1 || nx < 1) return -1;
  if (!(Lx > 0.0) || !(Ly > 0.0)) ANYFAIL(e, -1, "nq_any_particles_rk4: domain %g x %g", Lx, Ly);
  ANYCHK(e, hipSetDevice(e->device));
  const PtGrid g{nx, Lx, Ly, Lx / nx, Ly / nx};
  hipLaunchKernelGGL(k_pt_rk4_c, dim3(pt_blocks(n)), dim3(256), 0, e->stream, reinterpret_cast<cd*>(pos), n, reinterpret_cast<const cd*>(U0),
                     reinterpret_cast<const cd*>(U1), g, Ub, dt);
  ANYCHK(e, hipGetLastError());
  return 0;
}
int nq_any_interp(nq_any* e, void* out, const void* plane, const void* pos, int n, int nx, double Lx, double Ly) {
  if (!e || !out || !plane || !pos || n < 1 || nx < 1) return -1;
  if (!(Lx > 0.0) || !(Ly > 0.0)) ANYFAIL(e, -1, "nq_any_interp: domain %g x %g", Lx, Ly);
  ANYCHK(e, hipSetDevice(e->device));
  const PtGrid g{nx, Lx, Ly, Lx / nx, Ly / nx};
  hipLaunchKernelGGL(k_pt_interp_c, dim3(pt_blocks(n)), dim3(256), 0, e->stream, reinterpret_cast<cd*>(out), reinterpret_cast<const cd*>(plane),
                     reinterpret_cast<const cd*>(pos), n, g);
  ANYCHK(e, hipGetLastError());
  return 0;
}
// Drifter mode on engine planes: the step of nq_particles_wave from time t, P0 / P1 the physical phi of
// the state the step starts from and of the state after it; and a phi e^{-i f0 t} at the particles.  The phases are formed here,
// on the host.
int nq_any_particles_rk4_wave(nq_any* e, void* pos, int n, const void* U0, const void* U1, const void* P0, const void* P1, int nx, double Lx,
                              double Ly, double Ub, double dt, double amplitude, double f0, double t) {
  if (!e || !pos || !U0 || !U1 || !P0 || !P1 || n < 1 || nx < 1) return -1;
  if (!(Lx > 0.0) || !(Ly > 0.0)) ANYFAIL(e, -1, "nq_any_particles_rk4_wave: domain %g x %g", Lx, Ly);
  if (!(amplitude > 0.0) || !std::isfinite(amplitude) || !std::isfinite(f0) || !std::isfinite(t))
    ANYFAIL(e, -1, "nq_any_particles_rk4_wave: amplitude = %g (finite, > 0), f0 = %g, t = %g", amplitude, f0, t);
  ANYCHK(e, hipSetDevice(e->device));
  const PtGrid g{nx, Lx, Ly, Lx / nx, Ly / nx};
  PtWave wv;
  wv.a = amplitude;
  pt_phase(f0, t, &wv.c[0], &wv.s[0]);
  pt_phase(f0, t + 0.5 * dt, &wv.c[1], &wv.s[1]);
  pt_phase(f0, t + dt, &wv.c[2], &wv.s[2]);
  hipLaunchKernelGGL(k_pt_rk4_wc, dim3(pt_blocks(n)), dim3(256), 0, e->stream, reinterpret_cast<cd*>(pos), n, reinterpret_cast<const cd*>(U0),
                     reinterpret_cast<const cd*>(U1), reinterpret_cast<const cd*>(P0), reinterpret_cast<const cd*>(P1), g, Ub, dt, wv);
  ANYCHK(e, hipGetLastError());
  return 0;
}
int nq_any_interp_wave(nq_any* e, void* out, const void* phi, const void* pos, int n, int nx, double Lx, double Ly, double amplitude, double f0,
                       double t) {
  if (!e || !out || !phi || !pos || n < 1 || nx < 1) return -1;
  if (!(Lx > 0.0) || !(Ly > 0.0)) ANYFAIL(e, -1, "nq_any_interp_wave: domain %g x %g", Lx, Ly);
  if (!std::isfinite(amplitude) || !std::isfinite(f0) || !std::isfinite(t))
    ANYFAIL(e, -1, "nq_any_interp_wave: amplitude = %g, f0 = %g, t = %g", amplitude, f0, t);
  ANYCHK(e, hipSetDevice(e->device));
  const PtGrid g{nx, Lx, Ly, Lx / nx, Ly / nx};
  double co, si;
  pt_phase(f0, t, &co, &si);
  hipLaunchKernelGGL(k_pt_interp_wc, dim3(pt_blocks(n)), dim3(256), 0, e->stream, reinterpret_cast<cd*>(out), reinterpret_cast<const cd*>(phi),
                     reinterpret_cast<const cd*>(pos), n, g, amplitude, co, si);
  ANYCHK(e, hipGetLastError());
  return 0;
}
// Ray mode on engine planes: the step of nq_particles_rays, wv = k + i l beside pos = x + i y, Z0 / Z1
// complex planes with zeta in the real part (every engine plane is complex); and omega at the rays.
int nq_any_particles_rk4_rays(nq_any* e, void* pos, void* wv, int n, const void* U0, const void* U1, const void* Z0, const void* Z1, int nx,
                              double Lx, double Ly, double Ub, double eta, double dt) {
  if (!e || !pos || !wv || !U0 || !U1 || !Z0 || !Z1 || n < 1 || nx < 1) return -1;
  if (!(Lx > 0.0) || !(Ly > 0.0)) ANYFAIL(e, -1, "nq_any_particles_rk4_rays: domain %g x %g", Lx, Ly);
  if (!std::isfinite(eta)) ANYFAIL(e, -1, "nq_any_particles_rk4_rays: eta = %g", eta);
  ANYCHK(e, hipSetDevice(e->device));
  const PtGrid g{nx, Lx, Ly, Lx / nx, Ly / nx};
  hipLaunchKernelGGL(k_pt_rk4_rc, dim3(pt_blocks(n)), dim3(256), 0, e->stream, reinterpret_cast<cd*>(pos), reinterpret_cast<cd*>(wv), n,
                     reinterpret_cast<const cd*>(U0), reinterpret_cast<const cd*>(U1), reinterpret_cast<const cd*>(Z0),
                     reinterpret_cast<const cd*>(Z1), g, Ub, eta, dt);
  ANYCHK(e, hipGetLastError());
  return 0;
}
int nq_any_interp_omega(nq_any* e, void* out, const void* U, const void* Z, const void* pos, const void* wv, int n, int nx, double Lx, double Ly,
                        double Ub, double eta) {
  if (!e || !out || !U || !Z || !pos || !wv || n < 1 || nx < 1) return -1;
  if (!(Lx > 0.0) || !(Ly > 0.0)) ANYFAIL(e, -1, "nq_any_interp_omega: domain %g x %g", Lx, Ly);
  if (!std::isfinite(eta)) ANYFAIL(e, -1, "nq_any_interp_omega: eta = %g", eta);
  ANYCHK(e, hipSetDevice(e->device));
  const PtGrid g{nx, Lx, Ly, Lx / nx, Ly / nx};
  hipLaunchKernelGGL(k_pt_omega_c, dim3(pt_blocks(n)), dim3(256), 0, e->stream, reinterpret_cast<cd*>(out), reinterpret_cast<const cd*>(U),
                     reinterpret_cast<const cd*>(Z), reinterpret_cast<const cd*>(pos), reinterpret_cast<const cd*>(wv), n, g, Ub, eta);
  ANYCHK(e, hipGetLastError());
  return 0;
}
// Stretch mode on engine planes: the step of nq_particles_tangent, fa = f11 + i f21 and fb = f12 + i f22
// beside pos = x + i y; with the wave, drifter mode's velocity and its gradient from P0 / P1 at time t
int nq_any_particles_rk4_tangent(nq_any* e, void* pos, void* fa, void* fb, int n, const void* U0, const void* U1, int nx, double Lx, double Ly,
                                 double Ub, double dt) {
  if (!e || !pos || !fa || !fb || !U0 || !U1 || n < 1 || nx < 1) return -1;
  if (!(Lx > 0.0) || !(Ly > 0.0)) ANYFAIL(e, -1, "nq_any_particles_rk4_tangent: domain %g x %g", Lx, Ly);
  ANYCHK(e, hipSetDevice(e->device));
  const PtGrid g = {nx, Lx, Ly, Lx / nx, Ly / nx};
  hipLaunchKernelGGL(k_pt_rk4_tc, dim3(pt_blocks(n)), dim3(256), 0, e->stream, reinterpret_cast<cd*>(pos), reinterpret_cast<cd*>(fa),
                     reinterpret_cast<cd*>(fb), n, reinterpret_cast<const cd*>(U0), reinterpret_cast<const cd*>(U1), g, Ub, dt);
  ANYCHK(e, hipGetLastError());
  return 0;
}
int nq_any_particles_rk4_wave_tangent(nq_any* e, void* pos, void* fa, void* fb, int n, const void* U0, const void* U1, const void* P0, const void* P1,
                                      int nx, double Lx, double Ly, double Ub, double dt, double amplitude, double f0, double t) {
  if (!e || !pos || !fa || !fb || !U0 || !U1 || !P0 || !P1 || n < 1 || nx < 1) return -1;
  if (!(Lx > 0.0) || !(Ly > 0.0)) ANYFAIL(e, -1, "nq_any_particles_rk4_wave_tangent: domain %g x %g", Lx, Ly);
  if (!(amplitude > 0.0) || !std::isfinite(amplitude) || !std::isfinite(f0) || !std::isfinite(t))
    ANYFAIL(e, -1, "nq_any_particles_rk4_wave_tangent: amplitude = %g (finite, > 0), f0 = %g, t = %g", amplitude, f0, t);
  ANYCHK(e, hipSetDevice(e->device));
  const PtGrid g = {nx, Lx, Ly, Lx / nx, Ly / nx};
  PtWave wv;
  wv.a = amplitude;
  pt_phase(f0, t, &wv.c[0], &wv.s[0]);
  pt_phase(f0, t + 0.5 * dt, &wv.c[1], &wv.s[1]);
  pt_phase(f0, t + dt, &wv.c[2], &wv.s[2]);
  hipLaunchKernelGGL(k_pt_rk4_wtc, dim3(pt_blocks(n)), dim3(256), 0, e->stream, reinterpret_cast<cd*>(pos), reinterpret_cast<cd*>(fa),
                     reinterpret_cast<cd*>(fb), n, reinterpret_cast<const cd*>(U0), reinterpret_cast<const cd*>(U1), reinterpret_cast<const cd*>(P0),
                     reinterpret_cast<const cd*>(P1), g, Ub, dt, wv);
  ANYCHK(e, hipGetLastError());
  return 0;
}
// out[i] = ln sigma_1 (which 0) or det F (1) of the columns fa[i], fb[i], imaginary part 0
int nq_any_tangent_value(nq_any* e, void* out, const void* fa, const void* fb, int n, int which) {
  if (!e || !out || !fa || !fb || n < 1 || which < 0 || which > 1) return -1;
  ANYCHK(e, hipSetDevice(e->device));
  const double *a = static_cast<const double*>(fa), *b = static_cast<const double*>(fb);
  hipLaunchKernelGGL(k_pt_tan_value, dim3(pt_blocks(n)), dim3(256), 0, e->stream, a, b, a + 1, b + 1, 2, n, which, static_cast<double*>(out), 2);
  ANYCHK(e, hipGetLastError());
  return 0;
}
// Stochastic forcing on engine planes: plane += sqrt_dt Re(amp) xi with the generator, counters and
// Hermitian rule of the fused contexts.  layout 0: (rows, rows/2+1) half spectrum, the q rule; 1: full (rows, rows) plane,
// independent values of `stream`; 2: full plane, the Hermitian extension of the q rule (the reference's full-plane qh).
// work_in (null: none) is the plane W of the work sums, read before the increment (it may be `plane` itself):
// out2 = {sum w Re(conj(W) D), sum w |D|^2} / M^2 with the half-spectrum weights on layout 0.
int nq_any_forcing(nq_any* e, void* plane, const void* amp, int rows, int cols, int layout, unsigned long long seed, long long s, int stream,
                   double sqrt_dt, const void* work_in, double* out2) {
  if (!e || !plane || !amp || rows < 2 || (rows & 1) || s < 0) return -1;
  if (layout < 0 || layout > 2) ANYFAIL(e, -1, "nq_any_forcing: layout %d (0: half plane, 1: full plane, 2: full plane, Hermitian)", layout);
  if (cols != (layout == 0 ? rows / 2 + 1 : rows)) ANYFAIL(e, -1, "nq_any_forcing: %d columns for layout %d of %d rows", cols, layout, rows);
  if (stream != 0 && stream != 1) ANYFAIL(e, -1, "nq_any_forcing: stream %d", stream);
  if ((work_in == nullptr) != (out2 == nullptr)) ANYFAIL(e, -1, "nq_any_forcing: work_in and work_out2 go together");
  ANYCHK(e, hipSetDevice(e->device));
  const FcBox b = {rows, rows / 2, layout == 0 ? rows / 2 : rows / 2, rows, cols};      // the whole plane (A lives on the device)
  const dim3 g = fc_grid(b);
  const int np = (int)(g.x * g.y);
  double* part = nullptr;
  AnyScratch tmp;
  if (out2) ANYCHK(e, tmp.get(&part, (size_t)2 * np + 2));
  const uint32_t s32 = (uint32_t)((unsigned long long)s & 0xffffffffull);
  cd* y = reinterpret_cast<cd*>(plane);
  const cd *A = reinterpret_cast<const cd*>(amp), *W = reinterpret_cast<const cd*>(work_in);
  if (layout == 0)
    hipLaunchKernelGGL(k_force_half<cd>, g, dim3(64, 4), 0, e->stream, y, (cd*)nullptr, cols, A, b, sqrt_dt, s32, seed, W, cols, (const double*)nullptr,
                       (const double*)nullptr, part, (cd*)nullptr);
  else if (layout == 1)
    hipLaunchKernelGGL((k_force_full<cd, false>), g, dim3(64, 4), 0, e->stream, y, A, b, sqrt_dt, s32, (uint32_t)stream, seed, W, (const double*)nullptr,
                       (const double*)nullptr, part, (cd*)nullptr);
  else
    hipLaunchKernelGGL((k_force_full<cd, true>), g, dim3(64, 4), 0, e->stream, y, A, b, sqrt_dt, s32, 0u, seed, W, (const double*)nullptr,
                       (const double*)nullptr, part, (cd*)nullptr);
  ANYCHK(e, hipGetLastError());
  if (!out2) return 0;
  const double M = (double)rows * rows;
  hipLaunchKernelGGL(k_force_accum, dim3(1), dim3(256), 0, e->stream, (const double*)part, np, (const double*)nullptr, 0, 1.0 / (M * M), (double*)nullptr,
                     part + 2 * np);
  ANYCHK(e, hipMemcpyAsync(out2, part + 2 * np, sizeof(double) * 2, hipMemcpyDeviceToHost, e->stream));
  return nq_any_sync(e);
}
// ETDRK4 planes of the linear operator c(l, k) on the whole (n, cols) plane, no filter folded in (the any-size path multiplies by
// `filtr` as the reference does): eq as k_etdrk4_coeffs (0 q Kernel family, 1 phi, 2 QGModel's q, 3 its passive scalar);
// kk (cols values), ll (n values) host arrays; out6: E, Eh, Q, f0, fab, fc planes of this engine.
// near_*: the entries within delta of the contour (at most cap), for the host to recompute (niwqg_amd/_etdrk4.py) and hand back
int nq_any_etdrk4(nq_any* e, int eq, const nq_params* p, const double* kk, const double* ll, const double* contour32, int n, int cols,
                  void* const* out6, double delta, int cap, int* near_count, int* near_l, int* near_k) {
  if (!e || !p || !kk || !ll || !contour32 || !out6 || n < 2 || cols < 1 || eq < 0 || eq > 3) return -1;
  ANYCHK(e, hipSetDevice(e->device));
  double *dk = nullptr, *dl = nullptr;
  cd* dc = nullptr;
  int *cnt = nullptr, *lo = nullptr, *ko = nullptr;
  AnyScratch tmp;
  ANYCHK(e, tmp.get(&dk, cols));
  ANYCHK(e, tmp.get(&dl, n));
  ANYCHK(e, tmp.get(&dc, 32));
  ANYCHK(e, hipMemcpy(dk, kk, sizeof(double) * cols, hipMemcpyHostToDevice));
  ANYCHK(e, hipMemcpy(dl, ll, sizeof(double) * n, hipMemcpyHostToDevice));
  ANYCHK(e, hipMemcpy(dc, contour32, sizeof(cd) * 32, hipMemcpyHostToDevice));
  cd* o[6];
  for (int i = 0; i < 6; ++i) o[i] = reinterpret_cast<cd*>(out6[i]);
  hipLaunchKernelGGL(k_etdrk4_coeffs, dim3((cols + 63) / 64, n), dim3(64), 0, e->stream, eq, n, cols, cols, 0, *p, (const double*)dk, (const double*)dl,
                     (const double*)nullptr, (const cd*)dc, o[0], o[1], o[2], o[3], o[4], o[5]);
  int found = 0;
  if (near_count && near_l && near_k && cap > 0) {
    ANYCHK(e, tmp.get(&cnt, 1));
    ANYCHK(e, tmp.get(&lo, cap));
    ANYCHK(e, tmp.get(&ko, cap));
    ANYCHK(e, hipMemsetAsync(cnt, 0, sizeof(int), e->stream));
    hipLaunchKernelGGL(k_coeff_flag, dim3((cols + 63) / 64, n), dim3(64), 0, e->stream, eq, n, cols, 0, *p, (const double*)dk, (const double*)dl, (const cd*)dc,
                       delta * delta, cap, cnt, lo, ko);
    ANYCHK(e, hipMemcpyAsync(&found, cnt, sizeof(int), hipMemcpyDeviceToHost, e->stream));
    ANYCHK(e, hipStreamSynchronize(e->stream));
    const int take = found < cap ? found : cap;
    if (take > 0) {
      ANYCHK(e, hipMemcpy(near_l, lo, sizeof(int) * take, hipMemcpyDeviceToHost));
      ANYCHK(e, hipMemcpy(near_k, ko, sizeof(int) * take, hipMemcpyDeviceToHost));
    }
    *near_count = found;
  }
  ANYCHK(e, hipStreamSynchronize(e->stream));
  ANYCHK(e, hipGetLastError());
  return 0;
}
// vals: count x 4 complex (Qh, f0, fab, fc) for the entries (l, k) of a (n, cols) plane set
int nq_any_etdrk4_patch(nq_any* e, void* const* out6, int cols, int count, const int* l, const int* k, const double* vals) {
  if (!e || !out6 || count < 0 || (count > 0 && (!l || !k || !vals))) return -1;
  if (count == 0) return 0;
  ANYCHK(e, hipSetDevice(e->device));
  int *dl = nullptr, *dk = nullptr;
  cd* dv = nullptr;
  AnyScratch tmp;
  ANYCHK(e, tmp.get(&dl, count));
  ANYCHK(e, tmp.get(&dk, count));
  ANYCHK(e, tmp.get(&dv, (size_t)4 * count));
  ANYCHK(e, hipMemcpy(dl, l, sizeof(int) * count, hipMemcpyHostToDevice));
  ANYCHK(e, hipMemcpy(dk, k, sizeof(int) * count, hipMemcpyHostToDevice));
  ANYCHK(e, hipMemcpy(dv, vals, sizeof(cd) * 4 * count, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_coeff_patch, dim3((count + 255) / 256), dim3(256), 0, e->stream, count, (const int*)dl, (const int*)dk, (const cd*)dv, cols, cols, 0,
                     (const double*)nullptr, reinterpret_cast<cd*>(out6[2]), reinterpret_cast<cd*>(out6[3]), reinterpret_cast<cd*>(out6[4]), reinterpret_cast<cd*>(out6[5]), 0);
  ANYCHK(e, hipStreamSynchronize(e->stream));
  return 0;
}

}  // extern "C"

// ==================================================================================================================
// Low-mode time series recorded in the step, frequency - wavenumber spectra on the device (DESIGN.md section 5j;
// kernels: csrc/nq_freq.hpp, included here because k_fq_bin walks the shells with shell_run above)
// ==================================================================================================================
#include "nq_freq.hpp"
static_assert(NqFreq::NF == FQ_NFIELDS, "NqFreq holds one ring per recordable field");

// one record of every attached field from the buffers that hold the current state (what nq_get_field reads), one launch
static int fq_record(nq_ctx* c) {
  NqFreq* F = c->fq;
  const int slot = F->rg.slot(), R = 2 * F->K + 1;
  FqRecord a = {};
  int maxc = 0;
  for (int f = 0; f < F->nf; ++f) {
    const int id = F->field[f];
    a.src[f] = id == FQ_PHI ? c->w.y[c->w.cur] : (id == FQ_Q ? c->q.y[c->q.cur] : c->ph);
    a.pitch[f] = id == FQ_PHI ? c->N : c->Ph;
    a.ncols[f] = F->ncols[f];
    a.proj[f] = (id == FQ_PSI && c->kernel_family) ? 1 : 0;
    a.dst[f] = F->ring[f] + (size_t)slot * R * F->ncols[f];
    if (F->ncols[f] > maxc) maxc = F->ncols[f];
  }
  hipLaunchKernelGGL(k_fq_record, dim3((maxc + 63) / 64, (R + 3) / 4, F->nf), dim3(64, 4), 0, c->stream, a, c->N, F->K);
  HIPCHK(c, hipGetLastError());
  F->rg.wrote();
  return 0;
}
static int fq_after_step(nq_ctx* c) {
  return c->fq->rg.tick() ? fq_record(c) : 0;
}
static int fq_find(const NqFreq* F, int field) {
  for (int f = 0; f < F->nf; ++f)
    if (F->field[f] == field) return f;
  return -1;
}
// The spectrum pass on the engine's stream: window -> transform along the record axis -> bin.  ring: [length][2K+1][ncols];
// work: T x modes; dwin: T; dtab: T x nb (device); out: T x nb (host), row p = FFT bin p (omega_p = 2 pi fftfreq(T, Delta)[p]).
static int fq_spectrum_run(nq_any* e, const cd* ring, int N, int K, int ncols, int full, int kappa, int length, int first, int T,
                           const double* window, int demean, double dk, int nb, cd* work, double* dwin, double* dtab, double* out) {
  const int nm = (2 * K + 1) * ncols;
  double sw2 = 0.0;
  for (int n = 0; n < T; ++n) sw2 += window[n] * window[n];
  if (!(sw2 > 0.0)) ANYFAIL(e, -1, "frequency spectrum: the window is zero everywhere");
  const double M = (double)N * N, scale = 0.5 / (M * M * (double)T * sw2);
  ANYCHK(e, hipMemcpyAsync(dwin, window, sizeof(double) * T, hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL(k_fq_window, dim3((nm + 255) / 256), dim3(256), 0, e->stream, ring, work, (const double*)dwin, nm, length, first, T, demean ? 1 : 0);
  ANYCHK(e, hipGetLastError());
  const int rc = nq_any_fft(e, work, work, T, nm, 0, 0);
  if (rc) return rc;
  hipLaunchKernelGGL(k_fq_bin, dim3(nb, T), dim3(256), 0, e->stream, (const cd*)work, T, K, ncols, full, kappa, dk * dk, scale, nb, dtab);
  ANYCHK(e, hipGetLastError());
  ANYCHK(e, hipMemcpyAsync(out, dtab, sizeof(double) * (size_t)T * nb, hipMemcpyDeviceToHost, e->stream));
  return nq_any_sync(e);
}

// ---- time-mean and covariance maps (kernels: csrc/nq_avg.hpp) ----------------------------------------
// slot of a public field id: hist_slot's for the real fields, AVG_PHI for the Kernel family's phi
static int av_slot(const nq_ctx* c, int field) {
  if (field == NQ_AVG_PHI) return c->kernel_family ? AVG_PHI : -1;
  return hist_slot(c, field);
}
// one sample: the current state (what nq_field_hist bins) is added to every sum plane, one launch
static int av_sample(nq_ctx* c, const char* what) {
  NqAvg* A = c->av;
  if (c->kernel_family ? !c->have_phi : !c->have_q) NQ_FAIL(c, -4, "%s: %s has not been called", what, c->kernel_family ? "set_phi" : "set_q");
  if (c->kernel_family) {
    if (A->flow) flow_moments(c, A->sel, A->args);
    else launch_xmoments(c, A->args);
  } else {
    AvgSrc s = {};
    hist_qg_planes(c, A->args.mask, &s.p[0], &s.p[1]);
    s.stride[0] = s.stride[1] = 1;
    const size_t n = (size_t)c->N * c->N;
    hipLaunchKernelGGL(k_moments_plane, dim3(hist_plane_grid(n)), dim3(256), 0, c->stream, s, n, A->args);
  }
  HIPCHK(c, hipGetLastError());
  ++A->rg.count;
  return 0;
}
static int av_after_step(nq_ctx* c) {
  return c->av->rg.tick() ? av_sample(c, "nq_step (averages)") : 0;
}

// ---- time-mean spectra, transfer and flux (kernel: csrc/nq_tspec.hpp) -------------------------------------
// one sample: the device parts of nq_diagnostics_binned and / or nq_transfer_binned on the current state -- with both bodies, each
// products pass once for the two of them -- and one launch that adds what they left in spec_out / tr_out to the sums.  Nothing is
// downloaded and the host does not wait; the planes and tables the bodies write were allocated at attach.
static int ts_sample(nq_ctx* c, const char* what) {
  NqTspec* T = c->ts;
  const bool sp = T->mask & NQ_TSPEC_SPECTRA, tr = T->mask & NQ_TSPEC_TRANSFER;
  std::vector<nq_ctx*> grp(1, c);
  if (sp && tr) SLABTRY(tick_both_device(c, what, T->nb));
  else if (sp) SLABTRY(tick_binned_device(grp, what, T->nb));
  else SLABTRY(tick_transfer_device(grp, what, T->nb));
  TspecArgs a = T->args;
  a.spec = sp ? c->spec_out : nullptr;
  a.tr = tr ? c->tr_out : nullptr;
  hipLaunchKernelGGL(k_tspec_accumulate, dim3(tspec_grid(sp, tr, T->nb)), dim3(TSPEC_THREADS), 0, c->stream, a);
  HIPCHK(c, hipGetLastError());
  ++T->rg.count;
  return 0;
}
static int ts_after_step(nq_ctx* c) {
  return c->ts->rg.tick() ? ts_sample(c, "nq_step (time-mean spectra)") : 0;
}

// ---- nq_step's hooks (declared below dev_alloc) ----------------------------------------------------------------------------
// Before the step the particles form U0 from the state it starts from.  After it: the forcing first -- the forced, re-inverted
// state is what the particles' U1 and the next step see -- then the particles, then the recorder, whose record of this step
// is that same forced, re-inverted state, then the averages, which add that state to their sums, and last the time-mean spectra,
// whose sample is what the binned host calls would return right after this step.  The first non-zero return code ends the call.
static void attachments_before_step(nq_ctx* c) {
  if (c->pt) pt_before_step(c);
}
static int attachments_after_step(nq_ctx* c) {
  int rc = c->fc ? fc_apply(c) : 0;
  if (!rc && c->pt) rc = pt_after_step(c);
  if (!rc && c->fq) rc = fq_after_step(c);
  if (!rc && c->av) rc = av_after_step(c);
  if (!rc && c->ts) rc = ts_after_step(c);
  return rc;
}

extern "C" {

int nq_freq_attach(nq_ctx* c, int kmax, int every, int length, int nfields, const int* fields) {
  NQ_SINGLE_RANK(c, "nq_freq_attach");
  if (c->fq) NQ_FAIL(c, -4, "nq_freq_attach: a recorder is attached already (nq_freq_detach first)");
  if (kmax < 1 || kmax >= c->N / 2) NQ_FAIL(c, -1, "nq_freq_attach: kmax = %d (1 <= kmax < nx/2 = %d)", kmax, c->N / 2);
  if (every < 1 || length < 2) NQ_FAIL(c, -1, "nq_freq_attach: every = %d (>= 1), length = %d (>= 2)", every, length);
  if (nfields < 1 || nfields > FQ_NFIELDS || !fields) NQ_FAIL(c, -1, "nq_freq_attach: %d fields", nfields);
  for (int f = 0; f < nfields; ++f) {
    if (fields[f] < 0 || fields[f] >= FQ_NFIELDS) NQ_FAIL(c, -1, "nq_freq_attach: field %d (0: phi, 1: q, 2: psi)", fields[f]);
    for (int g = 0; g < f; ++g)
      if (fields[g] == fields[f]) NQ_FAIL(c, -1, "nq_freq_attach: field %d given twice", fields[f]);
    if (fields[f] == FQ_PHI && !c->kernel_family) NQ_FAIL(c, -1, "nq_freq_attach: QGModel has no wave field (q and psi only)");
    if (fields[f] != FQ_PHI && c->ybj) NQ_FAIL(c, -1, "nq_freq_attach: YBJModel's psi is steady (phi only)");
  }
  HIPCHK(c, hipSetDevice(c->device));
  c->fq = new NqFreq();
  NqFreq* F = c->fq;
  F->K = kmax;
  F->nf = nfields;
  F->rg.init(length, every);
  const size_t R = 2 * (size_t)kmax + 1;
  int rc = 0;
  for (int f = 0; f < nfields && !rc; ++f) {
    F->field[f] = fields[f];
    F->ncols[f] = fields[f] == FQ_PHI ? 2 * kmax + 1 : kmax + 1;
    rc = att_alloc(c, F, &F->ring[f], (size_t)length * R * F->ncols[f], "nq_freq_attach");
  }
  if (!rc) rc = fq_record(c);                     // record 0: the state at attach
  if (!rc) rc = nq_sync(c);
  if (rc) return att_fail(c, c->fq, rc);
  return 0;
}
int nq_freq_detach(nq_ctx* c) {
  NQ_SINGLE_RANK(c, "nq_freq_detach");
  if (!c->fq) NQ_FAIL(c, -4, "nq_freq_detach: no recorder attached");
  att_release(c, c->fq);
  return 0;
}
int nq_freq_info(nq_ctx* c, long long* info3) {
  NQ_SINGLE_RANK(c, "nq_freq_info");
  NqFreq* F = c->fq;
  if (!F) NQ_FAIL(c, -4, "nq_freq_info: no recorder attached");
  if (!info3) return -1;
  info3[0] = F->rg.count;
  info3[1] = F->rg.held();
  info3[2] = F->rg.steps;
  return 0;
}
int nq_freq_series(nq_ctx* c, int field, long long* steps, double* out_cplx) {
  NQ_SINGLE_RANK(c, "nq_freq_series");
  NqFreq* F = c->fq;
  if (!F) NQ_FAIL(c, -4, "nq_freq_series: no recorder attached");
  const int f = fq_find(F, field);
  if (f < 0) NQ_FAIL(c, -1, "nq_freq_series: field %d is not recorded", field);
  HIPCHK(c, hipSetDevice(c->device));
  const long long m = F->rg.held();
  const size_t rec = (size_t)(2 * F->K + 1) * F->ncols[f];
  for (long long r = 0; r < m; ++r) {
    const int slot = F->rg.oldest(r);
    if (steps) steps[r] = F->rg.ring_step[slot];
    if (out_cplx)
      HIPCHK(c, hipMemcpyAsync(out_cplx + 2 * (size_t)r * rec, F->ring[f] + (size_t)slot * rec, sizeof(cd) * rec, hipMemcpyDeviceToHost, c->stream));
  }
  return nq_sync(c);
}
int nq_freq_spectrum(nq_ctx* c, int field, const double* window, int demean, double dk, int nb, double* out) {
  NQ_SINGLE_RANK(c, "nq_freq_spectrum");
  NqFreq* F = c->fq;
  if (!F) NQ_FAIL(c, -4, "nq_freq_spectrum: no recorder attached");
  if (!window || !out) return -1;
  const int f = fq_find(F, field);
  if (f < 0) NQ_FAIL(c, -1, "nq_freq_spectrum: field %d is not recorded", field);
  const int T = (int)F->rg.held(), length = F->rg.cap;
  if (T < 2) NQ_FAIL(c, -1, "nq_freq_spectrum: %d record held (at least 2)", T);
  if (nb != nq_shell_of(F->K, F->K) + 1) NQ_FAIL(c, -1, "nq_freq_spectrum: nb = %d, the block has %d shells", nb, nq_shell_of(F->K, F->K) + 1);
  for (int n = 0; n < T; ++n)
    if (!std::isfinite(window[n])) NQ_FAIL(c, -1, "nq_freq_spectrum: the window is not finite at record %d", n);
  if (!std::isfinite(dk) || !(dk > 0.0)) NQ_FAIL(c, -1, "nq_freq_spectrum: dk = %g", dk);
  HIPCHK(c, hipSetDevice(c->device));
  const long long eng_before = F->eng ? nq_any_device_bytes(F->eng) : 0;
  if (!F->work) {                                   // first call: the work plane of a full ring of the widest field, window, table
    int maxc = 0;
    for (int g = 0; g < F->nf; ++g) maxc = F->ncols[g] > maxc ? F->ncols[g] : maxc;
    const char* what = "nq_freq_spectrum";
    const DevMark before = F->mark();
    int rc = att_alloc(c, F, &F->work, (size_t)length * (2 * (size_t)F->K + 1) * maxc, what);
    if (!rc) rc = att_alloc(c, F, &F->win, (size_t)length, what);
    if (!rc) rc = att_alloc(c, F, &F->tab, (size_t)length * nb, what);
    if (!rc && !F->eng) {
      rc = nq_any_create(c->device, &F->eng);
      if (rc) c->err = g_last_error;
    }
    if (rc) {                                       // the recorder stays as it was
      c->bytes -= F->rollback(before);
      F->work = nullptr;
      F->win = F->tab = nullptr;
      return rc;
    }
  }
  int rc = nq_sync(c);                              // every record queued on the context's stream is in the ring
  if (rc) return rc;
  rc = fq_spectrum_run(F->eng, F->ring[f], c->N, F->K, F->ncols[f], field == FQ_PHI ? 1 : 0, field == FQ_PSI ? 1 : 0, length, F->rg.oldest(0), T, window,
                       demean, dk, nb, F->work, F->win, F->tab, out);
  const long long grown = nq_any_device_bytes(F->eng) - eng_before;      // the engine's work rows count as the recorder's
  F->bytes += grown;
  c->bytes += grown;
  if (rc) NQ_FAIL(c, rc, "nq_freq_spectrum: %s", nq_any_last_error(F->eng));
  return 0;
}

// ---- time-mean and covariance maps ---------------------------------------------------------------------
int nq_avg_attach(nq_ctx* c, int nfields, const int* fields, int nproducts, const int* pairs, int every) {
  NQ_SINGLE_RANK(c, "nq_avg_attach");
  if (c->av) NQ_FAIL(c, -4, "nq_avg_attach: averages are attached already (nq_avg_detach first)");
  if (!fields || nfields < 1 || nfields > AVG_SLOTS + 1) NQ_FAIL(c, -1, "nq_avg_attach: %d fields (1 to %d)", nfields, AVG_SLOTS + 1);
  if (nproducts < 0 || nproducts > AVG_MAX_PRODUCTS || (nproducts > 0 && !pairs)) NQ_FAIL(c, -1, "nq_avg_attach: %d products (0 to %d)", nproducts, AVG_MAX_PRODUCTS);
  if (every < 0) NQ_FAIL(c, -1, "nq_avg_attach: every = %d (>= 0)", every);
  // slots: a list of old fields keeps av_slot's; one that names a flow field (Kernel family) takes the real fields in list order
  const bool flow = any_flow(nfields, fields);
  int mask = 0, slot[AVG_SLOTS + 1], nreal = 0;
  FlowSel sel = flow_sel_none(c);
  for (int i = 0; i < nfields; ++i) {
    if (is_flow(fields[i]) && !c->kernel_family)
      NQ_FAIL(c, -1, "nq_avg_attach: flow field %d (NQ_FLOW_*) on a QGModel context: its plane route has no velocity or strain values yet (DESIGN.md section 7)", fields[i]);
    int s = is_flow(fields[i]) ? 0 : av_slot(c, fields[i]);
    if (s < 0)
      NQ_FAIL(c, -1, "nq_avg_attach: field %d is not available here (Kernel family: NQ_AVG_Q, NQ_AVG_QPSI, NQ_AVG_PHI2, NQ_AVG_PHI and the NQ_FLOW_* fields; QGModel: NQ_AVG_Q, with its passive scalar NQ_AVG_C)", fields[i]);
    for (int k = 0; k < i; ++k)
      if (fields[k] == fields[i]) NQ_FAIL(c, -1, "nq_avg_attach: field %d listed twice", fields[i]);
    if (s != AVG_PHI) {
      if (nreal == AVG_SLOTS) NQ_FAIL(c, -1, "nq_avg_attach: more than %d real fields", AVG_SLOTS);
      if (flow) {
        s = nreal;
        sel.code[s] = fields[i];
      }
      ++nreal;
    } else {
      sel.phi = 1;
    }
    slot[i] = s;
    mask |= 1 << s;
  }
  int pa[AVG_MAX_PRODUCTS], pb[AVG_MAX_PRODUCTS];
  for (int p = 0; p < nproducts; ++p) {
    int s[2];
    for (int k = 0; k < 2; ++k) {
      const int f = pairs[2 * p + k];
      s[k] = -1;
      for (int i = 0; i < nfields; ++i)
        if (fields[i] == f && slot[i] != AVG_PHI) s[k] = slot[i];
      if (s[k] < 0)
        NQ_FAIL(c, -1, "nq_avg_attach: product %d names field %d, which is not a real field of the list", p, f);
    }
    pa[p] = s[0] < s[1] ? s[0] : s[1];
    pb[p] = s[0] < s[1] ? s[1] : s[0];
    if (flow && pa[p] != pb[p] && nreal > flow_nv_of(c))
      NQ_FAIL(c, -1, "nq_avg_attach: a product of two different fields with flow fields (NQ_FLOW_*) at nx = %d: a thread of that row plan holds one value (DESIGN.md section 7)", c->N);
    for (int o = 0; o < p; ++o)
      if (pa[o] == pa[p] && pb[o] == pb[p]) NQ_FAIL(c, -1, "nq_avg_attach: the pair (%d, %d) is listed twice", pairs[2 * p], pairs[2 * p + 1]);
  }
  HIPCHK(c, hipSetDevice(c->device));
  c->av = new NqAvg();
  NqAvg* A = c->av;
  A->nf = nfields;
  A->np = nproducts;
  A->rg.init(1, every);
  A->args.mask = mask;
  A->args.np = nproducts;
  A->flow = flow;
  A->sel = sel;
  const size_t n = (size_t)c->N * c->N;
  int rc = 0;
  for (int i = 0; i < nfields && !rc; ++i) {
    const int s = slot[i];
    A->field[i] = fields[i];
    if (s == AVG_PHI) {
      rc = att_alloc(c, A, &A->args.sum_phi, n, "nq_avg_attach");
      A->plane[i] = A->args.sum_phi;
    } else {
      rc = att_alloc(c, A, &A->args.sum[s], n, "nq_avg_attach");
      A->plane[i] = A->args.sum[s];
    }
  }
  for (int p = 0; p < nproducts && !rc; ++p) {
    A->args.pa[p] = pa[p];
    A->args.pb[p] = pb[p];
    rc = att_alloc(c, A, &A->args.prod[p], n, "nq_avg_attach");
    A->plane[nfields + p] = A->args.prod[p];
  }
  if (rc) return att_fail(c, c->av, rc);
  return 0;
}
int nq_avg_detach(nq_ctx* c) {
  NQ_SINGLE_RANK(c, "nq_avg_detach");
  if (!c->av) NQ_FAIL(c, -4, "nq_avg_detach: no averages attached");
  att_release(c, c->av);
  return 0;
}
int nq_avg_sample(nq_ctx* c) {
  NQ_SINGLE_RANK(c, "nq_avg_sample");
  if (!c->av) NQ_FAIL(c, -4, "nq_avg_sample: no averages attached");
  HIPCHK(c, hipSetDevice(c->device));
  return av_sample(c, "nq_avg_sample");
}
int nq_avg_reset(nq_ctx* c) {
  NQ_SINGLE_RANK(c, "nq_avg_reset");
  NqAvg* A = c->av;
  if (!A) NQ_FAIL(c, -4, "nq_avg_reset: no averages attached");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = (size_t)c->N * c->N;
  for (int i = 0; i < A->nf + A->np; ++i)
    HIPCHK(c, hipMemsetAsync(A->plane[i], 0, (A->plane[i] == (void*)A->args.sum_phi ? sizeof(cd) : sizeof(double)) * n, c->stream));
  A->rg.count = 0;
  return 0;
}
int nq_avg_info(nq_ctx* c, long long* info3) {
  NQ_SINGLE_RANK(c, "nq_avg_info");
  NqAvg* A = c->av;
  if (!A) NQ_FAIL(c, -4, "nq_avg_info: no averages attached");
  if (!info3) return -1;
  info3[0] = A->rg.count;
  info3[1] = A->rg.steps;
  info3[2] = A->nf + A->np;
  return 0;
}
int nq_avg_read(nq_ctx* c, int plane_index, double* out) {
  NQ_SINGLE_RANK(c, "nq_avg_read");
  NqAvg* A = c->av;
  if (!A) NQ_FAIL(c, -4, "nq_avg_read: no averages attached");
  if (!out) return -1;
  if (plane_index < 0 || plane_index >= A->nf + A->np) NQ_FAIL(c, -1, "nq_avg_read: plane %d of %d", plane_index, A->nf + A->np);
  HIPCHK(c, hipSetDevice(c->device));
  const void* src = A->plane[plane_index];
  const size_t bytes = (src == (const void*)A->args.sum_phi ? sizeof(cd) : sizeof(double)) * (size_t)c->N * c->N;
  HIPCHK(c, hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToHost, c->stream));
  return nq_sync(c);
}

// ---- time-mean spectra, transfer and flux -----------------------------------------------------------------
int nq_tspec_attach(nq_ctx* c, int what_mask, int every) {
  NQ_SINGLE_RANK(c, "nq_tspec_attach");
  if (c->ts) NQ_FAIL(c, -4, "nq_tspec_attach: time-mean spectra are attached already (nq_tspec_detach first)");
  if (what_mask < 1 || what_mask > (NQ_TSPEC_SPECTRA | NQ_TSPEC_TRANSFER))
    NQ_FAIL(c, -1, "nq_tspec_attach: what_mask = %d (NQ_TSPEC_SPECTRA | NQ_TSPEC_TRANSFER, at least one)", what_mask);
  if (every < 0) NQ_FAIL(c, -1, "nq_tspec_attach: every = %d (>= 0)", every);
  const int nb = nq_shell_count(c->N);
  if (nb < 1 || nb > TSPEC_MAX_NB) NQ_FAIL(c, -1, "nq_tspec_attach: %d shells (1 to %d: the LDS row of the running sum)", nb, TSPEC_MAX_NB);
  HIPCHK(c, hipSetDevice(c->device));
  // what the selected bodies allocate on their first call: here, so that no sample allocates; context-owned, as ever
  if ((what_mask & NQ_TSPEC_SPECTRA) && !c->spec_out) ALLOC(c, c->spec_out, (size_t)32 * nb);
  if ((what_mask & NQ_TSPEC_SPECTRA) && c->kernel_family && !c->spec_r) ALLOC(c, c->spec_r, (size_t)2 * c->N * c->Wf);
  if ((what_mask & NQ_TSPEC_TRANSFER) && !c->tr_out) ALLOC(c, c->tr_out, (size_t)NQ_TRANSFER_ROWS * nb);
  c->ts = new NqTspec();
  NqTspec* T = c->ts;
  T->mask = what_mask;
  T->nb = nb;
  T->rg.init(1, every);
  const int rc = att_alloc(c, T, &T->tab, T->doubles(), "nq_tspec_attach");
  if (rc) return att_fail(c, c->ts, rc);
  const size_t ns = (size_t)TSPEC_SPEC_ROWS * nb, nt = (size_t)TSPEC_TR_ROWS * nb;
  T->args.nb = nb;
  T->args.s1 = T->tab;
  T->args.s2 = T->tab + ns;
  T->args.t1 = T->tab + 2 * ns;
  T->args.t2 = T->tab + 2 * ns + nt;
  T->args.p1 = T->tab + 2 * ns + 2 * nt;
  T->args.p2 = T->tab + 2 * ns + 3 * nt;
  return 0;
}
int nq_tspec_detach(nq_ctx* c) {
  NQ_SINGLE_RANK(c, "nq_tspec_detach");
  if (!c->ts) NQ_FAIL(c, -4, "nq_tspec_detach: no time-mean spectra attached");
  att_release(c, c->ts);
  return 0;
}
int nq_tspec_sample(nq_ctx* c) {
  NQ_SINGLE_RANK(c, "nq_tspec_sample");
  if (!c->ts) NQ_FAIL(c, -4, "nq_tspec_sample: no time-mean spectra attached");
  HIPCHK(c, hipSetDevice(c->device));
  return ts_sample(c, "nq_tspec_sample");
}
int nq_tspec_reset(nq_ctx* c) {
  NQ_SINGLE_RANK(c, "nq_tspec_reset");
  NqTspec* T = c->ts;
  if (!T) NQ_FAIL(c, -4, "nq_tspec_reset: no time-mean spectra attached");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemsetAsync(T->tab, 0, sizeof(double) * T->doubles(), c->stream));
  T->rg.count = 0;
  return 0;
}
int nq_tspec_info(nq_ctx* c, long long* info3) {
  NQ_SINGLE_RANK(c, "nq_tspec_info");
  NqTspec* T = c->ts;
  if (!T) NQ_FAIL(c, -4, "nq_tspec_info: no time-mean spectra attached");
  if (!info3) return -1;
  info3[0] = T->rg.count;
  info3[1] = T->rg.steps;
  info3[2] = T->mask;
  return 0;
}
int nq_tspec_read(nq_ctx* c, int which, double* out) {
  NQ_SINGLE_RANK(c, "nq_tspec_read");
  NqTspec* T = c->ts;
  if (!T) NQ_FAIL(c, -4, "nq_tspec_read: no time-mean spectra attached");
  if (!out) return -1;
  if (which < 0 || which >= TSPEC_TABLES) NQ_FAIL(c, -1, "nq_tspec_read: table %d (NQ_TSPEC_S1 .. NQ_TSPEC_P2 = 0 .. %d)", which, TSPEC_TABLES - 1);
  const double* src[TSPEC_TABLES] = {T->args.s1, T->args.s2, T->args.t1, T->args.t2, T->args.p1, T->args.p2};
  const size_t n = (size_t)(which < 2 ? TSPEC_SPEC_ROWS : TSPEC_TR_ROWS) * T->nb;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(out, src[which], sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
  return nq_sync(c);
}

// One sample on engine planes (the any-size path steps from Python and calls this after its own step): the rule and the kernel of
// QGModel's fused contexts.  src[i] (complex engine planes of `elems` values) read as what[i] (0: Re, 1: |a|^2, 2: the complex
// value itself, at most once and in no product) is added to sums[i] (elems doubles; what 2: elems complex); pairs: 2 x nproducts
// indices into src (what 0 or 1), psums[p] += their product.
int nq_any_moments(nq_any* e, long long elems, int nfields, const void* const* src, const int* what, void* const* sums, int nproducts,
                   const int* pairs, void* const* psums) {
  if (!e || !src || !what || !sums || elems <= 0 || (nproducts > 0 && (!pairs || !psums))) return -1;
  if (nfields < 1 || nfields > AVG_SLOTS + 1) ANYFAIL(e, -1, "nq_any_moments: %d fields (1 to %d)", nfields, AVG_SLOTS + 1);
  if (nproducts < 0 || nproducts > AVG_MAX_PRODUCTS) ANYFAIL(e, -1, "nq_any_moments: %d products (0 to %d)", nproducts, AVG_MAX_PRODUCTS);
  AvgSrc s = {};
  AvgArgs a = {};
  int slot_of[AVG_SLOTS + 1], nreal = 0;
  for (int i = 0; i < nfields; ++i) {
    if (!src[i] || !sums[i]) return -1;
    if (what[i] == 2) {
      if (a.mask & (1 << AVG_PHI)) ANYFAIL(e, -1, "nq_any_moments: more than one complex field");
      a.mask |= 1 << AVG_PHI;
      s.phi = reinterpret_cast<const cd*>(src[i]);
      a.sum_phi = reinterpret_cast<cd*>(sums[i]);
      slot_of[i] = -1;
    } else if (what[i] == 0 || what[i] == 1) {
      if (nreal == AVG_SLOTS) ANYFAIL(e, -1, "nq_any_moments: more than %d real fields", AVG_SLOTS);
      a.mask |= 1 << nreal;
      s.p[nreal] = reinterpret_cast<const double*>(src[i]);
      s.stride[nreal] = 2;
      s.what[nreal] = what[i];
      a.sum[nreal] = reinterpret_cast<double*>(sums[i]);
      slot_of[i] = nreal++;
    } else {
      ANYFAIL(e, -1, "nq_any_moments: what = %d (0: Re, 1: |a|^2, 2: complex)", what[i]);
    }
  }
  a.np = nproducts;
  for (int p = 0; p < nproducts; ++p) {
    const int ia = pairs[2 * p], ib = pairs[2 * p + 1];
    if (ia < 0 || ia >= nfields || ib < 0 || ib >= nfields || slot_of[ia] < 0 || slot_of[ib] < 0 || !psums[p])
      ANYFAIL(e, -1, "nq_any_moments: product %d does not name two real fields of the list", p);
    a.pa[p] = slot_of[ia];
    a.pb[p] = slot_of[ib];
    a.prod[p] = reinterpret_cast<double*>(psums[p]);
  }
  ANYCHK(e, hipSetDevice(e->device));
  const size_t n = (size_t)elems;
  hipLaunchKernelGGL(k_moments_plane, dim3(hist_plane_grid(n)), dim3(256), 0, e->stream, s, n, a);
  ANYCHK(e, hipGetLastError());
  return 0;
}

// The same on engine planes (the any-size path steps from Python and calls this after its own step): one record of nf planes
// into slot `slot` of their rings, ONE launch.  planes[f]: (rows, cols[f]) with cols[f] >= K + 1; full[f] != 0: the block takes
// columns 0..K and cols - K..cols - 1 (a full plane, cols[f] == rows), else columns 0..K (a half spectrum, or the first columns
// of the reference's full-plane q-hat).  rings[f]: [length][2K + 1][2K + 1 or K + 1] complex.
int nq_any_freq_record(nq_any* e, int nf, void* const* rings, const void* const* planes, const int* cols, const int* full, int rows, int K,
                       int length, int slot) {
  if (!e || !rings || !planes || !cols || !full) return -1;
  if (nf < 1 || nf > FQ_NFIELDS) ANYFAIL(e, -1, "nq_any_freq_record: %d fields", nf);
  if (rows < 4 || (rows & 1) || K < 1 || K >= rows / 2) ANYFAIL(e, -1, "nq_any_freq_record: kmax = %d on %d rows (1 <= kmax < rows/2)", K, rows);
  if (length < 2 || slot < 0 || slot >= length) ANYFAIL(e, -1, "nq_any_freq_record: slot %d of %d", slot, length);
  ANYCHK(e, hipSetDevice(e->device));
  FqRecord a = {};
  const int R = 2 * K + 1;
  int maxc = 0;
  for (int f = 0; f < nf; ++f) {
    if (!rings[f] || !planes[f]) return -1;
    if (full[f] ? cols[f] != rows : cols[f] < K + 1) ANYFAIL(e, -1, "nq_any_freq_record: %d columns for a %s block of kmax %d", cols[f], full[f] ? "full" : "half", K);
    a.src[f] = reinterpret_cast<const cd*>(planes[f]);
    a.pitch[f] = cols[f];
    a.ncols[f] = full[f] ? R : K + 1;
    a.proj[f] = 0;
    a.dst[f] = reinterpret_cast<cd*>(rings[f]) + (size_t)slot * R * a.ncols[f];
    if (a.ncols[f] > maxc) maxc = a.ncols[f];
  }
  hipLaunchKernelGGL(k_fq_record, dim3((maxc + 63) / 64, (R + 3) / 4, nf), dim3(64, 4), 0, e->stream, a, rows, K);
  ANYCHK(e, hipGetLastError());
  return 0;
}
// The spectrum pass of nq_freq_spectrum on an engine-owned ring: T records, the oldest in slot `first`; full / kappa as the field
// (phi: 1, 0; q: 0, 0; psi: 0, 1); out: (T, nb), row p = FFT bin p.  The work plane lives for the call.
int nq_any_freq_spectrum(nq_any* e, const void* ring, int rows, int K, int full, int kappa, int length, int first, int T, const double* window,
                         int demean, double dk, int nb, double* out) {
  if (!e || !ring || !window || !out) return -1;
  if (rows < 4 || (rows & 1) || K < 1 || K >= rows / 2) ANYFAIL(e, -1, "nq_any_freq_spectrum: kmax = %d on %d rows (1 <= kmax < rows/2)", K, rows);
  if (length < 2 || T < 2 || T > length || first < 0 || first >= length) ANYFAIL(e, -1, "nq_any_freq_spectrum: %d records from slot %d of %d", T, first, length);
  if (nb != nq_shell_of(K, K) + 1) ANYFAIL(e, -1, "nq_any_freq_spectrum: nb = %d, the block has %d shells", nb, nq_shell_of(K, K) + 1);
  for (int n = 0; n < T; ++n)
    if (!std::isfinite(window[n])) ANYFAIL(e, -1, "nq_any_freq_spectrum: the window is not finite at record %d", n);
  if (!std::isfinite(dk) || !(dk > 0.0)) ANYFAIL(e, -1, "nq_any_freq_spectrum: dk = %g", dk);
  ANYCHK(e, hipSetDevice(e->device));
  const int ncols = full ? 2 * K + 1 : K + 1;
  const size_t wel = (size_t)T * (2 * (size_t)K + 1) * ncols;
  cd* work = nullptr;
  double *dwin = nullptr, *dtab = nullptr;
  AnyScratch tmp;
  if (tmp.get(&work, wel) != hipSuccess) {
    (void)hipGetLastError();
    ANYFAIL(e, -5, "nq_any_freq_spectrum: cannot allocate %zu bytes of device memory", wel * sizeof(cd));
  }
  ANYCHK(e, tmp.get(&dwin, (size_t)T));
  ANYCHK(e, tmp.get(&dtab, (size_t)T * nb));
  return fq_spectrum_run(e, reinterpret_cast<const cd*>(ring), rows, K, ncols, full ? 1 : 0, kappa ? 1 : 0, length, first, T, window, demean, dk, nb, work,
                         dwin, dtab, out);
}

}  // extern "C"

// ==================================================================================================================
// Lagrangian spectra and dispersion of the particle records (kernels: csrc/nq_lagr.hpp)
// ==================================================================================================================
#include "nq_lagr.hpp"

enum { LG_UV = 4, LG_UVW = NQ_LAGR_UVW, LG_UVT = NQ_LAGR_UVT };   // the composites u + i v, uw + i vw and (u + uw) + i (v + vw)

// the group-sorted index list: G runs of `order`, run g is offsets[g] .. offsets[g + 1] - 1; null: fine, else what is wrong
static const char* lg_check_groups(int n, int G, const int* order, const int* offsets) {
  if (G < 1 || G > 256) return "the number of groups must be 1 to 256";
  if (!order || !offsets) return "no index list";
  if (offsets[0] != 0 || offsets[G] != n) return "the offsets must run from 0 to n";
  for (int g = 0; g < G; ++g)
    if (offsets[g + 1] < offsets[g]) return "the offsets decrease";
  for (int i = 0; i < n; ++i)
    if (order[i] < 0 || order[i] >= n) return "an index of the list is outside [0, n)";
  return nullptr;
}
static const char* lg_check_pairs(int n, int npairs, const int* pi, const int* pj) {
  if (npairs < 0 || (npairs > 0 && (!pi || !pj))) return "no pair lists";
  for (int q = 0; q < npairs; ++q)
    if (pi[q] < 0 || pi[q] >= n || pj[q] < 0 || pj[q] >= n || pi[q] == pj[q]) return "a pair index is outside [0, n), or i = j";
  return nullptr;
}
// columns of the work plane per chunk: a rule of (n, F) alone -- the plane stays within 256 MiB -- or the caller's `chunk`, cut to it
static int lg_chunk(int n, int F, int chunk) {
  long long cmax = ((256LL << 20) / ((long long)sizeof(cd) * F)) / 256 * 256;
  if (cmax < 256) cmax = 256;
  long long C = chunk > 0 ? chunk : cmax;
  if (C > cmax) C = cmax;
  if (C > n) C = n;
  return (int)C;
}
struct LgDev {
  cd* work;
  double* win;
  LgSeries* ser;
  int *order, *offs, *pairs;
  double* tab;
};
// The spectrum pass on the engine's stream, chunk by chunk: window -> transform along the record axis -> power per group, the
// chunks' partials added in chunk order.  out: (F, G) host, row p = FFT bin p, the sums over each group times 1 / (2 F sum w^2).
static int lg_spectrum_run(nq_any* e, const LgDev& d, const LgSeries* ser, int n, int T, int F, const double* window, int demean, int G,
                           const int* order, const int* offsets, int C, double* out) {
  double sw2 = 0.0;
  for (int k = 0; k < T; ++k) sw2 += window[k] * window[k];
  if (!(sw2 > 0.0)) ANYFAIL(e, -1, "Lagrangian spectrum: the window is zero everywhere");
  const double scale = 0.5 / ((double)F * sw2);
  ANYCHK(e, hipMemcpyAsync(d.win, window, sizeof(double) * T, hipMemcpyHostToDevice, e->stream));
  ANYCHK(e, hipMemcpyAsync(d.ser, ser, sizeof(LgSeries) * T, hipMemcpyHostToDevice, e->stream));
  ANYCHK(e, hipMemcpyAsync(d.order, order, sizeof(int) * n, hipMemcpyHostToDevice, e->stream));
  ANYCHK(e, hipMemcpyAsync(d.offs, offsets, sizeof(int) * (G + 1), hipMemcpyHostToDevice, e->stream));
  for (int c0 = 0; c0 < n; c0 += C) {
    const int Cw = n - c0 < C ? n - c0 : C;
    hipLaunchKernelGGL(k_lg_window, dim3((Cw + 255) / 256), dim3(256), 0, e->stream, (const LgSeries*)d.ser, (const int*)d.order, d.work,
                       (const double*)d.win, c0, Cw, T, F, demean ? 1 : 0);
    ANYCHK(e, hipGetLastError());
    const int rc = nq_any_fft(e, d.work, d.work, F, Cw, 0, 0);
    if (rc) return rc;
    hipLaunchKernelGGL(k_lg_power, dim3(G, F), dim3(256), 0, e->stream, (const cd*)d.work, (const int*)d.offs, c0, Cw, F, G, scale, c0 == 0 ? 1 : 0, d.tab);
    ANYCHK(e, hipGetLastError());
  }
  ANYCHK(e, hipMemcpyAsync(out, d.tab, sizeof(double) * (size_t)F * G, hipMemcpyDeviceToHost, e->stream));
  return nq_any_sync(e);
}
// The dispersion pass on `st`: out (T, G, 6) host sums, outp (T, 5) host sums of the pairs (npairs > 0); returns after the copies
static hipError_t lg_dispersion_run(hipStream_t st, const LgDev& d, const LgSeries* pos, int n, int T, int G, const int* order, const int* offsets,
                                    int npairs, const int* pi, const int* pj, double* out, double* outp) {
  hipError_t r = hipMemcpyAsync(d.ser, pos, sizeof(LgSeries) * T, hipMemcpyHostToDevice, st);
  if (r == hipSuccess) r = hipMemcpyAsync(d.order, order, sizeof(int) * n, hipMemcpyHostToDevice, st);
  if (r == hipSuccess) r = hipMemcpyAsync(d.offs, offsets, sizeof(int) * (G + 1), hipMemcpyHostToDevice, st);
  if (r != hipSuccess) return r;
  const size_t single = (size_t)T * G * LG_SINGLE_SUMS;
  hipLaunchKernelGGL(k_lg_disp, dim3(G, T), dim3(256), 0, st, (const LgSeries*)d.ser, (const int*)d.order, (const int*)d.offs, G, d.tab);
  if ((r = hipGetLastError()) != hipSuccess) return r;
  if (npairs > 0) {
    r = hipMemcpyAsync(d.pairs, pi, sizeof(int) * npairs, hipMemcpyHostToDevice, st);
    if (r == hipSuccess) r = hipMemcpyAsync(d.pairs + npairs, pj, sizeof(int) * npairs, hipMemcpyHostToDevice, st);
    if (r != hipSuccess) return r;
    hipLaunchKernelGGL(k_lg_pairs, dim3(T), dim3(256), 0, st, (const LgSeries*)d.ser, (const int*)d.pairs, (const int*)(d.pairs + npairs), npairs, d.tab + single);
    if ((r = hipGetLastError()) != hipSuccess) return r;
    r = hipMemcpyAsync(outp, d.tab + single, sizeof(double) * (size_t)T * LG_PAIR_SUMS, hipMemcpyDeviceToHost, st);
    if (r != hipSuccess) return r;
  }
  r = hipMemcpyAsync(out, d.tab, sizeof(double) * single, hipMemcpyDeviceToHost, st);
  if (r != hipSuccess) return r;
  return hipStreamSynchronize(st);
}

// The stretching pass on `st` (section 5u): ser[r] holds the four f-columns of record r; out (T, G, 4) host sums
static hipError_t lg_stretching_run(hipStream_t st, const LgDev& d, const LgSeries* ser, int n, int T, int G, const int* order, const int* offsets,
                                    double* out) {
  hipError_t r = hipMemcpyAsync(d.ser, ser, sizeof(LgSeries) * T, hipMemcpyHostToDevice, st);
  if (r == hipSuccess) r = hipMemcpyAsync(d.order, order, sizeof(int) * n, hipMemcpyHostToDevice, st);
  if (r == hipSuccess) r = hipMemcpyAsync(d.offs, offsets, sizeof(int) * (G + 1), hipMemcpyHostToDevice, st);
  if (r != hipSuccess) return r;
  hipLaunchKernelGGL(k_lg_stretch, dim3(G, T), dim3(256), 0, st, (const LgSeries*)d.ser, (const int*)d.order, (const int*)d.offs, G, d.tab);
  if ((r = hipGetLastError()) != hipSuccess) return r;
  r = hipMemcpyAsync(out, d.tab, sizeof(double) * (size_t)T * G * LG_STRETCH_SUMS, hipMemcpyDeviceToHost, st);
  if (r != hipSuccess) return r;
  return hipStreamSynchronize(st);
}

// ---- fused contexts: the records are the particles' ring; work memory hangs on NqParticles ----------------------------------
static int lg_column(const NqParticles* P, int name) {
  int col = 2;
  for (int nm : P->names) {
    if (nm == name) return col;
    col += nm == PT_PHI ? 2 : 1;
  }
  return -1;
}
// every buffer holds at least need[b] bytes after this; when one is short they are all given back and allocated again under one
// mark, so a failure leaves the particles as they were before their first call
static int lg_reserve(nq_ctx* c, NqParticles* P, const size_t* need, const char* what) {
  bool enough = true;
  for (int b = 0; b < NqParticles::LG_NBUF; ++b) enough = enough && P->lg_have[b] >= need[b];
  if (enough) return 0;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (P->eng) {
    const int rc = nq_any_sync(P->eng);
    if (rc) NQ_FAIL(c, rc, "%s: %s", what, nq_any_last_error(P->eng));
  }
  size_t want[NqParticles::LG_NBUF];
  for (int b = 0; b < NqParticles::LG_NBUF; ++b) {
    want[b] = need[b] > P->lg_have[b] ? need[b] : P->lg_have[b];
    if (P->lg[b]) c->bytes -= P->release(P->lg[b], (long long)P->lg_have[b]);
    P->lg[b] = nullptr;
    P->lg_have[b] = 0;
  }
  const DevMark before = P->mark();
  int rc = 0;
  for (int b = 0; b < NqParticles::LG_NBUF && !rc; ++b) {
    if (!want[b]) continue;
    char* p = nullptr;
    rc = att_alloc(c, P, &p, want[b], what);
    if (!rc) {
      P->lg[b] = p;
      P->lg_have[b] = want[b];
    }
  }
  if (rc) {
    c->bytes -= P->rollback(before);
    for (int b = 0; b < NqParticles::LG_NBUF; ++b) {
      P->lg[b] = nullptr;
      P->lg_have[b] = 0;
    }
  }
  return rc;
}
static LgDev lg_dev(const NqParticles* P) {
  LgDev d;
  d.work = static_cast<cd*>(P->lg[NqParticles::LG_WORK]);
  d.win = static_cast<double*>(P->lg[NqParticles::LG_WIN]);
  d.ser = static_cast<LgSeries*>(P->lg[NqParticles::LG_SER]);
  d.order = static_cast<int*>(P->lg[NqParticles::LG_ORDER]);
  d.offs = static_cast<int*>(P->lg[NqParticles::LG_OFFS]);
  d.pairs = static_cast<int*>(P->lg[NqParticles::LG_PAIRS]);
  d.tab = static_cast<double*>(P->lg[NqParticles::LG_TAB]);
  return d;
}

extern "C" {

int nq_lagr_spectrum(nq_ctx* c, int kind, int T, int F, const double* window, int demean, int G, const int* order, const int* offsets, int chunk,
                     double* out) {
  NQ_SINGLE_RANK(c, "nq_lagr_spectrum");
  NqParticles* P = c->pt;
  if (!P) NQ_FAIL(c, -4, "nq_lagr_spectrum: no particles attached");
  if (!window || !out) return -1;
  if (P->rg.every <= 0) NQ_FAIL(c, -1, "nq_lagr_spectrum: the particles were attached with record_every = 0");
  const int held = (int)P->rg.held();
  if (held < 2) NQ_FAIL(c, -1, "nq_lagr_spectrum: %d record held (at least 2)", held);
  if (T != held) NQ_FAIL(c, -1, "nq_lagr_spectrum: a window of %d values, %d records are held", T, held);
  if (F < T || (F > 8192 && F != 16384)) NQ_FAIL(c, -1, "nq_lagr_spectrum: nfft = %d (from T = %d to 8192, or 16384)", F, T);
  if (!(pt_name_ok(kind) || kind == LG_UV || kind == LG_UVW || kind == LG_UVT) || kind == PT_ZETA || pt_name_of_rays(kind) || pt_name_of_tangent(kind))
    NQ_FAIL(c, -1, "nq_lagr_spectrum: name %d (0 u, 1 v, 2 q, 3 phi, 4 u + i v, 5 uw, 6 vw, 7 uw + i vw, 8 (u + uw) + i (v + vw))", kind);
  // the columns of the series: re + i im, plus re2 + i im2 for the sum of two velocities
  int cre, cim = -1, cre2 = -1, cim2 = -1;
  bool have;
  if (kind == LG_UV || kind == LG_UVT) {
    cre = lg_column(P, PT_U);
    cim = lg_column(P, PT_V);
    have = cre >= 0 && cim >= 0;
    if (kind == LG_UVT) {
      cre2 = lg_column(P, PT_UW);
      cim2 = lg_column(P, PT_VW);
      have = have && cre2 >= 0 && cim2 >= 0;
    }
  } else if (kind == LG_UVW) {
    cre = lg_column(P, PT_UW);
    cim = lg_column(P, PT_VW);
    have = cre >= 0 && cim >= 0;
  } else {
    cre = lg_column(P, kind);
    have = cre >= 0;
    if (kind == PT_PHI) cim = cre + 1;
  }
  if (!have) NQ_FAIL(c, -1, "nq_lagr_spectrum: name %d is not recorded", kind);
  for (int k = 0; k < T; ++k)
    if (!std::isfinite(window[k])) NQ_FAIL(c, -1, "nq_lagr_spectrum: the window is not finite at record %d", k);
  const int n = P->n;
  if (const char* bad = lg_check_groups(n, G, order, offsets)) NQ_FAIL(c, -1, "nq_lagr_spectrum: %s", bad);
  HIPCHK(c, hipSetDevice(c->device));
  if (!P->eng) {
    const int rc = nq_any_create(c->device, &P->eng);
    if (rc) {
      P->eng = nullptr;
      NQ_FAIL(c, rc, "nq_lagr_spectrum: %s", g_last_error.c_str());
    }
  }
  const int C = lg_chunk(n, F, chunk);
  size_t need[NqParticles::LG_NBUF] = {};
  need[NqParticles::LG_WORK] = sizeof(cd) * (size_t)F * C;
  need[NqParticles::LG_WIN] = sizeof(double) * T;
  need[NqParticles::LG_SER] = sizeof(LgSeries) * T;
  need[NqParticles::LG_ORDER] = sizeof(int) * (size_t)n;
  need[NqParticles::LG_OFFS] = sizeof(int) * (G + 1);
  need[NqParticles::LG_TAB] = sizeof(double) * (size_t)F * G;
  int rc = lg_reserve(c, P, need, "nq_lagr_spectrum");
  if (rc) return rc;
  rc = nq_sync(c);                                  // every record queued on the context's stream is in the ring
  if (rc) return rc;
  const size_t rec = (size_t)(2 + P->ncol) * n;
  std::vector<LgSeries> ser((size_t)T);
  for (int r = 0; r < T; ++r) {
    const double* base = P->ring + (size_t)P->rg.oldest(r) * rec;
    ser[r].re = base + (size_t)cre * n;
    ser[r].im = cim >= 0 ? base + (size_t)cim * n : nullptr;
    ser[r].re2 = cre2 >= 0 ? base + (size_t)cre2 * n : nullptr;
    ser[r].im2 = cim2 >= 0 ? base + (size_t)cim2 * n : nullptr;
    ser[r].stride = 1;
  }
  const long long eng_before = nq_any_device_bytes(P->eng);
  rc = lg_spectrum_run(P->eng, lg_dev(P), ser.data(), n, T, F, window, demean, G, order, offsets, C, out);
  const long long grown = nq_any_device_bytes(P->eng) - eng_before;       // the engine's work rows count as the particles'
  P->bytes += grown;
  c->bytes += grown;
  if (rc) NQ_FAIL(c, rc, "nq_lagr_spectrum: %s", nq_any_last_error(P->eng));
  return 0;
}

int nq_lagr_dispersion(nq_ctx* c, int T, int G, const int* order, const int* offsets, int npairs, const int* pi, const int* pj, double* out,
                       double* out_pairs) {
  NQ_SINGLE_RANK(c, "nq_lagr_dispersion");
  NqParticles* P = c->pt;
  if (!P) NQ_FAIL(c, -4, "nq_lagr_dispersion: no particles attached");
  if (!out || (npairs > 0 && !out_pairs)) return -1;
  if (P->rg.every <= 0) NQ_FAIL(c, -1, "nq_lagr_dispersion: the particles were attached with record_every = 0");
  const int held = (int)P->rg.held();
  if (held < 2) NQ_FAIL(c, -1, "nq_lagr_dispersion: %d record held (at least 2)", held);
  if (T != held) NQ_FAIL(c, -1, "nq_lagr_dispersion: tables of %d records, %d are held", T, held);
  const int n = P->n;
  if (const char* bad = lg_check_groups(n, G, order, offsets)) NQ_FAIL(c, -1, "nq_lagr_dispersion: %s", bad);
  if (const char* bad = lg_check_pairs(n, npairs, pi, pj)) NQ_FAIL(c, -1, "nq_lagr_dispersion: %s", bad);
  HIPCHK(c, hipSetDevice(c->device));
  size_t need[NqParticles::LG_NBUF] = {};
  need[NqParticles::LG_SER] = sizeof(LgSeries) * T;
  need[NqParticles::LG_ORDER] = sizeof(int) * (size_t)n;
  need[NqParticles::LG_OFFS] = sizeof(int) * (G + 1);
  need[NqParticles::LG_TAB] = sizeof(double) * (size_t)T * ((size_t)G * LG_SINGLE_SUMS + LG_PAIR_SUMS);
  need[NqParticles::LG_PAIRS] = sizeof(int) * 2 * (size_t)npairs;
  int rc = lg_reserve(c, P, need, "nq_lagr_dispersion");
  if (rc) return rc;
  rc = nq_sync(c);
  if (rc) return rc;
  const size_t rec = (size_t)(2 + P->ncol) * n;
  std::vector<LgSeries> pos((size_t)T);
  for (int r = 0; r < T; ++r) {
    const double* base = P->ring + (size_t)P->rg.oldest(r) * rec;
    pos[r].re = base;
    pos[r].im = base + n;
    pos[r].stride = 1;
  }
  HIPCHK(c, lg_dispersion_run(c->stream, lg_dev(P), pos.data(), n, T, G, order, offsets, npairs, pi, pj, out, out_pairs));
  return 0;
}

int nq_lagr_stretching(nq_ctx* c, int T, int G, const int* order, const int* offsets, double* out) {
  NQ_SINGLE_RANK(c, "nq_lagr_stretching");
  NqParticles* P = c->pt;
  if (!P) NQ_FAIL(c, -4, "nq_lagr_stretching: no particles attached");
  if (!out) return -1;
  if (P->rg.every <= 0) NQ_FAIL(c, -1, "nq_lagr_stretching: the particles were attached with record_every = 0");
  if (!P->tan) NQ_FAIL(c, -1, "nq_lagr_stretching: stretch mode is off (nq_particles_tangent)");
  int col[4];
  for (int k = 0; k < 4; ++k) {
    col[k] = lg_column(P, PT_F11 + k);
    if (col[k] < 0) NQ_FAIL(c, -1, "nq_lagr_stretching: all of f11, f12, f21, f22 must be recorded (name %d is not)", PT_F11 + k);
  }
  const int held = (int)P->rg.held();
  if (held < 2) NQ_FAIL(c, -1, "nq_lagr_stretching: %d record held (at least 2)", held);
  if (T != held) NQ_FAIL(c, -1, "nq_lagr_stretching: tables of %d records, %d are held", T, held);
  if (P->rg.count - held < P->tan_count0)
    NQ_FAIL(c, -1, "nq_lagr_stretching: the ring still holds %lld records written before the reset at particle step %lld", P->tan_count0 - (P->rg.count - held),
            P->tan_step0);
  const int n = P->n;
  if (const char* bad = lg_check_groups(n, G, order, offsets)) NQ_FAIL(c, -1, "nq_lagr_stretching: %s", bad);
  HIPCHK(c, hipSetDevice(c->device));
  size_t need[NqParticles::LG_NBUF] = {};
  need[NqParticles::LG_SER] = sizeof(LgSeries) * T;
  need[NqParticles::LG_ORDER] = sizeof(int) * (size_t)n;
  need[NqParticles::LG_OFFS] = sizeof(int) * (G + 1);
  need[NqParticles::LG_TAB] = sizeof(double) * (size_t)T * G * LG_STRETCH_SUMS;
  int rc = lg_reserve(c, P, need, "nq_lagr_stretching");
  if (rc) return rc;
  rc = nq_sync(c);
  if (rc) return rc;
  const size_t rec = (size_t)(2 + P->ncol) * n;
  std::vector<LgSeries> ser((size_t)T);
  for (int r = 0; r < T; ++r) {
    const double* base = P->ring + (size_t)P->rg.oldest(r) * rec;
    ser[r].re = base + (size_t)col[0] * n;
    ser[r].im = base + (size_t)col[1] * n;
    ser[r].re2 = base + (size_t)col[2] * n;
    ser[r].im2 = base + (size_t)col[3] * n;
    ser[r].stride = 1;
  }
  HIPCHK(c, lg_stretching_run(c->stream, lg_dev(P), ser.data(), n, T, G, order, offsets, out));
  return 0;
}

// The same passes on engine planes (the any-size path keeps one plane per record and name).  re[r], im[r]: the device address of
// particle 0's real and imaginary part in record r, oldest first (im NULL: a real series; an entry of a complex plane: the plane's
// address and that plus 8 bytes); stride: doubles between particles (2 on a complex plane).  The work memory lives for the call.
int nq_any_lagr_spectrum(nq_any* e, int n, int T, const void* const* re, const void* const* im, int stride, int F, const double* window, int demean,
                         int G, const int* order, const int* offsets, int chunk, double* out) {
  if (!e || !re || !window || !out) return -1;
  if (n < 1 || T < 2 || stride < 1) ANYFAIL(e, -1, "nq_any_lagr_spectrum: n = %d, %d records (at least 2), stride %d", n, T, stride);
  if (F < T || (F > 8192 && F != 16384)) ANYFAIL(e, -1, "nq_any_lagr_spectrum: nfft = %d (from T = %d to 8192, or 16384)", F, T);
  for (int k = 0; k < T; ++k) {
    if (!re[k] || (im && !im[k])) ANYFAIL(e, -1, "nq_any_lagr_spectrum: record %d has no plane", k);
    if (!std::isfinite(window[k])) ANYFAIL(e, -1, "nq_any_lagr_spectrum: the window is not finite at record %d", k);
  }
  if (const char* bad = lg_check_groups(n, G, order, offsets)) ANYFAIL(e, -1, "nq_any_lagr_spectrum: %s", bad);
  ANYCHK(e, hipSetDevice(e->device));
  const int C = lg_chunk(n, F, chunk);
  LgDev d = {};
  AnyScratch tmp;
  if (tmp.get(&d.work, (size_t)F * C) != hipSuccess) {
    (void)hipGetLastError();
    ANYFAIL(e, -5, "nq_any_lagr_spectrum: cannot allocate %zu bytes of device memory", (size_t)F * C * sizeof(cd));
  }
  ANYCHK(e, tmp.get(&d.win, (size_t)T));
  ANYCHK(e, tmp.get(&d.ser, (size_t)T));
  ANYCHK(e, tmp.get(&d.order, (size_t)n));
  ANYCHK(e, tmp.get(&d.offs, (size_t)G + 1));
  ANYCHK(e, tmp.get(&d.tab, (size_t)F * G));
  std::vector<LgSeries> ser((size_t)T);
  for (int r = 0; r < T; ++r) {
    ser[r].re = static_cast<const double*>(re[r]);
    ser[r].im = im ? static_cast<const double*>(im[r]) : nullptr;
    ser[r].stride = stride;
  }
  const int rc = lg_spectrum_run(e, d, ser.data(), n, T, F, window, demean, G, order, offsets, C, out);
  if (rc) (void)hipStreamSynchronize(e->stream);   // the temporaries go back with nothing queued on them
  return rc;
}

// pos[r]: the (1, n) complex plane x + i y of record r, oldest first
int nq_any_lagr_dispersion(nq_any* e, int n, int T, const void* const* pos, int G, const int* order, const int* offsets, int npairs, const int* pi,
                           const int* pj, double* out, double* out_pairs) {
  if (!e || !pos || !out || (npairs > 0 && !out_pairs)) return -1;
  if (n < 1 || T < 2) ANYFAIL(e, -1, "nq_any_lagr_dispersion: n = %d, %d records (at least 2)", n, T);
  for (int k = 0; k < T; ++k)
    if (!pos[k]) ANYFAIL(e, -1, "nq_any_lagr_dispersion: record %d has no plane", k);
  if (const char* bad = lg_check_groups(n, G, order, offsets)) ANYFAIL(e, -1, "nq_any_lagr_dispersion: %s", bad);
  if (const char* bad = lg_check_pairs(n, npairs, pi, pj)) ANYFAIL(e, -1, "nq_any_lagr_dispersion: %s", bad);
  ANYCHK(e, hipSetDevice(e->device));
  LgDev d = {};
  AnyScratch tmp;
  ANYCHK(e, tmp.get(&d.ser, (size_t)T));
  ANYCHK(e, tmp.get(&d.order, (size_t)n));
  ANYCHK(e, tmp.get(&d.offs, (size_t)G + 1));
  ANYCHK(e, tmp.get(&d.tab, (size_t)T * ((size_t)G * LG_SINGLE_SUMS + LG_PAIR_SUMS)));
  if (npairs > 0) ANYCHK(e, tmp.get(&d.pairs, 2 * (size_t)npairs));
  std::vector<LgSeries> ser((size_t)T);
  for (int r = 0; r < T; ++r) {
    ser[r].re = static_cast<const double*>(pos[r]);
    ser[r].im = ser[r].re + 1;
    ser[r].stride = 2;
  }
  const hipError_t r = lg_dispersion_run(e->stream, d, ser.data(), n, T, G, order, offsets, npairs, pi, pj, out, out_pairs);
  if (r != hipSuccess) (void)hipStreamSynchronize(e->stream);
  ANYCHK(e, r);
  return 0;
}

// f[4 r + k]: the device address of particle 0's f11, f12, f21, f22 (k = 0..3) in record r, oldest first
int nq_any_lagr_stretching(nq_any* e, int n, int T, const void* const* f, int stride, int G, const int* order, const int* offsets, double* out) {
  if (!e || !f || !out) return -1;
  if (n < 1 || T < 2 || stride < 1) ANYFAIL(e, -1, "nq_any_lagr_stretching: n = %d, %d records (at least 2), stride %d", n, T, stride);
  for (int k = 0; k < 4 * T; ++k)
    if (!f[k]) ANYFAIL(e, -1, "nq_any_lagr_stretching: record %d has no plane of entry %d", k / 4, k % 4);
  if (const char* bad = lg_check_groups(n, G, order, offsets)) ANYFAIL(e, -1, "nq_any_lagr_stretching: %s", bad);
  ANYCHK(e, hipSetDevice(e->device));
  LgDev d = {};
  AnyScratch tmp;
  ANYCHK(e, tmp.get(&d.ser, (size_t)T));
  ANYCHK(e, tmp.get(&d.order, (size_t)n));
  ANYCHK(e, tmp.get(&d.offs, (size_t)G + 1));
  ANYCHK(e, tmp.get(&d.tab, (size_t)T * G * LG_STRETCH_SUMS));
  std::vector<LgSeries> ser((size_t)T);
  for (int r = 0; r < T; ++r) {
    ser[r].re = static_cast<const double*>(f[4 * r]);
    ser[r].im = static_cast<const double*>(f[4 * r + 1]);
    ser[r].re2 = static_cast<const double*>(f[4 * r + 2]);
    ser[r].im2 = static_cast<const double*>(f[4 * r + 3]);
    ser[r].stride = stride;
  }
  const hipError_t r = lg_stretching_run(e->stream, d, ser.data(), n, T, G, order, offsets, out);
  if (r != hipSuccess) (void)hipStreamSynchronize(e->stream);
  ANYCHK(e, r);
  return 0;
}

}  // extern "C"
