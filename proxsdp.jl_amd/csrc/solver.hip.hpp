// Device-resident PDHG solve: the replacement for chambolle_pock
// (/root/reference/src/pdhg.jl:1-530) and everything below it.
//
// Host role: the scalar control logic of pdhg.jl:166-483 (a few dozen flops per
// iteration), the K x K Rayleigh-quotient eigenproblem of the thick-restart
// Lanczos, and kernel launches.  Every vector of length Nx or Q, the sparse
// operator in both orientations and the Lanczos basis live in HBM for the whole
// solve; per iteration the host reads back a handful of scalars.
//
// Here: buffer and handle owners, workspace types, the Solver class, device set-up, the dense eigensolver, the sign driver, the
// block workers.  Lanczos engine: lanczos.hip.hpp; loop: pdhg_loop.hip.hpp; dispatch: projection.hip.hpp; test hooks: test_hooks.hip.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <array>
#include <atomic>
#include <memory>
#include <mutex>
#include <condition_variable>
#include <functional>
#include <exception>
#include <rocblas/rocblas.h>
#include <rocsolver/rocsolver.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <thread>
#include <tuple>
#include <type_traits>
#include <utility>
#include <vector>

#include "host_util.hpp"
#include "block_pool.hpp"
#include "kernels.hip.hpp"
#include "lanczos_block1.hip.hpp"
#include "lanczos_wide.hip.hpp"
#include "small_sign.hip.hpp"
#include "sign_project.hip.hpp"
#include "rccl_dl.hpp"
#include "shard_group.hpp"
#include "prep.hpp"

struct proxsdp_model;               // (model.hip.hpp: a Solver kept set up between solves)

namespace proxsdp {

struct HipError : std::runtime_error { using std::runtime_error::runtime_error; };

#define PX_HIP(call)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess)                                                                \
            throw ::proxsdp::HipError(std::string(#call) + ": " + hipGetErrorString(e_) + " (" +       \
                           __FILE__ + ":" + std::to_string(__LINE__) + ")");                \
    } while (0)
#define PX_ROC(call)                                                                         \
    do {                                                                                     \
        rocblas_status s_ = (call);                                                          \
        if (s_ != rocblas_status_success)                                                    \
            throw ::proxsdp::HipError(std::string(#call) + ": rocblas status " + std::to_string((int)s_)); \
    } while (0)

// Where the device buffers allocated on this thread are counted (proxsdp_model_info.device_bytes): a model handle points it
// at its own counter for the length of a call, the block workers inherit it (start_block_workers); null everywhere else.
// `allocated`: where a call that wants to know what IT allocated (proxsdp_model_rows.bytes_allocated) has the bytes added up.
struct DevAccount {
    static inline thread_local std::atomic<long long>* sink = nullptr;
    static inline thread_local long long* allocated = nullptr;
};

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    std::atomic<long long>* acct = nullptr;     // the counter this allocation was added to, with `held` bytes
    size_t held = 0;
    DevBuf() = default;
    explicit DevBuf(size_t count) { alloc(count); }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n), acct(o.acct), held(o.held) { o.p = nullptr; o.n = 0; o.acct = nullptr; o.held = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            release();
            p = o.p; n = o.n; acct = o.acct; held = o.held;
            o.p = nullptr; o.n = 0; o.acct = nullptr; o.held = 0;
        }
        return *this;
    }
    ~DevBuf() { release(); }
    void alloc(size_t count) {
        release();
        n = count;
        if (count == 0) return;
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), count * sizeof(T));
        if (e != hipSuccess) { p = nullptr; throw std::bad_alloc(); }
        acct = DevAccount::sink;
        held = count * sizeof(T);
        if (acct) acct->fetch_add((long long)held);
        if (DevAccount::allocated) *DevAccount::allocated += (long long)held;
    }
    void release() {
        if (p) { (void)hipFree(p); p = nullptr; if (acct) acct->fetch_sub((long long)held); }
        n = 0; acct = nullptr; held = 0;
    }
    void zero(hipStream_t s) { if (n) PX_HIP(hipMemsetAsync(p, 0, n * sizeof(T), s)); }
    void upload(const T* h, size_t count, hipStream_t s) {
        if (count) PX_HIP(hipMemcpyAsync(p, h, count * sizeof(T), hipMemcpyHostToDevice, s));
    }
    void download(T* h, size_t count, hipStream_t s) const {
        if (count) PX_HIP(hipMemcpyAsync(h, p, count * sizeof(T), hipMemcpyDeviceToHost, s));
    }
};

// pinned host memory (fast, truly asynchronous small read-backs)
struct PinnedBuf {
    double* p = nullptr;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    PinnedBuf(PinnedBuf&& o) noexcept : p(o.p) { o.p = nullptr; }
    PinnedBuf& operator=(PinnedBuf&& o) noexcept { if (this != &o) { release(); p = o.p; o.p = nullptr; } return *this; }
    ~PinnedBuf() { release(); }
    void alloc(size_t count, unsigned flags = hipHostMallocDefault) {
        release();
        if (hipHostMalloc((void**)&p, count * sizeof(double), flags) != hipSuccess) { p = nullptr; throw std::bad_alloc(); }
    }
    void release() { if (p) { (void)hipHostFree(p); p = nullptr; } }
};

// move-only owners of the runtime's handles, beside the two buffers above: create() on an owner that holds a handle does
// nothing, the destructor ignores errors, and the implicit conversion hands the raw handle to the runtime's calls.
// Declare them AFTER the buffers they are used with: members are destroyed in reverse order, handles first.
template <typename H, typename Traits>
struct Owned {
    H h = nullptr;
    Owned() = default;
    Owned(const Owned&) = delete;
    Owned& operator=(const Owned&) = delete;
    Owned(Owned&& o) noexcept : h(o.h) { o.h = nullptr; }
    Owned& operator=(Owned&& o) noexcept { if (this != &o) { release(); h = o.h; o.h = nullptr; } return *this; }
    ~Owned() { release(); }
    void release() { if (h) { Traits::destroy(h); h = nullptr; } }
    operator H() const { return h; }
};
struct EventTraits { static void destroy(hipEvent_t e) { (void)hipEventDestroy(e); } };
struct StreamTraits { static void destroy(hipStream_t s) { (void)hipStreamDestroy(s); } };
struct BlasTraits { static void destroy(rocblas_handle b) { (void)rocblas_destroy_handle(b); } };
struct Event : Owned<hipEvent_t, EventTraits> {
    void create(unsigned flags = hipEventDefault) { if (!h) PX_HIP(hipEventCreateWithFlags(&h, flags)); }
};
struct Stream : Owned<hipStream_t, StreamTraits> {
    void create(unsigned flags = hipStreamDefault) { if (!h) PX_HIP(hipStreamCreateWithFlags(&h, flags)); }
};
struct BlasHandle : Owned<rocblas_handle, BlasTraits> {
    void create() { if (!h) PX_ROC(rocblas_create_handle(&h)); }
};

// milliseconds per call of `launch`, run `repeat` times on `s` between two events
template <typename F>
inline double time_launches(hipStream_t s, int repeat, F&& launch) {
    Event a, b;
    a.create(); b.create();
    PX_HIP(hipEventRecord(a, s));
    for (int i = 0; i < repeat; ++i) launch();
    PX_HIP(hipEventRecord(b, s));
    PX_HIP(hipEventSynchronize(b));
    float t = 0.f;
    PX_HIP(hipEventElapsedTime(&t, a, b));
    return (double)t / repeat;
}

static inline double now_s() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
static inline int ceil_div(long long a, long long b) { return (int)((a + b - 1) / b); }
// workgroups of a launch with one per 64 x 64 tile of the upper triangle of nt x nt tiles, padded to the 8 XCDs (xcd_tile)
static inline int tile_grid(int nt) { return 8 * ceil_div(nt * (nt + 1) / 2, 8); }
static inline int grid_for(long long n) {        // memory-bound passes: cap the grid, grid-stride the rest
    long long g = (n + dev::TPB - 1) / dev::TPB;
    return (int)std::max<long long>(1, std::min<long long>(g, 2048));
}
// spin on a stream or event query until it reports completion; every 4096 polls the caller may give up (by throwing)
template <typename Query, typename GiveUp>
inline void poll_ready(Query query, GiveUp give_up) {
    for (unsigned spins = 0;; ++spins) {
        const hipError_t e = query();
        if (e == hipSuccess) return;
        if (e != hipErrorNotReady) PX_HIP(e);
        if ((spins & 0xfff) == 0xfff) give_up();
#if defined(__x86_64__)
        _mm_pause();
#endif
    }
}
}  // namespace proxsdp
#include "shard_comm.hip.hpp"       // (the transports of a block-sharded solve: built on the buffers and macros above)
#include "merge_device.hip.hpp"     // (the rank-one merge of the split eigensolve on the device: the same buffers and owners)
namespace proxsdp {

// structs.jl:2-30
struct CircularVector {
    std::vector<double> v;
    int l = 0;
    void init(int len) { v.assign(len, 0.0); l = len; }
    double& at(long long i) { return v[(size_t)(((i - 1) % l + l) % l)]; }
    double max_abs_diff() const {
        double val = 0.0;
        for (int i = 0; i < l; ++i) val = std::max(val, std::fabs(v[i] - v[(i + l - 1) % l]));
        return val;
    }
};

// ------------------------------------------------------------------ per-block Lanczos workspace
struct EigEvents {                  // optional profiling of the dominant kernel
    std::vector<Event> e0, e1;
    size_t used = 0;
    // start / stop events of one more profiled launch (created on first use)
    std::pair<hipEvent_t, hipEvent_t> acquire() {
        if (used == e0.size()) {
            Event a, b;
            a.create(); b.create();
            e0.push_back(std::move(a)); e1.push_back(std::move(b));
        }
        ++used;
        return {e0[used - 1], e1[used - 1]};
    }
    // add the durations of the profiled launches since the last harvest to (ms, count)
    void harvest(double& ms_sum, int64_t& count) {
        for (size_t s = 0; s < used; ++s) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, e0[s], e1[s]) == hipSuccess) { ms_sum += ms; count++; }
        }
        used = 0;
    }
};

// The solver's stream.  Block workers (one host thread per PSD block while the blocks are
// projected concurrently) override it for their thread with the block's own stream, so every
// launch / copy / synchronisation inside the per-block code lands on that stream.
struct StreamRef {
    Stream main;
    static inline thread_local hipStream_t tl = nullptr;
    operator hipStream_t() const { return tl ? tl : main.h; }
};

// One cycle record `alphas[ld] | betas[ld] | LanczosCtl` of a workspace (EigWork::record: the narrow one, ld = MAXK, or the
// wide one, ld = LZW_MAXK): on the device, its pinned mirror, its length in doubles, the control block in it
struct LzRecBuf { double* dev = nullptr; double* host = nullptr; size_t doubles = 0; int ld = 0; dev::LanczosCtl* ctl = nullptr; };
enum class LzEngine { step, block1, wide };   // a run's cycles: kernels.hip.hpp, lanczos_block1.hip.hpp, lanczos_wide.hip.hpp
// What Solver::lz_plan decides once per run; everything after it reads this
struct LzPlan {
    LzEngine engine = LzEngine::step;
    LzRecBuf rec;                     // the record (and control block) this engine's kernels write
    bool split = false;               // split + rank-one merge of the K x K eigensolve (host_eig_merge.hpp), first part under the cycle
    bool dev_wanted = false;          // options.device_eig_merge asks for the merge on the device (one on the host is a fallback) ...
    bool dev_merge = false;           // ... and the run is one merge_device.hip.hpp serves: this run's merges go there
    bool fop_owner = false;           // operator form: t = Vp'v finished by column owners in the mat-vec launch (fop_owner_body)
};
// Host state of ONE thick-restart Lanczos run (one PSD block): what KrylovKit keeps between the restarts of an
// eigsolve call.  The single-block driver and the batched multi-block driver (lanczos_batch: one launch per step for
// several blocks) share the restart logic on it line by line.
struct LzRun {
    LzPlan plan;
    int nev = 0, krylovdim = 0, ld = 0;
    bool arpack = false, positive_part = false;
    double tol = 0.0, step_tol = 0.0;
    long long maxiter = 0;
    std::vector<double> T, Tw, D, U, f, al, be, Qa, da, ea;
    int howmany = 0, numiter = 1, converged = 0, K = 0, kfirst = 0, pos_count = -1, m_arrow = 0;
    bool pos_fail = false, presymv = false;
    bool first_speculated = false;    // the first mat-vec of the cycle in progress was speculated by the cycle before (lz_restart; read by the observer only)
    double betaK = 0.0;
    int k1 = 0;                       // split + rank-one merge (EigWork::split): the cycle in progress is split at step k1 ...
    bool split_cycle = false, split_ready = false;   // ... if at all, and split.first() succeeded for it
    bool merge_active = false;        // D / f of the last eigensolve came from the merge: U holds no vectors yet
    bool dev_staged = false;          // device merge: Q1 of the cycle in progress is on its way to the device
    bool merge_on_device = false;     // the last merge ran there: the Ritz-vector coefficients are DeviceMerge::Uall
    std::vector<double> erow;
};

// The host members of a block's workspace that a solve writes.  RULE: declare a per-solve host member of EigWork here, with
// the value a fresh workspace has as its initialiser, and Solver::reset_eigwork puts it back by assigning a default-constructed
// EigSolveState.  What the set-up computes (sizes, record pointers, ELL structures, fop_ok, the sign projection's tile shape)
// belongs in EigWork itself; so does a member whose reset value comes from the set-up (arrow_p), which reset_eigwork names.
struct EigSolveState {
    int ustage_next = 0;
    int rot_form = 0, rot_launches = 0;   // the last rotate_launch: PROXSDP_ROTATE_SCALAR / _MFMA / _WIDE (0: nothing launched), its launches
    // results of the last call
    std::vector<double> vals;
    int count = 0, converged_eigs = 0, numiter = 0, prev_numiter = 1;
    bool converged = false;
    int F_first = 0, F_r = 0;
    bool have_factors = false;                     // x_prev of this block is F[:, F_first .. +F_r) diag(Flam) F'
    bool use_fop = false;                          // the projection in progress uses the operator form
    // what else the dispatch (projection.hip.hpp) knows of x_prev; have_factors, F_first / F_r and ritz_ok stay beside the
    // buffers they describe: the Lanczos drivers read or drop them
    struct XPrev {
        bool sparse = true;                        // x_prev is zero off the support (initial iterate)
        int last_npos = -1;                        // positive eigenvalues found by the last projection of this block
    } xprev;
    // a block without the operator form's structures keeps no F: there the last converged Krylov projection's pairs stay
    // where the run left them -- Z[:, ritz_first .. +ritz_r) and vals[ritz_first ..) -- and ritz_ok says that x_prev of this
    // block is still their reconstruction: set at the end of that projection, dropped by whatever writes Z / vals (lanczos,
    // lanczos_batch) or the block (project_block, project_blocks, the exit path's rescale).  Read by extract_factors only.
    bool ritz_ok = false;
    int ritz_first = 0, ritz_r = 0;
    int batch_slot = 0;                            // position of this block in the batched run in progress
    // one-workgroup cycle kernel (lanczos_block1.hip.hpp): the restart rotation is deferred into the next cycle's launch
    int b1_rot_K = 0;                             // > 0: a rotation is pending, U (K x kfirst, compact) at b1_rot_U (pinned staging)
    const double* b1_rot_U = nullptr;
    LzRun lzrun;                                   // host state of the run in progress (buffers reused across projections)
    struct LanczosFullEig {                        // full_eig! served by the Lanczos engine (full_eig_by_lanczos)
        long long served = 0;                      // calls of this block it served
        bool disabled = false;                     // ... switched off after a failed verification (full_eig_lanczos_verify)
        int cert_fails = 0;                        // failed certificates of this block (full_eig_lanczos_certify)
    } fel;
    bool cye_pending = false;                      // cye[] hold a profiled k_lz_block1 launch
    const double* esv = nullptr;                   // support values of E for the projection in progress
    // per-block execution context: counters are merged into the solver's after the projections
    proxsdp_stats lst{};
    long long mv_iter = 0, recon_r = 0;
    bool fe_pending = false;
    int sg_row = -1, sg_ok = 16, sg_idle = 0, sg_hold = 0;   // shortened schedule of the sign iteration (full_eig_by_sign)
    bool sg_pending = false;                       // fe[] hold a sign projection's events (all of it is "solver")
    // cost-based engine choice on the Krylov branch (psd_sign_engine, exact_projection_by_sign): wall-clock averages of this
    // block's Lanczos and sign projections, projections since the last Lanczos probe
    struct SignStandIn {
        double kry_ms = -1.0, sign_ms = -1.0;
        int streak = 0, backoff = 0;
        int verified_left = 0;                     // projections the engine may still serve before it is checked again
        bool disabled = false, check_pending = false;
    } sign;
};

struct EigWork : EigSolveState {
    int n = 0, nt = 0, npad = 0, nwg = 0, cap = 0, pld = 0;   // cap = columns of V (krylovdim_max + 1)
    int64_t N = 0;
    DevBuf<double> V, Z;            // npad x cap each (V: Krylov basis, Z: rotation target / Ritz vectors)
    DevBuf<double> w, Ppart, hpart1, hpart2, hsum1, hred, U, lam, resid, Apart, arrow;
    DevBuf<double> resid2;           // second, independent start vector: certificate run of a Lanczos-served full_eig!
    int napart = 0;
    PinnedBuf arrow_host;
    const double* arrow_p = nullptr;   // where the kernels read the arrow part: behind U after a restart upload
    // alphas[MAXK] | betas[MAXK] | LanczosCtl in ONE device record, read back with one copy
    DevBuf<double> rec;
    double* alphas_p = nullptr; double* betas_p = nullptr; dev::LanczosCtl* ctl_p = nullptr;
    PinnedBuf rec_pinned;           // pinned mirror of `rec`
    double* rec_host = nullptr;
    static constexpr size_t REC_DOUBLES = 2 * dev::MAXK + sizeof(dev::LanczosCtl) / sizeof(double);
    static constexpr size_t USTAGE_DOUBLES = (size_t)dev::MAXK * dev::MAXK + 2 * dev::MAXK;
    size_t ustage_doubles = USTAGE_DOUBLES;   // U / Ustage capacity of THIS workspace (wide: LZW_MAXK^2 + 2 LZW_MAXK)
    // wide Lanczos (options.lanczos_wide_krylov = 1, Krylov dimension 256..511): own records, sized only when the block's
    // largest Krylov dimension exceeds 255 (the narrow buffers above are kept: the positive-part engine uses them)
    bool wide = false;
    DevBuf<double> hpw1, hpw2, hsw1, hsw2, recw;   // partial dots [pld x KW] + |w'|^2 records [pld], their sums [KW + 1], alphas | betas | ctl
    PinnedBuf recw_pinned;
    dev::LanczosCtl* ctlw_p = nullptr;
    static constexpr size_t RECW_DOUBLES = 2 * dev::LZW_MAXK + sizeof(dev::LanczosCtl) / sizeof(double);
    LzRecBuf record(bool wide_one) const {             // the record of the step kernels (and of k_lz_block1), or the wide kernels' own
        if (wide_one) return {recw.p, recw_pinned.p, RECW_DOUBLES, dev::LZW_MAXK, ctlw_p};
        return {rec.p, rec_host, REC_DOUBLES, dev::MAXK, ctl_p};
    }
    // full-eig fallback
    DevBuf<double> A, D, E;
    DevBuf<rocblas_int> info;
    std::vector<double> resid_host;
    PinnedBuf Ustage[2];            // pinned: the upload is a truly asynchronous copy (a pageable source makes the runtime stage and wait)
    // operator-form mat-vec (kernels.hip.hpp "Operator-form mat-vec")
    DevBuf<double> F, Flam, tpart, tred, ebuf, apartf;   // (lam / Flam swap roles every projection)   // F: npad x cap, the previous projection's Ritz vectors (swapped with Z)
    DevBuf<int> ell_col, ell_sidx;                 // E in ELL form, [k * npad + row]
    DevBuf<int> wr_ptr, wr_row, wr_lo, wr_hi, ov_col, ov_sidx;   // entries beyond the ELL width (hub rows)
    dev::EllOverflow ov{};
    int ell_w = 0;
    bool b1_ell_in_lds = false;                    // the last k_lz_block1 launch on the operator form held E in LDS (launch_block1)
    bool fop_ok = false;                           // structures built (support path, narrow rows)
    // the previous projection's factors (valid while have_factors, or use_fop for the projection in progress)
    struct Factors { const double* V; const double* lam; int r; };
    Factors prev_factors() const { return {F.p + (size_t)F_first * npad, Flam.p, F_r}; }
    void forget_factors() { have_factors = false; xprev.sparse = false; use_fop = false; }   // x_prev is only the packed block now
    // early read-back of the recurrence coefficients (host_eig_merge): side stream + events (below) + pinned mirror
    PinnedBuf rec_early;
    SplitEig split;
    DeviceMerge dmerge;                            // buffers of the device merge (allocated on first use)
    DevBuf<double> warm_part;                      // partial sums of the warm start (k_lz_warm_sum)
    // full_eig! by the matrix sign function (sign_project.hip.hpp): A | X | X' | Y | Q, ld x ld each
    DevBuf<double> sgA, sgX, sgX2, sgY, sgQ, sg_part, sg_part2, sg_sc;
    PinnedBuf sg_host;
    int sg_ld = 0;
    int sg_npart = 0;
    bool sg_small = false;                         // products on 32 x 32 tiles (blocks up to side 3072)
    int sg_nt48 = 0;                               // > 0: products on 48 x 48 tiles, this many per side (chosen by makespan)
    // the sign engine's verification (EigSolveState::sign) and the scratch for in-place calls
    DevBuf<double> sg_cmp;                         // max |difference|, max |value| of a verification
    DevBuf<double> sg_out;
    DevBuf<double> sg_in;                          // the packed block times a power of two (sign_project_rescaled)
    // streams and events last: destroyed before the buffers above
    Stream stream;                                 // own stream (concurrent block projections)
    Event done;
    Stream side;                                   // early read-back of the recurrence coefficients
    Event ev_mid, ev_early;
    EigEvents ev, evo;                             // profiled mat-vec / orthogonalisation launches
    Event fe[3];                                   // full_eig!: before solver | after solver | after reconstruction
    Event cye[2];                                  // profiled k_lz_block1 launch
    Event sg_ev;
};
static_assert(std::is_nothrow_move_constructible<EigWork>::value, "eig.resize() moves workspaces");


// `c` mat-vec launches of block W in the stats (negative: launches counted before that did no work)
static inline void count_matvecs(EigWork& W, long long c) {
    W.lst.symv_launches += c;
    W.lst.symv_bytes += (double)c * (8.0 * (double)W.N + 16.0 * (double)W.n);
}

// chunks of 64 columns in a basis of `cols` columns: the <NCH> argument of the step kernels' templates
static inline int lz_nch(int cols) { return (cols <= 64) ? 1 : (cols <= 128) ? 2 : (cols <= 192) ? 3 : 4; }
// f(std::integral_constant<int, lz_nch(cols)>{})
template <typename F>
static inline void with_nch(int cols, F&& f) {
    switch (lz_nch(cols)) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 3: f(std::integral_constant<int, 3>{}); break;
        default: f(std::integral_constant<int, 4>{}); break;
    }
}

// requests of one batched rotation launch (lanczos_batch): filled through Solver::rotate while a sink is installed
struct RotSink {
    // one slot per block of the batch: filled by that block's restart logic (possibly on a helper thread), packed into
    // the contiguous pinned staging buffer by flush_rotations on the calling thread
    struct Req { EigWork* W = nullptr; const double* V = nullptr; double* out = nullptr; int K = 0, ncols = 0, copy_src = -1,
                 copy_dst = 0, nextra = 0; bool valid = false; std::vector<double> data; };
    std::array<Req, dev::LZB_MAX> slot;
};

// What a caller may ask of ONE solve beyond problem and options.  The C entries (capi.hip) fill one and check it there
// (check_request); Solver::req carries it through the run; clearing it is `req = SolveRequest{}`.  All null / false: a plain
// proxsdp_hip_solve, no code of the features below runs.
struct SolveRequest {
    // state seam (proxsdp_hip_solve_ex): continue from / write out the iterate at an iteration boundary
    const proxsdp_state* resume_state = nullptr;
    proxsdp_state* capture_state = nullptr;
    // factors of the PSD solution (proxsdp_hip_solve_factored): where the caller wants them
    proxsdp_psd_factors* factors_out = nullptr;
    // warm start (proxsdp_hip_solve_from): the caller's point, validated by the entry; start_out: proxsdp_hip_start_point
    // (the solve returns after the start path and writes the internal vectors there)
    const proxsdp_start* start = nullptr;
    proxsdp_state* start_out = nullptr;
    // solution vectors on the device (proxsdp_hip_solve_device; exit_device.hip.hpp): the exit path as kernels, the caller's
    // device buffers for the result (out_dev) and for the start point (start_dev)
    bool device_exit = false;
    const proxsdp_device_vectors* start_dev = nullptr;
    proxsdp_device_vectors* out_dev = nullptr;
    // the start the solver enters from: start_dev without a start stands for one with no factors and cold steps
    const proxsdp_start* start_point() const { return (!start && start_dev) ? &none : start; }
private:
    proxsdp_start none = [] { proxsdp_start s{}; s.struct_size = (int64_t)sizeof(proxsdp_start); return s; }();
};

// The host scalars of a Solver that a solve writes.  RULE: declare a per-solve host member here, with the value it has after
// setup() as its initialiser, and Solver::reset_for_solve puts it back by assigning a default-constructed SolveState: the
// second solve on a model handle then starts from what a fresh solver has.  What comes from the options or the problem
// (init_parameters, reduce_global_constants), what the set-up built, and the certificate flags (restore_cert_data owns them)
// stay in Solver.  (A plain struct: the members that were private to Solver are reachable through it; nothing outside
// Solver and the model handle uses them.)
struct SolveState {
    // scalar state (Params, structs.jl:159-192); theta, beta and adapt_level come from the options (init_parameters)
    double primal_step = 0, primal_step_old = 0, dual_step = 0;
    long long iter = 0;
    int rank_update = 0, update_cont = 0, stop_reason = 0;
    std::string stop_reason_string = "Not optimized";
    double dual_feasibility = -1.0;
    bool certificate_search = false, certificate_found = false;
    long long certificate_search_min_iter = 0;
    int last_trials = 0;
    long long lz_matvec_iter = 0; long long recon_r_iter = 0;
    double equa_feasibility = 0, ineq_feasibility = 0;
    bool have_snapshot = false;
    bool start_active = false;            // the start gave a point: x_old = x at iteration 1 (a cold solve has x_old = 0)
    proxsdp_stats st{};
    std::exception_ptr shard_error;       // this shard's projection failed in the current iteration (see primal_step_dev)
    size_t dense_ev_used = 0;             // (Solver::dense_ev: one pair of events per pass of the current iteration)
    long long dense_passes_seen = 0;
    // PROXSDP_HIP_DEBUG: host seconds of the batched and of the single-block runs, and their cycles
    struct BatchDebug { double enqueue = 0, wait = 0, restart = 0, flush = 0, cycles = 0; } dbg_batch;
    struct LzDebug { double wait = 0, after_cycle = 0, results = 0, cycles = 0; } dbg_lz;
    double sigma_max = 0.0;               // what approx_norm = false computed (0 otherwise)
    double loop_t0 = 0;                   // start of the loop (trace column 12, stats.loop_time)
    double g_elapsed = 0;
    bool g_not_converged_rank = false, g_any_below_full = false;
    bool small_pending = false;
    int xc = 0, mtyc = 0, yc = 0, mxc = 0;     // index of the "current" buffer of each ping-pong pair
};

constexpr int NCAND = 3;    // linesearch candidates per batch (options.general_batch = 0: one); the scalar record always holds NCAND
// The device state of a Solver that follows the rows of M = [A; G]: sized by Q = p + m or by the nnz stored entries, or derived
// from M's pattern.  RULE: a device member sized by the rows or by the stored entries is declared here and allocated by build()
// / build_exit() / build_segments(), nowhere else; the set-up stages only fill.  A row change of a model handle
// (proxsdp_model::change_rows) builds a second RowState for the new shape, fills it from this one and exchanges the two.
// Not here, because the handle refuses every model whose rows would change them (capi.hip): the equilibration diagonals, the
// coupling rows' weights, the dense matrix.  The support path's structures are redone as a unit (proxsdp_model::rebuild_support).
struct RowState {
    DevBuf<int> csr_ptr, csr_col, csc_ptr, csc_row;      // the operator in both orientations, int32 indices
    DevBuf<double> csr_val, csc_val;
    bool csr_wave = false;                               // the launch shape of M x: a wave per row; the rows longer than
    int n_seg = 0, n_long = 0;                           // Solver::LONG_ROW in segments (k_spmv_csr_seg)
    DevBuf<int> seg_lo_d, seg_hi_d, long_row_d, long_ptr_d;
    DevBuf<double> segpart_d;
    DevBuf<double> bh_d, ybuf[2], Mxbuf[2], ycand_d;    // [b; h], the ping-pong pairs of y and M x, the candidates' y_c
    struct Exit {                                        // the device exit path's (exit_device.hip.hpp), built on its first use
        DevBuf<double> cval, rval;                       // the caller's unscaled values in CSC / CSR storage order
        DevBuf<double> bh, slack, part;                  // [b_orig; h_orig]; M x - [b; h]; the feasibility reductions' shares
        int feas_wg = 1;
    } exit;
    DevBuf<int> csc_pos_d, csr_pos_d;                    // a model handle's position maps (Prep::csc_pos / csr_pos), else empty

    void build(int64_t n, int64_t p, int64_t m, int64_t nnz, bool record_maps) {
        const size_t nz = (size_t)std::max<int64_t>(nnz, 1), q1 = (size_t)std::max<int64_t>(p + m, 1);
        csr_ptr.alloc((size_t)(p + m) + 1); csr_col.alloc(nz); csr_val.alloc(nz);
        csc_ptr.alloc((size_t)n + 1); csc_row.alloc(nz); csc_val.alloc(nz);
        bh_d.alloc(q1); ycand_d.alloc((size_t)NCAND * q1);
        for (int k = 0; k < 2; ++k) { ybuf[k].alloc(q1); Mxbuf[k].alloc(q1); }
        if (record_maps) { csc_pos_d.alloc(nz); csr_pos_d.alloc(nz); }
    }
    void build_exit(int64_t p, int64_t m, int64_t nnz, int feas_grid) {
        const size_t nz = (size_t)std::max<int64_t>(nnz, 1), q1 = (size_t)std::max<int64_t>(p + m, 1);
        exit.cval.alloc(nz); exit.rval.alloc(nz); exit.bh.alloc(q1); exit.slack.alloc(q1);
        exit.feas_wg = feas_grid; exit.part.alloc((size_t)4 * feas_grid);
    }
    void build_segments(int segments, int long_rows) {
        n_seg = segments; n_long = long_rows;
        if (n_seg > 0) { seg_lo_d.alloc(n_seg); seg_hi_d.alloc(n_seg); long_row_d.alloc(n_long); long_ptr_d.alloc(n_long + 1); segpart_d.alloc(n_seg); }
    }
};

class Solver : public SolveState {
public:
    // time0 is stamped BEFORE prepare(): the reference's clock starts at the top of chambolle_pock
    // (pdhg.jl:13), so preprocessing and equilibration count towards Result.time and time_limit
    // grp / grp_rank: this solver is shard grp_rank of an in-process shard group (proxsdp_hip_solve_sharded)
    // record_maps: prepare() keeps the position maps a model handle updates its values through (Prep::csc_pos / csr_pos)
    Solver(const proxsdp_problem& prob, const proxsdp_options& opt_in, proxsdp_result& res_out,
           ShardGroup* grp = nullptr, int grp_rank = 0, bool record_maps = false)
        : opt(opt_in), res(res_out), time0(now_s()),
          P(prepare(prob, &opt_in, grp != nullptr || prob.reduce_fn != nullptr || prob.nccl_comm != nullptr, record_maps)) {
        user_resid = prob.eig_resid;
        // the transport: the group, else the communicator (reduce_fn is ignored beside one), else the callbacks
        if (grp) comm.reset(new GroupComm(*grp, grp_rank, opt.host_wait_spin != 0));
        else if (prob.nccl_comm != nullptr) comm.reset(new RcclComm(prob.nccl_comm, st));
        else if (prob.reduce_fn != nullptr) comm.reset(new CallbackComm(prob));
        if (prob.n_coupling > 0) {
            if ((!prob.reduce_fn || !prob.reduce_vec_fn) && prob.nccl_comm == nullptr && grp == nullptr)
                throw std::invalid_argument("coupling rows need nccl_comm, or reduce_fn and reduce_vec_fn");
            if (!prob.coupling_rows || !prob.coupling_owned)
                throw std::invalid_argument("coupling rows need coupling_rows and coupling_owned");
            for (int64_t k = 0; k < prob.n_coupling; ++k) {
                const int64_t r = prob.coupling_rows[k];
                if (r < 0 || r >= prob.p + prob.m) throw std::invalid_argument("coupling row out of range");
                coup_rows.push_back((int)r);
                coup_owned.push_back(prob.coupling_owned[k] != 0);
            }
        }
    }
    // engine-only instance for the kernel-level test entry points (no problem data)
    Solver(const proxsdp_options& opt_in, proxsdp_result& res_out) : opt(opt_in), res(res_out) {
        time0 = now_s();
    }
    // no thread is alive when the members go; the handles (last members) are destroyed before the buffers
    ~Solver() {
        if (warm.joinable()) warm.join();
        block_pool.reset();
    }
    void run();
    // run() = setup(); solve().  A model handle (model.hip.hpp) calls setup() once and then, per solve, reset_for_solve() --
    // every member a solve writes back at the value setup() left -- and solve()
    void setup();
    void solve();
    void reset_for_solve();
    void reset_eigwork(EigWork& W);
    void restore_cert_data();
    void release_host_threads();
    double t_init0 = 0;             // start of what stats.init_time counts
    // the phases of run(), in its order (pdhg_loop.hip.hpp)
    void check_run_options();
    void init_parameters();
    void reduce_global_constants();
    void start_host_helpers();
    void alloc_iterate_pairs();
    void alloc_iterate();
    void classify_blocks();
    void start_block_workers();
    void setup_small_batch();
    void setup_soc();
    bool initial_steps();
    enum class Loop { next, stop };
    void iterate(long long k);
    Loop after_iteration(long long k);
    void finish();
    // a stop rule's declaration and the certificate search it may start (after_iteration)
    enum class Cert { infeasible, dual_infeasible };
    bool declare(int reason, const std::string& str, Cert kind, bool at_limit = false);
    void cert_infeas();
    void cert_dual_infeas();
    void snapshot();
    void update_dual_feasibility(const std::vector<double>& cvec);
    bool shard_general = false;     // block-sharded solve: this shard runs the general vector path (classify_blocks)

    // pieces also used by the kernel-level test entry points
    void setup_device();
    void alloc_eigwork(EigWork& W, int n, int max_nev);
    void lanczos_start_vector(EigWork& W, const double* user);
    // (thread-local: several batched runs may be in progress at once, one per group of blocks, each on its own worker thread)
    static inline thread_local RotSink* rot_sink = nullptr;
    // per-GROUP state of a batched run (round 5: equal-side blocks are split into groups that run CONCURRENTLY, each on its own
    // stream and host thread -- one group's restart logic on the host overlaps the other group's cycle on the GPU)
    struct BatchCtx {
        DevBuf<double> U;
        PinnedBuf U_host, rec_host;
        std::unique_ptr<SpinPool> pool;            // helper threads for the per-block restart logic
        Event ev;                                  // end of a batched cycle's record copies (the speculated mat-vecs run behind it)
    };
    std::vector<std::unique_ptr<BatchCtx>> batch_ctx;
    std::mutex batch_stats_mu;
    // helper threads for the rank-one merge of the K x K eigensolve (secular roots, Gu-Eisenstat weights, eigenvector columns:
    // independent per root / column, so the results do not depend on who computes them).  They spin only while a projection
    // with krylovdim >= 64 is in progress (armed at its start, disarmed at its end).
    std::unique_ptr<SpinPool> merge_pool;
    ParFor merge_par;
    int merge_helpers() const { return opt.host_merge_threads < 0 ? 3 : std::min(15, (int)opt.host_merge_threads); }
    static constexpr size_t LZB_USTRIDE = 64 * 64 + 2 * dev::MAXK;
    int block1_lds_cap = 0;                       // dynamic LDS granted to k_lz_block1 (setup_device)
    DevBuf<long long> b1_dbg;                     // PROXSDP_HIP_DEBUG_B1: tick sums of k_lz_block1 (prologue | loop | epilogue | steps | launches)
    bool sg48_ok = false;                         // 72 KiB of dynamic LDS granted to k_sym_gemm48 (setup_device)
    int fop_owner_knob = -1;                      // PROXSDP_HIP_FOP_OWNER (setup_device): 0 = records form always, unset = auto
    // the host driver of the Lanczos engine (lanczos.hip.hpp), in its order: launches, rotations, a run, the drivers
    EigEvents* profiled_launch(EigWork& W, int phase) const;
    void launch_symv(EigWork& W, const double* xp, const double* v, bool use_ctl, dev::LanczosCtl* ctl = nullptr);
    void launch_symv_finish(EigWork& W, const double* xp, int kclose, double tol, bool use_carry);
    void lz_launch_finish(EigWork& W, int k, double tol, bool use_carry);
    void lz_launch_begin(EigWork& W, const double* start, dev::LanczosCtl* ctl);
    void lz_launch_orth(EigWork& W, int k, int first, int keep, EigEvents* prof);
    void lz_first_matvec(EigWork& W, const double* xp, int k, bool& presymv, dev::LanczosCtl* ctl);
    void lz_launch_step(EigWork& W, const double* xp, int k, int kfirst, double step_tol, bool& presymv);
    void lzw_step(EigWork& W, LzRun& R, const double* xp, int k);
    bool block1_plan(const EigWork& W, int krylovdim, bool split_wanted) const;
    void launch_block1(EigWork& W, const double* xp, int kfirst, int krylovdim, double tol);
    void lz_read_record(const LzRecBuf& rec, double* dst, hipStream_t s);
    void rotate(EigWork& W, int K, const std::vector<double>& U, int ldu, int ncols, double* out, int copy_src, int copy_dst,
                const double* extra, int nextra);
    void rotate_launch(EigWork& W, int K, const double* Ud, int ncols, double* out, int copy_src, int copy_dst);
    void flush_rotations(RotSink& sink, BatchCtx& C);
    bool lz_init(EigWork& W, LzRun& R, int nev, bool positive_part);
    void lz_plan(EigWork& W, LzRun& R, bool single_block);
    void lz_prepare_arrow(LzRun& R);
    bool lz_split_first(EigWork& W, LzRun& R);
    bool lz_after_cycle(EigWork& W, LzRun& R, bool speculated);
    void lz_rayleigh(EigWork& W, LzRun& R, int K, double betaK, bool from_arrow, bool check_first);
    void lz_rotate_ritz(EigWork& W, LzRun& R, int ncols, double* out, int copy_src, int copy_dst, const double* extra, int nextra);
    void lz_restart(EigWork& W, LzRun& R, int keep, bool speculated);
    void lz_finish_run(EigWork& W, LzRun& R);
    void lz_start_basis(EigWork& W, LzRun& R);
    void lz_arm_split(EigWork& W, LzRun& R, ArmedPool& helpers);
    void lz_enqueue_cycle(EigWork& W, LzRun& R, const double* xp);
    bool lz_speculate(EigWork& W, LzRun& R, const double* xp);
    void lz_read_back(EigWork& W, LzRun& R);
    void lanczos(EigWork& W, const double* xp, int nev, bool positive_part = false);
    // test seam of lanczos() (test_hooks.hip.hpp test_lanczos_cycles): called once per cycle between lz_read_back and
    // lz_after_cycle -- the basis final, the record's pinned mirror valid, V and Z not yet swapped.  Null in every solve.
    const std::function<void(EigWork&, LzRun&)>* lz_observer = nullptr;
    void lanczos_eager(EigWork& W, const double* xp, int nev);
    bool lanczos_certificate(EigWork& W, const double* xp, int npos, int msteps, double& theta_max, double& scale);
    void lanczos_batch(const std::vector<int>& blocks, const double* xbase, const std::vector<int>& nevs, int ctx_slot = 0);
    void full_eig_values(EigWork& W, const double* xp, double offscale, bool vectors, std::vector<double>& Dhost);
    void begin_full_eig_events(EigWork& W);
    void harvest_full_eig_events(EigWork& W);
    void launch_reconstruct(EigWork& W, const double* Z, int ldz, const double* lam, int r, double* xp_out,
                            const double* xp_old = nullptr, int blk = -1);
    // factors of the PSD solution (req.factors_out; null: a plain solve, no new code runs): the residual kernel's launch,
    // and the extraction at the snapshot that fills `res`
    DevBuf<double> fac_V, fac_lam, fac_part;
    void factor_residual(const double* xp, int n, const double* V, int ldv, const double* lam, int r,
                         double& resid2, double& xnorm2);
    void extract_factors(const std::vector<double>& one_vals);

    // hooks of the kernel-level test entry points (test_hooks.hip.hpp)
    void test_project(int idx, double* xp, int tr);
    void test_full_eig(const double* xin, double* xout) { current_rank.assign(1, 0); min_eig.assign(1, 0.0); full_eig_project(0, xin, xout, false); }
    long long test_rank() const { return current_rank.empty() ? 0 : current_rank[0]; }
    double test_min_eig() const { return min_eig.empty() ? 0.0 : min_eig[0]; }
    void test_spmv(bool transpose, const double* in, double* out);
    void test_trial_batch(proxsdp_trial_batch& t);
    void test_project_cones(proxsdp_project_cones& t);
    void test_cone_tail(const double* x, int64_t n, const int64_t* so, const int32_t* sl, int nsoc,
                        const int64_t* oo, int none, double* x_soc, double* gap_in, double* gap_out,
                        double* x_clamp, double* mineig);
    void test_sym_product(proxsdp_sym_product& t);
    void test_reconstruct_fused(proxsdp_reconstruct_fused& t);
    void test_rotate(proxsdp_rotation& t);
    void test_tail_copy(proxsdp_tail_copy& t);
    void test_lanczos_cycles(proxsdp_lanczos_cycles& t, const double* xp, proxsdp_positive_part* pp = nullptr);
    void test_operator_cycles(proxsdp_operator_cycles& t, proxsdp_positive_part* pp = nullptr);
    void test_positive_part(proxsdp_positive_part& t, const struct LzCycleSink& out, const double* xp, int n);
    void test_observed_run(const struct LzCycleSink& out, const double* xp);
    void launch_tail_copy(const double* xin, double* xout);
    void test_sign_unpack(const double* packed, double sentinel, double* A, double* sc);

    bool debug = std::getenv("PROXSDP_HIP_DEBUG") != nullptr;
    proxsdp_options opt;
    proxsdp_result& res;
    double time0 = 0;               // (declared before P: initialised first)
    Prep P;
    SolveRequest req;               // what this solve was asked for beyond problem and options
    const double* user_resid = nullptr;
    // block-sharded solve: how this shard reaches the others (shard_comm.hip.hpp); none when the solve is not sharded
    std::unique_ptr<ShardComm> comm;
    bool sharded() const { return comm != nullptr; }
    long long current_iteration() const { return iter; }   // (the iteration a failed shard stopped in: proxsdp_hip_solve_sharded)
    void reduce(std::vector<double>& sums, std::vector<double>& maxs) { if (comm) comm->reduce(stream, sums, maxs); }
    void reduce_vec_host(std::vector<double>& v) { if (!v.empty()) comm->reduce_vec_host(stream, v); }
    // coupling rows of a block-sharded solve (include/proxsdp_hip.h): partial M x summed over the shards
    std::vector<int> coup_rows;
    std::vector<char> coup_owned;
    DevBuf<int> coup_rows_d;
    DevBuf<double> roww_d;
    void reduce_coupling(double* Mx_dev) {         // Mx[coupling rows] <- sum over shards
        if (!coup_rows.empty()) comm->reduce_coupling(stream, Mx_dev, coup_rows_d.p, (int)coup_rows.size());
    }
    // wait for the solver's (or the calling block thread's) stream at a read-back on the critical path
    void wait_stream() {
        if (!comm || !comm->bounded_wait(stream)) wait_for_stream(stream, opt.host_wait_spin != 0);
    }
    // state seam (req.resume_state, req.capture_state)
    void check_state_shape(const proxsdp_state& s, const char* what) const;
    void apply_resume();
    void write_capture();
    // warm start (req.start_point(), req.start_out)
    DevBuf<long long> start_ord_d;
    DevBuf<double> start_src_d, start_V, start_lam;
    void apply_start();
    void write_start_point();
    // solution vectors on the device (req.device_exit, req.start_dev, req.out_dev; exit_device.hip.hpp)
    void check_start_dev();
    void cache_solution_device(bool zero_c);
    void test_exit_vectors(const double* x, const double* y, bool zero_c, double* primal, double* dual_cone, double* dual_eq,
                           double* dual_in, double* slack_eq, double* slack_in, double* viol, double* neg, int64_t neg_cap);
    int ada_count = 0;                    // pdhg.jl:306-332 (a local of chambolle_pock)
    void wait_event(hipEvent_t ev) {
        if (opt.host_wait_spin == 0) PX_HIP(hipEventSynchronize(ev));
        else poll_ready([&]() { return hipEventQuery(ev); }, []() {});
    }
    // global (all-shard) problem constants; equal to the local ones when not sharded
    double g_n = 0, g_Q = 0, g_p = 0, g_m = 0, g_norm_b = 0, g_norm_h = 0, g_norm_c = 0, g_frob = 0;
    bool g_conic = false;
    bool init_only = false;         // proxsdp_hip_dense_scaling: run() returns after the "Init" section
    std::thread warm;               // loads rocSOLVER's code objects while the loop runs
    // concurrent block projections: one worker thread per PSD block (up to 8), each driving its
    // block's Lanczos on the block's own stream
    std::mutex blas_mutex;
    std::unique_ptr<BlockPool> block_pool;     // (block_pool.hpp) up while the blocks are projected concurrently
    bool parallel_blocks() const { return block_pool != nullptr; }
    void run_blocks(const std::vector<int>& blocks, const std::function<void(int)>& job);
    void merge_block_stats();
    void start_rocsolver_warmup();

private:
    friend struct ::proxsdp_model;
    // device state
    DevBuf<double> xbuf[2], Mtybuf[2], c_d, part, scal;
    RowState rs;                               // the operator, y, M x, [b; h]: everything sized by the rows (the rule is at the struct)
    void build_rows() { if (rs.csr_ptr.n == 0) rs.build(P.n, P.p, P.m, P.nnz, P.record_maps); }   // (the first set-up stage that needs it)
    std::vector<double> stacked_bh(const std::vector<double>& b, const std::vector<double>& h) const;
    DevBuf<long long> one_off, soc_off;
    DevBuf<int> soc_len;
    DevBuf<double> one_min, soc_gap_d;
    std::vector<int> one_blocks;               // indices of 1x1 PSD blocks
    std::vector<int> big_blocks;               // indices of the blocks that are projected by an eigensolver
    // blocks of side 2..64 below min_size_krylov_eigs: one batched Jacobi launch on the dense vector path
    std::vector<int> small_blocks, large_blocks;
    DevBuf<long long> small_off;
    DevBuf<int> small_side, small_rank;        // small_rank: [rank | npos] per block
    PinnedBuf small_rank_host;
    int small_maxn = 0;
    int small_jacobi_max = 64;                 // small blocks up to this side: batched Jacobi; above: k_small_sign_project
    int small_sign_maxn = 0;                   // largest side served by k_small_sign_project (0: none)
    std::vector<int> small_sweeps;             // per small block, from the last harvest: sweeps k_small_psd_project ran (-1: a sign block)
    int small_sign_cap = 0;                    // largest side whose dynamic LDS the device grants (setup_device; 64 on gfx950)
    // per-iteration read-backs written by the kernels straight into pinned host memory: only where the iteration leaves little
    // dirty data behind (a kernel that stores to host memory ends with a system-scope release)
    bool zero_copy_small() const { return P.n <= (1 << 16); }
    void project_small_blocks(double* x);
    void harvest_small_ranks();
    int rotate_lds_cap = 60 * 1024;           // dynamic LDS granted to k_lz_rotate (setup_device)
    int rotate_mfma_lds_cap = 0;              // ... to k_lz_rotate_mfma
    // rows longer than LONG_ROW entries: segmented SpMV (kernels.hip.hpp k_spmv_csr_seg)
    static constexpr int LONG_ROW = 8192;
    void setup_long_rows(RowState& to, const std::vector<int>& rp);

    // scalar state (Params, structs.jl:159-192) that init_parameters() and reduce_global_constants() set; the rest is SolveState's
    double theta = 1, beta = 1, adapt_level = 0.9;
    std::vector<long long> target_rank, current_rank;
    std::vector<double> min_eig;
    long long max_iter_local = 0;
    double time_limit = 0;
    // histories (Residuals, structs.jl:100-125)
    CircularVector h_gap, h_pobj, h_dobj, h_feas, h_pres, h_dres, h_comb;

    void primal_step_dev();
    void psd_projection(double* x);
    // the dispatch of psd_projection! (projection.hip.hpp), in call order
    void project_blocks(const std::vector<int>& blocks, const double* xin, double* xout, bool fuse);
    bool krylov_branch(int idx) const;
    bool batch_eligible(int idx, bool fuse) const;
    bool fop_eligible(const EigWork& W, bool fuse) const;
    void arm_fop(EigWork& W);
    void project_block(int idx, const double* xin, double* xout, bool fuse);
    void full_eig_branch(int idx, const double* xp, double* xo, bool fuse);
    void krylov_run(int idx, const double* xp, double* xo, bool fuse, int nev);
    void finish_krylov_run(int idx, const double* xp, double* xo, bool fuse, int nev);
    void ritz_pairs_to_block(int idx, const double* xp, double* xo, bool fuse, int first, int npos);
    void dense_pairs_to_block(int idx, const double* xp_in, double* xp_out, bool fuse, int npos);
    struct ShadowBookkeeping;
    bool matches_shadow(EigWork& W, const double* xo);
    void build_block_operator(EigWork& W, const BlockInfo& B, const std::vector<int>& supp, size_t s0, size_t s1);
    void setup_support();
    void setup_dense();
    std::vector<int> support_list() const;
    bool support_path_wanted(size_t ns) const;
    void upload_support(const std::vector<int>& supp);
    void upload_sparse_operator();
    void upload_pattern(RowState& to, const Prep& R);
    void launch_clamp_scalars(double* x, int cnt);
    void launch_soc_project(double* x, int nsoc);
    void launch_soc_gap(const double* x, int nsoc);
    void launch_primal_update_S(double* x, double tau);
    void alloc_candidates();
    // one batch of linesearch candidates (pdhg_loop.hip.hpp): launch shapes, the launches, the read-back
    struct BatchShape {
        int gq, gx; long long cstride, ystride, mstride;
        // the vector path: the batch runs over cnt entries of x -- supp[0 .. cnt) (the support path; c, x_old and M'y are
        // compact on the support) or, with supp == nullptr, every entry (the general path; full vectors)
        const int* supp; long long cnt;
        const double* xold; const double* cv;        // x_old and c on those entries
        double* mty_cur; double* mty_commit;         // M'y of the iterate, and where commit puts the accepted candidate's
    };
    BatchShape batch_shape() const;
    void batch_evaluate(const dev::TrialBatch& tb, int nc, double xold_coef);
    void batch_mty(const dev::TrialBatch& tb, int nc);
    void batch_residuals(const dev::TrialBatch& tb, int nc, int c0, double xold_coef);
    const double* batch_read_back(int nc);
    const double* linesearch_and_residuals();
    void reduce_candidates(int nc);
    void record_residuals(const double* s);
    void dense_mv(const double* x, double* y, bool scaled);
    void dense_mtv(int nc, const double* Y, long long ystride, bool scaled, double* OUT, long long ostride,
                   const double* old, const double* addc, double* normpart, long long cstride, bool addback);
    void full_eig_project(int idx, const double* xp_in, double* xp_out, bool fuse);
    bool full_eig_by_lanczos(int idx, const double* xp_in, double* xp_out, bool fuse);
    bool full_eig_by_sign(int idx, const double* xp_in, double* xp_out, bool fuse, bool force = false);
    bool sign_project_rescaled(int idx, double* xp_out, bool fused, bool force, const proxsdp_stats& before);
    void truncated_project_dense(int idx, const double* xp_in, double* xp_out, bool fuse, int nev);
    // acceptance threshold of the Lanczos-served full_eig! (options.full_eig_lanczos_posres, default 1e-6 of the spectral
    // scale), never looser than 1 % of the tightest tolerance the user asked for (a user at tolerance 1e-7
    // must not be handed a projection that may miss a positive eigenvalue of 1e-6)
    double lanczos_posres() const {
        const double base = opt.full_eig_lanczos_posres > 0.0 ? opt.full_eig_lanczos_posres : 1e-6;
        const double tmin = std::min({opt.tol_gap, opt.tol_feasibility, opt.tol_primal, opt.tol_dual});
        return tmin > 0.0 ? std::min(base, 1e-2 * tmin) : base;
    }
    // the step kernels run Krylov dimensions up to 255; with lanczos_wide_krylov = 1 the wide kernels up to 511 (not under
    // krylovkit_eager, whose driver is written on the step kernels)
    int krylov_dim(int nev) const { return std::max(2 * nev + 1, (int)opt.eigsolver_min_lanczos); }   // (eigsolver.jl: krylovdim / ncv)
    bool krylovdim_fits(int nev) const {
        const int kd = krylov_dim(nev);
        if (kd <= dev::LZ_KMAX) return true;
        return opt.lanczos_wide_krylov == 1 && kd <= dev::LZW_MAXK - 1 && !(opt.krylovkit_eager && opt.eigsolver != 1);
    }
    bool exact_projection_by_sign(int idx, const double* xp, double* xo, bool fuse, int nev);
    void verify_sign_engine(int idx, const double* xo);
    template <int EPI, bool FUSE>
    void sym_gemm(EigWork& W, const double* Pm, const double* Qm, double* T, const double* Y, double ca, double cb,
                  double cc, const double* dsc, double* part, double* xp_out, const double* xp_old, int blk);
    // tile shape of the sign iteration's products, and what follows from it (shared with the kernel-level test entries)
    bool sign_tile48_fits(int n, int ld) const { return sg48_ok && ceil_div(n, dev::SG_T48) * dev::SG_T48 <= ld; }
    static int sym_gemm_grid(const EigWork& W, bool final_epi);
    void sign_choose_tiles(EigWork& W);
    void sign_unpack(EigWork& W, const double* xp_in, double* A, double* sc);
    void sign_scale(EigWork& W, double* sc);
    void spmv(const double* x, double* y);
    void spmv_sparse(const double* x, double* y);
    bool convergedrank() const;
    bool soc_convergence();
    double dual_feas_host(const std::vector<double>& y, const std::vector<double>& cvec,
                          std::vector<double>* dual_eq, std::vector<double>* dual_in, std::vector<double>* dual_cone);
    void cache_solution(const std::vector<double>& cvec);
    template <typename Fill> double dual_block_min_eig(size_t idx, Fill&& fill);
    void finish_snapshot(double dfeas);
    // the device exit path's pieces and what they read (exit_device.hip.hpp)
    struct ExitDev {
        bool ready = false;                    // (with it RowState::exit: the unscaled values, [b_orig; h_orig], the slack)
        DevBuf<double> c, zero;                // c_orig; zeros (dense A with c = 0)
        DevBuf<long long> inv, one_off, soc_off;
        DevBuf<int> soc_len;
        std::vector<int> ones;                 // the 1x1 PSD cones, in cone order
        DevBuf<double> dc, base;               // the dual cone; c + A'y of a dense A
        DevBuf<double> prim, dcone, onev;      // staging where the caller gave no device buffer; the 1x1 cones' x
        DevBuf<double> scal;
    } xd;
    void exit_rescale_iterate();
    void exit_device_setup();
    int exit_feas_grid(int64_t m) const;
    void exit_form_vectors(bool zero_c);
    void exit_cone_violations(double viol[4]);
    void exit_write_vectors(const proxsdp_device_vectors* dv, double* primal, double* dual_cone, double* dual_eq,
                            double* dual_in, double* slack_eq, double* slack_in);
    void certificate_parameters();
    void bump_rank(int idx);
    std::vector<double> b_host, h_host, c_host;   // current (possibly zeroed by a certificate search)
    bool cert_zeroed_c = false, cert_zeroed_bh = false;   // ... and with them c_d / cS_d, bh_d: reset_for_solve uploads them again
    // support-aware vector passes
    bool use_support = false;
    // the general path inside a block-sharded solve: its residual pass takes the row weights (b'y and h'y count a coupling
    // row on its owner only), as the support path's always does; a solve that is not sharded keeps the null pointer
    bool general_row_weights = false;
    int ns = 0, rstride = 0, n_res_wg = 0;
    std::vector<int> supp_h;                    // the support list as uploaded (upload_support)
    std::vector<int> tile_base;                 // first residual-partial slot of each PSD block
    DevBuf<int> supp_d;
    DevBuf<unsigned> mask_d;
    DevBuf<double> cS_d, xsave_d, MtyS_cur, respart_d;
    DevBuf<double> Ediag_d, Ddiag_d; // equilibration diagonals (exit path)
    DevBuf<double> esv_d;            // [2][ns]: support values of E (update only | whole entry), k_primal_update_S
    // dense constraint matrix (proxsdp_problem.M_dense): borrowed device pointer or own upload
    const double* Md = nullptr;
    DevBuf<double> Md_own, dmv_part;
    DevBuf<unsigned char> offdiag_d;
    int dmv_slices = 1, dmv_qpad = 0;
    static constexpr int DMV_ROWS = 8, DMV_UNR = 4;       // k_dense_mv shape (rows per workgroup, strips in flight)
    // equilibration / approx_norm = false on a dense A: set-up on the device (one pass over M: row sums + extrema), scale
    // vectors E (rows of the dense block) and D o s (columns) for the products, Lanczos for sigma_max
    void upload_dense();
    void setup_dense_scaling();
    double spectral_norm_device();
    DevBuf<double> drow_d, dcol_d;   // E[0..p), D o s
    double dense_frob2 = 0.0;        // ||E A D S||_F^2 of the dense block, from the set-up pass's row sums
    void dense_ev_begin();
    void dense_ev_end();
    void dense_ev_harvest();
    // linesearch candidates (linesearch_and_residuals): y_c, M'y_c, partials, the scalar record on the device and its
    // read-back (support path: hbscal; otherwise the pinned hscal_pin)
    DevBuf<double> Mtycand_d, bpart, bscal;      // (y_c: RowState::ycand_d)
    std::vector<double> hbscal;
    PinnedBuf hscal_pin;

public:
    // The last members, destroyed first and in reverse: ev_main, dense_ev, the rocBLAS handle and the main stream go before
    // any buffer, as they always did; then every block's workspace (its own streams and events before its buffers,
    // EigWork's order); then the solver's buffers above.
    std::vector<EigWork> eig;
    StreamRef stream;
    BlasHandle blas;
    std::vector<std::pair<Event, Event>> dense_ev;
    Event ev_main;                             // run_blocks: the block streams start behind it
};

// ------------------------------------------------------------------ setup
inline void Solver::alloc_eigwork(EigWork& W, int n, int max_nev) {
    W.n = n;
    W.N = (int64_t)n * (n + 1) / 2;
    W.nt = ceil_div(n, dev::TILE);
    W.npad = W.nt * dev::TILE;
    W.nwg = ceil_div(n, dev::TPB);
    // the step kernels run Krylov dimensions up to dev::LZ_KMAX = 255; a projection whose Krylov dimension
    // max(2 target_rank + 1, eigsolver_min_lanczos) is larger (options.jl:76,88 accept any value) is served by the dense
    // eigensolver instead (Solver::truncated_project_dense): the workspace is sized for what the kernels can run
    // (with lanczos_wide_krylov = 1 up to 511 columns: the wide kernels, lanczos_wide.hip.hpp)
    const int kd_want = krylov_dim(max_nev);
    W.wide = opt.lanczos_wide_krylov == 1 && kd_want > dev::LZ_KMAX;
    int kd = std::min(kd_want, W.wide ? dev::LZW_MAXK - 1 : dev::LZ_KMAX);
    W.cap = kd + 1;
    W.V.alloc((size_t)W.npad * W.cap);
    W.Z.alloc((size_t)W.npad * W.cap);
    W.w.alloc(W.npad);
    W.Ppart.alloc((size_t)W.nt * W.npad);
    W.pld = ceil_div(W.nt, dev::WAVE) * dev::WAVE;   // partial dots: [MAXK][pld], padding stays zero
    W.hpart1.alloc((size_t)W.pld * dev::MAXK);
    W.hpart2.alloc((size_t)W.pld * dev::MAXK);
    W.hpart1.zero(stream); W.hpart2.zero(stream);
    W.hsum1.alloc(dev::MAXK);
    W.hred.alloc(dev::MAXK); W.hred.zero(stream);
    W.napart = tile_grid(W.nt);
    W.Apart.alloc(W.napart); W.Apart.zero(stream);      // padding tiles never write: stay zero
    W.arrow.alloc(2 * dev::MAXK); W.arrow.zero(stream);   // arrow: f | D (see k_lz_orth)
    W.arrow_host.alloc(2 * dev::MAXK);
    W.rec.alloc(EigWork::REC_DOUBLES);
    W.alphas_p = W.rec.p; W.betas_p = W.rec.p + dev::MAXK;
    W.ctl_p = reinterpret_cast<dev::LanczosCtl*>(W.rec.p + 2 * dev::MAXK);
    W.rec_pinned.alloc(EigWork::REC_DOUBLES);
    W.rec_host = W.rec_pinned.p;
    W.ustage_doubles = W.wide ? (size_t)dev::LZW_MAXK * dev::LZW_MAXK + 2 * dev::LZW_MAXK : EigWork::USTAGE_DOUBLES;
    W.U.alloc(W.ustage_doubles);
    W.Ustage[0].alloc(W.ustage_doubles); W.Ustage[1].alloc(W.ustage_doubles);
    if (W.wide) {
        // records of the nt producers: V'w at [g * KW, g * KW + KW), |w'|^2 at pld * KW + g (g < nt <= pld; nt reaches 725 at
        // side 46340, beyond KW: the norm records get a row of their own, sized by pld)
        if (W.nt > W.pld) throw std::logic_error("wide Lanczos: more producers than partial-dot records");
        const size_t hpw_doubles = dev::lzw_hpart_doubles(W.pld);
        W.hpw1.alloc(hpw_doubles); W.hpw2.alloc(hpw_doubles);
        W.hpw1.zero(stream); W.hpw2.zero(stream);
        W.hsw1.alloc(dev::KW + 1); W.hsw2.alloc(dev::KW + 1);
        W.hsw1.zero(stream); W.hsw2.zero(stream);
        W.recw.alloc(EigWork::RECW_DOUBLES); W.recw.zero(stream);
        W.ctlw_p = reinterpret_cast<dev::LanczosCtl*>(W.recw.p + 2 * dev::LZW_MAXK);
        W.recw_pinned.alloc(EigWork::RECW_DOUBLES);
    }
    W.arrow_p = W.arrow.p;
    W.lam.alloc(std::max(n, dev::MAXK));
    W.resid.alloc(W.npad);
    W.V.zero(stream); W.Z.zero(stream); W.w.zero(stream);
    W.hsum1.zero(stream); W.rec.zero(stream);
    W.resid.zero(stream);
}

inline void Solver::setup_device() {
    int ndev = 0;
    PX_HIP(hipGetDeviceCount(&ndev));
    if (ndev <= 0) throw HipError("no HIP device available");
    if (opt.device_id < 0 || opt.device_id >= ndev) throw std::invalid_argument("device_id out of range");
    if (opt.lanczos_wide_krylov != 0 && opt.lanczos_wide_krylov != 1) throw std::invalid_argument("lanczos_wide_krylov must be 0 or 1");
    if (opt.lanczos_cycle_kernel == 1) opt.lanczos_cycle_kernel = 0;   // (1 selected the retired persistent cycle kernel)
    PX_HIP(hipSetDevice(opt.device_id));
    stream.main.create();
    // gfx950: 160 KiB of LDS per CU.  The restart rotation at K = 127, keep = 78 needs 145 KiB (U tile + V tile): with 144 KiB
    // it fell into two launches (54 us on average, profiles/r03b); take the largest grant the runtime accepts
    rotate_lds_cap = 60 * 1024;
    for (int kb : {160, 156, 152, 144}) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(dev::k_lz_rotate),
                                hipFuncAttributeMaxDynamicSharedMemorySize, kb * 1024) == hipSuccess) { rotate_lds_cap = kb * 1024; break; }
        (void)hipGetLastError();
    }
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(dev::k_lzb_rotate), hipFuncAttributeMaxDynamicSharedMemorySize, rotate_lds_cap);
    for (int kb : {156, 152, 144, 128, 96, 64}) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(dev::k_lz_rotate_mfma),
                                hipFuncAttributeMaxDynamicSharedMemorySize, kb * 1024) == hipSuccess) { rotate_mfma_lds_cap = kb * 1024; break; }
        (void)hipGetLastError();
    }
    sg48_ok = true;
    for (const void* f : {reinterpret_cast<const void*>(dev::k_sym_gemm48<dev::SG_PLAIN, 4>), reinterpret_cast<const void*>(dev::k_sym_gemm48<dev::SG_POLY, 4>)})
        sg48_ok = sg48_ok && hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dev::sg48_lds_bytes(4)) == hipSuccess;
    if (!sg48_ok) (void)hipGetLastError();
    // one-launch small-block projection: 4 matrices of side x (side + 2) doubles in LDS (132 KiB at side 64).  Probed here so
    // that a device / partition that does not grant it sends the larger of those blocks to the tiled engines instead of
    // failing the solve
    small_sign_cap = 0;
    for (int sd : {64, 56, 48, 40, 32, 24, 16}) {
        const size_t bytes = dev::small_sign_lds_bytes(sd);
        if (bytes <= 48 * 1024 || hipFuncSetAttribute(reinterpret_cast<const void*>(dev::k_small_sign_project),
                                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess) {
            small_sign_cap = sd;
            break;
        }
        (void)hipGetLastError();
    }
    if (std::getenv("PROXSDP_HIP_DEBUG_B1") != nullptr) { b1_dbg.alloc(8); b1_dbg.zero(stream); }
    // PROXSDP_HIP_FOP_OWNER = 0: the operator-form step stays on the records form (A/B measurement); unset: lz_plan decides
    if (const char* env = std::getenv("PROXSDP_HIP_FOP_OWNER")) fop_owner_knob = (env[0] == '0' && env[1] == 0) ? 0 : -1;
    block1_lds_cap = 0;
    for (int kb : {160, 144, 128, 112, 96}) {
        bool ok = true;
        for (const void* f : {reinterpret_cast<const void*>(dev::k_lz_block1<1, false>), reinterpret_cast<const void*>(dev::k_lz_block1<2, false>),
                              reinterpret_cast<const void*>(dev::k_lz_block1<1, true>), reinterpret_cast<const void*>(dev::k_lz_block1<2, true>)})
            ok = ok && hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, kb * 1024) == hipSuccess;
        if (ok) { block1_lds_cap = kb * 1024; break; }
        (void)hipGetLastError();
    }
    blas.create();
    PX_ROC(rocblas_set_stream(blas, stream));
}

// rocSOLVER's first dsyevd in a process pays ~3 s of code-object loading.  The exit path
// (cone_feas, pdhg.jl:685) always needs one.  Optional (PROXSDP_HIP_WARMUP=1): a dummy dsyevd
// on a private handle/stream in a background thread -- OFF by default because the loader
// serialises against the solver thread's launches.
inline void Solver::start_rocsolver_warmup() {
    const int dev_id = opt.device_id;
    warm = std::thread([dev_id]() {
        if (hipSetDevice(dev_id) != hipSuccess) return;
        try {
            Stream s;
            BlasHandle h;                               // (destroyed before its stream)
            s.create(); h.create();
            (void)rocblas_set_stream(h, s);
            double* buf = nullptr;
            rocblas_int* info = nullptr;
            const int n = 96;                           // large enough to take the blocked path
            if (hipMalloc((void**)&buf, sizeof(double) * (n * n + 2 * n)) == hipSuccess &&
                hipMalloc((void**)&info, sizeof(rocblas_int)) == hipSuccess) {
                (void)hipMemsetAsync(buf, 0, sizeof(double) * (n * n + 2 * n), s);
                (void)rocsolver_dsyevd(h, rocblas_evect_original, rocblas_fill_upper, n, buf, n,
                                       buf + n * n, buf + n * n + n, info);
                (void)rocsolver_dsyevd(h, rocblas_evect_none, rocblas_fill_upper, n, buf, n,
                                       buf + n * n, buf + n * n + n, info);
                (void)hipStreamSynchronize(s);
            }
            if (buf) (void)hipFree(buf);
            if (info) (void)hipFree(info);
        } catch (...) {}                                // (a warm-up that cannot get its stream or handle does nothing)
    });
}

// ------------------------------------------------------------------ kernels launch helpers
inline void Solver::launch_reconstruct(EigWork& W, const double* Z, int ldz, const double* lam, int r, double* xp_out,
                                       const double* xp_old, int blk) {
    const int ntile = W.napart;
    // fp64 MFMA SYRK from rank 16 on in auto mode (measured cross-over at n = 4000: equal at 12-16,
    // 1.17x at 26, 1.32x at 63, 1.7x at n/2; docs/DESIGN_history_r1_r3.md section 5)
    const bool mfma = opt.reconstruct_mfma == 1 || (opt.reconstruct_mfma < 0 && r >= 16);
    if (mfma) {
        W.lst.mfma_reconstructions++;
        if (use_support && xp_old != nullptr && blk >= 0)
            hipLaunchKernelGGL(dev::k_reconstruct_mfma<true>, dim3(ntile), dim3(dev::TPB), 0, stream,
                               Z, ldz, lam, r, W.n, xp_out, xp_old, mask_d.p, (long long)P.blocks[blk].off,
                               respart_d.p + tile_base[blk], rstride);
        else
            hipLaunchKernelGGL(dev::k_reconstruct_mfma<false>, dim3(ntile), dim3(dev::TPB), 0, stream,
                               Z, ldz, lam, r, W.n, xp_out, (const double*)nullptr, (const unsigned*)nullptr, 0LL,
                               (double*)nullptr, 0);
        return;
    }
    if (use_support && xp_old != nullptr && blk >= 0)
        hipLaunchKernelGGL(dev::k_reconstruct_packed<true>, dim3(ntile), dim3(dev::TPB), 0, stream,
                           Z, ldz, lam, r, W.n, xp_out, xp_old, mask_d.p, (long long)P.blocks[blk].off,
                           respart_d.p + tile_base[blk], rstride);
    else
        hipLaunchKernelGGL(dev::k_reconstruct_packed<false>, dim3(ntile), dim3(dev::TPB), 0, stream,
                           Z, ldz, lam, r, W.n, xp_out, (const double*)nullptr, (const unsigned*)nullptr, 0LL,
                           (double*)nullptr, 0);
}

// ||X - V diag(lam) V'||_F^2 and ||X||_F^2 of a packed block with plain entries (k_factor_residual): device pointers in, the
// tiles' partial pairs summed on the host in tile order.  Synchronises the stream.
inline void Solver::factor_residual(const double* xp, int n, const double* V, int ldv, const double* lam, int r,
                                    double& resid2, double& xnorm2) {
    const int nt = ceil_div(n, dev::TILE);
    const int tiles = nt * (nt + 1) / 2;
    if (fac_part.n < (size_t)2 * tiles) fac_part.alloc((size_t)2 * tiles);
    hipLaunchKernelGGL(dev::k_factor_residual, dim3(tile_grid(nt)), dim3(dev::TPB), 0, stream,
                       xp, n, V, ldv, lam, r, fac_part.p);
    PX_HIP(hipGetLastError());
    std::vector<double> h((size_t)2 * tiles);
    fac_part.download(h.data(), h.size(), stream);
    PX_HIP(hipStreamSynchronize(stream));
    resid2 = 0.0; xnorm2 = 0.0;
    for (int t = 0; t < tiles; ++t) { resid2 += h[2 * t]; xnorm2 += h[2 * t + 1]; }
}

// eigen!(Symmetric(smat(xp))) through rocSOLVER dsyevd (ascending), the dense
// fallback (prox_operators.jl:113, pdhg.jl:685)
inline void Solver::full_eig_values(EigWork& W, const double* xp, double offscale, bool vectors,
                                    std::vector<double>& Dhost) {
    const int n = W.n;
    if (W.A.n < (size_t)n * n) {
        W.A.alloc((size_t)n * n); W.D.alloc(n); W.E.alloc(n); W.info.alloc(1);
    }
    const int ntile = W.nt * (W.nt + 1) / 2;
    // a block of tiny or huge entries (largest |entry| outside [2^-400, 2^400]): dsyevd's squares leave the fp64 range -- at
    // 2^-600 it returned the diagonal, silently; at 2^520 it did not converge -- so such a block is scaled by an exact power of
    // two on the way in and its eigenvalues scaled back, all on the device (no host round trip; nothing happens in range)
    if (W.sg_cmp.n < 2) W.sg_cmp.alloc(2);
    W.sg_cmp.zero(stream);
    hipLaunchKernelGGL(dev::k_maxdiff, dim3(grid_for(W.N)), dim3(dev::TPB), 0, stream, xp, xp, (long long)W.N, W.sg_cmp.p);
    hipLaunchKernelGGL(dev::k_unpack_upper, dim3(ntile), dim3(dev::TPB), 0, stream, xp, n, W.A.p, n, offscale);
    hipLaunchKernelGGL(dev::k_ldexp_range, dim3(grid_for((long long)n * n)), dim3(dev::TPB), 0, stream, W.A.p, (long long)n * n,
                       (const double*)W.sg_cmp.p + 1, -1);
    std::lock_guard<std::mutex> lk(blas_mutex);          // one rocBLAS handle: dense fallbacks run one at a time
    PX_ROC(rocblas_set_stream(blas, (hipStream_t)stream));
    PX_ROC(rocsolver_dsyevd(blas, vectors ? rocblas_evect_original : rocblas_evect_none, rocblas_fill_upper,
                            n, W.A.p, n, W.D.p, W.E.p, W.info.p));
    hipLaunchKernelGGL(dev::k_ldexp_range, dim3(1), dim3(dev::TPB), 0, stream, W.D.p, (long long)n, (const double*)W.sg_cmp.p + 1, 1);
    Dhost.resize(n);
    rocblas_int info = 0;
    W.D.download(Dhost.data(), n, stream);
    PX_HIP(hipMemcpyAsync(&info, W.info.p, sizeof(info), hipMemcpyDeviceToHost, stream));
    PX_HIP(hipStreamSynchronize(stream));
    if (info != 0) throw HipError("rocsolver_dsyevd did not converge (info=" + std::to_string(info) + ")");
}

// workgroups Solver::sym_gemm launches for one product on W's tile shape: one per tile of the block upper triangle, rounded up
// to a multiple of 8 (the XCD-interleaved tile order; the padding workgroups return at once).  The final product always runs
// on 64 x 64 tiles: its residual partials are indexed by them.
inline int Solver::sym_gemm_grid(const EigWork& W, bool final_epi) {
    const int side = final_epi ? W.nt : (W.sg_nt48 > 0 ? W.sg_nt48 : (W.sg_small ? 2 * W.nt : W.nt));
    return tile_grid(side);
}

// full_eig! (prox_operators.jl:111-126)
template <int EPI, bool FUSE>
inline void Solver::sym_gemm(EigWork& W, const double* Pm, const double* Qm, double* T, const double* Y, double ca,
                             double cb, double cc, const double* dsc, double* part, double* xp_out,
                             const double* xp_old, int blk) {
    W.lst.sign_products++;
    const int grid = sym_gemm_grid(W, EPI == dev::SG_FINAL);
    if constexpr (EPI != dev::SG_FINAL) {
        if (W.sg_nt48 > 0) {                                // 48 x 48 tiles: fewer, larger tiles where that shortens the busiest CU's queue
            hipLaunchKernelGGL((dev::k_sym_gemm48<EPI, 4>), dim3(grid), dim3(dev::TPB), dev::sg48_lds_bytes(4), stream, Pm, Qm, W.sg_ld,
                               W.sg_nt48, T, Y, ca, cb, cc, dsc, part);
            return;
        }
        if (W.sg_small) {                                   // 32 x 32 tiles: small blocks need the workgroups
            hipLaunchKernelGGL((dev::k_sym_gemm32<EPI>), dim3(grid), dim3(dev::TPB), 0, stream, Pm, Qm, W.sg_ld, 2 * W.nt, T, Y,
                               ca, cb, cc, dsc, part);
            return;
        }
    }
    hipLaunchKernelGGL((dev::k_sym_gemm<EPI, FUSE>), dim3(grid), dim3(dev::TPB), 0, stream, Pm, Qm, W.sg_ld, W.nt, T, Y,
                       ca, cb, cc, dsc, part, W.n, xp_out, xp_old, FUSE ? (const unsigned*)mask_d.p : nullptr,
                       FUSE ? (long long)P.blocks[blk].off : 0LL, FUSE ? respart_d.p + tile_base[blk] : nullptr,
                       FUSE ? rstride : 0);
}

// Tile shape of W's products (W.nt set): 32 x 32 up to the padded side sign_small_tile_max, 48 x 48 where they fit and shorten
// the busiest CU's queue, else 64 x 64; W.sg_npart = workgroups (= `part` slots) of a product of that shape.
inline void Solver::sign_choose_tiles(EigWork& W) {
    const int n = W.n, ld = W.nt * dev::TILE;
    const int small_max = opt.sign_small_tile_max > 0 ? opt.sign_small_tile_max : 3072;   // measured: 32-tiles win up to n ~ 3500
    W.sg_small = ld <= small_max;
    const int nt32 = 2 * W.nt;
    // tile shape by makespan: the busiest of the 256 CUs runs ceil(tiles / 256) tiles of T x T entries each.  n = 1000: 528 tiles of
    // 32 x 32 (3 x 1024) against 231 of 48 x 48 (1 x 2304); n = 800: 325 (2 x 1024) against 153 (2304) -- the 32-tiles stay.  Measured
    // (tools/gpurun_tile48_sizes.sh, ms per projection 32 / 48): 700: 0.44 / 0.44, 800: 0.77 / 0.83, 1000: 1.21 / 1.00, 1200: 1.57 / 2.0,
    // 1500: 2.9 / ~3.6, 2000 (a tie of the rule): 6.6 / 6.4, 2500: 12.9 / 13.2 -- the rule picks the faster one each time.
    // PROXSDP_HIP_SIGN_TILE48 = 0 / 1: never / whenever the tiles fit (measurement)
    W.sg_nt48 = 0;
    const int nb48 = ceil_div(n, dev::SG_T48);
    const char* env = std::getenv("PROXSDP_HIP_SIGN_TILE48");
    const int knob = env != nullptr ? std::atoi(env) : -1;
    if (W.sg_small && knob != 0 && sign_tile48_fits(n, ld)) {
        const int cus = 256;
        const long long c32 = (long long)ceil_div(nt32 * (nt32 + 1) / 2, cus) * 32 * 32;
        const long long c48 = (long long)ceil_div(nb48 * (nb48 + 1) / 2, cus) * 48 * 48;
        if (knob == 1 || c48 <= c32) W.sg_nt48 = nb48;
    }
    W.sg_npart = sym_gemm_grid(W, false);
}

// A = smat(xp_in) in full storage (the padding of A is not written) and sc[0] = 1 / f^2, sc[6] = f = ||A||_F
inline void Solver::sign_unpack(EigWork& W, const double* xp_in, double* A, double* sc) {
    const int ntile = W.nt * (W.nt + 1) / 2;
    hipLaunchKernelGGL(dev::k_unpack_sym, dim3(ntile), dim3(dev::TPB), 0, stream, xp_in, W.n, A, W.nt * dev::TILE,
                       dev::INV_SQRT2, W.sg_part.p);
    hipLaunchKernelGGL(dev::k_sign_scalars, dim3(1), dim3(dev::TPB), 0, stream, (const double*)W.sg_part.p, ntile, 0, sc);
}

// Y0 = A A / f^2 and its Frobenius norm g: s = f sqrt(g) >= ||A||_2   (sc[1], sc[4], sc[8..10])
inline void Solver::sign_scale(EigWork& W, double* sc) {
    sym_gemm<dev::SG_PLAIN, false>(W, W.sgA.p, W.sgA.p, W.sgY.p, nullptr, 0, 0, 0, sc + 0, W.sg_part.p, nullptr, nullptr, -1);
    hipLaunchKernelGGL(dev::k_sign_scalars, dim3(1), dim3(dev::TPB), 0, stream, (const double*)W.sg_part.p, W.sg_npart, 1, sc);
}

// full_eig! without an eigendecomposition: X+ = (X + X sign(X)) / 2, sign by an odd-polynomial
// iteration of fp64 MFMA products (sign_project.hip.hpp).  current_rank = #{lambda > 0} =
// (tr S + tr S^2) / 2 (the reference counts lambda > tol_psd: eigenvalues in (0, tol_psd] are the only
// difference, and the count only feeds Result.final_rank on this path: min_eig = 0 blocks bump_rank).
inline bool Solver::full_eig_by_sign(int idx, const double* xp_in, double* xp_out, bool fuse, bool force) {
    EigWork& W = eig[idx];
    const int n = W.n;
    if (!force) {
        if (opt.full_eig_sign == 0) return false;
        // auto: from side 33 on (below: the batched Jacobi kernel / rocSOLVER are faster), up to the side whose five
        // padded work matrices fit comfortably (side 16384: 10.7 GB; the cap was 4096 until round 4 -- maxG55 / maxG60,
        // sides 5000 / 7000, fell to rocSOLVER's dsyevd at ~0.2 % of the fp64 peak) and while HBM has room for them
        if (opt.full_eig_sign < 0 && (n < 33 || n > 16384)) return false;
        // auto: X+ carries an absolute error of up to ~1e-10 x the spectral scale on this path (l_0 of the
        // iteration): users who ask for tolerances near that floor get the LAPACK-accurate dense eigensolver
        if (opt.full_eig_sign < 0 && std::min({opt.tol_gap, opt.tol_feasibility, opt.tol_primal, opt.tol_dual}) < 1e-8) return false;
    }
    const proxsdp_stats lst0 = W.lst;                        // (a projection that has to be scaled runs twice and counts once)
    const int ld = W.nt * dev::TILE;
    const int grid = sym_gemm_grid(W, true);
    if (W.sg_ld != ld) {
        // first use: the five work matrices must fit -- whoever asks (auto mode, full_eig_sign = 1, or the opt-in
        // psd_sign_engine with force = true: ADVICE r4); no room, or an allocation that fails anyway (several block
        // threads can pass the test together), DECLINES this engine instead of failing the solve
        static std::mutex sign_alloc_mu;
        std::lock_guard<std::mutex> lk(sign_alloc_mu);
        size_t free_b = 0, total_b = 0;
        const size_t need = (size_t)6 * (size_t)ld * (size_t)ld * sizeof(double);
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < need) return false;
        const size_t sz = (size_t)ld * ld;
        try {
            W.sgA.alloc(sz); W.sgX.alloc(sz); W.sgX2.alloc(sz); W.sgY.alloc(sz); W.sgQ.alloc(sz);
        } catch (const std::bad_alloc&) {
            W.sgA.release(); W.sgX.release(); W.sgX2.release(); W.sgY.release(); W.sgQ.release();
            (void)hipGetLastError();
            return false;
        }
        W.sgA.zero(stream);                                  // the padding stays zero: only entries < n are rewritten
        sign_choose_tiles(W);
        // rows / columns [48 nb48, ld) are never written by the 48-tiles and are read by every product's K loop
        // (measured and dropped: walking the tiles in S x S patches per XCD instead of column-major ranges -- half the
        // operand blocks per XCD's L2 -- changes nothing, 0.95 - 0.98 ms per projection either way: the Infinity Cache
        // serves the misses under the 24 loads in flight; eight k-steps per group instead of four: slower, 1.01 ms)
        if (W.sg_nt48 > 0) { W.sgX.zero(stream); W.sgX2.zero(stream); W.sgY.zero(stream); W.sgQ.zero(stream); }
        W.sg_part.alloc(W.sg_npart); W.sg_part2.alloc(W.sg_npart); W.sg_sc.alloc(16); W.sg_host.alloc(16);
        W.sg_sc.zero(stream);
        W.sg_ld = ld;
    }
    const bool prof = opt.profile_symv_every > 0;
    if (prof) begin_full_eig_events(W);
    const bool fz = fuse && use_support;
    double* sc = W.sg_sc.p;
    sign_unpack(W, xp_in, W.sgA.p, sc);
    sign_scale(W, sc);
    double* X = W.sgX.p;
    double* Xn = W.sgX2.p;
    // rows [from, SIGN_STEPS) of the table; `first`: X does not exist yet (the step works on A and Y0)
    auto run_rows = [&](int from, bool first) {
        for (int k = from; k < dev::SIGN_STEPS; ++k) {
            const dev::SignStep& c = dev::SIGN_TABLE[k];
            const bool last = k + 1 == dev::SIGN_STEPS;
            if (first && k == from) {
                sym_gemm<dev::SG_POLY, false>(W, W.sgY.p, W.sgY.p, W.sgQ.p, W.sgY.p, c.a, c.b, c.c, sc + 8, nullptr, nullptr, nullptr, -1);
                sym_gemm<dev::SG_PLAIN, false>(W, W.sgA.p, W.sgQ.p, X, nullptr, 0, 0, 0, sc + 1, nullptr, nullptr, nullptr, -1);
            } else if (last && dev::SIGN_LAST_CUBIC) {
                // Q = (3 I - X X) / 2 straight from the product's epilogue (the Y term is switched off)
                sym_gemm<dev::SG_POLY, false>(W, X, X, W.sgQ.p, X, 1.5, 0.0, -0.5, nullptr, nullptr, nullptr, nullptr, -1);
                sym_gemm<dev::SG_PLAIN, false>(W, X, W.sgQ.p, Xn, nullptr, 0, 0, 0, nullptr, W.sg_part2.p, nullptr, nullptr, -1);
                std::swap(X, Xn);
            } else {
                sym_gemm<dev::SG_PLAIN, false>(W, X, X, W.sgY.p, nullptr, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, -1);
                sym_gemm<dev::SG_POLY, false>(W, W.sgY.p, W.sgY.p, W.sgQ.p, W.sgY.p, c.a, c.b, c.c, nullptr, nullptr, nullptr, nullptr, -1);
                sym_gemm<dev::SG_PLAIN, false>(W, X, W.sgQ.p, Xn, nullptr, 0, 0, 0, nullptr, last ? W.sg_part2.p : nullptr,
                                               nullptr, nullptr, -1);
                std::swap(X, Xn);
            }
        }
    };
    // SHORTENED SCHEDULE.  The table is laid out for |eigenvalues| down to 1e-10 s; the matrices a solve projects rarely
    // come closer to singular than 1e-5 s (measured on the SDPLIB iterates: 1e-5 .. 1e-3).  So the iteration STARTS AT ROW
    // j > 0 (the rows from l_j on: every |eigenvalue| >= l_j s converges exactly as before: to 1 - 1e-13 after the last,
    // cubic, row) and the result is TESTED: with t_i the eigenvalues of the computed S,
    // ||S||_F^2 - ||S S||_F^2 = sum t_i^2 (1 - t_i^2) vanishes iff every t_i is in {0, +-1}; an eigenvalue that started
    // below l_j has been amplified by gain_j (the product of the rows' slopes at 0) and shows up as t^2 unless it started
    // below sqrt(tau) / gain_j <= 1e-10 s -- the size of eigenvalue the full table does not resolve either.  tau = 4e-13 n:
    // the converged eigenvalues contribute <= 2e-13 each (measured on SDPLIB iterates: the statistic stays below 6e-11 at
    // n = 501 / 1000 when it passes and above 1e-8 when it fails).  A failed test continues with the rows from
    // l_r <= 1e-10 gain_j on: same guarantee as the full table, 63 - 64 products instead of 57.
    auto launch_final = [&]() {
        if (fz) sym_gemm<dev::SG_FINAL, true>(W, W.sgA.p, X, nullptr, nullptr, 0, 0, 0, nullptr, W.sg_part.p, xp_out, xp_in, idx);
        else sym_gemm<dev::SG_FINAL, false>(W, W.sgA.p, X, nullptr, nullptr, 0, 0, 0, nullptr, W.sg_part.p, xp_out, nullptr, -1);
        if (prof) { PX_HIP(hipEventRecord(W.fe[1], stream)); PX_HIP(hipEventRecord(W.fe[2], stream)); W.fe_pending = true; }
    };
    static const dev::SignSchedule sched;
    const int row_opt = opt.sign_start_row;
    const double tau = 4e-13 * (double)n;
    const int jmax = sched.max_start_row(tau);
    // auto: per block, start at row 8 (the iterates of the SDPLIB solves fail its test once in 70 .. 400 projections);
    // a failure moves the next 8 projections two rows down (an eigenvalue crossing zero lingers for a few iterations),
    // a second failure soon after lowers the block's row for good (back up one row per 64 clean projections);
    // at row 0 (no test) the shortened schedule is tried again every 64 projections
    const int jtop = std::min(8, jmax);
    if (W.sg_row < 0) W.sg_row = jtop;
    if (row_opt < 0 && W.sg_row == 0 && jtop > 0 && ++W.sg_idle >= 64) { W.sg_row = std::min(6, jtop); W.sg_idle = 0; W.sg_ok = 16; }
    int j0 = row_opt < 0 ? (W.sg_hold > 0 ? std::max(0, W.sg_row - 2) : W.sg_row) : row_opt;
    j0 = std::max(0, std::min(j0, jmax));
    if (row_opt < 0 && j0 == 0 && W.sg_hold > 0) --W.sg_hold;          // (a hold at row 0 runs the full table, untested)
    bool resolved = false;
    run_rows(j0, true);
    if (j0 > 0) {
        // the test: ||S S||_F^2 needs one more product (its result is not used otherwise)
        sym_gemm<dev::SG_PLAIN, false>(W, X, X, W.sgY.p, nullptr, 0, 0, 0, nullptr, W.sg_part.p, nullptr, nullptr, -1);
        hipLaunchKernelGGL(dev::k_sign_check, dim3(3), dim3(dev::TPB), 0, stream, (const double*)W.sg_part2.p,
                           (const double*)W.sg_part.p, W.sg_npart, (const double*)X, ld, n, sc);
        PX_HIP(hipMemcpyAsync(W.sg_host.p, sc, 16 * sizeof(double), hipMemcpyDeviceToHost, stream));
        // the final product is enqueued BEFORE the host looks at the test (out of place only: a redo must find its input
        // intact): the GPU runs it while the host reads the three scalars and goes back to enqueueing the iteration
        const bool ahead = (const double*)xp_out != xp_in;
        if (ahead) {
            W.sg_ev.create(hipEventDisableTiming);
            PX_HIP(hipEventRecord(W.sg_ev, stream));
            launch_final();
            wait_event(W.sg_ev);
        } else {
            wait_stream();
        }
        const double m2 = W.sg_host.p[7], m4 = W.sg_host.p[11];
        resolved = std::isfinite(m2) && std::isfinite(m4) && std::fabs(m2 - m4) <= tau;
        if (debug) std::fprintf(stderr, "[dbg] sign short: block %d row %d m2 - m4 %.3e tau %.3e %s\n", idx, j0, m2 - m4, tau, resolved ? "pass" : "FAIL");
        if (resolved) {
            W.lst.sign_short_pass++;
            if (row_opt < 0) {
                if (W.sg_hold > 0) --W.sg_hold;
                if (++W.sg_ok >= 64 + 16 && W.sg_row < jtop) { W.sg_row++; W.sg_ok = 16; }
            }
            if (!ahead) launch_final();
        } else {
            W.lst.sign_short_fail++;
            if (row_opt < 0) {
                if (W.sg_ok < 16) W.sg_row = std::max(0, W.sg_row - 1);
                W.sg_hold = 8; W.sg_ok = 0;
            }
            run_rows(sched.fallback_row(j0), false);
        }
    }
    if (!resolved) {
        launch_final();
        hipLaunchKernelGGL(dev::k_sign_scalars, dim3(1), dim3(dev::TPB), 0, stream, (const double*)W.sg_part2.p, W.sg_npart, 3, sc);
        hipLaunchKernelGGL(dev::k_sign_scalars, dim3(1), dim3(dev::TPB), 0, stream, (const double*)W.sg_part.p, grid, 2, sc);
        PX_HIP(hipMemcpyAsync(W.sg_host.p, sc, 16 * sizeof(double), hipMemcpyDeviceToHost, stream));
        wait_stream();
    }
    // f = |A|_F came out 0 or non-finite: the zero matrix, non-finite input, or squares outside the fp64 range
    if (const double f = W.sg_host.p[6]; (!(f > 0.0) || !std::isfinite(f)) && xp_in != W.sg_in.p) {   // (not the scaled pass itself)
        if (sign_project_rescaled(idx, xp_out, fz, force, lst0)) return true;
    }
    const double tr = W.sg_host.p[5], fro2 = W.sg_host.p[7];
    if (!std::isfinite(tr) || !std::isfinite(fro2)) throw HipError("sign-function projection produced non-finite values");
    const int npos = (int)std::llround(0.5 * (tr + fro2));
    if (!force) { W.lst.full_eigs++; W.lst.full_eigs_sign++; }
    current_rank[idx] = std::max(0, std::min(npos, n));
    min_eig[idx] = 0.0;                                      // prox_operators.jl:114
    W.xprev.last_npos = current_rank[idx];
    return true;
}

// The sign-function projection of a block whose |A|_F^2 left the fp64 range (largest |entry| below ~1e-162: the sum of
// squares underflows, at 2^-600 to an exact 0, and the iteration returned A / 2; or above ~1e+154: it overflows).  The
// projection is positively homogeneous: the block is taken again from its unpacked copy sgA, scaled by an exact power of two
// to a largest |entry| in [1/2, 1), projected, and the result scaled back.  False: nothing to do -- the zero matrix (what was
// computed stands) or non-finite input (the caller raises the error).  `before`: the block's counters before the first pass.
inline bool Solver::sign_project_rescaled(int idx, double* xp_out, bool fused, bool force, const proxsdp_stats& before) {
    EigWork& W = eig[idx];
    const int ld = W.nt * dev::TILE;
    if (W.sg_cmp.n < 2) W.sg_cmp.alloc(2);
    W.sg_cmp.zero(stream);
    const long long sz = (long long)ld * ld;
    hipLaunchKernelGGL(dev::k_maxdiff, dim3(grid_for(sz)), dim3(dev::TPB), 0, stream, (const double*)W.sgA.p, (const double*)W.sgA.p, sz, W.sg_cmp.p);
    double h[2] = {0.0, 0.0};
    W.sg_cmp.download(h, 2, stream);
    PX_HIP(hipStreamSynchronize(stream));
    const double amax = h[1];
    if (amax == 0.0 || !std::isfinite(amax)) return false;
    if (fused) throw HipError("sign-function projection: a block outside the fp64 range of its squares on the support path");
    int e = 0;
    (void)std::frexp(amax, &e);
    if (W.sg_in.n < (size_t)W.N) W.sg_in.alloc(W.N);
    hipLaunchKernelGGL(dev::k_pack_ldexp, dim3(grid_for(W.N)), dim3(dev::TPB), 0, stream, (const double*)W.sgA.p, ld, (long long)W.N, -e, W.sg_in.p);
    W.lst = before;                                          // (the pass that ran on the unscaled block is not counted)
    if (!full_eig_by_sign(idx, W.sg_in.p, xp_out, false, force)) return false;
    hipLaunchKernelGGL(dev::k_ldexp, dim3(grid_for(W.N)), dim3(dev::TPB), 0, stream, xp_out, (long long)W.N, e);
    return true;
}

// ---- concurrent block projections (the job pool itself: block_pool.hpp)
// run job(idx) for every listed block: concurrently on the blocks' streams when the pool is
// up, otherwise in sequence on the solver's stream.  Returns after all host work is done and
// the solver's stream has been made to wait for the block streams.
inline void Solver::run_blocks(const std::vector<int>& blocks, const std::function<void(int)>& job) {
    bool have_streams = true;
    for (int idx : blocks) have_streams = have_streams && eig[idx].stream != nullptr;
    if (!parallel_blocks() || blocks.size() < 2 || !have_streams) {
        for (int idx : blocks) job(idx);
        merge_block_stats();
        return;
    }
    PX_HIP(hipEventRecord(ev_main, stream.main));
    // on a worker: the block's stream is the thread's stream, behind the main stream's work so far
    block_pool->run(blocks, [this, &job](int idx) {
        struct TlReset { ~TlReset() { StreamRef::tl = nullptr; } } reset;
        StreamRef::tl = eig[idx].stream;
        PX_HIP(hipStreamWaitEvent(eig[idx].stream, ev_main, 0));
        job(idx);
        PX_HIP(hipEventRecord(eig[idx].done, eig[idx].stream));
    });
    for (int idx : blocks) PX_HIP(hipStreamWaitEvent(stream.main, eig[idx].done, 0));
    merge_block_stats();
}
inline void Solver::merge_block_stats() {
    // per-block counters (filled on the blocks' own threads) into the solver's; one line per field
#define PX_MERGE(f) st.f += a.f
    for (EigWork& W : eig) {
        proxsdp_stats& a = W.lst;
        PX_MERGE(lanczos_matvecs); PX_MERGE(lanczos_restarts); PX_MERGE(lanczos_calls);
        PX_MERGE(full_eigs); PX_MERGE(krylov_fallbacks);
        PX_MERGE(symv_launches); PX_MERGE(symv_bytes);
        PX_MERGE(symv_profiled); PX_MERGE(symv_profiled_ms);
        PX_MERGE(orth_profiled); PX_MERGE(orth_profiled_ms);
        PX_MERGE(full_eig_solver_ms); PX_MERGE(full_eig_recon_ms);
        PX_MERGE(full_eigs_lanczos); PX_MERGE(full_eigs_lanczos_checks); PX_MERGE(full_eigs_lanczos_mismatches);
        PX_MERGE(full_eigs_lanczos_certified); PX_MERGE(full_eigs_lanczos_cert_failed); PX_MERGE(cert_matvecs);
        PX_MERGE(dense_truncated_projections); PX_MERGE(wide_krylov_projections);
        PX_MERGE(full_eigs_sign); PX_MERGE(sign_products); PX_MERGE(sign_short_pass); PX_MERGE(sign_short_fail);
        PX_MERGE(sign_engine_projections); PX_MERGE(sign_engine_rejected);
        PX_MERGE(sign_engine_checks); PX_MERGE(sign_engine_mismatches);
        PX_MERGE(batched_block_steps);
        PX_MERGE(host_eigs); PX_MERGE(host_eig_time); PX_MERGE(host_eig_merges); PX_MERGE(host_eig_overlap_time);
        PX_MERGE(reserved_s[PROXSDP_STATS_DEVICE_EIG_MERGES]); PX_MERGE(reserved_s[PROXSDP_STATS_DEVICE_EIG_MERGE_FALLBACKS]);
        PX_MERGE(reserved_s[PROXSDP_STATS_FOP_OWNER_STEPS]);
        PX_MERGE(warm_starts); PX_MERGE(device_eigs); PX_MERGE(mfma_reconstructions);
        PX_MERGE(cycle_launches); PX_MERGE(cycle_steps); PX_MERGE(cycle_ms);
        PX_MERGE(fop_projections);
        a = proxsdp_stats{};
        lz_matvec_iter += W.mv_iter; recon_r_iter += W.recon_r;
        W.mv_iter = 0; W.recon_r = 0;
    }
#undef PX_MERGE
}

}  // namespace proxsdp
