// C ABI of libproxsdp_hip.so (include/proxsdp_hip.h).  Nothing unwinds across
// this boundary: every entry point catches, records the message in a
// thread-local buffer and returns a negative PROXSDP_E_* code.  There is no CPU
// fallback: without a HIP device the compute entry points fail with PROXSDP_E_HIP.
#include <functional>
#include <memory>
#include <new>
#include <string>

#include "lanczos.hip.hpp"
#include "pdhg_loop.hip.hpp"
#include "projection.hip.hpp"
#include "exit_device.hip.hpp"
#include "test_hooks.hip.hpp"
#include "shard_split.hpp"
#include "model.hip.hpp"

namespace {
thread_local std::string g_last_error;

template <typename F>
int guarded(F&& f) {
    try {
        g_last_error.clear();
        return f();
    } catch (const std::bad_alloc&) {
        g_last_error = "out of memory";
        return PROXSDP_E_NOMEM;
    } catch (const proxsdp::HipError& e) {
        g_last_error = e.what();
        return PROXSDP_E_HIP;
    } catch (const std::invalid_argument& e) {
        g_last_error = e.what();
        return PROXSDP_E_INVALID;
    } catch (const std::domain_error& e) {
        g_last_error = e.what();
        return PROXSDP_E_UNSUPP;
    } catch (const std::exception& e) {
        g_last_error = e.what();
        return PROXSDP_E_INTERNAL;
    } catch (...) {
        g_last_error = "unknown error";
        return PROXSDP_E_INTERNAL;
    }
}

// the caller's options (NULL: the defaults), refused when they are not this ABI's struct
proxsdp_options checked_options(const proxsdp_options* o) {
    proxsdp_options d;
    proxsdp::default_options(&d);
    if (o) {
        if (o->struct_size != (int64_t)sizeof(proxsdp_options))
            throw std::invalid_argument("proxsdp_options.struct_size mismatch (ABI version?)");
        d = *o;
    }
    return d;
}

// engine-only solver for the kernel-level entry points: one block of side n
struct Engine {
    proxsdp_result dummy{};
    proxsdp::Solver S;
    Engine(const proxsdp_options* opt, int64_t n, int max_nev)
        : S(checked_options(opt), dummy) {
        if (n < 1 || n > 46340) throw std::invalid_argument("n out of range");
        S.setup_device();
        S.eig.resize(1);
        S.alloc_eigwork(S.eig[0], (int)n, std::min<int>(std::max(max_nev, 2), (int)n));
    }
    void set_resid(const double* resid) {
        proxsdp::EigWork& W = S.eig[0];
        S.lanczos_start_vector(W, resid);
        W.resid.upload(W.resid_host.data(), W.npad, S.stream);
        PX_HIP(hipStreamSynchronize(S.stream));
    }
};
}  // namespace

extern "C" {

int proxsdp_hip_abi_version(void) { return PROXSDP_HIP_ABI_VERSION; }

void proxsdp_hip_default_options(proxsdp_options* opt) {
    if (opt) proxsdp::default_options(opt);
}

int proxsdp_hip_set_option(proxsdp_options* opt, const char* name, double value) {
    if (!opt || !name) { g_last_error = "NULL argument"; return PROXSDP_E_INVALID; }
    int rc = proxsdp::set_option(opt, name, value);
    if (rc != 0) g_last_error = std::string("No parameter matching ") + name;
    return rc;
}

int proxsdp_hip_get_option(const proxsdp_options* opt, const char* name, double* value) {
    if (!opt || !name || !value) { g_last_error = "NULL argument"; return PROXSDP_E_INVALID; }
    int rc = proxsdp::get_option(opt, name, value);
    if (rc != 0) g_last_error = std::string("No parameter matching ") + name;
    return rc;
}

// ---- RCCL communicator helpers (block-sharded solve, native collectives: proxsdp_problem.nccl_comm)
int proxsdp_hip_rccl_available(void) {
    return guarded([&]() -> int { return proxsdp::Rccl::get().ok() ? 1 : 0; });
}
int proxsdp_hip_rccl_unique_id(void* id128) {
    return guarded([&]() -> int {
        if (!id128) throw std::invalid_argument("NULL id buffer");
        proxsdp::Rccl& rc = proxsdp::Rccl::get();
        rc.require();
        ncclUniqueId id;
        rc.check(rc.GetUniqueId(&id), "ncclGetUniqueId");
        std::memcpy(id128, id.internal, NCCL_UNIQUE_ID_BYTES);
        return 0;
    });
}
int proxsdp_hip_rccl_comm_init(int32_t nranks, const void* id128, int32_t rank, int32_t device_id, void** comm) {
    return guarded([&]() -> int {
        if (!id128 || !comm || nranks < 1 || rank < 0 || rank >= nranks) throw std::invalid_argument("invalid argument");
        proxsdp::Rccl& rc = proxsdp::Rccl::get();
        rc.require();
        if (hipSetDevice(device_id) != hipSuccess) throw proxsdp::HipError("hipSetDevice failed");
        ncclUniqueId id;
        std::memcpy(id.internal, id128, NCCL_UNIQUE_ID_BYTES);
        ncclComm_t c = nullptr;
        rc.check(rc.CommInitRank(&c, nranks, id, rank), "ncclCommInitRank");
        *comm = c;
        return 0;
    });
}
int proxsdp_hip_rccl_comm_destroy(void* comm) {
    return guarded([&]() -> int {
        if (!comm) return 0;
        proxsdp::Rccl& rc = proxsdp::Rccl::get();
        rc.require();
        rc.check(rc.CommDestroy(static_cast<ncclComm_t>(comm)), "ncclCommDestroy");
        return 0;
    });
}

const char* proxsdp_hip_last_error(void) { return g_last_error.c_str(); }

int proxsdp_hip_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        g_last_error = std::string("hipGetDeviceCount: ") + hipGetErrorString(e);
        return PROXSDP_E_HIP;
    }
    return n;
}

int proxsdp_hip_solve(const proxsdp_problem* prob, const proxsdp_options* opt, proxsdp_result* res) {
    return proxsdp_hip_solve_ex(prob, opt, res, nullptr, nullptr);
}

// every solve entry point: the result before the solve (begin_solve: with the options; a trace the caller gave no buffer
// for is not written)
static void reset_result(proxsdp_result* res) {
    res->status = PROXSDP_STATUS_NOT_CALLED;
    res->trace_rows = 0; res->result_count = 0; res->certificate_found = 0;
    res->status_string[0] = 0;
}
static proxsdp_options begin_solve(const proxsdp_options* opt, proxsdp_result* res) {
    proxsdp_options o = checked_options(opt);
    reset_result(res);
    if (o.trace_capacity > 0 && !res->trace) o.trace_capacity = 0;
    return o;
}

// the solve behind every one-call entry (req: validated by the caller through check_request, or empty)
static int solve_impl(const proxsdp_problem* prob, const proxsdp_options* opt, proxsdp_result* res,
                      const proxsdp::SolveRequest& req) {
    bool comm_aborted = false;
    const int rc = guarded([&]() -> int {
        if (!prob || !res) throw std::invalid_argument("NULL problem or result");
        const proxsdp_options o = begin_solve(opt, res);
        proxsdp::Solver S(*prob, o, *res);
        S.req = req;
        try {
            S.run();
        } catch (...) {
            // this rank leaves the solve: the transport stops its own pending collectives so that its stream drains (RCCL:
            // ncclCommAbort, only when a collective of this solve was enqueued; the peers' waits are bounded and fail the
            // same way).  An aborted communicator is released: the caller learns it through PROXSDP_E_COMM_ABORTED.
            comm_aborted = S.comm && S.comm->abort_if_pending();
            throw;
        }
        return 0;
    });
    if (rc != 0 && comm_aborted) {
        g_last_error += " [the RCCL communicator was aborted (ncclCommAbort): it is released, do not destroy or reuse it]";
        return PROXSDP_E_COMM_ABORTED;
    }
    return rc;
}

int proxsdp_hip_solve_ex(const proxsdp_problem* prob, const proxsdp_options* opt, proxsdp_result* res,
                         const proxsdp_state* resume, proxsdp_state* capture) {
    proxsdp::SolveRequest req;
    req.resume_state = resume; req.capture_state = capture;
    return solve_impl(prob, opt, res, req);
}

// ---- what a request carries is checked here, on the host, before a solver -- and with it the device -- exists
static bool is_shard(const proxsdp_problem* prob) {
    return prob->reduce_fn || prob->reduce_vec_fn || prob->nccl_comm || prob->n_coupling != 0;
}

// the factors of the PSD solution (proxsdp_psd_factors; Solver::extract_factors)
static void check_factors_arg(const proxsdp_problem* prob, const proxsdp_result* res, const proxsdp_psd_factors* fac) {
        if (!prob || !res || !fac) throw std::invalid_argument("NULL problem, result or factors");
        if (fac->struct_size != (int64_t)sizeof(proxsdp_psd_factors))
            throw std::invalid_argument("proxsdp_psd_factors.struct_size mismatch");
        if (prob->n_psd < 0 || fac->n_psd != prob->n_psd) throw std::invalid_argument("proxsdp_psd_factors.n_psd != problem.n_psd");
        if (prob->n_psd > 0 && !prob->psd_ptr) throw std::invalid_argument("psd_ptr/psd_idx is NULL");
        if (!fac->cap || !fac->vec_ptr || !fac->val_ptr || !fac->rank || !fac->rank_found || !fac->source || !fac->resid ||
            !fac->xnorm)
            throw std::invalid_argument("proxsdp_psd_factors: NULL array");
        bool any = false;
        for (int64_t k = 0; k < fac->n_psd; ++k) {
            const int64_t len = prob->psd_ptr[k + 1] - prob->psd_ptr[k];
            if (len <= 0) throw std::invalid_argument("empty PSD cone");
            const int64_t side = proxsdp::psd_side(len);
            if (side < 0) throw std::invalid_argument("PSD cone length is not triangular");
            const int64_t cap = fac->cap[k];
            if (cap < 0) throw std::invalid_argument("proxsdp_psd_factors.cap is negative");
            any = any || cap > 0;
            const int64_t want = std::min(cap, side);           // (a block has at most `side` pairs)
            if (fac->vec_ptr[k] < 0 || fac->val_ptr[k] < 0 || fac->vec_ptr[k + 1] - fac->vec_ptr[k] < side * want ||
                fac->val_ptr[k + 1] - fac->val_ptr[k] < want)
                throw std::invalid_argument("proxsdp_psd_factors: vec_ptr / val_ptr span too small for cap");
        }
        if (any && (!fac->vectors || !fac->values)) throw std::invalid_argument("proxsdp_psd_factors: NULL vectors / values");
}

// the warm start (proxsdp_start)
static void check_start_arg(const proxsdp_problem* prob, const proxsdp_start* st) {
    if (!prob) throw std::invalid_argument("NULL problem");
    if (!st) return;
    if (st->struct_size != (int64_t)sizeof(proxsdp_start)) throw std::invalid_argument("proxsdp_start.struct_size mismatch");
    if (prob->n < 0 || prob->p < 0 || prob->m < 0 || prob->n_psd < 0) throw std::invalid_argument("negative dimension");
    if (st->n_psd != 0 && st->n_psd != prob->n_psd) throw std::invalid_argument("proxsdp_start.n_psd is neither 0 nor problem.n_psd");
    if (prob->n_psd > 0 && !prob->psd_ptr) throw std::invalid_argument("psd_ptr/psd_idx is NULL");
    if (st->n_psd != 0 && (!st->rank || !st->vec_ptr || !st->val_ptr)) throw std::invalid_argument("proxsdp_start: NULL rank / vec_ptr / val_ptr");
    if (!(st->primal_step >= 0.0) || !std::isfinite(st->primal_step) || !(st->beta >= 0.0) || !std::isfinite(st->beta))
        throw std::invalid_argument("proxsdp_start: primal_step and beta must be finite and >= 0");
    auto all_finite = [](const double* v, int64_t len) {
        for (int64_t i = 0; i < len; ++i) if (!std::isfinite(v[i])) return false;
        return true;
    };
    if (st->target_rank)
        for (int64_t k = 0; k < prob->n_psd; ++k)
            if (st->target_rank[k] < 0) throw std::invalid_argument("proxsdp_start.target_rank is negative");
    bool any = false;
    for (int64_t k = 0; k < st->n_psd; ++k) {
        const int64_t len = prob->psd_ptr[k + 1] - prob->psd_ptr[k];
        if (len <= 0) throw std::invalid_argument("empty PSD cone");
        const int64_t side = proxsdp::psd_side(len);
        if (side < 0) throw std::invalid_argument("PSD cone length is not triangular");
        const int64_t r = st->rank[k];
        if (r < -1 || r > side) throw std::invalid_argument("proxsdp_start.rank must be -1 .. side");
        if (r <= 0) continue;
        any = true;
        if (st->vec_ptr[k] < 0 || st->val_ptr[k] < 0 || st->vec_ptr[k + 1] - st->vec_ptr[k] < side * r ||
            st->val_ptr[k + 1] - st->val_ptr[k] < r)
            throw std::invalid_argument("proxsdp_start: vec_ptr / val_ptr span too small for rank");
    }
    if (any && (!st->vectors || !st->values)) throw std::invalid_argument("proxsdp_start: NULL vectors / values");
    for (int64_t k = 0; k < st->n_psd; ++k) {
        const int64_t r = st->rank[k];
        if (r <= 0) continue;
        const int64_t side = proxsdp::psd_side(prob->psd_ptr[k + 1] - prob->psd_ptr[k]);   // (triangular: checked above)
        if (!all_finite(st->vectors + st->vec_ptr[k], side * r) || !all_finite(st->values + st->val_ptr[k], r))
            throw std::invalid_argument("proxsdp_start: non-finite factor entry");
        for (int64_t j = 0; j < r; ++j)
            if (!(st->values[st->val_ptr[k] + j] > 0.0)) throw std::invalid_argument("proxsdp_start.values must be > 0");
    }
    if ((st->primal && !all_finite(st->primal, prob->n)) || (st->dual_eq && !all_finite(st->dual_eq, prob->p)) ||
        (st->dual_in && !all_finite(st->dual_in, prob->m)))
        throw std::invalid_argument("proxsdp_start: non-finite entry in primal / dual_eq / dual_in");
    if (is_shard(prob)) throw std::domain_error("a warm start does not serve a shard of a block-sharded solve");
}

// solution vectors on the device (proxsdp_device_vectors): all but that the start vectors hold finite numbers
// (Solver::check_start_dev, a device reduction after set-up)
static void check_device_vectors(const proxsdp_device_vectors* v, int32_t device_id, const char* what) {
    if (!v) return;
    if (v->struct_size != (int64_t)sizeof(proxsdp_device_vectors))
        throw std::invalid_argument(std::string("proxsdp_device_vectors (") + what + "): struct_size mismatch");
    if (v->device_id != device_id)
        throw std::invalid_argument(std::string("proxsdp_device_vectors (") + what + "): device_id is not options.device_id");
}

// One request against the problem it is for (shape: the problem, or a handle's dimensions and cones): each entry sets the
// fields it accepts, so one damaged argument is refused with the same code and message at every entry that takes it.
// device_id: the options' (read only when device vectors are given); entry: named when the problem is a shard.
static void check_request(const proxsdp_problem* shape, const proxsdp_result* res, int32_t device_id,
                          const proxsdp::SolveRequest& q, const char* entry) {
    check_start_arg(shape, q.start);
    if (q.factors_out) check_factors_arg(shape, res, q.factors_out);
    check_device_vectors(q.start_dev, device_id, "start");
    check_device_vectors(q.out_dev, device_id, "out");
    if (const proxsdp_device_vectors* d = q.start_dev) {
        if (d->dual_cone || d->slack_eq || d->slack_in)
            throw std::invalid_argument("proxsdp_device_vectors (start): dual_cone, slack_eq and slack_in must be NULL");
        if (q.start && ((q.start->primal && d->primal) || (q.start->dual_eq && d->dual_eq) || (q.start->dual_in && d->dual_in)))
            throw std::invalid_argument("a start vector is given both on the host (proxsdp_start) and on the device");
        if (shape->n < 0 || shape->p < 0 || shape->m < 0) throw std::invalid_argument("negative dimension");
    }
    if (is_shard(shape)) throw std::domain_error(std::string(entry) + " does not serve a shard of a block-sharded solve");
}

int proxsdp_hip_solve_factored(const proxsdp_problem* prob, const proxsdp_options* opt, proxsdp_result* res,
                               proxsdp_psd_factors* fac) {
    proxsdp::SolveRequest req;
    req.factors_out = fac;
    const int rc = guarded([&]() -> int {
        if (!prob || !res || !fac) throw std::invalid_argument("NULL problem, result or factors");
        check_request(prob, res, 0, req, "proxsdp_hip_solve_factored");
        return 0;
    });
    return rc != 0 ? rc : solve_impl(prob, opt, res, req);
}

int proxsdp_hip_solve_from(const proxsdp_problem* prob, const proxsdp_options* opt, proxsdp_result* res,
                           const proxsdp_start* start, proxsdp_psd_factors* fac) {
    proxsdp::SolveRequest req;
    req.start = start; req.factors_out = fac;
    const int rc = guarded([&]() -> int {
        if (!prob || !res) throw std::invalid_argument("NULL problem or result");
        check_request(prob, res, 0, req, "proxsdp_hip_solve_from");
        return 0;
    });
    return rc != 0 ? rc : solve_impl(prob, opt, res, req);
}

int proxsdp_hip_solve_device(const proxsdp_problem* prob, const proxsdp_options* opt, proxsdp_result* res,
                             const proxsdp_start* start, const proxsdp_device_vectors* start_dev,
                             proxsdp_psd_factors* fac, proxsdp_device_vectors* out_dev) {
    proxsdp::SolveRequest req;
    req.start = start; req.start_dev = start_dev; req.factors_out = fac; req.out_dev = out_dev;
    req.device_exit = true;
    const int rc = guarded([&]() -> int {
        if (!prob || !res) throw std::invalid_argument("NULL problem or result");
        check_request(prob, res, checked_options(opt).device_id, req, "proxsdp_hip_solve_device");
        return 0;
    });
    return rc != 0 ? rc : solve_impl(prob, opt, res, req);
}

// ---- a model that stays set up on the device (model.hip.hpp): what is decided on the host is decided here, before a device call

int proxsdp_hip_model_create(const proxsdp_problem* prob, const proxsdp_options* opt, proxsdp_model** out) {
    return guarded([&]() -> int {
        if (!prob || !out) throw std::invalid_argument("NULL problem or handle");
        *out = nullptr;
        const proxsdp_options o = checked_options(opt);
        if (is_shard(prob)) throw std::domain_error("proxsdp_hip_model_create does not serve a shard of a block-sharded solve");
        if (prob->M_dense != nullptr)
            throw std::domain_error("proxsdp_hip_model_create does not serve M_dense: the matrix is borrowed, a handle would outlive the loan");
        if (o.rocsolver_warmup != 0) throw std::domain_error("proxsdp_hip_model_create does not serve rocsolver_warmup");
        *out = new proxsdp_model(*prob, o);
        return 0;
    });
}

int proxsdp_hip_model_destroy(proxsdp_model* mdl) {
    return guarded([&]() -> int {
        if (!mdl) return 0;
        (void)hipSetDevice(mdl->opt0.device_id);
        mdl->drain();
        delete mdl;
        return 0;
    });
}

int proxsdp_hip_model_info(const proxsdp_model* mdl, proxsdp_model_info* info) {
    return guarded([&]() -> int {
        if (!info) throw std::invalid_argument("NULL info");
        proxsdp::check_struct_size(info, "proxsdp_model_info");
        if (!mdl) throw std::invalid_argument("NULL handle");
        mdl->info(*info);
        return 0;
    });
}

int proxsdp_hip_model_dump(proxsdp_model* mdl, proxsdp_model_dump* out) {
    return guarded([&]() -> int {
        if (!out) throw std::invalid_argument("NULL dump");
        proxsdp::check_struct_size(out, "proxsdp_model_dump");
        if (!mdl) throw std::invalid_argument("NULL handle");
        mdl->dump(*out);
        return 0;
    });
}

int proxsdp_hip_model_update(proxsdp_model* mdl, const proxsdp_model_data* upd) {
    return guarded([&]() -> int {
        if (!upd) throw std::invalid_argument("NULL data");
        proxsdp::check_struct_size(upd, "proxsdp_model_data");
        if (upd->on_device != 0 && upd->on_device != 1) throw std::invalid_argument("proxsdp_model_data.on_device must be 0 or 1");
        if (!upd->c && !upd->b && !upd->h && !upd->A_nzval && !upd->G_nzval) throw std::invalid_argument("proxsdp_model_data: every pointer is NULL");
        if (!mdl) throw std::invalid_argument("NULL handle");
        const proxsdp::Prep& P = mdl->S->P;
        if (P.equilibrated) throw std::domain_error("proxsdp_hip_model_update does not serve an equilibrated model: E and D depend on the values");
        if ((upd->A_nzval || upd->G_nzval) && !mdl->opt0.approx_norm)
            throw std::domain_error("proxsdp_hip_model_update does not serve A_nzval / G_nzval with approx_norm = 0: sigma_max depends on them");
        if (upd->on_device == 0) {
            const double* src[5] = {upd->c, upd->b, upd->h, upd->A_nzval, upd->G_nzval};
            const int64_t len[5] = {P.n, P.p, P.m, P.nnzA, P.nnz - P.nnzA};
            const char* name[5] = {"c", "b", "h", "A_nzval", "G_nzval"};
            for (int q = 0; q < 5; ++q)
                for (int64_t i = 0; src[q] && i < len[q]; ++i)
                    if (!std::isfinite(src[q][i])) throw std::invalid_argument(std::string("proxsdp_model_data: non-finite entry in ") + name[q]);
        }
        mdl->update(*upd);
        return 0;
    });
}

int proxsdp_hip_model_rows(proxsdp_model* mdl, proxsdp_model_rows* ch) {
    return guarded([&]() -> int {
        proxsdp::check_rows_struct(ch);
        if (!mdl) throw std::invalid_argument("NULL handle");
        if (mdl->S->P.equilibrated) throw std::domain_error("proxsdp_hip_model_rows does not serve an equilibrated model: E and D depend on the rows");
        if (!mdl->opt0.approx_norm) throw std::domain_error("proxsdp_hip_model_rows does not serve approx_norm = 0: sigma_max depends on the rows");
        mdl->change_rows(*ch);
        return 0;
    });
}

int proxsdp_hip_model_triangles(proxsdp_model* mdl, proxsdp_triangle_cuts* tc) {
    return guarded([&]() -> int {
        proxsdp::check_triangle_struct(tc, true);
        if (!mdl) throw std::invalid_argument("NULL handle");
        if (mdl->cone(tc->cone, "proxsdp_triangle_cuts").n < 3)
            throw std::invalid_argument("proxsdp_triangle_cuts: cone " + std::to_string(tc->cone) + " has side < 3");
        mdl->triangles(*tc);
        return 0;
    });
}

int proxsdp_host_triangle_cuts(const double* X, int64_t side, const int64_t* cone_idx, int32_t index_base, proxsdp_triangle_cuts* tc) {
    return guarded([&]() -> int {
        proxsdp::check_triangle_struct(tc, false);
        if (!X) throw std::invalid_argument("proxsdp_host_triangle_cuts: X is NULL");
        if (side < 3 || side > 46340) throw std::invalid_argument("proxsdp_host_triangle_cuts: side must be 3 .. 46340");
        if (index_base != 0 && index_base != 1) throw std::invalid_argument("index_base must be 0 or 1");
        proxsdp::host_triangle_cuts(X, side, cone_idx, index_base, *tc);
        return 0;
    });
}

int proxsdp_hip_model_cliques(proxsdp_model* mdl, proxsdp_clique_cuts* q) {
    return guarded([&]() -> int {
        proxsdp::check_clique_struct(q, true);
        if (!mdl) throw std::invalid_argument("NULL handle");
        const int64_t side = mdl->cone(q->cone, "proxsdp_clique_cuts").n;
        if (side < q->base_size + 2)
            throw std::invalid_argument("proxsdp_clique_cuts: cone " + std::to_string(q->cone) + " has side < base_size + 2");
        proxsdp::check_clique_bases(*q, side);
        mdl->cliques(*q);
        return 0;
    });
}

int proxsdp_host_clique_cuts(const double* X, int64_t side, const int64_t* cone_idx, int32_t index_base, proxsdp_clique_cuts* q) {
    return guarded([&]() -> int {
        proxsdp::check_clique_struct(q, false);
        if (!X) throw std::invalid_argument("proxsdp_host_clique_cuts: X is NULL");
        if (side < q->base_size + 2 || side > proxsdp::CLQ_MAX_SIDE)
            throw std::invalid_argument("proxsdp_host_clique_cuts: side must be base_size + 2 .. 46340");
        if (index_base != 0 && index_base != 1) throw std::invalid_argument("index_base must be 0 or 1");
        proxsdp::check_clique_bases(*q, side);
        proxsdp::host_clique_cuts(X, side, cone_idx, index_base, *q);
        return 0;
    });
}

int proxsdp_hip_model_inactive_rows(proxsdp_model* mdl, proxsdp_inactive_rows* q) {
    return guarded([&]() -> int {
        proxsdp::check_inactive_struct(q);
        if (!mdl) throw std::invalid_argument("NULL handle");
        mdl->inactive_rows(*q);
        return 0;
    });
}

int proxsdp_hip_model_round(proxsdp_model* mdl, proxsdp_rounding* q) {
    return guarded([&]() -> int {
        proxsdp::check_rounding_struct(q, true);
        if (!mdl) throw std::invalid_argument("NULL handle");
        const proxsdp::BlockInfo& B = mdl->cone(q->cone, "proxsdp_rounding");
        proxsdp::check_rounding_factors(*q, B.n, q->on_device == 0);
        // (the host mirror of the exit path's c is what the device holds: create and every update leave the two equal)
        if (q->adj_ptr && proxsdp::round_adjacency_count(mdl->S->P.c_orig.data() + B.off, B.n) > q->adj_cap)
            throw std::invalid_argument("proxsdp_rounding.adj_cap is smaller than the adjacency");
        mdl->round(*q);
        return 0;
    });
}

int proxsdp_host_round(int64_t side, const int64_t* adj_ptr, const int64_t* adj_col, const double* adj_val, const double* diag,
                       proxsdp_rounding* q) {
    return guarded([&]() -> int {
        proxsdp::check_rounding_struct(q, false);
        if (side > proxsdp::ROUND_MAX_SIDE) throw std::invalid_argument("proxsdp_host_round: side must be 2 .. 46340");
        proxsdp::check_rounding_factors(*q, side, true);
        proxsdp::check_round_adjacency(side, adj_ptr, adj_col, adj_val, diag);
        proxsdp::host_round(side, adj_ptr, adj_col, adj_val, diag, *q);
        return 0;
    });
}

int proxsdp_host_round_directions(int64_t seed, int32_t r, int32_t trials, double* g) {
    return guarded([&]() -> int {
        if (!g) throw std::invalid_argument("proxsdp_host_round_directions: g is NULL");
        proxsdp::check_round_shape(r, trials);
        if (r > proxsdp::ROUND_MAX_SIDE) throw std::invalid_argument("proxsdp_host_round_directions: r must be 1 .. 46340");
        for (int64_t k = 0; k < r; ++k)
            for (int64_t t = 0; t < trials; ++t) g[k * trials + t] = proxsdp::round_direction((uint64_t)seed, r, k, t);
        return 0;
    });
}

int proxsdp_hip_model_bound(proxsdp_model* mdl, proxsdp_dual_bound* q) {
    return guarded([&]() -> int {
        if (!q) throw std::invalid_argument("NULL proxsdp_dual_bound");
        proxsdp::check_struct_size(q, "proxsdp_dual_bound");
        if (!mdl) throw std::invalid_argument("NULL handle");
        const proxsdp::Prep& P = mdl->S->P;
        if (!P.socs.empty()) throw std::domain_error("proxsdp_hip_model_bound does not serve a model with a second-order cone");
        if (P.conelen != P.n || P.blocks.empty())
            throw std::domain_error("proxsdp_hip_model_bound serves models whose variables all lie in PSD cones: some variable is outside every cone");
        if (P.dense()) throw std::domain_error("proxsdp_hip_model_bound does not serve a dense M_dense");
        if (P.equilibrated) throw std::domain_error("proxsdp_hip_model_bound does not serve an equilibrated model: the duals of a result are rescaled");
        proxsdp::check_bound_struct(q, P.p, P.m, (int64_t)P.blocks.size(), true);
        mdl->bound(*q);
        return 0;
    });
}

int proxsdp_host_dual_bound(int64_t n, int64_t p, int64_t m, const double* c, const proxsdp_csc* M, const double* bh,
                            int64_t n_psd, const int64_t* psd_ptr, const int64_t* psd_idx, int32_t index_base,
                            proxsdp_dual_bound* q) {
    return guarded([&]() -> int {
        if (n < 1 || p < 0 || m < 0 || n_psd < 1) throw std::invalid_argument("proxsdp_host_dual_bound: n, n_psd must be >= 1 and p, m >= 0");
        if (index_base != 0 && index_base != 1) throw std::invalid_argument("index_base must be 0 or 1");
        if (!c || !M || (p + m > 0 && !bh) || !psd_ptr || !psd_idx) throw std::invalid_argument("proxsdp_host_dual_bound: a NULL argument");
        proxsdp::check_bound_struct(q, p, m, n_psd, false);
        proxsdp::check_csc(*M, p + m, n, index_base, "M");
        for (int64_t i = 0; i < n; ++i)
            if (!std::isfinite(c[i])) throw std::invalid_argument("proxsdp_host_dual_bound: non-finite entry in c");
        for (int64_t r = 0; r < p + m; ++r)
            if (!std::isfinite(bh[r])) throw std::invalid_argument("proxsdp_host_dual_bound: non-finite entry in bh");
        for (int64_t e = 0; e < M->colptr[n] - index_base; ++e)
            if (!std::isfinite(M->nzval[e])) throw std::invalid_argument("proxsdp_host_dual_bound: non-finite entry in M");
        proxsdp::host_dual_bound(n, p, m, c, *M, bh, n_psd, psd_ptr, psd_idx, index_base, *q);
        return 0;
    });
}

static void check_cholesky_args(const double* A, int64_t s, double shift, const int64_t* fail_col) {
    if (!A || !fail_col) throw std::invalid_argument("cholesky: A or fail_col is NULL");
    if (s < 1 || s > proxsdp::BOUND_MAX_SIDE) throw std::invalid_argument("cholesky: s must be 1 .. 46340");
    if (!(shift >= 0.0) || !std::isfinite(shift)) throw std::invalid_argument("cholesky: shift must be finite and >= 0");
}

int proxsdp_hip_cholesky(const double* A, int64_t s, double shift, double* R_out, int64_t* fail_col) {
    return guarded([&]() -> int {
        check_cholesky_args(A, s, shift, fail_col);
        Engine E(nullptr, 2, 2);
        *fail_col = proxsdp::device_cholesky(E.S.stream, A, s, shift, R_out);
        return 0;
    });
}

int proxsdp_host_cholesky(const double* A, int64_t s, double shift, double* R_out, int64_t* fail_col) {
    return guarded([&]() -> int {
        check_cholesky_args(A, s, shift, fail_col);
        double nu = 0.0;
        for (int64_t i = 0; i < s; ++i) {
            double a = 0.0;
            for (int64_t j = 0; j < s; ++j) a += std::fabs(A[i * s + j]);
            nu = std::max(nu, a);
        }
        std::vector<double> W(A, A + s * s);
        for (int64_t i = 0; i < s; ++i) W[(size_t)(i * s + i)] = A[i * s + i] + shift;
        *fail_col = proxsdp::host_cholesky(W.data(), s, proxsdp::bound_pivot_floor(nu));
        if (R_out)
            for (int64_t c = 0; c < s; ++c)
                for (int64_t r = 0; r < s; ++r) R_out[c * s + r] = r >= c ? W[(size_t)(c * s + r)] : 0.0;
        return 0;
    });
}

int proxsdp_hip_model_solve(proxsdp_model* mdl, const proxsdp_options* run_opt, proxsdp_result* res,
                            const proxsdp_start* start, const proxsdp_device_vectors* start_dev,
                            proxsdp_psd_factors* fac, proxsdp_device_vectors* out_dev) {
    const double t_entry = proxsdp::now_s();
    return guarded([&]() -> int {
        if (!mdl || !res) throw std::invalid_argument("NULL handle or result");
        proxsdp_options run;
        if (run_opt) {
            run = checked_options(run_opt);
            // every option but the ones that shape nothing in the set-up must be create's
            static const char* const free_fields[] = {"time_limit", "max_iter", "log_verbose", "log_freq", "warn_on_limit", "trace_capacity"};
            for (const proxsdp::OptEntry& e : proxsdp::option_table()) {
                bool is_free = false;
                for (const char* f : free_fields) is_free = is_free || std::strcmp(f, e.name) == 0;
                if (is_free) continue;
                const size_t w = e.type == proxsdp::OT_I32 ? 4 : 8;
                if (std::memcmp(reinterpret_cast<const char*>(&run) + e.offset, reinterpret_cast<const char*>(&mdl->opt0) + e.offset, w) != 0)
                    throw std::invalid_argument(std::string("proxsdp_hip_model_solve: run_opt.") + e.name +
                                                " differs from the options of proxsdp_hip_model_create");
            }
        }
        proxsdp::SolveRequest req;
        req.start = start; req.start_dev = start_dev; req.factors_out = fac; req.out_dev = out_dev;
        req.device_exit = true;
        check_request(&mdl->shape, res, mdl->opt0.device_id, req, "proxsdp_hip_model_solve");
        reset_result(res);
        mdl->solve(t_entry, run_opt ? &run : nullptr, res, req);
        return 0;
    });
}

int proxsdp_hip_model_norm2(const double* v, int64_t n, int32_t grid, double* out) {
    return guarded([&]() -> int {
        if ((n > 0 && !v) || !out || n < 0 || grid > 65535) throw std::invalid_argument("invalid argument");
        Engine E(nullptr, 2, 2);
        proxsdp::Solver& S = E.S;
        proxsdp::DevBuf<double> d((size_t)std::max<int64_t>(n, 1)), part, sum;
        d.upload(v, (size_t)n, S.stream);
        *out = proxsdp::model_norm2(S.stream, d.p, n, part, sum, grid);
        return 0;
    });
}

int proxsdp_hip_exit_vectors(const proxsdp_problem* prob, const proxsdp_options* opt, const double* x, const double* y,
                             int32_t zero_c, double* primal, double* dual_cone, double* dual_eq, double* dual_in,
                             double* slack_eq, double* slack_in, double* viol, double* neg, int64_t neg_cap) {
    return guarded([&]() -> int {
        if (!prob) throw std::invalid_argument("NULL problem");
        if ((prob->n > 0 && !x) || (prob->p + prob->m > 0 && !y)) throw std::invalid_argument("exit vectors: NULL iterate");
        check_request(prob, nullptr, 0, proxsdp::SolveRequest{}, "proxsdp_hip_exit_vectors");
        proxsdp_result dummy{};
        const proxsdp_options o = begin_solve(opt, &dummy);
        proxsdp::Solver S(*prob, o, dummy);
        S.test_exit_vectors(x, y, zero_c != 0, primal, dual_cone, dual_eq, dual_in, slack_eq, slack_in, viol, neg, neg_cap);
        return 0;
    });
}

int proxsdp_hip_start_point(const proxsdp_problem* prob, const proxsdp_options* opt, const proxsdp_start* start,
                            proxsdp_state* out) {
    return guarded([&]() -> int {
        if (!prob || !out) throw std::invalid_argument("NULL problem or state");
        proxsdp::SolveRequest req;
        req.start = start; req.start_out = out;
        check_request(prob, nullptr, 0, req, "proxsdp_hip_start_point");
        if (out->struct_size != (int64_t)sizeof(proxsdp_state)) throw std::invalid_argument("proxsdp_state.struct_size mismatch");
        if (out->n != prob->n || out->Q != prob->p + prob->m || out->n_psd != prob->n_psd)
            throw std::invalid_argument("start point: n / Q / n_psd do not match the problem");
        if (!out->x || !out->Mty || (out->Q > 0 && (!out->y || !out->Mx)) || (out->n_psd > 0 && !out->target_rank))
            throw std::invalid_argument("start point: NULL array");
        proxsdp_result dummy{};
        const proxsdp_options o = begin_solve(opt, &dummy);
        proxsdp::Solver S(*prob, o, dummy);
        S.req = req;
        S.run();
        return 0;
    });
}

// ---- block-sharded solve from one call: in-process shards (shard_split.hpp, shard_group.hpp)
namespace {
struct ShardRun {
    proxsdp::ShardData data;
    proxsdp_result res{};
    std::vector<double> primal, dual_cone, dual_eq, dual_in, slack_eq, slack_in, trace;
    int code = 0;
    bool peer = false;                 // stopped because another shard did
    bool left = false;                 // has left the group
    long long iter = -1;               // iteration it stopped in (-1: the solver was never constructed)
    std::string err;
};

// counters, byte counts and summed event durations add up over the shards; wall-clock timers take the maximum
void merge_shard_stats(proxsdp_stats& a, const proxsdp_stats& b) {
#define PX_SUM(f) a.f += b.f
#define PX_MAX(f) a.f = std::max(a.f, b.f)
    PX_SUM(lanczos_matvecs); PX_SUM(lanczos_restarts); PX_SUM(lanczos_calls); PX_SUM(full_eigs); PX_SUM(krylov_fallbacks);
    PX_SUM(linesearch_trials); PX_SUM(symv_launches); PX_SUM(symv_profiled); PX_SUM(symv_profiled_ms); PX_SUM(symv_bytes);
    PX_SUM(algorithmic_bytes);
    PX_MAX(init_time); PX_MAX(loop_time); PX_MAX(exit_time); PX_MAX(t_primal); PX_MAX(t_psd); PX_MAX(t_linesearch); PX_MAX(t_residual);
    PX_SUM(dense_passes); PX_SUM(dense_ms); PX_SUM(fop_projections); PX_SUM(exit_matvecs);
    PX_MAX(host_eig_time);
    PX_SUM(host_eigs); PX_SUM(device_eigs); PX_SUM(batched_small_eigs); PX_SUM(mfma_reconstructions); PX_SUM(orth_profiled);
    PX_SUM(orth_profiled_ms); PX_SUM(full_eig_solver_ms); PX_SUM(full_eig_recon_ms); PX_SUM(cycle_launches);
    PX_SUM(full_eigs_lanczos); PX_SUM(cycle_steps); PX_SUM(cycle_ms); PX_SUM(warm_starts); PX_SUM(full_eigs_sign);
    PX_SUM(sign_products); PX_SUM(sign_engine_projections); PX_SUM(sign_engine_rejected); PX_SUM(sign_engine_checks);
    PX_SUM(sign_engine_mismatches); PX_SUM(full_eigs_lanczos_checks); PX_SUM(full_eigs_lanczos_mismatches);
    PX_SUM(batched_block_steps); PX_SUM(rccl_reductions); PX_SUM(batched_profiled_blocks); PX_SUM(host_eig_merges);
    PX_MAX(host_eig_overlap_time);
    PX_SUM(sign_short_pass); PX_SUM(sign_short_fail); PX_SUM(full_eigs_lanczos_certified); PX_SUM(full_eigs_lanczos_cert_failed);
    PX_SUM(cert_matvecs); PX_SUM(dense_truncated_projections); PX_SUM(wide_krylov_projections);
    for (int k = 0; k < 4; ++k) PX_SUM(reserved_s[k]);
    PX_SUM(dense_setup_passes); PX_SUM(dense_sigma_steps);
#undef PX_SUM
#undef PX_MAX
}

// body(s) for every shard of a group: shard 0 on the calling thread, the others on threads of their own.  When a thread cannot
// be started (std::system_error), the shards that never started leave the group -- the started ones would otherwise wait for
// them --, the started ones are joined, and the error is the caller's
void run_shard_threads(int n_shards, proxsdp::ShardGroup& group, const std::function<void(int)>& body) {
    std::vector<std::thread> th;
    th.reserve((size_t)std::max(n_shards - 1, 0));
    try {
        for (int s = 1; s < n_shards; ++s) th.emplace_back(std::cref(body), s);
    } catch (...) {
        for (int s = (int)th.size(); s < n_shards; ++s) group.leave();       // shard 0 and shards th.size() + 1 ...
        for (auto& t : th) t.join();
        throw;
    }
    body(0);
    for (auto& t : th) t.join();
}
}  // namespace

int proxsdp_hip_solve_sharded(const proxsdp_problem* prob, const proxsdp_options* opt, int32_t n_shards,
                              const int32_t* device_ids, const int32_t* psd_owner, const int32_t* soc_owner,
                              const int32_t* free_owner, proxsdp_result* res, proxsdp_stats* shard_stats) {
    int shard_rc = 0;
    std::string shard_msg;
    const int rc = guarded([&]() -> int {
        if (!prob || !res) throw std::invalid_argument("NULL problem or result");
        const proxsdp_options o = begin_solve(opt, res);
        // ---- everything that is rejected before a thread starts
        const proxsdp::ShardPlan L = proxsdp::plan_shards(*prob, n_shards, psd_owner, soc_owner, free_owner);
        proxsdp::reject_for_shard(false, !o.approx_norm, o.equilibration != 0 || o.equilibration_force != 0);
        if (o.debug_fail_iteration > 0) {
            const char* e = std::getenv("PROXSDP_HIP_FAULT_INJECTION");
            if (!(e && e[0] == '1')) throw std::invalid_argument("debug_fail_iteration needs PROXSDP_HIP_FAULT_INJECTION=1 in the environment (test switch)");
        }
        int ndev = 0;
        PX_HIP(hipGetDeviceCount(&ndev));
        if (ndev <= 0) throw proxsdp::HipError("no HIP device available");
        proxsdp::ShardGroup group(n_shards);
        for (int s = 0; s < n_shards; ++s) {
            group.device[s] = device_ids ? device_ids[s] : o.device_id;
            if (group.device[s] < 0 || group.device[s] >= ndev) throw std::invalid_argument("device_ids: device out of range");
        }
        // shards on different devices read each other's partial buffers: peer access for every ordered pair of distinct
        // devices, or the partials are staged in pinned host memory by all
        for (int a = 0; a < n_shards && !group.stage_host; ++a)
            for (int b = 0; b < n_shards; ++b) {
                if (group.device[a] == group.device[b]) continue;
                int can = 0;
                if (hipDeviceCanAccessPeer(&can, group.device[a], group.device[b]) != hipSuccess || !can) {
                    (void)hipGetLastError();
                    group.stage_host = true;
                    break;
                }
            }
        std::vector<ShardRun> runs(n_shards);
        for (int s = 0; s < n_shards; ++s) {
            ShardRun& R = runs[s];
            R.data = proxsdp::split_shard(*prob, L, s);
            const size_t n = R.data.vars.size(), p = R.data.rows_eq.size(), m = R.data.rows_in.size();
            R.primal.assign(n, 0.0); R.dual_cone.assign(n, 0.0);
            R.dual_eq.assign(p + 1, 0.0); R.slack_eq.assign(p + 1, 0.0); R.dual_in.assign(m + 1, 0.0); R.slack_in.assign(m + 1, 0.0);
            R.trace.assign((size_t)std::max(o.trace_capacity, 0) * PROXSDP_TRACE_COLS + 1, 0.0);
            R.res.primal = R.primal.data(); R.res.dual_cone = R.dual_cone.data();
            R.res.dual_eq = R.dual_eq.data(); R.res.slack_eq = R.slack_eq.data();
            R.res.dual_in = R.dual_in.data(); R.res.slack_in = R.slack_in.data();
            R.res.trace = R.trace.data();
        }
        // ---- one host thread per shard; whatever happens in it ends in its ShardRun, and it always leaves the group
        auto body = [&](int s) {
            ShardRun& R = runs[s];
            R.code = guarded([&]() -> int {
                proxsdp_options os = o;
                os.device_id = group.device[s];
                if (n_shards > 1) {
                    // the AUTO helper-thread counts are shared among the shards of the process (both knobs leave every
                    // result bit-identical); explicit values are the caller's business
                    if (os.block_threads < 0) os.block_threads = 8 / n_shards >= 2 ? 8 / n_shards : 0;
                    if (os.host_merge_threads < 0) os.host_merge_threads = 3 / n_shards;
                    if (s != n_shards - 1) os.debug_fail_iteration = 0;       // fault injection: the last shard only
                }
                const proxsdp_problem sp = R.data.problem();
                proxsdp::Solver S(sp, os, R.res, &group, s);
                // on the way out, however that happens: finish this shard's own launches (its last coupling-sum kernel reads
                // the peers' buffers), leave the group, and keep this solver's device buffers until every shard has left
                struct Farewell {
                    proxsdp::Solver& S; proxsdp::ShardGroup& g; bool& left;
                    ~Farewell() {
                        if (S.stream.main) (void)hipStreamSynchronize(S.stream.main);
                        g.leave(); left = true;
                        g.wait_all_left();
                    }
                } farewell{S, group, R.left};
                try {
                    S.run();
                } catch (const proxsdp::PeerFailure&) {
                    R.peer = true; R.iter = S.current_iteration();
                    throw;
                } catch (...) {
                    R.iter = S.current_iteration();
                    throw;
                }
                R.iter = S.current_iteration();
                return 0;
            });
            if (R.code != 0) R.err = g_last_error;          // (thread-local: carried over to the caller's thread below)
            if (!R.left) group.leave();                      // (the solver was never constructed)
        };
        run_shard_threads(n_shards, group, body);
        if (shard_stats) for (int s = 0; s < n_shards; ++s) shard_stats[s] = runs[s].res.stats;
        // ---- the lowest shard that failed for reasons of its own (else the lowest that failed at all)
        int bad = -1;
        for (int s = 0; s < n_shards && bad < 0; ++s) if (runs[s].code != 0 && !runs[s].peer) bad = s;
        for (int s = 0; s < n_shards && bad < 0; ++s) if (runs[s].code != 0) bad = s;
        if (bad >= 0) {
            shard_rc = runs[bad].code;
            shard_msg = "shard " + std::to_string(bad) + " of " + std::to_string(n_shards) + ": " + runs[bad].err +
                        " [shards stopped in iteration";
            for (int s = 0; s < n_shards; ++s) shard_msg += " " + std::to_string(runs[s].iter);
            shard_msg += "]";
            return 0;
        }
        // ---- the whole model's result
        const proxsdp_result& R0 = runs[0].res;
        res->status = R0.status; res->certificate_found = R0.certificate_found;
        res->primal_feasible_user_tol = R0.primal_feasible_user_tol; res->dual_feasible_user_tol = R0.dual_feasible_user_tol;
        res->result_count = R0.result_count; res->final_rank = R0.final_rank; res->iter = R0.iter;
        res->primal_residual = R0.primal_residual; res->dual_residual = R0.dual_residual;
        res->objval = R0.objval; res->dual_objval = R0.dual_objval; res->gap = R0.gap; res->time = R0.time;
        res->dual_feasibility = R0.dual_feasibility;
        std::memcpy(res->status_string, R0.status_string, sizeof(res->status_string));
        for (int s = 0; s < n_shards; ++s) {
            const ShardRun& R = runs[s];
            proxsdp::gather_shard(R.data, R.primal.data(), R.dual_cone.data(), R.dual_eq.data(), R.dual_in.data(),
                                  R.slack_eq.data(), R.slack_in.data(), *res);
        }
        res->stats = R0.stats;
        for (int s = 1; s < n_shards; ++s) merge_shard_stats(res->stats, runs[s].res.stats);
        if (o.trace_capacity > 0) {
            const int64_t rows = R0.trace_rows;
            for (int s = 1; s < n_shards; ++s)
                if (runs[s].res.trace_rows != rows) throw std::logic_error("the shards' traces differ in length");
            std::copy(runs[0].trace.begin(), runs[0].trace.begin() + rows * PROXSDP_TRACE_COLS, res->trace);
            const int first_psd = prob->n_psd > 0 ? L.psd_owner[0] : 0;
            for (int64_t r = 0; r < rows; ++r) {
                double mv = 0.0;
                for (int s = 0; s < n_shards; ++s) mv += runs[s].trace[r * PROXSDP_TRACE_COLS + 13];
                res->trace[r * PROXSDP_TRACE_COLS + 13] = mv;
                res->trace[r * PROXSDP_TRACE_COLS + 10] = runs[first_psd].trace[r * PROXSDP_TRACE_COLS + 10];
            }
            res->trace_rows = rows;
        }
        return 0;
    });
    if (rc == 0 && shard_rc != 0) {
        g_last_error = shard_msg;
        return shard_rc;
    }
    return rc;
}

int proxsdp_hip_coupling_sum(const double* parts, int32_t n_shards, int64_t len, const int64_t* rows,
                             const double* v_in, int64_t n, double* v_out) {
    return guarded([&]() -> int {
        if (!parts || !rows || !v_in || !v_out || n_shards < 1 || n_shards > 1024 || len < 1 || n < 1 ||
            len >= ((int64_t)1 << 31) || n >= ((int64_t)1 << 31))
            throw std::invalid_argument("invalid argument");
        std::vector<int> r32(len);
        for (int64_t k = 0; k < len; ++k) {
            if (rows[k] < 0 || rows[k] >= n) throw std::invalid_argument("row outside the vector");
            r32[k] = (int)rows[k];
        }
        Engine E(nullptr, 2, 2);
        proxsdp::Solver& S = E.S;
        // one device buffer per shard, as in a solve (separate allocations: odd lengths leave the later ones unaligned to
        // nothing but the allocator's granularity -- the kernel makes no alignment assumption beyond 8 bytes)
        std::vector<proxsdp::DevBuf<double>> part(n_shards);
        std::vector<const double*> tab(n_shards);
        for (int s = 0; s < n_shards; ++s) {
            part[s].alloc((size_t)len);
            part[s].upload(parts + (size_t)s * len, (size_t)len, S.stream);
            tab[s] = part[s].p;
        }
        proxsdp::DevBuf<const double*> tab_d((size_t)n_shards);
        proxsdp::DevBuf<int> rows_d((size_t)len);
        proxsdp::DevBuf<double> v((size_t)n);
        tab_d.upload(tab.data(), (size_t)n_shards, S.stream);
        rows_d.upload(r32.data(), (size_t)len, S.stream);
        v.upload(v_in, (size_t)n, S.stream);
        proxsdp::launch_coupling_sum(S.stream, tab_d.p, n_shards, rows_d.p, (int)len, v.p);
        PX_HIP(hipGetLastError());
        v.download(v_out, (size_t)n, S.stream);
        PX_HIP(hipStreamSynchronize(S.stream));
        return 0;
    });
}

int proxsdp_hip_psd_project(const double* packed_in, int64_t n, int32_t target_rank, int32_t mode,
                            const proxsdp_options* opt, const double* resid, double* packed_out,
                            int32_t* out_rank, double* out_min_eig, int64_t* out_nmatvec,
                            int32_t* out_converged, int32_t* out_fell_back) {
    return guarded([&]() -> int {
        if (!packed_in || !packed_out) throw std::invalid_argument("NULL buffer");
        if (target_rank < 1) throw std::invalid_argument("target_rank < 1");
        proxsdp_options o = checked_options(opt);
        if (mode == 1) { o.full_eig_decomp = 1; o.full_eig_lanczos = 0; o.full_eig_sign = 0; }
        // mode 4: full_eig! by the sign-function projection (fp64 MFMA products)
        if (mode == 4) { o.full_eig_decomp = 1; o.full_eig_lanczos = 0; o.full_eig_sign = 1; }
        // the test entry point takes the Krylov branch whenever mode == 0
        if (mode == 0) { o.min_size_krylov_eigs = 0; o.max_target_rank_krylov_eigs = std::max(o.max_target_rank_krylov_eigs, target_rank); }
        // mode 2: full_eig! served by the Lanczos engine, `target_rank` = the estimate of the number of
        // positive eigenvalues (in a solve: the count of the block's previous projection)
        if (mode == 2) { o.full_eig_decomp = 1; o.full_eig_lanczos = 1; o.min_size_krylov_eigs = 0; }
        const int ws = mode == 2 ? std::min<int>({(int)n, 94, 2 * (target_rank + std::max(3, target_rank / 8)) + 2}) : target_rank;
        Engine E(&o, n, ws);
        E.set_resid(resid);
        proxsdp::Solver& S = E.S;
        const int64_t N = n * (n + 1) / 2;
        proxsdp::DevBuf<double> x(N);
        x.upload(packed_in, N, S.stream);
        S.P.blocks.push_back({(int)n, N, 0});
        if (mode == 2) S.eig[0].xprev.last_npos = target_rank;
        if (mode == 3 || mode == 5) {                       // the small-block kernels on this one block: 3 batched Jacobi, 5 LDS-resident sign projection
            if (n < 2 || n > 64) throw std::invalid_argument("mode 3 / 5: 2 <= n <= 64");
            proxsdp::DevBuf<long long> off(1); proxsdp::DevBuf<int> side(1), rk(2);
            const long long o0 = 0; const int s0 = (int)n;
            off.upload(&o0, 1, S.stream); side.upload(&s0, 1, S.stream);
            if (mode == 3) {
                const size_t lds = ((size_t)2 * n * (n | 1) + 64) * sizeof(double) + 64 * sizeof(int);
                if (lds > 48 * 1024)
                    PX_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(proxsdp::dev::k_small_psd_project),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
                hipLaunchKernelGGL(proxsdp::dev::k_small_psd_project, dim3(1), dim3(proxsdp::dev::TPB), lds, S.stream,
                                   x.p, (const long long*)off.p, (const int*)side.p, o.tol_psd, rk.p, rk.p + 1, 2, 64, (int*)nullptr);
            } else {
                const size_t lds = proxsdp::dev::small_sign_lds_bytes((int)n);
                if (lds > 48 * 1024)
                    PX_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(proxsdp::dev::k_small_sign_project),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
                // target_rank doubles as the start row of the schedule here (1 = full table ... 9 = row 8, the solver's default)
                static const proxsdp::dev::SignSchedule sched;
                const int j0 = std::max(0, std::min(target_rank - 1, proxsdp::dev::SIGN_STEPS - 3));
                hipLaunchKernelGGL(proxsdp::dev::k_small_sign_project, dim3(1), dim3(proxsdp::dev::SS_TPB), lds, S.stream,
                                   x.p, (const long long*)off.p, (const int*)side.p, 2, 64, rk.p, rk.p + 1, j0, sched.fallback_row(j0), (int*)nullptr);
            }
            int hr[2] = {0, 0};
            rk.download(hr, 2, S.stream);
            x.download(packed_out, N, S.stream);
            PX_HIP(hipStreamSynchronize(S.stream));
            if (out_rank) *out_rank = hr[0];
            if (out_min_eig) *out_min_eig = 0.0;
            if (out_nmatvec) *out_nmatvec = 0;
            if (out_converged) *out_converged = hr[1];
            if (out_fell_back) *out_fell_back = 0;
            return 0;
        }
        S.test_project(0, x.p, target_rank);
        x.download(packed_out, N, S.stream);
        PX_HIP(hipStreamSynchronize(S.stream));
        if (out_rank) *out_rank = (int32_t)S.test_rank();
        if (out_min_eig) *out_min_eig = S.test_min_eig();
        S.merge_block_stats();
        if (out_nmatvec) *out_nmatvec = S.st.lanczos_matvecs;
        if (out_converged) *out_converged = S.eig[0].converged_eigs;
        if (out_fell_back) *out_fell_back = mode == 2 ? (int32_t)(S.st.full_eigs_lanczos == 0) : (int32_t)S.st.krylov_fallbacks;
        return 0;
    });
}

int proxsdp_hip_full_eig_kernel(const double* packed_in, int64_t n, int32_t sign, double* packed_out,
                                int32_t repeat, double* ms, int32_t* out_rank, int64_t* out_products) {
    return guarded([&]() -> int {
        if (!packed_in || !packed_out) throw std::invalid_argument("NULL buffer");
        proxsdp_options o = checked_options(nullptr);
        o.full_eig_decomp = 1; o.full_eig_lanczos = 0; o.full_eig_sign = sign < 0 ? -1 : (sign ? 1 : 0);   // (-1: the solver's own choice of engine)
        if (sign >= 100) o.sign_start_row = sign - 100;
        Engine E(&o, n, 2);
        proxsdp::Solver& S = E.S;
        const int64_t N = n * (n + 1) / 2;
        proxsdp::DevBuf<double> x(N), y(N);
        x.upload(packed_in, N, S.stream);
        S.P.blocks.push_back({(int)n, N, 0});
        S.test_full_eig(x.p, y.p);             // warm-up (allocations, rocSOLVER workspace)
        PX_HIP(hipStreamSynchronize(S.stream));
        const int reps = std::max(1, repeat);
        const double t0 = proxsdp::now_s();
        for (int i = 0; i < reps; ++i) S.test_full_eig(x.p, y.p);
        PX_HIP(hipStreamSynchronize(S.stream));
        if (ms) *ms = (proxsdp::now_s() - t0) * 1e3 / reps;
        y.download(packed_out, N, S.stream);
        PX_HIP(hipStreamSynchronize(S.stream));
        S.merge_block_stats();
        if (out_rank) *out_rank = (int32_t)S.test_rank();
        if (out_products) *out_products = S.st.sign_products / (reps + 1);
        return 0;
    });
}

int proxsdp_hip_eigsolve(const double* packed, int64_t n, int32_t nev, const proxsdp_options* opt,
                         const double* resid, int32_t cap, double* vals, double* vecs,
                         int32_t* out_count, int32_t* out_converged, int64_t* out_nmatvec,
                         int32_t* out_numiter) {
    return guarded([&]() -> int {
        if (!packed || !vals || !vecs) throw std::invalid_argument("NULL buffer");
        if (nev < 1) throw std::invalid_argument("nev < 1");
        Engine E(opt, n, nev);
        E.set_resid(resid);
        proxsdp::Solver& S = E.S;
        proxsdp::EigWork& W = S.eig[0];
        const int64_t N = n * (n + 1) / 2;
        proxsdp::DevBuf<double> x(N);
        x.upload(packed, N, S.stream);
        S.lanczos(W, x.p, nev);
        PX_HIP(hipStreamSynchronize(S.stream));
        const int cnt = std::min<int>(W.count, cap);
        for (int i = 0; i < cnt; ++i) vals[i] = W.vals[i];
        if (cnt > 0)
            PX_HIP(hipMemcpy2D(vecs, (size_t)n * 8, W.Z.p, (size_t)W.npad * 8, (size_t)n * 8, cnt,
                               hipMemcpyDeviceToHost));
        if (out_count) *out_count = W.count;
        if (out_converged) *out_converged = W.converged_eigs;
        S.merge_block_stats();
        if (out_nmatvec) *out_nmatvec = S.st.lanczos_matvecs;
        if (out_numiter) *out_numiter = W.numiter;
        return 0;
    });
}

int proxsdp_hip_symv_packed(const double* packed, int64_t n, const double* v, double* y,
                            int32_t repeat, double* ms) {
    return guarded([&]() -> int {
        if (!packed || !v || !y) throw std::invalid_argument("NULL buffer");
        Engine E(nullptr, n, 2);
        proxsdp::Solver& S = E.S;
        proxsdp::EigWork& W = S.eig[0];
        const int64_t N = n * (n + 1) / 2;
        proxsdp::DevBuf<double> x(N), vd(W.npad);
        x.upload(packed, N, S.stream);
        vd.zero(S.stream);
        vd.upload(v, n, S.stream);
        PX_HIP(hipMemsetAsync(W.ctl_p, 0, sizeof(proxsdp::dev::LanczosCtl), S.stream));
        // y = (sum of partials)/sqrt2
        S.launch_symv(W, x.p, vd.p, false);
        hipLaunchKernelGGL(proxsdp::dev::k_symv_collect, dim3(W.nt), dim3(proxsdp::dev::TPB), 0, S.stream,
                           W.Ppart.p, W.nt, W.npad, W.w.p);
        W.w.download(y, n, S.stream);
        PX_HIP(hipStreamSynchronize(S.stream));
        if (repeat > 0 && ms) {
            for (int i = 0; i < 3; ++i) S.launch_symv(W, x.p, vd.p, false);
            *ms = proxsdp::time_launches(S.stream, repeat, [&]() { S.launch_symv(W, x.p, vd.p, false); });
        }
        return 0;
    });
}

int proxsdp_hip_reconstruct(const double* Z, const double* lambda, int64_t n, int32_t r,
                            double* packed_out, int32_t repeat, double* ms) {
    return proxsdp_hip_reconstruct_kernel(Z, lambda, n, r, -1, packed_out, repeat, ms);
}

int proxsdp_hip_reconstruct_kernel(const double* Z, const double* lambda, int64_t n, int32_t r, int32_t mfma,
                                   double* packed_out, int32_t repeat, double* ms) {
    return guarded([&]() -> int {
        if ((r > 0 && (!Z || !lambda)) || !packed_out) throw std::invalid_argument("NULL buffer");
        if (r < 0) throw std::invalid_argument("r < 0");
        proxsdp_options o = checked_options(nullptr);
        o.reconstruct_mfma = mfma;
        Engine E(&o, n, 2);
        proxsdp::Solver& S = E.S;
        proxsdp::EigWork& W = S.eig[0];
        const int64_t N = n * (n + 1) / 2;
        proxsdp::DevBuf<double> x(N), Zd((size_t)std::max<int64_t>(1, n * r)), ld(std::max(1, r));
        Zd.upload(Z, (size_t)n * r, S.stream);
        ld.upload(lambda, r, S.stream);
        S.launch_reconstruct(W, Zd.p, (int)n, ld.p, r, x.p);
        x.download(packed_out, N, S.stream);
        PX_HIP(hipStreamSynchronize(S.stream));
        if (repeat > 0 && ms) {
            *ms = proxsdp::time_launches(S.stream, repeat, [&]() { S.launch_reconstruct(W, Zd.p, (int)n, ld.p, r, x.p); });
        }
        return 0;
    });
}

int proxsdp_hip_factor_residual(const double* packed, int64_t n, const double* V, int64_t ldv,
                                const double* lam, int32_t r, double* resid2, double* xnorm2) {
    return proxsdp_hip_factor_residual_kernel(packed, n, V, ldv, lam, r, resid2, xnorm2, 0, nullptr);
}

int proxsdp_hip_factor_residual_kernel(const double* packed, int64_t n, const double* V, int64_t ldv,
                                       const double* lam, int32_t r, double* resid2, double* xnorm2,
                                       int32_t repeat, double* ms) {
    return guarded([&]() -> int {
        if (!packed || !resid2 || !xnorm2 || (r > 0 && (!V || !lam))) throw std::invalid_argument("NULL buffer");
        if (r < 0) throw std::invalid_argument("r < 0");
        if (n < 1 || n > 46340) throw std::invalid_argument("n out of range");
        if (r > 0 && (ldv < n || ldv >= (int64_t)1 << 31)) throw std::invalid_argument("ldv out of range");
        Engine E(nullptr, n, 2);
        proxsdp::Solver& S = E.S;
        const int64_t N = n * (n + 1) / 2;
        const size_t vcount = r > 0 ? (size_t)ldv * (r - 1) + (size_t)n : 0;   // the last column ends at its row n - 1
        proxsdp::DevBuf<double> x(N), Vd(std::max<size_t>(1, vcount)), ld(std::max(1, r));
        x.upload(packed, N, S.stream);
        Vd.upload(V, vcount, S.stream);
        ld.upload(lam, r, S.stream);
        S.factor_residual(x.p, (int)n, Vd.p, (int)ldv, ld.p, r, *resid2, *xnorm2);
        if (repeat > 0 && ms) {
            const int nt = proxsdp::ceil_div((int)n, proxsdp::dev::TILE);
            const int grid = proxsdp::tile_grid(nt);
            *ms = proxsdp::time_launches(S.stream, repeat, [&]() {
                hipLaunchKernelGGL(proxsdp::dev::k_factor_residual, dim3(grid), dim3(proxsdp::dev::TPB), 0, S.stream,
                                   (const double*)x.p, (int)n, (const double*)Vd.p, (int)ldv, (const double*)ld.p, (int)r,
                                   S.fac_part.p);
            });
            // what comes back is the LAST launch's: a kernel that wrote to the block would show here
            S.factor_residual(x.p, (int)n, Vd.p, (int)ldv, ld.p, r, *resid2, *xnorm2);
        }
        return 0;
    });
}

int proxsdp_hip_spmv(const proxsdp_csc* M, int32_t index_base, int32_t transpose,
                     const double* in, double* out) {
    return guarded([&]() -> int {
        if (!M || !in || !out) throw std::invalid_argument("NULL argument");
        // run through the same preparation + kernels as the solver
        proxsdp_problem pr{};
        pr.n = M->ncols; pr.p = M->nrows; pr.m = 0;
        pr.A = *M;
        std::vector<int64_t> zc((size_t)M->ncols + 1, index_base);
        pr.G.nrows = 0; pr.G.ncols = M->ncols; pr.G.colptr = zc.data();
        std::vector<double> zb((size_t)std::max<int64_t>(M->nrows, 1), 0.0), zcv((size_t)std::max<int64_t>(M->ncols, 1), 0.0);
        pr.b = zb.data(); pr.h = zb.data(); pr.c = zcv.data();
        pr.index_base = index_base;
        proxsdp_options o;
        proxsdp::default_options(&o);
        proxsdp_result dummy{};
        proxsdp::Solver S(pr, o, dummy);
        S.test_spmv(transpose != 0, in, out);
        return 0;
    });
}

int proxsdp_hip_trial_batch(const proxsdp_csc* M, int32_t index_base, const double* c, proxsdp_trial_batch* t) {
    return guarded([&]() -> int {
        if (!M || !c || !t) throw std::invalid_argument("NULL argument");
        if (t->struct_size != (int64_t)sizeof(proxsdp_trial_batch)) throw std::invalid_argument("trial batch: struct_size mismatch");
        // the same preparation as a solve: M as the equality rows of a problem without cones (test_trial_batch sets p)
        proxsdp_problem pr{};
        pr.n = M->ncols; pr.p = M->nrows; pr.m = 0;
        pr.A = *M;
        std::vector<int64_t> zc((size_t)M->ncols + 1, index_base);
        pr.G.nrows = 0; pr.G.ncols = M->ncols; pr.G.colptr = zc.data();
        std::vector<double> zb((size_t)std::max<int64_t>(M->nrows, 1), 0.0);
        pr.b = zb.data(); pr.h = zb.data(); pr.c = c;
        pr.index_base = index_base;
        proxsdp_options o;
        proxsdp::default_options(&o);
        proxsdp_result dummy{};
        proxsdp::Solver S(pr, o, dummy);
        S.test_trial_batch(*t);
        return 0;
    });
}

int proxsdp_hip_cone_tail(const double* x, int64_t n, const int64_t* soc_off, const int32_t* soc_len, int32_t nsoc,
                          const int64_t* one_off, int32_t n_one, double* x_soc, double* gap_in, double* gap_out,
                          double* x_clamp, double* min_eig) {
    return guarded([&]() -> int {
        if (n < 1 || nsoc < 0 || n_one < 0 || !x || !x_soc || !x_clamp || (nsoc > 0 && (!soc_off || !soc_len || !gap_in || !gap_out)) ||
            (n_one > 0 && (!one_off || !min_eig))) throw std::invalid_argument("invalid argument");
        for (int32_t k = 0; k < nsoc; ++k)
            if (soc_len[k] < 1 || soc_off[k] < 0 || soc_off[k] > n - soc_len[k]) throw std::invalid_argument("cone outside x");
        for (int32_t k = 0; k < n_one; ++k)
            if (one_off[k] < 0 || one_off[k] >= n) throw std::invalid_argument("1x1 block outside x");
        Engine E(nullptr, 2, 2);
        E.S.test_cone_tail(x, n, soc_off, soc_len, nsoc, one_off, n_one, x_soc, gap_in, gap_out, x_clamp, min_eig);
        return 0;
    });
}

int proxsdp_hip_project_cones(const proxsdp_problem* prob, const proxsdp_options* opt, proxsdp_project_cones* t) {
    return guarded([&]() -> int {
        if (!prob || !t) throw std::invalid_argument("NULL argument");
        if (t->struct_size != (int64_t)sizeof(proxsdp_project_cones)) throw std::invalid_argument("project cones: struct_size mismatch");
        proxsdp_options o = checked_options(opt);
        o.trace_capacity = 0;
        proxsdp_result dummy{};
        proxsdp::Solver S(*prob, o, dummy);
        S.test_project_cones(*t);
        return 0;
    });
}

int proxsdp_hip_sym_product(proxsdp_sym_product* t) {
    return guarded([&]() -> int {
        if (!t) throw std::invalid_argument("NULL argument");
        if (t->struct_size != (int64_t)sizeof(proxsdp_sym_product)) throw std::invalid_argument("sym product: struct_size mismatch");
        if (t->n < 1 || t->n > 4096) throw std::invalid_argument("sym product: n out of range");
        Engine E(nullptr, t->n, 2);
        E.S.test_sym_product(*t);
        return 0;
    });
}

int proxsdp_hip_reconstruct_fused(proxsdp_reconstruct_fused* t) {
    return guarded([&]() -> int {
        if (!t) throw std::invalid_argument("NULL argument");
        if (t->struct_size != (int64_t)sizeof(proxsdp_reconstruct_fused)) throw std::invalid_argument("reconstruct: struct_size mismatch");
        if (t->n < 1 || t->n > 46340) throw std::invalid_argument("reconstruct: n out of range");
        if (t->r < 0) throw std::invalid_argument("reconstruct: r < 0");
        if (t->ldz < t->n) throw std::invalid_argument("reconstruct: ldz < n");
        if (t->mfma < -1 || t->mfma > 1) throw std::invalid_argument("reconstruct: mfma must be -1, 0 or 1");
        if ((t->r > 0 && (!t->Z || !t->lam)) || !t->xp || !t->respart) throw std::invalid_argument("reconstruct: NULL buffer");
        const int64_t N = (int64_t)t->n * (t->n + 1) / 2;
        if (t->xold && (!t->mask || t->mask_off < 0 || t->mask_words * 32 < t->mask_off + N))
            throw std::invalid_argument("reconstruct: the mask does not cover the block");
        const int nt = proxsdp::ceil_div(t->n, proxsdp::dev::TILE);
        if (t->respart_cap < 2 * (int64_t)proxsdp::tile_grid(nt)) throw std::invalid_argument("reconstruct: respart_cap < 2 grid");
        proxsdp_options o = checked_options(nullptr);
        o.reconstruct_mfma = t->mfma;
        Engine E(&o, t->n, 2);
        E.S.test_reconstruct_fused(*t);
        return 0;
    });
}

int proxsdp_hip_rotate(proxsdp_rotation* t) {
    return guarded([&]() -> int {
        if (!t) throw std::invalid_argument("NULL argument");
        if (t->struct_size != (int64_t)sizeof(proxsdp_rotation)) throw std::invalid_argument("rotation: struct_size mismatch");
        if (t->n < 1 || t->n > 46340) throw std::invalid_argument("rotation: n out of range");
        if (t->K < 1) throw std::invalid_argument("rotation: K < 1");
        if (t->ncols < 0 || t->ncols > t->K) throw std::invalid_argument("rotation: ncols must be 0 .. K");
        if (t->copy_src < -1 || t->Kv < std::max(t->K, t->copy_src + 1)) throw std::invalid_argument("rotation: V has too few columns");
        if (t->out_cols < 1 || t->ncols > t->out_cols || (t->copy_src >= 0 && (t->copy_dst < 0 || t->copy_dst >= t->out_cols)))
            throw std::invalid_argument("rotation: a written column lies outside out");
        if (t->wide != 0 && t->wide != 1) throw std::invalid_argument("rotation: wide must be 0 or 1");
        if (!t->V || (t->ncols > 0 && !t->U) || !t->out) throw std::invalid_argument("rotation: NULL buffer");
        // the workspace rule of Solver::alloc_eigwork: the wide records exist from Krylov dimension 256 on, with the option set
        const int kd = std::max(t->K, std::max(t->Kv, t->out_cols) - 1);
        if (t->wide && kd <= proxsdp::dev::LZ_KMAX) throw std::invalid_argument("rotation: wide = 1 needs the wide workspace (Krylov dimension > 255)");
        if (kd > (t->wide ? proxsdp::dev::LZW_MAXK - 1 : proxsdp::dev::LZ_KMAX)) throw std::invalid_argument("rotation: Krylov dimension out of range");
        proxsdp_options o = checked_options(nullptr);
        o.lanczos_wide_krylov = t->wide;
        o.eigsolver_min_lanczos = kd;
        Engine E(&o, t->n, 2);
        E.S.test_rotate(*t);
        return 0;
    });
}

int proxsdp_hip_tail_copy(proxsdp_tail_copy* t) {
    return guarded([&]() -> int {
        if (!t) throw std::invalid_argument("NULL argument");
        if (t->struct_size != (int64_t)sizeof(proxsdp_tail_copy)) throw std::invalid_argument("tail copy: struct_size mismatch");
        if (t->N < 1 || t->start < 0 || t->start >= t->N) throw std::invalid_argument("tail copy: start must be 0 .. N-1");
        if (t->wgs < 1 || t->wgs > 65536) throw std::invalid_argument("tail copy: wgs out of range");
        if (!t->xin || !t->mask || !t->xout || !t->respart) throw std::invalid_argument("tail copy: NULL buffer");
        if (t->mask_words * 32 < t->N) throw std::invalid_argument("tail copy: the mask does not cover x");
        Engine E(nullptr, 2, 2);
        E.S.test_tail_copy(*t);
        return 0;
    });
}

// columns of the workspace Engine(&o, n, ws_rank) allocates (Solver::alloc_eigwork without the wide records)
static int engine_cap(const proxsdp_options& o, int64_t n, int ws_rank) {
    const int wsr = std::min<int>(std::max(ws_rank, 2), (int)n);
    return std::min(std::max(2 * wsr + 1, (int)o.eigsolver_min_lanczos), proxsdp::dev::LZ_KMAX) + 1;
}
// The positive-part entry's own arguments (the wrapped struct's n is valid) and the Krylov dimension of its run in place of the
// Krylov branch's kd (o.lanczos_wide_krylov is 0): checked before a device is touched and before an output array is written
static int checked_positive_part_dim(const proxsdp_options& o, int64_t n, int nev, int kd, const proxsdp_positive_part& pp) {
    if (pp.ws_rank < 1) throw std::invalid_argument("positive part: ws_rank < 1");
    if (pp.run != 0 && pp.run != 1) throw std::invalid_argument("positive part: run must be 0 or 1");
    if (pp.cert_steps < 0 || pp.cert_steps > proxsdp::dev::KLD) throw std::invalid_argument("positive part: cert_steps out of range");
    if (pp.npos_in < -1 || pp.npos_in > n) throw std::invalid_argument("positive part: npos_in must be -1 .. n");
    if (!pp.run && pp.npos_in < 0) throw std::invalid_argument("positive part: no run needs a locked set (npos_in >= 0)");
    if (pp.npos_in > 0 && (!pp.locked || !pp.locked_vals)) throw std::invalid_argument("positive part: NULL locked set");
    if (!pp.vals || !pp.Z || !pp.cert_alphas || !pp.cert_betas || !pp.basis || !pp.resid2) throw std::invalid_argument("positive part: NULL buffer");
    for (int64_t q = 0; q < (int64_t)std::max(pp.npos_in, 0) * n; ++q)
        if (!std::isfinite(pp.locked[q])) throw std::invalid_argument("positive part: a locked entry is not finite");
    for (int32_t q = 0; q < pp.npos_in; ++q)
        if (!std::isfinite(pp.locked_vals[q])) throw std::invalid_argument("positive part: a locked value is not finite");
    if (o.eigsolver == 1) throw std::invalid_argument("positive part: eigsolver = 1 never takes the positive-part run");
    const int cap = engine_cap(o, n, pp.ws_rank);
    if (pp.cap != cap) throw std::invalid_argument("positive part: cap must be min(max(2 min(max(ws_rank, 2), n) + 1, eigsolver_min_lanczos), 255) + 1");
    return proxsdp::lz_positive_part_dim(cap, kd, nev, (int)o.full_eig_lanczos_kdim10);
}

// the caller's arrays of a positive-part call hold the sentinel wherever nothing is written (after every argument check)
static void prefill_positive_part(proxsdp_positive_part& t, int32_t ldv, double sentinel) {
    const size_t cap = (size_t)t.cap;
    for (double* a : {t.vals, t.cert_alphas, t.cert_betas}) std::fill(a, a + cap, sentinel);
    std::fill(t.Z, t.Z + cap * ldv, sentinel);
    std::fill(t.basis, t.basis + cap * ldv, sentinel);
    std::fill(t.resid2, t.resid2 + ldv, sentinel);
    t.converged = t.count = t.numiter = t.warm = 0;
    t.cert_ran = t.npos = t.steps = t.stop = t.kstop = 0;
    t.differ = t.matvecs = 0;
    t.theta_max = t.scale = t.posres = 0.0;
}

// proxsdp_hip_lanczos_cycles; pp: the same block and arrays under proxsdp_hip_positive_part
static void run_lanczos_cycles(proxsdp_lanczos_cycles* t, proxsdp_positive_part* pp) {
    if (!t) throw std::invalid_argument("NULL argument");
    if (t->struct_size != (int64_t)sizeof(proxsdp_lanczos_cycles)) throw std::invalid_argument("lanczos cycles: struct_size mismatch");
    if (t->n < 1 || t->n > 46340) throw std::invalid_argument("lanczos cycles: n out of range");
    if (t->nev < 1 || t->nev > t->n) throw std::invalid_argument("lanczos cycles: nev must be 1 .. n");
    if (t->max_cycles < 1) throw std::invalid_argument("lanczos cycles: max_cycles < 1");
    if (!t->packed || !t->info || !t->V || !t->alphas || !t->betas || !t->D || !t->f) throw std::invalid_argument("lanczos cycles: NULL buffer");
    proxsdp_options o = checked_options(t->opt);
    if (o.lanczos_wide_krylov != 0 && o.lanczos_wide_krylov != 1) throw std::invalid_argument("lanczos_wide_krylov must be 0 or 1");
    if (o.krylovkit_eager && o.eigsolver != 1) throw std::invalid_argument("lanczos cycles: krylovkit_eager runs another driver");
    if (pp) o.lanczos_wide_krylov = 0;               // (a positive-part run keeps the step kernels' columns)
    const int kd = std::max(2 * t->nev + 1, (int)o.eigsolver_min_lanczos);
    // (a positive-part run clips its dimension to the workspace: the Krylov branch's two refusals are not its own)
    if (!pp && kd > proxsdp::dev::LZ_KMAX && o.lanczos_wide_krylov != 1)
        throw std::invalid_argument("lanczos cycles: a Krylov dimension > 255 needs the wide workspace (lanczos_wide_krylov = 1)");
    if (!pp && kd > proxsdp::dev::LZW_MAXK - 1) throw std::invalid_argument("lanczos cycles: Krylov dimension beyond the workspace");
    const int kdr = pp ? checked_positive_part_dim(o, t->n, t->nev, kd, *pp) : kd;       // the run's
    if (t->cols != kdr + 1 || t->ldv != proxsdp::ceil_div(t->n, proxsdp::dev::TILE) * proxsdp::dev::TILE)
        throw std::invalid_argument("lanczos cycles: cols must be krylovdim + 1, ldv 64 ceil(n / 64)");
    o.krylovkit_max_iter = t->max_cycles; o.arpack_max_iter = t->max_cycles;   // the driver ends the run itself
    // the caller's arrays hold the sentinel wherever the run writes nothing
    const size_t nc = (size_t)t->max_cycles * t->cols;
    std::fill(t->info, t->info + (size_t)t->max_cycles * PROXSDP_LZ_INFO, -1);
    std::fill(t->V, t->V + nc * t->ldv, t->sentinel);
    for (double* a : {t->alphas, t->betas, t->D, t->f}) std::fill(a, a + nc, t->sentinel);
    if (pp) prefill_positive_part(*pp, t->ldv, t->sentinel);
    t->npad = t->ldv; t->krylovdim = kdr; t->cycles = 0;
    Engine E(&o, t->n, pp ? pp->ws_rank : t->nev);
    E.set_resid(t->resid);
    const int64_t N = (int64_t)t->n * (t->n + 1) / 2;
    proxsdp::DevBuf<double> x(N);
    x.upload(t->packed, N, E.S.stream);
    E.S.test_lanczos_cycles(*t, x.p, pp);
}
int proxsdp_hip_lanczos_cycles(proxsdp_lanczos_cycles* t) {
    return guarded([&]() -> int { run_lanczos_cycles(t, nullptr); return 0; });
}

// proxsdp_hip_operator_cycles; pp: the same block and arrays under proxsdp_hip_positive_part
static void run_operator_cycles(proxsdp_operator_cycles* t, proxsdp_positive_part* pp) {
    if (!t) throw std::invalid_argument("NULL argument");
    if (t->struct_size != (int64_t)sizeof(proxsdp_operator_cycles)) throw std::invalid_argument("operator cycles: struct_size mismatch");
    if (t->n < 2 || t->n > 46340) throw std::invalid_argument("operator cycles: n must be 2 .. 46340");
    if (t->nev < 1 || t->nev > t->n) throw std::invalid_argument("operator cycles: nev must be 1 .. n");
    if (t->max_cycles < 1) throw std::invalid_argument("operator cycles: max_cycles < 1");
    if (t->rp < 0 || t->rp > proxsdp::dev::RLD - 1 || t->rp > t->n) throw std::invalid_argument("operator cycles: rp must be 0 .. min(127, n)");
    if (t->f_first < 0 || t->f_first > proxsdp::dev::RLD - 1) throw std::invalid_argument("operator cycles: f_first must be 0 .. 127");
    if (t->no_factors != 0 && t->no_factors != 1) throw std::invalid_argument("operator cycles: no_factors must be 0 or 1");
    if (t->no_factors && t->rp != 0) throw std::invalid_argument("operator cycles: the second form has no factors (rp = 0)");
    const int64_t N = (int64_t)t->n * (t->n + 1) / 2;
    if (t->ns < 0 || t->ns > N) throw std::invalid_argument("operator cycles: ns must be 0 .. n (n + 1) / 2");
    if (!t->info || !t->V || !t->alphas || !t->betas || !t->D || !t->f || (t->ns > 0 && (!t->support || !t->esv)) ||
        (t->rp > 0 && (!t->F || !t->lam)) || (t->probe_v && (!t->probe_ev || !t->probe_tpart || !t->probe_apart)))
        throw std::invalid_argument("operator cycles: NULL buffer");
    for (int64_t s = 0; s < t->ns; ++s)
        if (t->support[s] < 0 || t->support[s] >= N || (s > 0 && t->support[s] <= t->support[s - 1]))
            throw std::invalid_argument("operator cycles: support indices must be strictly ascending and below n (n + 1) / 2");
    auto finite = [](const double* a, size_t cnt) { for (size_t q = 0; q < cnt; ++q) if (!std::isfinite(a[q])) return false; return true; };
    if (t->ns > 0 && !finite(t->esv + (t->no_factors ? t->ns : 0), (size_t)t->ns)) throw std::invalid_argument("operator cycles: a support value is not finite");
    if (t->rp > 0 && (!finite(t->F, (size_t)t->n * t->rp) || !finite(t->lam, t->rp))) throw std::invalid_argument("operator cycles: a factor entry is not finite");
    for (int c = 0; c < t->rp; ++c) if (!(t->lam[c] > 0.0)) throw std::invalid_argument("operator cycles: lam must be positive");
    if ((t->resid && !finite(t->resid, t->n)) || (t->probe_v && !finite(t->probe_v, t->n))) throw std::invalid_argument("operator cycles: a vector entry is not finite");
    proxsdp_options o = checked_options(t->opt);
    if (o.lanczos_operator == 0) throw std::invalid_argument("operator cycles: lanczos_operator = 0 switches the operator form off");
    if (o.krylovkit_eager && o.eigsolver != 1) throw std::invalid_argument("operator cycles: krylovkit_eager runs another driver");
    const int kd = std::max(2 * t->nev + 1, (int)o.eigsolver_min_lanczos);
    if (!pp && kd > proxsdp::dev::LZ_KMAX) throw std::invalid_argument("operator cycles: the operator form takes a Krylov dimension of at most 255");
    o.lanczos_wide_krylov = 0;
    const int kdr = pp ? checked_positive_part_dim(o, t->n, t->nev, kd, *pp) : kd;       // the run's (clipped to the workspace)
    if (t->cols != kdr + 1 || t->ldv != proxsdp::ceil_div(t->n, proxsdp::dev::TILE) * proxsdp::dev::TILE)
        throw std::invalid_argument("operator cycles: cols must be krylovdim + 1, ldv 64 ceil(n / 64)");
    o.krylovkit_max_iter = t->max_cycles; o.arpack_max_iter = t->max_cycles;   // the driver ends the run itself
    const size_t nc = (size_t)t->max_cycles * t->cols;
    std::fill(t->info, t->info + (size_t)t->max_cycles * PROXSDP_OP_INFO, -1);
    std::fill(t->V, t->V + nc * t->ldv, t->sentinel);
    for (double* a : {t->alphas, t->betas, t->D, t->f}) std::fill(a, a + nc, t->sentinel);
    if (pp) prefill_positive_part(*pp, t->ldv, t->sentinel);
    t->npad = t->ldv; t->krylovdim = kdr; t->cycles = 0; t->ell_w = 0; t->overflow_rows = 0;
    Engine E(&o, t->n, pp ? pp->ws_rank : t->nev);
    E.set_resid(t->resid);
    E.S.test_operator_cycles(*t, pp);
}
int proxsdp_hip_operator_cycles(proxsdp_operator_cycles* t) {
    return guarded([&]() -> int { run_operator_cycles(t, nullptr); return 0; });
}

static_assert(sizeof(proxsdp_positive_part) == 192 && offsetof(proxsdp_positive_part, locked) == 48 &&
              offsetof(proxsdp_positive_part, cert_ran) == 96 && offsetof(proxsdp_positive_part, differ) == 120 &&
              offsetof(proxsdp_positive_part, resid2) == 184, "proxsdp_positive_part: the layout tests/test_host_abi.py states");
int proxsdp_hip_positive_part(proxsdp_positive_part* t) {
    return guarded([&]() -> int {
        if (!t) throw std::invalid_argument("NULL argument");
        if (t->struct_size != (int64_t)sizeof(proxsdp_positive_part)) throw std::invalid_argument("positive part: struct_size mismatch");
        if ((t->packed_run != nullptr) == (t->operator_run != nullptr)) throw std::invalid_argument("positive part: one of packed_run and operator_run");
        // (the wrapped struct's own entry code checks its struct_size before a field of it is read; this entry's arguments are
        // checked and its arrays prefilled there too, behind the wrapped struct's)
        if (t->cap < 2 || t->cap > proxsdp::dev::KLD) throw std::invalid_argument("positive part: cap out of range");
        if (t->packed_run) run_lanczos_cycles(t->packed_run, t);
        else run_operator_cycles(t->operator_run, t);
        return 0;
    });
}

int64_t proxsdp_host_block1_lds_doubles(int32_t nt, int32_t fop, int64_t xN, int32_t ell_w_lds) {
    if (nt < 1 || nt > proxsdp::dev::B1_MAXNT || xN < 0 || ell_w_lds < 0 || ell_w_lds > 32) return -1;
    return proxsdp::dev::b1_lds_plan(nt, nt * proxsdp::dev::TILE, fop != 0, xN, ell_w_lds).total;
}

int proxsdp_hip_sign_unpack(const double* packed, int64_t n, double sentinel, double* A, double* sc) {
    return guarded([&]() -> int {
        if (!packed || !A || !sc || n < 1 || n > 4096) throw std::invalid_argument("invalid argument");
        Engine E(nullptr, n, 2);
        E.S.test_sign_unpack(packed, sentinel, A, sc);
        return 0;
    });
}

int proxsdp_hip_dense_scaling(const proxsdp_problem* prob, const proxsdp_options* opt,
                              double* E, double* D, double* frob, double* sigma_max, int32_t* equilibrated) {
    return guarded([&]() -> int {
        if (!prob) throw std::invalid_argument("NULL problem");
        if (!prob->M_dense) throw std::invalid_argument("proxsdp_hip_dense_scaling needs a dense A (M_dense)");
        proxsdp_options o = checked_options(opt);
        o.trace_capacity = 0;
        proxsdp_result dummy{};
        proxsdp::Solver S(*prob, o, dummy);
        S.init_only = true;
        S.run();                                            // returns after the Init section
        const proxsdp::Prep& R = S.P;
        for (int64_t i = 0; E && i < R.Q; ++i) E[i] = R.equilibrated ? R.Ediag[i] : 1.0;
        for (int64_t k = 0; D && k < R.n; ++k) D[k] = R.equilibrated ? R.Ddiag[k] : 1.0;
        if (frob) *frob = S.g_frob;
        if (sigma_max) *sigma_max = S.sigma_max;
        if (equilibrated) *equilibrated = R.equilibrated ? 1 : 0;
        return 0;
    });
}

int proxsdp_hip_primal_update(const double* x, const double* Mty, const double* c, double tau, int64_t n,
                              double* x_out) {
    return guarded([&]() -> int {
        if (n < 0 || (n > 0 && (!x || !Mty || !c || !x_out))) throw std::invalid_argument("invalid argument");
        if (n == 0) return 0;
        Engine E(nullptr, 2, 2);
        hipStream_t st = E.S.stream;
        proxsdp::DevBuf<double> dx(n), dm(n), dc(n), dout(n);
        dx.upload(x, n, st); dm.upload(Mty, n, st); dc.upload(c, n, st);
        hipLaunchKernelGGL(proxsdp::dev::k_primal_update, dim3(proxsdp::grid_for(n)), dim3(proxsdp::dev::TPB), 0, st,
                           dout.p, (const double*)dx.p, (const double*)dm.p, (const double*)dc.p, tau, (long long)n);
        dout.download(x_out, n, st);
        PX_HIP(hipStreamSynchronize(st));
        return 0;
    });
}

int proxsdp_hip_dual_trial(const double* y, const double* Mx, const double* Mx_old, const double* bh,
                           int64_t p, int64_t Q, double bt, double theta, double* y_out, double* ynorm2) {
    return guarded([&]() -> int {
        if (Q <= 0 || p < 0 || p > Q || !y || !Mx || !Mx_old || !bh || !y_out) throw std::invalid_argument("invalid argument");
        Engine E(nullptr, 2, 2);
        hipStream_t st = E.S.stream;
        const int g = std::min(proxsdp::PSTRIDE, proxsdp::grid_for(Q));
        proxsdp::DevBuf<double> dy(Q), d1(Q), d0(Q), dbh(Q), dout(Q), part(proxsdp::PSTRIDE), sc(2);
        dy.upload(y, Q, st); d1.upload(Mx, Q, st); d0.upload(Mx_old, Q, st); dbh.upload(bh, Q, st);
        part.zero(st);
        proxsdp::dev::TrialBatch tb{};               // one linesearch candidate
        tb.nc = 1; tb.bt[0] = bt; tb.theta[0] = theta;
        hipLaunchKernelGGL(proxsdp::dev::k_dual_trial_batch, dim3(g, 1), dim3(proxsdp::dev::TPB), 0, st,
                           (const double*)dy.p, (const double*)d1.p, (const double*)d0.p, (const double*)dbh.p,
                           (int)p, (int)Q, tb, dout.p, (long long)Q, part.p, 0LL);
        hipLaunchKernelGGL(proxsdp::dev::k_combine_multi, dim3(1), dim3(proxsdp::dev::TPB), 0, st,
                           (const double*)part.p, proxsdp::PSTRIDE, g, 0ull, sc.p, 1, (const double*)nullptr, 0, 0, (double*)nullptr);
        dout.download(y_out, Q, st);
        double nrm = 0.0;
        sc.download(&nrm, 1, st);
        PX_HIP(hipStreamSynchronize(st));
        if (ynorm2) *ynorm2 = nrm;
        return 0;
    });
}

int proxsdp_hip_residuals(const double* x, const double* x_old, const double* Mty, const double* Mty_old,
                          const double* c, double tau, int64_t n,
                          const double* y, const double* y_old, const double* Mx, const double* Mx_old,
                          const double* bh, int64_t p, int64_t Q, double sigma, double* out) {
    return guarded([&]() -> int {
        if (n <= 0 || Q <= 0 || p < 0 || p > Q || !x || !x_old || !Mty || !Mty_old || !c || !y || !y_old || !Mx ||
            !Mx_old || !bh || !out) throw std::invalid_argument("invalid argument");
        Engine E(nullptr, 2, 2);
        hipStream_t st = E.S.stream;
        using proxsdp::DevBuf;
        const int gx = std::min(proxsdp::PSTRIDE, proxsdp::grid_for(n)), gq = std::min(proxsdp::PSTRIDE, proxsdp::grid_for(Q));
        DevBuf<double> dx(n), dxo(n), dm(n), dmo(n), dc(n), dy(Q), dyo(Q), d1(Q), d0(Q), dbh(Q);
        DevBuf<double> part((size_t)11 * proxsdp::PSTRIDE), sc(9);
        dx.upload(x, n, st); dxo.upload(x_old, n, st); dm.upload(Mty, n, st); dmo.upload(Mty_old, n, st); dc.upload(c, n, st);
        dy.upload(y, Q, st); dyo.upload(y_old, Q, st); d1.upload(Mx, Q, st); d0.upload(Mx_old, Q, st); dbh.upload(bh, Q, st);
        part.zero(st);
        // one candidate of the linesearch's residual batch: the x part lands in quantities 2..4, the y part in 5..10
        proxsdp::dev::TrialBatch tb{};
        tb.nc = 1; tb.tau[0] = tau; tb.sigma[0] = sigma;
        hipLaunchKernelGGL(proxsdp::dev::k_residual_xy<false>, dim3(std::max(gx, gq), 1, 2), dim3(proxsdp::dev::TPB), 0, st,
                           (const double*)dx.p, (const int*)nullptr, (long long)n, (const double*)dxo.p, 1.0,
                           (const double*)dm.p, (long long)n, (const double*)dmo.p, (const double*)dc.p, gx,
                           (const double*)dy.p, (long long)Q, (const double*)dyo.p, (const double*)d1.p, (const double*)d0.p,
                           (const double*)dbh.p, (int)p, (int)Q, gq, tb, part.p, proxsdp::PSTRIDE, 0LL, (const double*)nullptr);
        // one workgroup per quantity: the x part's three over gx partials, the y part's six over gq
        hipLaunchKernelGGL(proxsdp::dev::k_combine_multi, dim3(3), dim3(proxsdp::dev::TPB), 0, st,
                           (const double*)(part.p + (size_t)2 * proxsdp::PSTRIDE), proxsdp::PSTRIDE, gx, 0x3ull, sc.p, 3,
                           (const double*)nullptr, 0, 0, (double*)nullptr);
        hipLaunchKernelGGL(proxsdp::dev::k_combine_multi, dim3(6), dim3(proxsdp::dev::TPB), 0, st,
                           (const double*)(part.p + (size_t)5 * proxsdp::PSTRIDE), proxsdp::PSTRIDE, gq, 0xFull, sc.p + 3, 6,
                           (const double*)nullptr, 0, 0, (double*)nullptr);
        sc.download(out, 9, st);
        PX_HIP(hipStreamSynchronize(st));
        return 0;
    });
}

int proxsdp_host_symeig(int32_t k, double* a, double* d) {
    return proxsdp_host_symeig_threads(k, a, d, -1);
}

int proxsdp_host_symeig_threads(int32_t k, double* a, double* d, int32_t threads) {
    if (k < 0 || !a || !d) { g_last_error = "invalid argument"; return PROXSDP_E_INVALID; }
    int rc = proxsdp::symeig_dense(k, a, d, false, threads);
    if (rc != 0) { g_last_error = "QL iteration did not converge"; return PROXSDP_E_INTERNAL; }
    return 0;
}

int proxsdp_host_symeig_arrow(int32_t K, int32_t m, const double* D, const double* f,
                              const double* al, const double* be, double* U, double* d) {
    if (K < 2 || m < 1 || m >= K || !D || !f || !al || !be || !U || !d) { g_last_error = "invalid argument"; return PROXSDP_E_INVALID; }
    const int n1 = m + 1;
    std::vector<double> Qa((size_t)n1 * n1, 0.0), da(n1), ea(n1);
    for (int j = 0; j < m; ++j) { Qa[(size_t)j * n1 + j] = D[j]; Qa[(size_t)j * n1 + m] = Qa[(size_t)m * n1 + j] = f[j]; }
    proxsdp::householder_tridiag(n1, Qa.data(), da.data(), ea.data());
    int rc = proxsdp::symeig_tridiag_from(K, m, Qa.data(), da.data(), ea.data(), al, be, U, d);
    if (rc != 0) { g_last_error = "QL iteration did not converge"; return PROXSDP_E_INTERNAL; }
    return 0;
}

int proxsdp_host_symeig_split(int32_t K, int32_t m, int32_t k1, const double* D, const double* f,
                              const double* al, const double* be, double* U, double* d, int32_t* info) {
    return proxsdp_host_symeig_split_threads(K, m, k1, D, f, al, be, 0, U, d, info);
}

int proxsdp_host_symeig_split_threads(int32_t K, int32_t m, int32_t k1, const double* D, const double* f,
                                      const double* al, const double* be, int32_t threads, double* U, double* d, int32_t* info) {
    return guarded([&]() -> int {
        if (K < 2 || m < 0 || m >= K || k1 < 1 || k1 >= K || !al || !be || !U || !d) throw std::invalid_argument("invalid argument");
        proxsdp::SplitEig S;
        std::unique_ptr<proxsdp::SpinPool> pool;
        proxsdp::ParFor par;
        proxsdp::ArmedPool helpers;
        if (threads > 0) {
            pool.reset(new proxsdp::SpinPool(std::min<int>(threads, 15)));
            helpers.arm(pool.get());
            par = [&pool](int n, const std::function<void(int)>& body) { pool->run(n, body); };
            S.M.par = &par;
            S.M.nchunk = std::min<int>(threads, 15) + 1;
        }
        if (S.first(k1, m, D, f, al, be) != 0 || S.second(K, al, be) != 0) throw std::invalid_argument("split eigensolver failed");
        std::vector<int> cols(K);
        for (int c = 0; c < K; ++c) { cols[c] = c; d[c] = S.M.evals[c]; }
        S.M.vectors(cols.data(), K, U);
        if (info) { info[0] = S.M.k; info[1] = (int)S.M.df.size(); info[2] = S.M.max_iter_seen; }
        return 0;
    });
}
int proxsdp_device_symeig_split(int32_t K, int32_t m, int32_t k1, const double* D, const double* f,
                                const double* al, const double* be, double* U, double* d, int32_t* info) {
    return guarded([&]() -> int {
        if (K < 2 || m < 0 || m >= K || k1 < 1 || k1 >= K || !al || !be || !U || !d) throw std::invalid_argument("invalid argument");
        if (!proxsdp::DeviceMerge::eligible(K)) throw std::invalid_argument("device merge serves 2 <= K <= 255");
        proxsdp::SplitEig S;
        if (S.first(k1, m, D, f, al, be) != 0 || S.tail(K, al, be) != 0) throw std::invalid_argument("split eigensolver failed");
        proxsdp::DeviceMerge dm;                             // (declared before the stream: buffers outlive the handle)
        proxsdp::Stream st;
        st.create(hipStreamNonBlocking);
        dm.stage_first(S, st);
        std::vector<double> Dd(K), fd(K);
        const bool ok = dm.run(S, K, 1.0, st, [](hipEvent_t e) { PX_HIP(hipEventSynchronize(e)); }, Dd.data(), fd.data());
        std::vector<double> Ud((size_t)K * K);
        std::vector<int> it(std::max(dm.k, 1), 0);
        dm.Uall.download(Ud.data(), Ud.size(), st);
        if (dm.k > 0) dm.iters_d.download(it.data(), (size_t)dm.k, st);
        PX_HIP(hipStreamSynchronize(st));
        if (!ok) throw std::runtime_error("device merge handed the eigensolve back");
        for (int c = 0; c < K; ++c) {                        // the device's order is descending
            d[c] = Dd[K - 1 - c];
            std::copy(Ud.begin() + (size_t)(K - 1 - c) * K, Ud.begin() + (size_t)(K - c) * K, U + (size_t)c * K);
        }
        if (info) { info[0] = dm.k; info[1] = dm.ndf; info[2] = dm.k > 0 ? *std::max_element(it.begin(), it.end()) : 0; }
        return 0;
    });
}

int proxsdp_host_merge_plan(int32_t K, int32_t m, int32_t k1, const double* D, const double* f, const double* al,
                            const double* be, int32_t with_qf, double* Q1, double* Q2, double* Qf, double* d, double* z,
                            int32_t* colsrc, int32_t* nd, int32_t* rot_idx, double* rot_cs, int32_t* counts) {
    return guarded([&]() -> int {
        if (K < 2 || m < 0 || m >= K || k1 < 1 || k1 >= K || !al || !be || !Q1 || !Q2 || !Qf || !d || !z || !colsrc || !nd ||
            !rot_idx || !rot_cs || !counts) throw std::invalid_argument("invalid argument");
        proxsdp::SplitEig S;
        if (S.first(k1, m, D, f, al, be) != 0 || S.tail(K, al, be) != 0) throw std::invalid_argument("split eigensolver failed");
        const int k2 = K - k1;
        proxsdp::Rank1Merge& M = S.M;
        M.plan(k1, k2, S.Q1.data(), S.d1.data(), S.Q2.data(), S.d2.data(), S.beta, with_qf != 0);
        std::copy(S.Q1.begin(), S.Q1.end(), Q1);
        std::copy(S.Q2.begin(), S.Q2.end(), Q2);
        if (with_qf) std::copy(M.Qf.begin(), M.Qf.end(), Qf);
        std::copy(M.d.begin(), M.d.end(), d);
        std::copy(M.z.begin(), M.z.end(), z);
        std::copy(M.colsrc.begin(), M.colsrc.end(), colsrc);
        std::copy(M.nd.begin(), M.nd.end(), nd);
        for (size_t q = 0; q < M.rots.size(); ++q) {
            rot_idx[2 * q] = M.rots[q].pj; rot_idx[2 * q + 1] = M.rots[q].j;
            rot_cs[2 * q] = M.rots[q].c; rot_cs[2 * q + 1] = M.rots[q].s;
        }
        counts[0] = M.k; counts[1] = (int)M.df.size(); counts[2] = (int)M.rots.size();
        return 0;
    });
}

int proxsdp_host_start_vector(int64_t n, int64_t seed, int32_t init, double* out) {
    if (n < 0 || !out) { g_last_error = "invalid argument"; return PROXSDP_E_INVALID; }
    proxsdp::start_vector(n, (uint64_t)seed, init, out);
    return 0;
}

int proxsdp_host_preprocess(const proxsdp_problem* prob, int64_t* order, int64_t* var_ordering,
                            double* c_scaled, double* frobenius_norm_M) {
    return guarded([&]() -> int {
        if (!prob) throw std::invalid_argument("NULL problem");
        proxsdp::Prep R = proxsdp::prepare(*prob, nullptr, prob->reduce_fn != nullptr || prob->nccl_comm != nullptr);
        for (int64_t i = 0; i < R.n; ++i) {
            if (order) order[i] = R.ord[i];
            if (var_ordering) var_ordering[i] = R.inv[i];
            if (c_scaled) c_scaled[i] = R.c[i];
        }
        if (frobenius_norm_M) *frobenius_norm_M = R.frob;
        return 0;
    });
}

int proxsdp_host_model_prepare(const proxsdp_problem* prob, proxsdp_model_dump* out, int64_t* nnz_A, int32_t* csc_pos,
                               int32_t* csr_pos) {
    return guarded([&]() -> int {
        if (!prob || !out) throw std::invalid_argument("NULL problem or dump");
        proxsdp::check_struct_size(out, "proxsdp_model_dump");
        if (is_shard(prob) || prob->M_dense) throw std::domain_error("proxsdp_host_model_prepare does not serve a shard of a block-sharded solve or M_dense");
        const proxsdp::Prep R = proxsdp::prepare(*prob, nullptr, false, true);
        std::vector<int32_t> supp;
        for (int64_t k = 0; k < R.n; ++k)
            if (R.colptr[k + 1] > R.colptr[k] || R.c[k] != 0.0) supp.push_back((int32_t)k);
        out->n = R.n; out->Q = R.Q; out->nnz = R.nnz; out->ns = (int64_t)supp.size();
        out->norms[0] = R.norm_b; out->norms[1] = R.norm_h; out->norms[2] = R.norm_c; out->norms[3] = R.frob;
        if (nnz_A) *nnz_A = R.nnzA;
        for (int64_t q = 0; q < R.nnz; ++q) {
            if (out->csc_val) out->csc_val[q] = R.val[q];
            if (out->csr_val) out->csr_val[q] = R.rval[q];
            if (out->csc_val_orig) out->csc_val_orig[q] = R.val_orig[q];
            if (out->csr_val_orig) out->csr_val_orig[R.csr_pos[q]] = R.val_orig[R.csc_pos[q]];
            if (csc_pos) csc_pos[q] = R.csc_pos[q];
            if (csr_pos) csr_pos[q] = R.csr_pos[q];
        }
        for (int64_t k = 0; k < R.n; ++k) {
            if (out->c) out->c[k] = R.c[k];
            if (out->c_orig) out->c_orig[k] = R.c_orig[k];
        }
        for (int64_t i = 0; i < R.Q && out->bh; ++i) out->bh[i] = i < R.p ? R.b[i] : R.h[i - R.p];
        for (size_t q = 0; q < supp.size(); ++q) {
            if (out->support) out->support[q] = supp[q];
            if (out->cS) out->cS[q] = R.c[supp[q]];
        }
        return 0;
    });
}

int proxsdp_host_model_rows_plan(const proxsdp_problem* prob, proxsdp_model_rows* ch, proxsdp_model_dump* out,
                                 int32_t* csc_src, int32_t* csr_src, int32_t* bh_src, int32_t* csc_pos, int32_t* csr_pos) {
    return guarded([&]() -> int {
        proxsdp::check_rows_struct(ch);
        if (ch->on_device != 0) throw std::invalid_argument("proxsdp_host_model_rows_plan takes host values (on_device = 0)");
        if (!prob || !out) throw std::invalid_argument("NULL problem or dump");
        proxsdp::check_struct_size(out, "proxsdp_model_dump");
        if (is_shard(prob) || prob->M_dense) throw std::domain_error("proxsdp_host_model_rows_plan does not serve a shard of a block-sharded solve or M_dense");
        const proxsdp::Prep P = proxsdp::prepare(*prob, nullptr, false, true);
        proxsdp::RowsPlan pl = proxsdp::plan_rows(P, prob->index_base, *ch);
        std::vector<double> rorig;
        proxsdp::apply_rows_host(P, pl, ch->add_val, ch->add_h, rorig);
        const proxsdp::Prep& R = pl.R;
        std::vector<int32_t> supp;
        for (int64_t k = 0; k < R.n; ++k)
            if (R.colptr[k + 1] > R.colptr[k] || P.c[k] != 0.0) supp.push_back((int32_t)k);
        out->n = R.n; out->Q = R.Q; out->nnz = R.nnz; out->ns = (int64_t)supp.size();
        out->norms[0] = P.norm_b; out->norms[1] = R.norm_h; out->norms[2] = P.norm_c; out->norms[3] = R.frob;
        for (int64_t q = 0; q < R.nnz; ++q) {
            if (out->csc_val) out->csc_val[q] = R.val[q];
            if (out->csr_val) out->csr_val[q] = R.rval[q];
            if (out->csc_val_orig) out->csc_val_orig[q] = R.val_orig[q];
            if (out->csr_val_orig) out->csr_val_orig[q] = rorig[q];
            if (csc_src) csc_src[q] = pl.csc_src[q];
            if (csr_src) csr_src[q] = pl.csr_src[q];
            if (csc_pos) csc_pos[q] = R.csc_pos[q];
            if (csr_pos) csr_pos[q] = R.csr_pos[q];
        }
        for (int64_t k = 0; k < R.n; ++k) {
            if (out->c) out->c[k] = P.c[k];
            if (out->c_orig) out->c_orig[k] = P.c_orig[k];
        }
        for (int64_t i = 0; i < R.Q; ++i) {
            if (out->bh) out->bh[i] = i < R.p ? P.b[i] : R.h[i - R.p];
            if (bh_src) bh_src[i] = pl.bh_src[i];
        }
        for (size_t q = 0; q < supp.size(); ++q) {
            if (out->support) out->support[q] = supp[q];
            if (out->cS) out->cS[q] = P.c[supp[q]];
        }
        ch->m_new = R.m; ch->nnz_new = R.nnz; ch->support_rebuilt = 0; ch->bytes_allocated = 0; ch->seconds = 0.0;
        if (ch->kept) std::copy(pl.kept.begin(), pl.kept.end(), ch->kept);
        return 0;
    });
}

int proxsdp_host_split_shard(const proxsdp_problem* prob, int32_t n_shards, const int32_t* psd_owner,
                             const int32_t* soc_owner, const int32_t* free_owner, int32_t shard, proxsdp_shard* out) {
    return guarded([&]() -> int {
        if (!prob || !out) throw std::invalid_argument("NULL problem or output");
        if (out->struct_size != (int64_t)sizeof(proxsdp_shard)) throw std::invalid_argument("proxsdp_shard.struct_size mismatch");
        const proxsdp::ShardPlan L = proxsdp::plan_shards(*prob, n_shards, psd_owner, soc_owner, free_owner);
        if (shard < 0 || shard >= n_shards) throw std::invalid_argument("shard outside 0 .. n_shards - 1");
        const proxsdp::ShardData S = proxsdp::split_shard(*prob, L, shard);
        out->n = (int64_t)S.vars.size(); out->p = (int64_t)S.rows_eq.size(); out->m = (int64_t)S.rows_in.size();
        out->nnz_A = (int64_t)S.A_rowval.size(); out->nnz_G = (int64_t)S.G_rowval.size();
        out->n_coupling = (int64_t)S.coup_rows.size();
        out->n_psd = (int64_t)S.psd_ids.size(); out->len_psd = (int64_t)S.psd_idx.size();
        out->n_soc = (int64_t)S.soc_ids.size(); out->len_soc = (int64_t)S.soc_idx.size();
        out->len_eig = (int64_t)S.eig_resid.size();
        auto put = [](const auto& v, auto* dst) { if (dst) std::copy(v.begin(), v.end(), dst); };
        put(S.vars, out->vars); put(S.rows_eq, out->rows_eq); put(S.rows_in, out->rows_in);
        put(S.coup_rows, out->coupling_rows); put(S.coup_owned, out->coupling_owned);
        put(S.A_colptr, out->A_colptr); put(S.A_rowval, out->A_rowval); put(S.A_nzval, out->A_nzval);
        put(S.G_colptr, out->G_colptr); put(S.G_rowval, out->G_rowval); put(S.G_nzval, out->G_nzval);
        put(S.b, out->b); put(S.h, out->h); put(S.c, out->c);
        put(S.psd_ids, out->psd_ids); put(S.psd_ptr, out->psd_ptr); put(S.psd_idx, out->psd_idx);
        put(S.soc_ids, out->soc_ids); put(S.soc_ptr, out->soc_ptr); put(S.soc_idx, out->soc_idx);
        put(S.eig_resid, out->eig_resid);
        return 0;
    });
}

int proxsdp_host_group_reduce(int32_t n_shards, int32_t rounds, int32_t nsum, int32_t nmax, const double* records,
                              int32_t leave_shard, int32_t leave_after, double timeout_s,
                              double* out, int32_t* rounds_done, int32_t* failed) {
    return guarded([&]() -> int {
        if (n_shards < 1 || n_shards > 256 || rounds < 0 || nsum < 0 || nmax < 0 || nsum + nmax < 1 || !records || !out ||
            !rounds_done || !failed || leave_shard >= n_shards)
            throw std::invalid_argument("invalid argument");
        const size_t w = (size_t)nsum + (size_t)nmax;
        proxsdp::ShardGroup group(n_shards, timeout_s);
        auto body = [&](int s) {
            rounds_done[s] = 0; failed[s] = 0;
            try {
                for (int k = 0; k < rounds; ++k) {
                    if (s == leave_shard && k == leave_after) break;
                    const double* rec = records + ((size_t)k * n_shards + s) * w;
                    std::vector<double> sums(rec, rec + nsum), maxs(rec + nsum, rec + w);
                    group.reduce(s, sums, maxs);
                    double* o = out + ((size_t)s * rounds + k) * w;
                    std::copy(sums.begin(), sums.end(), o);
                    std::copy(maxs.begin(), maxs.end(), o + nsum);
                    rounds_done[s] = k + 1;
                }
            } catch (...) { failed[s] = 1; }
            group.leave();
        };
        run_shard_threads(n_shards, group, body);
        return 0;
    });
}

int proxsdp_host_equilibrate_rowsums(const double* rowsums, int64_t Q, int64_t n, const proxsdp_options* opt,
                                     double* E, double* d) {
    return guarded([&]() -> int {
        if (Q <= 0 || n <= 0 || !rowsums || !E || !d) throw std::invalid_argument("invalid argument");
        const proxsdp_options o = checked_options(opt);
        std::vector<double> Ed;
        proxsdp::equilibrate_rowsums(rowsums, Q, n, o, Ed, *d);
        std::copy(Ed.begin(), Ed.end(), E);
        return 0;
    });
}

#ifdef PX_TIMELINE
// measurement builds only (tools/timeline/): copy of the step kernels' stamp table
int proxsdp_hip_debug_timeline(unsigned long long* out, int64_t count, int32_t clear) {
    return guarded([&]() -> int {
        const size_t total = sizeof(proxsdp::dev::g_tl) / sizeof(unsigned long long);
        if (out && count > 0)
            PX_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(proxsdp::dev::g_tl), std::min<size_t>(total, (size_t)count) * sizeof(unsigned long long)));
        if (clear) {
            void* p = nullptr;
            PX_HIP(hipGetSymbolAddress(&p, HIP_SYMBOL(proxsdp::dev::g_tl)));
            PX_HIP(hipMemset(p, 0, sizeof(proxsdp::dev::g_tl)));
        }
        return (int)std::min<size_t>(total, (size_t)1 << 30);
    });
}
#endif

}  // extern "C"
