// Host-side split of a whole model into the shards of a block-sharded solve, and the gather of their results (no HIP
// calls here).  The C++ restatement of proxsdp_jl_amd/sharded.py (default_owners, variable_owners, split_block_diagonal,
// gather_solution) behind proxsdp_hip_solve_sharded: shard s holds the cones assigned to it (a cone is never split), the
// free variables assigned to it, the rows of A and G whose entries all lie in its variables (PRIVATE rows) and every
// COUPLING row (entries in the variables of more than one shard) restricted to its own columns, with the same
// right-hand side on every shard; the lowest shard that touches a coupling row owns it.  A row without entries belongs
// to shard 0.  The caller's row and variable order is kept inside a shard.
#pragma once
#include <algorithm>
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>
#include "prep.hpp"

namespace proxsdp {

// one shard's sub-problem, 0-based throughout, plus its maps into the caller's numbering
struct ShardData {
    std::vector<int64_t> vars, rows_eq, rows_in;          // the caller's variable / row numbers, ascending
    std::vector<int64_t> coup_rows;                       // coupling rows in the SHARD's row numbering (equalities first)
    std::vector<int32_t> coup_owned;
    std::vector<int64_t> A_colptr, A_rowval, G_colptr, G_rowval;
    std::vector<double> A_nzval, G_nzval, b, h, c;
    std::vector<int64_t> psd_ids, psd_ptr, psd_idx, soc_ids, soc_ptr, soc_idx;   // *_ids: the caller's cone numbers
    std::vector<double> eig_resid;                        // the caller's start vectors of this shard's PSD cones (or empty)
    // proxsdp_problem over the vectors above (valid while this object lives and is not modified)
    proxsdp_problem problem() const {
        proxsdp_problem P{};
        P.n = (int64_t)vars.size(); P.p = (int64_t)rows_eq.size(); P.m = (int64_t)rows_in.size();
        P.A = proxsdp_csc{P.p, P.n, A_colptr.data(), A_rowval.data(), A_nzval.data()};
        P.G = proxsdp_csc{P.m, P.n, G_colptr.data(), G_rowval.data(), G_nzval.data()};
        P.b = b.data(); P.h = h.data(); P.c = c.data();
        P.n_psd = (int64_t)psd_ids.size(); P.psd_ptr = psd_ptr.data(); P.psd_idx = psd_idx.data();
        P.n_soc = (int64_t)soc_ids.size(); P.soc_ptr = soc_ptr.data(); P.soc_idx = soc_idx.data();
        P.index_base = 0;
        P.eig_resid = eig_resid.empty() ? nullptr : eig_resid.data();
        P.n_coupling = (int64_t)coup_rows.size();
        P.coupling_rows = coup_rows.empty() ? nullptr : coup_rows.data();
        P.coupling_owned = coup_owned.empty() ? nullptr : coup_owned.data();
        return P;
    }
};

// the owner maps of one call: validated, defaults filled in
struct ShardPlan {
    int n_shards = 1;
    std::vector<int32_t> psd_owner, soc_owner, free_owner, var_owner;
    std::vector<int64_t> free_vars;                       // ids of the variables outside every cone, ascending
};

// Everything proxsdp_hip_solve_sharded rejects before a thread starts (and proxsdp_host_split_shard with it): a model that
// is itself a shard, a dense A, an owner outside 0 .. n_shards - 1, a variable in two cones, a shard without variables.
// Owner lists left NULL take sharded.default_owners' values: ONE round-robin over the PSD cones, then the SOC cones, then
// the free variables in ascending id.
inline ShardPlan plan_shards(const proxsdp_problem& P, int32_t n_shards, const int32_t* psd_owner, const int32_t* soc_owner,
                             const int32_t* free_owner) {
    if (n_shards < 1) throw std::invalid_argument("n_shards must be >= 1");
    if (P.reduce_fn != nullptr || P.reduce_vec_fn != nullptr || P.nccl_comm != nullptr || P.n_coupling != 0)
        throw std::invalid_argument("the model of an in-process sharded solve must not itself be a shard "
                                    "(reduce_fn, reduce_vec_fn, nccl_comm and n_coupling must be unset)");
    if (P.M_dense != nullptr) throw std::invalid_argument("A_dense cannot be combined with a block-sharded solve");
    const int base = P.index_base;
    if (base != 0 && base != 1) throw std::invalid_argument("index_base must be 0 or 1");
    if (P.n < 0 || P.p < 0 || P.m < 0) throw std::invalid_argument("negative dimension");
    if (P.n >= (int64_t)1 << 31) throw std::invalid_argument("n >= 2^31 not supported");
    if (P.p + P.m >= (int64_t)1 << 31) throw std::invalid_argument("p + m >= 2^31 not supported");
    check_csc(P.A, P.p, P.n, base, "A");
    check_csc(P.G, P.m, P.n, base, "G");
    if ((P.p > 0 && !P.b) || (P.m > 0 && !P.h) || (P.n > 0 && !P.c)) throw std::invalid_argument("b, h or c is NULL");
    if (P.n_psd < 0 || P.n_soc < 0) throw std::invalid_argument("negative cone count");
    if (P.n_psd > 0 && (!P.psd_ptr || !P.psd_idx)) throw std::invalid_argument("psd_ptr/psd_idx is NULL");
    if (P.n_soc > 0 && (!P.soc_ptr || !P.soc_idx)) throw std::invalid_argument("soc_ptr/soc_idx is NULL");
    ShardPlan L;
    L.n_shards = n_shards;
    auto owner_ok = [&](int64_t o) {
        if (o < 0 || o >= n_shards) throw std::invalid_argument("owner outside 0 .. n_shards - 1");
        return (int32_t)o;
    };
    L.var_owner.assign(P.n, -1);
    L.psd_owner.resize(P.n_psd); L.soc_owner.resize(P.n_soc);
    for (int64_t k = 0; k < P.n_psd; ++k) L.psd_owner[k] = owner_ok(psd_owner ? psd_owner[k] : k % n_shards);
    for (int64_t j = 0; j < P.n_soc; ++j) L.soc_owner[j] = owner_ok(soc_owner ? soc_owner[j] : (P.n_psd + j) % n_shards);
    auto cones = [&](int64_t cnt, const int64_t* ptr, const int64_t* idx, const std::vector<int32_t>& own, const char* what) {
        for (int64_t k = 0; k < cnt; ++k) {
            if (ptr[k + 1] <= ptr[k]) throw std::invalid_argument(std::string("empty ") + what + " cone");
            for (int64_t q = ptr[k]; q < ptr[k + 1]; ++q) {
                const int64_t v = idx[q] - base;
                if (v < 0 || v >= P.n) throw std::invalid_argument(std::string(what) + " cone variable out of range");
                if (L.var_owner[v] >= 0) throw std::invalid_argument("a variable belongs to more than one cone");
                L.var_owner[v] = own[k];
            }
        }
    };
    cones(P.n_psd, P.psd_ptr, P.psd_idx, L.psd_owner, "PSD");
    cones(P.n_soc, P.soc_ptr, P.soc_idx, L.soc_owner, "SOC");
    for (int64_t v = 0; v < P.n; ++v) if (L.var_owner[v] < 0) L.free_vars.push_back(v);
    L.free_owner.resize(L.free_vars.size());
    for (size_t i = 0; i < L.free_vars.size(); ++i) {
        L.free_owner[i] = owner_ok(free_owner ? free_owner[i] : (int64_t)((P.n_psd + P.n_soc + (int64_t)i) % n_shards));
        L.var_owner[L.free_vars[i]] = L.free_owner[i];
    }
    std::vector<int64_t> held(n_shards, 0);
    for (int64_t v = 0; v < P.n; ++v) held[L.var_owner[v]]++;
    for (int s = 0; s < n_shards; ++s)
        if (held[s] == 0)
            throw std::invalid_argument("shard " + std::to_string(s) + " of " + std::to_string(n_shards) +
                                        " would own no variable: every shard must own at least one");
    return L;
}

// rows of one matrix (A or G) for shard `rank`: the selected caller rows (original order), the shard's CSC restricted to
// its columns, the positions of the coupling rows inside the selection and their owned flags
inline void split_rows(const proxsdp_csc& M, int base, const ShardPlan& L, int rank, const std::vector<int64_t>& mine,
                       std::vector<int64_t>& sel, std::vector<int64_t>& colptr, std::vector<int64_t>& rowval,
                       std::vector<double>& nzval, std::vector<int64_t>& local, std::vector<int32_t>& owned) {
    const int64_t rows = M.nrows, cols = M.ncols;
    const int32_t none = std::numeric_limits<int32_t>::max();
    std::vector<int32_t> omin(rows, none), omax(rows, -1);
    for (int64_t j = 0; j < cols; ++j)
        for (int64_t q = M.colptr[j] - base; q < M.colptr[j + 1] - base; ++q) {
            const int64_t r = M.rowval[q] - base;
            omin[r] = std::min(omin[r], L.var_owner[j]);
            omax[r] = std::max(omax[r], L.var_owner[j]);
        }
    std::vector<int64_t> pos(rows, -1);
    for (int64_t r = 0; r < rows; ++r) {
        if (omax[r] < 0) omin[r] = omax[r] = 0;           // a row without entries belongs to shard 0
        const bool coupled = omin[r] != omax[r];
        if (!coupled && omax[r] != rank) continue;
        pos[r] = (int64_t)sel.size();
        if (coupled) { local.push_back(pos[r]); owned.push_back(omin[r] == rank ? 1 : 0); }
        sel.push_back(r);
    }
    colptr.assign(mine.size() + 1, 0);
    for (size_t k = 0; k < mine.size(); ++k) {
        const int64_t j = mine[k];
        for (int64_t q = M.colptr[j] - base; q < M.colptr[j + 1] - base; ++q) {
            rowval.push_back(pos[M.rowval[q] - base]);    // (every row with an entry in one of `mine` is selected)
            nzval.push_back(M.nzval[q]);
        }
        colptr[k + 1] = (int64_t)rowval.size();
    }
}

inline ShardData split_shard(const proxsdp_problem& P, const ShardPlan& L, int rank) {
    ShardData S;
    const int base = P.index_base;
    std::vector<int64_t> remap(P.n, -1);
    for (int64_t v = 0; v < P.n; ++v)
        if (L.var_owner[v] == rank) { remap[v] = (int64_t)S.vars.size(); S.vars.push_back(v); }
    std::vector<int64_t> ca, cg;
    std::vector<int32_t> oa, og;
    split_rows(P.A, base, L, rank, S.vars, S.rows_eq, S.A_colptr, S.A_rowval, S.A_nzval, ca, oa);
    split_rows(P.G, base, L, rank, S.vars, S.rows_in, S.G_colptr, S.G_rowval, S.G_nzval, cg, og);
    for (int64_t r : S.rows_eq) S.b.push_back(P.b[r]);
    for (int64_t r : S.rows_in) S.h.push_back(P.h[r]);
    for (int64_t v : S.vars) S.c.push_back(P.c[v]);
    S.coup_rows = ca;
    for (int64_t r : cg) S.coup_rows.push_back((int64_t)S.rows_eq.size() + r);
    S.coup_owned = oa;
    S.coup_owned.insert(S.coup_owned.end(), og.begin(), og.end());
    auto cones = [&](int64_t cnt, const int64_t* ptr, const int64_t* idx, const std::vector<int32_t>& own,
                     std::vector<int64_t>& ids, std::vector<int64_t>& sptr, std::vector<int64_t>& sidx) {
        sptr.assign(1, 0);
        for (int64_t k = 0; k < cnt; ++k) {
            if (own[k] != rank) continue;
            ids.push_back(k);
            for (int64_t q = ptr[k]; q < ptr[k + 1]; ++q) sidx.push_back(remap[idx[q] - base]);
            sptr.push_back((int64_t)sidx.size());
        }
    };
    cones(P.n_psd, P.psd_ptr, P.psd_idx, L.psd_owner, S.psd_ids, S.psd_ptr, S.psd_idx);
    cones(P.n_soc, P.soc_ptr, P.soc_idx, L.soc_owner, S.soc_ids, S.soc_ptr, S.soc_idx);
    if (P.eig_resid != nullptr) {                         // start vectors: one per PSD cone, sides concatenated
        const double* ur = P.eig_resid;
        for (int64_t k = 0; k < P.n_psd; ++k) {
            const int64_t len = P.psd_ptr[k + 1] - P.psd_ptr[k];
            int64_t side = 0;
            while (side * (side + 1) / 2 < len) ++side;
            if (L.psd_owner[k] == rank) S.eig_resid.insert(S.eig_resid.end(), ur, ur + side);
            ur += side;
        }
    }
    return S;
}

// gather_solution: shard vectors (local, lengths n_s / p_s / m_s) into the whole model's (caller-allocated, may be NULL).
// A private row comes from its shard, a coupling row from the shard that owns it.
inline void gather_shard(const ShardData& S, const double* primal, const double* dual_cone, const double* dual_eq,
                         const double* dual_in, const double* slack_eq, const double* slack_in, proxsdp_result& out) {
    const size_t p_loc = S.rows_eq.size();
    std::vector<char> own_eq(p_loc, 1), own_in(S.rows_in.size(), 1);
    for (size_t k = 0; k < S.coup_rows.size(); ++k) {
        const size_t r = (size_t)S.coup_rows[k];
        if (r < p_loc) own_eq[r] = (char)(S.coup_owned[k] != 0);
        else own_in[r - p_loc] = (char)(S.coup_owned[k] != 0);
    }
    for (size_t k = 0; k < S.vars.size(); ++k) {
        if (out.primal) out.primal[S.vars[k]] = primal[k];
        if (out.dual_cone) out.dual_cone[S.vars[k]] = dual_cone[k];
    }
    for (size_t k = 0; k < p_loc; ++k) {
        if (!own_eq[k]) continue;
        if (out.dual_eq) out.dual_eq[S.rows_eq[k]] = dual_eq[k];
        if (out.slack_eq) out.slack_eq[S.rows_eq[k]] = slack_eq[k];
    }
    for (size_t k = 0; k < S.rows_in.size(); ++k) {
        if (!own_in[k]) continue;
        if (out.dual_in) out.dual_in[S.rows_in[k]] = dual_in[k];
        if (out.slack_in) out.slack_in[S.rows_in[k]] = slack_in[k];
    }
}

}  // namespace proxsdp
