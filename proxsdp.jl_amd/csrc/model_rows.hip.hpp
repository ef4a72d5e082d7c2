// Inequality rows of a model handle added and dropped in place (proxsdp_hip_model_rows; model.hip.hpp).  No line of the
// reference stands behind this file: ProxSDP rebuilds AffineSets, ConicSets and every workspace per optimize!
// (/root/reference/src/MOI_wrapper.jl:220-342), so a cutting-plane round costs a whole set-up there.
//
// Host.  plan_rows() takes the handle's Prep and the change and gives the members of the Prep that change -- the pattern of
// M = [A; G'] in both orientations, the position maps, m, Q, nnz -- exactly as prepare() gives them for
//     G' = [the rows of G that stay, in their old order; the new rows in the order given]
// stored column by column: a column's kept entries in the order they are stored now, then its new entries by ascending new
// row (the entries of one row and column in the order the row lists them).  With the pattern come the SOURCE maps: for every
// position of the new value arrays and of [b; h'], where its number comes from -- q >= 0: position q of the old array;
// -1 - t: entry t of the caller's add_val (add_h).  Nothing here reads a value, so the plan is the same on both routes.
//
// Device.  Two kernels move the numbers: k_rows_values (one launch per orientation) gathers the unscaled and the scaled
// array of that orientation through the source map -- a kept entry is copied from the two old arrays, a new entry is the
// caller's number and ONE product with its column's factor (sqrt(2)/2 on off-diagonal PSD columns, 1.0 elsewhere, contraction
// off: k_model_values' arithmetic) -- and k_rows_bh forms [b; h'] for the loop and the exit path.  Kept values never visit
// the host.  Both are plain grid-stride gathers: the map and the outputs are contiguous per wavefront, the reads of the old
// arrays follow the map.
#pragma once
#include "model_update.hip.hpp"
#include "struct_check.hpp"

namespace proxsdp {
namespace dev {

#pragma clang fp contract(off)
// position w of a new value array (cnt of them): src[w] >= 0 copies old_orig / old_scaled [src[w]]; src[w] = -1 - t takes
// add_val[t], unscaled into out_orig and times the factor of its column add_k[t] (solver order) into out_scaled
__global__ void __launch_bounds__(TPB)
k_rows_values(const int* __restrict__ src, long long cnt, const double* __restrict__ old_orig, const double* __restrict__ old_scaled,
              const double* __restrict__ add_val, const int* __restrict__ add_k, const unsigned char* __restrict__ offdiag,
              double cte, double* __restrict__ out_orig, double* __restrict__ out_scaled) {
    const long long stride = (long long)gridDim.x * TPB;
    for (long long w = (long long)blockIdx.x * TPB + threadIdx.x; w < cnt; w += stride) {
        const int s = src[w];
        double v, sv;
        if (s >= 0) { v = old_orig[s]; sv = old_scaled[s]; }
        else {
            const int t = -1 - s;
            v = add_val[t];
            sv = v * (offdiag[add_k[t]] ? cte : 1.0);
        }
        out_orig[w] = v; out_scaled[w] = sv;
    }
}

// row i of the new [b; h'] (Q of them): src[i] >= 0 copies old_bh[src[i]], src[i] = -1 - t takes add_h[t]; into the loop's and
// the exit path's vector (the two are equal: an equilibrated model takes no row change)
__global__ void __launch_bounds__(TPB)
k_rows_bh(const int* __restrict__ src, long long Q, const double* __restrict__ old_bh, const double* __restrict__ add_h,
          double* __restrict__ bh, double* __restrict__ bh_exit) {
    const long long stride = (long long)gridDim.x * TPB;
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < Q; i += stride) {
        const int s = src[i];
        const double v = s >= 0 ? old_bh[s] : add_h[-1 - s];
        bh[i] = v; bh_exit[i] = v;
    }
}
#pragma clang fp contract(fast)

}  // namespace dev

// ---- the checks of a change that need no model (capi.hip runs them before it looks at the handle)
inline void check_rows_struct(const proxsdp_model_rows* ch) {
    if (!ch) throw std::invalid_argument("NULL change");
    check_struct_size(ch, "proxsdp_model_rows");
    if (ch->on_device != 0 && ch->on_device != 1) throw std::invalid_argument("proxsdp_model_rows.on_device must be 0 or 1");
    if (ch->n_drop < 0 || ch->n_add < 0) throw std::invalid_argument("proxsdp_model_rows: negative n_drop or n_add");
    if (ch->n_drop == 0 && ch->n_add == 0) throw std::invalid_argument("proxsdp_model_rows: n_drop and n_add are both 0");
    if (ch->n_drop > 0 && !ch->drop) throw std::invalid_argument("proxsdp_model_rows: drop is NULL");
    if (ch->n_add > 0) {
        if (!ch->add_ptr) throw std::invalid_argument("proxsdp_model_rows: add_ptr is NULL");
        if (!ch->add_h) throw std::invalid_argument("proxsdp_model_rows: add_h is NULL");
        if (ch->add_ptr[0] != 0) throw std::invalid_argument("proxsdp_model_rows: add_ptr[0] != 0");
        for (int64_t r = 0; r < ch->n_add; ++r)
            if (ch->add_ptr[r + 1] < ch->add_ptr[r]) throw std::invalid_argument("proxsdp_model_rows: add_ptr not monotone");
        const int64_t na = ch->add_ptr[ch->n_add];
        if (na > 0 && (!ch->add_col || !ch->add_val)) throw std::invalid_argument("proxsdp_model_rows: add_col / add_val is NULL");
        if (ch->on_device == 0) {
            for (int64_t t = 0; t < na; ++t)
                if (!std::isfinite(ch->add_val[t])) throw std::invalid_argument("proxsdp_model_rows: non-finite entry in add_val");
            for (int64_t r = 0; r < ch->n_add; ++r)
                if (!std::isfinite(ch->add_h[r])) throw std::invalid_argument("proxsdp_model_rows: non-finite entry in add_h");
        }
    }
}

struct RowsPlan {
    Prep R;                                     // what changes of the Prep -- m, Q, nnz, the pattern in both orientations, the
                                                // position maps, the value arrays and h (sized, not filled) -- and nothing
                                                // else: the n-sized members stay where they are (commit_rows)
    std::vector<int32_t> touched;               // solver-order columns that lost or gained an entry (repeats possible)
    std::vector<int32_t> csc_src, csr_src;      // per position of the new val / rval (see the head of the file)
    std::vector<int32_t> bh_src;                // per row of the new [b; h']
    std::vector<int32_t> add_k;                 // per entry of add_val: its column in solver order
    std::vector<int64_t> kept;                  // per new inequality row: the old row, -1 for an added one
    int64_t nnz_add = 0;
};

// The checks that need the model, then the plan.  base: the index base of create (add_col follows it; drop is 0-based).
inline RowsPlan plan_rows(const Prep& P, int base, const proxsdp_model_rows& ch) {
    const int64_t n = P.n, p = P.p, m = P.m, nd = ch.n_drop, na = ch.n_add;
    std::vector<int64_t> newrow((size_t)m, 0);                  // old inequality row -> new one, -1 dropped
    for (int64_t k = 0; k < nd; ++k) {
        const int64_t r = ch.drop[k];
        if (r < 0 || r >= m) throw std::invalid_argument("proxsdp_model_rows: drop number out of range");
        if (newrow[r] < 0) throw std::invalid_argument("proxsdp_model_rows: drop number repeated");
        newrow[r] = -1;
    }
    const int64_t nnz_add = na > 0 ? ch.add_ptr[na] : 0;
    for (int64_t t = 0; t < nnz_add; ++t) {
        const int64_t j = ch.add_col[t] - base;
        if (j < 0 || j >= n) throw std::invalid_argument("proxsdp_model_rows: column out of range");
    }
    RowsPlan pl;
    pl.nnz_add = nnz_add;
    const int64_t mk = m - nd, m2 = mk + na, Q2 = p + m2;
    if (Q2 >= (int64_t)1 << 31) throw std::invalid_argument("p + m >= 2^31 not supported");
    pl.kept.reserve((size_t)m2);
    for (int64_t r = 0; r < m; ++r)
        if (newrow[r] >= 0) { newrow[r] = (int64_t)pl.kept.size(); pl.kept.push_back(r); }
    pl.kept.resize((size_t)m2, -1);
    int64_t nnz_drop = 0;
    for (int64_t q = 0; q < P.nnz; ++q)
        if (P.rowidx[q] >= p && newrow[P.rowidx[q] - p] < 0) ++nnz_drop;
    const int64_t nnz2 = P.nnz - nnz_drop + nnz_add;
    if (nnz2 >= ((int64_t)1 << 31) - 1) throw std::invalid_argument("nnz(M) >= 2^31 not supported by the sparse path");

    // the new entries by column (solver order), rows ascending, a row's entries in the order it lists them: a stable
    // counting sort of t = 0, 1, ... by column
    pl.add_k.resize((size_t)nnz_add);
    std::vector<int64_t> astart((size_t)n + 1, 0);
    for (int64_t t = 0; t < nnz_add; ++t) {
        pl.add_k[t] = (int32_t)P.inv[ch.add_col[t] - base];
        astart[pl.add_k[t] + 1]++;
    }
    for (int64_t k = 0; k < n; ++k) astart[k + 1] += astart[k];
    std::vector<int64_t> alist((size_t)nnz_add), arow((size_t)nnz_add);
    {
        std::vector<int64_t> cur(astart.begin(), astart.end() - 1);
        for (int64_t r = 0; r < na; ++r)
            for (int64_t t = ch.add_ptr[r]; t < ch.add_ptr[r + 1]; ++t) { alist[cur[pl.add_k[t]]++] = t; arow[t] = r; }
    }

    // ---- the reordered CSC of [A; G'] and where its values come from
    Prep& R = pl.R;
    R.n = n; R.p = p; R.m = m2; R.Q = Q2; R.nnz = nnz2; R.nnzA = P.nnzA;
    R.colptr.assign((size_t)n + 1, 0);
    R.rowidx.assign((size_t)nnz2, 0);
    pl.csc_src.assign((size_t)nnz2, 0);
    std::vector<int32_t> old_to_new((size_t)P.nnz, -1);
    int64_t w = 0;
    for (int64_t k = 0; k < n; ++k) {
        R.colptr[k] = w;
        for (int64_t q = P.colptr[k]; q < P.colptr[k + 1]; ++q) {
            int64_t row = P.rowidx[q];
            if (row >= p) {
                const int64_t nr = newrow[row - p];
                if (nr < 0) { pl.touched.push_back((int32_t)k); continue; }
                row = p + nr;
            }
            R.rowidx[w] = (int32_t)row; pl.csc_src[w] = (int32_t)q; old_to_new[q] = (int32_t)w; ++w;
        }
        for (int64_t a = astart[k]; a < astart[k + 1]; ++a, ++w) {
            const int64_t t = alist[a];
            R.rowidx[w] = (int32_t)(p + mk + arow[t]); pl.csc_src[w] = (int32_t)(-1 - t);
        }
    }
    R.colptr[n] = w;
    pl.touched.insert(pl.touched.end(), pl.add_k.begin(), pl.add_k.end());
    // ---- position maps: A's entries follow their values; G' is numbered column by column in the caller's order
    R.csc_pos.assign((size_t)nnz2, 0);
    for (int64_t q = 0; q < P.nnzA; ++q) R.csc_pos[q] = old_to_new[P.csc_pos[q]];
    int64_t g = P.nnzA;
    for (int64_t j = 0; j < n; ++j) {
        const int64_t k = P.inv[j];
        for (int64_t q = R.colptr[k]; q < R.colptr[k + 1]; ++q)
            if (R.rowidx[q] >= p) R.csc_pos[g++] = (int32_t)q;
    }
    // ---- the CSR: finish_matrix's counting sort on the pattern
    std::vector<int32_t> to_csr((size_t)nnz2), old_to_csr((size_t)P.nnz);
    for (int64_t q = 0; q < P.nnz; ++q) old_to_csr[P.csc_pos[q]] = P.csr_pos[q];
    R.rowptr.assign((size_t)Q2 + 1, 0);
    for (int64_t q = 0; q < nnz2; ++q) R.rowptr[R.rowidx[q] + 1]++;
    for (int64_t r = 0; r < Q2; ++r) R.rowptr[r + 1] += R.rowptr[r];
    R.colidx.assign((size_t)nnz2, 0);
    pl.csr_src.assign((size_t)nnz2, 0);
    {
        std::vector<int64_t> cur(R.rowptr.begin(), R.rowptr.end() - 1);
        for (int64_t k = 0; k < n; ++k)
            for (int64_t q = R.colptr[k]; q < R.colptr[k + 1]; ++q) {
                const int64_t d = cur[R.rowidx[q]]++;
                R.colidx[d] = (int32_t)k;
                to_csr[q] = (int32_t)d;
                pl.csr_src[d] = pl.csc_src[q] >= 0 ? old_to_csr[pl.csc_src[q]] : pl.csc_src[q];
            }
    }
    R.csr_pos.assign((size_t)nnz2, 0);
    for (int64_t q = 0; q < nnz2; ++q) R.csr_pos[q] = to_csr[R.csc_pos[q]];
    // ---- [b; h']
    pl.bh_src.resize((size_t)Q2);
    for (int64_t i = 0; i < p; ++i) pl.bh_src[i] = (int32_t)i;
    for (int64_t r = 0; r < m2; ++r) pl.bh_src[p + r] = pl.kept[r] >= 0 ? (int32_t)(p + pl.kept[r]) : (int32_t)(-1 - (r - mk));
    R.val.assign((size_t)nnz2, 0.0); R.val_orig.assign((size_t)nnz2, 0.0); R.rval.assign((size_t)nnz2, 0.0);
    R.h.assign((size_t)m2, 0.0); R.h_orig.assign((size_t)m2, 0.0);
    return pl;
}

// the plan's members take their places in the handle's Prep (moves: nothing here can fail)
inline void commit_rows(Prep& P, RowsPlan& pl) {
    Prep& R = pl.R;
    P.m = R.m; P.Q = R.Q; P.nnz = R.nnz;
    P.colptr = std::move(R.colptr); P.rowidx = std::move(R.rowidx); P.rowptr = std::move(R.rowptr); P.colidx = std::move(R.colidx);
    P.csc_pos = std::move(R.csc_pos); P.csr_pos = std::move(R.csr_pos);
    P.val = std::move(R.val); P.val_orig = std::move(R.val_orig); P.rval = std::move(R.rval);
    P.h = std::move(R.h); P.h_orig = std::move(R.h_orig);
}

// is position k in the support set {column non-empty or c_k != 0} under the column pointers cp
inline bool in_support(const std::vector<int64_t>& cp, const std::vector<double>& c, int64_t k) { return cp[k + 1] > cp[k] || c[k] != 0.0; }

// ||M||_F from the host mirror, in finish_matrix's order: one running sum over the scaled values in reordered CSC order
inline double host_frob(const Prep& R) {
    double ss = 0.0;
    for (int64_t q = 0; q < R.nnz; ++q) ss += R.val[q] * R.val[q];
    return std::sqrt(ss);
}
// ||h'|| and ||M'||_F from the host mirrors, in prepare()'s order
inline void rows_host_norms(Prep& R) { R.norm_h = norm2(R.h.data(), R.m); R.frob = host_frob(R); }

// The planner's values on the host (proxsdp_host_model_rows_plan: no device): the kernels' arithmetic from the old Prep's
// arrays and HOST add_val / add_h, then the two norms.  rval_orig: the unscaled values in CSR order (the dump's csr_val_orig).
inline void apply_rows_host(const Prep& P, RowsPlan& pl, const double* add_val, const double* add_h, std::vector<double>& rval_orig) {
    Prep& R = pl.R;
    const double cte = std::sqrt(2.0) / 2.0;
    std::vector<double> old_rorig((size_t)P.nnz);
    for (int64_t q = 0; q < P.nnz; ++q) old_rorig[P.csr_pos[q]] = P.val_orig[P.csc_pos[q]];
    rval_orig.assign((size_t)R.nnz, 0.0);
    for (int64_t w = 0; w < R.nnz; ++w) {
        const int32_t s = pl.csc_src[w];
        if (s >= 0) { R.val_orig[w] = P.val_orig[s]; R.val[w] = P.val[s]; }
        else { const double v = add_val[-1 - s]; R.val_orig[w] = v; R.val[w] = v * (P.offdiag[pl.add_k[-1 - s]] ? cte : 1.0); }
        const int32_t sr = pl.csr_src[w];
        if (sr >= 0) { rval_orig[w] = old_rorig[sr]; R.rval[w] = P.rval[sr]; }
        else { const double v = add_val[-1 - sr]; rval_orig[w] = v; R.rval[w] = v * (P.offdiag[pl.add_k[-1 - sr]] ? cte : 1.0); }
    }
    for (int64_t r = 0; r < R.m; ++r) {
        const int32_t s = pl.bh_src[P.p + r];
        R.h[r] = s >= 0 ? P.h[s - P.p] : add_h[-1 - s];
    }
    R.h_orig = R.h;
    rows_host_norms(R);
}

}  // namespace proxsdp
