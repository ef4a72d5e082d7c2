// The host half of the triangle separation and the slack-row test (triangle_cuts.hip.hpp has the contract and the kernels):
// the argument checks, the order of the rows, the decoding of a row into the caller's arrays, the serial restatement behind
// proxsdp_host_triangle_cuts, the gate of a later sweep, the slack rows of host vectors.  No HIP in this file: it builds
// with a plain C++17 compiler (tests/c_harness/triangle_cuts_check.cpp, which is also what the address and undefined-behaviour
// sanitizers are pointed at).
#pragma once
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/proxsdp_hip.h"
#include "struct_check.hpp"

namespace proxsdp {

constexpr int TRI_DIGIT_BITS = 12;
constexpr int TRI_BINS = 1 << TRI_DIGIT_BITS;
constexpr int TRI_LIN_BITS = 50;                // lin < 4 * 46340^3 < 2^49
constexpr int TRI_LIN_SHIFT = 64 - TRI_LIN_BITS;
constexpr int TRI_DIGITS = (128 - TRI_LIN_SHIFT + TRI_DIGIT_BITS - 1) / TRI_DIGIT_BITS;     // digits down to lin's last bit
constexpr int64_t TRI_MAX_COUNT = (int64_t)1 << 20;

typedef unsigned __int128 tri_u128;

// ---- what is decided on the host before a handle or a device is looked at
inline void check_triangle_struct(const proxsdp_triangle_cuts* tc, bool model_entry) {
    if (!tc) throw std::invalid_argument("NULL proxsdp_triangle_cuts");
    check_struct_size(tc, "proxsdp_triangle_cuts");
    if (model_entry && tc->on_device != 0 && tc->on_device != 1) throw std::invalid_argument("proxsdp_triangle_cuts.on_device must be 0 or 1");
    if (tc->count < 1 || tc->count > TRI_MAX_COUNT) throw std::invalid_argument("proxsdp_triangle_cuts.count must be 1 .. 2^20");
    if (!std::isfinite(tc->min_violation) || tc->min_violation < 0.0)
        throw std::invalid_argument("proxsdp_triangle_cuts.min_violation must be finite and >= 0");
    if (!std::isfinite(tc->rhs)) throw std::invalid_argument("proxsdp_triangle_cuts.rhs must be finite");
    if (tc->cand_cap < 0 || tc->cand_cap > ((int64_t)1 << 24)) throw std::invalid_argument("proxsdp_triangle_cuts.cand_cap must be 0 .. 2^24");
    if (model_entry && !tc->primal) throw std::invalid_argument("proxsdp_triangle_cuts.primal is NULL");
    if (!tc->tri || !tc->pattern || !tc->violation || !tc->add_col || !tc->add_val || !tc->add_h)
        throw std::invalid_argument("proxsdp_triangle_cuts: NULL output array");
}

inline int64_t tri_scanned(int64_t s) { return 4 * (s * (s - 1) * (s - 2) / 6); }

inline double tri_now_s() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

struct TriCand { unsigned long long vb, lin; };                     // the bits of v; lin = ((i s + j) s + k) 4 + pattern
// v descending, then (i, j, k, pattern) ascending
inline bool tri_before(const TriCand& a, const TriCand& b) { return a.vb != b.vb ? a.vb > b.vb : a.lin < b.lin; }

// the first min(count, size) candidates in order into the caller's arrays.  col(i, j), i < j: the variable number of X_ij
template <typename Col>
inline void tri_write_rows(std::vector<TriCand>& cand, int64_t s, proxsdp_triangle_cuts& tc, Col&& col) {
    const size_t keep = std::min<size_t>(cand.size(), (size_t)tc.count);
    std::partial_sort(cand.begin(), cand.begin() + keep, cand.end(), tri_before);
    static const double sign[4][3] = {{-1.0, -1.0, -1.0}, {-1.0, 1.0, 1.0}, {1.0, -1.0, 1.0}, {1.0, 1.0, -1.0}};
    for (size_t r = 0; r < keep; ++r) {
        unsigned long long l = cand[r].lin;
        const int p = (int)(l & 3); l >>= 2;
        const int64_t k = (int64_t)(l % (unsigned long long)s); l /= (unsigned long long)s;
        const int64_t j = (int64_t)(l % (unsigned long long)s), i = (int64_t)(l / (unsigned long long)s);
        tc.tri[3 * r] = i; tc.tri[3 * r + 1] = j; tc.tri[3 * r + 2] = k;
        tc.pattern[r] = p;
        double v;
        std::memcpy(&v, &cand[r].vb, sizeof v);
        tc.violation[r] = v;
        tc.add_col[3 * r] = col(i, j); tc.add_col[3 * r + 1] = col(i, k); tc.add_col[3 * r + 2] = col(j, k);
        for (int q = 0; q < 3; ++q) tc.add_val[3 * r + q] = sign[p][q];
        tc.add_h[r] = tc.rhs;
    }
    tc.n_rows = (int64_t)keep;
}

// proxsdp_host_triangle_cuts: the serial enumeration.  X: s x s row-major, only i < j read; idx: the cone's variable list
// (upper triangle column by column, numbers as add_col reports them) or NULL = tri_index(i, j) + base
inline void host_triangle_cuts(const double* X, int64_t s, const int64_t* idx, int base, proxsdp_triangle_cuts& tc) {
    const double t0 = tri_now_s();
    const double minv = tc.min_violation, rhs = tc.rhs;
    for (int64_t i = 0; i < s; ++i)
        for (int64_t j = i + 1; j < s; ++j)
            if (!std::isfinite(X[i * s + j])) throw std::invalid_argument("proxsdp_host_triangle_cuts: non-finite entry in X");
    std::vector<TriCand> cand;
    const size_t limit = 2 * (size_t)tc.count + 1024;
    int64_t violated = 0;
    auto take = [&](double v, unsigned long long lin) {
        if (!(v > minv)) return;
        ++violated;
        TriCand c;
        std::memcpy(&c.vb, &v, sizeof v);
        c.lin = lin;
        cand.push_back(c);
        if (cand.size() >= limit) {                                 // keep the first `count` in order, drop the rest
            std::nth_element(cand.begin(), cand.begin() + tc.count, cand.end(), tri_before);
            cand.resize((size_t)tc.count);
        }
    };
    for (int64_t i = 0; i < s; ++i)
        for (int64_t j = i + 1; j < s; ++j) {
            const double A = X[i * s + j];
            for (int64_t k = j + 1; k < s; ++k) {
                const double B = X[i * s + k], C = X[j * s + k];
                const unsigned long long lin = (unsigned long long)((i * s + j) * s + k) * 4ull;
                take(((-A - B) - C) - rhs, lin);
                take(((-A + B) + C) - rhs, lin + 1);
                take(((A - B) + C) - rhs, lin + 2);
                take(((A + B) - C) - rhs, lin + 3);
            }
        }
    tri_write_rows(cand, s, tc, [&](int64_t i, int64_t j) { const int64_t q = j * (j + 1) / 2 + i; return idx ? idx[q] : q + base; });
    tc.violated = violated; tc.scanned = tri_scanned(s); tc.passes = 0; tc.bytes_allocated = 0; tc.sweep_seconds = 0.0;
    tc.seconds = tri_now_s() - t0;
}

// The gate of a sweep whose rows must carry the leading `pbits` bits P of K, or larger ones: such a row has
// bits(v) >= the high word of P padded with zeros, that is v >= vlo, that is v > the double just below vlo (the images of
// positive doubles are monotone).  The gate only spares the rows that the prefix test would turn away: the result is the same.
inline double tri_gate(double min_violation, tri_u128 P, int pbits) {
    if (pbits <= 0) return min_violation;
    const unsigned long long vlo_bits = (unsigned long long)((P << (128 - pbits)) >> 64);
    double vlo;
    std::memcpy(&vlo, &vlo_bits, sizeof vlo);
    if (!(vlo > 0.0) || !std::isfinite(vlo)) return min_violation;
    return std::max(min_violation, std::nextafter(vlo, -std::numeric_limits<double>::infinity()));
}

// ---- rows that went slack
inline void check_inactive_struct(const proxsdp_inactive_rows* q) {
    if (!q) throw std::invalid_argument("NULL proxsdp_inactive_rows");
    check_struct_size(q, "proxsdp_inactive_rows");
    if (q->on_device != 0 && q->on_device != 1) throw std::invalid_argument("proxsdp_inactive_rows.on_device must be 0 or 1");
    if (!q->dual_in || !q->slack_in || !q->rows) throw std::invalid_argument("proxsdp_inactive_rows: NULL array");
    if (!std::isfinite(q->dual_tol) || q->dual_tol < 0.0 || !std::isfinite(q->slack_tol) || q->slack_tol < 0.0)
        throw std::invalid_argument("proxsdp_inactive_rows: dual_tol and slack_tol must be finite and >= 0");
}

// host vectors: the rows in ascending order (a NaN fails either comparison)
inline void inactive_rows_host(int64_t m, proxsdp_inactive_rows& q) {
    q.n_rows = 0;
    for (int64_t r = 0; r < m; ++r)
        if (std::fabs(q.dual_in[r]) <= q.dual_tol && q.slack_in[r] < -q.slack_tol) q.rows[q.n_rows++] = r;
}

}  // namespace proxsdp
