// The host half of the pentagonal / heptagonal separation (clique_cuts.hip.hpp has the kernels, include/proxsdp_hip.h the
// contract): the argument checks, the total order of the extensions of a base, the serial restatement behind
// proxsdp_host_clique_cuts, and what both entries do with the best extension of every base -- normal form, merge, sort, the
// rows in the caller's arrays.  No HIP in this file: it builds with a plain C++17 compiler
// (tests/c_harness/clique_cuts_check.cpp, which is also what the address and undefined-behaviour sanitizers are pointed at).
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

constexpr int64_t CLQ_MAX_BASES = 65536;
constexpr int64_t CLQ_MAX_SIDE = 46340;
constexpr int CLQ_MAX_K = 7;                    // nodes of the largest row
constexpr int CLQ_DEFAULT_BATCH = 1024;

// The best extension of a base so far.  key = (l side + m) 4 + code: the lexicographic order of (l, m, code) as one number
// (< 2^34 for every side a cone may have).  CLQ_NO_KEY with v = -infinity: nothing seen yet.
struct CliqueBest { double v; unsigned long long key; };
constexpr unsigned long long CLQ_NO_KEY = ~0ull;

// the total order: the greater v, equal v by the smaller (l, m, code).  A NaN is never better than anything.
#if defined(__HIPCC__)
__host__ __device__
#endif
inline bool clique_better(double v, unsigned long long key, double bv, unsigned long long bkey) {
    return v > bv || (v == bv && key < bkey);
}

inline double clq_now_s() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// ---- what is decided on the host before a handle or a device is looked at
inline void check_clique_struct(const proxsdp_clique_cuts* q, bool model_entry) {
    if (!q) throw std::invalid_argument("NULL proxsdp_clique_cuts");
    check_struct_size(q, "proxsdp_clique_cuts");
    if (model_entry && q->on_device != 0 && q->on_device != 1) throw std::invalid_argument("proxsdp_clique_cuts.on_device must be 0 or 1");
    if (q->base_size != 3 && q->base_size != 5) throw std::invalid_argument("proxsdp_clique_cuts.base_size must be 3 or 5");
    if (q->n_base < 1 || q->n_base > CLQ_MAX_BASES) throw std::invalid_argument("proxsdp_clique_cuts.n_base must be 1 .. 65536");
    if (!std::isfinite(q->rhs)) throw std::invalid_argument("proxsdp_clique_cuts.rhs must be finite");
    if (!std::isfinite(q->min_violation) || q->min_violation < 0.0)
        throw std::invalid_argument("proxsdp_clique_cuts.min_violation must be finite and >= 0");
    if (q->grid < 0) throw std::invalid_argument("proxsdp_clique_cuts.grid must be >= 0");
    if (q->batch < 0) throw std::invalid_argument("proxsdp_clique_cuts.batch must be >= 0");
    if (model_entry && !q->primal) throw std::invalid_argument("proxsdp_clique_cuts.primal is NULL");
    if (!q->base_nodes) throw std::invalid_argument("proxsdp_clique_cuts.base_nodes is NULL");
    if (!q->base_sign) throw std::invalid_argument("proxsdp_clique_cuts.base_sign is NULL");
    if (!q->nodes || !q->signs || !q->violation || !q->from_base || !q->add_col || !q->add_val || !q->add_h)
        throw std::invalid_argument("proxsdp_clique_cuts: NULL output array");
}

// the bases against the side of the cone (the struct has passed check_clique_struct)
inline void check_clique_bases(const proxsdp_clique_cuts& q, int64_t s) {
    const int bq = q.base_size;
    for (int64_t b = 0; b < q.n_base; ++b)
        for (int u = 0; u < bq; ++u) {
            const int64_t a = q.base_nodes[b * bq + u];
            const int sg = q.base_sign[b * bq + u];
            if (a < 0 || a >= s)
                throw std::invalid_argument("proxsdp_clique_cuts.base_nodes: base " + std::to_string(b) + " has a node outside the cone");
            if (u > 0 && a <= q.base_nodes[b * bq + u - 1])
                throw std::invalid_argument("proxsdp_clique_cuts.base_nodes: base " + std::to_string(b) + " is not strictly ascending");
            if (sg != 1 && sg != -1)
                throw std::invalid_argument("proxsdp_clique_cuts.base_sign: base " + std::to_string(b) + " has a sign that is not +-1");
            if (u == 0 && sg != 1)
                throw std::invalid_argument("proxsdp_clique_cuts.base_sign: the first sign of base " + std::to_string(b) + " is not +1");
        }
}

inline int64_t clique_scanned(int64_t n_base, int64_t s, int bq) { return n_base * 4 * ((s - bq) * (s - bq - 1) / 2); }

// ---- from the best extension of every base to the caller's arrays (both entries end here)
struct CliqueRow {
    int64_t nodes[CLQ_MAX_K];
    int8_t signs[CLQ_MAX_K];
    double v;
    int64_t base;
};

// best[b]: the best extension of base b under clique_better.  col(i, j), i < j: the variable number of X_ij
template <typename Col>
inline void clique_write_rows(const std::vector<CliqueBest>& best, int64_t s, proxsdp_clique_cuts& q, Col&& col) {
    const int bq = q.base_size, k = bq + 2, np = k * (k - 1) / 2;
    std::vector<CliqueRow> rows;
    for (int64_t b = 0; b < q.n_base; ++b) {
        if (best[(size_t)b].key == CLQ_NO_KEY || !(best[(size_t)b].v > q.min_violation)) continue;
        const unsigned long long key = best[(size_t)b].key;
        const int code = (int)(key & 3);
        const int64_t l = (int64_t)((key >> 2) / (unsigned long long)s), m = (int64_t)((key >> 2) % (unsigned long long)s);
        CliqueRow r{};
        r.v = best[(size_t)b].v; r.base = b;
        // the base's nodes and the two new ones, merged ascending (l < m, neither in the base)
        const int64_t nn[2] = {l, m};
        const int8_t ns[2] = {(int8_t)((code & 2) ? -1 : 1), (int8_t)((code & 1) ? -1 : 1)};
        int u = 0, w = 0;
        for (int o = 0; o < k; ++o) {
            const bool take_new = u == bq || (w < 2 && nn[w] < q.base_nodes[b * bq + u]);
            if (take_new) { r.nodes[o] = nn[w]; r.signs[o] = ns[w]; ++w; }
            else { r.nodes[o] = q.base_nodes[b * bq + u]; r.signs[o] = q.base_sign[b * bq + u]; ++u; }
        }
        if (r.signs[0] < 0)
            for (int o = 0; o < k; ++o) r.signs[o] = (int8_t)-r.signs[o];
        rows.push_back(r);
    }
    q.violated_bases = (int64_t)rows.size();
    // equal (nodes, signs) next to each other, the member to keep first: the greatest v, then the lowest base
    auto same = [k](const CliqueRow& a, const CliqueRow& b) {
        return std::equal(a.nodes, a.nodes + k, b.nodes) && std::equal(a.signs, a.signs + k, b.signs);
    };
    std::sort(rows.begin(), rows.end(), [k](const CliqueRow& a, const CliqueRow& b) {
        for (int o = 0; o < k; ++o)
            if (a.nodes[o] != b.nodes[o]) return a.nodes[o] < b.nodes[o];
        for (int o = 0; o < k; ++o)
            if (a.signs[o] != b.signs[o]) return a.signs[o] < b.signs[o];
        if (a.v != b.v) return a.v > b.v;
        return a.base < b.base;
    });
    rows.erase(std::unique(rows.begin(), rows.end(), same), rows.end());
    std::sort(rows.begin(), rows.end(), [](const CliqueRow& a, const CliqueRow& b) { return a.v != b.v ? a.v > b.v : a.base < b.base; });
    for (size_t r = 0; r < rows.size(); ++r) {
        const CliqueRow& R = rows[r];
        for (int o = 0; o < k; ++o) { q.nodes[r * k + o] = R.nodes[o]; q.signs[r * k + o] = R.signs[o]; }
        q.violation[r] = R.v;
        q.from_base[r] = R.base;
        int e = 0;
        for (int u = 0; u < k; ++u)
            for (int w = u + 1; w < k; ++w, ++e) {
                q.add_col[r * np + e] = col(R.nodes[u], R.nodes[w]);
                q.add_val[r * np + e] = (double)(-R.signs[u] * R.signs[w]);
            }
        q.add_h[r] = q.rhs;
    }
    q.n_rows = (int64_t)rows.size();
    q.scanned = clique_scanned(q.n_base, s, bq);
}

// ---- the serial restatement
// B of base b.  x(i, j), i < j: X_ij
template <typename Xat>
inline double clique_base_value(const proxsdp_clique_cuts& q, int64_t b, Xat&& x) {
    const int bq = q.base_size;
    double B = 0.0;
    bool first = true;
    for (int u = 0; u < bq; ++u)
        for (int w = u + 1; w < bq; ++w) {
            const double sg = (double)(-q.base_sign[b * bq + u] * q.base_sign[b * bq + w]);
            const double term = sg * x(q.base_nodes[b * bq + u], q.base_nodes[b * bq + w]);
            B = first ? term : B + term;
            first = false;
        }
    return B;
}

// proxsdp_host_clique_cuts.  X: s x s row-major, only i < j read; idx: the cone's variable list or NULL = tri_index + base
inline void host_clique_cuts(const double* X, int64_t s, const int64_t* idx, int base, proxsdp_clique_cuts& q) {
    const double t0 = clq_now_s();
    const int bq = q.base_size;
    for (int64_t i = 0; i < s; ++i)
        for (int64_t j = i + 1; j < s; ++j)
            if (!std::isfinite(X[i * s + j])) throw std::invalid_argument("proxsdp_host_clique_cuts: non-finite entry in X");
    auto x = [&](int64_t i, int64_t j) { return i < j ? X[i * s + j] : X[j * s + i]; };
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<CliqueBest> best((size_t)q.n_base);
    std::vector<double> t((size_t)s);
    for (int64_t b = 0; b < q.n_base; ++b) {
        const int64_t* a = q.base_nodes + b * bq;
        const int8_t* sg = q.base_sign + b * bq;
        for (int64_t l = 0; l < s; ++l) {
            bool own = false;
            for (int u = 0; u < bq; ++u) own = own || a[u] == l;
            if (own) { t[(size_t)l] = nan; continue; }               // the base's own nodes: no comparison below passes
            double acc = (double)sg[0] * x(a[0], l);
            for (int u = 1; u < bq; ++u) acc = acc + (double)sg[u] * x(a[u], l);
            t[(size_t)l] = acc;
        }
        const double B = clique_base_value(q, b, x);
        CliqueBest bb{-std::numeric_limits<double>::infinity(), CLQ_NO_KEY};
        for (int64_t l = 0; l < s; ++l) {
            const double tl = t[(size_t)l];
            if (tl != tl) continue;
            const double p = B - tl, n = B + tl;                     // B - tau_l t_l for tau_l = +1, -1
            for (int64_t m = l + 1; m < s; ++m) {
                const double tm = t[(size_t)m], xv = X[l * s + m];
                const double v[4] = {((p - tm) - xv) - q.rhs, ((p + tm) + xv) - q.rhs, ((n - tm) + xv) - q.rhs, ((n + tm) - xv) - q.rhs};
                for (int c = 0; c < 4; ++c)
                    if (v[c] > bb.v) { bb.v = v[c]; bb.key = (unsigned long long)((l * s + m) * 4 + c); }
            }
        }
        best[(size_t)b] = bb;
    }
    clique_write_rows(best, s, q, [&](int64_t i, int64_t j) { const int64_t e = j * (j + 1) / 2 + i; return idx ? idx[e] : e + base; });
    q.bytes_allocated = 0; q.sweep_seconds = 0.0;
    q.seconds = clq_now_s() - t0;
}

}  // namespace proxsdp
