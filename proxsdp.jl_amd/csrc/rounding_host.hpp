// The host half of the rounding of a PSD cone's factors to a +-1 vector (rounding.hip.hpp has the kernels; the contract is in
// include/proxsdp_hip.h, "rounding on a model handle"): the argument checks, the direction generator, the adjacency of a
// cone's part of c built serially, the choice of the best trial, and the serial restatement behind proxsdp_host_round, which
// takes the adjacency as an argument.  No HIP in this file: it builds with a plain C++17 compiler
// (tests/c_harness/rounding_check.cpp, which is also what the address and undefined-behaviour sanitizers are pointed at).
// Every expression that the contract spells out is written here in the contract's order; build with -ffp-contract=off.
#pragma once
#include <chrono>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/proxsdp_hip.h"
#include "struct_check.hpp"

namespace proxsdp {

constexpr int ROUND_MAX_TRIALS = 65536;
constexpr int ROUND_MAX_SWEEPS = 1000;
constexpr int64_t ROUND_MAX_SIDE = 46340;
constexpr int ROUND_LDS_SIDE = 4096;            // the default of proxsdp_rounding.lds_side: 32 KiB of words per wave
constexpr int ROUND_LDS_SIDE_MAX = 8192;        // 64 KiB

// the generator of start_vector (host_util.hpp; oracle/eig.py), restated so that this file stands alone
inline uint64_t round_splitmix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
inline double round_uniform53(uint64_t seed, uint64_t counter) {
    const uint64_t key = seed ^ ((counter + 1ull) * 0xD1342543DE82EF95ull);
    return (double)(round_splitmix64(key) >> 11) * (1.0 / 9007199254740992.0);
}
// g(k, t) of `r` directions per trial
inline double round_direction(uint64_t seed, int64_t r, int64_t k, int64_t t) {
    const uint64_t base = ((uint64_t)t * (uint64_t)r + (uint64_t)k) * 12ull;
    double z = round_uniform53(seed, base);
    for (int q = 1; q < 12; ++q) z = z + round_uniform53(seed, base + (uint64_t)q);
    return z - 6.0;
}

inline double round_now_s() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

inline void check_round_shape(int64_t r, int64_t trials) {
    if (trials < 64 || trials > ROUND_MAX_TRIALS || trials % 64 != 0)
        throw std::invalid_argument("proxsdp_rounding.trials must be a multiple of 64 in 64 .. 65536");
    if (r < 1) throw std::invalid_argument("proxsdp_rounding.r must be 1 .. side");
}

// ---- what is decided on the host before a handle or a device is looked at
inline void check_rounding_struct(const proxsdp_rounding* q, bool model_entry) {
    if (!q) throw std::invalid_argument("NULL proxsdp_rounding");
    check_struct_size(q, "proxsdp_rounding");
    if (model_entry && q->on_device != 0 && q->on_device != 1) throw std::invalid_argument("proxsdp_rounding.on_device must be 0 or 1");
    if (!q->V || !q->values || !q->signs) throw std::invalid_argument("proxsdp_rounding: V, values or signs is NULL");
    check_round_shape(q->r, q->trials);
    if (q->max_sweeps < 0 || q->max_sweeps > ROUND_MAX_SWEEPS) throw std::invalid_argument("proxsdp_rounding.max_sweeps must be 0 .. 1000");
    if (q->grid_adjacency < 0 || q->grid_directions < 0 || q->grid_signs < 0 || q->grid_search < 0)
        throw std::invalid_argument("proxsdp_rounding: a launch knob is negative");
    if (model_entry && q->adj_ptr && (!q->adj_col || !q->adj_val || !q->diag || q->adj_cap < 0))
        throw std::invalid_argument("proxsdp_rounding: the adjacency needs adj_ptr, adj_col, adj_val, diag and adj_cap >= 0");
}

// the side is known: r against it, and host factors
inline void check_rounding_factors(const proxsdp_rounding& q, int64_t s, bool on_host) {
    if (s < 2) throw std::invalid_argument("proxsdp_rounding: the cone has side < 2");
    if (q.r > s) throw std::invalid_argument("proxsdp_rounding.r must be 1 .. side");
    if (!on_host) return;
    for (int64_t k = 0; k < q.r; ++k)
        if (!std::isfinite(q.values[k]) || !(q.values[k] > 0.0))
            throw std::invalid_argument("proxsdp_rounding: values must be finite and > 0");
    for (int64_t e = 0; e < s * (int64_t)q.r; ++e)
        if (!std::isfinite(q.V[e])) throw std::invalid_argument("proxsdp_rounding: non-finite entry in V");
}

// w_k = sqrt(values[k]); values: r host numbers (the device route downloads them first), checked here once more by name
inline std::vector<double> round_weights(const double* values, int64_t r) {
    std::vector<double> w((size_t)r);
    for (int64_t k = 0; k < r; ++k) {
        if (!std::isfinite(values[k]) || !(values[k] > 0.0)) throw std::invalid_argument("proxsdp_rounding: values must be finite and > 0");
        w[(size_t)k] = std::sqrt(values[k]);
    }
    return w;
}

// number of j != i with a non-zero entry, over all i, of a cone's part of c.  cc: the cone's s (s + 1) / 2 entries, upper
// triangle column by column
inline int64_t round_adjacency_count(const double* cc, int64_t s) {
    int64_t nnz = 0;
    for (int64_t j = 0; j < s; ++j)
        for (int64_t i = 0; i < j; ++i)
            if (cc[j * (j + 1) / 2 + i] != 0.0) nnz += 2;
    return nnz;
}

struct RoundAdjacency {
    std::vector<int64_t> ptr, col;
    std::vector<double> val, diag;
};
// the adjacency of the contract from a cone's part of c, serially
inline RoundAdjacency round_adjacency(const double* cc, int64_t s) {
    RoundAdjacency a;
    a.ptr.assign((size_t)s + 1, 0);
    a.diag.resize((size_t)s);
    for (int64_t i = 0; i < s; ++i) {
        a.diag[(size_t)i] = cc[i * (i + 1) / 2 + i];
        for (int64_t j = 0; j < s; ++j) {
            if (j == i) continue;
            const double w = j < i ? cc[i * (i + 1) / 2 + j] : cc[j * (j + 1) / 2 + i];
            if (w != 0.0) { a.col.push_back(j); a.val.push_back(w); }
        }
        a.ptr[(size_t)i + 1] = (int64_t)a.col.size();
    }
    return a;
}

inline void check_round_adjacency(int64_t s, const int64_t* ptr, const int64_t* col, const double* val, const double* diag) {
    if (!ptr || !diag) throw std::invalid_argument("proxsdp_host_round: adj_ptr or diag is NULL");
    if (ptr[0] != 0) throw std::invalid_argument("proxsdp_host_round: adj_ptr[0] must be 0");
    for (int64_t i = 0; i < s; ++i)
        if (ptr[i + 1] < ptr[i]) throw std::invalid_argument("proxsdp_host_round: adj_ptr must not decrease");
    if (ptr[s] > 0 && (!col || !val)) throw std::invalid_argument("proxsdp_host_round: adj_col or adj_val is NULL");
    for (int64_t i = 0; i < s; ++i) {
        if (!std::isfinite(diag[i])) throw std::invalid_argument("proxsdp_host_round: non-finite entry in diag");
        for (int64_t e = ptr[i]; e < ptr[i + 1]; ++e) {
            if (col[e] < 0 || col[e] >= s || col[e] == i) throw std::invalid_argument("proxsdp_host_round: adj_col outside the side, or on the diagonal");
            if (e > ptr[i] && col[e] <= col[e - 1]) throw std::invalid_argument("proxsdp_host_round: adj_col must ascend within a node");
            if (!std::isfinite(val[e])) throw std::invalid_argument("proxsdp_host_round: non-finite entry in adj_val");
        }
    }
}

// the value of a sign vector (sg: +-1.0 per node), in the contract's order
inline double round_value(int64_t s, const int64_t* ptr, const int64_t* col, const double* val, const double* diag, const double* sg) {
    double f = 0.0;
    for (int64_t i = 0; i < s; ++i) f = f + diag[i];
    for (int64_t i = 0; i < s; ++i) {
        double u = 0.0;
        for (int64_t e = ptr[i]; e < ptr[i + 1]; ++e)
            if (col[e] > i) u = u + val[e] * sg[col[e]];
        f = f + sg[i] * u;
    }
    return f;
}

// the smallest value, the lowest trial among equal ones
inline int64_t round_best(const double* v, int64_t T) {
    int64_t best = 0;
    for (int64_t t = 1; t < T; ++t)
        if (v[t] < v[best]) best = t;
    return best;
}

// proxsdp_host_round: one trial after the other.  q: checked by check_rounding_struct / check_rounding_factors, the adjacency
// by check_round_adjacency
inline void host_round(int64_t s, const int64_t* ptr, const int64_t* col, const double* val, const double* diag, proxsdp_rounding& q) {
    const double t0 = round_now_s();
    const int64_t r = q.r, T = q.trials;
    const std::vector<double> w = round_weights(q.values, r);
    std::vector<double> g((size_t)r), sg((size_t)s), best_sg((size_t)s);
    double best_final = 0.0, best_rounded = 0.0;
    int64_t best_t = -1, flips = 0;
    int sweeps_max = 0;
    for (int64_t t = 0; t < T; ++t) {
        for (int64_t k = 0; k < r; ++k) g[(size_t)k] = round_direction((uint64_t)q.seed, r, k, t);
        for (int64_t i = 0; i < s; ++i) {
            double y = 0.0;
            for (int64_t k = 0; k < r; ++k) y = y + (q.V[i + k * s] * w[(size_t)k]) * g[(size_t)k];
            sg[(size_t)i] = y < 0.0 ? -1.0 : 1.0;
        }
        const double rounded = round_value(s, ptr, col, val, diag, sg.data());
        int sweeps = 0;
        while (sweeps < q.max_sweeps) {
            ++sweeps;
            int64_t flipped = 0;
            for (int64_t i = 0; i < s; ++i) {
                double a = 0.0;
                for (int64_t e = ptr[i]; e < ptr[i + 1]; ++e) a = a + val[e] * sg[(size_t)col[e]];
                if (sg[(size_t)i] * a > 0.0) { sg[(size_t)i] = -sg[(size_t)i]; ++flipped; }
            }
            flips += flipped;
            if (flipped == 0) break;
        }
        if (sweeps > sweeps_max) sweeps_max = sweeps;
        const double fin = round_value(s, ptr, col, val, diag, sg.data());
        if (q.values_rounded) q.values_rounded[t] = rounded;
        if (q.values_final) q.values_final[t] = fin;
        if (best_t < 0 || rounded < best_rounded) best_rounded = rounded;
        if (best_t < 0 || fin < best_final) { best_final = fin; best_t = t; best_sg = sg; }
    }
    for (int64_t i = 0; i < s; ++i) q.signs[i] = best_sg[(size_t)i] < 0.0 ? (int8_t)-1 : (int8_t)1;
    q.best_trial = best_t; q.value = best_final; q.value_rounded = best_rounded;
    q.flips = flips; q.sweeps = sweeps_max;
    q.bytes_allocated = 0; q.search_seconds = 0.0;
    q.seconds = round_now_s() - t0;
}

}  // namespace proxsdp
