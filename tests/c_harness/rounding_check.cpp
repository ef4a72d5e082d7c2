// Stand-alone check of the host half of the rounding (proxsdp.jl_amd/csrc/rounding_host.hpp): no HIP, no library.  The serial
// restatement behind proxsdp_host_round against a second restatement written here independently (a dense weight matrix, integer
// signs, a generator of its own, one trial at a time with its own bookkeeping), on dyadic and real weights, with isolated
// nodes, a zero row of V and an all-zero objective; the adjacency built from a packed triangle; the tie rule; the refusals.
// Built plain by tests/test_rounding_host.py; the same program is what -fsanitize=address,undefined is pointed at.
#include <algorithm>
#include <cstdio>
#include <random>

#include "rounding_host.hpp"

using namespace proxsdp;

static int failures = 0;
static void report(const char* name, bool ok) {
    std::printf("%s: %s\n", name, ok ? "ok" : "FAILED");
    if (!ok) ++failures;
}

// ---- the second restatement
static uint64_t mix2(uint64_t z) {
    z = z + 0x9E3779B97F4A7C15ull;
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
static double dir2(uint64_t seed, int64_t r, int64_t k, int64_t t) {
    double u[12];
    for (int q = 0; q < 12; ++q) {
        const uint64_t counter = (uint64_t)((t * r + k) * 12 + q);
        u[q] = std::ldexp((double)(mix2(seed ^ ((counter + 1) * 0xD1342543DE82EF95ull)) >> 11), -53);
    }
    double z = u[0] + u[1];
    for (int q = 2; q < 12; ++q) z = z + u[q];
    return z - 6.0;
}

struct Dense {
    int64_t s;
    std::vector<double> W, d;                   // W: s x s symmetric, zero diagonal
    double w(int64_t i, int64_t j) const { return W[(size_t)(i * s + j)]; }
};
static double value2(const Dense& D, const std::vector<int>& sg) {
    double f = 0.0;
    for (int64_t i = 0; i < D.s; ++i) f = f + D.d[(size_t)i];
    for (int64_t i = 0; i < D.s; ++i) {
        double u = 0.0;
        for (int64_t j = i + 1; j < D.s; ++j)
            if (D.w(i, j) != 0.0) u = u + D.w(i, j) * (double)sg[(size_t)j];
        f = f + (double)sg[(size_t)i] * u;
    }
    return f;
}
struct Want {
    std::vector<int> signs;
    std::vector<double> vr, vf;
    int64_t best = 0, flips = 0;
    int sweeps = 0;
};
static Want restate2(const Dense& D, const std::vector<double>& V, const std::vector<double>& lam, int64_t r, int64_t T,
                     uint64_t seed, int max_sweeps) {
    Want out;
    const int64_t s = D.s;
    std::vector<std::vector<int>> all;
    for (int64_t t = 0; t < T; ++t) {
        std::vector<int> sg((size_t)s);
        for (int64_t i = 0; i < s; ++i) {
            double y = 0.0;
            for (int64_t k = 0; k < r; ++k) {
                const double a = V[(size_t)(k * s + i)] * std::sqrt(lam[(size_t)k]);
                y = y + a * dir2(seed, r, k, t);
            }
            sg[(size_t)i] = y < 0.0 ? -1 : 1;
        }
        out.vr.push_back(value2(D, sg));
        int done = 0;
        for (int sw = 1; sw <= max_sweeps && !done; ++sw) {
            out.sweeps = std::max(out.sweeps, sw);
            done = 1;
            for (int64_t i = 0; i < s; ++i) {
                double a = 0.0;
                for (int64_t j = 0; j < s; ++j)
                    if (j != i && D.w(i, j) != 0.0) a = a + D.w(i, j) * (double)sg[(size_t)j];
                if ((double)sg[(size_t)i] * a > 0.0) { sg[(size_t)i] = -sg[(size_t)i]; ++out.flips; done = 0; }
            }
        }
        out.vf.push_back(value2(D, sg));
        all.push_back(sg);
    }
    for (int64_t t = 0; t < T; ++t)
        if (out.vf[(size_t)t] < out.vf[(size_t)out.best]) out.best = t;
    out.signs = all[(size_t)out.best];
    return out;
}

// ---- fixtures
static Dense make_graph(int64_t s, unsigned seed, double degree, bool dyadic, int64_t isolated) {
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::normal_distribution<double> N(0.0, 1.0);
    Dense D{s, std::vector<double>((size_t)(s * s), 0.0), std::vector<double>((size_t)s, 0.0)};
    const double p = std::min(1.0, degree / (double)std::max<int64_t>(s - 1, 1));
    for (int64_t i = 0; i < s; ++i)
        for (int64_t j = i + 1; j < s; ++j) {
            const bool edge = U(rng) < p;
            const double w = dyadic ? (U(rng) < 0.25 ? -0.5 : 0.5) : N(rng);
            if (edge && i != isolated && j != isolated) D.W[(size_t)(i * s + j)] = D.W[(size_t)(j * s + i)] = w;
        }
    for (int64_t i = 0; i < s; ++i) {
        double sum = 0.0;
        for (int64_t j = 0; j < s; ++j) sum += D.w(i, j);
        D.d[(size_t)i] = dyadic ? -0.5 * sum : N(rng);
    }
    return D;
}
static std::vector<double> pack(const Dense& D) {
    std::vector<double> cc;
    for (int64_t j = 0; j < D.s; ++j)
        for (int64_t i = 0; i <= j; ++i) cc.push_back(i == j ? D.d[(size_t)j] : D.w(i, j));
    return cc;
}
static void make_factors(int64_t s, int64_t r, unsigned seed, int64_t zero_row, std::vector<double>& V, std::vector<double>& lam) {
    std::mt19937_64 rng(seed);
    std::normal_distribution<double> N(0.0, 1.0);
    V.assign((size_t)(s * r), 0.0);
    lam.assign((size_t)r, 0.0);
    for (double& v : V) v = N(rng);
    for (int64_t k = 0; k < r; ++k) lam[(size_t)k] = 0.25 + (double)(r - k);
    if (zero_row >= 0)
        for (int64_t k = 0; k < r; ++k) V[(size_t)(k * s + zero_row)] = 0.0;
}

struct Call {
    std::vector<int8_t> signs;
    std::vector<double> vr, vf;
    proxsdp_rounding q{};
    Call(int64_t s, int64_t r, int64_t T, uint64_t seed, int max_sweeps, const std::vector<double>& V, const std::vector<double>& lam)
        : signs((size_t)s, (int8_t)7), vr((size_t)T, -7.0), vf((size_t)T, -7.0) {
        q.struct_size = (int64_t)sizeof(proxsdp_rounding);
        q.r = (int32_t)r; q.trials = (int32_t)T; q.seed = (int64_t)seed; q.max_sweeps = max_sweeps;
        q.V = V.data(); q.values = lam.data();
        q.signs = signs.data(); q.values_rounded = vr.data(); q.values_final = vf.data();
    }
};

static bool run_case(int64_t s, int64_t r, int64_t T, uint64_t seed, int max_sweeps, bool dyadic, int64_t isolated, int64_t zero_row,
                     bool zero_c) {
    Dense D = make_graph(s, (unsigned)(seed + 17), 4.0, dyadic, isolated);
    if (zero_c) { std::fill(D.W.begin(), D.W.end(), 0.0); std::fill(D.d.begin(), D.d.end(), 0.0); }
    std::vector<double> V, lam;
    make_factors(s, r, (unsigned)(seed + 3), zero_row, V, lam);
    const std::vector<double> cc = pack(D);
    const RoundAdjacency A = round_adjacency(cc.data(), s);
    bool ok = (int64_t)A.col.size() == round_adjacency_count(cc.data(), s);
    // the adjacency against the dense matrix
    for (int64_t i = 0; i < s && ok; ++i) {
        int64_t e = A.ptr[(size_t)i];
        for (int64_t j = 0; j < s; ++j)
            if (j != i && D.w(i, j) != 0.0) { ok = ok && e < A.ptr[(size_t)i + 1] && A.col[(size_t)e] == j && A.val[(size_t)e] == D.w(i, j); ++e; }
        ok = ok && e == A.ptr[(size_t)i + 1] && A.diag[(size_t)i] == D.d[(size_t)i];
    }
    Call c(s, r, T, seed, max_sweeps, V, lam);
    check_rounding_struct(&c.q, false);
    check_rounding_factors(c.q, s, true);
    check_round_adjacency(s, A.ptr.data(), A.col.data(), A.val.data(), A.diag.data());
    host_round(s, A.ptr.data(), A.col.data(), A.val.data(), A.diag.data(), c.q);
    const Want w = restate2(D, V, lam, r, T, seed, max_sweeps);
    ok = ok && c.q.best_trial == w.best && c.q.flips == w.flips && c.q.sweeps == w.sweeps;
    ok = ok && c.q.value == w.vf[(size_t)w.best] && c.q.value_rounded == *std::min_element(w.vr.begin(), w.vr.end());
    for (int64_t t = 0; t < T; ++t) ok = ok && c.vr[(size_t)t] == w.vr[(size_t)t] && c.vf[(size_t)t] == w.vf[(size_t)t];
    for (int64_t i = 0; i < s; ++i) ok = ok && (int)c.signs[(size_t)i] == w.signs[(size_t)i];
    if (zero_row >= 0 && max_sweeps == 0) ok = ok && c.signs[(size_t)zero_row] == 1;
    if (zero_c) ok = ok && c.q.best_trial == 0 && c.q.value == 0.0 && c.q.flips == 0 && c.q.sweeps == (max_sweeps > 0 ? 1 : 0);
    return ok;
}

template <typename F>
static bool refuses(F&& f) {
    try { f(); } catch (const std::invalid_argument&) { return true; }
    return false;
}

int main() {
    {
        bool ok = true;
        for (int64_t r : {1, 2, 17})
            for (int64_t t : {0, 1, 63, 64, 191})
                for (int64_t k = 0; k < r; ++k) ok = ok && round_direction(12345u, r, k, t) == dir2(12345u, r, k, t);
        report("directions equal the second generator", ok);
    }
    report("side 2, r 1 and 2", run_case(2, 1, 64, 1, 50, true, -1, -1, false) && run_case(2, 2, 128, 2, 1, false, -1, -1, false));
    report("side 3 and 4, r up to the side", run_case(3, 2, 64, 3, 50, false, -1, -1, false) && run_case(4, 4, 192, 4, 50, true, -1, -1, false));
    report("side 16, dyadic, every sweep limit", run_case(16, 9, 192, 5, 0, true, -1, -1, false) &&
           run_case(16, 9, 192, 5, 1, true, -1, -1, false) && run_case(16, 9, 192, 5, 50, true, -1, -1, false));
    report("side 16, real weights", run_case(16, 2, 128, 6, 50, false, -1, -1, false));
    report("sides 63, 64, 65", run_case(63, 17, 64, 7, 50, true, -1, -1, false) && run_case(64, 9, 128, 8, 50, false, -1, -1, false) &&
           run_case(65, 1, 64, 9, 50, true, -1, -1, false));
    report("side 130", run_case(130, 17, 64, 10, 50, false, -1, -1, false));
    report("an isolated node and a zero row of V", run_case(16, 3, 64, 11, 50, true, 5, 5, false) && run_case(16, 3, 64, 11, 0, false, 0, 9, false));
    report("an all-zero objective: trial 0, value 0, no flip, one sweep", run_case(16, 3, 128, 12, 50, true, -1, -1, true) &&
           run_case(5, 2, 64, 13, 0, true, -1, -1, true));
    {
        const double v[6] = {3.0, 1.0, 2.0, 1.0, -0.0, 1.0};
        const double z[3] = {0.0, -0.0, 0.0};
        report("the lowest trial among equal values", round_best(v, 4) == 1 && round_best(v, 6) == 4 && round_best(z, 3) == 0);
    }
    {
        std::vector<double> V, lam;
        make_factors(4, 2, 1, -1, V, lam);
        Call c(4, 2, 64, 0, 10, V, lam);
        bool ok = !refuses([&] { check_rounding_struct(&c.q, true); check_rounding_factors(c.q, 4, true); });
        auto bad = [&](auto&& change) {
            Call d(4, 2, 64, 0, 10, V, lam);
            change(d.q);
            return refuses([&] { check_rounding_struct(&d.q, true); check_rounding_factors(d.q, 4, true); });
        };
        ok = ok && refuses([&] { check_rounding_struct(nullptr, true); });
        ok = ok && bad([](proxsdp_rounding& q) { q.struct_size -= 8; }) && bad([](proxsdp_rounding& q) { q.on_device = 2; });
        ok = ok && bad([](proxsdp_rounding& q) { q.V = nullptr; }) && bad([](proxsdp_rounding& q) { q.values = nullptr; });
        ok = ok && bad([](proxsdp_rounding& q) { q.signs = nullptr; });
        ok = ok && bad([](proxsdp_rounding& q) { q.r = 0; }) && bad([](proxsdp_rounding& q) { q.r = 5; });
        for (int T : {0, -64, 63, 100, 65600}) ok = ok && bad([T](proxsdp_rounding& q) { q.trials = T; });
        ok = ok && bad([](proxsdp_rounding& q) { q.max_sweeps = -1; }) && bad([](proxsdp_rounding& q) { q.max_sweeps = 1001; });
        ok = ok && bad([](proxsdp_rounding& q) { q.grid_search = -1; });
        ok = ok && bad([](proxsdp_rounding& q) { static int64_t p[5]; q.adj_ptr = p; });
        ok = ok && refuses([&] { check_rounding_factors(c.q, 1, true); });
        for (double v : {0.0, -1.0, (double)NAN, (double)INFINITY}) {
            std::vector<double> l2 = lam;
            l2[1] = v;
            Call d(4, 2, 64, 0, 10, V, l2);
            ok = ok && refuses([&] { check_rounding_factors(d.q, 4, true); }) && !refuses([&] { check_rounding_factors(d.q, 4, false); });
        }
        std::vector<double> V2 = V;
        V2[7] = (double)NAN;
        Call e(4, 2, 64, 0, 10, V2, lam);
        ok = ok && refuses([&] { check_rounding_factors(e.q, 4, true); });
        report("the refusals of the struct and the factors", ok);
    }
    {
        const int64_t ptr[4] = {0, 1, 2, 2}, col[2] = {1, 0};
        const double val[2] = {0.5, 0.5}, diag[3] = {0.0, 0.0, 0.0};
        bool ok = !refuses([&] { check_round_adjacency(3, ptr, col, val, diag); });
        const int64_t p1[4] = {1, 1, 2, 2}, p2[4] = {0, 2, 1, 2}, c1[2] = {0, 0}, c2[2] = {3, 0}, p3[4] = {0, 2, 2, 2}, c3[2] = {2, 1};
        const double v1[2] = {0.5, (double)NAN}, d1[3] = {0.0, (double)INFINITY, 0.0};
        ok = ok && refuses([&] { check_round_adjacency(3, p1, col, val, diag); }) && refuses([&] { check_round_adjacency(3, p2, col, val, diag); });
        ok = ok && refuses([&] { check_round_adjacency(3, ptr, c1, val, diag); }) && refuses([&] { check_round_adjacency(3, ptr, c2, val, diag); });
        ok = ok && refuses([&] { check_round_adjacency(3, p3, c3, val, diag); });
        ok = ok && refuses([&] { check_round_adjacency(3, ptr, col, v1, diag); }) && refuses([&] { check_round_adjacency(3, ptr, col, val, d1); });
        ok = ok && refuses([&] { check_round_adjacency(3, nullptr, col, val, diag); }) && refuses([&] { check_round_adjacency(3, ptr, nullptr, val, diag); });
        report("the refusals of a malformed adjacency", ok);
    }
    std::printf(failures ? "%d check(s) FAILED\n" : "all checks passed\n", failures);
    return failures ? 1 : 0;
}
