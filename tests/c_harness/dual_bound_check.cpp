// Stand-alone check of the host half of the certified dual bound (proxsdp.jl_amd/csrc/dual_bound_host.hpp): no HIP, no
// library.  The serial Cholesky on exact integer products and on its failure cases, against a second factorisation written
// here (row by row, long double); the planner of the shift search against its stated sequence; the directed rounding of
// gamma, delta and the combination; the trace caps; the whole host bound on a model with a known optimum; the refusals of the
// checks.  Built by tests/test_dual_bound_host.py with -fsanitize=address,undefined (the runtimes linked statically) and run
// directly.
#include <cstdio>
#include <random>

#include "dual_bound_host.hpp"

using namespace proxsdp;

static int failures = 0;
static void report(const char* name, bool ok) {
    std::printf("%s: %s\n", name, ok ? "ok" : "FAILED");
    if (!ok) ++failures;
}

// L: s x s lower triangular with small integers (unit diagonal or 1 .. 3), row-major
static std::vector<double> integer_factor(int64_t s, unsigned seed, bool unit) {
    std::mt19937 g(seed);
    std::uniform_int_distribution<int> off(-2, 2), dg(1, 3);
    std::vector<double> L((size_t)(s * s), 0.0);
    for (int64_t i = 0; i < s; ++i) {
        for (int64_t j = 0; j < i; ++j) L[(size_t)(i * s + j)] = off(g);
        L[(size_t)(i * s + i)] = unit ? 1.0 : dg(g);
    }
    return L;
}
// A = L L' (symmetric: row-major = column-major)
static std::vector<double> product(const std::vector<double>& L, int64_t s) {
    std::vector<double> A((size_t)(s * s), 0.0);
    for (int64_t i = 0; i < s; ++i)
        for (int64_t j = 0; j < s; ++j) {
            double a = 0.0;
            for (int64_t k = 0; k <= std::min(i, j); ++k) a += L[(size_t)(i * s + k)] * L[(size_t)(j * s + k)];
            A[(size_t)(i * s + j)] = a;
        }
    return A;
}
// the second factorisation: row by row (Cholesky-Banachiewicz) in long double; returns the failing row or -1
static int64_t cholesky2(const std::vector<double>& A, int64_t s, std::vector<long double>& L) {
    L.assign((size_t)(s * s), 0.0L);
    for (int64_t i = 0; i < s; ++i)
        for (int64_t j = 0; j <= i; ++j) {
            long double a = A[(size_t)(i * s + j)];
            for (int64_t k = 0; k < j; ++k) a -= L[(size_t)(i * s + k)] * L[(size_t)(j * s + k)];
            if (i == j) { if (!(a > 0.0L)) return i; L[(size_t)(i * s + i)] = std::sqrt(a); }
            else L[(size_t)(i * s + j)] = a / L[(size_t)(j * s + j)];
        }
    return -1;
}

static void check_exact_products() {
    bool ok = true;
    for (int64_t s : {1, 2, 7, 16, 33, 65})
        for (int unit = 0; unit < 2; ++unit) {
            const std::vector<double> L = integer_factor(s, (unsigned)(10 * s + unit), unit != 0);
            std::vector<double> W = product(L, s);
            ok = ok && host_cholesky(W.data(), s, 0.0) == -1;
            for (int64_t j = 0; j < s; ++j)
                for (int64_t i = j; i < s; ++i) ok = ok && W[(size_t)(j * s + i)] == L[(size_t)(i * s + j)];
        }
    report("exact integer products factor bit for bit", ok);
}

static void check_failures() {
    bool ok = true;
    for (int64_t s : {1, 2, 9, 40}) {
        const std::vector<double> L = integer_factor(s, (unsigned)s, false);
        std::vector<double> A = product(L, s);
        A[(size_t)(s * s - 1)] -= L[(size_t)(s * s - 1)] * L[(size_t)(s * s - 1)] + 1.0;
        std::vector<double> W = A;
        ok = ok && host_cholesky(W.data(), s, 0.0) == s - 1;
        std::vector<double> Zr((size_t)(s * s), 0.0), N((size_t)(s * s), std::nan(""));
        ok = ok && host_cholesky(Zr.data(), s, 0.0) == 0 && host_cholesky(N.data(), s, 0.0) == 0;
        // the strict upper triangle is neither read nor written
        std::vector<double> U = product(L, s);
        for (int64_t j = 0; j < s; ++j)
            for (int64_t i = 0; i < j; ++i) U[(size_t)(j * s + i)] = std::nan("");
        ok = ok && host_cholesky(U.data(), s, 0.0) == -1;
        for (int64_t j = 0; j < s; ++j)
            for (int64_t i = 0; i < j; ++i) ok = ok && std::isnan(U[(size_t)(j * s + i)]);
    }
    // the pivot floor: a pivot equal to the floor fails
    double one = 4.0;
    ok = ok && host_cholesky(&one, 1, 4.0) == 0;
    one = 4.0;
    ok = ok && host_cholesky(&one, 1, 3.5) == -1 && one == 2.0;
    report("bad pivots, NaN and the floor are results", ok);
}

static void check_against_second_factorisation() {
    bool ok = true;
    std::mt19937 g(5);
    std::normal_distribution<double> nd;
    for (int64_t s : {3, 17, 64, 90}) {
        std::vector<double> G((size_t)(s * (s + 2))), A((size_t)(s * s));
        for (double& v : G) v = nd(g);
        for (int64_t i = 0; i < s; ++i)
            for (int64_t j = 0; j <= i; ++j) {
                double a = i == j ? 0.25 : 0.0;
                for (int64_t k = 0; k < s + 2; ++k) a += G[(size_t)(i * (s + 2) + k)] * G[(size_t)(j * (s + 2) + k)] / (double)s;
                A[(size_t)(i * s + j)] = A[(size_t)(j * s + i)] = a;
            }
        std::vector<long double> L2;
        std::vector<double> W = A;
        ok = ok && cholesky2(A, s, L2) == -1 && host_cholesky(W.data(), s, 0.0) == -1;
        const double g1 = bound_gamma((double)(s + 1));
        for (int64_t i = 0; i < s; ++i)
            for (int64_t j = 0; j <= i; ++j) {
                long double rr = 0.0L;                              // (R'R)_ij of the fp64 factor, in long double
                for (int64_t k = 0; k <= j; ++k) rr += (long double)W[(size_t)(k * s + i)] * (long double)W[(size_t)(k * s + j)];
                const long double lim = (long double)(g1 / (1.0 - g1)) * std::sqrt((long double)A[(size_t)(i * s + i)] * A[(size_t)(j * s + j)]);
                ok = ok && std::fabs(rr - (long double)A[(size_t)(i * s + j)]) <= lim;
                ok = ok && std::fabs((long double)W[(size_t)(j * s + i)] - L2[(size_t)(i * s + j)]) <= 1e-9L;
            }
    }
    report("real matrices: the backward-error bound and a second factorisation", ok);
}

static void check_search() {
    bool ok = true;
    // a threshold t: a try completes exactly when sigma >= t
    auto run = [&](double nu, double t, std::vector<double>& tried) {
        ShiftSearch S(nu);
        tried.clear();
        while (!S.done()) { const double sg = S.next(); tried.push_back(sg); S.report(sg >= t); }
        return S;
    };
    std::vector<double> tried;
    ShiftSearch a = run(8.0, 0.0, tried);
    ok = ok && a.certified && a.best() == 0.0 && a.tries == 1;
    a = run(8.0, 1e-300, tried);                                    // completes at j = 0: no bisection
    ok = ok && a.certified && a.tries == 2 && a.best() == std::ldexp(8.0, -48);
    a = run(8.0, 0.3, tried);
    ok = ok && a.certified && a.best() >= 0.3 && a.best() <= 0.3 * std::pow(16.0, 1.0 / 32.0) * (1 + 1e-12);
    ok = ok && tried[0] == 0.0;
    int grid = 0;
    for (size_t q = 1; q < tried.size() && tried[q] < 0.3; ++q) { ok = ok && tried[q] == std::ldexp(8.0, -48 + 4 * (int)(q - 1)); ++grid; }
    ok = ok && a.tries == 1 + (grid + 1) + 5 && a.tries <= 19;
    a = run(8.0, 8.0, tried);                                       // only sigma_12 = nu completes
    ok = ok && a.certified && a.tries == 19 && a.best() <= 8.0;
    a = run(8.0, 9.0, tried);
    ok = ok && !a.certified && a.tries == 14 && tried.back() == 8.0;
    a = run(0.0, 1.0, tried);
    ok = ok && !a.certified && a.tries == 14;
    a = run(1e308, 1e300, tried);                                   // no overflow in the geometric mean
    ok = ok && a.certified && std::isfinite(a.best()) && a.best() >= 1e300;
    report("the shift search follows its stated sequence", ok);
}

static void check_rounding() {
    bool ok = true;
    for (double j : {1.0, 3.0, 260.0, 46343.0, 1e9}) {
        const long double ju = (long double)j * 0x1p-53L, exact = ju / (1.0L - ju);
        ok = ok && (long double)bound_gamma(j) >= exact && (long double)bound_gamma(j) <= exact * (1.0L + 1e-15L);
    }
    std::vector<double> d = {1.0, 3.0, 0.1, 7.5};
    const double dl = bound_delta(d.data(), 4, 0.5);
    const long double g = 7.0L * 0x1p-53L / (1.0L - 7.0L * 0x1p-53L);
    const long double want = g / (1.0L - g) * 13.6L + 0x1p-53L * 8.0L;
    ok = ok && (long double)dl >= want && (long double)dl <= want * (1.0L + 1e-14L);
    const double T[2] = {3.0, 5.0}, low[2] = {-0.1, 0.7};
    const int32_t cert[2] = {1, 1}, not_cert[2] = {1, 0};
    const double b = bound_combine(2.0, 4.0, 10, 2, T, low, cert);
    const long double exact = 2.0L - (12.0L * 0x1p-53L / (1.0L - 12.0L * 0x1p-53L)) * 4.0L - 0.3L;
    ok = ok && (long double)b <= exact && (long double)b >= exact - 1e-14L;
    ok = ok && bound_combine(2.0, 4.0, 10, 2, T, low, not_cert) == -std::numeric_limits<double>::infinity();
    report("gamma, delta and the combination are rounded to the safe side", ok);
}

static void check_caps() {
    bool ok = true;
    // 3 diagonal columns 0, 2, 5 of a side-3 cone; rows: 0: 2 x0 = 3; 1: x2 = 1; 2: x5 = 4; 3: -x5 = -2; 4: x0 + x1 = 9
    const int64_t colptr[7] = {0, 2, 3, 4, 4, 4, 6};
    const int64_t rowidx[6] = {0, 4, 4, 1, 2, 3};
    const double val[6] = {2.0, 1.0, 1.0, 1.0, 1.0, -1.0};
    const double b[5] = {3.0, 1.0, 4.0, -2.0, 9.0};
    std::vector<int32_t> cnt = {1, 1, 1, 1, 2};
    auto diag = [](int64_t i) { return i * (i + 3) / 2; };
    const double T = bound_trace_cap(3, diag, colptr, rowidx, 0, val, cnt, b, 5, 0);
    double want = 0.0;
    for (double c : {1.5, 1.0, 2.0}) want = bound_up(want + bound_up(c));
    ok = ok && T == want;
    // row 0 made an inequality (p = 0 .. : rows >= p do not count): diagonal 0 is uncovered
    bool threw = false;
    try { (void)bound_trace_cap(3, diag, colptr, rowidx, 0, val, cnt, b, 0, 4); } catch (const std::invalid_argument& e) {
        threw = std::string(e.what()).find("cone 4") != std::string::npos;
    }
    ok = ok && threw;
    const double bneg[5] = {-3.0, 1.0, 4.0, -2.0, 9.0};
    threw = false;
    try { (void)bound_trace_cap(3, diag, colptr, rowidx, 0, val, cnt, bneg, 5, 0); } catch (const std::invalid_argument&) { threw = true; }
    ok = ok && threw;
    report("trace caps from the equality rows", ok);
}

struct Out {
    std::vector<double> shift, low, rad, delta, T;
    std::vector<int32_t> tries, cert;
    proxsdp_dual_bound q{};
    explicit Out(size_t k) : shift(k, 7), low(k, 7), rad(k, 7), delta(k, 7), T(k, 7), tries(k, 7), cert(k, 7) {
        q.struct_size = sizeof(proxsdp_dual_bound);
        q.shift = shift.data(); q.lambda_lower = low.data(); q.radius = rad.data(); q.delta = delta.data();
        q.trace_used = T.data(); q.factorisations = tries.data(); q.certified = cert.data();
    }
};

static void check_known_optimum() {
    bool ok = true;
    for (int64_t s : {1, 2, 6, 19}) {
        // Z = (s I - v v') B (s I - v v'), B = g g' (rank one), C = Z - Diag(y), rows X_ii = 1, duals y - eta
        std::mt19937 g((unsigned)s);
        std::uniform_int_distribution<int> sg(0, 1), gi(-2, 2), yi(-5, 5);
        std::vector<double> v((size_t)s), gv((size_t)s), y((size_t)s), w((size_t)s);
        double vg = 0.0, ysum = 0.0;
        for (int64_t i = 0; i < s; ++i) { v[i] = sg(g) ? 1.0 : -1.0; gv[i] = gi(g); y[i] = yi(g); vg += v[i] * gv[i]; ysum += y[i]; }
        for (int64_t i = 0; i < s; ++i) w[i] = (double)s * gv[i] - v[i] * vg;          // (s I - v v') g
        const int64_t N = s * (s + 1) / 2;
        std::vector<double> c((size_t)N), nz((size_t)s, 1.0), bh((size_t)s, 1.0), ye((size_t)s);
        std::vector<int64_t> colptr((size_t)N + 1, 0), rowval((size_t)s), idx((size_t)N), ptr = {0, N};
        for (int64_t j = 0, e = 0; j < s; ++j)
            for (int64_t i = 0; i <= j; ++i, ++e) {
                c[(size_t)e] = i == j ? w[i] * w[i] - y[i] : 2.0 * w[i] * w[j];
                idx[(size_t)e] = e;
                colptr[(size_t)e + 1] = colptr[(size_t)e] + (i == j ? 1 : 0);
                if (i == j) rowval[(size_t)colptr[(size_t)e]] = i;
            }
        const double eta = 0.125;
        for (int64_t i = 0; i < s; ++i) ye[i] = y[i] - eta;
        proxsdp_csc M{s, N, colptr.data(), rowval.data(), nz.data()};
        Out o(1);
        o.q.dual_eq = ye.data();
        check_bound_struct(&o.q, s, 0, 1, false);
        host_dual_bound(N, s, 0, c.data(), M, bh.data(), 1, ptr.data(), idx.data(), 0, o.q);
        // lambda_min(Z - eta I) = -eta exactly (Z v = 0), the ideal bound is p* = -sum(y)
        ok = ok && o.cert[0] == 1 && o.q.bound <= -ysum && o.q.bound >= -ysum - (double)s * (0.1 * eta + 1e-6);
        ok = ok && o.q.dual_objective == -(ysum - (double)s * eta) && o.low[0] <= -eta && o.tries[0] <= 19;
    }
    report("the host bound on a model with a known optimum", ok);
}

static void check_refusals() {
    bool ok = true;
    auto refused = [](auto&& f) { try { f(); } catch (const std::invalid_argument&) { return true; } catch (const std::domain_error&) { return true; } return false; };
    Out o(1);
    double y[2] = {1.0, std::nan("")}, cap_bad[1] = {-1.0};
    o.q.dual_eq = y;
    ok = ok && refused([&] { check_bound_struct(nullptr, 1, 0, 1, false); });
    ok = ok && refused([&] { check_bound_struct(&o.q, 2, 0, 1, false); });              // a NaN dual
    ok = ok && !refused([&] { check_bound_struct(&o.q, 1, 0, 1, false); });
    o.q.on_device = 1;
    ok = ok && refused([&] { check_bound_struct(&o.q, 1, 0, 1, false); }) && !refused([&] { check_bound_struct(&o.q, 2, 0, 1, true); });
    o.q.on_device = 0; o.q.trace_cap = cap_bad;
    ok = ok && refused([&] { check_bound_struct(&o.q, 1, 0, 1, false); });
    o.q.trace_cap = nullptr; o.q.radius = nullptr;
    ok = ok && refused([&] { check_bound_struct(&o.q, 1, 0, 1, false); });
    const int64_t ptr[2] = {0, 3}, idx[3] = {0, 1, 2}, twice[3] = {0, 1, 1}, ptr2[2] = {0, 2};
    ok = ok && bound_cone_sides(3, 1, ptr, idx, 0) == std::vector<int64_t>{2};
    ok = ok && refused([&] { (void)bound_cone_sides(4, 1, ptr, idx, 0); });             // a variable outside every cone
    ok = ok && refused([&] { (void)bound_cone_sides(3, 1, ptr, twice, 0); });
    ok = ok && refused([&] { (void)bound_cone_sides(2, 1, ptr2, idx, 0); });            // not a triangle
    report("the checks refuse what the header says", ok);
}

int main() {
    check_exact_products();
    check_failures();
    check_against_second_factorisation();
    check_search();
    check_rounding();
    check_caps();
    check_known_optimum();
    check_refusals();
    std::printf(failures ? "%d check(s) FAILED\n" : "all checks passed\n", failures);
    return failures ? 1 : 0;
}
