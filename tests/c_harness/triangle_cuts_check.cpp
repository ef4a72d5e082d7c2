// Stand-alone check of the host half of the triangle separation (proxsdp.jl_amd/csrc/triangle_cuts_host.hpp): no HIP, no
// library.  The serial restatement against a brute force written here a second time (all rows into one vector, a full
// std::sort under the documented order), on matrices with distinct and with all-equal violations, for counts below, at and
// above the number of violated rows; the untouched tail of the output arrays; the gate of a later sweep against the prefix
// test it stands in for; the slack rows of host vectors.  Built plain by tests/test_triangle_cuts_host.py; the same program
// is what -fsanitize=address,undefined is pointed at.
#include <cstdio>
#include <random>

#include "triangle_cuts_host.hpp"

using namespace proxsdp;

struct Row { double v; int64_t i, j, k; int p; };

static std::vector<Row> brute(const std::vector<double>& X, int64_t s, double minv, double rhs) {
    static const double sg[4][3] = {{-1, -1, -1}, {-1, 1, 1}, {1, -1, 1}, {1, 1, -1}};
    std::vector<Row> out;
    for (int64_t i = 0; i < s; ++i)
        for (int64_t j = i + 1; j < s; ++j)
            for (int64_t k = j + 1; k < s; ++k)
                for (int p = 0; p < 4; ++p) {
                    const double v = ((sg[p][0] * X[i * s + j] + sg[p][1] * X[i * s + k]) + sg[p][2] * X[j * s + k]) - rhs;
                    if (v > minv) out.push_back({v, i, j, k, p});
                }
    std::sort(out.begin(), out.end(), [](const Row& a, const Row& b) {
        if (a.v != b.v) return a.v > b.v;
        if (a.i != b.i) return a.i < b.i;
        if (a.j != b.j) return a.j < b.j;
        if (a.k != b.k) return a.k < b.k;
        return a.p < b.p;
    });
    return out;
}

struct Out {
    std::vector<int64_t> tri, col;
    std::vector<int32_t> pat;
    std::vector<double> vio, val, h;
    proxsdp_triangle_cuts tc{};
    Out(int64_t count, double minv, double rhs)
        : tri(3 * count, -7), col(3 * count, -7), pat(count, -7), vio(count, -7.0), val(3 * count, -7.0), h(count, -7.0) {
        tc.struct_size = sizeof tc; tc.count = count; tc.min_violation = minv; tc.rhs = rhs;
        tc.tri = tri.data(); tc.pattern = pat.data(); tc.violation = vio.data();
        tc.add_col = col.data(); tc.add_val = val.data(); tc.add_h = h.data();
    }
};

static int check(const char* name, const std::vector<double>& X, int64_t s, double minv, double rhs, int base) {
    const std::vector<Row> want = brute(X, s, minv, rhs);
    const int64_t nv = (int64_t)want.size();
    int bad = 0;
    for (int64_t count : {(int64_t)1, (int64_t)5, std::max<int64_t>(nv, 1), nv + 7}) {
        Out o(count, minv, rhs);
        check_triangle_struct(&o.tc, false);
        host_triangle_cuts(X.data(), s, nullptr, base, o.tc);
        const int64_t keep = std::min(count, nv);
        bad += o.tc.n_rows != keep || o.tc.violated != nv || o.tc.scanned != 4 * (s * (s - 1) * (s - 2) / 6);
        for (int64_t r = 0; r < keep && !bad; ++r) {
            const Row& w = want[r];
            bad += o.tri[3 * r] != w.i || o.tri[3 * r + 1] != w.j || o.tri[3 * r + 2] != w.k || o.pat[r] != w.p ||
                   std::memcmp(&o.vio[r], &w.v, sizeof(double)) != 0 || o.h[r] != rhs ||
                   o.col[3 * r] != w.j * (w.j + 1) / 2 + w.i + base || o.col[3 * r + 2] != w.k * (w.k + 1) / 2 + w.j + base;
        }
        for (int64_t r = keep; r < count; ++r) bad += o.pat[r] != -7 || o.tri[3 * r] != -7 || o.vio[r] != -7.0 || o.val[3 * r] != -7.0;
    }
    std::printf("%s (side %lld, %lld violated): %s\n", name, (long long)s, (long long)nv, bad ? "FAILED" : "ok");
    return bad;
}

int main() {
    int bad = 0;
    std::mt19937_64 rng(7);
    std::normal_distribution<double> nd;
    for (int64_t s : {3, 4, 12, 33}) {                              // Gram matrices of unit vectors in the plane / in space
        const int r = s < 12 ? 2 : 3;
        std::vector<double> V(s * r), X(s * s);
        for (int64_t i = 0; i < s; ++i) {
            double nn = 0.0;
            for (int q = 0; q < r; ++q) { V[i * r + q] = nd(rng); nn += V[i * r + q] * V[i * r + q]; }
            for (int q = 0; q < r; ++q) V[i * r + q] /= std::sqrt(nn);
        }
        for (int64_t i = 0; i < s; ++i)
            for (int64_t j = 0; j < s; ++j) {
                double d = 0.0;
                for (int q = 0; q < r; ++q) d += V[i * r + q] * V[j * r + q];
                X[i * s + j] = d;
            }
        bad += check("gram", X, s, 1e-3, 1.0, 0);
        bad += check("gram, rhs 0.9, base 1", X, s, 0.05, 0.9, 1);
    }
    for (int64_t s : {12, 40}) {                                    // all violations equal: the index order alone decides
        std::vector<double> X(s * s, -0.5);
        for (int64_t i = 0; i < s; ++i) X[i * s + i] = 1.0;
        bad += check("ties", X, s, 1e-3, 1.0, 0);
    }
    {                                                               // a cut matrix violates nothing
        const int64_t s = 12;
        std::vector<double> X(s * s);
        for (int64_t i = 0; i < s; ++i)
            for (int64_t j = 0; j < s; ++j) X[i * s + j] = ((i % 3 == 0) == (j % 3 == 0)) ? 1.0 : -1.0;
        bad += check("feasible", X, s, 1e-3, 1.0, 0);
    }
    {   // the gate: v passes it exactly when bits(v) >= the prefix padded with zeros, for prefixes of 12 .. 60 bits of real values
        int gbad = 0;
        std::uniform_real_distribution<double> ud(1e-3, 2.0);
        for (int t = 0; t < 20000; ++t) {
            const double a = ud(rng), b = t % 3 ? ud(rng) : std::nextafter(a, t % 2 ? 0.0 : 4.0);
            unsigned long long ab, bb;
            std::memcpy(&ab, &a, 8); std::memcpy(&bb, &b, 8);
            const int pbits = 12 * (1 + t % 5);
            const tri_u128 P = (tri_u128)(ab >> (64 - pbits));
            const double g = tri_gate(1e-3, P, pbits);
            const bool want = (bb >> (64 - pbits)) >= (ab >> (64 - pbits)) && b > 1e-3;
            gbad += (b > g) != want;
        }
        gbad += tri_gate(0.25, 0, 0) != 0.25 || tri_gate(0.25, 0, 24) != 0.25;
        std::printf("gate: %s\n", gbad ? "FAILED" : "ok");
        bad += gbad;
    }
    {   // slack rows of host vectors: thresholds, signed zero, NaN
        const double nan = std::numeric_limits<double>::quiet_NaN();
        const std::vector<double> d = {0.0, -0.0, 1e-8, -1e-8, std::nextafter(1e-8, 1.0), 0.5, nan, 0.0, 0.0};
        const std::vector<double> sl = {-1.0, -1.0, -1.0, -1.0, -1.0, -1.0, -1.0, -1e-3, nan};
        std::vector<int64_t> rows(d.size(), -7);
        proxsdp_inactive_rows q{};
        q.struct_size = sizeof q; q.dual_in = d.data(); q.slack_in = sl.data(); q.dual_tol = 1e-8; q.slack_tol = 1e-3; q.rows = rows.data();
        check_inactive_struct(&q);
        inactive_rows_host((int64_t)d.size(), q);
        const bool ok = q.n_rows == 4 && rows[0] == 0 && rows[1] == 1 && rows[2] == 2 && rows[3] == 3 && rows[4] == -7;
        std::printf("slack rows: %s\n", ok ? "ok" : "FAILED");
        bad += !ok;
    }
    return bad ? 1 : 0;
}
