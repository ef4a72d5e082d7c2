// Stand-alone check of the host half of the pentagonal / heptagonal separation (proxsdp.jl_amd/csrc/clique_cuts_host.hpp): no
// HIP, no library.  The serial restatement against a brute force written here a second time (every extension of every base
// into one vector, a full std::sort under the documented order, a std::map for the merge), on matrices with distinct and
// with all-equal values, for triangles and pentagons as bases; the untouched tail of the output arrays; the total order; the
// refusals of the two checks.  Built by tests/test_clique_cuts_host.py with -fsanitize=address,undefined (the runtimes linked
// statically) and run directly.
#include <cstdio>
#include <map>
#include <random>

#include "clique_cuts_host.hpp"

using namespace proxsdp;

struct Ext { double v; int64_t l, m; int code; };
struct Want { std::vector<int64_t> nodes; std::vector<int> signs; double v; int64_t base; };

static double xat(const std::vector<double>& X, int64_t s, int64_t i, int64_t j) { return i < j ? X[i * s + j] : X[j * s + i]; }

static std::vector<Want> brute(const std::vector<double>& X, int64_t s, int q, const std::vector<int64_t>& nodes,
                               const std::vector<int8_t>& sign, double minv, double rhs, int64_t* violated) {
    const int64_t nb = (int64_t)nodes.size() / q;
    std::map<std::pair<std::vector<int64_t>, std::vector<int>>, std::pair<double, int64_t>> found;
    *violated = 0;
    for (int64_t b = 0; b < nb; ++b) {
        const int64_t* a = &nodes[b * q];
        const int8_t* sg = &sign[b * q];
        double B = 0.0;
        bool first = true;
        for (int u = 0; u < q; ++u)
            for (int w = u + 1; w < q; ++w) {
                const double term = (double)(-sg[u] * sg[w]) * xat(X, s, a[u], a[w]);
                B = first ? term : B + term;
                first = false;
            }
        auto in_base = [&](int64_t l) { return std::find(a, a + q, l) != a + q; };
        auto tt = [&](int64_t l) {
            double t = (double)sg[0] * xat(X, s, a[0], l);
            for (int u = 1; u < q; ++u) t = t + (double)sg[u] * xat(X, s, a[u], l);
            return t;
        };
        std::vector<Ext> all;
        for (int64_t l = 0; l < s; ++l)
            for (int64_t m = l + 1; m < s; ++m) {
                if (in_base(l) || in_base(m)) continue;
                for (int c = 0; c < 4; ++c) {
                    const double tl = c & 2 ? -1.0 : 1.0, tm = c & 1 ? -1.0 : 1.0;
                    all.push_back({(((B - tl * tt(l)) - tm * tt(m)) - (tl * tm) * xat(X, s, l, m)) - rhs, l, m, c});
                }
            }
        std::sort(all.begin(), all.end(), [](const Ext& x, const Ext& y) {
            if (x.v != y.v) return x.v > y.v;
            if (x.l != y.l) return x.l < y.l;
            if (x.m != y.m) return x.m < y.m;
            return x.code < y.code;
        });
        const Ext& e = all.front();
        if (!(e.v > minv)) continue;
        ++*violated;
        std::vector<std::pair<int64_t, int>> both;
        for (int u = 0; u < q; ++u) both.push_back({a[u], (int)sg[u]});
        both.push_back({e.l, e.code & 2 ? -1 : 1});
        both.push_back({e.m, e.code & 1 ? -1 : 1});
        std::sort(both.begin(), both.end());
        std::vector<int64_t> nn;
        std::vector<int> ss;
        for (auto& p : both) { nn.push_back(p.first); ss.push_back(p.second * both[0].second); }
        auto it = found.find({nn, ss});
        if (it == found.end() || e.v > it->second.first) found[{nn, ss}] = {e.v, b};
    }
    std::vector<Want> out;
    for (auto& f : found) out.push_back({f.first.first, f.first.second, f.second.first, f.second.second});
    std::sort(out.begin(), out.end(), [](const Want& x, const Want& y) { return x.v != y.v ? x.v > y.v : x.base < y.base; });
    return out;
}

struct Out {
    std::vector<int64_t> nodes, from, col;
    std::vector<int8_t> signs;
    std::vector<double> vio, val, h;
    proxsdp_clique_cuts q{};
    Out(int bq, const std::vector<int64_t>& bn, const std::vector<int8_t>& bs, double minv, double rhs) {
        const int64_t nb = (int64_t)bn.size() / bq;
        const int k = bq + 2, np = k * (k - 1) / 2;
        nodes.assign(nb * k, -7); from.assign(nb, -7); col.assign(nb * np, -7); signs.assign(nb * k, -7);
        vio.assign(nb, -7.0); val.assign(nb * np, -7.0); h.assign(nb, -7.0);
        q.struct_size = sizeof q; q.base_size = bq; q.n_base = nb; q.min_violation = minv; q.rhs = rhs;
        q.base_nodes = bn.data(); q.base_sign = bs.data();
        q.nodes = nodes.data(); q.signs = signs.data(); q.violation = vio.data(); q.from_base = from.data();
        q.add_col = col.data(); q.add_val = val.data(); q.add_h = h.data();
    }
};

static int check(const char* name, const std::vector<double>& X, int64_t s, int bq, const std::vector<int64_t>& bn,
                 const std::vector<int8_t>& bs, double minv, double rhs, int base) {
    int64_t violated = 0;
    const std::vector<Want> want = brute(X, s, bq, bn, bs, minv, rhs, &violated);
    const int k = bq + 2, np = k * (k - 1) / 2;
    Out o(bq, bn, bs, minv, rhs);
    check_clique_struct(&o.q, false);
    check_clique_bases(o.q, s);
    host_clique_cuts(X.data(), s, nullptr, base, o.q);
    const int64_t nb = o.q.n_base, n = (int64_t)want.size();
    int bad = o.q.n_rows != n || o.q.violated_bases != violated || o.q.scanned != nb * 4 * ((s - bq) * (s - bq - 1) / 2);
    for (int64_t r = 0; r < n && !bad; ++r) {
        const Want& w = want[r];
        for (int u = 0; u < k; ++u) bad += o.nodes[r * k + u] != w.nodes[u] || o.signs[r * k + u] != w.signs[u];
        bad += std::memcmp(&o.vio[r], &w.v, sizeof(double)) != 0 || o.from[r] != w.base || o.h[r] != rhs;
        int e = 0;
        for (int u = 0; u < k; ++u)
            for (int x = u + 1; x < k; ++x, ++e)
                bad += o.col[r * np + e] != w.nodes[x] * (w.nodes[x] + 1) / 2 + w.nodes[u] + base ||
                       o.val[r * np + e] != (double)(-w.signs[u] * w.signs[x]);
    }
    for (int64_t r = n; r < nb; ++r)
        bad += o.nodes[r * k] != -7 || o.signs[r * k] != -7 || o.vio[r] != -7.0 || o.from[r] != -7 || o.col[r * np] != -7 ||
               o.val[r * np] != -7.0 || o.h[r] != -7.0;
    std::printf("%s (side %lld, q %d, %lld bases, %lld rows): %s\n", name, (long long)s, bq, (long long)nb, (long long)n,
                bad ? "FAILED" : "ok");
    return bad;
}

// every q-subset of 0 .. s-1 whose number is a multiple of `step`, with signs from the generator (the first +1)
static void subsets(int64_t s, int q, int step, std::mt19937_64& rng, std::vector<int64_t>& bn, std::vector<int8_t>& bs) {
    bn.clear(); bs.clear();
    std::vector<int64_t> a(q);
    for (int u = 0; u < q; ++u) a[u] = u;
    for (int64_t c = 0;; ++c) {
        if (c % step == 0)
            for (int u = 0; u < q; ++u) { bn.push_back(a[u]); bs.push_back(u == 0 || (rng() & 1) ? 1 : -1); }
        int u = q - 1;
        while (u >= 0 && a[u] == s - q + u) --u;
        if (u < 0) break;
        ++a[u];
        for (int w = u + 1; w < q; ++w) a[w] = a[w - 1] + 1;
    }
}

template <typename F>
static int refused(const char* text, F&& f) {
    try { f(); } catch (const std::invalid_argument& e) { return std::strstr(e.what(), text) ? 0 : 1; }
    return 1;
}

int main() {
    int bad = 0;
    std::mt19937_64 rng(7);
    std::normal_distribution<double> nd;
    std::vector<int64_t> bn;
    std::vector<int8_t> bs;
    for (int64_t s : {5, 7, 12, 33}) {                              // Gram matrices of unit vectors in space
        const int r = 3;
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
        subsets(s, 3, s > 12 ? 11 : 1, rng, bn, bs);
        bad += check("gram, triangles", X, s, 3, bn, bs, 1e-3, 2.0, 0);
        bad += check("gram, triangles, rhs 1.9, base 1", X, s, 3, bn, bs, 0.05, 1.9, 1);
        if (s >= 7) {
            subsets(s, 5, s > 12 ? 977 : (s > 7 ? 3 : 1), rng, bn, bs);
            bad += check("gram, pentagons", X, s, 5, bn, bs, 1e-3, 3.0, 0);
        }
    }
    for (int64_t s : {7, 40}) {                                     // all values equal: the order of (l, m, code) alone decides
        std::vector<double> X(s * s, -0.5);
        for (int64_t i = 0; i < s; ++i) X[i * s + i] = 1.0;
        bn = {0, 1, 2, 3, 4, 5, 0, 2, s - 1};
        bs.assign(9, 1);
        bad += check("ties, triangles", X, s, 3, bn, bs, 1e-3, 2.0, 0);
        bn = {0, 1, 2, 3, 4};
        bs.assign(5, 1);
        bad += check("ties, pentagon", X, s, 5, bn, bs, 1e-3, 3.0, 0);
    }
    {                                                               // a cut matrix yields no row
        const int64_t s = 12;
        std::vector<double> X(s * s);
        for (int64_t i = 0; i < s; ++i)
            for (int64_t j = 0; j < s; ++j) X[i * s + j] = ((i % 3 == 0) == (j % 3 == 0)) ? 1.0 : -1.0;
        subsets(s, 3, 1, rng, bn, bs);
        bad += check("feasible", X, s, 3, bn, bs, 0.0, 2.0, 0);
    }
    {   // the total order: greater v, then the smaller key; a NaN is never better
        const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
        const bool ok = clique_better(1.0, 9, 0.5, 1) && !clique_better(0.5, 1, 1.0, 9) && clique_better(1.0, 3, 1.0, 4) &&
                        !clique_better(1.0, 4, 1.0, 4) && !clique_better(nan, 0, -inf, CLQ_NO_KEY) &&
                        clique_better(-1.0, 7, -inf, CLQ_NO_KEY);
        std::printf("order: %s\n", ok ? "ok" : "FAILED");
        bad += !ok;
    }
    {   // refusals of the two checks
        bn = {0, 1, 2, 1, 3, 4};
        bs = {1, -1, 1, 1, 1, -1};
        int rbad = 0;
        auto with = [&](auto&& damage) { Out o(3, bn, bs, 1e-3, 2.0); damage(o); check_clique_struct(&o.q, true); check_clique_bases(o.q, 5); };
        const double one = 1.0;
        auto fine = [&](Out& o) { o.q.primal = &one; };
        rbad += refused("struct_size", [&] { with([&](Out& o) { fine(o); o.q.struct_size -= 8; }); });
        rbad += refused("on_device", [&] { with([&](Out& o) { fine(o); o.q.on_device = 2; }); });
        rbad += refused("base_size", [&] { with([&](Out& o) { fine(o); o.q.base_size = 4; }); });
        rbad += refused("n_base", [&] { with([&](Out& o) { fine(o); o.q.n_base = 0; }); });
        rbad += refused("n_base", [&] { with([&](Out& o) { fine(o); o.q.n_base = 65537; }); });
        rbad += refused("rhs", [&] { with([&](Out& o) { fine(o); o.q.rhs = std::numeric_limits<double>::infinity(); }); });
        rbad += refused("min_violation", [&] { with([&](Out& o) { fine(o); o.q.min_violation = -1e-9; }); });
        rbad += refused("grid", [&] { with([&](Out& o) { fine(o); o.q.grid = -1; }); });
        rbad += refused("batch", [&] { with([&](Out& o) { fine(o); o.q.batch = -1; }); });
        rbad += refused("primal is NULL", [&] { with([&](Out&) {}); });
        rbad += refused("base_nodes is NULL", [&] { with([&](Out& o) { fine(o); o.q.base_nodes = nullptr; }); });
        rbad += refused("base_sign is NULL", [&] { with([&](Out& o) { fine(o); o.q.base_sign = nullptr; }); });
        rbad += refused("NULL output", [&] { with([&](Out& o) { fine(o); o.q.from_base = nullptr; }); });
        rbad += refused("outside the cone", [&] { bn[5] = 5; with(fine); });
        bn[5] = 4;
        rbad += refused("outside the cone", [&] { bn[0] = -1; with(fine); });
        bn[0] = 0;
        rbad += refused("not strictly ascending", [&] { bn[4] = 1; with(fine); });
        bn[4] = 3;
        rbad += refused("not +-1", [&] { bs[2] = 0; with(fine); });
        bs[2] = 1;
        rbad += refused("first sign", [&] { bs[3] = -1; with(fine); });
        bs[3] = 1;
        try { with(fine); } catch (const std::exception&) { ++rbad; }
        rbad += refused("NULL proxsdp_clique_cuts", [&] { check_clique_struct(nullptr, true); });
        std::printf("refusals: %s\n", rbad ? "FAILED" : "ok");
        bad += rbad;
    }
    return bad ? 1 : 0;
}
