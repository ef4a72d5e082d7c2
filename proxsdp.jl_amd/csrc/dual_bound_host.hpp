// The HIP-free half of the certified dual bound (include/proxsdp_hip.h "a certified dual bound"): the argument checks, the
// directed-rounding helpers, the plain serial column Cholesky, the planner of the shift search, the trace caps, the final
// combination, and proxsdp_host_dual_bound -- the whole contract with no device and no handle.  The device half
// (dual_bound.hip.hpp) replaces the forming of the dual matrix, the reductions and the factorisation by kernels and shares
// everything else.  No Lanczos, no eigenvalue estimate and no solver tolerance enters: the proof of a cone's figure is a
// completed floating-point Cholesky factorisation with its backward-error bound (Higham, Accuracy and Stability of Numerical
// Algorithms, 2nd ed., Theorem 10.3 / section 10.1; Rump, BIT 46 (2006)).
#pragma once
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>
#include "prep.hpp"
#include "struct_check.hpp"

namespace proxsdp {

constexpr int64_t BOUND_MAX_SIDE = 46340;
constexpr double BOUND_U = 0x1p-53;                 // unit round-off of fp64
constexpr int BOUND_GRID_STEPS = 13;                // sigma_j = nu 2^(-48 + 4 j), j = 0 .. 12
constexpr int BOUND_BISECTIONS = 5;

inline double bound_up(double x) { return std::nextafter(x, std::numeric_limits<double>::infinity()); }
inline double bound_down(double x) { return std::nextafter(x, -std::numeric_limits<double>::infinity()); }
inline double bound_clock() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// gamma(j) = j u / (1 - j u), rounded up (j u is exact: a scaling by a power of two)
inline double bound_gamma(double j) {
    const double ju = j * BOUND_U;
    return bound_up(ju / bound_down(1.0 - ju));
}

// the pivot threshold of a factorisation: a pivot must exceed 2^-500 nu
inline double bound_pivot_floor(double nu) { return std::ldexp(nu, -500); }

// delta of a completed factorisation of A(sigma): gamma(s + 3) / (1 - gamma(s + 3)) tr+(A) + u max |a_ii|, a_ii = fl(z_ii +
// sigma), every operation rounded up.  The first term bounds the 2-norm of R~'R~ - A (entrywise at most
// gamma(s + 1) / (1 - gamma(s + 1)) sqrt(a_ii a_jj), a rank-one matrix of norm tr A), the second the rounding of the diagonal.
inline double bound_delta(const double* zdiag, int64_t s, double sigma) {
    double tr = 0.0, mx = 0.0;
    for (int64_t i = 0; i < s; ++i) {
        const double a = zdiag[i] + sigma;
        tr = bound_up(tr + std::fabs(a));
        mx = std::max(mx, std::fabs(a));
    }
    const double g = bound_gamma((double)(s + 3));
    const double f = bound_up(g / bound_down(1.0 - g));
    return bound_up(bound_up(f * tr) + bound_up(BOUND_U * mx));
}

// The plain serial column Cholesky of the lower triangle, in place.  A: column-major, ld = s, entry (i, j), i >= j, at
// A[j * s + i]; the strict upper triangle is neither read nor written.  Column j: a_ij -= l_ik l_jk for k < j in order, the
// pivot test a_jj > floor (a NaN fails it), l_jj = sqrt(a_jj), l_ij = a_ij / l_jj.  Returns -1 when it completed, else the
// first failing column (the columns before it hold L, the rest is partly updated).
inline int64_t host_cholesky(double* A, int64_t s, double floor) {
    for (int64_t j = 0; j < s; ++j) {
        double* aj = A + j * s;
        for (int64_t k = 0; k < j; ++k) {
            const double* ak = A + k * s;
            const double ljk = ak[j];
            for (int64_t i = j; i < s; ++i) aj[i] -= ak[i] * ljk;
        }
        const double piv = aj[j];
        if (!(piv > floor)) return j;
        const double d = std::sqrt(piv);
        aj[j] = d;
        for (int64_t i = j + 1; i < s; ++i) aj[i] = aj[i] / d;
    }
    return -1;
}

// The shift search, decided only by "completed" or "failed": sigma = 0; then sigma_j = nu 2^(-48 + 4 j), j = 0 .. 12, until
// one completes; when that was at j >= 1, five bisection steps by the geometric mean between the last failure and the first
// success.  At most 1 + 13 + 5 = 19 tries.  next() gives the shift to try, report() takes the outcome.
struct ShiftSearch {
    double nu = 0.0, lo = 0.0, hi = 0.0;
    int stage = 0;                                  // 0: sigma = 0; 1: the grid; 2: bisection; 3: done
    int j = 0, bis = 0, tries = 0;
    bool certified = false;
    explicit ShiftSearch(double nu_) : nu(nu_) {}
    bool done() const { return stage == 3; }
    double next() const {
        if (stage == 0) return 0.0;
        if (stage == 1) return std::ldexp(nu, -48 + 4 * j);
        return std::sqrt(lo) * std::sqrt(hi);
    }
    void report(bool ok) {
        const double sigma = next();
        ++tries;
        if (stage == 0) {
            if (ok) { hi = 0.0; certified = true; stage = 3; } else { lo = 0.0; stage = 1; }
        } else if (stage == 1) {
            if (ok) {
                hi = sigma; certified = true;
                stage = j >= 1 ? 2 : 3;
            } else {
                lo = sigma;
                if (++j == BOUND_GRID_STEPS) stage = 3;
            }
        } else {
            if (ok) hi = sigma; else lo = sigma;
            if (++bis == BOUND_BISECTIONS) stage = 3;
        }
    }
    double best() const { return hi; }              // the smallest completed shift (when certified)
};

// One cone of side >= 2: runs the search through try_shift(sigma) -> completed?, and writes the cone's outputs.
// lambda_lower = -(sigma* + delta(sigma*) + rho), every sum rounded up before the sign.
template <class Try>
void bound_certify_cone(int64_t s, const double* zdiag, double nu, double rho, Try&& try_shift, double& shift,
                        double& lambda_lower, double& delta, int32_t& tries, int32_t& certified) {
    ShiftSearch S(nu);
    while (!S.done()) S.report(try_shift(S.next()));
    tries = S.tries;
    certified = S.certified ? 1 : 0;
    if (!S.certified) {
        shift = std::numeric_limits<double>::infinity(); delta = 0.0;
        lambda_lower = -std::numeric_limits<double>::infinity();
        return;
    }
    shift = S.best();
    delta = bound_delta(zdiag, s, shift);
    lambda_lower = -bound_up(bound_up(shift + delta) + rho);
}

// d_safe = d - gamma(Q + 2) D and bound = d_safe + sum_k T_k min(0, l_k), every product and sum rounded down
inline double bound_combine(double d, double D, int64_t Q, int64_t n_psd, const double* T, const double* lower, const int32_t* certified) {
    for (int64_t k = 0; k < n_psd; ++k)
        if (!certified[k]) return -std::numeric_limits<double>::infinity();
    double bound = bound_down(d - bound_up(bound_gamma((double)(Q + 2)) * D));
    for (int64_t k = 0; k < n_psd; ++k) {
        const double l = std::min(0.0, lower[k]);
        if (l < 0.0) bound = bound_down(bound + bound_down(T[k] * l));
    }
    return bound;
}

// T of one cone from the rows: every diagonal variable must be the only entry of some equality row a X_ii = b with a != 0
// and b / a >= 0; its cap is the smallest nextafter(b / a, +inf) over such rows, T the sum of the caps, each partial sum
// rounded up.  diagcol(i): the matrix column of X_ii; rowcnt[r]: stored entries of row r; rows >= p are inequalities.
template <class Ptr, class Row, class DiagCol>
double bound_trace_cap(int64_t s, DiagCol&& diagcol, const Ptr* colptr, const Row* rowidx, int64_t base, const double* val,
                       const std::vector<int32_t>& rowcnt, const double* b, int64_t p, int64_t cone) {
    double T = 0.0;
    for (int64_t i = 0; i < s; ++i) {
        const int64_t k = diagcol(i);
        double cap = std::numeric_limits<double>::infinity();
        for (int64_t q = (int64_t)colptr[k] - base; q < (int64_t)colptr[k + 1] - base; ++q) {
            const int64_t r = (int64_t)rowidx[q] - base;
            if (r >= p || rowcnt[(size_t)r] != 1 || val[q] == 0.0) continue;
            const double t = b[r] / val[q];
            if (t >= 0.0 && std::isfinite(t)) cap = std::min(cap, bound_up(t));
        }
        if (!std::isfinite(cap))
            throw std::invalid_argument("proxsdp_dual_bound: trace_cap is NULL and diagonal " + std::to_string(i) + " of cone " +
                                        std::to_string(cone) + " is not fixed by an equality row a X_ii = b with b / a >= 0");
        T = bound_up(T + cap);
    }
    return T;
}

// what is decided on the host about the struct alone (p, m, n_psd: the model's); host duals and caps are checked here
inline void check_bound_struct(const proxsdp_dual_bound* q, int64_t p, int64_t m, int64_t n_psd, bool handle) {
    if (!q) throw std::invalid_argument("NULL proxsdp_dual_bound");
    check_struct_size(q, "proxsdp_dual_bound");
    if (q->on_device != 0 && q->on_device != 1) throw std::invalid_argument("proxsdp_dual_bound.on_device must be 0 or 1");
    if (!handle && q->on_device != 0) throw std::invalid_argument("proxsdp_host_dual_bound: on_device must be 0");
    if ((p > 0 && !q->dual_eq) || (m > 0 && !q->dual_in)) throw std::invalid_argument("proxsdp_dual_bound: dual_eq or dual_in is NULL");
    if (!q->shift || !q->lambda_lower || !q->radius || !q->factorisations || !q->certified)
        throw std::invalid_argument("proxsdp_dual_bound: a NULL output array");
    if (q->on_device == 0) {
        for (int64_t r = 0; r < p; ++r)
            if (!std::isfinite(q->dual_eq[r])) throw std::invalid_argument("proxsdp_dual_bound: non-finite entry in dual_eq");
        for (int64_t r = 0; r < m; ++r)
            if (!std::isfinite(q->dual_in[r])) throw std::invalid_argument("proxsdp_dual_bound: non-finite entry in dual_in");
    }
    for (int64_t k = 0; q->trace_cap && k < n_psd; ++k)
        if (!std::isfinite(q->trace_cap[k]) || q->trace_cap[k] < 0.0)
            throw std::invalid_argument("proxsdp_dual_bound: trace_cap of cone " + std::to_string(k) + " is negative or not finite");
}

// the cone lists of a model the call serves: every variable in exactly one PSD cone, each list a whole triangle; returns the sides
inline std::vector<int64_t> bound_cone_sides(int64_t n, int64_t n_psd, const int64_t* psd_ptr, const int64_t* psd_idx, int base) {
    if (n < 1 || n_psd < 1 || !psd_ptr || !psd_idx) throw std::invalid_argument("proxsdp_host_dual_bound: no PSD cone");
    std::vector<int64_t> sides;
    std::vector<uint8_t> seen((size_t)n, 0);
    int64_t covered = 0;
    for (int64_t k = 0; k < n_psd; ++k) {
        const int64_t N = psd_ptr[k + 1] - psd_ptr[k];
        int64_t s = (int64_t)std::floor((std::sqrt(8.0 * (double)N + 1.0) - 1.0) / 2.0);
        while (s * (s + 1) / 2 < N) ++s;
        if (N < 1 || s * (s + 1) / 2 != N || s > BOUND_MAX_SIDE)
            throw std::invalid_argument("proxsdp_host_dual_bound: cone " + std::to_string(k) + " is not a triangle of side 1 .. 46340");
        for (int64_t e = psd_ptr[k]; e < psd_ptr[k + 1]; ++e) {
            const int64_t v = psd_idx[e] - base;
            if (v < 0 || v >= n || seen[(size_t)v]) throw std::invalid_argument("proxsdp_host_dual_bound: a cone variable is out of range or listed twice");
            seen[(size_t)v] = 1;
        }
        covered += N;
        sides.push_back(s);
    }
    if (covered != n) throw std::domain_error("proxsdp_host_dual_bound serves models whose variables all lie in PSD cones: some variable is outside every cone");
    return sides;
}

// proxsdp_host_dual_bound: c (n), M = [A; G] ((p + m) x n, CSC, the caller's variable order), bh = [b; h], the cone lists
// (host code is compiled with -ffp-contract=off)
inline void host_dual_bound(int64_t n, int64_t p, int64_t m, const double* c, const proxsdp_csc& M, const double* bh,
                            int64_t n_psd, const int64_t* psd_ptr, const int64_t* psd_idx, int base, proxsdp_dual_bound& q) {
    const double t0 = bound_clock();
    const int64_t Q = p + m;
    const std::vector<int64_t> sides = bound_cone_sides(n, n_psd, psd_ptr, psd_idx, base);
    std::vector<double> y((size_t)std::max<int64_t>(Q, 1), 0.0);
    for (int64_t r = 0; r < p; ++r) y[(size_t)r] = q.dual_eq[r];
    for (int64_t r = 0; r < m; ++r) y[(size_t)(p + r)] = q.dual_in[r] > 0.0 ? q.dual_in[r] : 0.0;
    double d = 0.0, D = 0.0;
    for (int64_t r = 0; r < Q; ++r) { const double t = bh[r] * y[(size_t)r]; d -= t; D += std::fabs(t); }
    std::vector<int32_t> rowcnt((size_t)std::max<int64_t>(Q, 1), 0);
    const int64_t nnz = M.colptr[n] - base;
    for (int64_t e = 0; e < nnz; ++e) rowcnt[(size_t)(M.rowval[e] - base)]++;
    std::vector<double> T((size_t)n_psd);
    double factor_seconds = 0.0;
    for (int64_t k = 0; k < n_psd; ++k) {
        const int64_t s = sides[(size_t)k];
        const int64_t* idx = psd_idx + psd_ptr[k];
        T[(size_t)k] = q.trace_cap ? q.trace_cap[k]
                                   : bound_trace_cap(s, [&](int64_t i) { return idx[i * (i + 3) / 2] - base; }, M.colptr, M.rowval, base,
                                                     M.nzval, rowcnt, bh, p, k);
        // the dual matrix and its radius, entry by entry as k_bound_dual_cone forms them
        std::vector<double> Z((size_t)(s * s)), R((size_t)(s * s));
        for (int64_t jj = 0; jj < s; ++jj)
            for (int64_t ii = 0; ii <= jj; ++ii) {
                const int64_t col = idx[jj * (jj + 1) / 2 + ii] - base;
                double acc = 0.0, aab = 0.0;
                const int64_t q0 = M.colptr[col] - base, q1 = M.colptr[col + 1] - base;
                for (int64_t e = q0; e < q1; ++e) {
                    const double yr = y[(size_t)(M.rowval[e] - base)];
                    acc += M.nzval[e] * yr;
                    aab += std::fabs(M.nzval[e]) * std::fabs(yr);
                }
                double v = c[col] + acc;
                const double ju = (double)(q1 - q0 + 2) * BOUND_U;
                double rad = (ju / (1.0 - ju)) * (std::fabs(c[col]) + aab);
                if (ii != jj) { v = v / 2.0; rad = rad / 2.0; }
                Z[(size_t)(ii * s + jj)] = Z[(size_t)(jj * s + ii)] = v;
                R[(size_t)(ii * s + jj)] = R[(size_t)(jj * s + ii)] = rad;
            }
        double nu = 0.0, rho = 0.0;
        bool finite = true;
        for (int64_t i = 0; i < s; ++i) {
            double a = 0.0, r = 0.0;
            for (int64_t j = 0; j < s; ++j) { a = bound_up(a + std::fabs(Z[(size_t)(i * s + j)])); r = bound_up(r + R[(size_t)(i * s + j)]); }
            finite = finite && std::isfinite(a) && std::isfinite(r);
            nu = std::max(nu, a); rho = std::max(rho, r);
        }
        q.radius[k] = finite ? rho : std::numeric_limits<double>::infinity();
        if (!finite) {                                               // an overflow in c + M'y: nothing can be certified
            q.shift[k] = std::numeric_limits<double>::infinity(); q.lambda_lower[k] = -std::numeric_limits<double>::infinity();
            q.factorisations[k] = 0; q.certified[k] = 0;
            if (q.delta) q.delta[k] = 0.0;
        } else if (s == 1) {
            q.shift[k] = 0.0; q.factorisations[k] = 0; q.certified[k] = 1;
            q.lambda_lower[k] = bound_down(Z[0] - R[0]);
            if (q.delta) q.delta[k] = 0.0;
        } else {
            std::vector<double> zdiag((size_t)s), W((size_t)(s * s));
            for (int64_t i = 0; i < s; ++i) zdiag[(size_t)i] = Z[(size_t)(i * s + i)];
            double delta = 0.0;
            bound_certify_cone(s, zdiag.data(), nu, rho, [&](double sigma) {
                const double tf = bound_clock();
                W = Z;
                for (int64_t i = 0; i < s; ++i) W[(size_t)(i * s + i)] = zdiag[(size_t)i] + sigma;
                const bool ok = host_cholesky(W.data(), s, bound_pivot_floor(nu)) < 0;
                factor_seconds += bound_clock() - tf;
                return ok;
            }, q.shift[k], q.lambda_lower[k], delta, q.factorisations[k], q.certified[k]);
            if (q.delta) q.delta[k] = delta;
        }
        if (q.trace_used) q.trace_used[k] = T[(size_t)k];
    }
    q.dual_objective = d;
    q.bound = bound_combine(d, D, Q, n_psd, T.data(), q.lambda_lower, q.certified);
    q.bytes_allocated = 0;
    q.factor_seconds = factor_seconds;
    q.seconds = bound_clock() - t0;
}

}  // namespace proxsdp
