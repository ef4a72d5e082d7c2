// Stand-alone check of csrc/shard_group.hpp (host-only, no HIP): ShardGroup::reduce and reduce_vec from S = 1, 2, 3 and 8
// threads against a serial sum in rank order, bit for bit, including a shard that leaves mid-way.  Meant for the sanitizers:
//   c++ -std=c++17 -O1 -g -pthread -fsanitize=thread            -I proxsdp.jl_amd/csrc tests/c_harness/shard_group_check.cpp
//   c++ -std=c++17 -O1 -g -pthread -fsanitize=address,undefined -I proxsdp.jl_amd/csrc tests/c_harness/shard_group_check.cpp
// Exit status 0 and "ok" on success.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <thread>

#include "shard_group.hpp"

namespace {
constexpr int NS = 5, NM = 4, NV = 7;

// shard s's record of round k: order-revealing sums (1e16, 1, -1e16 dealt over the shards), -0.0 and a NaN now and then
double value(int k, int s, int q) {
    const double big[4] = {1e16, 1.0, -1e16, 3.0};
    if (q == 0) return big[(k + s) % 4];
    if (q == 1) return -0.0;
    if (q == 2 && k % 50 == 7 && s == k % 3) return std::nan("");
    if (q == NS + 1 && k % 50 == 8 && s == (k / 2) % 3) return std::nan("");       // (std::max keeps or drops it by order)
    return std::sin(1.0 + k * 0.37 + s * 1.9 + q * 0.11) * (q % 2 ? 1e-3 : 1e3);
}
bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// rounds alternate reduce / reduce_vec; shard `leaver` (-1: none) stops before round `leave_at`.  Returns the failures seen
int run(int S, int rounds, int leaver, int leave_at) {
    proxsdp::ShardGroup group(S, 20.0);
    std::vector<int> done(S, 0), failed(S, 0), wrong(S, 0);
    auto body = [&](int s) {
        try {
            for (int k = 0; k < rounds; ++k) {
                if (s == leaver && k == leave_at) break;
                if (k % 2 == 0) {
                    std::vector<double> sums(NS), maxs(NM);
                    for (int q = 0; q < NS; ++q) sums[q] = value(k, s, q);
                    for (int q = 0; q < NM; ++q) maxs[q] = value(k, s, NS + q);
                    group.reduce(s, sums, maxs);
                    for (int q = 0; q < NS + NM; ++q) {
                        double a = value(k, 0, q);
                        for (int r = 1; r < S; ++r) a = q < NS ? a + value(k, r, q) : std::max(a, value(k, r, q));
                        wrong[s] += !same_bits(a, q < NS ? sums[q] : maxs[q - NS]);
                    }
                } else {
                    std::vector<double> v(NV);
                    for (int q = 0; q < NV; ++q) v[q] = value(k, s, q);
                    group.reduce_vec(s, v);
                    for (int q = 0; q < NV; ++q) {
                        double a = value(k, 0, q);
                        for (int r = 1; r < S; ++r) a += value(k, r, q);
                        wrong[s] += !same_bits(a, v[q]);
                    }
                }
                done[s] = k + 1;
            }
        } catch (const proxsdp::PeerFailure&) { failed[s] = 1; }
        group.leave();
        group.wait_all_left();
    };
    std::vector<std::thread> th;
    for (int s = 1; s < S; ++s) th.emplace_back(body, s);
    body(0);
    for (auto& t : th) t.join();
    int bad = 0;
    for (int s = 0; s < S; ++s) {
        bad += wrong[s];
        if (leaver < 0 || S == 1) bad += failed[s] || done[s] != rounds;
        else if (s == leaver) bad += failed[s] || done[s] != leave_at;
        else bad += !failed[s] || done[s] != leave_at;          // every peer completes exactly the rounds the leaver joined
    }
    return bad;
}
}  // namespace

int main() {
    int bad = 0;
    for (int S : {1, 2, 3, 8}) {
        bad += run(S, 400, -1, 0);
        if (S > 1) bad += run(S, 400, S - 1, 201);
        std::printf("S = %d: %s\n", S, bad ? "FAILED" : "ok");
    }
    return bad ? 1 : 0;
}
