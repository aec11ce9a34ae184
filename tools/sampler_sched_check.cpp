// Host check of the sampler's batch schedule (sac-expert_amd/csrc/sampler_sched.h): no GPU, no HIP.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I sac-expert_amd/csrc \
//       tools/sampler_sched_check.cpp -o sampler_sched_check && ./sampler_sched_check
// For every call length G in 1..600 on rings of 8, 16, 32, 64 and 128 slots, the grown schedule
// (largest batch 64, capped by the ring) and the fixed ones (batches of 2, 4, 8):
//   * the batches tile [0, G) in order;
//   * no batch exceeds half the ring;
//   * a batch's slots are consecutive: s % ring + (e - s) <= ring;
//   * a batch is drawn only behind the last reader of every slot it overwrites (slot u % ring
//     holds update u - ring, read last by the actor.head of update u - ring + 1), and before the
//     chain reaches its first update;
//   * G = 256 on 128 slots is at most 9 batches (1, 4, 16, 43, 64, 64, 64).
// Exit status 0 and one summary line when all hold; the first violation otherwise.
#include "sampler_sched.h"

#include <cstdio>
#include <cstdlib>
#include <string>

using Batches = std::vector<std::pair<int, int>>;

static int check(const Batches& b, int G, int ring, const char* what) {
    auto bad = [&](const char* why, size_t i) {
        std::fprintf(stderr, "%s: G=%d ring=%d batch %zu [%d, %d): %s\n", what, G, ring, i,
                     i < b.size() ? b[i].first : -1, i < b.size() ? b[i].second : -1, why);
        return 1;
    };
    if (b.empty() || b.front().first != 0 || b.back().second != G) return bad("does not cover [0, G)", 0);
    std::vector<int> holds(ring, -1);          // the update whose inputs each slot holds
    for (size_t i = 0; i < b.size(); ++i) {
        const int s = b[i].first, e = b[i].second, n = e - s;
        if (n < 1) return bad("empty", i);
        if (i > 0 && b[i - 1].second != s) return bad("not in order / gap", i);
        if (2 * n > ring) return bad("more than half the ring", i);
        if (s % ring + n > ring) return bad("slots not consecutive", i);
        const int after = sacx::sampler_emit_after(b[i], ring);   // drawn behind this update's actor.head
        if (s > 0 && after >= s) return bad("drawn no earlier than its first update", i);
        if (i > 0 && after < sacx::sampler_emit_after(b[i - 1], ring)) return bad("emitted out of order", i);
        for (int u = s; u < e; ++u) {
            const int old = holds[u % ring];
            if (old != (u >= ring ? u - ring : -1)) return bad("slot holds another update than the ring's", i);
            // update old's inputs are read last by the actor.head of update old + 1
            if (old >= 0 && old + 1 > after) return bad("overwrites a slot before its last reader", i);
            holds[u % ring] = u;
        }
    }
    return 0;
}

int main() {
    long cases = 0;
    for (int ring : {8, 16, 32, 64, 128}) {
        const int gmax = sacx::sampler_grow_max(ring, 64);
        if (gmax < 1 || 2 * gmax > ring || ring % gmax) {
            std::fprintf(stderr, "sampler_grow_max(%d, 64) = %d\n", ring, gmax);
            return 1;
        }
        for (int G = 1; G <= 600; ++G) {
            if (check(sacx::sampler_batches_grown(G, gmax), G, ring, "grown")) return 1;
            ++cases;
            for (int nbatch : {2, 4, 8}) {
                if (2 * nbatch > ring) continue;
                if (check(sacx::sampler_batches_fixed(G, nbatch), G, ring, "fixed")) return 1;
                ++cases;
            }
        }
    }
    const Batches b256 = sacx::sampler_batches_grown(256, sacx::sampler_grow_max(128, 64));
    std::string sizes;
    for (const auto& p : b256) sizes += (sizes.empty() ? "" : ", ") + std::to_string(p.second - p.first);
    if (b256.size() > 9) {
        std::fprintf(stderr, "G=256 on 128 slots: %zu batches (%s)\n", b256.size(), sizes.c_str());
        return 1;
    }
    // today's fixed schedule is unchanged: 1, 2, 4, 1, then 8s (35 batches per 256 updates)
    const Batches f256 = sacx::sampler_batches_fixed(256, 8);
    if (f256.size() != 35 || f256[1].second != 3 || f256[2].second != 7 || f256[3].second != 8) {
        std::fprintf(stderr, "fixed schedule of 8 changed: %zu batches\n", f256.size());
        return 1;
    }
    std::printf("sampler_sched ok: %ld schedules; G=256 on 128 slots: %zu batches (%s)\n", cases, b256.size(),
                sizes.c_str());
    return 0;
}
