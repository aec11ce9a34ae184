// The sampler's batch schedule: which updates each k_rng + k_gather launch of a G-update call
// draws, and behind which update of the chain it may start.  Plain C++ (no HIP), so the host can
// test it alone (tools/sampler_sched_check.cpp).
//
// A batch [s, e) fills the slots s % nslot .. s % nslot + (e - s) - 1 of the ring: consecutive
// slots (the kernels address slot + u), so it never runs past the ring's end.  Slot u % nslot is
// last read through update u's folded alpha rows in update u + 1's actor.head, so the batch is
// drawn behind the actor.head of update e - nslot (sampler_emit_after; <= 0: its slots are fresh at
// the call's start) and must be done before update s.  A batch of at most half the ring leaves
// the sampler at least half a ring of lead over the chain.
#pragma once
#include <algorithm>
#include <utility>
#include <vector>

namespace sacx {

// Fixed batches: sizes ramp 1, 2, 4, ... up to nbatch, never crossing a multiple of nbatch (nslot
// is one), so the first update of the call waits for one update's draws only.
inline std::vector<std::pair<int, int>> sampler_batches_fixed(int G, int nbatch) {
    std::vector<std::pair<int, int>> batches;
    for (int s0 = 0, ramp = 1; s0 < G; ramp = std::min(nbatch, 2 * ramp)) {
        const int sz = std::min({ramp, nbatch - s0 % nbatch, G - s0});
        batches.push_back({s0, s0 + sz});
        s0 += sz;
    }
    return batches;
}

// The largest batch of the grown schedule on a ring of nslot slots: at most cap and half the ring,
// and a divisor of the ring (whole batches tile it)
inline int sampler_grow_max(int nslot, int cap) {
    int g = std::max(1, std::min(cap, nslot / 2));
    while (g > 1 && nslot % g) --g;
    return g;
}

// Grown batches: sizes 1, 4, 16, 64, ... up to gmax (= sampler_grow_max), each four times the last
// (a batch of 4 k updates is drawn while the chain runs the k before it and its own first ones: the
// draw takes a fifth of an update's time), never crossing a multiple of gmax.  Every batch start is
// a cross-queue edge of the chain, so a long call has a fifth of the fixed schedule's: G = 256 on
// 128 slots is 1, 4, 16, 43, 64, 64, 64.
inline std::vector<std::pair<int, int>> sampler_batches_grown(int G, int gmax) {
    std::vector<std::pair<int, int>> batches;
    for (int s0 = 0, cls = 1; s0 < G; cls = std::min(gmax, 4 * cls)) {
        const int sz = std::min({cls, gmax - s0 % gmax, G - s0});
        batches.push_back({s0, s0 + sz});
        s0 += sz;
    }
    return batches;
}

// the update whose actor.head is the last reader of batch [s, e)'s slots (<= 0: none in this call)
inline int sampler_emit_after(const std::pair<int, int>& batch, int nslot) { return batch.second - nslot; }

// Calls of at least this many updates take the grown schedule (shorter ones keep the fixed one:
// their few batches are all drawn at the call's start)
constexpr int kSamplerGrowMinG = 128;

}  // namespace sacx
