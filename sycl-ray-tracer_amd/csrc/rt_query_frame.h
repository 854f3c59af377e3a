// rt_query_frame.h — the device half the persistent query kernels share.
// The CLAIM, one text for all of them (k_query<ANY>, k_closest, and k_path_query / k_path_gather through rt_path_rounds.h): how a wave
// draws entries from the scene's shard cursors (rt_internal.h: kQueryHeads, kQueryHeadStride, kQueryChunk) and hands them to its idle
// lanes. The only atomic on a cursor is here. 32 bits throughout — every query struct's n is a uint32_t — and an entry index widens to
// size_t only where it indexes memory.
// The FRAME k_query<ANY> (rt_query.hip) and k_closest (rt_closest.hip) share, query_frame<P>: persistent waves around a traversal
// phase. Each unit keeps its launch struct, a policy struct P and a one-line __global__ wrapper; what differs between the kinds is in P:
//   P::start(q, i, T, stack)          entry i into the calling lane: its loads, then its traversal started (true) or, where the entry is
//                                     refused, its marks written (false: never traversed; the lane takes the next entry)
//   P::phase(T)                       what the steps of one traversal phase share, taken once every lane of the phase has been started
//   P::step(S, T, x, stack, top, ph)  one wave-uniform step of the phase
//   P::store(q, i, T, x)              the results of a finished lane
//   P::Lane                           what a lane keeps beside its Trav (x above)
//   P::kBlock, P::kRefill             threads per workgroup; idle lanes of a wave that end its traversal phase
// (path_rounds keeps a frame of its own: its refill is conditional and sits around shading rounds.) The claim's state, and query_frame's
// scene and launch struct, go BY VALUE (rt_path_rounds.h: k_path_query's spills); the policy's functions and the lambdas take references.
#pragma once
#include "rt_internal.h"
#include "rt_device.h"

namespace rt {

// wave-uniform: the shard drawn on, shards found exhausted, the claimed entries not yet handed out [cb, ce)
struct Claim { uint32_t head, heads_done, cb, ce; };
// what a claim draws on, from the launch struct: the shard cursors and the number of entries
struct ClaimList { unsigned long long* cursor; uint32_t n; };

RT_DEV Claim claim_begin() { return Claim{blockIdx.x % kQueryHeads, 0u, 0u, 0u}; }
RT_DEV bool claim_open(Claim c) { return c.heads_done < kQueryHeads || c.cb != c.ce; }       // a refill can still yield an entry
RT_DEV bool claim_exhausted(Claim c) { return c.cb == c.ce && c.heads_done == kQueryHeads; } // every shard exhausted, every claimed entry handed out

// The claim: while nothing is left to hand out, the next chunk of this shard, or the move to the next shard. Shard h of n entries is
// [n * h / kQueryHeads, n * (h + 1) / kQueryHeads). Afterwards cb == ce only when every shard is exhausted.
RT_DEV Claim claim_chunk(Claim c, ClaimList q) {
    while (c.cb == c.ce && c.heads_done < kQueryHeads) {
        const uint32_t lo = (uint32_t)((unsigned long long)q.n * c.head / kQueryHeads);
        const uint32_t len = (uint32_t)((unsigned long long)q.n * (c.head + 1u) / kQueryHeads) - lo;
        unsigned long long o = 0;
        if ((threadIdx.x & 63u) == 0u) o = atomicAdd(q.cursor + c.head * kQueryHeadStride, (unsigned long long)kQueryChunk);
        const uint32_t at = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(o < len ? o : len)); // (o < 2^32: n is 32 bits, every wave overshoots a shard once)
        if (at < len) {
            c.cb = lo + at, c.ce = lo + (len - at > kQueryChunk ? at + kQueryChunk : len);
        } else {
            c.head = c.head + 1u == kQueryHeads ? 0u : c.head + 1u, c.heads_done++;
        }
    }
    return c;
}

// REFILL every idle lane, or until every shard is exhausted. is_idle() is the lane's state, read again after every hand-out; start(i)
// gives entry i to the calling lane, which starts it (and is idle no more) or marks it rejected, stays idle and takes the next one.
template <class Idle, class Start>
RT_DEV Claim claim_refill(Claim c, ClaimList q, Idle is_idle, Start start) {
    for (;;) {
        const bool mine = is_idle();
        const lmask idle = __ballot(mine);
        const uint32_t cnt = (uint32_t)__popcll(idle);
        if (cnt == 0u) break;
        c = claim_chunk(c, q);
        if (c.cb == c.ce) break; // every shard exhausted
        // the hand-out: the first min(ce - cb, cnt) claimed entries go to the idle lanes in lane order
        const uint32_t take = c.ce - c.cb < cnt ? c.ce - c.cb : cnt;
        const uint32_t rank = lane_rank(idle);
        if (mine && rank < take) start(c.cb + rank); // (an index < n: [cb, ce) lies inside its shard)
        c.cb += take;
    }
    return c;
}

// A wave claims kQueryChunk entries at a time and hands them to its idle lanes, takes wave-uniform traversal steps until P::kRefill of its
// lanes are idle, writes their results and refills them: a lane whose entry was short takes the next one instead of waiting for the wave's
// longest (rt_intersect_batch's kernel runs each wave until its slowest lane is done). Once every shard is exhausted the wave traverses
// until all its lanes are done and ends. No wave waits for another: the barrier of RT_TRAVERSAL_LDS (the staged top of the tree) comes
// before the loop, and every loop ends when the shards are exhausted.
template <class P, class Q>
RT_DEV void query_frame(SceneDev S, Q q) {
    RT_TRAVERSAL_LDS(P::kBlock)
    Trav T;
    T.cur = kTravDone;
    typename P::Lane x{};
    uint32_t ent = 0; // the lane's entry while `busy`
    bool busy = false;
    Claim claim = claim_begin();
    for (;;) {
        claim = claim_refill(claim, ClaimList{q.cursor, q.n}, [&] { return !busy; }, [&](uint32_t i) {
            if (P::start(q, i, T, stack)) ent = i, busy = true;
        });
        if (__ballot(busy) == 0ull) break; // (a lane is idle after the refill only when every shard is exhausted)
        const auto ph = P::phase(T);
        const uint32_t stop = claim_exhausted(claim) ? 64u : P::kRefill;
        while (count(trav_done(T)) < stop) P::step(S, T, x, stack, top, ph);
        if (busy && T.cur == kTravDone) P::store(q, ent, T, x), busy = false;
    }
}

} // namespace rt
