// dk_graph_reach.h -- device code of the reachability calls on the graph mirror: which members of a layer a
// traversal that starts at the entry point can arrive at over OUT-edges, and in how many hops.  Included by device_backend.hip only:
// like dk_graph_info.h these kernels read no rows, so they have no metric and live in that unit.
//
// Members, lists and the clamped count word are LayerView's (dk_graph_info.h).  An entry u -> v counts only between two members; a
// target that is no member is never dereferenced.  A level-synchronous BFS: hop[v] is 0 for the member seeds, -1 for the other
// members, -2 for everything else; round d expands the queue of the nodes with hop d and appends the nodes it is first to reach
// (compare-exchange -1 -> d + 1 on hop[v]: one winner, so a node is queued, and expanded, exactly once) to the other queue.  Every
// kernel is an ordinary grid-stride launch; the host launches a round, reads the next queue's length and stops at 0.
//
// The loops that hold a ballot have a WAVE-UNIFORM trip count (they step over the wave's first item, every lane of the wave goes
// round the same number of times) and no `continue` ahead of the ballot: a lane past the end takes part with "nothing to append"
// (range_sort_kernel's hang).  The blocks are kGraphInfoBlock = 256 threads, whole waves.
#pragma once
#include "dk_graph_info.h"

namespace hnsw {

enum { kReachSeedId = 0, kReachSeedBits = 1, kReachSeedHops = 2 };

// What a layer's kernels add up (device memory, zeroed in front of the layer's first launch)
struct ReachAcc {
    unsigned long long members; // members of the layer
    unsigned long long seeds;   // ... that are seeds (hop 0, the first queue)
    unsigned long long reached; // ... with hop >= 0 (the pack kernel's count)
    unsigned long long entries; // list entries the expansions read: the sum of the expanded nodes' out-degrees
    int qn[2];                  // lengths of the two queues; the host reads these 8 bytes after every round
    int max_hop, pad;
};

struct ReachSeeds {
    int mode;             // kReachSeedId: the one id `id`; kReachSeedBits: `bits`; kReachSeedHops: the nodes with prev_hop[v] >= 0
    int id;
    const unsigned *bits; // nbits bits in the allow-sets' format, ids >= nbits no seeds
    long long nbits;
    const int *prev_hop;  // the hop array of the layer above (the chain): its reached set is this layer's seed set
};

#define GR_RELAXED __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// One queue append per wave: the lanes with `win` get consecutive places behind one atomic add of the leader.  Called by every
// lane of the wave (the ballot and the shuffle are the wave's); returns how many lanes appended.
__device__ __forceinline__ int reach_append(bool win, int v, int *__restrict__ q, int *q_len)
{
    const unsigned long long b = __ballot(win);
    const int lane = (int)(threadIdx.x & 63u);
    const int leader = b ? __ffsll((long long)b) - 1 : 0;
    int base = 0;
    if (b && lane == leader) base = __hip_atomic_fetch_add(q_len, __popcll(b), GR_RELAXED);
    base = __shfl(base, leader);
    if (win) q[base + __popcll(b & ((1ull << lane) - 1ull))] = v;
    return __popcll(b);
}

// ---- thread per node: hop[], the first queue, members and seeds counted -----------------------------------------------------
__global__ void __launch_bounds__(kGraphInfoBlock)
graph_reach_init_kernel(LayerView g, ReachSeeds s, int *__restrict__ hop, int *__restrict__ q, ReachAcc *__restrict__ acc)
{
    const int lane = (int)(threadIdx.x & 63u);
    const long long step = (long long)gridDim.x * kGraphInfoBlock;
    unsigned members = 0u, seeds = 0u; // wave totals, the same in every lane
    for (long long first = (long long)blockIdx.x * kGraphInfoBlock + (threadIdx.x & ~63u); first < g.n; first += step) {
        const long long v = first + lane;
        const bool in = v < g.n;
        const bool mem = in && g.member(v);
        bool seed = false;
        if (mem) {
            if (s.mode == kReachSeedId) seed = v == (long long)s.id;
            else if (s.mode == kReachSeedBits) seed = v < s.nbits && ((s.bits[v >> 5] >> (v & 31)) & 1u);
            else seed = s.prev_hop[v] >= 0;
        }
        if (in) hop[v] = seed ? 0 : mem ? -1 : -2;
        members += (unsigned)__popcll(__ballot(mem));
        seeds += (unsigned)reach_append(seed, (int)v, q, &acc->qn[0]);
    }
    if (lane == 0 && members) (void)__hip_atomic_fetch_add(&acc->members, (unsigned long long)members, GR_RELAXED);
    if (lane == 0 && seeds) (void)__hip_atomic_fetch_add(&acc->seeds, (unsigned long long)seeds, GR_RELAXED);
}

// ---- one round: work item i is slot 1 + i % (stride - 1) of the list of q_in[i / (stride - 1)] ---------------------------------
// q_in holds q_n nodes of hop d (members, each once); the winners go to q_out with hop d + 1 and acc->qn[src ^ 1] counts them.
// acc->qn[src] is not read by this launch (q_n is the argument): it is zeroed here, for the round after this one to count in.
__global__ void __launch_bounds__(kGraphInfoBlock)
graph_reach_expand_kernel(LayerView g, const int *__restrict__ q_in, int q_n, int *__restrict__ q_out, int *hop, int d, int src, ReachAcc *__restrict__ acc)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_store(&acc->qn[src], 0, GR_RELAXED);
    const int lane = (int)(threadIdx.x & 63u);
    const int per = g.stride() - 1;
    const long long total = (long long)q_n * per, step = (long long)gridDim.x * kGraphInfoBlock;
    unsigned entries = 0u; // the wave's, the same in every lane
    for (long long first = (long long)blockIdx.x * kGraphInfoBlock + (threadIdx.x & ~63u); first < total; first += step) {
        const long long i = first + lane;
        bool read = false, win = false;
        int v = -1;
        if (i < total) {
            const long long at = i / per;
            const int slot = 1 + (int)(i - at * per);
            const int u = q_in[at];
            const int *l = g.list(u);
            if (l && slot <= g.count(l)) {
                read = true;
                v = l[slot];
                if (g.member(v)) {
                    int expected = -1;
                    win = __hip_atomic_compare_exchange_strong(hop + v, &expected, d + 1, __ATOMIC_RELAXED, GR_RELAXED);
                }
            }
        }
        entries += (unsigned)__popcll(__ballot(read));
        (void)reach_append(win, v, q_out, &acc->qn[src ^ 1]);
    }
    if (lane == 0 && entries) (void)__hip_atomic_fetch_add(&acc->entries, (unsigned long long)entries, GR_RELAXED);
}

// ---- thread per node: the reached set as a bitset in the allow-sets' format, its size and the largest hop ----------------------
// A wave's ballot is two of the bitset's words (the wave's first node is a multiple of 64); bits == nullptr: only the two figures.
__global__ void __launch_bounds__(kGraphInfoBlock)
graph_reach_pack_kernel(long long n, const int *__restrict__ hop, unsigned *__restrict__ bits, ReachAcc *__restrict__ acc)
{
    const int lane = (int)(threadIdx.x & 63u);
    const long long step = (long long)gridDim.x * kGraphInfoBlock, words = (n + 31) / 32;
    unsigned reached = 0u; // the wave's, the same in every lane
    int mx = 0;
    for (long long first = (long long)blockIdx.x * kGraphInfoBlock + (threadIdx.x & ~63u); first < n; first += step) {
        const long long v = first + lane;
        const int h = v < n ? hop[v] : -2;
        const unsigned long long b = __ballot(h >= 0);
        mx = h > mx ? h : mx;
        reached += (unsigned)__popcll(b);
        const long long w = (first >> 5) + (lane >> 5);
        if (bits && (lane & 31) == 0 && w < words) bits[w] = (unsigned)(b >> (lane & 32));
    }
    if (lane == 0 && reached) (void)__hip_atomic_fetch_add(&acc->reached, (unsigned long long)reached, GR_RELAXED);
    for (int o = 32; o > 0; o >>= 1) { // (every lane is here: the loop above ends for the whole wave at once)
        const int other = __shfl_xor(mx, o);
        mx = other > mx ? other : mx;
    }
    if (lane == 0 && mx > 0) (void)__hip_atomic_fetch_max(&acc->max_hop, mx, GR_RELAXED);
}

#undef GR_RELAXED

} // namespace hnsw
