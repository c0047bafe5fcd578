// chord_bcast.hip -- Chord overlay broadcast on a converged ring, for gfx950 (MI355X).
//
// Chord::forwardBroadcast (Chord.cc:1410-1445) driven as BroadcastTestApp::rpcBroadcastRequest does
// (BroadcastTestApp.cc:216-340), for a batch of broadcasts at once.  On a converged ring the ranges a
// node hands to its children partition its own range, so every node receives one request and the
// tree can be expanded level by level: level k holds the nodes reached after k hops.  The host
// loops over the levels (ovs_chord_broadcast_batch); each level is one launch over that level's
// items, which appends the next level's items behind them in one queue.  No wave waits for another:
// every loop below is bounded by a row length (<= 161 steps) or the item count.
//
// At node v with limit L (the initiator: its own key, which makes (v, L) the whole ring,
// OverlayKey.cc:587-599) the candidates are getFinger(159) .. getFinger(0), then successor 0.  A
// candidate f is a child iff f.key lies in (v.key, L), i.e. 0 < f - v < L - v, and then L := f.key.
// Finger i lies at least 2^i past v, so the scan starts at i = msb(L - v); positions below
// i_lo(v) = msb(succ0 - v) + 1 all resolve to successor 0 (ChordFingerTable.cc:183-184), which the
// final successor step covers.  The row entry of a finger carries its key and coordinates, so the
// interval test and the coordinate delay need no second gather; the test is done on the exact
// 160-bit distances (the key is in the line already, a 64-bit summary would save nothing).
//
// Delay of the j-th request v sends at time t: v's transmit queue is idle when the request arrives (a
// node receives once and sends only then), so it is fanout_arrival (tier_dev.hpp) at rank j.
#include "chord_bcast.hpp"
#include "tier_dev.hpp"

namespace ovs {

namespace {

// the first 40 B of a NodeRec or a FingerEnt: key, row offset (NodeRec) / node index (FingerEnt), x, y
struct Head {
    K160 k;
    uint32_t aux;
    double x, y;
};

__device__ __forceinline__ Head load_head(const void* p)
{
    const uint4 b = reinterpret_cast<const uint4*>(p)[1];
    const uint2 c = reinterpret_cast<const uint2*>(p)[4];
    Head h;
    h.k = load_key(p);
    h.aux = b.y;
    h.x = dbl(b.z, b.w);
    h.y = dbl(c.x, c.y);
    return h;
}

__device__ __forceinline__ BcastItem load_item(const BcastItem* q)
{
    const uint2* p = reinterpret_cast<const uint2*>(q);
    const uint2 a = p[0], b = p[1], c = p[2];
    BcastItem it;
    it.b = a.x; it.node = a.y; it.limit = b.x;
    it.hops = (uint16_t)(b.y & 0xFFFFu); it.rank = (uint16_t)(b.y >> 16);
    it.t = (int64_t)((uint64_t)c.x | ((uint64_t)c.y << 32));
    return it;
}

// the child's queue item and its record (one 16 B store); slot >= cap is dropped and reported
__device__ __forceinline__ void emit(BcastItem* __restrict__ queue, uint64_t slot, uint64_t cap,
                                     ovs_bcast_node* __restrict__ nodes, uint32_t n, unsigned long long* ctl, uint32_t b,
                                     uint32_t child, uint32_t limit, uint32_t parent, uint32_t hops, uint32_t rank, int64_t t)
{
    if (slot >= cap) {
        atomicOr(&ctl[1], BCAST_ERR_OVERFLOW);
        return;
    }
    const uint32_t hr = hops | (rank << 16);
    uint2* p = reinterpret_cast<uint2*>(queue + slot);
    p[0] = make_uint2(b, child);
    p[1] = make_uint2(limit, hr);
    p[2] = make_uint2((uint32_t)(uint64_t)t, (uint32_t)((uint64_t)t >> 32));
    if (nodes)
        *reinterpret_cast<uint4*>(nodes + (uint64_t)b * n + child) =
            make_uint4((uint32_t)(uint64_t)t, (uint32_t)((uint64_t)t >> 32), parent, hr);
}

// what forwardBroadcast needs of the item's node: its record, successor 0, the limit distance and
// the part of its finger row that can lie below the limit (steps 0 .. m-1; step m is successor 0)
struct Sender {
    Head v, s0;
    uint32_t s0i;
    K160 dL;        // (limit - v) mod 2^160; 0 = the whole ring (the initiator)
    bool whole;
    int m;
    uint32_t row;   // index of the step-0 entry
};

__device__ __forceinline__ Sender load_sender(const ChordView& V, const BcastItem& it)
{
    Sender S;
    S.v = load_head(V.nodes + it.node);
    S.s0i = it.node + 1 == V.n ? 0u : it.node + 1;
    S.s0 = load_head(V.nodes + S.s0i);
    S.dL = k_sub(load_key(V.nodes + it.limit), S.v.k);
    S.whole = k_zero(S.dL);
    const int ilo = k_msb(k_sub(S.s0.k, S.v.k)) + 1;
    const int itop = S.whole ? KEYBITS - 1 : k_msb(S.dL);
    S.m = itop >= ilo ? itop - ilo + 1 : 0;
    S.row = S.v.aux + (uint32_t)(KEYBITS - 1 - itop);
    return S;
}

__device__ __forceinline__ int64_t arrival(const BcastConsts& BC, int64_t t, int rank, const Head& a, const Head& b)
{
    return fanout_arrival(t, (uint32_t)rank, BC.bw, BC.access2, a.x, a.y, b.x, b.y, BC.round);
}

// Late levels: many nodes with 0-2 children each.  One lane per item walks its row twice: first
// it only decides which steps are children (a bit per step), then the block reserves the queue
// slots of all its children with ONE atomic (a reservation per wave and step measured 195 ms at
// n = 2^20, nb = 64: 21M returning atomics on one address), and the second walk re-reads the
// accepted entries alone and writes the children.
__global__ __launch_bounds__(256) void k_bcast_lanes(ChordView V, BcastConsts BC, BcastItem* __restrict__ queue,
                                                     uint64_t lo, uint64_t hi, uint64_t cap,
                                                     ovs_bcast_node* __restrict__ nodes, unsigned long long* ctl)
{
    __shared__ unsigned int wsum[4];
    __shared__ unsigned long long bbase;
    const uint64_t i = lo + (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    BcastItem it{};
    Sender S{};
    bool valid = i < hi;
    if (valid) {
        it = load_item(queue + i);
        valid = it.node < V.n;
    }
    uint64_t acc0 = 0, acc1 = 0, acc2 = 0;          // step k is a child: bit k
    unsigned int cnt = 0;
    if (valid) {
        S = load_sender(V, it);
        K160 cur = S.dL;
        bool whole = S.whole;
        for (int k = 0; k <= S.m; ++k) {            // S.m <= 160
            const K160 ck = k < S.m ? load_head(V.frow + S.row + (uint32_t)k).k : S.s0.k;
            const K160 d = k_sub(ck, S.v.k);
            if (!k_zero(d) && (whole || k_lt(d, cur))) {
                const uint64_t bit = 1ull << (k & 63);
                if (k < 64) acc0 |= bit; else if (k < 128) acc1 |= bit; else acc2 |= bit;
                cur = d; whole = false; ++cnt;
            }
        }
    }
    // exclusive prefix of cnt over the block: wave scan, then the four wave totals
    unsigned int inc = cnt;
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned int o = __shfl_up(inc, off);
        if (lane >= off) inc += o;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned int tot = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        bbase = tot ? atomicAdd(&ctl[0], (unsigned long long)tot) : 0ull;
    }
    __syncthreads();
    unsigned long long slot = bbase + (inc - cnt);
    for (int w = 0; w < wave; ++w) slot += wsum[w];
    if (!cnt) return;
    uint32_t lim = it.limit;
    int j = 0;
    for (int part = 0; part < 3; ++part) {
        uint64_t a = part == 0 ? acc0 : part == 1 ? acc1 : acc2;
        while (a) {
            const int k = part * 64 + __ffsll((long long)a) - 1;
            a &= a - 1;
            Head c;
            uint32_t ci;
            if (k < S.m) { c = load_head(V.frow + S.row + (uint32_t)k); ci = c.aux; }
            else { c = S.s0; ci = S.s0i; }
            emit(queue, slot + (unsigned long long)j, cap, nodes, V.n, ctl, it.b, ci, lim, it.node, (uint32_t)it.hops + 1u,
                 (uint32_t)j, arrival(BC, it.t, j, S.v, c));
            lim = ci; ++j;
        }
    }
}

// Early levels: few nodes with many children each.  One wave per item, one lane per row step.
// Down the row the fingers' distances never grow (a finger that wraps to the node itself counts as
// the farthest), so a step is a child iff it is inside the limit and its finger differs from the
// step before -- the same set as the sequential update of the limit gives.
__global__ __launch_bounds__(256) void k_bcast_waves(ChordView V, BcastConsts BC, BcastItem* __restrict__ queue,
                                                     uint64_t lo, uint64_t hi, uint64_t cap,
                                                     ovs_bcast_node* __restrict__ nodes, unsigned long long* ctl)
{
    const uint64_t i = lo + (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const uint64_t lt = (1ull << lane) - 1ull;   // spelled as wave_reserve spells it: the compiler keeps one copy
    if (i >= hi) return;                       // the whole wave
    const BcastItem it = load_item(queue + i);
    if (it.node >= V.n) return;
    const Sender S = load_sender(V, it);
    uint32_t carry = it.limit;
    int jbase = 0;
    for (int k0 = 0; k0 <= S.m; k0 += 64) {
        const int k = k0 + lane;
        const bool act = k <= S.m;
        Head c{};
        uint32_t ci = 0, prev = NONE;
        bool ok = false;
        if (act) {
            if (k < S.m) { c = load_head(V.frow + S.row + (uint32_t)k); ci = c.aux; }
            else { c = S.s0; ci = S.s0i; }
            if (k > 0) prev = V.frow[S.row + (uint32_t)(k - 1)].idx;
            const K160 d = k_sub(c.k, S.v.k);
            ok = !k_zero(d) && (S.whole || k_lt(d, S.dL)) && ci != prev;
        }
        const uint64_t mask = __ballot(ok);
        if (!mask) continue;
        const uint64_t below = mask & lt;
        const uint32_t above = __shfl(ci, below ? 63 - __clzll((long long)below) : 0);
        const unsigned long long slot = wave_append(ok, ctl, cap, BCAST_ERR_OVERFLOW);   // one reservation per wave and step
        if (slot != NO_SLOT) {
            const int rank = jbase + __popcll(below);
            emit(queue, slot, cap, nodes, V.n, ctl, it.b, ci, below ? above : carry, it.node, (uint32_t)it.hops + 1u,
                 (uint32_t)rank, arrival(BC, it.t, rank, S.v, c));
        }
        carry = __shfl(ci, 63 - __clzll((long long)mask));
        jbase += __popcll(mask);
    }
}

__global__ void k_bcast_fill(uint4* __restrict__ nodes, uint64_t total)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) nodes[i] = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, NONE, 0u);
}

__global__ void k_bcast_init(const uint32_t* __restrict__ initiators, uint64_t nb, uint32_t n,
                             BcastItem* __restrict__ queue, uint64_t cap, ovs_bcast_node* __restrict__ nodes,
                             unsigned long long* ctl)
{
    const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b == 0) atomicAdd(&ctl[0], (unsigned long long)nb);
    if (b >= nb || b >= cap) return;
    const uint32_t v = initiators[b];
    uint2* p = reinterpret_cast<uint2*>(queue + b);
    if (v >= n) {
        // outside the network: an item no level expands and the statistics skip
        atomicOr(&ctl[1], BCAST_ERR_INITIATOR);
        p[0] = make_uint2((uint32_t)b, NONE);
        p[1] = make_uint2(NONE, 0u);
        p[2] = make_uint2(0u, 0u);
        return;
    }
    p[0] = make_uint2((uint32_t)b, v);
    p[1] = make_uint2(v, 0u);
    p[2] = make_uint2(0u, 0u);
    if (nodes) *reinterpret_cast<uint4*>(nodes + b * n + v) = make_uint4(0u, 0u, NONE, 0u);
}

// per (broadcast, hop count): how many nodes; per broadcast: the latest arrival.  A wave adds one
// count per distinct (broadcast, hops) among its 64 items -- neighbours in the queue mostly share it.
__global__ __launch_bounds__(256) void k_bcast_stats(const BcastItem* __restrict__ queue, uint64_t total,
                                                     unsigned long long* __restrict__ hist,
                                                     unsigned long long* __restrict__ last)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    BcastItem it{};
    bool valid = i < total;
    if (valid) {
        it = load_item(queue + i);
        valid = it.node != NONE;
    }
    const uint32_t h = it.hops < BCAST_MAX_HOPS ? it.hops : BCAST_MAX_HOPS;
    const unsigned long long key = ((unsigned long long)it.b << 16) | h;
    uint64_t rem = __ballot(valid);
    while (rem) {
        const int l0 = __ffsll((long long)rem) - 1;
        const unsigned long long k0 = shfl64(key, l0);
        const bool mine = valid && key == k0;
        const uint64_t m = __ballot(mine);
        const unsigned long long t = wave_max_u64(mine ? (unsigned long long)it.t : 0ull);   // the other lanes add 0
        if (lane == l0) {
            atomicAdd(&hist[(k0 >> 16) * BCAST_HIST + (k0 & 0xFFFFu)], (unsigned long long)__popcll(m));
            atomicMax(&last[k0 >> 16], t);
        }
        rem &= ~m;
    }
}

}  // namespace

hipError_t launch_bcast_fill(ovs_bcast_node* nodes, uint64_t total, hipStream_t s)
{
    const uint64_t blocks = blocks256(total);
    if (!grid_ok(blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_bcast_fill, dim3((unsigned)blocks), dim3(256), 0, s, reinterpret_cast<uint4*>(nodes), total);
    return hipGetLastError();
}

hipError_t launch_bcast_init(const uint32_t* initiators, uint64_t nb, uint32_t n, BcastItem* queue, uint64_t cap,
                             ovs_bcast_node* nodes, unsigned long long* ctl, hipStream_t s)
{
    const uint64_t blocks = blocks256(nb);
    if (!grid_ok(blocks) || nb > 0xFFFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_bcast_init, dim3((unsigned)blocks), dim3(256), 0, s, initiators, nb, n, queue, cap, nodes, ctl);
    return hipGetLastError();
}

hipError_t launch_bcast_level(const ChordView& V, const BcastConsts& BC, BcastItem* queue, uint64_t lo, uint64_t hi,
                              uint64_t cap, ovs_bcast_node* nodes, unsigned long long* ctl, bool wave_per_item,
                              hipStream_t s)
{
    if (hi <= lo) return hipSuccess;
    const uint64_t cnt = hi - lo;
    const uint64_t blocks = wave_per_item ? (cnt + 3) / 4 : blocks256(cnt);
    if (!grid_ok(blocks)) return hipErrorInvalidValue;
    if (wave_per_item)
        hipLaunchKernelGGL(k_bcast_waves, dim3((unsigned)blocks), dim3(256), 0, s, V, BC, queue, lo, hi, cap, nodes, ctl);
    else
        hipLaunchKernelGGL(k_bcast_lanes, dim3((unsigned)blocks), dim3(256), 0, s, V, BC, queue, lo, hi, cap, nodes, ctl);
    return hipGetLastError();
}

hipError_t launch_bcast_stats(const BcastItem* queue, uint64_t total, unsigned long long* hist,
                              unsigned long long* last, hipStream_t s)
{
    if (total == 0) return hipSuccess;
    const uint64_t blocks = blocks256(total);
    if (!grid_ok(blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_bcast_stats, dim3((unsigned)blocks), dim3(256), 0, s, queue, total, hist, last);
    return hipGetLastError();
}

}  // namespace ovs
