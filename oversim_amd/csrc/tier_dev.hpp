// tier_dev.hpp -- what the application-tier translation units (chord_bcast.hip, scribe.hip, dht.hip,
// kbr_rpc.hip, stats.hip) share: wave reductions, the 64-bit shuffle and mixer, key loads and compares,
// the wave-aggregated queue append, the fan-out arrival time and the launch arithmetic.  Every device
// function is forced inline; nothing here has state and there are no kernels.
#pragma once
#include "engine.hpp"

namespace ovs {

// ---- wave-wide integer reductions: every lane gets the result; called by all 64 lanes ----
template <class Op>
__device__ __forceinline__ uint64_t wave_reduce_u64(uint64_t v, Op op)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, (uint64_t)__shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v)
{
    return wave_reduce_u64(v, [](uint64_t a, uint64_t b) { return a + b; });
}
__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v)
{
    return wave_reduce_u64(v, [](uint64_t a, uint64_t b) { return b < a ? b : a; });
}
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v)
{
    return wave_reduce_u64(v, [](uint64_t a, uint64_t b) { return b > a ? b : a; });
}

__device__ __forceinline__ unsigned long long shfl64(unsigned long long v, int src)
{
    const unsigned int lo = __shfl((unsigned int)v, src), hi = __shfl((unsigned int)(v >> 32), src);
    return (unsigned long long)lo | ((unsigned long long)hi << 32);
}

__device__ __forceinline__ uint64_t mix64(uint64_t x)
{
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
    return x;
}

// ---- 160-bit keys in records ----
// five key words against a key, word by word (the words may lie in global memory: the first difference ends it)
__device__ __forceinline__ bool words_are_key(const uint32_t* w, const K160& k)
{
    return w[0] == k.w[0] && w[1] == k.w[1] && w[2] == k.w[2] && w[3] == k.w[3] && w[4] == k.w[4];
}
__device__ __forceinline__ bool rec_is_key(const KeyRec& r, const K160& k) { return words_are_key(r.w, k); }

// the key at the start of a 64 B NodeRec or FingerEnt: one 16 B load and one dword
__device__ __forceinline__ K160 load_key(const void* rec)
{
    const uint4 a = *reinterpret_cast<const uint4*>(rec);
    K160 k;
    k.w[0] = a.x; k.w[1] = a.y; k.w[2] = a.z; k.w[3] = a.w; k.w[4] = reinterpret_cast<const uint32_t*>(rec)[4];
    return k;
}

// ---- wave-aggregated appends (called by all lanes of a wave) ----
constexpr unsigned long long NO_SLOT = ~0ull;

// One atomicAdd on *counter per wave reserves a slot for every lane with `won`: the ballot's first
// lane adds the popcount, every lane gets the base, a lane's slot is the base plus the winners below it.
__device__ __forceinline__ unsigned long long wave_reserve(bool won, unsigned long long* counter)
{
    const uint64_t mask = __ballot(won);
    if (!mask) return NO_SLOT;
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((long long)mask) - 1;
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(counter, (unsigned long long)__popcll(mask));
    base = shfl64(base, leader);
    return won ? base + (unsigned long long)__popcll(mask & ((1ull << lane) - 1ull)) : NO_SLOT;
}

// The same on a queue with control words ctl[0] = length, ctl[1] = error bits: a slot past the
// capacity is not handed out and sets overflow_bit.
__device__ __forceinline__ unsigned long long wave_append(bool won, unsigned long long* ctl, uint64_t cap,
                                                          unsigned long long overflow_bit)
{
    const unsigned long long slot = wave_reserve(won, &ctl[0]);
    if (slot == NO_SLOT || slot < cap) return slot;
    atomicOr(&ctl[1], overflow_bit);
    return NO_SLOT;
}

// ---- the rank-th copy a node sends at t from an idle transmit queue (SimpleNodeEntry.cc:164-194) ----
// It has left after (rank + 1) serialisation times and the receiver adds one more:
//   arrival = t + (rank + 2) * T(bits / datarate) + 2 * T(accessDelay) + coordDelay(a, b).
__device__ __forceinline__ int64_t fanout_arrival(int64_t t, uint32_t rank, int64_t bw, int64_t access2, double ax,
                                                  double ay, double bx, double by, int round)
{
    return t + (int64_t)(rank + 2) * bw + access2 + coord_ns(ax, ay, bx, by, round);
}

// ---- launch arithmetic (host) ----
inline uint64_t blocks256(uint64_t n) { return (n + 255) / 256; }
// a block count a one-dimensional grid can take (0 blocks is no launch)
inline bool grid_ok(uint64_t blocks) { return blocks >= 1 && blocks <= 0x7FFFFFFFull; }
// a grid-stride launch: enough blocks of per_block items for n, at most per_cu blocks per CU
inline unsigned capped_grid(uint64_t n, int per_block, int num_cu, int per_cu)
{
    const uint64_t blocks = (n + per_block - 1) / per_block;
    const uint64_t cap = (uint64_t)(num_cu > 0 ? num_cu : 1) * per_cu;
    return (unsigned)(blocks > cap ? cap : blocks);
}

// What every statistics launch starts with: the per-node counter rows zeroed and the sums set to
// `init` (minima at ~0, the rest 0).
template <class Sums>
inline hipError_t stats_prelude(uint32_t* node_counts, int rows, uint32_t nnodes, Sums* S, const Sums& init,
                                hipStream_t s)
{
    const hipError_t e = hipMemsetAsync(node_counts, 0, sizeof(uint32_t) * rows * (uint64_t)nnodes, s);
    return e != hipSuccess ? e : hipMemcpyAsync(S, &init, sizeof init, hipMemcpyHostToDevice, s);
}

}  // namespace ovs
