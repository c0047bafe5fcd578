// engine.hpp -- device-side data layout and shared device functions of the
// MI355X lookup-routing engine (internal; the public boundary is include/ovs_kbr.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "key160.hpp"
#include "../../include/ovs_kbr.h"

namespace ovs {

constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr int KEYBITS = 160;

// the parts of one device allocation start 256 B apart (host code and the launchers that size work buffers)
inline uint64_t up256(uint64_t b) { return (b + 255) & ~255ull; }

// blocks of b threads that cover n work items (host: every launcher's grid size)
inline unsigned nblk(uint64_t n, unsigned b) { return (unsigned)((n + b - 1) / b); }

// ---------------------------------------------------------------------------
// Per-launch constants derived from ovs_params on the host.  All times are
// int64 ns (simtime-scale = -9, default.ini:27).
struct DelayConsts {
    int64_t msgCall;     // 2*T(L*8/datarate) + 2*T(accessDelay) for FindNodeCall (83 B)
    int64_t msgResp1;    // same for a FindNodeResponse with one NodeHandle (87 B)
    int64_t msgRoute;    // same for the one-way route message (186 B)
    int64_t rpcTimeout;  // T(rpcUdpTimeout)
    int64_t lookupTimeout;  // T(LOOKUP_TIMEOUT)
    int32_t round;       // SimTime(double) rounding rule
    int32_t respBase;    // FindNodeResponse bytes with zero nodes (61 B)
    int32_t respPerNode; // 26 B per NodeHandle
    int32_t callBytes;   // 83 B
    int32_t routeBytes;  // one-way route message, 186 B for testMsgSize = 100 B
    double datarate;
    int64_t access2;     // 2*T(accessDelay)
    int64_t msgRespSib;  // same for the responsible node's FindNodeResponse on a converged Chord ring:
                         // min(numSiblings, 1 + successors) NodeHandles (== msgResp1 for numSiblings = 1)
    int32_t lookupCall;  // LookupCall (ovs_lookup_batch): the lookup ends at the last response, no route message
    int64_t bwCall;      // T(L*8/datarate) of a FindNodeCall, of the route message, and of a FindNodeResponse
    int64_t bwRoute;     // with 0..16 NodeHandles: the constant serialisation terms, precomputed on the host
    int64_t bwResp[17];
};


// SimTime(double) at scale 1e-9: truncation or round-half-up (recorded in every fixture)
__device__ __forceinline__ int64_t simtime_ns(double seconds, int round)
{
    const double x = __dmul_rn(seconds, 1e9);
    return round ? (int64_t)floor(__dadd_rn(x, 0.5)) : (int64_t)x;
}

// coordDelay = SimTime(0.001 * (float)||a-b||), SimpleNodeEntry.cc:145-153,186.
// Explicit _rn operations: no FMA contraction, identical rounding to the
// reference's x86-64 double arithmetic; sqrt correctly rounded, then to float.
__device__ __forceinline__ int64_t coord_ns(double ax, double ay, double bx, double by, int round)
{
    const double dx = __dsub_rn(ax, bx);
    const double dy = __dsub_rn(ay, by);
    const double s = __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy));
    const float f = __double2float_rn(__dsqrt_rn(s));
    return simtime_ns(__dmul_rn(0.001, (double)f), round);
}

// T(L*8 / datarate): the serialisation delay of an L-byte packet
__device__ __forceinline__ int64_t bw_ns(int32_t bytes, double datarate, int round)
{
    return simtime_ns(__ddiv_rn((double)((int64_t)bytes * 8), datarate), round);
}

// 2*T(L*8/datarate) + 2*T(accessDelay) of a FindNodeResponse carrying `nodes` NodeHandles
__device__ __forceinline__ int64_t resp_ns(const DelayConsts& DC, int nodes)
{
    return 2 * bw_ns(DC.respBase + DC.respPerNode * nodes, DC.datarate, DC.round) + DC.access2;
}

__device__ __forceinline__ KeyRec load_rec(const KeyRec* __restrict__ recs, uint32_t i)
{
    const uint2* p = reinterpret_cast<const uint2*>(recs + i);
    const uint2 a = p[0], b = p[1], c = p[2];
    KeyRec r;
    r.w[0] = a.x; r.w[1] = a.y; r.w[2] = b.x; r.w[3] = b.y; r.w[4] = c.x; r.aux = c.y;
    return r;
}

// the key of record i (a 64-bit index: rows of records are longer than 2^32 entries)
__device__ __forceinline__ K160 rkey(const KeyRec* __restrict__ recs, uint64_t i) { return key_of(load_rec(recs + i, 0)); }

// visitOnlyOnce filter: one bit per node hash; a clear bit proves the node unvisited
__device__ __forceinline__ uint64_t vis_bit(uint32_t x) { return 1ull << ((x * 0x9E3779B1u) >> 26); }

// The ovs_route_out of a finished single-path IterativeLookup under a one-way route (KBRTestApp's one-way test):
// the lookup took `hops` responders and t ns from source S at (sx, sy).  On OVS_LOOKUP_OK the route message goes
// to getResult()[0] = `responsible` at (rx, ry) (sendRouteMessage, BaseOverlay.cc:1107-1146, 1240-1258) unless
// that is the source itself; any other status yields the NONE / 0 / -1 record.  The caller supplies (rx, ry): where
// the responsible node is not the iteration's responder, its coordinates come from the overlay's own record loader.
__device__ __forceinline__ ovs_route_out iter_route_out(uint8_t status, int hops, int64_t t, uint32_t responsible, uint32_t S,
                                                        double sx, double sy, double rx, double ry, const DelayConsts& DC)
{
    ovs_route_out o;
    o.hops = (uint16_t)hops;
    o.status = status;
    if (status == OVS_LOOKUP_OK) {
        o.responsible = responsible;
        o.one_way_hops = (uint8_t)(hops + (responsible != S ? 1 : 0));
        int64_t lat = t;
        if (responsible != S) lat += DC.msgRoute + coord_ns(sx, sy, rx, ry, DC.round);
        o.latency_ns = lat;
    } else {
        o.responsible = NONE;
        o.one_way_hops = 0;
        o.latency_ns = -1;
    }
    return o;
}

// ---------------------------------------------------------------------------
// Converged-ring (ideal) Chord layout.  A hop at responder c normally reads ONE
// 64 B line: the finger entry closestPreceedingNode selects carries, besides the
// finger's index, everything the NEXT hop needs about that finger (key,
// coordinates, finger-row offset, the distances of its successor window), so
// the lookup never gathers the next node's record separately.  Ring distances
// d from a node enter as their top 64 bits (bits 96..159, top64()); a compare of
// D = K - c against such a distance is decided unless the top bits are equal,
// and then falls back to the exact keys in recs[] (a tie means K lies within
// 2^96 of a node: node-ID keys, or adjacent IDs closer than 2^96).
//
// NodeRec: per node -- lookup sources, successor hand-offs, shard arrivals.
struct alignas(64) NodeRec {
    uint32_t w[5];   // node key
    uint32_t row;    // offset of the node's finger row (valid on the arc that owns the row)
    double x, y;     // SimpleUnderlay coordinates
    uint64_t gS0;    // top64(succ0 - v)
    uint64_t gSL;    // top64(succ[ns-1] - v), ns = min(successorListSize, n - 1)
    uint64_t gP;     // top64((pred - v) mod 2^160)
};
static_assert(sizeof(NodeRec) == 64, "NodeRec is one 64 B line");

// FingerEnt: row(v)[159 - i] = finger i of v (non-trivial i >= i_lo(v)).
struct alignas(64) FingerEnt {
    uint32_t w[5];   // finger key
    uint32_t idx;    // finger node index
    double x, y;     // finger coordinates
    uint64_t gS0c;   // bits 63..16: the top 48 bits of the finger's gS0; bits 15..0: window codes 1, 2
    uint64_t gSL;    // the finger's gSL (its NodeRec field)
    uint32_t row;    // the finger's own row offset
    uint32_t wc;     // window codes 3..6, one byte each (code 3 lowest)
};
static_assert(sizeof(FingerEnt) == 64, "FingerEnt is one 64 B line");
static_assert(offsetof(FingerEnt, gS0c) == offsetof(NodeRec, gS0) && offsetof(FingerEnt, gSL) == offsetof(NodeRec, gSL),
              "a lane unpacks either line the same way");

// WinRec: per node of the arc, top64(succ_j - v) for j = 0..7 (unused slots all-ones);
// read only when K falls inside the successor window.
struct alignas(64) WinRec {
    uint64_t g[8];
};

__device__ __host__ __forceinline__ uint64_t top64(const K160& a) { return (uint64_t)a.w[3] | ((uint64_t)a.w[4] << 32); }

// ---- the window fields of a FingerEnt.  Besides gSL an entry carries a coarse copy of its finger's
// successor window, so that a lookup arriving through the entry with K inside that window picks the
// successor without reading the finger's WinRec:
//  * gS0 narrowed to its top 48 bits (bits 159..112 of succ0 - v).  A compare against it is decided
//    when the top 48 bits differ, as a top64 compare is when the 64 differ; equal bits take the
//    exact keys in recs[] either way.
//  * six window codes, code_j = g_j >> sh for the interior successors j = 1..6 of a window of 8
//    (g_j = top64(succ_j - v), what the WinRec holds), sh = finger_code_shift(gSL).  g_j <= gSL, so a
//    code fits in 8 bits, and codes never decrease in j.  code_j != Dt >> sh decides g_j against Dt;
//    equal codes decide nothing, and the lookup reads the WinRec as before.
//  * "no codes" -- the window has not 8 successors, or gSL == 0 -- is code 1 = 0xFF above code 6 = 0.
constexpr int FINGER_GS0_DROP = 16;                    // low bits of gS0 a finger entry does not carry
constexpr uint64_t FINGER_NO_CODES = 0x0000000000FFull;

__device__ __host__ __forceinline__ int finger_code_shift(uint64_t gSL)
{
    const int m = gSL ? 63 - __builtin_clzll(gSL) : 0;
    return m > 7 ? m - 7 : 0;
}

// the six codes of an entry, code j in byte j - 1
__device__ __host__ __forceinline__ uint64_t finger_codes(uint64_t gS0c, uint32_t wc)
{
    return (gS0c & 0xFFFFull) | ((uint64_t)wc << 16);
}

__device__ __host__ __forceinline__ bool finger_has_codes(uint64_t codes)
{
    return (uint32_t)(codes & 0xFF) <= (uint32_t)(codes >> 40);
}

// the finger's gS0 as far as the entry carries it (low FINGER_GS0_DROP bits zero)
__device__ __host__ __forceinline__ uint64_t finger_gs0(uint64_t gS0c) { return gS0c & ~0xFFFFull; }

// an entry's gS0c and wc from its finger's gS0, gSL and interior window distances g[0..5] = g_1..g_6
// (coded == false: a window of another size, no codes)
__device__ __host__ __forceinline__ void finger_pack(uint64_t gS0, uint64_t gSL, const uint64_t (&g)[6], bool coded,
                                                     uint64_t* gS0c, uint32_t* wc)
{
    uint64_t codes = FINGER_NO_CODES;
    if (coded && gSL) {
        const int sh = finger_code_shift(gSL);
        codes = 0;
#pragma unroll
        for (int j = 0; j < 6; ++j) codes |= ((g[j] >> sh) & 0xFF) << (8 * j);
    }
    *gS0c = finger_gs0(gS0) | (codes & 0xFFFF);
    *wc = (uint32_t)(codes >> 16);
}

// the farthest successor j of a window of 8 with g_j < Dt, from the codes and cD = Dt >> sh, given that
// g_0 < Dt < g_7 is known: the number of interior codes below cD.  *tie: an interior code equals cD
// (the result is then not decided)
__device__ __host__ __forceinline__ int finger_win_scan(uint64_t codes, uint32_t cD, bool* tie)
{
    int tj = 0;
    bool eq = false;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const uint32_t cj = (uint32_t)(codes >> (8 * j)) & 0xFF;
        tj += cj < cD ? 1 : 0;
        eq |= cj == cD;
    }
    *tie = eq;
    return tj;
}

__device__ __forceinline__ double dbl(uint32_t lo, uint32_t hi) { return __hiloint2double((int)hi, (int)lo); }

// Chord device view.
//  recs[n]      : sorted node keys (24 B), aux = offset of the node's finger row
//  xy[n]        : SimpleUnderlay coordinates (fp64)
//  nodes[n]     : ideal mode -- NodeRec per node (64 B)
//  win[hi-lo]   : ideal mode -- WinRec per node of the arc [lo, hi)
//  frow[...]    : ideal mode -- CSR rows of FingerEnt (64 B),
//                 row(v)[159 - i] = finger i for the non-trivial positions
//                 i >= i_lo(v) = msb(succ0 - v) + 1 (trivial positions resolve to
//                 succ0, ChordFingerTable.cc:183-184)
//  general mode : pred[n], succ[n*sls], nsucc[n], fres[n*160] = getFinger(i) resolved
struct ChordView {
    const KeyRec* __restrict__ recs;
    const double2* __restrict__ xy;
    const NodeRec* __restrict__ nodes;
    const FingerEnt* __restrict__ frow;
    const WinRec* __restrict__ win;
    uint32_t lo;       // ideal: first node of this context's arc (win index base)
    const uint32_t* __restrict__ pred;
    const uint32_t* __restrict__ succ;
    const uint8_t* __restrict__ nsucc;
    const uint32_t* __restrict__ fres;
    uint32_t n;
    int32_t ns;        // ideal: min(successorListSize, n-1)
    int32_t sls;       // successor list stride (general)
    int32_t numFingerCandidates;
    // sharded rings (ovs_chord_shard_replicate): the top `ftl` finger levels of EVERY node,
    // ftop[v * ftl + (159 - i)] = finger i of v for i >= 160 - ftl, so a lookup's first hops --
    // the long jumps that cross arcs -- are decided on the rank that holds the lookup
    const FingerEnt* __restrict__ ftop;
    int32_t ftl;
};

constexpr int MAXSHARDS = 64;
struct ShardMap {
    uint64_t lo[MAXSHARDS + 1];   // arc r = [lo[r], lo[r+1]) of the sorted ring
    int n;
};

struct LookupConsts {
    int32_t hopCountMax;
    int32_t numSiblings;
    int32_t numRedundantNodes;
    int32_t recursive;          // routingType semi-/full-recursive: hop-by-hop route message
};

}  // namespace ovs
