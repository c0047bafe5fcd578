// pastry_host.hpp -- what Pastry's host and device code share and a plain C++ compiler can build: the table
// shape, the key arithmetic, the parameter refusals, the leaf-set replay for small networks and the validation
// of explicit tables (tests/pastry_host_driver.cpp runs them under the sanitizers without a HIP compiler).
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/ovs_kbr.h"
#include "key160.hpp"

namespace ovs {

constexpr int PASTRY_MAX_LEAVES = 32;
constexpr uint32_t PASTRY_NONE = 0xFFFFFFFFu;

struct PastryShape {
    int b = 4;           // bitsPerDigit
    int L = 16;          // numberOfLeaves
    int opt = 0;         // optimizeLookup
    int reg = 1;         // useRegularNextHop
    OVS_HD int P() const { return 1 << b; }
    OVS_HD int max_rows() const { return 160 / b; }
};

inline PastryShape pastry_shape_of(const ovs_pastry_params& bp)
{
    PastryShape sh;
    sh.b = bp.bitsPerDigit; sh.L = bp.numberOfLeaves; sh.opt = bp.optimizeLookup ? 1 : 0; sh.reg = bp.useRegularNextHop ? 1 : 0;
    return sh;
}

// the table parameters the engine implements; the reason otherwise
inline const char* pastry_shape_refusal(const ovs_pastry_params& bp)
{
    if (bp.bitsPerDigit < 1 || bp.bitsPerDigit > 4) return "Pastry: bitsPerDigit must be 1..4";
    if (bp.numberOfLeaves % 2) return "Pastry: numberOfLeaves must be even.";
    if (bp.numberOfLeaves < 2 || bp.numberOfLeaves > PASTRY_MAX_LEAVES) return "Pastry: numberOfLeaves must be 2..32";
    if (bp.numberOfNeighbors != 0)
        return "Pastry: numberOfNeighbors != 0 is not implemented (the neighbourhood set is filled by proximity)";
    return nullptr;
}

// what ovs_pastry_route_batch refuses before it looks at the batch
inline const char* pastry_route_refusal(const ovs_params& P, const ovs_pastry_params& bp)
{
    if (P.routingType == 0 || P.routingType == 3)
        return "Pastry: iterative lookups need PastryFindNodeExtData (DESIGN.md §8); routingType must be semi-recursive";
    if (P.routingType == 2) return "Pastry: full-recursive routing is not implemented; routingType must be semi-recursive";
    if (P.routingType == 4) return "Pastry: source-routing-recursive is not implemented; routingType must be semi-recursive";
    if (P.routingType != 1) return "Pastry: routingType must be semi-recursive";
    if (bp.routeMsgAcks)
        return "Pastry: routeMsgAcks = true is not implemented (the per-hop NextHopCall ack shares the forwarder's "
               "transmit queue with the forwarded message, DESIGN.md §9); set routeMsgAcks = false";
    if (P.numSiblings != 1) return "Pastry routes implement numSiblings = 1";
    if (P.recNumRedundantNodes < 1 || P.recNumRedundantNodes > 8) return "Pastry routes implement recNumRedundantNodes 1..8";
    return pastry_shape_refusal(bp);
}

// What ovs_pastry_lookup_batch and ovs_pastry_iterative_route_batch refuse before they look at the batch.  route:
// the one-way message, whose final sendRouteMessage passes routeMsgAcks (BaseOverlay.cc:1254-1257); the LookupCall
// sends FindNodeCalls only and runs with either value.
inline const char* pastry_iterative_refusal(const ovs_params& P, const ovs_pastry_params& bp, bool route)
{
    if (P.routingType != 0)
        return "Pastry: iterative lookups run with routingType = iterative (semi-recursive routes: ovs_pastry_route_batch)";
    if (P.hopCountMax < 1)
        return "Pastry: iterative lookups need hopCountMax >= 1 (the hop list is the visitOnlyOnce list)";
    if (P.lookupRedundantNodes != 1) return "Pastry: iterative lookups implement lookupRedundantNodes = 1";
    if (P.lookupParallelRpcs != 1) return "Pastry: iterative lookups implement lookupParallelRpcs = 1";
    if (P.lookupParallelPaths != 1) return "Pastry: iterative lookups implement lookupParallelPaths = 1";
    if (P.lookupMerge) return "Pastry: iterative lookups implement lookupMerge = false";
    if (!P.lookupVisitOnlyOnce) return "Pastry: iterative lookups implement lookupVisitOnlyOnce = true";
    if (P.lookupFinishOnFirstUnchanged) return "Pastry: iterative lookups implement lookupFinishOnFirstUnchanged = false";
    if (route && bp.routeMsgAcks)
        return "Pastry: routeMsgAcks = true is not implemented (the per-hop NextHopCall ack shares the forwarder's "
               "transmit queue with the forwarded message, DESIGN.md §9); set routeMsgAcks = false";
    if (route && P.numSiblings != 1) return "Pastry routes implement numSiblings = 1";
    return pastry_shape_refusal(bp);
}

// ---- routes under routeMsgAcks (ovs_pastry_acked_route_batch, ovs_pastry_rpc_batch) -----------------------------
// Wire lengths in bytes, the 28 B UDP/IP header counted once.  NEXTHOPCALL_L = BASECALL_L = BASERPC_L = TYPE_L 8 +
// NONCE_L 32 + NODEHANDLE_L 208 + TIER_L 8 = 256 bits (CommonMessages.msg:30, 34, 42, 52, 69-71, 88) around the
// route message (BaseOverlay.cc:1135-1144): BASEROUTE_L 424 bits + BASEAPPDATA_L 40 bits + the payload.
// NEXTHOPRESPONSE_L = BASERESPONSE_L = BASERPC_L + AUTHBLOCK_L (800 bits under measureAuthBlock) with no NCS
// info (CommonMessages.msg:57, 73-76, 89).
inline int64_t pastry_nexthop_call_bytes(const ovs_params& P) { return 32 + 58 + (int64_t)P.testMsgSize + 28; }
inline int64_t pastry_nexthop_ack_bytes(const ovs_params& P) { return 32 + (P.measureAuthBlock ? 100 : 0) + 28; }
// the direct KbrTestResponse: payload + BASEAPPDATA_L 40 bits (BaseOverlay.cc:1340-1341, CommonMessages.msg:68)
inline int64_t pastry_rpc_response_bytes(const ovs_params& P) { return (int64_t)P.testMsgSize + 5 + 28; }
// SimpleUnderlayNetwork.underlayConfigurator.sendQueueLength = 1MB (default.ini:553), read as 10^6 B
constexpr int64_t PASTRY_SEND_QUEUE_BYTES = 1000000;

// What ovs_pastry_acked_route_batch (rpc false) and ovs_pastry_rpc_batch (rpc true) refuse before they look at
// the batch: what pastry_route_refusal / pastry_iterative_refusal refuse apart from routeMsgAcks, the routing
// types without an acked form, and a transmit queue that one ack plus the packet behind it overruns
// (SimpleNodeEntry.cc:168-181: the reference drops the second packet there).
inline const char* pastry_acked_refusal(const ovs_params& P, const ovs_pastry_params& bp, bool rpc)
{
    ovs_pastry_params plain = bp;
    plain.routeMsgAcks = 0;
    if (P.routingType == 0 && !rpc) {
        if (const char* why = pastry_iterative_refusal(P, plain, true)) return why;
    } else {
        if (P.routingType == 0 || P.routingType == 3)
            return "Pastry: the RPC test is implemented for routingType = semi-recursive (the iterative lookup test is "
                   "not part of it)";
        if (const char* why = pastry_route_refusal(P, plain)) return why;
    }
    if (P.testMsgSize < 0) return "Pastry: testMsgSize must be >= 0";
    if (bp.routeMsgAcks)
        // the KbrTestResponse behind a responder's ack is shorter than the call
        if (pastry_nexthop_ack_bytes(P) + pastry_nexthop_call_bytes(P) > PASTRY_SEND_QUEUE_BYTES)
            return "Pastry: a NextHopResponse and the NextHopCall behind it exceed sendQueueLength = 1MB in a forwarder's "
                   "transmit queue (testMsgSize); the reference drops there and drops are not modelled";
    return nullptr;
}

// KeyRingMetric::distance (Comparator.h:121-131) = PastryStateObject::keyDist (PastryStateObject.cc:107-132)
OVS_HD K160 p_ring_dist(const K160& x, const K160& y)
{
    const K160 d1 = k_sub(x, y), d2 = k_sub(y, x);
    return k_gt(d1, d2) ? d2 : d1;
}

// OverlayKey::sharedPrefixLength (OverlayKey.cc:530-555) in bits
OVS_HD int p_spl_bits(const K160& a, const K160& b) { return 159 - k_msb(k_xor(a, b)); }
// ... in digits: equal keys give keyLength whatever the digit size (533)
OVS_HD int p_spl_digits(const K160& a, const K160& b, int bpd) { return k_eq(a, b) ? 160 : p_spl_bits(a, b) / bpd; }

// getBitRange(p, nb) (458-474), p + nb <= 160, nb <= 4
OVS_HD uint32_t p_bits(const K160& a, int p, int nb)
{
    const int q = p >> 5, f = p & 31;
    uint32_t v = k_word(a, q) >> f;
    if (f + nb > 32) v |= k_word(a, q + 1) << (32 - f);
    return v & ((1u << nb) - 1u);
}
// PastryRoutingTable::digitAt (28-32); the caller keeps (n + 1) * b <= 160
OVS_HD uint32_t p_digit(const K160& a, int n, int b) { return p_bits(a, 160 - (n + 1) * b, b); }

// ---- the leaf set of a small network, replayed on the host --------------------------------------------------
// PastryLeafSet::mergeNode / insertLeaf / balanceLeafSet (PastryLeafSet.cc:261-410, without callUpdate) for owner
// `me`: every other node merged clockwise from the owner's successor.  out[L], PASTRY_NONE = unspecified.
struct PastryLeafReplay {
    const K160* ids;
    uint32_t me;
    int L;
    std::vector<uint32_t> lv;
    bool full = false;

    PastryLeafReplay(const K160* ids, uint32_t me, int L) : ids(ids), me(me), L(L), lv((size_t)L, PASTRY_NONE) {}
    int smaller() const { return L / 2 - 1; }
    int bigger() const { return L / 2; }
    // isBetween with unspecified keys (OverlayKey.cc:590)
    bool btw(uint32_t x, uint32_t a, uint32_t b) const
    {
        return x != PASTRY_NONE && a != PASTRY_NONE && b != PASTRY_NONE && between_open(ids[x], ids[a], ids[b]);
    }
    void balance()
    {
        const size_t n = lv.size();
        if (full || (lv[0] != PASTRY_NONE && lv[n - 2] != PASTRY_NONE) || (lv[n - 1] != PASTRY_NONE && lv[1] != PASTRY_NONE)) return;
        for (int il = smaller(), ir = bigger(); ir != (int)n; --il, ++ir) {
            if (lv[(size_t)il] == PASTRY_NONE) {
                if (lv[(size_t)ir] == PASTRY_NONE || ir + 1 == (int)n || lv[(size_t)ir + 1] == PASTRY_NONE) return;
                lv[(size_t)il] = lv[(size_t)ir + 1];
                lv[(size_t)ir + 1] = PASTRY_NONE;
                return;
            }
            if (lv[(size_t)ir] == PASTRY_NONE) {
                if (il == 0 || lv[(size_t)il - 1] == PASTRY_NONE) return;
                lv[(size_t)ir] = lv[(size_t)il - 1];
                lv[(size_t)il - 1] = PASTRY_NONE;
                return;
            }
        }
    }
    void insert(int it, uint32_t node)
    {
        if (it <= smaller()) {
            lv.insert(lv.begin() + it + 1, node);
            if (lv.front() != PASTRY_NONE && lv.back() == PASTRY_NONE) lv.back() = lv.front();
            lv.erase(lv.begin());
        } else {
            lv.insert(lv.begin() + it, node);
            if (lv.back() != PASTRY_NONE && lv.front() == PASTRY_NONE) lv.front() = lv.back();
            lv.pop_back();
        }
        full = lv.front() != PASTRY_NONE && lv.back() != PASTRY_NONE;
        if (!full) balance();
    }
    bool merge(uint32_t node)
    {
        uint32_t last_left = me, last_right = me;
        int il = smaller(), ir = bigger();
        for (uint32_t x : lv) {
            if (x == PASTRY_NONE) { full = false; continue; }
            if (x == node) return false;
        }
        while (true) {
            if (!full) {
                if (lv[(size_t)il] == PASTRY_NONE && lv[(size_t)ir] == PASTRY_NONE) { insert(il, node); return true; }
                if (lv[(size_t)il] == PASTRY_NONE && !btw(node, last_right, lv[(size_t)ir])) { insert(il, node); return true; }
                if (lv[(size_t)ir] == PASTRY_NONE && !btw(node, lv[(size_t)il], last_left)) { insert(ir, node); return true; }
            }
            if (btw(node, lv[(size_t)il], last_left)) { insert(il, node); return true; }
            if (btw(node, last_right, lv[(size_t)ir])) { insert(ir, node); return true; }
            last_right = lv[(size_t)ir];
            if (++ir == L) break;
            last_left = lv[(size_t)il];
            --il;
        }
        return false;
    }
};

inline void pastry_host_leaves(const K160* ids, uint32_t n, int L, uint32_t me, uint32_t* out)
{
    PastryLeafReplay r(ids, me, L);
    for (uint32_t j = 1; j < n; ++j) r.merge((me + j) % n);
    for (int j = 0; j < L; ++j) out[j] = r.lv[(size_t)j];
}

// Explicit tables: leaf[n][L], table[n][rows][2^b] node indices, PASTRY_NONE = unspecified.  false + *err
// naming the node otherwise.
inline bool pastry_validate_tables(const K160* ids, uint64_t n, const PastryShape& sh, int rows, const uint32_t* leaf,
                                   const uint32_t* table, std::string* err)
{
    if (rows < 1 || rows > sh.max_rows()) { *err = "rows must be 1 .. 160 / bitsPerDigit"; return false; }
    const uint64_t P = (uint64_t)sh.P();
    for (uint64_t v = 0; v < n; ++v) {
        const std::string where = "node " + std::to_string(v);
        const uint32_t* lr = leaf + v * (uint64_t)sh.L;
        int cnt = 0;
        for (int j = 0; j < sh.L; ++j) {
            if (lr[j] == PASTRY_NONE) continue;
            if (lr[j] >= n) { *err = where + ": leaf index out of range"; return false; }
            if (lr[j] == v) { *err = where + ": the leaf set holds its owner"; return false; }
            for (int i = 0; i < j; ++i)
                if (lr[i] == lr[j]) { *err = where + ": the leaf set holds a node twice"; return false; }
            ++cnt;
        }
        if (!cnt) { *err = where + ": the leaf set is empty"; return false; }
        for (int r = 0; r < rows; ++r)
            for (uint64_t c = 0; c < P; ++c) {
                const uint32_t x = table[(v * (uint64_t)rows + (uint64_t)r) * P + c];
                if (x == PASTRY_NONE) continue;
                if (x >= n) { *err = where + ": table index out of range"; return false; }
                // shares exactly r digits with the owner (x == v shares all) and has digit c at r
                if (x == v || p_spl_bits(ids[v], ids[x]) / sh.b != r || p_digit(ids[x], r, sh.b) != (uint32_t)c) {
                    *err = where + " row " + std::to_string(r) + " column " + std::to_string(c) +
                           ": the entry does not share the row's prefix or has another digit";
                    return false;
                }
            }
    }
    return true;
}

}  // namespace ovs
