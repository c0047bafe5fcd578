// ovs_route.cpp -- the route / lookup / findNode seam of the C ABI (include/ovs_kbr.h): route_check / route_device and
// lookup_check / lookup_device (ctx.hpp), the entry points built on them, the findNode batches and the delay batch.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>

#include "ctx.hpp"
#include "persist.hpp"

using namespace ovs;

namespace ovs {

// A zeroed work counter for one launch of a persistent route kernel (the dynamic tail of K1,
// launch_chord_route, and K2, kad_route), released when the lease goes out of scope: get() is
// nullptr when none can be had -- the kernel then runs static slices only.
DynSlots::Lease dyn_acquire(ovs_ctx* c, uint64_t n, hipStream_t s)
{
    if (!persist_dyn_enabled()) return {};                // A/B: static slices only
    if (n < (1ull << 18)) return {};                      // small batches: static slices (no memset, no event)
    return c->dyn.acquire(s);
}

// K1 key order, opt-in (OVS_K1_SORT=1): one-way iterative Chord batches of at least
// OVS_K1_SORT_MIN lookups (default 2^20) routed in the order of their keys' top bits.  Off by default:
// measured, the sort costs more than the locality it buys at any bin width one pass can sort
static bool ksort_wanted(uint64_t n)
{
    const char* o = std::getenv("OVS_K1_SORT");      // read per call (one getenv per batch)
    const int on = o ? std::atoi(o) : 0;
    const char* m = std::getenv("OVS_K1_SORT_MIN");
    const uint64_t lim = m ? (uint64_t)std::strtoull(m, nullptr, 10) : (1ull << 20);
    return on != 0 && n >= lim && n < 0xFFFFFFFFull;
}

// coordDelay of the farthest pair the bounding box admits (host copy of engine.hpp coord_ns: the
// same IEEE operations; every step is monotone in |dx|, |dy|, so no pair of nodes exceeds it)
static int64_t coord_ns_host(double dx, double dy, int round)
{
    const double s2 = dx * dx + dy * dy;
    const float f = (float)std::sqrt(s2);
    return simtime_host(0.001 * (double)f, round);
}

// extendedFingerTable (Chord.cc:416-419, 627-641; ChordFingerTable.cc:195-228) changes a lookup only
// through its start: IterativeLookup::start takes numFingerCandidates nodes from the source's
// findNode, the first of them the non-extended choice, and with lookupMerge = false the first
// response replaces them (IterativeLookup.cc:840-846) while every later FindNodeCall asks for one
// node -- so routes differ only when a first FindNodeCall times out (the reference then tries the
// next candidate).  Accepted when no call can: the largest RTT the coordinates' bounding box admits
// (call + the largest response + twice the farthest coordinate delay) is below rpcUdpTimeout
// (the oracle restates the candidates, tests/test_oracle_extended.py).
static ovs_status check_extended_fingers(ovs_ctx* c, const ovs_params& P)
{
    if (!c->ideal)
        return fail(c, OVS_ENOTSUP, "extendedFingerTable: explicit tables carry no finger candidate lists");
    if (P.routingType != 0) return OVS_OK;     // recursive routes: route messages, no RPC timeouts
    if (!c->bbox_ok) {
        if (!c->xy || c->n == 0) return fail(c, OVS_ESTATE, "no network loaded");
        CallFrame F(false, c->stream);
        double* d = F.scratch<double>(4 * 256);
        if (!F.ok()) return frame_fail(c, F);
        int blocks = 0;
        double h[4 * 256];
        hipError_t e = launch_xy_bbox(c->xy, c->n, d, &blocks, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(h, d, sizeof(double) * 4 * blocks, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return hip_fail(c, e, "coordinate bounding box");
        c->bbox[0] = h[0]; c->bbox[1] = h[1]; c->bbox[2] = h[2]; c->bbox[3] = h[3];
        for (int b = 1; b < blocks; ++b) {
            c->bbox[0] = std::min(c->bbox[0], h[4 * b]); c->bbox[1] = std::max(c->bbox[1], h[4 * b + 1]);
            c->bbox[2] = std::min(c->bbox[2], h[4 * b + 2]); c->bbox[3] = std::max(c->bbox[3], h[4 * b + 3]);
        }
        c->bbox_ok = true;
    }
    const DelayConsts DC = delay_consts(P);
    const int64_t cd = coord_ns_host(c->bbox[1] - c->bbox[0], c->bbox[3] - c->bbox[2], P.simtimeRound);
    const int64_t resp = 2 * simtime_host((double)((int64_t)(DC.respBase + DC.respPerNode * (1 + P.successorListSize)) * 8) /
                                              P.datarate, P.simtimeRound) + DC.access2;
    const int64_t rtt = DC.msgCall + std::max(resp, DC.msgResp1) + 2 * cd;
    if (rtt >= DC.rpcTimeout)
        return fail(c, OVS_ENOTSUP,
                    "extendedFingerTable: a FindNodeCall could time out (largest RTT " + std::to_string(rtt) +
                        " ns >= rpcUdpTimeout), where the extended table's next start candidate would be tried");
    return OVS_OK;
}

ovs_status check_chord_route(ovs_ctx* c, const ovs_params& P)
{
    if (P.lookupMerge) return fail(c, OVS_EINVAL, "Chord doesn't work with iterativeLookupConfig.merge = true!");
    if (P.extendedFingerTable) {
        if (ovs_status st = check_extended_fingers(c, P)) return st;
    }
    if (P.routingType != 0) {
        // recursive: the route message follows findNode's first acceptable candidate hop by hop
        if (P.numSiblings != 1) return fail(c, OVS_ENOTSUP, "recursive Chord routing implements numSiblings=1");
        if (!c->ideal)
            return fail(c, OVS_ENOTSUP, "recursive routing is implemented for converged (ovs_chord_load) rings");
        return OVS_OK;
    }
    if (P.lookupRedundantNodes != 1 || P.lookupParallelRpcs != 1 || P.numSiblings != 1)
        return fail(c, OVS_ENOTSUP,
                    "Chord route kernel implements lookupRedundantNodes=1, lookupParallelRpcs=1, numSiblings=1");
    return OVS_OK;
}

ovs_status check_sources(ovs_ctx* c, const uint32_t* src, uint64_t n, bool dev)
{
    if (dev) return OVS_OK;
    for (uint64_t i = 0; i < n; ++i)
        if (src[i] >= c->n) return fail(c, OVS_EINVAL, "source index out of range (lookup " + std::to_string(i) + ")");
    return OVS_OK;
}

// the overlays with entry points of their own, refused; a caller that serves Koorde says so, and may word the
// EpiChord refusal itself
static ovs_status refuse_dedicated(ovs_ctx* c, bool serves_koorde = false, const char* epichord = nullptr)
{
    if (c->overlay == OVS_OVERLAY_KOORDE && !serves_koorde)
        return fail(c, OVS_ENOTSUP, "Koorde: ovs_route_batch and ovs_koorde_find_node_batch only");
    if (c->overlay == OVS_OVERLAY_EPICHORD)
        return fail(c, OVS_ENOTSUP, epichord ? epichord : "EpiChord: ovs_epichord_find_node_batch only");
    if (c->overlay == OVS_OVERLAY_BROOSE)
        return fail(c, OVS_ENOTSUP, "Broose: ovs_broose_route_batch and ovs_broose_find_node_batch only");
    if (c->overlay == OVS_OVERLAY_PASTRY)
        return fail(c, OVS_ENOTSUP, "Pastry: ovs_pastry_route_batch and ovs_pastry_find_node_batch only");
    return OVS_OK;
}

ovs_status route_check(ovs_ctx* c, const ovs_params& P, hipStream_t s)
{
    if (!c->overlay) return fail(c, OVS_ESTATE, "no network loaded");
    ovs_status st = refuse_dedicated(c, true, "EpiChord lookups rewrite the caches they route over (DESIGN.md §9): "
                                        "ovs_epichord_find_node_batch only");
    if (st != OVS_OK) return st;
    if ((st = check_common(c, P)) != OVS_OK) return st;
    HIPCHK(c, hipSetDevice(c->device));
    if (c->overlay == OVS_OVERLAY_CHORD) {
        if ((st = check_chord_route(c, P)) != OVS_OK) return st;
        if (c->ideal && (c->shard_lo != 0 || c->shard_hi != c->n))
            return fail(c, OVS_ESTATE, "context holds one arc of a sharded ring: use ovs_shard_step");
        // explicit tables: the hop list (hopCountMax entries) is the lookup's visited set
        if (!c->ideal && P.hopCountMax < 1)
            return fail(c, OVS_ENOTSUP, "explicit Chord tables need hopCountMax >= 1 (the hop list is the visited set)");
        return ensure_nodes(c, s);
    }
    if (c->overlay == OVS_OVERLAY_KOORDE) {
        if (P.routingType != 0) return fail(c, OVS_ENOTSUP, "Koorde routing is implemented for routingType = iterative");
        // the hop list (hopCountMax entries) is the visitOnlyOnce list: no hop limit leaves it without a size
        if (P.hopCountMax < 1) return fail(c, OVS_ENOTSUP, "Koorde lookups need hopCountMax >= 1");
        if (P.lookupRedundantNodes != 1 || P.lookupParallelRpcs != 1 || P.lookupMerge || P.numSiblings != 1 ||
            !P.lookupVisitOnlyOnce)
            return fail(c, OVS_ENOTSUP,
                        "Koorde route kernel implements lookupRedundantNodes=1, lookupParallelRpcs=1, merge off, "
                        "visitOnlyOnce, numSiblings=1 (the Koorde defaults)");
        return OVS_OK;
    }
    if (P.routingType < 0 || P.routingType > 4)
        return fail(c, OVS_ENOTSUP, "Kademlia routing is implemented for routingType = iterative / semi-recursive / "
                                    "full-recursive / exhaustive-iterative / source-routing-recursive");
    if (c->kad.general && P.routingType == 3)
        return fail(c, OVS_ENOTSUP, "CSR (b > 1 / nr128 / nkademlia) tables: routingType iterative or recursive");
    if (P.numSiblings != 1)
        return fail(c, OVS_ENOTSUP, "the one-way route implements numSiblings = 1 (LookupCall: ovs_lookup_batch)");
    if (c->kad.lo != 0 || c->kad.hi != c->n)
        return fail(c, OVS_ESTATE, "context holds one arc of a sharded network: use ovs_kad_shard_step");
    return OVS_OK;
}

ovs_status visited_lists(ovs_ctx* c, uint32_t** dhop, uint64_t n, uint64_t H, hipStream_t s, CachedBuf::Lease* vis)
{
    if (*dhop) {
        HIPCHK(c, hipMemsetAsync(*dhop, 0xFF, sizeof(uint32_t) * n * H, s));
        return OVS_OK;
    }
    *vis = c->kvis.acquire(sizeof(uint32_t) * n * H, s);
    if (!*vis) return lease_fail(c, "kvis", *vis);
    *dhop = reinterpret_cast<uint32_t*>(vis->data());
    return OVS_OK;
}

ovs_status route_device(ovs_ctx* c, const ovs_params& P, CallFrame& F, const K160* dk, const uint32_t* ds, uint64_t n,
                        ovs_route_out* dout, uint32_t* dhop, uint32_t* drpc, hipStream_t s)
{
    const int H = P.hopCountMax > 0 ? P.hopCountMax : 1;
    const bool hop_seq = dhop != nullptr;
    // hop sequence buffer: always needed for explicit Chord tables and Koorde (the visited check).
    // Koorde without a hop_seq request uses a context scratch buffer, unpadded: K3 reads back only
    // the entries a lookup wrote
    const bool koorde_scratch = c->overlay == OVS_OVERLAY_KOORDE && !hop_seq;
    // exhaustive-iterative Kademlia: the responder list is the lookup's visited set
    const bool kad_exh = c->overlay == OVS_OVERLAY_KADEMLIA && P.routingType == 3;
    // source-routing-recursive Kademlia: the hop list is the message's visitedHops
    const bool kad_src = c->overlay == OVS_OVERLAY_KADEMLIA && P.routingType == 4;
    const bool need_hop = hop_seq || (c->overlay == OVS_OVERLAY_CHORD && !c->ideal) || kad_exh || kad_src;
    CachedBuf::Lease vis;
    if (!hop_seq && (koorde_scratch || need_hop)) {
        // an internal hop list (Koorde, explicit Chord tables, exhaustive Kademlia: the visited sets) in
        // the context's cached buffer, not a per-call allocation
        vis = c->kvis.acquire(sizeof(uint32_t) * n * H, s);
        if (!vis) return lease_fail(c, "kvis", vis);
        dhop = reinterpret_cast<uint32_t*>(vis.data());
    }
    if (dhop && !koorde_scratch) HIPCHK(c, hipMemsetAsync(dhop, 0xFF, sizeof(uint32_t) * n * H, s));
    const DelayConsts DC = delay_consts(P);
    hipError_t e;
    if (c->overlay == OVS_OVERLAY_CHORD) {
        LookupConsts LC{P.hopCountMax, P.numSiblings, P.lookupRedundantNodes, P.routingType != 0};
        if (c->ideal && !LC.recursive && ksort_wanted(n)) {
            // key order: the batch sorted by its keys' top bits, results written at the caller's indices, in
            // the context's key-order buffers: the sort's scratch, caller indices, sorted sources and keys
            const CachedBuf::Lease ks = c->ks.acquire(n * (sizeof(K160) + 8) + 4 * ksort_scratch_words() + 256, s);
            if (!ks) return lease_fail(c, "key-order buffers", ks);
            uint32_t* scr = reinterpret_cast<uint32_t*>(ks.data());
            uint32_t* pm = scr + ksort_scratch_words();
            uint32_t* ss = pm + n;
            K160* sk = reinterpret_cast<K160*>(ss + n);
            const char* kb = std::getenv("OVS_K1_SORT_BITS");
            e = ksort_launch(dk, ds, n, scr, sk, ss, pm, kb ? std::atoi(kb) : 14, s);
            if (e == hipSuccess) e = launch_chord_route(chord_view(c), c->ideal, DC, LC, sk, ss, n, dout, dhop, c->num_cu, s, pm);
        } else {
            const DynSlots::Lease dyn = dyn_acquire(c, n, s);
            e = launch_chord_route(chord_view(c), c->ideal, DC, LC, dk, ds, n, dout, dhop, c->num_cu, s, nullptr, dyn.get());
        }
        if (e == hipSuccess && drpc) {
            if (LC.recursive) e = hipMemsetAsync(drpc, 0, sizeof(uint32_t) * n, s);   // no FindNodeCalls
            else e = launch_fill_rpcs_from_hops(dout, n, drpc, s);
        }
    } else if (c->overlay == OVS_OVERLAY_KOORDE) {
        const DynSlots::Lease dyn = dyn_acquire(c, n, s);
        e = koorde_route(c->koorde, c->recs, c->xy, DC, P.hopCountMax, dk, ds, n, dout, dhop, !koorde_scratch, drpc,
                         c->num_cu, s, dyn.get());
    } else if (kad_exh) {
        // sendToKey with EXHAUSTIVE_ITERATIVE_ROUTING (BaseOverlay.cc:1434-1442): lookup(key, numSiblings = 1)
        // with redundantNodes = lookupRedundantNodes, the route message to getResult()[0]
        uint32_t* dres = F.scratch<uint32_t>(n);
        if (!F.ok()) return frame_fail(c, F);
        bool cap_err = false;
        // dhop was filled with NONE above: the kernel leaves the rows unpadded
        e = kad_exhaustive(c->kad, c->xy, (uint32_t)c->n, P, DC, P.lookupRedundantNodes, 1, true, dk, ds, n, dout, dres, dhop,
                           nullptr, drpc, c->num_cu, s, persist_dyn_enabled(), &cap_err, nullptr, false,
                           !hop_seq /* nobody reads the visited sets: their first entries in LDS */);
        if (e == hipSuccess && cap_err) return fail(c, OVS_ENOTSUP, "a lookup exceeded the kernel's capacity (64 timed-out nodes)");
    } else if (P.routingType == 1 || P.routingType == 2 || kad_src) {
        // R/Kademlia: recursive routing with Kademlia's recursiveRoutingHook (kad_general.hip)
        e = kad_route_recursive(c->kad, c->xy, (uint32_t)c->n, P, DC, simtime_host(P.rpcKeyTimeout, P.simtimeRound), 1, dk, ds,
                                n, dout, dhop, nullptr, s);
        if (e == hipSuccess && drpc) e = hipMemsetAsync(drpc, 0, sizeof(uint32_t) * n, s);   // no FindNodeCalls
    } else if (c->kad.general) {
        e = kad_route_general(c->kad, c->xy, (uint32_t)c->n, P, DC, dk, ds, n, dout, dhop, drpc, s, nullptr);
    } else {
        const DynSlots::Lease dyn = dyn_acquire(c, n, s);
        e = kad_route(c->kad, c->xy, (uint32_t)c->n, P, DC, dk, ds, n, dout, dhop, drpc, c->num_cu, s, nullptr, dyn.get());
    }
    vis.release();      // dhop is ordered by the buffer's event: a device-pointer call stays asynchronous
    return e == hipSuccess ? OVS_OK : hip_fail(c, e, "route kernel");
}

ovs_status lookup_check(ovs_ctx* c, const ovs_params& P0, int32_t num_siblings, hipStream_t s, int32_t* ns_out)
{
    if (!c->overlay) return fail(c, OVS_ESTATE, "no network loaded");
    ovs_status st = refuse_dedicated(c);
    if (st != OVS_OK) return st;
    const bool chord = c->overlay == OVS_OVERLAY_CHORD;
    // BaseOverlay::lookupRpc: numSiblings < 0 -> getMaxNumSiblings() (Chord.cc getMaxNumSiblings =
    // successorListSize, Kademlia.cc:347-350 = s); isSiblingFor rejects larger values
    const int32_t maxs = chord ? P0.successorListSize : P0.s;
    const int32_t ns = num_siblings < 0 ? maxs : num_siblings;
    if (ns > maxs) return fail(c, OVS_EINVAL, "numSiblings too big!");
    if (ns == 0 && P0.routingType == 3)
        return fail(c, OVS_ENOTSUP, "LookupCall with numSiblings = 0 (exact-key lookup): iterative or recursive routing");
    if (ns == 0 && chord && P0.routingType != 0)
        return fail(c, OVS_ENOTSUP, "Chord LookupCall with numSiblings = 0 (exact-key lookup): iterative routing");
    if (ns == 0 && chord && P0.hopCountMax < 1)
        return fail(c, OVS_ENOTSUP, "Chord exact-key LookupCalls need hopCountMax >= 1");
    if (ns > 8) return fail(c, OVS_ENOTSUP, "LookupCall implements numSiblings <= 8");
    ovs_params P = P0;
    P.numSiblings = 1;          // the route checks: one-way configuration, numSiblings applied by lookup_device
    if ((st = check_common(c, P)) != OVS_OK) return st;
    const bool kad_exh = !chord && P.routingType == 3;
    const bool kad_rec = !chord && (P.routingType == 1 || P.routingType == 2 || P.routingType == 4);
    if (P.routingType != 0 && !kad_exh && !kad_rec)
        return fail(c, OVS_ENOTSUP, "LookupCall is implemented for routingType = iterative (Kademlia: also recursive and "
                                    "exhaustive-iterative)");
    if (kad_exh && c->kad.general)
        return fail(c, OVS_ENOTSUP, "CSR (b > 1 / nr128 / nkademlia) tables: LookupCalls with routingType = iterative");
    if (kad_exh && ns > P.lookupRedundantNodes)
        return fail(c, OVS_EINVAL, "With EXHAUSTIVE_ITERATIVE_ROUTING numRedundantNodes must be >= numSiblings!");
    HIPCHK(c, hipSetDevice(c->device));
    *ns_out = ns;
    if (chord) {
        if ((st = check_chord_route(c, P)) != OVS_OK) return st;
        if (c->ideal && (c->shard_lo != 0 || c->shard_hi != c->n))
            return fail(c, OVS_ESTATE, "context holds one arc of a sharded ring: LookupCall needs the whole ring");
        if (!c->ideal && P.hopCountMax < 1)
            return fail(c, OVS_ENOTSUP, "explicit Chord tables need hopCountMax >= 1 (the hop list is the visited set)");
        return ensure_nodes(c, s);
    }
    if (c->kad.lo != 0 || c->kad.hi != c->n)
        return fail(c, OVS_ESTATE, "context holds one arc of a sharded network: LookupCall needs the whole network");
    return OVS_OK;
}

ovs_status lookup_device(ovs_ctx* c, const ovs_params& P0, int32_t ns, const K160* dk, const uint32_t* ds, uint64_t n,
                         ovs_route_out* dout, uint32_t* dsib, hipStream_t s)
{
    const bool chord = c->overlay == OVS_OVERLAY_CHORD;
    ovs_params P = P0;
    P.numSiblings = ns;
    const bool kad_exh = !chord && P.routingType == 3;
    const bool kad_rec = !chord && (P.routingType == 1 || P.routingType == 2 || P.routingType == 4);
    const int nslots = ns ? ns : 1;      // an exact-key lookup keeps a one-slot sibling vector (IterativeLookup.cc:149)
    DelayConsts DC = delay_consts(P);
    DC.lookupCall = 1;
    if (chord && c->ideal) DC.msgRespSib = ring_sibling_response_ns(DC, P, c->n, ns);
    CachedBuf::Lease vis;
    uint32_t* dhop = nullptr;
    // Chord exact-key lookups replay the one-way chain recorded one hop beyond hopCountMax
    const bool chord_exact = chord && ns == 0;
    const int H = chord_exact ? P.hopCountMax + 1 : P.hopCountMax > 0 ? P.hopCountMax : 1;
    // visited check (explicit tables; exhaustive lookups; source routing: the call's route, reversed by the response)
    const bool need_hop = (chord && !c->ideal) || kad_exh || chord_exact || (kad_rec && P.routingType == 4);
    if (need_hop) {
        // internal (a LookupCall records no hop sequence): the context's cached buffer
        vis = c->kvis.acquire(sizeof(uint32_t) * n * H, s);
        if (!vis) return lease_fail(c, "kvis", vis);
        dhop = reinterpret_cast<uint32_t*>(vis.data());
        HIPCHK(c, hipMemsetAsync(dhop, 0xFF, sizeof(uint32_t) * n * H, s));
    }
    hipError_t e;
    if (chord_exact) {
        // the chain: a one-way route (numSiblings 1, no LookupCall sizes) without timeouts
        DelayConsts DR = delay_consts(P);
        DR.rpcTimeout = DR.lookupTimeout = INT64_MAX / 4;
        LookupConsts LR{H, 1, P.lookupRedundantNodes, 0};
        e = launch_chord_route(chord_view(c), c->ideal, DR, LR, dk, ds, n, dout, dhop, c->num_cu, s);
        if (e == hipSuccess)
            e = launch_chord_exact_finish(chord_view(c), delay_consts(P), P.hopCountMax, dk, ds, dhop, H, dout, n, s);
    } else if (chord) {
        LookupConsts LC{P.hopCountMax, ns, P.lookupRedundantNodes, 0};
        const DynSlots::Lease dyn = dyn_acquire(c, n, s);
        e = launch_chord_route(chord_view(c), c->ideal, DC, LC, dk, ds, n, dout, dhop, c->num_cu, s, nullptr, dyn.get());
    } else if (kad_exh) {
        // lookupRpc with EXHAUSTIVE_ITERATIVE_ROUTING: redundantNodes = lookupRedundantNodes, numSiblings = ns
        bool cap_err = false;
        e = kad_exhaustive(c->kad, c->xy, (uint32_t)c->n, P, delay_consts(P), P.lookupRedundantNodes, ns, false, dk, ds,
                           n, dout, dsib, dhop, nullptr, nullptr, c->num_cu, s, persist_dyn_enabled(), &cap_err, nullptr, false,
                           true /* a LookupCall records no hop sequence: the visited sets' first entries in LDS */);
        if (e == hipSuccess && cap_err) e = hipErrorNotSupported;
    } else if (kad_rec) {
        // RecursiveLookup (RecursiveLookup.cc:52-139): a routed FindNodeCall, the response back by UDP
        // (semi-recursive), routed to the source's key (full-recursive) or along the call's route
        // reversed (source-routing-recursive)
        e = kad_route_recursive(c->kad, c->xy, (uint32_t)c->n, P, delay_consts(P),
                                simtime_host(P.rpcKeyTimeout, P.simtimeRound), ns, dk, ds, n, dout,
                                P.routingType == 4 ? dhop : nullptr, dsib, s);
    } else if (c->kad.general) {
        e = kad_route_general(c->kad, c->xy, (uint32_t)c->n, P, DC, dk, ds, n, dout, nullptr, nullptr, s, dsib);
    } else {
        const DynSlots::Lease dyn = dyn_acquire(c, n, s);
        e = kad_route(c->kad, c->xy, (uint32_t)c->n, P, DC, dk, ds, n, dout, nullptr, nullptr, c->num_cu, s,
                      dsib, dyn.get());
    }
    if (e == hipSuccess && !kad_exh) e = launch_lookup_finish(chord_view(c), chord, c->ideal, nslots, dout, dsib, n, s);
    vis.release();      // dhop is ordered by the buffer's event: a device-pointer call stays asynchronous
    return e == hipSuccess ? OVS_OK : hip_fail(c, e, "lookup kernel");
}

}  // namespace ovs

extern "C" {

ovs_status ovs_route_batch(ovs_ctx* c, const ovs_key160* keys, const uint32_t* src, uint64_t n,
                           ovs_route_out* out, uint32_t* hop_seq, uint32_t* rpcs, uint32_t flags, void* stream)
{
    if (!c || (!keys && n) || (!src && n) || (!out && n)) return OVS_EINVAL;
    const bool dev = flags & OVS_DEVICE_PTRS;
    hipStream_t s = dev ? (hipStream_t)stream : c->stream;   // NULL = the default stream
    ovs_status st = route_check(c, c->P, s);
    if (st != OVS_OK) return st;
    if (n == 0) return OVS_OK;
    if ((st = check_sources(c, src, n, dev)) != OVS_OK) return st;
    const int H = c->P.hopCountMax > 0 ? c->P.hopCountMax : 1;
    CallFrame F(dev, s);
    const K160* dk = F.in(reinterpret_cast<const K160*>(keys), n);
    const uint32_t* ds = F.in(src, n);
    ovs_route_out* dout = F.out(out, n);
    uint32_t* dhop = hop_seq ? F.out(hop_seq, n * (uint64_t)H) : nullptr;
    uint32_t* drpc = rpcs ? F.out(rpcs, n) : nullptr;
    if (!F.ok()) return frame_fail(c, F);
    if ((st = route_device(c, c->P, F, dk, ds, n, dout, dhop, drpc, s)) != OVS_OK) return st;
    return F.finish() == hipSuccess ? OVS_OK : frame_fail(c, F);
}

ovs_status ovs_lookup_batch(ovs_ctx* c, const ovs_key160* keys, const uint32_t* src, uint64_t n, int32_t num_siblings,
                            ovs_lookup_out* out, uint32_t* siblings, uint32_t flags, void* stream)
{
    static_assert(sizeof(ovs_lookup_out) == sizeof(ovs_route_out), "lookup results are finished in place");
    if (!c || (n && (!keys || !src || !out || !siblings))) return OVS_EINVAL;
    const bool dev = flags & OVS_DEVICE_PTRS;
    hipStream_t s = dev ? (hipStream_t)stream : c->stream;
    int32_t ns = 0;
    ovs_status st = lookup_check(c, c->P, num_siblings, s, &ns);
    if (st != OVS_OK) return st;
    if (n == 0) return OVS_OK;
    if ((st = check_sources(c, src, n, dev)) != OVS_OK) return st;
    CallFrame F(dev, s);
    const K160* dk = F.in(reinterpret_cast<const K160*>(keys), n);
    const uint32_t* ds = F.in(src, n);
    ovs_route_out* dout = F.out(reinterpret_cast<ovs_route_out*>(out), n);
    uint32_t* dsib = F.out(siblings, n * (uint64_t)(ns ? ns : 1));
    if (!F.ok()) return frame_fail(c, F);
    if ((st = lookup_device(c, c->P, ns, dk, ds, n, dout, dsib, s)) != OVS_OK) return st;
    return F.finish() == hipSuccess ? OVS_OK : frame_fail(c, F);
}

ovs_status ovs_find_node_batch(ovs_ctx* c, const uint32_t* node, const ovs_key160* keys, uint64_t n,
                               int32_t numRedundantNodes, int32_t numSiblings, uint32_t* out_nodes,
                               uint32_t max_out, uint8_t* out_count, uint8_t* out_sibling, uint32_t flags,
                               void* stream)
{
    if (!c || (n && (!node || !keys || !out_nodes || !out_count || !out_sibling)) || max_out == 0) return OVS_EINVAL;
    if (!c->overlay) return fail(c, OVS_ESTATE, "no network loaded");
    ovs_status st = refuse_dedicated(c);
    if (st != OVS_OK) return st;
    if (numSiblings > (c->overlay == OVS_OVERLAY_CHORD ? c->P.successorListSize : c->P.s))
        return fail(c, OVS_EINVAL, "numSiblings too big!");
    if (numRedundantNodes < 1 || numRedundantNodes > 64) return fail(c, OVS_EINVAL, "numRedundantNodes out of range");
    if (c->overlay == OVS_OVERLAY_CHORD && c->P.extendedFingerTable && numRedundantNodes > 1)
        return fail(c, OVS_ENOTSUP, "extendedFingerTable: findNode answers of more than one node (finger candidate "
                                    "lists) are not implemented");
    if (numSiblings < 0 && (numSiblings != -1 || c->overlay != OVS_OVERLAY_KADEMLIA))
        return fail(c, OVS_ENOTSUP, "numSiblings -1 (an exhaustive-iterative call) is implemented for Kademlia");
    HIPCHK(c, hipSetDevice(c->device));
    const bool dev = flags & OVS_DEVICE_PTRS;
    hipStream_t s = dev ? (hipStream_t)stream : c->stream;   // NULL = the default stream
    if (n == 0) return OVS_OK;
    std::string err;
    if (!dev && check_node_indices(node, n, c->n, &err)) return fail(c, OVS_EINVAL, err);
    CallFrame F(dev, s);
    const uint32_t* dn = F.in(node, n);
    const K160* dk = F.in(reinterpret_cast<const K160*>(keys), n);
    uint32_t* dout = F.out(out_nodes, n * (uint64_t)max_out);
    uint8_t* dc = F.out(out_count, n);
    uint8_t* dsb = F.out(out_sibling, n);
    if (!F.ok()) return frame_fail(c, F);
    hipError_t e;
    if (c->overlay == OVS_OVERLAY_CHORD)
        e = launch_chord_find_node(chord_view(c), c->ideal, dn, dk, n, numRedundantNodes, numSiblings, dout, max_out,
                                   dc, dsb, s);
    else if (c->kad.general)
        e = kad_find_node_general(c->kad, (uint32_t)c->n, dn, dk, n, numRedundantNodes, numSiblings, dout, max_out, dc,
                                  dsb, s);
    else
        e = kad_find_node(c->kad, (uint32_t)c->n, c->P, dn, dk, n, numRedundantNodes, numSiblings, dout,
                          max_out, dc, dsb, s);
    if (e != hipSuccess) return hip_fail(c, e, "findNode kernel");
    return F.finish() == hipSuccess ? OVS_OK : frame_fail(c, F);
}

ovs_status ovs_delay_batch(ovs_ctx* c, const uint32_t* a, const uint32_t* b, const int32_t* bytes, uint64_t n,
                           int64_t* out_ns, uint32_t flags, void* stream)
{
    if (!c || (n && (!a || !b || !bytes || !out_ns))) return OVS_EINVAL;
    if (!c->overlay) return fail(c, OVS_ESTATE, "no network loaded");
    HIPCHK(c, hipSetDevice(c->device));
    const bool dev = flags & OVS_DEVICE_PTRS;
    hipStream_t s = dev ? (hipStream_t)stream : c->stream;   // NULL = the default stream
    if (n == 0) return OVS_OK;
    std::string err;
    if (!dev && (check_node_indices(a, n, c->n, &err) || check_node_indices(b, n, c->n, &err))) return fail(c, OVS_EINVAL, err);
    CallFrame F(dev, s);
    const uint32_t* da = F.in(a, n);
    const uint32_t* db = F.in(b, n);
    const int32_t* dbytes = F.in(bytes, n);
    int64_t* dout = F.out(out_ns, n);
    if (!F.ok()) return frame_fail(c, F);
    hipError_t e = launch_delay(c->xy, delay_consts(c->P), da, db, dbytes, n, dout, s);
    if (e != hipSuccess) return hip_fail(c, e, "delay kernel");
    return F.finish() == hipSuccess ? OVS_OK : frame_fail(c, F);
}

ovs_status ovs_koorde_find_node_batch(ovs_ctx* c, const uint32_t* node, const ovs_key160* keys, ovs_koorde_ext* ext,
                                      uint32_t* next, uint64_t n)
{
    static_assert(sizeof(ovs_koorde_ext) == sizeof(KExt), "ovs_koorde_ext mirrors KExt");
    if (!c || (n && (!node || !keys || !ext || !next))) return OVS_EINVAL;
    if (c->overlay != OVS_OVERLAY_KOORDE) return fail(c, OVS_ESTATE, "no Koorde network loaded");
    if (n == 0) return OVS_OK;
    HIPCHK(c, hipSetDevice(c->device));
    std::string err;
    if (check_node_indices(node, n, c->n, &err)) return fail(c, OVS_EINVAL, err);
    CallFrame F(false, c->stream);
    const uint32_t* dn = F.in(node, n);
    const K160* dk = F.in(reinterpret_cast<const K160*>(keys), n);
    KExt* de = F.inout(reinterpret_cast<KExt*>(ext), n);
    uint32_t* dnext = F.out(next, n);
    if (!F.ok()) return frame_fail(c, F);
    hipError_t e = koorde_find_node(c->koorde, c->recs, dn, dk, de, dnext, n, c->stream);
    if (e != hipSuccess) return hip_fail(c, e, "koorde findNode kernel");
    return F.finish() == hipSuccess ? OVS_OK : frame_fail(c, F);
}

ovs_status ovs_epichord_find_node_batch(ovs_ctx* c, const uint32_t* node, const ovs_key160* keys, const uint32_t* src,
                                        const int64_t* now_ns, uint64_t n, int32_t numRedundantNodes,
                                        uint32_t* out_nodes, int64_t* out_last_ns, uint32_t max_out, uint8_t* out_count,
                                        uint8_t* out_status, uint32_t flags, void* stream)
{
    if (!c || (n && (!node || !keys || !src || !now_ns || !out_nodes || !out_last_ns || !out_count || !out_status)))
        return OVS_EINVAL;
    if (c->overlay != OVS_OVERLAY_EPICHORD) return fail(c, OVS_ESTATE, "no EpiChord snapshot loaded");
    if (numRedundantNodes < 0 || numRedundantNodes > EPI_MAXR)
        return fail(c, OVS_EINVAL, "numRedundantNodes must be 0..32");
    if (max_out < 3 || max_out < (uint32_t)(1 + numRedundantNodes))
        return fail(c, OVS_EINVAL, "max_out must be >= max(3, 1 + numRedundantNodes)");
    HIPCHK(c, hipSetDevice(c->device));
    const bool dev = flags & OVS_DEVICE_PTRS;
    hipStream_t s = dev ? (hipStream_t)stream : c->stream;
    if (n == 0) return OVS_OK;
    if (!dev) {
        for (uint64_t i = 0; i < n; ++i)
            if (node[i] >= c->n || (src[i] != NONE && src[i] >= c->n))
                return fail(c, OVS_EINVAL, "node / source index out of range");
    }
    CallFrame F(dev, s);
    const uint32_t* dn = F.in(node, n);
    const K160* dk = F.in(reinterpret_cast<const K160*>(keys), n);
    const uint32_t* dsrc = F.in(src, n);
    const int64_t* dnow = F.in(now_ns, n);
    uint32_t* dout = F.out(out_nodes, n * max_out);
    int64_t* dlast = F.out(out_last_ns, n * max_out);
    uint8_t* dc = F.out(out_count, n);
    uint8_t* dst = F.out(out_status, n);
    if (!F.ok()) return frame_fail(c, F);
    const int64_t ttl = simtime_host(c->P.cacheTTL, c->P.simtimeRound);
    hipError_t e = epichord_find_node(c->epi, c->recs, dn, dk, dsrc, dnow, n, numRedundantNodes, ttl, dout, dlast,
                                      max_out, dc, dst, s);
    if (e != hipSuccess) return hip_fail(c, e, "EpiChord findNode kernel");
    return F.finish() == hipSuccess ? OVS_OK : frame_fail(c, F);
}

}  // extern "C"
