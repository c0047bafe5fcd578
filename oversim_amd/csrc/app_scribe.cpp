// app_scribe.cpp -- Scribe (scribe.hip) on converged Chord rings and converged Pastry tables: the forest of
// group trees and the multicasts down them.  Joins under iterative routing and every publish are one-way
// routes (route_device; pastry_route_device on Pastry); scribe_check holds the route's refusals for such a
// network, so they come first.  The two overlays differ in the level kernel and the publish route only.
#include <algorithm>
#include <cstring>

#include "ctx.hpp"

using namespace ovs;

namespace {

// the tier's refusals and, last, the route's (check_common, check_chord_route): on a whole converged
// ring route_check has no others
ovs_status scribe_check(ovs_ctx* c)
{
    if (!c->overlay) return fail(c, OVS_ESTATE, "no network loaded");
    if (c->overlay == OVS_OVERLAY_KADEMLIA) return fail(c, OVS_ENOTSUP, "Scribe is implemented for Chord rings, not Kademlia");
    if (c->overlay == OVS_OVERLAY_KOORDE) return fail(c, OVS_ENOTSUP, "Scribe is implemented for Chord rings, not Koorde");
    if (c->overlay == OVS_OVERLAY_EPICHORD) return fail(c, OVS_ENOTSUP, "Scribe is implemented for Chord rings, not EpiChord");
    if (c->overlay == OVS_OVERLAY_PASTRY) {
        // the reference's own Scribe configuration; the route's refusals are ovs_pastry_route_batch's, in its order
        if (!c->pastry_rule)
            return fail(c, OVS_ENOTSUP, "Scribe on explicit tables (ovs_pastry_load_tables): parent chains there can close "
                                        "into cycles that hold no root (converged tables, ovs_pastry_load, only)");
        ovs_status st = check_common(c, c->P);
        if (st != OVS_OK) return st;
        if (const char* why = pastry_route_refusal(c->P, c->pastry_bp)) return fail(c, OVS_ENOTSUP, why);
        return OVS_OK;
    }
    if (c->overlay != OVS_OVERLAY_CHORD) return fail(c, OVS_ENOTSUP, "Scribe is implemented for Chord rings and Pastry");
    if (!c->ideal)
        return fail(c, OVS_ENOTSUP, "Scribe on explicit tables: the next hop there depends on more than (node, key), so the "
                                    "tree depends on the order of the joins (converged rings only)");
    if (c->shard_lo != 0 || c->shard_hi != c->n)
        return fail(c, OVS_ENOTSUP, "Scribe on one arc of a sharded ring (a shard context) is not implemented");
    if (c->P.routingType == 2)
        return fail(c, OVS_ENOTSUP, "Scribe under full-recursive routing: the responses are routed back through forward(), "
                                    "which is not implemented");
    if (c->P.routingType == 4)
        return fail(c, OVS_ENOTSUP, "Scribe under source-routing-recursive routing is not implemented");
    if (c->P.routingType != 0 && c->P.routingType != 1)
        return fail(c, OVS_ENOTSUP, "Scribe is implemented for routingType iterative and semi-recursive");
    ovs_status st = check_common(c, c->P);
    if (st != OVS_OK) return st;
    return check_chord_route(c, c->P);
}

// one allocation for a forest of T tree nodes and G groups
hipError_t scribe_alloc(ScribeForest& F, uint64_t T, uint64_t G)
{
    const uint64_t sz[9] = {8 * T, 4 * T, 4 * T, 4 * T, 4 * (T + 1), 4 * T, 4 * G, 4 * (G + 1), sizeof(K160) * G};
    uint64_t off[10] = {0};
    for (int i = 0; i < 9; ++i) off[i + 1] = off[i] + up256(sz[i] ? sz[i] : 1);
    hipError_t e = hipMalloc(&F.block, off[9]);
    if (e != hipSuccess) { F.block = nullptr; return e; }
    char* b = static_cast<char*>(F.block);
    F.key = reinterpret_cast<uint64_t*>(b + off[0]);
    F.parent = reinterpret_cast<uint32_t*>(b + off[1]);
    F.ptn = reinterpret_cast<uint32_t*>(b + off[2]);
    F.info = reinterpret_cast<uint32_t*>(b + off[3]);
    F.coff = reinterpret_cast<uint32_t*>(b + off[4]);
    F.cidx = reinterpret_cast<uint32_t*>(b + off[5]);
    F.root_tn = reinterpret_cast<uint32_t*>(b + off[6]);
    F.goff = reinterpret_cast<uint32_t*>(b + off[7]);
    F.gkeys = reinterpret_cast<K160*>(b + off[8]);
    F.T = T; F.G = G;
    return hipSuccess;
}

}  // namespace

extern "C" {

// The frontier loop: level k's items are q[lo, hi); its launch appends the parents nobody claimed
// before behind them and the queue length read back is the next hi.  A chain ends at the responsible
// node, which every hop approaches on a converged ring, so the loop ends on an empty frontier; n
// levels is the bound.  Everything is built beside the forest in place, which is replaced at the end.
ovs_status ovs_scribe_build(ovs_ctx* c, const ovs_key160* group_keys, uint64_t G, const uint32_t* member_group,
                            const uint32_t* member_node, uint64_t nm, uint64_t capacity, uint32_t flags, void* stream)
{
    static_assert(sizeof(ovs_scribe_node) == 16 && sizeof(ovs_scribe_msg_out) == 32 && sizeof(ovs_scribe_delivery) == 24,
                  "Scribe record sizes");
    if (!c || (G && !group_keys) || (nm && (!member_group || !member_node))) return OVS_EINVAL;
    ovs_status st = scribe_check(c);
    if (st != OVS_OK) return st;
    if (G >= 0x7FFFFFFFull || nm >= 0x7FFFFFFFull || capacity >= 0x7FFFFFFFull)
        return fail(c, OVS_EINVAL, "too many groups, memberships or tree nodes (31-bit indices)");
    const bool dev = flags & OVS_DEVICE_PTRS;
    if (!dev)
        for (uint64_t i = 0; i < nm; ++i)
            if (member_group[i] >= G || member_node[i] >= c->n)
                return fail(c, OVS_EINVAL, "membership " + std::to_string(i) + ": group or node out of range");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = dev ? (hipStream_t)stream : c->stream;
    st = ensure_nodes(c, s);
    if (st != OVS_OK) return st;
    const uint64_t cap = capacity ? capacity : 1;
    uint64_t hsize = 64;
    while (hsize < 2 * cap) hsize <<= 1;

    CallFrame F(dev, s);
    const K160* dgk = F.in(reinterpret_cast<const K160*>(group_keys), G);
    const uint32_t* dmg = F.in(member_group, nm);
    const uint32_t* dmn = F.in(member_node, nm);
    unsigned long long* tab = F.scratch<unsigned long long>(hsize);
    uint64_t* q = F.scratch<uint64_t>(cap);
    uint32_t* par = F.scratch<uint32_t>(cap);
    unsigned long long* ctl = F.scratch<unsigned long long>(2);
    if (!F.ok()) return frame_fail(c, F);
    HIPCHK(c, hipMemsetAsync(tab, 0xFF, sizeof(unsigned long long) * hsize, s));
    HIPCHK(c, hipMemsetAsync(par, 0xFF, sizeof(uint32_t) * cap, s));
    HIPCHK(c, hipMemsetAsync(ctl, 0, 2 * sizeof *ctl, s));
    unsigned long long h[2] = {0, 0};
    auto ctl_status = [&]() -> ovs_status {
        if (h[1] & SCRIBE_ERR_INPUT) return fail(c, OVS_EINVAL, "a membership's group or node is out of range");
        if ((h[1] & SCRIBE_ERR_OVERFLOW) || h[0] > capacity)
            return fail(c, OVS_ENOMEM, "the forest needs more than capacity = " + std::to_string(capacity) + " tree nodes");
        return OVS_OK;
    };
    HIPCHK(c, launch_scribe_init(dmg, dmn, nm, G, (uint32_t)c->n, tab, hsize - 1, q, capacity, ctl, s));
    HIPCHK(c, read_ctl(h, ctl, 2, s));
    if ((st = ctl_status()) != OVS_OK) return st;
    const uint64_t m0 = h[0];                   // the deduplicated memberships: q[0, m0)
    const ChordView V = chord_view(c);
    uint64_t lo = 0, hi = m0;
    if (c->P.routingType == 0 && m0) {
        // iterative: nobody forwards (BaseOverlay.cc:1434-1442), every join goes to the responsible node if
        // its lookup succeeds -- the route kernel's, whose status and responsible node are the parents
        K160* jk = F.scratch<K160>(m0);
        uint32_t* js = F.scratch<uint32_t>(m0);
        ovs_route_out* jr = F.scratch<ovs_route_out>(m0);
        if (!F.ok()) return frame_fail(c, F);
        HIPCHK(c, launch_scribe_route_in(dgk, q, m0, jk, js, s));
        st = route_device(c, c->P, F, jk, js, m0, jr, nullptr, nullptr, s);
        if (st != OVS_OK) return st;
        HIPCHK(c, launch_scribe_route_level(jr, q, par, m0, capacity, tab, hsize - 1, ctl, s));
        HIPCHK(c, read_ctl(h, ctl, 2, s));
        if ((st = ctl_status()) != OVS_OK) return st;
        lo = hi; hi = h[0];
    }
    // the hop limit acts on routed join messages only: under iterative routing the levels left are the
    // responsible nodes' joins through themselves, which a local lookup delivers without a hop check
    const int join_hcm = c->P.routingType == 0 ? 2 : c->P.hopCountMax;
    const bool pastry = c->overlay == OVS_OVERLAY_PASTRY;
    for (uint64_t level = 0; hi > lo && level <= c->n; ++level) {
        if (pastry)
            HIPCHK(c, launch_scribe_level_pastry(c->pastry, dgk, q, par, lo, hi, capacity, tab, hsize - 1, ctl, join_hcm,
                                                 c->P.recNumRedundantNodes, s));
        else
            HIPCHK(c, launch_scribe_level(V, dgk, q, par, lo, hi, capacity, tab, hsize - 1, ctl, join_hcm, s));
        HIPCHK(c, read_ctl(h, ctl, 2, s));
        if ((st = ctl_status()) != OVS_OK) return st;
        lo = hi; hi = h[0];
    }
    if (hi > lo) return fail(c, OVS_EDEVICE, "Scribe build: the joins did not end (network not converged?)");
    const uint64_t T = hi;

    ScribeForest NF;
    hipError_t e = scribe_alloc(NF, T, G);
    if (e != hipSuccess) return device_fail(c, e, "Scribe forest");
    auto drop = [&](ovs_status r) { hipFree(NF.block); return r; };
    void* work = nullptr;
    if ((e = hipMalloc(&work, scribe_finish_bytes(T))) != hipSuccess) return drop(device_fail(c, e, "Scribe sort buffers"));
    std::vector<uint32_t> goff(G + 1, 0), info(T);
    if (G) e = hipMemcpyAsync(NF.gkeys, dgk, sizeof(K160) * G, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = launch_scribe_finish(q, par, T, m0, NF, work, s);
    if (e == hipSuccess) e = hipMemcpyAsync(goff.data(), NF.goff, sizeof(uint32_t) * (G + 1), hipMemcpyDeviceToHost, s);
    uint32_t E = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&E, NF.coff + T, sizeof E, hipMemcpyDeviceToHost, s);
    std::vector<uint32_t> roots(G ? G : 1, NONE);
    if (e == hipSuccess && G) e = hipMemcpyAsync(roots.data(), NF.root_tn, sizeof(uint32_t) * G, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    hipFree(work);
    if (e != hipSuccess) return drop(hip_fail(c, e, "Scribe forest kernels"));
    if (F.finish() != hipSuccess) return drop(frame_fail(c, F));
    NF.E = E;
    NF.routingType = c->P.routingType;
    NF.hopCountMax = c->P.hopCountMax;
    for (uint64_t g = 0; g < G; ++g) {
        NF.roots += roots[g] != NONE;
        NF.max_tree = std::max<uint64_t>(NF.max_tree, goff[g + 1] - goff[g]);
    }
    if (c->scribe.block) hipFree(c->scribe.block);
    c->scribe = NF;
    return OVS_OK;
}

ovs_status ovs_scribe_clear(ovs_ctx* c)
{
    if (!c) return OVS_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    if (c->scribe.block) hipFree(c->scribe.block);
    c->scribe = ScribeForest{};
    return OVS_OK;
}

ovs_status ovs_scribe_count(ovs_ctx* c, uint64_t* nodes, uint64_t* edges, uint64_t* rooted)
{
    if (!c) return OVS_EINVAL;
    if (!c->scribe.block) return fail(c, OVS_ESTATE, "no Scribe forest (ovs_scribe_build)");
    if (nodes) *nodes = c->scribe.T;
    if (edges) *edges = c->scribe.E;
    if (rooted) *rooted = c->scribe.roots;
    return OVS_OK;
}

ovs_status ovs_scribe_export(ovs_ctx* c, ovs_scribe_node* out, uint32_t flags, void* stream)
{
    if (!c) return OVS_EINVAL;
    if (!c->scribe.block) return fail(c, OVS_ESTATE, "no Scribe forest (ovs_scribe_build)");
    if (!out && c->scribe.T) return OVS_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    const bool dev = flags & OVS_DEVICE_PTRS;
    hipStream_t s = dev ? (hipStream_t)stream : c->stream;
    CallFrame F(dev, s);
    ovs_scribe_node* d = F.out(out, c->scribe.T);
    if (!F.ok()) return frame_fail(c, F);
    HIPCHK(c, launch_scribe_export(c->scribe, d, s));
    if (F.finish() != hipSuccess) return frame_fail(c, F);
    return OVS_OK;
}

// The publish leg is the one-way route with the ScribePublishCall (and the data in it) in the
// KBRTestApp message's place; k_scribe_publish ends it, the level loop walks the child lists as the
// broadcast's does, k_scribe_collect sums up.
ovs_status ovs_scribe_multicast_batch(ovs_ctx* c, const uint32_t* msg_group, const uint32_t* msg_src, const uint8_t* msg_flags,
                                      uint64_t nm, int32_t payload_bytes, ovs_scribe_msg_out* out,
                                      ovs_scribe_delivery* deliveries, uint64_t deliv_cap, uint64_t* deliv_count,
                                      uint32_t flags, void* stream)
{
    if (!c || (nm && (!msg_group || !msg_src || !msg_flags || !out))) return OVS_EINVAL;
    ovs_status st = scribe_check(c);
    if (st != OVS_OK) return st;
    const ScribeForest& SF = c->scribe;
    if (!SF.block) return fail(c, OVS_ESTATE, "no Scribe forest (ovs_scribe_build)");
    if (SF.routingType != c->P.routingType || SF.hopCountMax != c->P.hopCountMax)
        return fail(c, OVS_ESTATE, "the Scribe forest was built under another routingType or hopCountMax: build it again");
    if (payload_bytes < 0 || payload_bytes > (1 << 24)) return fail(c, OVS_EINVAL, "payload_bytes must be 0..2^24");
    if (nm >= 0x7FFFFFFFull) return fail(c, OVS_EINVAL, "too many messages in one batch");
    const bool dev = flags & OVS_DEVICE_PTRS;
    if (!dev)
        for (uint64_t i = 0; i < nm; ++i)
            if (msg_group[i] >= SF.G || msg_src[i] >= c->n)
                return fail(c, OVS_EINVAL, "message " + std::to_string(i) + ": group or source out of range");
    if (deliv_count) *deliv_count = 0;
    if (nm == 0) return OVS_OK;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = dev ? (hipStream_t)stream : c->stream;
    st = ensure_nodes(c, s);
    if (st != OVS_OK) return st;

    // ScribePublishCall = BASECALL_L 256 bits (ScribeMessage.msg:38) around the ScribeDataMessage, KEY_L 160 +
    // 8 bits (:43), around the ALM payload: 53 B + payload.  Routed, it rides in a BaseAppDataMessage in a
    // BaseRouteMessage like the KBRTestApp message (route_bytes); to a known node, in the BaseAppDataMessage
    // alone (40 bits, BaseOverlay.cc:1340-1341).  ScribePublishResponse = BASECALL_L + 8 bits (:39: the macro
    // takes BASECALL_L, so measureAuthBlock adds nothing to it); a copy to a child = the ScribeDataMessage.
    const int32_t call_bytes = 53 + payload_bytes;
    auto bw = [&](int64_t bytes) { return simtime_host((double)(bytes * 8) / c->P.datarate, c->P.simtimeRound); };
    ScribeConsts SC{};
    SC.round = c->P.simtimeRound;
    SC.nnodes = (uint32_t)c->n;
    SC.access2 = 2 * simtime_host(c->P.accessDelay, c->P.simtimeRound);
    SC.bwData = bw(21 + payload_bytes + 5 + 28);
    SC.bwResp = bw(33 + 5 + 28);
    SC.msgDirect = 2 * bw(call_bytes + 5 + 28) + SC.access2;
    if (SC.bwResp >= (1ll << 32)) return fail(c, OVS_EINVAL, "datarate too low (a response takes over 4 s to serialise)");

    const uint64_t cap = std::max<uint64_t>(nm, nm * SF.max_tree);
    CallFrame F(dev, s);
    const uint32_t* dg = F.in(msg_group, nm);
    const uint32_t* ds = F.in(msg_src, nm);
    const uint8_t* df = F.in(msg_flags, nm);
    ovs_scribe_msg_out* dout = F.out(out, nm);
    ovs_scribe_delivery* dd = deliveries && deliv_cap ? F.out(deliveries, deliv_cap) : nullptr;
    K160* keys = F.scratch<K160>(nm);
    ovs_route_out* route = F.scratch<ovs_route_out>(nm);
    unsigned long long* ctl = F.scratch<unsigned long long>(4);
    if (!F.ok()) return frame_fail(c, F);
    const CachedBuf::Lease ql = c->scq.acquire(sizeof(ScribeItem) * cap, s);
    if (!ql) return lease_fail(c, "multicast queue", ql);
    ScribeItem* queue = reinterpret_cast<ScribeItem*>(ql.data());

    HIPCHK(c, hipMemsetAsync(ctl, 0, 4 * sizeof *ctl, s));
    HIPCHK(c, launch_scribe_msg_keys(SF, dg, ds, nm, (uint32_t)c->n, keys, ctl, s));
    unsigned long long h[4] = {0, 0, 0, 0};
    if (dev) {
        // device-pointer messages are checked on the device, before the route kernel reads their sources
        HIPCHK(c, read_ctl(h, ctl, 4, s));
        if (h[1] & SCRIBE_ERR_INPUT) return fail(c, OVS_EINVAL, "a message's group or source is out of range");
    }
    // the publish is routed under this call's message length: a copy of the parameters, the context's stay
    ovs_params PR = c->P;
    PR.testMsgSize = call_bytes;
    st = c->overlay == OVS_OVERLAY_PASTRY ? pastry_route_device(c, PR, keys, ds, nm, route, nullptr, s)
                                          : route_device(c, PR, F, keys, ds, nm, route, nullptr, nullptr, s);
    if (st != OVS_OK) return st;
    HIPCHK(c, launch_scribe_publish(SF, SC, c->xy, route, dg, ds, df, nm, dout, queue, s));
    h[0] = nm;
    HIPCHK(c, hipMemcpyAsync(ctl, h, sizeof(unsigned long long), hipMemcpyHostToDevice, s));
    uint64_t lo = 0, hi = nm;
    for (uint64_t level = 0; !h[1] && hi > lo && level <= SF.T; ++level) {
        HIPCHK(c, launch_scribe_down(SF, SC, c->xy, queue, lo, hi, cap, ctl, s));
        HIPCHK(c, read_ctl(h, ctl, 4, s));
        lo = hi;
        hi = std::min<uint64_t>(h[0], cap);
    }
    if (h[1]) return fail(c, OVS_EDEVICE, "multicast queue overflow");
    HIPCHK(c, launch_scribe_collect(SF, queue, hi, dout, dd, dd ? deliv_cap : 0, ctl + 2, s));
    HIPCHK(c, read_ctl(h, ctl, 4, s));
    if (dd) F.limit(dd, std::min<uint64_t>(h[2], deliv_cap));
    if (F.finish() != hipSuccess) return frame_fail(c, F);
    if (deliv_count) *deliv_count = h[2];
    return OVS_OK;
}

}  // extern "C"
