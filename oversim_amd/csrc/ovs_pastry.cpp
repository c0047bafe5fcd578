// ovs_pastry.cpp -- the Pastry entry points of the C ABI (include/ovs_kbr.h): the loaders, the export, the
// findNode batch, the semi-recursive route (pastry_route_device: the public calls', plain or under routeMsgAcks,
// and Scribe's publish leg) and the iterative lookup (pastry_lookup_check / pastry_lookup_device: the LookupCall
// batch, the one-way route under iterative routing and the DHT tier's lookup phase).  The generic calls refuse a
// Pastry context through refuse_dedicated (ovs_route.cpp); Scribe, the overlay broadcast and the DHT tier run on
// one (app_*.cpp).
#include <string>
#include <vector>

#include "ctx.hpp"
#include "kbr_rpc.hpp"

using namespace ovs;

namespace {

// what both loaders check between the frame's drop and the upload
ovs_status load_begin(ovs_ctx* c, const ovs_pastry_params* bp, const ovs_key160* ids, uint64_t n, const double* xy, bool dev)
{
    if (const char* why = pastry_shape_refusal(*bp)) return fail(c, OVS_ENOTSUP, why);
    if (n < 2) return fail(c, OVS_EINVAL, "Pastry needs at least 2 nodes");
    return upload_nodes(c, ids, n, xy, dev);
}

// Every FindNodeCall and FindNodeResponse of a Pastry lookup carries the PastryFindNodeExtData object:
// BasePastry::createLookup (BasePastry.cc:1212-1239) hands one to the lookup, createFindNodeCall copies it into
// each call (IterativeLookup.cc:385-388) -- the first from the lookup's own, the later ones from the response
// before (907-920) -- and findNodeRpc moves it from the call to the response (BaseOverlay.cc:1903-1907).
// PASTRYFINDNODEEXTDATA_L = NODEHANDLE_L + HOPCOUNT_L = 224 bits (PastryMessage.msg:35), 28 B.
DelayConsts pastry_iter_delay_consts(const ovs_params& P)
{
    DelayConsts d = delay_consts(P);     // measureAuthBlock is in respBase
    auto bw = [&](int32_t bytes) { return bw_host(P, bytes); };
    d.callBytes += 28;
    d.respBase += 28;
    d.msgCall = 2 * bw(d.callBytes) + d.access2;
    d.msgResp1 = 2 * bw(d.respBase + d.respPerNode) + d.access2;
    d.msgRespSib = d.msgResp1;
    d.bwCall = bw(d.callBytes);
    for (int i = 0; i <= 16; ++i) d.bwResp[i] = bw(d.respBase + d.respPerNode * i);
    return d;
}

// routes under routeMsgAcks: the constants beside DelayConsts (PastryAckConsts, pastry.hpp)
PastryAckConsts pastry_ack_consts(const ovs_params& P, const DelayConsts& DC)
{
    PastryAckConsts a{};
    a.bwAck = bw_host(P, (int32_t)pastry_nexthop_ack_bytes(P));
    a.msgAck = 2 * a.bwAck + DC.access2;
    a.msgCall = 2 * bw_host(P, (int32_t)pastry_nexthop_call_bytes(P)) + DC.access2;
    a.timeout = DC.rpcTimeout;
    return a;
}

// The one-way message on device pointers under the context's routeMsgAcks and routingType, after
// pastry_acked_refusal: dack may be nullptr; dhop as the plain calls take it.
ovs_status pastry_acked_device(ovs_ctx* c, const ovs_params& P, const K160* dk, const uint32_t* ds, uint64_t n, ovs_route_out* dout,
                               ovs_pastry_ack_out* dack, uint32_t* dhop, hipStream_t s)
{
    const bool acks = c->pastry_bp.routeMsgAcks != 0;
    if (P.routingType != 0) {
        const PastryAckConsts AC = pastry_ack_consts(P, delay_consts(P));
        return pastry_route_device(c, P, dk, ds, n, dout, dhop, s, acks ? &AC : nullptr, dack);
    }
    // the lookup is ovs_pastry_iterative_route_batch's; the final sendRouteMessage goes as one NextHopCall
    // (BaseOverlay.cc:1254-1257), which changes that message's length and adds its ack
    DelayConsts DC = pastry_iter_delay_consts(P);
    const PastryAckConsts AC = pastry_ack_consts(P, DC);
    if (acks) DC.msgRoute = AC.msgCall;
    const ovs_status st = pastry_lookup_device(c, P, 1, dk, ds, n, nullptr, nullptr, s, dout, dhop, nullptr, &DC);
    if (st != OVS_OK || !dack) return st;
    const hipError_t e =
        acks ? pastry_iter_acks(dout, ds, c->xy, (uint32_t)c->n, AC, P.simtimeRound, n, dack, s) : pastry_acks_none(n, dack, s);
    return e == hipSuccess ? OVS_OK : hip_fail(c, e, "pastry ack record kernel");
}

// The checks of a semi-recursive entry point before anything is staged, in the one order all of them keep: the
// arguments, the loaded overlay, check_common, the call's own refusal of the parameters (refusal(): its reason
// or nullptr), the device.
template <class Refusal>
ovs_status pastry_begin(ovs_ctx* c, bool args_ok, Refusal refusal)
{
    if (!c || !args_ok) return OVS_EINVAL;
    if (c->overlay != OVS_OVERLAY_PASTRY) return fail(c, OVS_ESTATE, "no Pastry network loaded");
    const ovs_status st = check_common(c, c->P);
    if (st != OVS_OK) return st;
    if (const char* why = refusal()) return fail(c, OVS_ENOTSUP, why);
    HIPCHK(c, hipSetDevice(c->device));
    return OVS_OK;
}

// What the batch entry points share after their checks: the pointer mode and stream, the empty batch, the sources'
// range, the frame with the staged keys and sources, and its finish.  A call returns st unless go is set.
struct PastryBatch {
    PastryBatch(ovs_ctx* c, const ovs_key160* keys, const uint32_t* src, uint64_t n, uint32_t flags, void* stream)
        : c(c), dev(flags & OVS_DEVICE_PTRS), s(dev ? (hipStream_t)stream : c->stream), F(dev, s)
    {
        if (n == 0 || (st = check_sources(c, src, n, dev)) != OVS_OK) return;
        dk = F.in(reinterpret_cast<const K160*>(keys), n);
        ds = F.in(src, n);
        go = true;
    }
    ovs_status finish() { return F.finish() == hipSuccess ? OVS_OK : frame_fail(c, F); }
    ovs_ctx* c;
    bool dev;
    hipStream_t s;
    CallFrame F;
    const K160* dk = nullptr;      // the staged keys and sources
    const uint32_t* ds = nullptr;
    ovs_status st = OVS_OK;        // what the call returns where go is false: an empty batch, a source out of range
    bool go = false;
};

// the two iterative entry points: lout + siblings (a LookupCall) or rout (the one-way route), on the two halves
// the DHT tier uses as well
ovs_status pastry_iter_call(ovs_ctx* c, const char* name, bool route, const ovs_key160* keys, const uint32_t* src, uint64_t n,
                            int32_t ns, ovs_route_out* rout, ovs_lookup_out* lout, uint32_t* siblings, uint32_t* hop_seq, uint32_t* rpcs,
                            uint32_t flags, void* stream)
{
    if (!c || (n && (!keys || !src || (route ? !rout : !lout || !siblings)))) return OVS_EINVAL;
    if (c->overlay != OVS_OVERLAY_PASTRY) return fail(c, OVS_ESTATE, "no Pastry network loaded");
    const ovs_params& P = c->P;
    ovs_status st = pastry_lookup_check(c, P, ns, &ns, route, name);
    if (st != OVS_OK) return st;
    PastryBatch B(c, keys, src, n, flags, stream);
    if (!B.go) return B.st;
    CallFrame& F = B.F;
    ovs_route_out* dro = rout ? F.out(rout, n) : nullptr;
    ovs_lookup_out* dlo = lout ? F.out(lout, n) : nullptr;
    uint32_t* dsib = siblings ? F.out(siblings, n * (uint64_t)ns) : nullptr;
    uint32_t* dhop = hop_seq ? F.out(hop_seq, n * (uint64_t)P.hopCountMax) : nullptr;
    uint32_t* drpc = rpcs ? F.out(rpcs, n) : nullptr;
    if (!F.ok()) return frame_fail(c, F);
    st = pastry_lookup_device(c, P, ns, B.dk, B.ds, n, dlo, dsib, B.s, dro, dhop, drpc);
    return st != OVS_OK ? st : B.finish();
}

}  // namespace

namespace ovs {

ovs_status pastry_lookup_check(ovs_ctx* c, const ovs_params& P, int32_t num_siblings, int32_t* ns, bool route, const char* name)
{
    if (const char* why = pastry_iterative_refusal(P, c->pastry_bp, route)) return fail(c, OVS_ENOTSUP, why);
    const ovs_status st = check_common(c, P);
    if (st != OVS_OK) return st;
    // getMaxNumSiblings (BasePastry.cc:1090-1093); lookupRpc turns a negative count into it (BaseOverlay.cc:1940-1944)
    const int maxsib = c->pastry.sh.L / 2;
    if (num_siblings < 0) num_siblings = maxsib;
    if (num_siblings == 0)
        return fail(c, OVS_ENOTSUP, std::string(name) + ": exact-key lookups (num_siblings = 0) are not implemented on Pastry");
    if (num_siblings > maxsib) return fail(c, OVS_EINVAL, "numSiblings too big! (num_siblings must be 1..numberOfLeaves/2 or -1)");
    HIPCHK(c, hipSetDevice(c->device));
    *ns = num_siblings;
    return OVS_OK;
}

ovs_status pastry_lookup_device(ovs_ctx* c, const ovs_params& P, int32_t ns, const K160* dk, const uint32_t* ds, uint64_t n,
                                ovs_lookup_out* dlook, uint32_t* dsib, hipStream_t s, ovs_route_out* drout, uint32_t* dhop,
                                uint32_t* drpc, const DelayConsts* DC)
{
    CachedBuf::Lease vis;
    const ovs_status st = visited_lists(c, &dhop, n, (uint64_t)P.hopCountMax, s, &vis);
    if (st != OVS_OK) return st;
    const DynSlots::Lease dyn = dyn_acquire(c, n, s);
    const hipError_t e = pastry_iter(c->pastry, DC ? *DC : pastry_iter_delay_consts(P), P.hopCountMax, ns, dk, ds, n, drout, dlook, dsib,
                                     dhop, drpc, c->num_cu, s, dyn.get());
    vis.release();
    return e == hipSuccess ? OVS_OK : hip_fail(c, e, "pastry iterative lookup kernel");
}

ovs_status pastry_route_device(ovs_ctx* c, const ovs_params& P, const K160* dk, const uint32_t* ds, uint64_t n, ovs_route_out* dout,
                               uint32_t* dhop, hipStream_t s, const PastryAckConsts* AC, ovs_pastry_ack_out* dack)
{
    const uint64_t H = (uint64_t)(P.hopCountMax > 1 ? P.hopCountMax : 1);
    if (dhop) HIPCHK(c, hipMemsetAsync(dhop, 0xFF, sizeof(uint32_t) * n * H, s));
    const DynSlots::Lease dyn = dyn_acquire(c, n, s);
    hipError_t e = pastry_route(c->pastry, delay_consts(P), AC, P.hopCountMax, P.recNumRedundantNodes, dk, ds, n, dout,
                                AC ? dack : nullptr, dhop, c->num_cu, s, dyn.get());
    if (e != hipSuccess) return hip_fail(c, e, AC ? "pastry acked route kernel" : "pastry route kernel");
    if (!AC && dack) e = pastry_acks_none(n, dack, s);
    return e == hipSuccess ? OVS_OK : hip_fail(c, e, "pastry ack record kernel");
}

}  // namespace ovs

extern "C" {

void ovs_pastry_params_default(ovs_pastry_params* p)
{
    if (!p) return;
    p->bitsPerDigit = 4;        // default.ini:226
    p->numberOfLeaves = 16;     // default.ini:227
    p->numberOfNeighbors = 0;   // default.ini:228
    p->optimizeLookup = 0;      // default.ini:234
    p->useRegularNextHop = 1;   // default.ini:236
    p->routeMsgAcks = 1;        // default.ini:245
}

int32_t ovs_pastry_num_rows(const ovs_ctx* c) { return c && c->overlay == OVS_OVERLAY_PASTRY ? c->pastry.rows : -1; }

ovs_status ovs_pastry_load(ovs_ctx* c, const ovs_pastry_params* bp, const ovs_key160* ids, uint64_t n, const double* xy,
                           uint32_t flags)
{
    if (!c || !bp || !ids || !xy) return OVS_EINVAL;
    // parameters outside the implemented ranges leave the loaded network as it is
    if (const char* why = pastry_shape_refusal(*bp)) return fail(c, OVS_ENOTSUP, why);
    LoadFrame L(c, OVS_OVERLAY_PASTRY, "Pastry");
    if (L.st) return L.st;
    const bool dev = flags & OVS_DEVICE_PTRS;
    if (ovs_status s = load_begin(c, bp, ids, n, xy, dev)) return s;
    const PastryShape sh = pastry_shape_of(*bp);
    if (n - 1 >= (uint64_t)sh.L) {
        const hipError_t e = pastry_build(c->recs, c->xy, (uint32_t)n, sh, c->pastry, c->stream);
        if (e != hipSuccess) return hip_fail(c, e, "pastry table build");
    } else {
        // at most numberOfLeaves nodes: the leaf sets are the reference's own merge, replayed here
        std::vector<K160> hid(n);
        HIPCHK(c, hipMemcpy(hid.data(), ids, sizeof(K160) * n, dev ? hipMemcpyDeviceToHost : hipMemcpyHostToHost));
        std::vector<uint32_t> leaf(n * (uint64_t)sh.L);
        for (uint32_t v = 0; v < (uint32_t)n; ++v) pastry_host_leaves(hid.data(), (uint32_t)n, sh.L, v, leaf.data() + (uint64_t)v * sh.L);
        int rows = 0;
        hipError_t e = pastry_rule_rows(c->recs, (uint32_t)n, sh.b, &rows, c->stream);
        if (e != hipSuccess) return hip_fail(c, e, "pastry row count");
        CallFrame F(false, c->stream);
        const uint32_t* dl = F.in(leaf.data(), leaf.size());
        if (!F.ok()) return frame_fail(c, F);
        e = pastry_build_explicit(c->recs, c->xy, (uint32_t)n, sh, rows, dl, nullptr, c->pastry, c->stream);
        if (e != hipSuccess) return hip_fail(c, e, "pastry table build");
        if (F.finish() != hipSuccess) return frame_fail(c, F);
    }
    c->pastry_bp = *bp;
    c->pastry_rule = true;
    return L.commit();
}

ovs_status ovs_pastry_load_tables(ovs_ctx* c, const ovs_pastry_params* bp, const ovs_key160* ids, uint64_t n, const double* xy,
                                  const uint32_t* leaf, const uint32_t* table, int32_t rows, uint32_t flags)
{
    if (!c || !bp || !ids || !xy || !leaf || !table) return OVS_EINVAL;
    if (flags & OVS_DEVICE_PTRS) return fail(c, OVS_ENOTSUP, "ovs_pastry_load_tables takes host buffers");
    if (const char* why = pastry_shape_refusal(*bp)) return fail(c, OVS_ENOTSUP, why);
    const PastryShape sh = pastry_shape_of(*bp);
    {
        // the tables are checked before anything is dropped or uploaded
        std::string err;
        if (n < 2 || n >= 0xFFFFFFFFull) return fail(c, OVS_EINVAL, "node count out of range");
        if (!pastry_validate_tables(reinterpret_cast<const K160*>(ids), n, sh, rows, leaf, table, &err))
            return fail(c, OVS_EINVAL, "Pastry tables: " + err);
    }
    LoadFrame L(c, OVS_OVERLAY_PASTRY, "Pastry");
    if (L.st) return L.st;
    if (ovs_status s = load_begin(c, bp, ids, n, xy, false)) return s;
    CallFrame F(false, c->stream);
    const uint32_t* dl = F.in(leaf, n * (uint64_t)sh.L);
    const uint32_t* dt = F.in(table, n * (uint64_t)rows * (uint64_t)sh.P());
    if (!F.ok()) return frame_fail(c, F);
    const hipError_t e = pastry_build_explicit(c->recs, c->xy, (uint32_t)n, sh, rows, dl, dt, c->pastry, c->stream);
    if (e != hipSuccess) return hip_fail(c, e, "pastry table upload");
    if (F.finish() != hipSuccess) return frame_fail(c, F);
    c->pastry_bp = *bp;
    c->pastry_rule = false;
    return L.commit();
}

ovs_status ovs_pastry_export(ovs_ctx* c, uint32_t* leaf, uint32_t* table)
{
    if (!c || !leaf || !table) return OVS_EINVAL;
    if (c->overlay != OVS_OVERLAY_PASTRY) return fail(c, OVS_ESTATE, "no Pastry network loaded");
    HIPCHK(c, hipSetDevice(c->device));
    const PastryTables& t = c->pastry;
    CallFrame F(false, c->stream);
    uint32_t* dl = F.out(leaf, c->n * (uint64_t)t.sh.L);
    uint32_t* dt = F.out(table, c->n * (uint64_t)t.rows * (uint64_t)t.sh.P());
    if (!F.ok()) return frame_fail(c, F);
    const hipError_t e = pastry_slot_nodes(t, dl, dt, c->stream);
    if (e != hipSuccess) return hip_fail(c, e, "pastry export");
    return F.finish() == hipSuccess ? OVS_OK : frame_fail(c, F);
}

ovs_status ovs_pastry_find_node_batch(ovs_ctx* c, const uint32_t* node, const ovs_key160* keys, uint64_t n,
                                      int32_t numRedundantNodes, int32_t numSiblings, uint32_t* out_nodes, uint32_t max_out,
                                      uint8_t* out_count, uint8_t* out_sibling, uint8_t* out_status)
{
    if (!c || max_out == 0 || (n && (!node || !keys || !out_nodes || !out_count || !out_sibling || !out_status))) return OVS_EINVAL;
    if (c->overlay != OVS_OVERLAY_PASTRY) return fail(c, OVS_ESTATE, "no Pastry network loaded");
    const PastryShape& sh = c->pastry.sh;
    // getMaxNumRedundantNodes / getMaxNumSiblings (BasePastry.cc:1090-1098, 1105-1110)
    if (numRedundantNodes < 1 || numRedundantNodes > sh.L)
        return fail(c, OVS_EINVAL, "numRedundantNodes must be 1..numberOfLeaves (getMaxNumRedundantNodes)");
    if (numSiblings < 0 || numSiblings > sh.L / 2)
        return fail(c, OVS_EINVAL, "numSiblings must be 0..numberOfLeaves/2 (getMaxNumSiblings)");
    if (n == 0) return OVS_OK;
    HIPCHK(c, hipSetDevice(c->device));
    for (uint64_t i = 0; i < n; ++i)
        if (node[i] >= c->n) return fail(c, OVS_EINVAL, "node index out of range");
    CallFrame F(false, c->stream);
    const uint32_t* dn = F.in(node, n);
    const K160* dk = F.in(reinterpret_cast<const K160*>(keys), n);
    uint32_t* dout = F.out(out_nodes, n * (uint64_t)max_out);
    uint8_t* dc = F.out(out_count, n);
    uint8_t* dsib = F.out(out_sibling, n);
    uint8_t* dst = F.out(out_status, n);
    if (!F.ok()) return frame_fail(c, F);
    const hipError_t e = pastry_find_node(c->pastry, dn, dk, n, numRedundantNodes, numSiblings, dout, max_out, dc, dsib, dst, c->stream);
    if (e != hipSuccess) return hip_fail(c, e, "pastry findNode kernel");
    return F.finish() == hipSuccess ? OVS_OK : frame_fail(c, F);
}

ovs_status ovs_pastry_route_batch(ovs_ctx* c, const ovs_key160* keys, const uint32_t* src, uint64_t n, ovs_route_out* out,
                                  uint32_t* hop_seq, uint32_t flags, void* stream)
{
    ovs_status st = pastry_begin(c, !n || (keys && src && out), [&] { return pastry_route_refusal(c->P, c->pastry_bp); });
    if (st != OVS_OK) return st;
    PastryBatch B(c, keys, src, n, flags, stream);
    if (!B.go) return B.st;
    const ovs_params& P = c->P;
    ovs_route_out* dout = B.F.out(out, n);
    uint32_t* dhop = hop_seq ? B.F.out(hop_seq, n * (uint64_t)(P.hopCountMax > 1 ? P.hopCountMax : 1)) : nullptr;
    if (!B.F.ok()) return frame_fail(c, B.F);
    st = pastry_route_device(c, P, B.dk, B.ds, n, dout, dhop, B.s);
    return st != OVS_OK ? st : B.finish();
}

ovs_status ovs_pastry_acked_route_batch(ovs_ctx* c, const ovs_key160* keys, const uint32_t* src, uint64_t n, ovs_route_out* out,
                                        ovs_pastry_ack_out* ack_out, uint32_t* hop_seq, uint32_t flags, void* stream)
{
    static_assert(sizeof(ovs_pastry_ack_out) == 16, "ovs_pastry_ack_out is 16 B");
    ovs_status st = pastry_begin(c, !n || (keys && src && out), [&] { return pastry_acked_refusal(c->P, c->pastry_bp, false); });
    if (st != OVS_OK) return st;
    PastryBatch B(c, keys, src, n, flags, stream);
    if (!B.go) return B.st;
    const ovs_params& P = c->P;
    const uint64_t H = P.routingType == 0 ? (uint64_t)P.hopCountMax : (uint64_t)(P.hopCountMax > 1 ? P.hopCountMax : 1);
    ovs_route_out* dout = B.F.out(out, n);
    ovs_pastry_ack_out* dack = ack_out ? B.F.out(ack_out, n) : nullptr;
    uint32_t* dhop = hop_seq ? B.F.out(hop_seq, n * H) : nullptr;
    if (!B.F.ok()) return frame_fail(c, B.F);
    st = pastry_acked_device(c, P, B.dk, B.ds, n, dout, dack, dhop, B.s);
    return st != OVS_OK ? st : B.finish();
}

// KBRTestApp's RPC test on Pastry (KBRTestApp.cc:172-189, 230-329): the call leg is the route above; the
// KbrTestResponse goes straight back (BaseOverlay.cc:1340-1341) behind the ack the responder has just sent,
// which k_rpc_finish adds as RpcConsts::respQueue; its timeout rule is ovs_rpc_batch's.
ovs_status ovs_pastry_rpc_batch(ovs_ctx* c, const ovs_key160* keys, const uint32_t* src, uint64_t n, ovs_rpc_out* out, uint32_t flags,
                                void* stream)
{
    ovs_status st = pastry_begin(c, !n || (keys && src && out), [&] { return pastry_acked_refusal(c->P, c->pastry_bp, true); });
    if (st != OVS_OK) return st;
    const ovs_params& P = c->P;
    if (!(P.rpcKeyTimeout >= 0)) return fail(c, OVS_EINVAL, "rpcKeyTimeout must be >= 0");
    PastryBatch B(c, keys, src, n, flags, stream);
    if (!B.go) return B.st;
    ovs_rpc_out* dout = B.F.out(out, n);
    if (!B.F.ok()) return frame_fail(c, B.F);
    CachedBuf::Lease buf = c->rpcb.acquire(sizeof(ovs_route_out) * n, B.s);
    if (!buf) return lease_fail(c, "RPC buffers", buf);
    ovs_route_out* droute = reinterpret_cast<ovs_route_out*>(buf.data());
    // the refusal leaves semi-recursive routing only: the route of pastry_acked_device, and its ack constants once
    const DelayConsts DC = delay_consts(P);
    const PastryAckConsts AC = pastry_ack_consts(P, DC);
    const bool acks = c->pastry_bp.routeMsgAcks != 0;
    if ((st = pastry_route_device(c, P, B.dk, B.ds, n, droute, nullptr, B.s, acks ? &AC : nullptr)) != OVS_OK) return st;
    RpcConsts RC{};
    RC.timeout = simtime_host(P.rpcKeyTimeout, P.simtimeRound);
    RC.respMsg = 2 * bw_host(P, (int32_t)pastry_rpc_response_bytes(P)) + DC.access2;
    RC.respQueue = acks ? AC.bwAck : 0;
    RC.round = P.simtimeRound;
    RC.full = 0;
    RC.nnodes = (uint32_t)c->n;
    const hipError_t e = launch_rpc_finish(droute, B.ds, c->recs, c->xy, RC, n, dout, nullptr, nullptr, c->num_cu, B.s);
    if (e != hipSuccess) return hip_fail(c, e, "RPC finish kernel");
    buf.release();
    return B.finish();
}

ovs_status ovs_pastry_lookup_batch(ovs_ctx* c, const ovs_key160* keys, const uint32_t* src, uint64_t n, int32_t num_siblings,
                                   ovs_lookup_out* out, uint32_t* siblings, uint32_t* hop_seq, uint32_t* rpcs, uint32_t flags,
                                   void* stream)
{
    return pastry_iter_call(c, "ovs_pastry_lookup_batch", false, keys, src, n, num_siblings, nullptr, out, siblings, hop_seq, rpcs, flags,
                            stream);
}

ovs_status ovs_pastry_iterative_route_batch(ovs_ctx* c, const ovs_key160* keys, const uint32_t* src, uint64_t n, ovs_route_out* out,
                                            uint32_t* hop_seq, uint32_t flags, void* stream)
{
    return pastry_iter_call(c, "ovs_pastry_iterative_route_batch", true, keys, src, n, 1, out, nullptr, nullptr, hop_seq,
                            nullptr, flags, stream);
}

}  // extern "C"
