// ovs_broose.cpp -- the Broose entry points of the C ABI (include/ovs_kbr.h): the loaders, the export, the
// findNode batch and the one-way route.  ovs_route_batch keeps its signature: the per-lookup direction
// flags come through the sibling entry point ovs_broose_route_batch, and route_check / lookup_check
// refuse a Broose context, so every application tier does.
#include <string>
#include <vector>

#include "ctx.hpp"

using namespace ovs;

namespace {

BrooseShape shape_of(const ovs_broose_params& bp)
{
    BrooseShape sh;
    sh.k = bp.bucketSize; sh.kr = bp.rBucketSize; sh.userDist = bp.userDist; sh.sb = bp.shiftingBits;
    return sh;
}

// bits -> bytes as cPacket::getByteLength does, plus UDP/IP
int32_t packet_bytes(int32_t bits) { return (bits + 7) / 8 + 28; }

// Every Broose FindNodeCall and FindNodeResponse of a lookup carries the extension object: the source's
// local findNode creates it unless the source is a sibling (Broose.cc:623-669), createFindNodeCall
// copies it into each call (IterativeLookup.cc:385-388) and findNodeRpc moves it from the call to the
// response (BaseOverlay.cc:1903-1907).  BROOSEFINDNODEEXTMESSAGE_L = KEY_L + STEP_L + RIGHTSHIFTING_L +
// NODEHANDLE_L = 377 bits (BrooseMessage.msg:33-40) is no whole number of bytes: lengths add in bits.
DelayConsts broose_delay_consts(const ovs_params& P)
{
    DelayConsts d = delay_consts(P);
    auto bw = [&](int32_t bytes) { return bw_host(P, bytes); };
    const int32_t ext = 160 + 8 + 1 + 208;
    d.callBytes = packet_bytes(440 + ext);                                         // FINDNODECALL_L
    const int32_t resp1 = packet_bytes(264 + 208 + ext + (P.measureAuthBlock ? 800 : 0));   // FINDNODERESPONSE_L, one NodeHandle
    d.msgCall = 2 * bw(d.callBytes) + d.access2;
    d.msgResp1 = 2 * bw(resp1) + d.access2;
    d.msgRespSib = d.msgResp1;
    d.bwCall = bw(d.callBytes);
    return d;
}

// what both loaders check between the frame's drop and the upload; the frame (ctx.hpp) does the rest
ovs_status load_begin(ovs_ctx* c, const ovs_broose_params* bp, const ovs_key160* ids, uint64_t n, const double* xy, bool dev,
                      BrooseShape* sh)
{
    *sh = shape_of(*bp);
    std::string err;
    if (!broose_shape_ok(*sh, &err)) return fail(c, OVS_ENOTSUP, "Broose: " + err);
    if (n < 2) return fail(c, OVS_EINVAL, "Broose needs at least 2 nodes");
    if (n * (uint64_t)sh->stride() >= 0xFFFFFFFFull * 16) return fail(c, OVS_EINVAL, "too many nodes for the bucket rows");
    return upload_nodes(c, ids, n, xy, dev);
}

}  // namespace

extern "C" {

void ovs_broose_params_default(ovs_broose_params* p)
{
    if (!p) return;
    p->bucketSize = 8;      // default.ini:295
    p->rBucketSize = 8;     // default.ini:296
    p->userDist = 0;        // default.ini:297
    p->shiftingBits = 2;    // default.ini:298
}

int32_t ovs_broose_num_rows(const ovs_broose_params* bp)
{
    std::string err;
    if (!bp || !broose_shape_ok(shape_of(*bp), &err)) return -1;
    return shape_of(*bp).nrows();
}

int32_t ovs_broose_row_cap(const ovs_broose_params* bp, int32_t row)
{
    std::string err;
    if (!bp || !broose_shape_ok(shape_of(*bp), &err) || row < 0 || row >= shape_of(*bp).nrows()) return -1;
    return shape_of(*bp).cap(row);
}

ovs_status ovs_broose_load(ovs_ctx* c, const ovs_broose_params* bp, const ovs_key160* ids, uint64_t n, const double* xy,
                           uint32_t flags)
{
    if (!c || !bp || !ids || !xy) return OVS_EINVAL;
    {
        // a shape outside the implemented ranges is refused before the frame drops the loaded network
        std::string err;
        if (!broose_shape_ok(shape_of(*bp), &err)) return fail(c, OVS_ENOTSUP, "Broose: " + err);
    }
    LoadFrame L(c, OVS_OVERLAY_BROOSE, "Broose");
    if (L.st) return L.st;
    BrooseShape sh;
    if (ovs_status s = load_begin(c, bp, ids, n, xy, flags & OVS_DEVICE_PTRS, &sh)) return s;
    const hipError_t e = broose_build(c->recs, c->xy, (uint32_t)n, sh, c->broose, c->stream);
    if (e != hipSuccess) return hip_fail(c, e, "broose snapshot build");
    return L.commit();
}

ovs_status ovs_broose_load_tables(ovs_ctx* c, const ovs_broose_params* bp, const ovs_key160* ids, uint64_t n, const double* xy,
                                  const uint64_t* row_off, const uint32_t* row_nodes, uint32_t flags)
{
    if (!c || !bp || !ids || !xy || !row_off) return OVS_EINVAL;
    if (flags & OVS_DEVICE_PTRS) return fail(c, OVS_ENOTSUP, "ovs_broose_load_tables takes host buffers");
    {
        // the tables are checked before anything is dropped or uploaded
        std::string err;
        const BrooseShape sh = shape_of(*bp);
        if (!broose_shape_ok(sh, &err)) return fail(c, OVS_ENOTSUP, "Broose: " + err);
        if (n < 2 || n >= 0xFFFFFFFFull) return fail(c, OVS_EINVAL, "node count out of range");
        const uint64_t total = row_off[n * (uint64_t)sh.nrows()];
        if (total && !row_nodes) return OVS_EINVAL;
        if (!broose_validate_tables(reinterpret_cast<const K160*>(ids), n, sh, row_off, row_nodes, &err))
            return fail(c, OVS_EINVAL, "Broose tables: " + err);
    }
    LoadFrame L(c, OVS_OVERLAY_BROOSE, "Broose");
    if (L.st) return L.st;
    BrooseShape sh;
    if (ovs_status s = load_begin(c, bp, ids, n, xy, false, &sh)) return s;
    const uint64_t nr = n * (uint64_t)sh.nrows(), total = row_off[nr];
    CallFrame F(false, c->stream);
    const uint64_t* doff = F.in(row_off, nr + 1);
    const uint32_t* dn = F.in(row_nodes, total);
    if (!F.ok()) return frame_fail(c, F);
    const hipError_t e = broose_build_from_csr(c->recs, c->xy, (uint32_t)n, sh, doff, dn, c->broose, c->stream);
    if (e != hipSuccess) return hip_fail(c, e, "broose table upload");
    if (F.finish() != hipSuccess) return frame_fail(c, F);
    return L.commit();
}

ovs_status ovs_broose_export(ovs_ctx* c, uint64_t* row_off, uint32_t* row_nodes, uint64_t cap, uint64_t* total)
{
    if (!c || !row_off || !total) return OVS_EINVAL;
    if (c->overlay != OVS_OVERLAY_BROOSE) return fail(c, OVS_ESTATE, "no Broose network loaded");
    HIPCHK(c, hipSetDevice(c->device));
    const BrooseShape& sh = c->broose.sh;
    const uint64_t slots = c->n * (uint64_t)sh.stride();
    std::vector<uint32_t> h(slots);
    CallFrame F(false, c->stream);
    uint32_t* d = F.out(h.data(), slots);
    if (!F.ok()) return frame_fail(c, F);
    const hipError_t e = broose_row_nodes(c->broose, d, c->stream);
    if (e != hipSuccess) return hip_fail(c, e, "broose export");
    if (F.finish() != hipSuccess) return frame_fail(c, F);
    uint64_t t = 0, g = 0;
    row_off[0] = 0;
    for (uint64_t v = 0; v < c->n; ++v)
        for (int r = 0; r < sh.nrows(); ++r) {
            const uint32_t* row = h.data() + v * sh.stride() + sh.at(r);
            for (int j = 0; j < sh.cap(r) && row[j] != NONE; ++j, ++t)
                if (row_nodes && t < cap) row_nodes[t] = row[j];
            row_off[++g] = t;
        }
    *total = t;
    return OVS_OK;
}

ovs_status ovs_broose_find_node_batch(ovs_ctx* c, const uint32_t* node, const ovs_key160* keys, ovs_broose_ext* ext,
                                      const uint8_t* right, uint64_t n, int32_t numRedundantNodes, int32_t numSiblings,
                                      uint32_t* out_nodes, uint32_t max_out, uint8_t* out_count, uint8_t* out_sibling,
                                      uint8_t* out_status)
{
    static_assert(sizeof(ovs_broose_ext) == sizeof(BExt), "ovs_broose_ext mirrors BExt");
    if (!c || max_out == 0 || (n && (!node || !keys || !ext || !right || !out_nodes || !out_count || !out_sibling || !out_status)))
        return OVS_EINVAL;
    if (c->overlay != OVS_OVERLAY_BROOSE) return fail(c, OVS_ESTATE, "no Broose network loaded");
    const BrooseShape& sh = c->broose.sh;
    // isSiblingFor: numSiblings > getMaxNumSiblings() = bucketSize is an error (Broose.cc:836-838, 346-349)
    if (numSiblings > sh.k) return fail(c, OVS_EINVAL, "numSiblings too big!");
    if (numSiblings < -1) return fail(c, OVS_EINVAL, "numSiblings must be >= -1");
    if (numRedundantNodes < 1 || numRedundantNodes > sh.k)
        return fail(c, OVS_EINVAL, "numRedundantNodes must be 1..bucketSize (getMaxNumRedundantNodes)");
    if (n == 0) return OVS_OK;
    HIPCHK(c, hipSetDevice(c->device));
    for (uint64_t i = 0; i < n; ++i) {
        if (node[i] >= c->n) return fail(c, OVS_EINVAL, "node index out of range");
        // an extension's step moves in multiples of shiftingBits towards 0 from at most 160 away
        if (ext[i].has_ext && (ext[i].step % sh.sb != 0 || ext[i].step > 160 || ext[i].step < -160 ||
                               (ext[i].right_shifting ? ext[i].step < 0 : ext[i].step > 0)))
            return fail(c, OVS_EINVAL, "extension " + std::to_string(i) + ": step is no state a Broose lookup reaches");
    }
    CallFrame F(false, c->stream);
    const uint32_t* dn = F.in(node, n);
    const K160* dk = F.in(reinterpret_cast<const K160*>(keys), n);
    BExt* de = F.inout(reinterpret_cast<BExt*>(ext), n);
    const uint8_t* dr = F.in(right, n);
    uint32_t* dout = F.out(out_nodes, n * (uint64_t)max_out);
    uint8_t* dc = F.out(out_count, n);
    uint8_t* dsib = F.out(out_sibling, n);
    uint8_t* dst = F.out(out_status, n);
    if (!F.ok()) return frame_fail(c, F);
    const hipError_t e = broose_find_node(c->broose, dn, dk, de, dr, n, numRedundantNodes, numSiblings, dout, max_out, dc, dsib,
                                          dst, c->stream);
    if (e != hipSuccess) return hip_fail(c, e, "broose findNode kernel");
    return F.finish() == hipSuccess ? OVS_OK : frame_fail(c, F);
}

ovs_status ovs_broose_route_batch(ovs_ctx* c, const ovs_key160* keys, const uint32_t* src, const uint8_t* right, uint64_t n,
                                  ovs_route_out* out, uint32_t* hop_seq, uint32_t* rpcs, uint32_t flags, void* stream)
{
    if (!c || (n && (!keys || !src || !right || !out))) return OVS_EINVAL;
    if (c->overlay != OVS_OVERLAY_BROOSE) return fail(c, OVS_ESTATE, "no Broose network loaded");
    const ovs_params& P = c->P;
    ovs_status st = check_common(c, P);
    if (st != OVS_OK) return st;
    if (P.routingType != 0) return fail(c, OVS_ENOTSUP, "Broose routing is implemented for routingType = iterative");
    // the hop list (hopCountMax entries) is the visitOnlyOnce list: no hop limit leaves it without a size
    if (P.hopCountMax < 1) return fail(c, OVS_ENOTSUP, "Broose lookups need hopCountMax >= 1");
    if (P.lookupRedundantNodes != 1 || P.lookupParallelRpcs != 1 || P.lookupMerge || P.numSiblings != 1 || !P.lookupVisitOnlyOnce)
        return fail(c, OVS_ENOTSUP, "Broose route kernel implements lookupRedundantNodes=1, lookupParallelRpcs=1, merge off, "
                                    "visitOnlyOnce, numSiblings=1 (the Broose defaults)");
    HIPCHK(c, hipSetDevice(c->device));
    const bool dev = flags & OVS_DEVICE_PTRS;
    hipStream_t s = dev ? (hipStream_t)stream : c->stream;
    if (n == 0) return OVS_OK;
    if ((st = check_sources(c, src, n, dev)) != OVS_OK) return st;
    const uint64_t H = (uint64_t)P.hopCountMax;
    CallFrame F(dev, s);
    const K160* dk = F.in(reinterpret_cast<const K160*>(keys), n);
    const uint32_t* ds = F.in(src, n);
    const uint8_t* dr = F.in(right, n);
    ovs_route_out* dout = F.out(out, n);
    uint32_t* dhop = hop_seq ? F.out(hop_seq, n * H) : nullptr;
    uint32_t* drpc = rpcs ? F.out(rpcs, n) : nullptr;
    if (!F.ok()) return frame_fail(c, F);
    CachedBuf::Lease vis;
    if ((st = visited_lists(c, &dhop, n, H, s, &vis)) != OVS_OK) return st;
    const DynSlots::Lease dyn = dyn_acquire(c, n, s);
    const hipError_t e = broose_route(c->broose, broose_delay_consts(P), P.hopCountMax, dk, ds, dr, n, dout, dhop, drpc, c->num_cu, s,
                                      dyn.get());
    vis.release();
    if (e != hipSuccess) return hip_fail(c, e, "broose route kernel");
    return F.finish() == hipSuccess ? OVS_OK : frame_fail(c, F);
}

}  // extern "C"
