// ovs_ctx.cpp -- the context of the C ABI declared in include/ovs_kbr.h, and what every call shares.
//
// The context owns the device routing tables (sorted 24 B node records, fp64 coordinates, CSR finger rows /
// Kademlia buckets) and one HIP stream.  Host-pointer calls stage their arrays in per-call device copies
// (CallFrame, call_frame.hpp), run on the context's stream and are synchronous; OVS_DEVICE_PTRS calls launch
// asynchronously on the caller's stream.  No C++ exception crosses the boundary.  ctx.hpp is the map.
#include <algorithm>
#include <cmath>
#include <string>

#include "ctx.hpp"

using namespace ovs;

namespace ovs {

int ctx_device(const ovs_ctx* c) { return c->device; }

ovs_status fail(ovs_ctx* c, ovs_status s, const std::string& msg)
{
    if (c) c->err = msg;
    return s;
}

hipStream_t ctx_cohort_stream(ovs_ctx* c, int i)
{
    if (i < 0 || i >= 4) return nullptr;
    if (!c->cohort[i] && hipStreamCreateWithFlags(&c->cohort[i], hipStreamNonBlocking) != hipSuccess)
        c->cohort[i] = nullptr;
    return c->cohort[i];
}

void* ctx_route_scratch(ovs_ctx* c) { return c->route_scratch; }

void ctx_set_route_scratch(ovs_ctx* c, void* p, void (*release)(void*))
{
    c->route_scratch = p;
    c->route_scratch_release = release;
}

ovs_status hip_fail(ovs_ctx* c, hipError_t e, const char* where)
{
    return fail(c, OVS_EDEVICE, std::string(where) + ": " + hipGetErrorString(e));
}

void free_tables(ovs_ctx* c)
{
    void* ptrs[] = {c->recs, c->xy, c->fingers, c->pred, c->succ, c->nsucc, c->fres, c->nodes, c->win, c->ftop};
    for (void* p : ptrs)
        if (p) hipFree(p);
    c->nodes = nullptr; c->win = nullptr; c->nodes_ns = -1; c->ftop = nullptr; c->ftl = 0;
    c->recs = nullptr; c->xy = nullptr; c->fingers = nullptr; c->pred = nullptr;
    c->succ = nullptr; c->nsucc = nullptr; c->fres = nullptr;
    kad_free(c->kad);
    koorde_free(c->koorde);
    epichord_free(c->epi);
    broose_free(c->broose);
    pastry_free(c->pastry);
    for (CachedBuf* b : {&c->kvis, &c->ks, &c->bq, &c->rpcb, &c->dhtb, &c->scq}) b->free();
    if (c->dht.slots) hipFree(c->dht.slots);
    if (c->dht.hdr) hipFree(c->dht.hdr);
    c->dht = DhtStore{};
    if (c->scribe.block) hipFree(c->scribe.block);
    c->scribe = ScribeForest{};
    c->overlay = 0; c->n = 0; c->nfing = 0;
    c->bbox_ok = false;
    c->ch.clear();
    c->kh.clear();
}

void free_kad_shard(ovs_ctx* c)
{
    void* ptrs[] = {c->kst, c->kact, c->kqids, c->kres, c->kbad, c->kiota, c->klist[0], c->klist[1], c->knl,
                    c->kkeys, c->ksrc};
    for (void* p : ptrs)
        if (p) hipFree(p);
    c->kst = nullptr; c->kact = nullptr; c->kqids = nullptr; c->kres = nullptr; c->kbad = nullptr;
    c->kkeys = nullptr; c->ksrc = nullptr;
    c->kiota = nullptr; c->klist[0] = c->klist[1] = nullptr; c->knl = nullptr; c->kcur = 0;
    c->knlook = 0; c->kcap = 0; c->kalpha = 0;
}

LoadFrame::LoadFrame(ovs_ctx* c, int overlay, const char* name) : c(c), overlay(overlay)
{
    const hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) { st = hip_fail(c, e, "hipSetDevice(c->device)"); return; }
    live = true;
    free_tables(c);
    free_kad_shard(c);
    if (c->P.overlay != overlay) st = fail(c, OVS_ESTATE, std::string("params.overlay is not ") + name);
}

// a CallFrame's or a cached buffer's failure as the call's status
ovs_status device_fail(ovs_ctx* c, hipError_t e, const std::string& what)
{
    return fail(c, e == hipErrorOutOfMemory ? OVS_ENOMEM : OVS_EDEVICE, what + ": " + hipGetErrorString(e));
}

ovs_status frame_fail(ovs_ctx* c, const CallFrame& F) { return device_fail(c, F.error(), F.what()); }

ovs_status lease_fail(ovs_ctx* c, const char* name, const CachedBuf::Lease& L)
{
    return device_fail(c, L.error(), std::string(name) + " " + L.what());
}

// SimTime(double) on the host (identical IEEE double arithmetic to the device path)
int64_t simtime_host(double seconds, int round)
{
    const double x = seconds * 1e9;
    return round ? (int64_t)std::floor(x + 0.5) : (int64_t)x;
}

int64_t bw_host(const ovs_params& P, int32_t bytes)
{
    return simtime_host((double)((int64_t)bytes * 8) / P.datarate, P.simtimeRound);
}

int32_t route_bytes(const ovs_params& P)
{
    // BASEROUTE_L 424 bits + BASEAPPDATA_L 40 bits + KBRTestMessage payload + UDP/IP 28 B
    // (CommonMessages.msg:50-59, SimpleUDP.cc:291)
    return 58 + P.testMsgSize + 28;
}

DelayConsts delay_consts(const ovs_params& P)
{
    DelayConsts d{};
    d.round = P.simtimeRound;
    auto bw = [&](int32_t bytes) { return bw_host(P, bytes); };
    const int64_t acc = simtime_host(P.accessDelay, P.simtimeRound);
    d.access2 = 2 * acc;
    d.callBytes = 83;        // FINDNODECALL_L 440 bits + 28 B
    d.respBase = 61;         // FINDNODERESPONSE_L 264 bits + 28 B
    // measureAuthBlock: BASERESPONSE_L adds AUTHBLOCK_L = SIGNATURE_L + CERT_L + PUBKEY_L = 800 bits to
    // every response (CommonMessages.msg:45-47, 57, 73); calls and route messages are unchanged
    if (P.measureAuthBlock) d.respBase += 100;
    if (P.overlay == OVS_OVERLAY_KOORDE) {
        // every Koorde FindNodeCall / FindNodeResponse carries a KoordeFindNodeExtMessage,
        // KEY_L + STEP_L = 168 bits (ChordMessage.msg:33,55; IterativeLookup.cc:385-388,
        // BaseOverlay.cc:1903-1907)
        d.callBytes += 21;
        d.respBase += 21;
    }
    d.respPerNode = 26;      // NODEHANDLE_L 208 bits
    d.routeBytes = route_bytes(P);
    d.msgCall = 2 * bw(d.callBytes) + 2 * acc;
    d.msgResp1 = 2 * bw(d.respBase + d.respPerNode) + 2 * acc;
    d.msgRoute = 2 * bw(route_bytes(P)) + 2 * acc;
    d.rpcTimeout = simtime_host(P.rpcUdpTimeout, P.simtimeRound);
    d.lookupTimeout = simtime_host(P.lookupTimeout, P.simtimeRound);
    d.datarate = P.datarate;
    d.msgRespSib = d.msgResp1;
    d.lookupCall = 0;
    d.bwCall = bw(d.callBytes);
    d.bwRoute = bw(d.routeBytes);
    for (int i = 0; i <= 16; ++i) d.bwResp[i] = bw(d.respBase + d.respPerNode * i);
    return d;
}

int64_t ring_sibling_response_ns(const DelayConsts& DC, const ovs_params& P, uint64_t n, int ns)
{
    const int64_t nsucc = std::min<int64_t>(P.successorListSize, (int64_t)n - 1);
    const int nodes = (int)std::min<int64_t>(ns, 1 + nsucc);
    return 2 * simtime_host((double)((int64_t)(DC.respBase + DC.respPerNode * nodes) * 8) / P.datarate, P.simtimeRound) +
           DC.access2;
}

ovs_status check_common(ovs_ctx* c, const ovs_params& P)
{
    if (P.keyLength != 160) return fail(c, OVS_ENOTSUP, "keyLength != 160 not supported");
    if (P.routingType < 0 || P.routingType > 4)
        return fail(c, OVS_ENOTSUP, "routingType must be iterative, semi-recursive, full-recursive, exhaustive-iterative "
                                    "or source-routing-recursive");
    const bool rec = P.routingType == 1 || P.routingType == 2 || P.routingType == 4;
    if (P.routingType == 3 && P.overlay != OVS_OVERLAY_KADEMLIA)
        return fail(c, OVS_ENOTSUP, "exhaustive-iterative routing is implemented for Kademlia");
    if (P.routingType == 3 && P.numSiblings > P.lookupRedundantNodes)
        return fail(c, OVS_EINVAL, "With EXHAUSTIVE_ITERATIVE_ROUTING numRedundantNodes must be >= numSiblings!");
    if (rec && P.recNumRedundantNodes < 1)
        return fail(c, OVS_EINVAL, "recNumRedundantNodes must be >= 1");
    if (rec && P.overlay == OVS_OVERLAY_KADEMLIA &&
        (P.recNumRedundantNodes > 16 || P.lookupRedundantNodes > 16 || !(P.rpcKeyTimeout >= 0)))
        return fail(c, OVS_ENOTSUP, "recursive Kademlia implements recNumRedundantNodes, lookupRedundantNodes <= 16 "
                                    "and rpcKeyTimeout >= 0");
    if (P.extendedFingerTable && P.overlay != OVS_OVERLAY_CHORD)
        return fail(c, OVS_ENOTSUP, "extendedFingerTable is implemented for Chord");
    if (P.extendedFingerTable && (P.numFingerCandidates < 1 || P.numFingerCandidates > 64))
        return fail(c, OVS_EINVAL, "numFingerCandidates must be 1..64");
    if (P.lookupParallelPaths != 1) return fail(c, OVS_ENOTSUP, "lookupParallelPaths != 1 not supported");
    if (P.lookupVerifySiblings || P.lookupMajoritySiblings)
        return fail(c, OVS_ENOTSUP, "lookupVerifySiblings/lookupMajoritySiblings not supported");
    if (P.jitter != 0.0)
        return fail(c, OVS_ENOTSUP, "udp.jitter must be 0 (truncnormal jitter is not reproducible)");
    if (!P.useCoordinateBasedDelay) return fail(c, OVS_ENOTSUP, "useCoordinateBasedDelay = false not supported");
    if (P.numSiblings < 0 || P.numSiblings > 8) return fail(c, OVS_EINVAL, "numSiblings out of range");
    if (P.hopCountMax < 0 || P.hopCountMax > 255) return fail(c, OVS_EINVAL, "hopCountMax out of range");
    if (!(P.datarate > 0)) return fail(c, OVS_EINVAL, "datarate must be > 0");
    return OVS_OK;
}

}  // namespace ovs

extern "C" {

int ovs_abi_version(void) { return OVS_ABI_VERSION; }

ovs_status ovs_ctx_create(int hip_device, ovs_ctx** out)
{
    if (!out) return OVS_EINVAL;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return OVS_EDEVICE;
    if (hip_device < 0 || hip_device >= ndev) return OVS_EINVAL;
    ovs_ctx* c = new (std::nothrow) ovs_ctx();
    if (!c) return OVS_ENOMEM;
    c->device = hip_device;
    if (hipSetDevice(hip_device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return OVS_EDEVICE;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, hip_device) == hipSuccess) c->num_cu = prop.multiProcessorCount;
    if (c->num_cu <= 0) c->num_cu = 256;
    ovs_params_default(OVS_OVERLAY_CHORD, &c->P);
    *out = c;
    return OVS_OK;
}

void ovs_ctx_destroy(ovs_ctx* c)
{
    if (!c) return;
    hipSetDevice(c->device);
    // this context's own stream; work the caller queued on its streams (c->stage keys, which the
    // caller may already have destroyed) is ordered before the frees below by hipFree itself, so
    // destroy waits for no other context's or communicator's work
    if (c->stream) hipStreamSynchronize(c->stream);
    free_tables(c);
    free_kad_shard(c);
    kad_exhaustive_release(c->device);
    if (c->d_bounds) hipFree(c->d_bounds);
    for (CachedBuf* b : {&c->kvis, &c->ks, &c->bq, &c->scq, &c->rpcb, &c->dhtb}) b->destroy();
    c->dyn.destroy();
    if (c->route_scratch && c->route_scratch_release) c->route_scratch_release(c->route_scratch);
    for (auto& kv : c->stage) stage_free(kv.second);
    for (hipStream_t cs : c->cohort)
        if (cs) hipStreamDestroy(cs);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;
}

const char* ovs_last_error(const ovs_ctx* c) { return c ? c->err.c_str() : "null context"; }

ovs_status ovs_set_params(ovs_ctx* c, const ovs_params* p)
{
    if (!c || !p) return OVS_EINVAL;
    if (ovs_status s = check_common(c, *p)) return s;
    if (c->overlay && p->overlay != c->overlay) return fail(c, OVS_ESTATE, "overlay type differs from loaded network");
    if (c->overlay == OVS_OVERLAY_KADEMLIA &&
        (p->k != c->P.k || p->s != c->P.s || p->b != c->P.b || p->kadSeed != c->P.kadSeed ||
         p->bucketType != c->P.bucketType || p->extraNodesFinalBucket != c->P.extraNodesFinalBucket ||
         p->globalNodeLimit != c->P.globalNodeLimit))
        return fail(c, OVS_ESTATE, "k/s/b/kadSeed/bucketType are fixed once a Kademlia network is loaded");
    if (c->overlay == OVS_OVERLAY_KOORDE &&
        (p->successorListSize != c->P.successorListSize || p->shiftingBits != c->P.shiftingBits ||
         p->deBruijnListSize != c->P.deBruijnListSize || p->useOtherLookup != c->P.useOtherLookup ||
         p->useSucList != c->P.useSucList))
        return fail(c, OVS_ESTATE, "the Koorde ring parameters are fixed once a Koorde network is loaded");
    if (c->overlay == OVS_OVERLAY_EPICHORD && p->successorListSize != c->P.successorListSize)
        return fail(c, OVS_ESTATE, "successorListSize is fixed once an EpiChord snapshot is loaded");
    c->P = *p;
    return OVS_OK;
}

ovs_status ovs_get_params(const ovs_ctx* c, ovs_params* p)
{
    if (!c || !p) return OVS_EINVAL;
    *p = c->P;
    return OVS_OK;
}

ovs_status ovs_sync(ovs_ctx* c)
{
    if (!c) return OVS_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipDeviceSynchronize());
    return OVS_OK;
}

}  // extern "C"
