// ovs_shard.cpp -- one arc of a sharded network behind the C ABI (include/ovs_kbr.h): the Chord shard steps and the
// Kademlia shard rounds and migration step.  shard_route.cpp drives these across ranks.
#include <algorithm>
#include <string>

#include "ctx.hpp"

using namespace ovs;

namespace ovs {
namespace {

// the arc boundaries on the device: uploaded (synchronously) only when they change, so a step
// never waits for the host copy of a pageable buffer behind the work queued on its stream
ovs_status upload_bounds(ovs_ctx* c, const uint64_t* lo, uint32_t nshards)
{
    if (!c->d_bounds) HIPCHK(c, hipMalloc(&c->d_bounds, sizeof(uint64_t) * (MAXSHARDS + 1)));
    if (c->h_bounds.size() == nshards + 1 && std::equal(lo, lo + nshards + 1, c->h_bounds.begin())) return OVS_OK;
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpy(c->d_bounds, lo, sizeof(uint64_t) * (nshards + 1), hipMemcpyHostToDevice));
    c->h_bounds.assign(lo, lo + nshards + 1);
    return OVS_OK;
}

// a step's arc map checked against the context's arc [lo, hi), the device selected and the bounds brought up
// to date there; *me: the context's arc
ovs_status arc_map(ovs_ctx* c, const uint64_t* shard_lo, uint32_t nshards, uint64_t lo, uint64_t hi, int* me)
{
    uint64_t bounds[MAXSHARDS + 1];
    std::string err;
    if (ovs_status st = check_arc_map(shard_lo, nshards, c->n, lo, hi, bounds, me, &err)) return fail(c, st, err);
    HIPCHK(c, hipSetDevice(c->device));
    return upload_bounds(c, bounds, nshards);
}

// a LookupCall's numSiblings across arcs (< 0: successorListSize), 1..8 and no more than the list holds
ovs_status shard_lookup_ns(ovs_ctx* c, int32_t num_siblings, bool bounded, int32_t* ns)
{
    *ns = num_siblings < 0 ? c->P.successorListSize : num_siblings;
    if (bounded && *ns > c->P.successorListSize) return fail(c, OVS_EINVAL, "numSiblings too big!");
    if (*ns < 1 || *ns > 8) return fail(c, OVS_ENOTSUP, "LookupCall across arcs implements numSiblings 1..8");
    return OVS_OK;
}

// ns = 0: one-way routes (ovs_shard_step); ns >= 1: LookupCalls with that many siblings
ovs_status shard_step(ovs_ctx* c, int ns, const ovs_lookup_rec* in, uint64_t n_in, ovs_lookup_rec* out,
                      uint64_t out_cap, unsigned long long* out_count, ovs_done_rec* done, uint64_t done_cap,
                      unsigned long long* done_count, const uint64_t* shard_lo, uint32_t nshards, void* stream,
                      const ovs_key160* fkeys = nullptr, const uint32_t* fsrc = nullptr, uint32_t fqid = 0)
{
    if (!c || !shard_lo || nshards == 0 || nshards > (uint32_t)MAXSHARDS) return OVS_EINVAL;
    if (n_in && ((!in && !(fkeys && fsrc)) || !out || !out_count || !done || !done_count)) return OVS_EINVAL;
    if (c->overlay != OVS_OVERLAY_CHORD || !c->ideal) return fail(c, OVS_ESTATE, "no Chord ring (shard) loaded");
    ovs_status st = check_common(c, c->P);
    if (st == OVS_OK) st = check_chord_route(c, c->P);
    if (st != OVS_OK) return st;
    int me = -1;
    if ((st = arc_map(c, shard_lo, nshards, c->shard_lo, c->shard_hi, &me)) != OVS_OK) return st;
    hipStream_t s = (hipStream_t)stream;   // device-pointer call: NULL = the default stream
    LookupConsts LC{c->P.hopCountMax, ns ? ns : c->P.numSiblings, c->P.lookupRedundantNodes, c->P.routingType != 0};
    DelayConsts DC = delay_consts(c->P);
    if (ns) {
        if (c->P.routingType != 0) return fail(c, OVS_ENOTSUP, "LookupCall is implemented for routingType = iterative");
        DC.lookupCall = 1;
        DC.msgRespSib = ring_sibling_response_ns(DC, c->P, c->n, ns);     // as ovs_lookup_batch
    }
    if ((st = ensure_nodes(c, s)) != OVS_OK) return st;
    const DynSlots::Lease dyn = dyn_acquire(c, n_in, s);
    HIPCHK(c, launch_chord_shard_step(chord_view(c), DC, LC, c->d_bounds, (int)nshards, me, in, n_in, out, out_cap,
                                      out_count, done, done_cap, done_count, c->stage[s], c->num_cu, s,
                                      reinterpret_cast<const K160*>(fkeys), fsrc, fqid, dyn.get()));
    return OVS_OK;
}

ovs_status kad_shard_begin_impl(ovs_ctx* c, int32_t lk_ns, uint32_t* sib, const ovs_key160* keys, const uint32_t* src,
                                uint64_t n, uint32_t qid_base, void* stream)
{
    if (!c || (n && (!keys || !src))) return OVS_EINVAL;
    if (c->overlay != OVS_OVERLAY_KADEMLIA) return fail(c, OVS_ESTATE, "no Kademlia network loaded");
    ovs_params P = c->P;
    if (lk_ns >= 0) P.numSiblings = 1;     // the route checks; numSiblings is the LookupCall's
    ovs_status st = check_common(c, P);
    if (st != OVS_OK) return st;
    if (P.routingType != 0) return fail(c, OVS_ENOTSUP, "Kademlia routing is implemented for routingType = iterative");
    if (lk_ns >= 0) P.numSiblings = lk_ns;
    if (!kad_params_supported_host(P, c->kad) || (lk_ns < 0 && P.numSiblings != 1))
        return fail(c, OVS_ENOTSUP, "lookup configuration not implemented");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const int alpha = c->P.lookupParallelRpcs;
    const int fcap = kad_shard_cap(P, c->kad);
    if (n > c->kcap || alpha != c->kalpha || fcap != c->kfcap) {
        free_kad_shard(c);
        const uint64_t cap = n ? n : 1;
        HIPCHK(c, hipMalloc(&c->kst, kad_lookup_state_bytes(alpha, fcap) * cap));
        HIPCHK(c, hipMalloc(&c->kact, cap));
        HIPCHK(c, hipMalloc(&c->kkeys, sizeof(K160) * cap));
        HIPCHK(c, hipMalloc(&c->ksrc, sizeof(uint32_t) * cap));
        HIPCHK(c, hipMalloc(&c->kqids, sizeof(uint32_t) * cap));
        HIPCHK(c, hipMalloc(&c->kres, (fcap > 8 ? sizeof(KadResN<16>) : sizeof(KadResN<8>)) * cap * kad_pend_slots(alpha)));
        HIPCHK(c, hipMalloc(&c->kiota, sizeof(uint64_t) * cap));
        HIPCHK(c, hipMalloc(&c->klist[0], sizeof(uint64_t) * cap));
        HIPCHK(c, hipMalloc(&c->klist[1], sizeof(uint64_t) * cap));
        HIPCHK(c, hipMalloc(&c->knl, sizeof(unsigned long long) * 3));
        c->kcap = cap; c->kalpha = alpha; c->kfcap = fcap;
    }
    c->knlook = n; c->kns = lk_ns; c->ksib = sib;
    if ((st = kad_shard_reset_errors(c, stream)) != OVS_OK) return st;      // the error count, allocated on first use
    c->kcur = 0;
    HIPCHK(c, kad_shard_init(reinterpret_cast<const K160*>(keys), src, n, qid_base, c->kkeys, c->ksrc, c->kact,
                             c->kqids, c->kiota, c->knl, c->kad.lo, c->kad.hi, c->kbad, s));
    return OVS_OK;
}

}  // namespace

ovs_status kad_shard_reset_errors(ovs_ctx* c, void* stream)
{
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->kbad) HIPCHK(c, hipMalloc(&c->kbad, sizeof(unsigned long long)));
    HIPCHK(c, hipMemsetAsync(c->kbad, 0, sizeof(unsigned long long), (hipStream_t)stream));
    return OVS_OK;
}

ovs_status kad_mig_step_impl(ovs_ctx* c, const void* in, uint64_t n_in, const ovs_key160* fkeys, const uint32_t* fsrc,
                             uint32_t fqid, void* out, uint64_t out_cap, unsigned long long* out_count, ovs_done_rec* done,
                             uint64_t done_cap, unsigned long long* done_count, const uint64_t* shard_lo,
                             uint32_t nshards, void* stream, bool reset_errors)
{
    if (!c || !shard_lo || nshards == 0 || nshards > (uint32_t)MAXSHARDS) return OVS_EINVAL;
    if (n_in && ((!in && !(fkeys && fsrc)) || !out || !out_count || !done || !done_count)) return OVS_EINVAL;
    if (c->overlay != OVS_OVERLAY_KADEMLIA) return fail(c, OVS_ESTATE, "no Kademlia network loaded");
    ovs_status st = check_common(c, c->P);
    if (st != OVS_OK) return st;
    if (!kad_mig_supported(c->P, c->kad))
        return fail(c, OVS_ENOTSUP, "the migration step implements one-way iterative KBR routes on snapshot tables with "
                                    "k and lookupRedundantNodes <= 8");
    int me = -1;
    if ((st = arc_map(c, shard_lo, nshards, c->kad.lo, c->kad.hi, &me)) != OVS_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    if (!c->kbad || reset_errors)
        if ((st = kad_shard_reset_errors(c, stream)) != OVS_OK) return st;
    const DynSlots::Lease dyn = dyn_acquire(c, n_in, s);
    hipError_t e = kad_mig_step(c->kad, c->xy, (uint32_t)c->n, c->P, delay_consts(c->P), in, n_in,
                                reinterpret_cast<const K160*>(fkeys), fsrc, fqid, c->d_bounds, (int)nshards, me, out,
                                out_cap, out_count, done, done_cap, done_count, c->kbad, c->num_cu, c->stage[s], s,
                                dyn.get());
    return e == hipSuccess ? OVS_OK : hip_fail(c, e, "kademlia migration step");
}

}  // namespace ovs

extern "C" {

ovs_status ovs_chord_shard_replicate(ovs_ctx* c, int32_t top_levels)
{
    if (!c) return OVS_EINVAL;
    if (c->overlay != OVS_OVERLAY_CHORD || !c->ideal) return fail(c, OVS_ESTATE, "no Chord ring (shard) loaded");
    if (top_levels < 0 || top_levels > 32) return fail(c, OVS_EINVAL, "top_levels must be 0..32");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());        // kernels of earlier steps may still read the old levels
    if (c->ftop) hipFree(c->ftop);
    c->ftop = nullptr; c->ftl = 0;
    if (top_levels == 0) return OVS_OK;
    const uint64_t tot = c->n * (uint64_t)top_levels;
    HIPCHK(c, hipMalloc(&c->ftop, sizeof(FingerEnt) * tot));
    c->ftl = top_levels;
    HIPCHK(c, launch_chord_top(c->recs, (uint32_t)c->n, top_levels, c->ftop, c->stream));
    if (c->nodes) HIPCHK(c, launch_chord_entries(c->recs, (uint32_t)c->n, c->nodes_ns, c->nodes, c->ftop, tot, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return OVS_OK;
}

int32_t ovs_chord_shard_levels(const ovs_ctx* c) { return c && c->ftop ? c->ftl : 0; }

ovs_status ovs_shard_make_records(ovs_ctx* c, const ovs_key160* keys, const uint32_t* src, uint64_t n,
                                  uint32_t qid_base, ovs_lookup_rec* recs, void* stream)
{
    if (!c || (n && (!keys || !src || !recs))) return OVS_EINVAL;
    if (c->overlay != OVS_OVERLAY_CHORD || !c->ideal) return fail(c, OVS_ESTATE, "no Chord ring (shard) loaded");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;   // device-pointer call: NULL = the default stream
    HIPCHK(c, launch_make_records(c->recs, reinterpret_cast<const K160*>(keys), src, n, qid_base, recs, s));
    return OVS_OK;
}

ovs_status ovs_shard_step_keys(ovs_ctx* c, int32_t num_siblings, const ovs_key160* keys, const uint32_t* src, uint64_t n,
                               uint32_t qid_base, ovs_lookup_rec* out, uint64_t out_cap, unsigned long long* out_count,
                               ovs_done_rec* done, uint64_t done_cap, unsigned long long* done_count,
                               const uint64_t* shard_lo, uint32_t nshards, void* stream)
{
    if (!c || (n && (!keys || !src))) return OVS_EINVAL;
    int32_t ns = 0;
    if (num_siblings != 0)
        if (ovs_status st = shard_lookup_ns(c, num_siblings, true, &ns)) return st;
    return shard_step(c, ns, nullptr, n, out, out_cap, out_count, done, done_cap, done_count, shard_lo, nshards, stream,
                      keys, src, qid_base);
}

ovs_status ovs_shard_step(ovs_ctx* c, const ovs_lookup_rec* in, uint64_t n_in, ovs_lookup_rec* out, uint64_t out_cap,
                          unsigned long long* out_count, ovs_done_rec* done, uint64_t done_cap,
                          unsigned long long* done_count, const uint64_t* shard_lo, uint32_t nshards, void* stream)
{
    return shard_step(c, 0, in, n_in, out, out_cap, out_count, done, done_cap, done_count, shard_lo, nshards, stream);
}

ovs_status ovs_shard_step_lookup(ovs_ctx* c, int32_t num_siblings, const ovs_lookup_rec* in, uint64_t n_in,
                                 ovs_lookup_rec* out, uint64_t out_cap, unsigned long long* out_count,
                                 ovs_done_rec* done, uint64_t done_cap, unsigned long long* done_count,
                                 const uint64_t* shard_lo, uint32_t nshards, void* stream)
{
    if (!c) return OVS_EINVAL;
    int32_t ns = 0;
    if (ovs_status st = shard_lookup_ns(c, num_siblings, true, &ns)) return st;
    return shard_step(c, ns, in, n_in, out, out_cap, out_count, done, done_cap, done_count, shard_lo, nshards, stream);
}

ovs_status ovs_shard_lookup_finish(ovs_ctx* c, const ovs_done_rec* done, uint64_t n, int32_t num_siblings,
                                   ovs_lookup_out* out, uint32_t* siblings, void* stream)
{
    if (!c || (n && (!done || !out || !siblings))) return OVS_EINVAL;
    if (c->overlay != OVS_OVERLAY_CHORD || !c->ideal) return fail(c, OVS_ESTATE, "no Chord ring (shard) loaded");
    int32_t ns = 0;
    if (ovs_status st = shard_lookup_ns(c, num_siblings, false, &ns)) return st;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_shard_lookup_finish(chord_view(c), ns, done, out, siblings, n, (hipStream_t)stream));
    return OVS_OK;
}

ovs_status ovs_kad_shard_begin(ovs_ctx* c, const ovs_key160* keys, const uint32_t* src, uint64_t n, uint32_t qid_base,
                               void* stream)
{
    return kad_shard_begin_impl(c, -1, nullptr, keys, src, n, qid_base, stream);
}

ovs_status ovs_kad_shard_begin_lookup(ovs_ctx* c, int32_t num_siblings, const ovs_key160* keys, const uint32_t* src,
                                      uint64_t n, uint32_t qid_base, uint32_t* siblings, void* stream)
{
    if (!c || (n && !siblings)) return OVS_EINVAL;
    if (c->overlay != OVS_OVERLAY_KADEMLIA) return fail(c, OVS_ESTATE, "no Kademlia network loaded");
    // BaseOverlay::lookupRpc: numSiblings < 0 -> getMaxNumSiblings() = s (Kademlia.cc:347-350)
    const int32_t ns = num_siblings < 0 ? c->P.s : num_siblings;
    if (ns > c->P.s) return fail(c, OVS_EINVAL, "numSiblings too big!");
    if (ns > 8) return fail(c, OVS_ENOTSUP, "LookupCall implements numSiblings <= 8");
    return kad_shard_begin_impl(c, ns, siblings, keys, src, n, qid_base, stream);
}

ovs_status ovs_kad_shard_step(ovs_ctx* c, ovs_kad_req* out, uint64_t out_cap, unsigned long long* out_count,
                              ovs_done_rec* done, uint64_t done_cap, unsigned long long* done_count,
                              unsigned long long* active_count, const uint64_t* shard_lo, uint32_t nshards, void* stream)
{
    if (!c || !shard_lo || nshards == 0 || nshards > (uint32_t)MAXSHARDS) return OVS_EINVAL;
    if (!out || !out_count || !done || !done_count || !active_count) return OVS_EINVAL;
    if (c->overlay != OVS_OVERLAY_KADEMLIA) return fail(c, OVS_ESTATE, "no Kademlia network loaded");
    if (!c->kst) return fail(c, OVS_ESTATE, "no lookups started (ovs_kad_shard_begin)");
    if (c->P.lookupParallelRpcs != c->kalpha && c->knlook)
        return fail(c, OVS_ESTATE, "lookupParallelRpcs changed since ovs_kad_shard_begin");
    if (kad_shard_cap(c->P, c->kad) != c->kfcap && c->knlook)
        return fail(c, OVS_ESTATE, "lookupRedundantNodes / k changed the findNode capacity since ovs_kad_shard_begin");
    if (out_cap < c->knlook * (uint64_t)kad_pend_slots(c->kalpha))
        return fail(c, OVS_EINVAL, "out_cap must hold a request per pending-call slot "
                                   "(n * lookupParallelRpcs; n * 8 for lookupParallelRpcs 5..8)");
    int me = -1;
    if (ovs_status st = arc_map(c, shard_lo, nshards, c->kad.lo, c->kad.hi, &me)) return st;
    hipStream_t s = (hipStream_t)stream;
    // this round's list: iota in round 1, then the ping-pong lists the previous round compacted
    const int cur = c->kcur, nxt = cur == 1 ? 2 : 1;
    const uint64_t* list = cur == 0 ? c->kiota : c->klist[cur - 1];
    hipError_t e = kad_shard_step(c->kad, c->xy, (uint32_t)c->n, c->P, delay_consts(c->P), c->kst, c->kact, c->kkeys,
                                  c->ksrc, c->kqids,
                                  c->kres, c->knlook, list, c->knl + cur, c->kiota, c->klist[nxt - 1], c->knl + nxt,
                                  c->d_bounds, (int)nshards, out, out_cap, out_count, done, done_cap, done_count,
                                  active_count, c->kns, c->ksib, c->kbad, c->num_cu, c->stage[s], s);
    if (e != hipSuccess) return hip_fail(c, e, "kademlia shard step");
    c->kcur = nxt;
    return OVS_OK;
}

int32_t ovs_kad_shard_resp_bytes(const ovs_ctx* c)
{
    if (!c || c->overlay != OVS_OVERLAY_KADEMLIA) return -1;
    return kad_shard_cap(c->P, c->kad) > 8 ? (int32_t)sizeof(ovs_kad_resp16) : (int32_t)sizeof(ovs_kad_resp);
}

ovs_status ovs_kad_shard_serve(ovs_ctx* c, const ovs_kad_req* in, uint64_t n, void* out, void* stream)
{
    if (!c || (n && (!in || !out))) return OVS_EINVAL;
    if (c->overlay != OVS_OVERLAY_KADEMLIA) return fail(c, OVS_ESTATE, "no Kademlia network loaded");
    if (c->kst && c->knlook && kad_shard_cap(c->P, c->kad) != c->kfcap)
        return fail(c, OVS_ESTATE, "lookupRedundantNodes / k changed the findNode capacity since ovs_kad_shard_begin");
    HIPCHK(c, hipSetDevice(c->device));
    hipError_t e = kad_shard_serve(c->kad, (uint32_t)c->n, c->P, in, n, out, c->kbad, (hipStream_t)stream);
    return e == hipSuccess ? OVS_OK : hip_fail(c, e, "kademlia shard serve");
}

ovs_status ovs_kad_shard_deliver(ovs_ctx* c, const void* in, uint64_t n, void* stream)
{
    if (!c || (n && !in)) return OVS_EINVAL;
    if (!c->kres) return fail(c, OVS_ESTATE, "no lookups started (ovs_kad_shard_begin)");
    if (c->overlay != OVS_OVERLAY_KADEMLIA) return fail(c, OVS_ESTATE, "no Kademlia network loaded");
    if (c->knlook && kad_shard_cap(c->P, c->kad) != c->kfcap)
        return fail(c, OVS_ESTATE, "lookupRedundantNodes / k changed the findNode capacity since ovs_kad_shard_begin");
    HIPCHK(c, hipSetDevice(c->device));
    hipError_t e = kad_shard_deliver(c->kfcap, in, n, c->kres, c->knlook * (uint64_t)kad_pend_slots(c->kalpha), c->kbad,
                                     (hipStream_t)stream);
    return e == hipSuccess ? OVS_OK : hip_fail(c, e, "kademlia shard deliver");
}

ovs_status ovs_kad_shard_replicate(ovs_ctx* c, int32_t top_levels)
{
    if (!c) return OVS_EINVAL;
    if (c->overlay != OVS_OVERLAY_KADEMLIA || !c->kad.snapshot || c->kad.general)
        return fail(c, OVS_ESTATE, "no Kademlia snapshot network (ovs_kad_load_shard) loaded");
    if (top_levels < 0 || top_levels > KTOP_MAX) return fail(c, OVS_EINVAL, "top_levels must be 0..7");
    if (c->kad.tl == top_levels) return OVS_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());      // kernels of earlier rounds may still read the tables
    const uint32_t lo = c->kad.lo, hi = c->kad.hi;
    hipError_t e = kad_build(c->recs, c->xy, (uint32_t)c->n, c->P.k, c->P.s, c->P.kadSeed, c->kad, c->stream, lo, hi,
                             top_levels);
    if (e != hipSuccess) { free_tables(c); return hip_fail(c, e, "kademlia table rebuild (replicated top buckets)"); }
    return OVS_OK;
}

int32_t ovs_kad_shard_levels(const ovs_ctx* c)
{
    return c && c->overlay == OVS_OVERLAY_KADEMLIA ? c->kad.tl : 0;
}

int32_t ovs_kad_shard_rec_bytes(const ovs_ctx* c)
{
    if (!c || c->overlay != OVS_OVERLAY_KADEMLIA) return -1;
    return (int32_t)kad_rec_bytes(c->P.lookupParallelRpcs);
}


ovs_status ovs_kad_shard_mig_step(ovs_ctx* c, const void* in, uint64_t n_in, const ovs_key160* fkeys, const uint32_t* fsrc,
                                  uint32_t fqid, void* out, uint64_t out_cap, unsigned long long* out_count,
                                  ovs_done_rec* done, uint64_t done_cap, unsigned long long* done_count,
                                  const uint64_t* shard_lo, uint32_t nshards, void* stream)
{
    // a batch's first round (in == NULL) starts the error count afresh
    return ovs::kad_mig_step_impl(c, in, n_in, fkeys, fsrc, fqid, out, out_cap, out_count, done, done_cap, done_count,
                                  shard_lo, nshards, stream, in == nullptr);
}

ovs_status ovs_kad_shard_errors(ovs_ctx* c, uint64_t* bad)
{
    if (!c || !bad) return OVS_EINVAL;
    *bad = 0;
    if (!c->kbad) return OVS_OK;
    HIPCHK(c, hipSetDevice(c->device));
    unsigned long long h = 0;
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpy(&h, c->kbad, sizeof h, hipMemcpyDeviceToHost));
    *bad = h;
    return OVS_OK;
}

}  // extern "C"
