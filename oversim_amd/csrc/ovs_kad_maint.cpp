// ovs_kad_maint.cpp -- Kademlia refresh lookups, refresh keys and maintenance rounds of the C ABI (include/ovs_kbr.h).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ctx.hpp"
#include "persist.hpp"

using namespace ovs;

namespace ovs {
namespace {

// rebuild the device tables of a whole-network Kademlia context from its host copy
ovs_status kad_upload_host_tables(ovs_ctx* c)
{
    const uint64_t n = c->n, S5 = 5ull * (uint64_t)c->P.s, k = (uint64_t)c->P.k;
    std::vector<uint32_t> hs(n * S5), hn(n * 160 * k);
    std::vector<uint8_t> hc(n * 160);
    if (!c->kh.export_k(hs.data(), hc.data(), hn.data())) {
        free_tables(c);    // the host copy was changed by the round: the device tables no longer match it
        return fail(c, OVS_ENOTSUP, "a bucket outgrew k (bucketType kademlia keeps k per bucket)");
    }
    // build into a temporary and swap it in only on success: a failed rebuild must leave the context
    // either with its previous tables or with none (free_tables below), never with null or half-built
    // tables that a later route would launch on
    KadTables nt{};
    bool staged = false;
    uint32_t bad[2] = {0, 0};
    hipError_t e = kad_build_from_host(c, hs.data(), hc.data(), hn.data(), nt, &staged, bad);
    if (!staged) return fail(c, OVS_ENOMEM, "maintenance round: device allocation failed");
    // test hook: OVS_FAULT_INJECT=kad_rebuild makes the rebuild report a broken invariant
    // (tests/test_gpu_kad_maint.py::test_failed_rebuild_leaves_no_tables)
    const char* inject = std::getenv("OVS_FAULT_INJECT");
    if (e == hipSuccess && inject && std::strcmp(inject, "kad_rebuild") == 0) { e = hipErrorInvalidValue; bad[1] = 99; }
    if (e == hipSuccess) {
        kad_free(c->kad);
        c->kad = nt;
    } else {
        kad_free(nt);
        // the host copy has already been changed by the round: the old device tables no longer
        // describe it, so the context drops its network (later calls fail with OVS_ESTATE)
        free_tables(c);
    }
    if (e == hipErrorInvalidValue && bad[1])
        return fail(c, OVS_EDEVICE, "maintenance round broke a table invariant at node " + std::to_string(bad[0]) + " (code " +
                                        std::to_string(bad[1]) + ")");
    return e == hipSuccess ? OVS_OK : hip_fail(c, e, "maintenance round: table rebuild");
}

}  // namespace
}  // namespace ovs

extern "C" {

ovs_status ovs_kad_refresh_batch(ovs_ctx* c, const ovs_key160* keys, const uint32_t* src, uint64_t n,
                                 int32_t R, ovs_lookup_out* out, uint32_t* siblings, uint32_t* responders,
                                 int64_t* rtt_ns, uint32_t* rpcs, uint32_t flags, void* stream)
{
    if (!c || (n && (!keys || !src || !out || !siblings))) return OVS_EINVAL;
    if (!c->overlay) return fail(c, OVS_ESTATE, "no network loaded");
    if (c->overlay != OVS_OVERLAY_KADEMLIA) return fail(c, OVS_ESTATE, "refresh lookups: Kademlia only");
    if (c->kad.lo != 0 || c->kad.hi != c->n)
        return fail(c, OVS_ESTATE, "context holds one arc of a sharded network: refresh lookups need the whole network");
    if (c->kad.general) return fail(c, OVS_ENOTSUP, "refresh lookups run on the 160-bucket kademlia tables");
    const ovs_params& P = c->P;
    std::string err;
    ovs_status st = check_refresh_redundant(R, true, &err);
    if (st == OVS_OK) st = check_refresh_params(P, KAD_MAX_ALPHA, &err);
    if (st != OVS_OK) return fail(c, st, err);
    HIPCHK(c, hipSetDevice(c->device));
    const bool dev = flags & OVS_DEVICE_PTRS;
    hipStream_t s = dev ? (hipStream_t)stream : c->stream;
    if (n == 0) return OVS_OK;
    if ((st = check_sources(c, src, n, dev)) != OVS_OK) return st;
    const uint64_t H = (uint64_t)P.hopCountMax;
    CallFrame F(dev, s);
    CachedBuf::Lease vis;
    const K160* dk = F.in(reinterpret_cast<const K160*>(keys), n);
    const uint32_t* ds = F.in(src, n);
    ovs_lookup_out* dout = F.out(out, n);
    uint32_t* dsib = F.out(siblings, n * (uint64_t)R);
    // the responder list is the lookup's visited set: always present on the device -- when the
    // caller asked for none, in the context's cached buffer (as K3's; a per-call hipMalloc / hipFree
    // of n * hopCountMax entries had put an allocation and a device synchronisation into every call)
    uint32_t* dresp = responders ? F.out(responders, n * H) : nullptr;
    int64_t* drtt = rtt_ns ? F.out(rtt_ns, n * H) : nullptr;
    uint32_t* drpc = rpcs ? F.out(rpcs, n) : nullptr;
    if (!F.ok()) return frame_fail(c, F);
    if (!responders) {
        vis = c->kvis.acquire(sizeof(uint32_t) * n * H, s);
        if (!vis) return lease_fail(c, "kvis", vis);
        dresp = reinterpret_cast<uint32_t*>(vis.data());
    }
    bool cap_err = false;
    const hipError_t e = kad_exhaustive(c->kad, c->xy, (uint32_t)c->n, P, delay_consts(P), R, R, false, dk, ds, n, dout,
                                        dsib, dresp, drtt, drpc, c->num_cu, s, persist_dyn_enabled(), &cap_err, nullptr,
                                        responders != nullptr /* else the internal visited lists: no padding */,
                                        responders == nullptr /* ... and their first entries in LDS */);
    vis.release();
    if (e != hipSuccess) return hip_fail(c, e, "refresh lookup kernel");
    if (cap_err) return fail(c, OVS_ENOTSUP, "a refresh lookup exceeded the kernel's capacity (64 timed-out nodes)");
    return F.finish() == hipSuccess ? OVS_OK : frame_fail(c, F);
}

ovs_status ovs_kad_maintenance_round(ovs_ctx* c, const uint32_t* nodes, uint64_t m, const uint8_t* flags,
                                     const uint32_t* stale, ovs_kad_round_stats* stats)
{
    if (!c || (m && !nodes)) return OVS_EINVAL;
    if (c->overlay != OVS_OVERLAY_KADEMLIA) return fail(c, OVS_ESTATE, "no Kademlia network loaded");
    if (c->kad.lo != 0 || c->kad.hi != c->n) return fail(c, OVS_ESTATE, "maintenance rounds need the whole network");
    if (c->kad.general) return fail(c, OVS_ENOTSUP, "maintenance rounds run on the 160-bucket kademlia tables");
    const ovs_params& P = c->P;
    if (P.routingType != 0) return fail(c, OVS_ENOTSUP, "maintenance rounds run iterative refresh lookups");
    const int Rs = 5 * P.s, Rb = P.lookupRedundantNodes;
    std::string err;
    ovs_status st = check_refresh_params(P, KAD_MAX_ALPHA, &err);
    if (st == OVS_OK) st = check_refresh_redundant(std::max(Rs, Rb), false, &err);
    if (st == OVS_OK) st = check_node_indices(nodes, m, c->n, &err);
    if (st != OVS_OK) return fail(c, st, err);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    if (c->kh.n() != c->n) {
        // a snapshot network (ovs_kad_load): its tables become the host copy
        const uint64_t n = c->n, S5 = 5ull * (uint64_t)P.s, k = (uint64_t)P.k;
        std::vector<uint32_t> hs(n * S5), hn(n * 160 * k);
        std::vector<uint8_t> hc(n * 160);
        const hipError_t e = kad_export(c->kad, (uint32_t)n, hs.data(), hc.data(), hn.data(), s);
        if (e != hipSuccess) return hip_fail(c, e, "maintenance round: table export");
        std::vector<K160> ids(n);
        std::vector<KeyRec> recs(n);
        HIPCHK(c, hipMemcpy(recs.data(), c->recs, sizeof(KeyRec) * n, hipMemcpyDeviceToHost));
        for (uint64_t v = 0; v < n; ++v) ids[v] = key_of(recs[v]);
        c->kh.import(ids.data(), n, P.k, P.s, hs.data(), hc.data(), hn.data());
    }
    KadRoundCount cnt;
    std::vector<K160> keys;
    std::vector<uint32_t> src;
    std::vector<int> R;
    c->kh.refresh_plan(nodes, m, flags, stale, Rs, Rb, &keys, &src, &R);
    const uint64_t nt = keys.size(), H = (uint64_t)P.hopCountMax;
    const int ccap = 2 * P.hopCountMax + 2 * P.lookupParallelRpcs + 16;
    cnt.lookups = nt;
    // host results of every lookup
    std::vector<uint32_t> resp(nt * H), cnode(nt * (uint64_t)ccap);
    std::vector<int64_t> tarr(nt * H), ctime(nt * (uint64_t)ccap);
    std::vector<ovs_lookup_out> outv(nt);
    const DelayConsts DC = delay_consts(P);
    // the round's lookups by redundancy (the sibling refresh's 5*s, the bucket refreshes' lookupRedundantNodes)
    std::vector<std::pair<int, std::vector<uint64_t>>> groups;
    for (const int Rg : {Rs, Rb}) {
        if (!groups.empty() && Rg == Rs) break;
        groups.push_back({Rg, {}});
        for (uint64_t t = 0; t < nt; ++t)
            if (R[t] == Rg) groups.back().second.push_back(t);
    }
    for (const auto& [Rg, ix] : groups) {
        if (ix.empty()) continue;
        const uint64_t ng = ix.size();
        std::vector<K160> gk(ng);
        std::vector<uint32_t> gs(ng);
        for (uint64_t q = 0; q < ng; ++q) { gk[q] = keys[ix[q]]; gs[q] = src[ix[q]]; }
        std::vector<uint32_t> hr(ng * H), hc(ng * (uint64_t)ccap);
        std::vector<int64_t> hta(ng * H), hct(ng * (uint64_t)ccap);
        std::vector<ovs_lookup_out> ho(ng);
        CallFrame F(false, s);
        const K160* dk = F.in(gk.data(), ng);
        const uint32_t* ds = F.in(gs.data(), ng);
        uint32_t* dsib = F.scratch<uint32_t>(ng * (uint64_t)Rg);
        uint32_t* drpc = F.scratch<uint32_t>(ng);
        uint32_t* dresp = F.out(hr.data(), ng * H);
        int64_t* dta = F.out(hta.data(), ng * H);
        uint32_t* dcn = F.out(hc.data(), ng * (uint64_t)ccap);
        int64_t* dct = F.out(hct.data(), ng * (uint64_t)ccap);
        ovs_lookup_out* dout = F.out(ho.data(), ng);
        if (!F.ok()) return frame_fail(c, F);
        const KadExhTrace tr{dta, dcn, dct, ccap};
        bool cap_err = false;
        const hipError_t e = kad_exhaustive(c->kad, c->xy, (uint32_t)c->n, P, DC, Rg, Rg, false, dk, ds, ng, dout, dsib,
                                            dresp, nullptr, drpc, c->num_cu, s, persist_dyn_enabled(), &cap_err, &tr);
        if (e != hipSuccess) return hip_fail(c, e, "maintenance round: refresh lookups");
        if (cap_err) return fail(c, OVS_ENOTSUP, "a refresh lookup exceeded the kernel's capacity");
        if (F.finish() != hipSuccess) return frame_fail(c, F);
        for (uint64_t q = 0; q < ng; ++q) {
            const uint64_t t = ix[q];
            std::copy(hr.begin() + q * H, hr.begin() + (q + 1) * H, resp.begin() + t * H);
            std::copy(hta.begin() + q * H, hta.begin() + (q + 1) * H, tarr.begin() + t * H);
            std::copy(hc.begin() + q * ccap, hc.begin() + (q + 1) * ccap, cnode.begin() + t * ccap);
            std::copy(hct.begin() + q * ccap, hct.begin() + (q + 1) * ccap, ctime.begin() + t * ccap);
            outv[t] = ho[q];
        }
    }
    // the carried nodes of every handled response: findNode(key, R, -1) at the responder on the
    // round-start tables (BaseOverlay::findNodeRpc, BaseOverlay.cc:1841-1915), on the device
    std::vector<uint8_t> ncarried(nt * H, 0);
    std::vector<int> nresp(nt, 0), ncall(nt, 0);
    for (uint64_t t = 0; t < nt; ++t) {
        while (nresp[t] < (int)H && resp[t * H + nresp[t]] != 0xFFFFFFFFu) ++nresp[t];
        while (ncall[t] < ccap && cnode[t * ccap + ncall[t]] != 0xFFFFFFFFu) ++ncall[t];
        if (outv[t].status != OVS_LOOKUP_OK) cnt.failed++;
    }
    std::vector<uint64_t> roff(nt * H, 0);
    uint64_t tot = 0;
    for (uint64_t t = 0; t < nt; ++t)
        for (int i = 0; i < nresp[t]; ++i) { roff[t * H + i] = tot; tot += (uint64_t)R[t]; }
    std::vector<uint32_t> carried(tot ? tot : 1, 0xFFFFFFFFu);
    for (const auto& [Rg, ix] : groups) {
        std::vector<uint32_t> pn;
        std::vector<K160> pk;
        std::vector<uint64_t> pri;
        for (const uint64_t t : ix)
            for (int i = 0; i < nresp[t]; ++i) { pn.push_back(resp[t * H + i]); pk.push_back(keys[t]); pri.push_back(t * H + i); }
        const uint64_t np = pn.size();
        if (np == 0) continue;
        std::vector<uint32_t> ho(np * (uint64_t)Rg);
        std::vector<uint8_t> hcount(np);
        CallFrame F(false, s);
        const uint32_t* dn = F.in(pn.data(), np);
        const K160* dk = F.in(pk.data(), np);
        uint32_t* dout = F.out(ho.data(), np * (uint64_t)Rg);
        uint8_t* dcount = F.out(hcount.data(), np);
        uint8_t* dsb = F.scratch<uint8_t>(np);
        if (!F.ok()) return frame_fail(c, F);
        const hipError_t e = kad_find_node(c->kad, (uint32_t)c->n, P, dn, dk, np, Rg, -1, dout, (uint32_t)Rg, dcount, dsb, s);
        if (e != hipSuccess) return hip_fail(c, e, "maintenance round: findNode of the responses");
        if (F.finish() != hipSuccess) return frame_fail(c, F);
        for (uint64_t q = 0; q < np; ++q) {
            ncarried[pri[q]] = hcount[q];
            std::copy(ho.begin() + q * Rg, ho.begin() + q * Rg + hcount[q], carried.begin() + roff[pri[q]]);
        }
    }
    std::vector<const uint32_t*> cptr(nt * H, nullptr);
    for (uint64_t t = 0; t < nt; ++t)
        for (int i = 0; i < nresp[t]; ++i) cptr[t * H + i] = carried.data() + roff[t * H + i];
    std::vector<KadRoundLookup> lk(nt);
    for (uint64_t t = 0; t < nt; ++t) {
        KadRoundLookup& L = lk[t];
        L.src = src[t];
        L.cnode = cnode.data() + t * ccap; L.ctime = ctime.data() + t * ccap; L.ncall = ncall[t];
        L.resp = resp.data() + t * H; L.tarr = tarr.data() + t * H; L.nresp = nresp[t];
        L.carried = cptr.data() + t * H; L.ncarried = ncarried.data() + t * H;
    }
    c->kh.apply_round(lk, &cnt);
    if (ovs_status us = kad_upload_host_tables(c)) return us;
    if (stats) {
        stats->lookups = cnt.lookups; stats->failed = cnt.failed; stats->responses = cnt.responses;
        stats->sib_changes = cnt.sib_changes; stats->bucket_changes = cnt.bucket_changes; stats->lost = cnt.lost;
        stats->replacement = cnt.replacement; stats->refreshed = cnt.refreshed;
    }
    return OVS_OK;
}

ovs_status ovs_kad_refresh_keys(ovs_ctx* c, const uint32_t* nodes, uint64_t m, const uint32_t* stale,
                                ovs_key160* keys, uint32_t* src, uint64_t cap, uint64_t* count, uint32_t flags,
                                void* stream)
{
    if (!c || !count || (m && !nodes) || (cap && (!keys || !src))) return OVS_EINVAL;
    if (c->overlay != OVS_OVERLAY_KADEMLIA) return fail(c, OVS_ESTATE, "bucket refresh: Kademlia network needed");
    if (c->kad.lo != 0 || c->kad.hi != c->n) return fail(c, OVS_ESTATE, "bucket refresh needs the whole network");
    if (c->kad.general) return fail(c, OVS_ENOTSUP, "refresh keys are generated for the 160-bucket kademlia tables");
    HIPCHK(c, hipSetDevice(c->device));
    const bool dev = flags & OVS_DEVICE_PTRS;
    hipStream_t s = dev ? (hipStream_t)stream : c->stream;
    *count = 0;
    if (m == 0) return OVS_OK;
    std::string err;
    if (!dev && check_node_indices(nodes, m, c->n, &err) != OVS_OK) return fail(c, OVS_EINVAL, err);
    CallFrame F(dev, s);
    const uint32_t* dn = F.in(nodes, m);
    const uint32_t* dst = stale ? F.in(stale, m * 5) : nullptr;
    K160* dk = cap ? F.out(reinterpret_cast<K160*>(keys), cap) : nullptr;
    uint32_t* dsrc = cap ? F.out(src, cap) : nullptr;
    if (!F.ok()) return frame_fail(c, F);
    uint64_t total = 0;
    const hipError_t e = kad_refresh_keys(c->kad, (uint32_t)c->n, dn, m, dst, dk, dsrc, cap, &total, s);
    if (e != hipSuccess) return hip_fail(c, e, "bucket refresh keys");
    F.limit(dk, total);         // the kernel wrote min(total, cap) pairs
    F.limit(dsrc, total);
    if (F.finish() != hipSuccess) return frame_fail(c, F);
    *count = total;
    return OVS_OK;
}

}  // extern "C"
