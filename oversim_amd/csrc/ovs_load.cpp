// ovs_load.cpp -- the Chord, Kademlia, Koorde and EpiChord loaders and exports of the C ABI (include/ovs_kbr.h),
// each in a LoadFrame (ctx.hpp), and the Chord fixfingers / stabilize rounds on loaded explicit tables.
#include <algorithm>
#include <string>
#include <type_traits>
#include <vector>

#include "ctx.hpp"

using namespace ovs;

namespace ovs {

ChordView chord_view(const ovs_ctx* c)
{
    ChordView V{};
    V.recs = c->recs; V.xy = c->xy; V.nodes = c->nodes; V.frow = c->fingers; V.win = c->win;
    V.lo = (uint32_t)c->shard_lo;
    V.pred = c->pred; V.succ = c->succ;
    V.nsucc = c->nsucc; V.fres = c->fres; V.n = (uint32_t)c->n;
    V.ns = (int)std::min<uint64_t>((uint64_t)c->P.successorListSize, c->n - 1);
    V.sls = c->sls;
    V.numFingerCandidates = c->P.numFingerCandidates;
    V.ftop = c->ftop; V.ftl = c->ftop ? c->ftl : 0;
    return V;
}

// NodeRec array of an ideal ring for the current successorListSize (rebuilt when it changes)
ovs_status ensure_nodes(ovs_ctx* c, hipStream_t s)
{
    if (!c->ideal || c->overlay != OVS_OVERLAY_CHORD) return OVS_OK;
    const int ns = (int)std::min<uint64_t>((uint64_t)c->P.successorListSize, c->n - 1);
    if (c->nodes && c->nodes_ns == ns) return OVS_OK;
    if (ns < 1) return fail(c, OVS_EINVAL, "successorListSize must be >= 1");
    if (!c->nodes) HIPCHK(c, hipMalloc(&c->nodes, sizeof(NodeRec) * c->n));
    if (!c->win) HIPCHK(c, hipMalloc(&c->win, sizeof(WinRec) * (c->shard_hi - c->shard_lo)));
    HIPCHK(c, launch_chord_nodes(c->recs, c->xy, (uint32_t)c->n, ns, c->nodes, c->fingers, c->nfing, c->win,
                                 (uint32_t)c->shard_lo, (uint32_t)c->shard_hi, s));
    // the replicated top levels carry their fingers' window distances too
    if (c->ftop) HIPCHK(c, launch_chord_entries(c->recs, (uint32_t)c->n, ns, c->nodes, c->ftop, c->n * (uint64_t)c->ftl, s));
    // the records are built once and then read by kernels on any stream (e.g. one stream per
    // cohort of ovs_shard_step): complete them before any other call can see nodes_ns set
    HIPCHK(c, hipStreamSynchronize(s));
    c->nodes_ns = ns;
    return OVS_OK;
}

// upload sorted ids (+ coordinates) into KeyRec / double2 arrays
ovs_status upload_nodes(ovs_ctx* c, const ovs_key160* ids, uint64_t n, const double* xy, bool dev)
{
    if (n < 2) return fail(c, OVS_EINVAL, "need at least 2 nodes");
    if (n >= 0xFFFFFFFFull) return fail(c, OVS_EINVAL, "too many nodes for 32-bit node indices");
    // device inputs may still be being written by work on any of the caller's streams (the load
    // call takes none to order against): the copies below run on the context's own
    // non-blocking stream, so wait for the whole device first (loads are not on the hot path)
    if (dev) HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMalloc(&c->recs, sizeof(KeyRec) * n));
    HIPCHK(c, hipMalloc(&c->xy, sizeof(double2) * n));
    // interleave 20 B keys into 24 B records with a strided 2-D copy
    HIPCHK(c, hipMemset2DAsync(c->recs, sizeof(KeyRec), 0, sizeof(KeyRec), n, c->stream));
    HIPCHK(c, hipMemcpy2DAsync(c->recs, sizeof(KeyRec), ids, sizeof(ovs_key160), sizeof(ovs_key160), n,
                               dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->xy, xy, sizeof(double2) * n, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                             c->stream));
    CallFrame F(false, c->stream);
    uint32_t hbad = 0;
    uint32_t* bad = F.out(&hbad, 1);
    if (!F.ok()) return frame_fail(c, F);
    HIPCHK(c, hipMemsetAsync(bad, 0, sizeof(uint32_t), c->stream));
    HIPCHK(c, launch_check_sorted(c->recs, (uint32_t)n, bad, c->stream));
    if (F.finish() != hipSuccess) return frame_fail(c, F);
    if (hbad) return fail(c, OVS_EINVAL, "node ids must be sorted ascending and unique");
    c->n = n;
    return OVS_OK;
}

// the finger rows of `rows` (m of them) from the host copy to the device: the whole table when that is
// cheaper than row by row
static ovs_status upload_finger_rows(ovs_ctx* c, const uint32_t* rows, uint64_t m)
{
    const uint64_t n = c->n;
    if (m * 8 >= n) {
        HIPCHK(c, hipMemcpy(c->fres, c->ch.fres.data(), sizeof(uint32_t) * n * 160, hipMemcpyHostToDevice));
        return OVS_OK;
    }
    for (uint64_t j = 0; j < m; ++j)
        HIPCHK(c, hipMemcpy(c->fres + (uint64_t)rows[j] * 160, c->ch.fres.data() + (uint64_t)rows[j] * 160,
                            sizeof(uint32_t) * 160, hipMemcpyHostToDevice));
    return OVS_OK;
}

hipError_t kad_build_from_host(ovs_ctx* c, const uint32_t* siblings, const uint8_t* bucket_count,
                               const uint32_t* bucket_nodes, KadTables& T, bool* staged, uint32_t bad[2])
{
    const uint64_t n = c->n, S5 = 5ull * (uint64_t)c->P.s, k = (uint64_t)c->P.k;
    CallFrame F(false, c->stream);
    uint32_t* dsib = F.scratch<uint32_t>(n * S5);
    uint8_t* dbc = F.scratch<uint8_t>(n * 160);
    uint32_t* dbn = F.scratch<uint32_t>(n * 160 * k);
    if (!(*staged = F.ok())) return F.error();
    hipError_t e = hipMemcpy(dsib, siblings, sizeof(uint32_t) * n * S5, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dbc, bucket_count, n * 160, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dbn, bucket_nodes, sizeof(uint32_t) * n * 160 * k, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = kad_build_explicit(c->recs, c->xy, (uint32_t)n, c->P.k, c->P.s, dsib, dbc, dbn, T, &bad[0], &bad[1], c->stream);
    return e;
}

namespace {

ovs_status chord_load_arc(ovs_ctx* c, const ovs_key160* ids, uint64_t n, const double* xy, uint64_t lo, uint64_t hi,
                          uint32_t flags)
{
    LoadFrame L(c, OVS_OVERLAY_CHORD, "Chord");
    if (L.st) return L.st;
    if (ovs_status s = upload_nodes(c, ids, n, xy, flags & OVS_DEVICE_PTRS)) return s;
    const hipError_t e = launch_chord_build(c->recs, (uint32_t)n, (uint32_t)lo, (uint32_t)hi, &c->fingers, &c->nfing, c->stream);
    if (e != hipSuccess) return hip_fail(c, e, "chord finger build");
    c->ideal = true; c->sls = c->P.successorListSize;
    c->shard_lo = lo; c->shard_hi = hi;
    return L.commit();
}

ovs_status kad_load_arc(ovs_ctx* c, const ovs_key160* ids, uint64_t n, const double* xy, uint64_t lo, uint64_t hi,
                        uint32_t flags)
{
    if (!c || !ids || !xy) return OVS_EINVAL;
    LoadFrame L(c, OVS_OVERLAY_KADEMLIA, "Kademlia");
    if (L.st) return L.st;
    std::string err;
    if (ovs_status s = check_kad_shape(c->P, "the snapshot rule builds b = 1 kademlia tables: other b / bucketType through "
                                              "ovs_kad_load_tables_csr", KMAX, &err))
        return fail(c, s, err);
    if (lo >= hi || hi > n) return fail(c, OVS_EINVAL, "arc [lo, hi) must be a non-empty part of [0, n)");
    if (ovs_status s = upload_nodes(c, ids, n, xy, flags & OVS_DEVICE_PTRS)) return s;
    const hipError_t e = kad_build(c->recs, c->xy, (uint32_t)n, c->P.k, c->P.s, c->P.kadSeed, c->kad, c->stream, (uint32_t)lo,
                                   (uint32_t)hi);
    if (e != hipSuccess) return hip_fail(c, e, "kademlia table build");
    return L.commit();
}

}  // namespace
}  // namespace ovs

extern "C" {

// the whole ring: the arc [0, n).  n = 0 is no arc ovs_chord_load_shard takes, and is refused here as
// every too small network is, by upload_nodes
ovs_status ovs_chord_load(ovs_ctx* c, const ovs_key160* ids, uint64_t n, const double* xy, uint32_t flags)
{
    if (!c || !ids || !xy) return OVS_EINVAL;
    return chord_load_arc(c, ids, n, xy, 0, n, flags);
}

ovs_status ovs_chord_load_shard(ovs_ctx* c, const ovs_key160* ids, uint64_t n, const double* xy, uint64_t lo,
                                uint64_t hi, uint32_t flags)
{
    if (!c || !ids || !xy || lo >= hi || hi > n) return OVS_EINVAL;
    return chord_load_arc(c, ids, n, xy, lo, hi, flags);
}

ovs_status ovs_chord_load_tables(ovs_ctx* c, const ovs_key160* ids, uint64_t n, const double* xy,
                                 const uint32_t* pred, const uint32_t* succ, const uint8_t* nsucc,
                                 const uint32_t* fingers, const uint8_t* deque_size, uint32_t flags)
{
    if (!c || !ids || !xy || !pred || !succ || !nsucc || !fingers || !deque_size) return OVS_EINVAL;
    if (flags & OVS_DEVICE_PTRS) return fail(c, OVS_ENOTSUP, "explicit tables are taken from host memory");
    LoadFrame L(c, OVS_OVERLAY_CHORD, "Chord");
    if (L.st) return L.st;
    if (ovs_status s = upload_nodes(c, ids, n, xy, false)) return s;
    const int sls = c->P.successorListSize;
    // keep the tables on the host too (batched maintenance rewrites them) and resolve
    // ChordFingerTable::getFinger(pos) there (ChordFingerTable.cc:174-193)
    std::string err;
    if (!c->ch.import(reinterpret_cast<const K160*>(ids), n, pred, succ, nsucc, fingers, deque_size, sls, &err))
        return fail(c, OVS_EINVAL, err);
    const std::vector<uint32_t>& fres = c->ch.fres;
    HIPCHK(c, hipMalloc(&c->pred, sizeof(uint32_t) * n));
    HIPCHK(c, hipMalloc(&c->succ, sizeof(uint32_t) * n * sls));
    HIPCHK(c, hipMalloc(&c->nsucc, n));
    HIPCHK(c, hipMalloc(&c->fres, sizeof(uint32_t) * n * 160));
    HIPCHK(c, hipMemcpy(c->pred, pred, sizeof(uint32_t) * n, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->succ, succ, sizeof(uint32_t) * n * sls, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->nsucc, nsucc, n, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->fres, fres.data(), sizeof(uint32_t) * n * 160, hipMemcpyHostToDevice));
    c->ideal = false; c->sls = sls;
    return L.commit();
}

ovs_status ovs_chord_export_fingers(ovs_ctx* c, uint32_t* out)
{
    if (!c || !out) return OVS_EINVAL;
    if (c->overlay != OVS_OVERLAY_CHORD) return fail(c, OVS_ESTATE, "no Chord network loaded");
    if (c->ideal && (c->shard_lo != 0 || c->shard_hi != c->n)) return fail(c, OVS_ESTATE, "sharded ring");
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t tot = c->n * 160;
    if (!c->ideal) {
        HIPCHK(c, hipMemcpy(out, c->fres, sizeof(uint32_t) * tot, hipMemcpyDeviceToHost));
        return OVS_OK;
    }
    CallFrame F(false, c->stream);
    uint32_t* d = F.out(out, tot);
    if (!F.ok()) return frame_fail(c, F);
    HIPCHK(c, launch_chord_export(c->recs, c->fingers, (uint32_t)c->n, d, c->stream));
    return F.finish() == hipSuccess ? OVS_OK : frame_fail(c, F);
}

ovs_status ovs_chord_fix_fingers(ovs_ctx* c, const uint32_t* nodes, uint64_t m, ovs_fixfingers_stats* stats)
{
    if (!c || (m && !nodes)) return OVS_EINVAL;
    if (c->overlay != OVS_OVERLAY_CHORD) return fail(c, OVS_ESTATE, "no Chord network loaded");
    if (c->ideal)
        return fail(c, OVS_ESTATE, "fixfingers rounds run on explicit tables (ovs_chord_load_tables); "
                                   "a converged ring is already their fixed point");
    if (c->P.extendedFingerTable)
        return fail(c, OVS_ENOTSUP, "extendedFingerTable: maintenance rounds keep one node per finger");
    std::string err;
    if (check_node_indices(nodes, m, c->n, &err)) return fail(c, OVS_EINVAL, err);
    // 1. handleFixFingersTimerExpired (Chord.cc:851-870): trivial fingers removed, lookups for the rest
    std::vector<K160> kk;
    std::vector<uint32_t> src;
    std::vector<uint8_t> pos;
    kk.reserve(m * 32); src.reserve(m * 32); pos.reserve(m * 32);
    c->ch.fix_fingers_plan(nodes, m, &kk, &src, &pos);
    std::vector<ovs_key160> keys(kk.size());
    for (size_t q = 0; q < kk.size(); ++q)
        for (int w = 0; w < 5; ++w) keys[q].w[w] = kk[q].w[w];
    HIPCHK(c, hipSetDevice(c->device));
    if (ovs_status st = upload_finger_rows(c, nodes, m)) return st;
    // 2. the FixfingersCalls, routed as KBR lookups on the device (sendRouteRpcCall -> sendToKey)
    std::vector<ovs_route_out> out(keys.size());
    ovs_status st = ovs_route_batch(c, keys.data(), src.data(), keys.size(), out.data(), nullptr, nullptr, 0, nullptr);
    if (st != OVS_OK) return st;
    // 3. handleRpcFixfingersResponse: finger i := the answering (responsible) node
    uint64_t ok = 0, hops = 0;
    std::vector<uint32_t> resp(out.size());
    std::vector<uint8_t> okv(out.size());
    for (size_t q = 0; q < out.size(); ++q) {
        hops += out[q].hops;
        okv[q] = out[q].status == OVS_LOOKUP_OK;
        resp[q] = out[q].responsible;
        ok += okv[q];
    }
    const uint64_t changed = c->ch.fix_fingers_apply(src, pos, resp, okv);
    for (uint64_t j = 0; j < m; ++j) c->ch.resolve_row(nodes[j]);
    if (ovs_status st = upload_finger_rows(c, nodes, m)) return st;
    if (stats) { stats->lookups = keys.size(); stats->ok = ok; stats->changed = changed; stats->hops = hops; }
    return OVS_OK;
}

ovs_status ovs_chord_stabilize(ovs_ctx* c, const uint32_t* nodes, uint64_t m, ovs_stabilize_stats* stats)
{
    if (!c || (m && !nodes)) return OVS_EINVAL;
    if (c->overlay != OVS_OVERLAY_CHORD) return fail(c, OVS_ESTATE, "no Chord network loaded");
    if (c->ideal) return fail(c, OVS_ESTATE, "stabilize rounds run on explicit tables (ovs_chord_load_tables)");
    if (c->P.extendedFingerTable)
        return fail(c, OVS_ENOTSUP, "extendedFingerTable: maintenance rounds keep one node per finger");
    const uint64_t n = c->n;
    const int sls = c->sls;
    std::string err;
    if (check_node_indices(nodes, m, n, &err)) return fail(c, OVS_EINVAL, err);
    uint64_t pred_changed = 0, succ_changed = 0, lists_changed = 0;
    std::vector<uint32_t> changed_succ0;
    c->ch.stabilize(nodes, m, &succ_changed, &lists_changed, &pred_changed, &changed_succ0);
    // upload: the lists, the predecessors, and the resolved finger rows whose successor changed
    // (getFinger falls back to the successor, ChordFingerTable.cc:174-193)
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(c->pred, c->ch.pred.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->succ, c->ch.succ.data(), sizeof(uint32_t) * n * sls, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->nsucc, c->ch.nsucc.data(), n, hipMemcpyHostToDevice));
    if (ovs_status st = upload_finger_rows(c, changed_succ0.data(), changed_succ0.size())) return st;
    if (stats) {
        stats->nodes = m; stats->succ_changed = succ_changed; stats->lists_changed = lists_changed;
        stats->pred_changed = pred_changed;
    }
    return OVS_OK;
}

ovs_status ovs_chord_export_tables(ovs_ctx* c, uint32_t* pred, uint32_t* succ, uint8_t* nsucc)
{
    if (!c || !pred || !succ || !nsucc) return OVS_EINVAL;
    if (c->overlay != OVS_OVERLAY_CHORD || c->ideal)
        return fail(c, OVS_ESTATE, "explicit Chord tables (ovs_chord_load_tables) needed");
    std::copy(c->ch.pred.begin(), c->ch.pred.end(), pred);
    std::copy(c->ch.succ.begin(), c->ch.succ.end(), succ);
    std::copy(c->ch.nsucc.begin(), c->ch.nsucc.end(), nsucc);
    return OVS_OK;
}

ovs_status ovs_kad_load(ovs_ctx* c, const ovs_key160* ids, uint64_t n, const double* xy, uint32_t flags)
{
    return kad_load_arc(c, ids, n, xy, 0, n, flags);
}

ovs_status ovs_kad_load_tables(ovs_ctx* c, const ovs_key160* ids, uint64_t n, const double* xy, const uint32_t* siblings,
                               const uint8_t* bucket_count, const uint32_t* bucket_nodes, uint32_t flags)
{
    if (!c || !ids || !xy || !siblings || !bucket_count || !bucket_nodes) return OVS_EINVAL;
    if (flags & OVS_DEVICE_PTRS) return fail(c, OVS_ENOTSUP, "explicit tables are taken from host memory");
    LoadFrame L(c, OVS_OVERLAY_KADEMLIA, "Kademlia");
    if (L.st) return L.st;
    std::string err;
    if (ovs_status s = check_kad_shape(c->P, "k-stride tables hold b = 1 kademlia buckets: other b / bucketType through "
                                              "ovs_kad_load_tables_csr", KMAX, &err))
        return fail(c, s, err);
    if (ovs_status s = upload_nodes(c, ids, n, xy, false)) return s;
    bool staged = false;
    uint32_t bad[2] = {0, 0};
    const hipError_t e = kad_build_from_host(c, siblings, bucket_count, bucket_nodes, c->kad, &staged, bad);
    if (!staged) return fail(c, OVS_ENOMEM, "explicit Kademlia tables: device allocation failed");
    if (e == hipErrorInvalidValue && bad[1]) return fail(c, OVS_EINVAL, kad_table_error(false, bad[0], bad[1]));
    if (e != hipSuccess) return hip_fail(c, e, "explicit Kademlia table build");
    c->kh.import(reinterpret_cast<const K160*>(ids), n, c->P.k, c->P.s, siblings, bucket_count, bucket_nodes);
    return L.commit();
}

int32_t ovs_kad_num_buckets(const ovs_params* p)
{
    if (!p || p->b < 1 || p->b > 5) return -1;
    return ((1 << p->b) - 1) * (KEYBITS / p->b);      // Kademlia.cc:176
}

ovs_status ovs_kad_load_tables_csr(ovs_ctx* c, const ovs_key160* ids, uint64_t n, const double* xy,
                                   const uint32_t* siblings, const uint64_t* bucket_off, const uint32_t* bucket_nodes,
                                   uint32_t flags)
{
    if (!c || !ids || !xy || !siblings || !bucket_off) return OVS_EINVAL;
    if (flags & OVS_DEVICE_PTRS) return fail(c, OVS_ENOTSUP, "explicit tables are taken from host memory");
    LoadFrame L(c, OVS_OVERLAY_KADEMLIA, "Kademlia");
    if (L.st) return L.st;
    const ovs_params& P = c->P;
    std::string err;
    if (ovs_status s = check_kad_shape(P, nullptr, KMAX, &err)) return fail(c, s, err);
    if (n == 0 || n >= 0xFFFFFFFFull) return fail(c, OVS_EINVAL, "network size out of range");
    const int nb = ovs_kad_num_buckets(&P);
    const uint64_t dir = n * (uint64_t)nb;
    if (bucket_off[0] != 0) return fail(c, OVS_EINVAL, "bucket_off[0] must be 0");
    for (uint64_t j = 0; j < dir; ++j)
        if (bucket_off[j + 1] < bucket_off[j]) return fail(c, OVS_EINVAL, "bucket_off must not decrease");
    const uint64_t total = bucket_off[dir];
    if (total >= 0xFFFFFFFFull) return fail(c, OVS_ENOTSUP, "more than 2^32 - 1 bucket members");
    if (total && !bucket_nodes) return fail(c, OVS_EINVAL, "bucket_nodes is NULL");
    if (ovs_status s = upload_nodes(c, ids, n, xy, false)) return s;
    const uint64_t S5 = 5ull * (uint64_t)P.s;
    std::vector<uint32_t> off32(dir + 1);
    for (uint64_t j = 0; j <= dir; ++j) off32[j] = (uint32_t)bucket_off[j];
    std::vector<int> caps(nb);
    for (int m = 0; m < nb; ++m) caps[m] = kad_bucket_size_host(P, m, KEYBITS);
    CallFrame F(false, c->stream);
    uint32_t* dsib = F.scratch<uint32_t>(n * S5);
    uint32_t* doff = F.scratch<uint32_t>(dir + 1);
    uint32_t* dmem = F.scratch<uint32_t>(total);
    if (!F.ok()) return fail(c, OVS_ENOMEM, "CSR Kademlia tables: device allocation failed");
    hipError_t e = hipMemcpy(dsib, siblings, sizeof(uint32_t) * n * S5, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(doff, off32.data(), sizeof(uint32_t) * (dir + 1), hipMemcpyHostToDevice);
    if (e == hipSuccess && total) e = hipMemcpy(dmem, bucket_nodes, sizeof(uint32_t) * total, hipMemcpyHostToDevice);
    uint32_t bad_node = 0, bad_code = 0;
    if (e == hipSuccess)
        e = kad_build_general(c->recs, c->xy, (uint32_t)n, P.k, P.s, P.b, caps.data(), dsib, doff, dmem, total, c->kad,
                              &bad_node, &bad_code, c->stream);
    if (e == hipErrorInvalidValue && bad_code) return fail(c, OVS_EINVAL, kad_table_error(true, bad_node, bad_code));
    if (e != hipSuccess) return hip_fail(c, e, "CSR Kademlia table build");
    return L.commit();
}

ovs_status ovs_kad_export_csr(ovs_ctx* c, uint32_t* siblings, uint64_t* bucket_off, uint32_t* bucket_nodes, uint64_t cap,
                              uint64_t* total)
{
    if (!c || !siblings || !bucket_off || !total || (cap && !bucket_nodes)) return OVS_EINVAL;
    if (c->overlay != OVS_OVERLAY_KADEMLIA) return fail(c, OVS_ESTATE, "no Kademlia network loaded");
    if (c->kad.lo != 0 || c->kad.hi != c->n) return fail(c, OVS_ESTATE, "export needs the whole network");
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t n = c->n, S5 = 5ull * (uint64_t)c->P.s;
    const KadTables& t = c->kad;
    if (t.general) {
        const uint64_t dir = n * (uint64_t)t.nb;
        std::vector<uint32_t> off32(dir + 1);
        HIPCHK(c, hipMemcpyAsync(siblings, t.sib, sizeof(uint32_t) * n * S5, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(off32.data(), t.goff, sizeof(uint32_t) * (dir + 1), hipMemcpyDeviceToHost, c->stream));
        const uint64_t ncopy = std::min<uint64_t>(cap, t.gtotal);
        if (ncopy)
            HIPCHK(c, hipMemcpyAsync(bucket_nodes, t.gidx, sizeof(uint32_t) * ncopy, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (uint64_t j = 0; j <= dir; ++j) bucket_off[j] = off32[j];
        *total = t.gtotal;
        return OVS_OK;
    }
    // the 160-bucket tables, converted
    const uint64_t k = (uint64_t)t.k;
    std::vector<uint8_t> bc(n * KEYBITS);
    std::vector<uint32_t> bn(n * KEYBITS * k);
    hipError_t e = kad_export(t, (uint32_t)n, siblings, bc.data(), bn.data(), c->stream);
    if (e != hipSuccess) return hip_fail(c, e, "kademlia export");
    uint64_t w = 0;
    bucket_off[0] = 0;
    for (uint64_t j = 0; j < n * KEYBITS; ++j) {
        for (uint64_t q = 0; q < bc[j]; ++q, ++w)
            if (w < cap) bucket_nodes[w] = bn[j * k + q];
        bucket_off[j + 1] = w;
    }
    *total = w;
    return OVS_OK;
}

ovs_status ovs_kad_load_shard(ovs_ctx* c, const ovs_key160* ids, uint64_t n, const double* xy, uint64_t lo,
                              uint64_t hi, uint32_t flags)
{
    return kad_load_arc(c, ids, n, xy, lo, hi, flags);
}

ovs_status ovs_kad_export(ovs_ctx* c, uint32_t* siblings, uint8_t* bucket_count, uint32_t* bucket_nodes)
{
    if (!c || !siblings || !bucket_count || !bucket_nodes) return OVS_EINVAL;
    if (c->overlay != OVS_OVERLAY_KADEMLIA) return fail(c, OVS_ESTATE, "no Kademlia network loaded");
    if (c->kad.lo != 0 || c->kad.hi != c->n) return fail(c, OVS_ESTATE, "export needs the whole network");
    if (c->kad.general) return fail(c, OVS_ENOTSUP, "CSR tables: ovs_kad_export_csr");
    HIPCHK(c, hipSetDevice(c->device));
    hipError_t e = kad_export(c->kad, (uint32_t)c->n, siblings, bucket_count, bucket_nodes, c->stream);
    return e == hipSuccess ? OVS_OK : hip_fail(c, e, "kademlia export");
}

ovs_status ovs_koorde_load(ovs_ctx* c, const ovs_key160* ids, uint64_t n, const double* xy, uint32_t flags)
{
    if (!c || !ids || !xy) return OVS_EINVAL;
    LoadFrame L(c, OVS_OVERLAY_KOORDE, "Koorde");
    if (L.st) return L.st;
    if (n < 2) return fail(c, OVS_EINVAL, "Koorde needs at least 2 nodes");
    if (c->P.successorListSize < 1) return fail(c, OVS_EINVAL, "successorListSize must be >= 1");
    if (c->P.shiftingBits < 1 || c->P.shiftingBits > 16 || c->P.deBruijnListSize < 1 || c->P.deBruijnListSize > 255)
        return fail(c, OVS_ENOTSUP, "Koorde shiftingBits must be 1..16 and deBruijnListSize 1..255");
    if (ovs_status s = upload_nodes(c, ids, n, xy, flags & OVS_DEVICE_PTRS)) return s;
    const hipError_t e = koorde_build(c->recs, c->xy, (uint32_t)n, c->P.successorListSize, c->P.shiftingBits,
                                      c->P.deBruijnListSize, c->P.useOtherLookup, c->P.useSucList, c->koorde, c->stream);
    if (e != hipSuccess) return hip_fail(c, e, "koorde build");
    return L.commit();
}

ovs_status ovs_koorde_export(ovs_ctx* c, uint32_t* db_node, uint32_t* db_start, uint8_t* db_num)
{
    if (!c || !db_node || !db_start || !db_num) return OVS_EINVAL;
    if (c->overlay != OVS_OVERLAY_KOORDE) return fail(c, OVS_ESTATE, "no Koorde network loaded");
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<KoordeNode> h(c->n);
    HIPCHK(c, hipMemcpyAsync(h.data(), c->koorde.nd, sizeof(KoordeNode) * c->n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (uint64_t i = 0; i < c->n; ++i) {
        db_node[i] = h[i].db; db_start[i] = h[i].dbStart; db_num[i] = (uint8_t)h[i].dbNum;
    }
    return OVS_OK;
}

ovs_status ovs_epichord_load(ovs_ctx* c, const ovs_key160* ids, uint64_t n, const double* xy, const uint32_t* succ,
                             const uint8_t* nsucc, const uint32_t* pred, const uint8_t* npred, const uint8_t* lists_full,
                             const uint64_t* cache_off, const uint32_t* cache_node, const int64_t* cache_last_ns,
                             const int64_t* cache_ttl_ns, uint32_t flags)
{
    if (!c || !ids || !xy || !succ || !nsucc || !pred || !npred || !lists_full || !cache_off) return OVS_EINVAL;
    if (flags & OVS_DEVICE_PTRS) return fail(c, OVS_ENOTSUP, "ovs_epichord_load takes host buffers");
    LoadFrame frame(c, OVS_OVERLAY_EPICHORD, "EpiChord");
    if (frame.st) return frame.st;
    const int L = c->P.successorListSize;
    if (L < 1 || L > EPI_MAXL) return fail(c, OVS_ENOTSUP, "EpiChord successorListSize must be 1..16");
    if (!(c->P.cacheTTL >= 0)) return fail(c, OVS_EINVAL, "cacheTTL must be >= 0");
    if (n < 2 || n >= 0xFFFFFFFFull) return fail(c, OVS_EINVAL, "node count out of range");
    std::vector<uint32_t> meta, cn;
    std::vector<int64_t> cl, ct;
    std::string err;
    if (!epichord_prepare(reinterpret_cast<const K160*>(ids), n, L, succ, nsucc, pred, npred, lists_full, cache_off,
                          cache_node, cache_last_ns, cache_ttl_ns, &meta, &cn, &cl, &ct, &err))
        return fail(c, OVS_EINVAL, err);
    const uint64_t E = cache_off[n];
    if (ovs_status st = upload_nodes(c, ids, n, xy, false)) return st;
    EpiTables& T = c->epi;
    T.n = (uint32_t)n; T.L = L; T.nent = E;
    auto up = [&](auto** d, const auto* h, uint64_t cnt) -> hipError_t {
        using TT = std::remove_pointer_t<std::remove_reference_t<decltype(*d)>>;
        hipError_t e = hipMalloc((void**)d, sizeof(TT) * (cnt ? cnt : 1));
        if (e == hipSuccess && cnt) e = hipMemcpyAsync(*d, h, sizeof(TT) * cnt, hipMemcpyHostToDevice, c->stream);
        return e;
    };
    hipError_t e = up(&T.succ, succ, n * L);
    if (e == hipSuccess) e = up(&T.pred, pred, n * L);
    if (e == hipSuccess) e = up(&T.meta, meta.data(), n);
    if (e == hipSuccess) e = up(&T.coff, cache_off, n + 1);
    if (e == hipSuccess) e = up(&T.cnode, cn.data(), E);
    if (e == hipSuccess) e = up(&T.clast, cl.data(), E);
    if (e == hipSuccess) e = up(&T.cttl, ct.data(), E);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return hip_fail(c, e, "EpiChord snapshot upload");
    return frame.commit();
}

}  // extern "C"
