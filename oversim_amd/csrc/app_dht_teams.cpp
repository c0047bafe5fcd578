// app_dht_teams.cpp -- replica-team DHTs (SymmetricDHT.cc, RepeatedHashingDHT.cc) on the host: the parameter
// checks of initializeDHT, the symmetric offset, and the batch calls.  A batch derives the team keys, routes them
// one-way without timeouts through the route seam (route_check / route_device) with every chain's responders
// recorded, and replays each operation's teams (dht_teams.hip); puts then go through the DHT tier's claim /
// arbitrate / write / reset kernels under the team keys.  Every refusal happens before anything is staged.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>

#include "app_dht.hpp"
#include "dht_teams.hpp"
#include "team_params.hpp"

using namespace ovs;

namespace {

// every refusal of a team batch; *dpt is dp with numReplica divided (initializeDHT)
ovs_status team_check(ovs_ctx* c, const ovs_dht_params* dp, const ovs_dht_team_params* tp, hipStream_t s, ovs_dht_params* dpt)
{
    std::string msg;
    const ovs_status ps = team_params_check(dp, tp, &msg);
    if (ps != OVS_OK) return fail(c, ps, msg);
    if (!c->overlay) return fail(c, OVS_ESTATE, "no network loaded");
    if (c->overlay == OVS_OVERLAY_KADEMLIA)
        return fail(c, OVS_ENOTSUP, "replica teams on Kademlia: the replay needs a route chain that does not depend on "
                                    "time, and a Kademlia lookup's next FindNodeCalls depend on which responses came first");
    if (c->overlay == OVS_OVERLAY_PASTRY)
        return fail(c, OVS_ENOTSUP, "replica teams on Pastry: the replay takes its chains from a one-way route that no "
                                    "timeout ends, and a Pastry lookup's chain branches to the start vector on timeouts");
    if (c->overlay == OVS_OVERLAY_CHORD && !c->ideal)
        return fail(c, OVS_ENOTSUP, "replica teams on explicit Chord tables: the replay takes its chains from the "
                                    "no-timeout route of a converged ring");
    *dpt = *dp;
    dpt->numReplica = dp->numReplica / tp->numReplicaTeams;
    const ovs_status st = dht_check(c, dpt, s);          // Koorde, EpiChord, shards, routingType, ... as the DHT tier
    if (st != OVS_OK) return st;
    if (c->P.hopCountMax < 1 || c->P.hopCountMax > TEAM_HCM_MAX)
        return fail(c, OVS_ENOTSUP, "replica teams need hopCountMax in 1..1000 (the recorded chain holds hopCountMax responders)");
    return OVS_OK;
}

// the chain's parameters: a one-way route to one sibling that no timeout ends
ovs_params chain_params(const ovs_ctx* c)
{
    ovs_params P = c->P;
    P.numSiblings = 1;
    P.rpcUdpTimeout = P.lookupTimeout = 1e8;
    return P;
}

TeamConsts team_consts(const ovs_ctx* c, const ovs_dht_params* dpt, const ovs_dht_team_params* tp)
{
    TeamConsts C{};
    C.D = dht_consts(c, dpt);
    C.lookupTimeout = simtime_host(c->P.lookupTimeout, c->P.simtimeRound);
    C.T = tp->numReplicaTeams;
    C.hcm = c->P.hopCountMax;
    const int64_t nsucc = std::min<int64_t>(c->P.successorListSize, (int64_t)c->n - 1);
    C.m = (int)std::min<int64_t>(dpt->numReplica, 1 + nsucc);
    C.respBase = 61 + (c->P.measureAuthBlock ? 100 : 0);      // FINDNODERESPONSE_L 264 bits + 28 B (+ AUTHBLOCK_L)
    return C;
}

K160 offset_of(const ovs_dht_team_params* tp)
{
    K160 off{};
    if (tp->mode == OVS_DHT_TEAMS_SYMMETRIC) team_offset(tp->numReplicaTeams, off.w);
    return off;
}

ovs_status team_batch(ovs_ctx* c, const ovs_dht_params* dp, const ovs_dht_team_params* tp, const ovs_key160* keys,
                      const uint32_t* src, const ovs_dht_op* ops, uint64_t n, void* out, void* team_out, int32_t* winner,
                      bool is_put, uint32_t flags, void* stream)
{
    if (!c || !dp || !tp || (n && (!keys || !src || !ops || !out || !team_out || !winner))) return OVS_EINVAL;
    const bool dev = flags & OVS_DEVICE_PTRS;
    hipStream_t s = dev ? (hipStream_t)stream : c->stream;
    ovs_dht_params dpt;
    ovs_status st = team_check(c, dp, tp, s, &dpt);
    if (st != OVS_OK) return st;
    const ovs_params PC = chain_params(c);
    if ((st = route_check(c, PC, s)) != OVS_OK) return st;
    if (n >= 0xFFFFFFFFull / TEAMS_MAX) return fail(c, OVS_EINVAL, "team batches hold fewer than 2^29 operations");
    if (n == 0) return OVS_OK;
    if ((st = check_sources(c, src, n, dev)) != OVS_OK) return st;
    if (!dev) {
        for (uint64_t i = 0; i < n; ++i) {
            if (ops[i].t0_ns < 0) return fail(c, OVS_EINVAL, "DHT operation with a negative time");
            if (ops[i].id == 0)
                return fail(c, OVS_ENOTSUP, is_put ? "put with id = 0: DHT.cc:869-874 draws a random id; the caller draws it"
                                                   : "get with id = 0: wildcard gets are not implemented");
            if (ops[i].kind == 0)
                return fail(c, OVS_ENOTSUP, is_put ? "put with kind = 0 (DHTDataStorage.cc:170-173 refuses it)"
                                                   : "get with kind = 0: wildcard gets are not implemented");
        }
    }
    const TeamConsts C = team_consts(c, &dpt, tp);
    const uint64_t T = (uint64_t)C.T, nt = n * T, np = nt * (uint64_t)C.D.R;
    CallFrame F(dev, s);
    const K160* dk = F.in(reinterpret_cast<const K160*>(keys), n);
    const uint32_t* ds = F.in(src, n);
    const ovs_dht_op* dops = F.in(ops, n);
    ovs_dht_put_out* dput = is_put ? F.out(static_cast<ovs_dht_put_out*>(out), n) : nullptr;
    ovs_dht_put_out* dtput = is_put ? F.out(static_cast<ovs_dht_put_out*>(team_out), nt) : nullptr;
    ovs_dht_get_out* dget = is_put ? nullptr : F.out(static_cast<ovs_dht_get_out*>(out), n);
    ovs_dht_get_out* dtget = is_put ? nullptr : F.out(static_cast<ovs_dht_get_out*>(team_out), nt);
    int32_t* dwin = F.out(winner, n);
    if (!F.ok()) return frame_fail(c, F);
    // team keys, sources and operations per team, the chains, and the put's pair arrays
    const uint64_t o_src = up256(sizeof(K160) * nt);
    const uint64_t o_ops = o_src + up256(sizeof(uint32_t) * nt);
    const uint64_t o_rt = o_ops + up256(sizeof(ovs_dht_op) * nt);
    const uint64_t o_hop = o_rt + up256(sizeof(ovs_route_out) * nt);
    const uint64_t o_pt = o_hop + up256(sizeof(uint32_t) * nt * (uint64_t)C.hcm);
    const uint64_t o_pn = o_pt + up256(sizeof(long long) * np);
    const uint64_t o_ps = o_pn + up256(sizeof(uint32_t) * np);
    CachedBuf::Lease buf = c->dhtb.acquire(is_put ? o_ps + sizeof(uint32_t) * np : o_pt, s);
    if (!buf) return lease_fail(c, "DHT team buffers", buf);
    K160* tk = reinterpret_cast<K160*>(buf.data());
    uint32_t* tsrc = reinterpret_cast<uint32_t*>(buf.data() + o_src);
    ovs_dht_op* tops = reinterpret_cast<ovs_dht_op*>(buf.data() + o_ops);
    ovs_route_out* rt = reinterpret_cast<ovs_route_out*>(buf.data() + o_rt);
    uint32_t* hop = reinterpret_cast<uint32_t*>(buf.data() + o_hop);
    hipError_t e = launch_team_keys(tp->mode, C.T, offset_of(tp), C.D.nnodes, dk, ds, dops, n, tk, tsrc, tops, s);
    if (e != hipSuccess) return hip_fail(c, e, "team keys kernel");
    if ((st = route_device(c, PC, F, tk, tsrc, nt, rt, hop, nullptr, s)) != OVS_OK) return st;
    DhtHeader h{};
    if (is_put) {
        long long* pt = reinterpret_cast<long long*>(buf.data() + o_pt);
        uint32_t* pn = reinterpret_cast<uint32_t*>(buf.data() + o_pn);
        uint32_t* ps = reinterpret_cast<uint32_t*>(buf.data() + o_ps);
        e = launch_team_put(c->dht, C, rt, hop, tk, ds, dops, c->xy, n, dtput, dput, dwin, pt, pn, s);
        // the store kernels see n * T operations of numReplica / T pairs each, keyed by the team keys
        if (e == hipSuccess) e = launch_dht_put_apply(c->dht, C.D, pn, tk, tops, nt, pt, ps, c->num_cu, s);
    } else {
        e = launch_team_get(c->dht, C, rt, hop, tk, ds, dops, c->xy, n, dtget, dget, dwin, s);
    }
    if (e == hipSuccess && !dev) e = hipMemcpyAsync(&h, c->dht.hdr, sizeof h, hipMemcpyDeviceToHost, s);
    buf.release();
    if (e != hipSuccess) return hip_fail(c, e, "DHT team kernel");
    if (F.finish() != hipSuccess) return frame_fail(c, F);
    if (h.team_overrun)
        return fail(c, OVS_EDEVICE, "replica teams: an operation's replay ran out of its event bound (an engine defect; "
                                    "ovs_dht_store_clear resets the count)");
    if (is_put && h.last_refused)
        return fail(c, OVS_ENOMEM, "DHT store too small for this put batch (slots in use + pairs without a slot > capacity); "
                                   "nothing was changed");
    if (is_put && h.last_collisions)
        return fail(c, OVS_EDEVICE, "DHT store: a put of this batch was dropped, another entry holds its 64-bit tag");
    return OVS_OK;
}

void copy_err(char* err, int err_len, const std::string& m)
{
    if (err && err_len > 0) std::snprintf(err, (size_t)err_len, "%s", m.c_str());
}

}  // namespace

extern "C" {

void ovs_dht_team_params_default(ovs_dht_team_params* out)
{
    if (!out) return;
    out->mode = OVS_DHT_TEAMS_SYMMETRIC;
    out->numReplicaTeams = 1;
}

ovs_status ovs_dht_team_params_check(const ovs_dht_params* dp, const ovs_dht_team_params* tp, char* err, int err_len)
{
    std::string msg;
    const ovs_status st = team_params_check(dp, tp, &msg);
    if (st != OVS_OK) copy_err(err, err_len, msg);
    return st;
}

ovs_status ovs_dht_team_offset(int32_t numReplicaTeams, ovs_key160* offset)
{
    if (!offset || numReplicaTeams < 1 || numReplicaTeams > TEAMS_MAX) return OVS_EINVAL;
    static_assert(sizeof(ovs_key160) == 20, "ovs_key160 is five words");
    uint32_t w[5];
    team_offset(numReplicaTeams, w);
    std::memcpy(offset, w, sizeof w);
    return OVS_OK;
}

ovs_status ovs_dht_team_keys(ovs_ctx* c, const ovs_dht_team_params* tp, const ovs_key160* keys, uint64_t n,
                             ovs_key160* team_keys, uint32_t flags, void* stream)
{
    if (!c || !tp || (n && (!keys || !team_keys))) return OVS_EINVAL;
    if (tp->mode != OVS_DHT_TEAMS_SYMMETRIC && tp->mode != OVS_DHT_TEAMS_REPEATED_HASHING)
        return fail(c, OVS_ENOTSUP, "team mode: symmetric or repeated hashing");
    if (tp->numReplicaTeams < 1 || tp->numReplicaTeams > TEAMS_MAX) return fail(c, OVS_ENOTSUP, "dht.numReplicaTeams outside 1..8");
    if (n >= 0xFFFFFFFFull / TEAMS_MAX) return fail(c, OVS_EINVAL, "team batches hold fewer than 2^29 operations");
    if (n == 0) return OVS_OK;
    const bool dev = flags & OVS_DEVICE_PTRS;
    hipStream_t s = dev ? (hipStream_t)stream : c->stream;
    HIPCHK(c, hipSetDevice(c->device));
    CallFrame F(dev, s);
    const K160* dk = F.in(reinterpret_cast<const K160*>(keys), n);
    K160* dt = F.out(reinterpret_cast<K160*>(team_keys), n * (uint64_t)tp->numReplicaTeams);
    if (!F.ok()) return frame_fail(c, F);
    const hipError_t e = launch_team_keys(tp->mode, tp->numReplicaTeams, offset_of(tp), 0, dk, nullptr, nullptr, n, dt, nullptr,
                                          nullptr, s);
    if (e != hipSuccess) return hip_fail(c, e, "team keys kernel");
    if (F.finish() != hipSuccess) return frame_fail(c, F);
    return OVS_OK;
}

ovs_status ovs_dht_team_put_batch(ovs_ctx* c, const ovs_dht_params* dp, const ovs_dht_team_params* tp, const ovs_key160* keys,
                                  const uint32_t* src, const ovs_dht_op* ops, uint64_t n, ovs_dht_put_out* out,
                                  ovs_dht_put_out* team_out, int32_t* winner, uint32_t flags, void* stream)
{
    return team_batch(c, dp, tp, keys, src, ops, n, out, team_out, winner, true, flags, stream);
}

ovs_status ovs_dht_team_get_batch(ovs_ctx* c, const ovs_dht_params* dp, const ovs_dht_team_params* tp, const ovs_key160* keys,
                                  const uint32_t* src, const ovs_dht_op* ops, uint64_t n, ovs_dht_get_out* out,
                                  ovs_dht_get_out* team_out, int32_t* winner, uint32_t flags, void* stream)
{
    return team_batch(c, dp, tp, keys, src, ops, n, out, team_out, winner, false, flags, stream);
}

// Two launches of the DHT tier's statistics kernel: over the out records (outcomes, latencies, per-node rows) and
// over the team records (hop counts, messages, bytes; nothing per node, so its sources, operations and
// expectations are zeroed placeholders that are read and never counted)
ovs_status ovs_dhttest_team_stats_batch(ovs_ctx* c, const ovs_dht_team_params* tp, const ovs_dht_put_out* put_out,
                                        const ovs_dht_put_out* put_team_out, const uint32_t* put_src, uint64_t n_put,
                                        const ovs_dht_get_out* get_out, const ovs_dht_get_out* get_team_out,
                                        const ovs_dht_op* get_ops, const uint32_t* get_src, const ovs_dhttest_expect* expect,
                                        uint64_t n_get, double measured_time_s, ovs_dhttest_stats* stats, uint32_t flags,
                                        void* stream)
{
    if (!c || !tp || !stats || (n_put && (!put_out || !put_team_out || !put_src)) ||
        (n_get && (!get_out || !get_team_out || !get_ops || !get_src || !expect)))
        return OVS_EINVAL;
    if (tp->numReplicaTeams < 1 || tp->numReplicaTeams > TEAMS_MAX) return fail(c, OVS_ENOTSUP, "dht.numReplicaTeams outside 1..8");
    if (n_put >= 0xFFFFFFFFull / TEAMS_MAX || n_get >= 0xFFFFFFFFull / TEAMS_MAX)
        return fail(c, OVS_EINVAL, "team batches hold fewer than 2^29 operations");
    bool dev;
    hipStream_t s;
    ovs_status st = stats_begin(c, measured_time_s, 0.0, flags, stream, &dev, &s);
    if (st != OVS_OK) return st;
    const uint64_t T = (uint64_t)tp->numReplicaTeams, np = n_put * T, ng = n_get * T, nz = std::max(np, ng);
    CallFrame F(dev, s);
    const ovs_dht_put_out* dpo = F.in(put_out, n_put);
    const ovs_dht_put_out* dpt = F.in(put_team_out, np);
    const uint32_t* dps = F.in(put_src, n_put);
    const ovs_dht_get_out* dgo = F.in(get_out, n_get);
    const ovs_dht_get_out* dgt = F.in(get_team_out, ng);
    const ovs_dht_op* dgp = F.in(get_ops, n_get);
    const uint32_t* dgs = F.in(get_src, n_get);
    const ovs_dhttest_expect* dex = F.in(expect, n_get);
    // 8 inputs, 3 placeholders and 2 x 2 buffers of dhttest_sums: 15 of the frame's 16 buffers in host-pointer mode
    // (a 17th request would fail the frame, and the call with it, by name: "call frame: too many buffers")
    uint32_t* zsrc = F.scratch<uint32_t>(nz);
    ovs_dht_op* zops = F.scratch<ovs_dht_op>(ng);
    ovs_dhttest_expect* zex = F.scratch<ovs_dhttest_expect>(ng);
    if (!F.ok()) return frame_fail(c, F);
    HIPCHK(c, hipMemsetAsync(zsrc, 0, sizeof(uint32_t) * (nz ? nz : 1), s));
    HIPCHK(c, hipMemsetAsync(zops, 0, sizeof(ovs_dht_op) * (ng ? ng : 1), s));
    HIPCHK(c, hipMemsetAsync(zex, 0, sizeof(ovs_dhttest_expect) * (ng ? ng : 1), s));
    DhtStatsDev h{}, ht{};
    std::vector<uint32_t> nc, none;
    if ((st = dhttest_sums(c, F, dpo, dps, n_put, dgo, dgp, dgs, dex, n_get, true, s, &h, &nc)) != OVS_OK) return st;
    if ((st = dhttest_sums(c, F, dpt, zsrc, np, dgt, zops, zsrc, zex, ng, false, s, &ht, &none)) != OVS_OK) return st;
    h.put_hop_n = ht.put_hop_n; h.put_hop = ht.put_hop;
    h.get_hop_n = ht.get_hop_n; h.get_hop = ht.get_hop;
    h.msgs = ht.msgs; h.bytes = ht.bytes;
    dhttest_finish(h, nc, c->n, measured_time_s, stats);
    return OVS_OK;
}

}  // extern "C"
