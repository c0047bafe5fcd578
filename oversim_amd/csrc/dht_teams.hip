// dht_teams.hip -- replica-team DHTs (src/applications/dht/SymmetricDHT.cc, RepeatedHashingDHT.cc).
//
// k_team_keys    per operation: the T derived keys (a 160-bit add of the offset, or SHA-1 of the key's 40 hex
//                characters: one 512-bit block, 80 rounds), and the sources / operations once per team for the
//                route launch and the store kernels.
// k_team_replay  one lane per operation: one event loop over all messages of the operation's T teams in
//                (time, scheduling order).  Every team walks its recorded chain of FindNodeCall responders
//                (IterativeLookup.cc:803-921, 1067-1170: rpcUdpTimeout per call, LOOKUP_TIMEOUT checked on every
//                response, the hop budget, the visited check the chain's end stands for), then runs its put or
//                get as k_dht_put_plan / k_dht_get restate DHT.cc.  Every send goes through its sender's transmit
//                queue (SimpleNodeEntry.cc:164-194): the source's is one register shared by all teams; any other
//                node only ever answers, and the tx.finished its answer left is kept with the RPC that asked, so
//                a node that answers twice finds its queue by a scan over the operation's RPCs.  A message to the
//                sending host itself has no delay and no queue (SimpleUDP.cc:320-345).
// An operation has at most T chain cursors and 8 put RPCs, or 8 hash + 8 value RPCs; all dynamically indexed
// per-lane state lives in LDS ([slot][lane]).  No lane waits for another one; the loop is bounded by the
// operation's event count.  All stores to memory are ordinary vector stores and atomics.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "dht_dev.hpp"
#include "dht_teams.hpp"

namespace ovs {

namespace {

constexpr int64_t NEVER = DHT_NEVER;
constexpr int FINDNODECALL_BYTES = 83;      // FINDNODECALL_L 440 bits + 28 B
constexpr int NODEHANDLE_BYTES = 26;        // NODEHANDLE_L 208 bits

// ---------------------------------------------------------------- team keys
__device__ __forceinline__ uint32_t rol(uint32_t x, int s) { return (x << s) | (x >> (32 - s)); }
__device__ __forceinline__ uint32_t hex_char(uint32_t nib) { return nib < 10 ? 48u + nib : 87u + nib; }

// OverlayKey::sha1(BinaryValue(key.toString(16))): the 40 characters most significant nibble first
// (OverlayKey.cc:60, 163-181), the digest read as a big-endian number (685-701)
__device__ K160 sha1_of_hex(const K160& k)
{
    uint32_t W[16];
#pragma unroll
    for (int t = 0; t < 10; ++t) {
        uint32_t w = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int pos = 39 - (4 * t + b);               // nibble position from the least significant one
            w = (w << 8) | hex_char((k.w[pos >> 3] >> (4 * (pos & 7))) & 15u);
        }
        W[t] = w;
    }
    W[10] = 0x80000000u;
    W[11] = W[12] = W[13] = W[14] = 0;
    W[15] = 320;
    uint32_t a = 0x67452301u, b = 0xEFCDAB89u, c = 0x98BADCFEu, d = 0x10325476u, e = 0xC3D2E1F0u;
#pragma unroll
    for (int t = 0; t < 80; ++t) {
        if (t >= 16) W[t & 15] = rol(W[(t + 13) & 15] ^ W[(t + 8) & 15] ^ W[(t + 2) & 15] ^ W[t & 15], 1);
        uint32_t f, kk;
        if (t < 20) { f = (b & c) | (~b & d); kk = 0x5A827999u; }
        else if (t < 40) { f = b ^ c ^ d; kk = 0x6ED9EBA1u; }
        else if (t < 60) { f = (b & c) | (b & d) | (c & d); kk = 0x8F1BBCDCu; }
        else { f = b ^ c ^ d; kk = 0xCA62C1D6u; }
        const uint32_t tmp = rol(a, 5) + f + e + kk + W[t & 15];
        e = d; d = c; c = rol(b, 30); b = a; a = tmp;
    }
    K160 o;
    o.w[4] = 0x67452301u + a; o.w[3] = 0xEFCDAB89u + b; o.w[2] = 0x98BADCFEu + c; o.w[1] = 0x10325476u + d;
    o.w[0] = 0xC3D2E1F0u + e;
    return o;
}

__device__ __forceinline__ K160 add160(const K160& a, const K160& b)
{
    K160 o;
    uint64_t carry = 0;
#pragma unroll
    for (int w = 0; w < 5; ++w) {
        const uint64_t s = (uint64_t)a.w[w] + b.w[w] + carry;
        o.w[w] = (uint32_t)s;
        carry = s >> 32;
    }
    return o;
}

__global__ __launch_bounds__(256) void k_team_keys(int mode, int T, K160 offset, uint32_t nnodes, const K160* __restrict__ keys,
                                                   const uint32_t* __restrict__ src, const ovs_dht_op* __restrict__ ops,
                                                   uint64_t n, K160* __restrict__ team_keys, uint32_t* __restrict__ team_src,
                                                   ovs_dht_op* __restrict__ team_ops)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    K160 k = keys[i];
    for (int j = 0; j < T; ++j) {
        team_keys[i * T + j] = k;
        if (team_src) {
            const uint32_t S = src[i];
            team_src[i * T + j] = S < nnodes ? S : 0u;
            team_ops[i * T + j] = ops[i];
        }
        k = mode == OVS_DHT_TEAMS_SYMMETRIC ? add160(k, offset) : sha1_of_hex(k);
    }
}

// ---------------------------------------------------------------- the replay
constexpr int TL = 64;                      // lanes of a block = operations
constexpr uint32_t I_RESP = 8u;             // the response is on its way (else the call)
constexpr uint32_t I_DEAD = 16u;            // the RPC timed out: its response is dropped
constexpr uint32_t I_HASH = 64u;            // get: a hash request
constexpr uint32_t I_HAS = 128u;            // get: the replica holds the entry
enum { PH_LOOKUP = 0, PH_DHT = 1, PH_DONE = 2 };

template <bool PUT>
struct TeamLds {
    static constexpr int RPCS = PUT ? DHT_MAXR : 2 * DHT_MAXR;
    static constexpr int SLOTS = TEAMS_MAX + RPCS;      // [0, T): the teams' chain cursors; TEAMS_MAX + k: DHT RPC k
    long long mt[SLOTS][TL];        // the message under way: its arrival; NEVER when none
    long long tt[SLOTS][TL];        // the RPC's timeout; NEVER once fired or cancelled
    long long rfin[SLOTS][TL];      // the responder's tx.finished after its answer to this RPC
    uint32_t seq[SLOTS][TL];        // scheduling order: the message's, the timeout's << 16
    uint32_t node[SLOTS][TL];       // the responder
    uint32_t info[SLOTS][TL];       // bits 0-2 team, I_*, bits 8-10 the sibling's position
    unsigned long long tok[PUT ? 1 : RPCS][TL];      // get: the answering entry's token
    uint32_t vlen[PUT ? 1 : RPCS][TL];
    uint32_t resp[PUT ? 1 : DHT_MAXR][TL];           // get: hash responses in arrival order: RPC, bit 8 popped, bits 9-11 team
    uint32_t tw[TEAMS_MAX][TL];     // team state (TeamState::pack)
    uint32_t tw2[TEAMS_MAX][TL];    // hops, messages << 16
    uint32_t tbytes[TEAMS_MAX][TL];
    unsigned long long ctok[TEAMS_MAX][TL];          // get: the chosen hash
};

struct TeamState {
    int phase, m, nreplica, nresp, ok, bad, nsent;
    bool value_sent, chosen_set, chosen_has;
    __device__ __forceinline__ uint32_t pack() const
    {
        return (uint32_t)phase | (uint32_t)m << 2 | (uint32_t)nreplica << 6 | (uint32_t)nresp << 10 |
               (value_sent ? 1u << 14 : 0u) | (chosen_set ? 1u << 15 : 0u) | (chosen_has ? 1u << 16 : 0u) |
               (uint32_t)ok << 17 | (uint32_t)bad << 21 | (uint32_t)nsent << 25;
    }
    __device__ __forceinline__ static TeamState unpack(uint32_t w)
    {
        TeamState s;
        s.phase = w & 3; s.m = (w >> 2) & 15; s.nreplica = (w >> 6) & 15; s.nresp = (w >> 10) & 15;
        s.value_sent = (w >> 14) & 1; s.chosen_set = (w >> 15) & 1; s.chosen_has = (w >> 16) & 1;
        s.ok = (w >> 17) & 15; s.bad = (w >> 21) & 15; s.nsent = (w >> 25) & 15;
        return s;
    }
};

template <bool PUT>
__global__ __launch_bounds__(TL) void k_team_replay(DhtStore st, TeamConsts C, const ovs_route_out* __restrict__ route,
                                                    const uint32_t* __restrict__ hopseq, const K160* __restrict__ tkeys,
                                                    const uint32_t* __restrict__ src, const ovs_dht_op* __restrict__ ops,
                                                    const double2* __restrict__ xy, uint64_t n,
                                                    std::conditional_t<PUT, ovs_dht_put_out, ovs_dht_get_out>* __restrict__ team_out,
                                                    std::conditional_t<PUT, ovs_dht_put_out, ovs_dht_get_out>* __restrict__ out,
                                                    int32_t* __restrict__ winner, long long* __restrict__ pair_t,
                                                    uint32_t* __restrict__ pair_node)
{
    using Out = std::conditional_t<PUT, ovs_dht_put_out, ovs_dht_get_out>;
    using Lds = TeamLds<PUT>;
    __shared__ Lds M;
    const int ln = threadIdx.x;
    const int T = C.T, R = C.D.R;
    const DhtConsts& D = C.D;
    uint64_t need = 0;
    const uint64_t stride = (uint64_t)gridDim.x * TL;
    for (uint64_t i = (uint64_t)blockIdx.x * TL + ln; i < n; i += stride) {
        const ovs_dht_op op = ops[i];
        const uint32_t S = src[i] < D.nnodes ? src[i] : 0u;
        const int64_t t0 = op.t0_ns;
        int64_t stx = 0;                    // the source's tx.finished, shared by all teams
        uint32_t sq = 0;                    // scheduling order
        int nrpc = 0, nr = 0, win = -1;
        for (int j = 0; j < T; ++j) {
            M.mt[j][ln] = NEVER; M.tt[j][ln] = NEVER; M.rfin[j][ln] = 0; M.node[j][ln] = NONE; M.info[j][ln] = (uint32_t)j;
            M.tw[j][ln] = 0; M.tw2[j][ln] = 0; M.tbytes[j][ln] = 0; M.ctok[j][ln] = 0;
        }
        if (PUT)
            for (int p = 0; p < T * R; ++p) { pair_t[i * T * R + p] = -1; pair_node[i * T * R + p] = NONE; }

        // ---- the transmit queues
        auto from_src = [&](uint32_t b, int wire, int64_t now) { return dht_send(stx, S, b, wire, now, xy, D); };
        // node a answers RPC `slot`: its queue is the latest tx.finished its earlier answers left
        auto to_src = [&](int slot, uint32_t a, int wire, int64_t now) {
            if (a == S) return now;
            int64_t q = 0;
            for (int x = 0; x < T; ++x)
                if (M.node[x][ln] == a && M.rfin[x][ln] > q) q = M.rfin[x][ln];
            for (int x = TEAMS_MAX; x < TEAMS_MAX + nrpc; ++x)
                if (M.node[x][ln] == a && M.rfin[x][ln] > q) q = M.rfin[x][ln];
            const int64_t arr = dht_send(q, a, S, wire, now, xy, D);
            M.rfin[slot][ln] = q;
            return arr;
        };
        // a call leaves the source: its timeout is scheduled first (BaseRpc.cc:257-258), then the message
        auto call = [&](int slot, uint32_t b, int wire, uint32_t info, int64_t now) {
            M.node[slot][ln] = b;
            M.rfin[slot][ln] = 0;
            M.info[slot][ln] = info;
            M.tt[slot][ln] = now + D.timeout;
            const uint32_t ts = sq++;
            const int64_t a = from_src(b, wire, now);
            M.mt[slot][ln] = a;
            M.seq[slot][ln] = sq++ | ts << 16;
            return a;
        };

        // ---- a team's end: its record as DHT.cc accounts it; the first one is what tier 2 accepts
        auto finish = [&](int j, TeamState& ts, uint8_t outcome, uint8_t status, int64_t now, Out o) {
            const uint32_t w2 = M.tw2[j][ln];
            o.outcome = outcome;
            o.status = status;
            o.latency_ns = outcome == OVS_DHT_LOOKUP_FAILED ? -1 : now - t0;
            o.hop_count = outcome == OVS_DHT_LOOKUP_FAILED ? 0 : (uint16_t)(w2 & 0xFFFFu);
            o.messages = (uint16_t)(w2 >> 16);
            o.bytes = M.tbytes[j][ln];
            o.num_sent = (uint8_t)ts.nsent;
            o.num_responses = (uint8_t)(PUT ? ts.ok : ts.nresp);
            team_out[i * T + j] = o;
            ts.phase = PH_DONE;
            if (win < 0) win = j;
        };
        auto blank = [&]() {
            Out o{};
            if constexpr (!PUT) o.server = NONE;
            return o;
        };

        // ---- get: the hash bookkeeping of k_dht_get, per team
        auto same_hash = [&](int k, bool has, unsigned long long tk) {
            const bool h = (M.info[TEAMS_MAX + k][ln] & I_HAS) != 0;
            return h == has && (!h || M.tok[PUT ? 0 : k][ln] == tk);
        };
        auto size_of = [&](int j, bool has, unsigned long long tk) {
            int c = 0;
            for (int x = 0; x < nr; ++x) {
                const uint32_t e = M.resp[PUT ? 0 : x][ln];
                if ((int)(e >> 9) == j && !(e & 256u) && same_hash((int)(e & 255u), has, tk)) ++c;
            }
            return c;
        };
        auto majority = [&](int j, bool& bhas, unsigned long long& btok) {
            int best = 0;
            for (int x = 0; x < nr; ++x) {
                const uint32_t e = M.resp[PUT ? 0 : x][ln];
                if ((int)(e >> 9) != j || (e & 256u)) continue;
                const int k = (int)(e & 255u);
                const bool h = (M.info[TEAMS_MAX + k][ln] & I_HAS) != 0;
                const unsigned long long tk = h ? M.tok[PUT ? 0 : k][ln] : 0;
                const int c = size_of(j, h, tk);
                const bool before = (!h && bhas) || (h == bhas && tk < btok);
                if (c > best || (c == best && best > 0 && before)) { best = c; bhas = h; btok = tk; }
            }
            return best;
        };
        auto pop_back = [&](int j, bool has, unsigned long long tk) {
            for (int x = nr - 1; x >= 0; --x) {
                const uint32_t e = M.resp[PUT ? 0 : x][ln];
                if ((int)(e >> 9) == j && !(e & 256u) && same_hash((int)(e & 255u), has, tk)) {
                    M.resp[PUT ? 0 : x][ln] = e | 256u;
                    return (int)((M.info[TEAMS_MAX + (e & 255u)][ln] >> 8) & 7u);
                }
            }
            return 0;
        };
        // the team's sibling at position x: the responsible node and its successors on the converged ring
        auto sibling = [&](int j, int x) {
            const uint32_t first = route[i * T + j].responsible;
            const uint64_t v = (uint64_t)(first < D.nnodes ? first : S) + (uint32_t)x;
            return (uint32_t)(v >= D.nnodes ? v - D.nnodes : v);
        };
        auto get_send = [&](int j, int x, bool is_hash, int64_t now) {
            if (nrpc >= Lds::RPCS) return;                    // cannot happen: at most 8 hash and 8 value requests
            const int k = nrpc++;
            const uint32_t r = sibling(j, x);
            const int64_t a = call(TEAMS_MAX + k, r, wire_bytes(GETCALL_BITS), (uint32_t)j | (is_hash ? I_HASH : 0u) | (uint32_t)x << 8, now);
            const K160 key = tkeys[i * T + j];
            const uint32_t q = dht_find(st, entry_tag(r, key, op.kind, op.id));      // DHT.cc:441-443
            bool has = false;
            unsigned long long tk = 0;
            uint32_t vl = 0;
            if (q != NONE) {
                const DhtSlot* sl = &st.slots[q];
                if (slot_is(sl, r, key, op.kind, op.id) && sl->vlen > 0 && sl->expiry > a) { has = true; tk = sl->token; vl = sl->vlen; }
            }
            if (has) M.info[TEAMS_MAX + k][ln] |= I_HAS;
            M.tok[PUT ? 0 : k][ln] = tk;
            M.vlen[PUT ? 0 : k][ln] = vl;
            const int bits = BASERPC_BITS + D.auth + 160 + (!has ? 0 : is_hash ? HASH_BITS : (int)vl + ENTRY_BITS);
            M.tw2[j][ln] += 2u << 16;
            M.tbytes[j][ln] += (uint32_t)(bits_bytes(GETCALL_BITS) + bits_bytes(bits));
        };
        // the value request to the last node that sent the chosen hash, or the get's failure (DHT.cc:198-221, 268-290, 686-714)
        auto value_or_fail = [&](int j, TeamState& ts, int64_t now, bool mark) {
            if (ts.chosen_set && size_of(j, ts.chosen_has, M.ctok[j][ln]) > 0) {
                get_send(j, pop_back(j, ts.chosen_has, M.ctok[j][ln]), false, now);
                if (mark) ts.value_sent = true;
            } else {
                finish(j, ts, OVS_DHT_FAILED, OVS_LOOKUP_OK, now, blank());
            }
        };

        // ---- the lookup's end
        auto lookup_ok = [&](int j, TeamState& ts, int64_t now) {             // DHT.cc:832-957
            ts.phase = PH_DHT;
            ts.m = C.m;
            if constexpr (PUT) {
                const int call_bits = BASERPC_BITS + D.auth + (int)op.vlen + ENTRY_BITS;      // PUTCALL_L
                const int resp_bits = BASERPC_BITS + D.auth + 8;                              // PUTRESPONSE_L
                const K160 key = tkeys[i * T + j];
                for (int x = 0; x < ts.m && nrpc < Lds::RPCS; ++x) {                          // DHT.cc:876-891
                    const uint32_t r = sibling(j, x);
                    const int64_t a = call(TEAMS_MAX + nrpc++, r, wire_bytes(call_bits), (uint32_t)j | (uint32_t)x << 8, now);
                    const uint64_t p = (i * T + j) * R + x;
                    pair_t[p] = a;
                    pair_node[p] = r;
                    if (dht_find(st, entry_tag(r, key, op.kind, op.id)) == NONE) ++need;
                }
                ts.nsent = ts.m;
                M.tw2[j][ln] += (uint32_t)(2 * ts.m) << 16;
                M.tbytes[j][ln] = (uint32_t)(ts.m * (bits_bytes(call_bits) + bits_bytes(resp_bits)));
            } else {
                const int first = ts.m < D.G ? ts.m : D.G;
                for (int x = 0; x < first; ++x) get_send(j, x, true, now);                    // DHT.cc:934-946
                ts.nsent = first;
                ts.nreplica = ts.m;
            }
        };
        auto lookup_failed = [&](int j, TeamState& ts, uint8_t status, int64_t now) {         // DHT.cc:852-864, 910-927
            finish(j, ts, OVS_DHT_LOOKUP_FAILED, status, now, blank());
        };
        auto chain_call = [&](int j, int hops, int64_t now) {
            const uint32_t cur = hopseq[(i * T + j) * (uint64_t)C.hcm + hops];
            call(j, cur < D.nnodes ? cur : S, FINDNODECALL_BYTES, (uint32_t)j, now);
        };

        // ---- t0: every team's LookupCall, in team order (SymmetricDHT.cc:48-74)
        for (int j = 0; j < T; ++j) {
            const ovs_route_out rt = route[i * T + j];
            TeamState ts = TeamState::unpack(0);
            if (rt.hops == 0) {
                // the source is responsible (IterativeLookup.cc:157-204: no hop, no delay); else nothing to ask
                if (rt.status == OVS_LOOKUP_OK) lookup_ok(j, ts, t0);
                else lookup_failed(j, ts, rt.status, t0);
            } else {
                chain_call(j, 0, t0);
            }
            M.tw[j][ln] = ts.pack();
        }

        // ---- the events in (time, scheduling order)
        const int max_events = T * (3 * C.hcm + 3) + 3 * Lds::RPCS + 8;
        for (int guard = 0; guard < max_events; ++guard) {
            int k = -1;
            bool is_to = false;
            long long now = NEVER;
            uint32_t bs = 0;
            auto look = [&](int x) {
                const uint32_t s = M.seq[x][ln];
                const long long e = M.mt[x][ln], f = M.tt[x][ln];
                if (e < now || (e == now && k >= 0 && (s & 0xFFFFu) < bs)) { now = e; k = x; is_to = false; bs = s & 0xFFFFu; }
                if (f < now || (f == now && k >= 0 && (s >> 16) < bs)) { now = f; k = x; is_to = true; bs = s >> 16; }
            };
            for (int x = 0; x < T; ++x) look(x);
            for (int x = TEAMS_MAX; x < TEAMS_MAX + nrpc; ++x) look(x);
            if (k < 0) break;
            const uint32_t inf = M.info[k][ln];
            const int j = (int)(inf & 7u);
            TeamState ts = TeamState::unpack(M.tw[j][ln]);
            if (is_to) {
                M.tt[k][ln] = NEVER;
                M.info[k][ln] = inf | I_DEAD;
                if (ts.phase == PH_DONE) continue;            // the team's pending RPCs went with its state
                if (k < TEAMS_MAX) {
                    lookup_failed(j, ts, now > t0 + C.lookupTimeout ? OVS_LOOKUP_TIMEOUT : OVS_LOOKUP_RPC_TIMEOUT, now);
                } else if constexpr (PUT) {                   // DHT.cc:172-180
                    if (2 * ++ts.bad >= ts.m) finish(j, ts, OVS_DHT_FAILED, OVS_LOOKUP_OK, now, blank());
                } else if (ts.value_sent) {                   // DHT.cc:198-221
                    value_or_fail(j, ts, now, false);
                } else if (ts.nreplica > D.G) {               // 226-240
                    get_send(j, --ts.nreplica, true, now);
                } else {
                    if (ts.nresp > 0) {                       // 243-259
                        bool bh = false; unsigned long long bt = 0;
                        ts.chosen_set = majority(j, bh, bt) > 0;
                        ts.chosen_has = bh; M.ctok[j][ln] = bt;
                    }
                    value_or_fail(j, ts, now, false);         // 268-290: the state stays
                }
                M.tw[j][ln] = ts.pack();
                continue;
            }
            if (!(inf & I_RESP)) {
                // the call arrives: the responder answers through its own queue, whether or not the caller still waits
                const uint32_t a = M.node[k][ln];
                int wire;
                if (k < TEAMS_MAX) {
                    const ovs_route_out rt = route[i * T + j];
                    const int hops = (int)(M.tw2[j][ln] & 0xFFFFu);
                    const bool sib = rt.status == OVS_LOOKUP_OK && hops + 1 == (int)rt.hops;
                    wire = C.respBase + NODEHANDLE_BYTES * (sib ? C.m : 1);
                } else if constexpr (PUT) {
                    wire = wire_bytes(BASERPC_BITS + D.auth + 8);
                } else {
                    const int kk = k - TEAMS_MAX;
                    const bool has = (inf & I_HAS) != 0;
                    wire = wire_bytes(BASERPC_BITS + D.auth + 160 +
                                      (!has ? 0 : (inf & I_HASH) ? HASH_BITS : (int)M.vlen[PUT ? 0 : kk][ln] + ENTRY_BITS));
                }
                M.mt[k][ln] = to_src(k, a, wire, now);
                M.seq[k][ln] = (M.seq[k][ln] & 0xFFFF0000u) | sq++;
                M.info[k][ln] = inf | I_RESP;
                continue;
            }
            // the response arrives at the source
            M.mt[k][ln] = NEVER;
            if ((inf & I_DEAD) || ts.phase == PH_DONE) continue;
            M.tt[k][ln] = NEVER;                              // the timeout is cancelled
            if (k < TEAMS_MAX) {                              // IterativePathLookup::handleResponse
                const ovs_route_out rt = route[i * T + j];
                if (now > t0 + C.lookupTimeout) {             // IterativeLookup.cc:808-815
                    lookup_failed(j, ts, OVS_LOOKUP_TIMEOUT, now);
                } else {
                    const int hops = (int)(M.tw2[j][ln] & 0xFFFFu) + 1;
                    M.tw2[j][ln] = (M.tw2[j][ln] & 0xFFFF0000u) | (uint32_t)hops;
                    if (rt.status == OVS_LOOKUP_OK && hops == (int)rt.hops) lookup_ok(j, ts, now);
                    else if (hops >= C.hcm) lookup_failed(j, ts, OVS_LOOKUP_HOPMAX, now);     // 1074-1086
                    else if (hops >= (int)rt.hops) lookup_failed(j, ts, rt.status, now);      // the chain's end: 1147-1168
                    else chain_call(j, hops, now);
                }
            } else if constexpr (PUT) {                       // DHT.cc:553-575
                if (++ts.ok >= ts.m / 2 + 1) finish(j, ts, OVS_DHT_SUCCESS, OVS_LOOKUP_OK, now, blank());
            } else {
                const int kk = k - TEAMS_MAX;
                if (ts.value_sent && !(inf & I_HASH)) {       // DHT.cc:585-598: also with an empty result array
                    Out o = blank();
                    if constexpr (!PUT) {
                        o.server = M.node[k][ln];
                        if (inf & I_HAS) { o.result_count = 1; o.value_token = M.tok[PUT ? 0 : kk][ln]; o.value_len = M.vlen[PUT ? 0 : kk][ln]; }
                    }
                    finish(j, ts, OVS_DHT_SUCCESS, OVS_LOOKUP_OK, now, o);
                } else {
                    bool go = true;
                    if (inf & I_HASH) {                       // DHT.cc:601-684
                        if (nr < DHT_MAXR) M.resp[PUT ? 0 : nr++][ln] = (uint32_t)kk | (uint32_t)j << 9;
                        ++ts.nresp;
                        if (ts.value_sent) {                  // 617-620
                            go = false;
                        } else {
                            bool bh = false; unsigned long long bt = 0;
                            const int cnt = majority(j, bh, bt);
                            if ((double)cnt / (double)ts.m >= D.ratio) {      // 635-637
                                ts.chosen_set = cnt > 0; ts.chosen_has = bh; M.ctok[j][ln] = bt;
                            } else if (ts.nresp >= D.G) {     // 638
                                if (ts.nreplica > D.G) {      // 640-653
                                    get_send(j, --ts.nreplica, true, now);
                                } else if (cnt == 0) {        // 654-678
                                    finish(j, ts, OVS_DHT_FAILED, OVS_LOOKUP_OK, now, blank());
                                    go = false;
                                } else {                      // 679-682
                                    ts.chosen_set = true; ts.chosen_has = bh; M.ctok[j][ln] = bt;
                                }
                            }
                        }
                    }
                    if (go && !ts.value_sent && ts.chosen_set) value_or_fail(j, ts, now, true);   // DHT.cc:686-714
                }
            }
            M.tw[j][ln] = ts.pack();
        }
        // cannot happen: every pending RPC has an event.  If the bound were wrong the operation is counted, and a
        // host-pointer call fails with OVS_EDEVICE
        bool overrun = false;
        for (int j = 0; j < T; ++j) {
            TeamState ts = TeamState::unpack(M.tw[j][ln]);
            if (ts.phase != PH_DONE) { finish(j, ts, OVS_DHT_FAILED, OVS_LOOKUP_OK, t0 - 1, blank()); overrun = true; }
        }
        if (overrun) atomicAdd(&st.hdr->team_overrun, 1ull);
        out[i] = team_out[i * T + win];
        winner[i] = win;
    }
    if constexpr (PUT) {
        need = wave_sum_u64(need);
        if ((threadIdx.x & 63) == 0 && need) atomicAdd(&st.hdr->need, (unsigned long long)need);
    }
}

template <bool PUT, class Out>
hipError_t team_launch(const DhtStore& st, const TeamConsts& C, const ovs_route_out* route, const uint32_t* hopseq,
                       const K160* team_keys, const uint32_t* src, const ovs_dht_op* ops, const double2* xy, uint64_t n,
                       Out* team_out, Out* out, int32_t* winner, long long* pair_t, uint32_t* pair_node, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    if (!st.slots || !st.cap || C.T < 1 || C.T > TEAMS_MAX || C.D.R < 1 || C.D.R > DHT_MAXR || C.T * C.D.R > DHT_MAXR ||
        C.D.G < 1 || C.D.G > DHT_MAXR || C.m < 1 || C.m > C.D.R || C.hcm < 1 || C.hcm > TEAM_HCM_MAX || C.D.nnodes == 0)
        return hipErrorInvalidValue;
    uint64_t blocks = (n + TL - 1) / TL;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(k_team_replay<PUT>, dim3((unsigned)blocks), dim3(TL), 0, s, st, C, route, hopseq, team_keys, src, ops,
                       xy, n, team_out, out, winner, pair_t, pair_node);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_team_keys(int mode, int T, const K160& offset, uint32_t nnodes, const K160* keys, const uint32_t* src,
                            const ovs_dht_op* ops, uint64_t n, K160* team_keys, uint32_t* team_src, ovs_dht_op* team_ops,
                            hipStream_t s)
{
    if (n == 0) return hipSuccess;
    if (T < 1 || T > TEAMS_MAX || (team_src != nullptr) != (team_ops != nullptr)) return hipErrorInvalidValue;
    const uint64_t blocks = blocks256(n);
    if (!grid_ok(blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_team_keys, dim3((unsigned)blocks), dim3(256), 0, s, mode, T, offset, nnodes, keys, src, ops, n,
                       team_keys, team_src, team_ops);
    return hipGetLastError();
}

hipError_t launch_team_put(const DhtStore& st, const TeamConsts& C, const ovs_route_out* route, const uint32_t* hopseq,
                           const K160* team_keys, const uint32_t* src, const ovs_dht_op* ops, const double2* xy, uint64_t n,
                           ovs_dht_put_out* team_out, ovs_dht_put_out* out, int32_t* winner, long long* pair_t,
                           uint32_t* pair_node, hipStream_t s)
{
    return team_launch<true>(st, C, route, hopseq, team_keys, src, ops, xy, n, team_out, out, winner, pair_t, pair_node, s);
}

hipError_t launch_team_get(const DhtStore& st, const TeamConsts& C, const ovs_route_out* route, const uint32_t* hopseq,
                           const K160* team_keys, const uint32_t* src, const ovs_dht_op* ops, const double2* xy, uint64_t n,
                           ovs_dht_get_out* team_out, ovs_dht_get_out* out, int32_t* winner, hipStream_t s)
{
    return team_launch<false>(st, C, route, hopseq, team_keys, src, ops, xy, n, team_out, out, winner, nullptr, nullptr, s);
}

}  // namespace ovs
