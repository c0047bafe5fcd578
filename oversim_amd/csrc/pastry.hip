// pastry.hip -- Pastry routing (src/overlay/pastry/BasePastry.cc, PastryLeafSet.cc, PastryRoutingTable.cc) for
// gfx950 (MI355X).
//
// The build kernels fill the converged tables: a leaf slot is a ring neighbour of the owner, a
// routing-table slot two bisections over the sorted ids.  pastry_find_node_dev (pastry_dev.hpp) is
// BasePastry::findNode at one node: the one restatement, called by the findNode batch kernel and by every hop of
// k_pastry_route<ACKS>, which runs one lane per semi-recursive route message (BaseOverlay::sendToKey's recursive
// branch, pastry_send_to_key) on the persistent-slice scheduler of persist.hpp; its ACKS instantiation is the same
// route under routeMsgAcks, every hop a NextHopCall with its ack.  A hop reads the node's record, its leaf
// row and the one table slot the key addresses; the table rows are scanned only for the closer-node fallback and
// when the first candidate of a numRedundantNodes > 1 answer is refused.  k_pastry_iter runs one lane per
// IterativeLookup (a LookupCall with its sibling vector, or the one-way message under iterative routing) on the
// same scheduler: FindNodeCalls from the source, one pastry_find_node_dev per responder.
#include "pastry_dev.hpp"

#include "broose_host.hpp"
#include "persist.hpp"

namespace ovs {

void pastry_free(PastryTables& t)
{
    if (t.rec) hipFree(t.rec);
    if (t.leaf) hipFree(t.leaf);
    if (t.tab) hipFree(t.tab);
    t.rec = nullptr; t.leaf = nullptr; t.tab = nullptr;
    t.n = 0; t.rows = 0;
}

namespace {

// ---------------------------------------------------------------------------
// the converged tables

// first index of [lo, hi) whose id is >= t
__device__ uint32_t lower_bound(const KeyRec* __restrict__ recs, uint32_t lo, uint32_t hi, const K160& t)
{
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (k_lt(rkey(recs, mid), t)) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the rows the rule fills: a node's last non-empty row is the one of the most digits it shares with another id,
// which a sorted neighbour attains
__global__ void k_pastry_max_rows(const KeyRec* __restrict__ recs, uint32_t n, int b, int* __restrict__ out)
{
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v + 1 >= n) return;
    atomicMax(out, min(p_spl_bits(rkey(recs, v), rkey(recs, v + 1)) / b + 1, 160 / b));
}

// n - 1 >= L: the L/2 ring predecessors (the nearest in slot L/2 - 1) and the L/2 ring successors (from slot L/2)
__global__ void k_pastry_leaf_rule(const KeyRec* __restrict__ recs, uint32_t n, int L, KeyRec* __restrict__ leaf)
{
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (uint64_t)n * (uint64_t)L) return;
    const uint64_t v = g / (uint64_t)L;
    const int j = (int)(g % (uint64_t)L), h = L / 2;
    const uint64_t x = j < h ? (v + n - (uint64_t)(h - j)) % n : (v + 1 + (uint64_t)(j - h)) % n;
    KeyRec e = load_rec(recs, (uint32_t)x);
    e.aux = (uint32_t)x;
    leaf[g] = e;
}

// slot (r, c) of owner v: empty where c is the owner's digit or no id is in the class (the owner's first r digits,
// then c); else the first id of the class at or above the owner's key with digit r replaced by c, else the
// class's smallest.  The class is a contiguous run of the sorted ids.
__global__ void k_pastry_tab_rule(const KeyRec* __restrict__ recs, uint32_t n, int b, int rows, KeyRec* __restrict__ tab)
{
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int P = 1 << b;
    if (g >= (uint64_t)n * (uint64_t)rows * (uint64_t)P) return;
    const uint32_t c = (uint32_t)(g % (uint64_t)P);
    const int r = (int)((g / (uint64_t)P) % (uint64_t)rows);
    const uint32_t v = (uint32_t)(g / ((uint64_t)P * (uint64_t)rows));
    const K160 me = rkey(recs, v);
    KeyRec e = empty_slot();
    const int p = 160 - (r + 1) * b;
    if (p >= 0 && p_digit(me, r, b) != c) {
        K160 dg;
        dg.w[0] = c ^ p_digit(me, r, b); dg.w[1] = dg.w[2] = dg.w[3] = dg.w[4] = 0;
        const K160 t = k_xor(me, b_shl(dg, p));
        const K160 base = b_shl(b_shr(t, p), p);
        const K160 top = k_add(base, k_pow2(p));
        const uint32_t lo = lower_bound(recs, 0, n, base);
        const uint32_t hi = k_lt(top, base) ? n : lower_bound(recs, lo, n, top);
        if (lo < hi) {
            const uint32_t i = lower_bound(recs, lo, hi, t);
            const uint32_t x = i < hi ? i : lo;
            e = load_rec(recs, x);
            e.aux = x;
        }
    }
    tab[g] = e;
}

// explicit node indices (validated on the host) into slots
__global__ void k_pastry_slots(const KeyRec* __restrict__ recs, uint32_t n, const uint32_t* __restrict__ idx, uint64_t total,
                               KeyRec* __restrict__ out)
{
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const uint32_t x = idx[g];
    KeyRec e = empty_slot();
    if (x < n) {
        e = load_rec(recs, x);
        e.aux = x;
    }
    out[g] = e;
}

__global__ void k_pastry_slot_nodes(const KeyRec* __restrict__ slots, uint64_t total, uint32_t* __restrict__ out)
{
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g < total) out[g] = load_rec(slots + g, 0).aux;
}

__global__ void k_pastry_rec(const KeyRec* __restrict__ recs, const double2* __restrict__ xy, uint32_t n, int rows, int P,
                             const KeyRec* __restrict__ tab, PastryRec* __restrict__ out)
{
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const K160 me = rkey(recs, v);
    const KeyRec* t = tab + (uint64_t)v * (uint64_t)rows * (uint64_t)P;
    int nr = 0;
    for (int s = 0; s < rows * P; ++s)
        if (load_rec(t, (uint32_t)s).aux != NONE) nr = s / P + 1;
    PastryRec o;
    for (int i = 0; i < 5; ++i) o.w[i] = me.w[i];
    o.nrows = (uint32_t)nr;
    o.pad0[0] = o.pad0[1] = 0;
    o.x = xy[v].x; o.y = xy[v].y;
    o.pad1[0] = o.pad1[1] = o.pad1[2] = o.pad1[3] = 0;
    out[v] = o;
}

__global__ void k_pastry_find_node(PView V, const uint32_t* __restrict__ node, const K160* __restrict__ keys, uint64_t nq,
                                   int nred, int nsib, uint32_t* __restrict__ out, uint32_t max_out, uint8_t* __restrict__ count,
                                   uint8_t* __restrict__ sib, uint8_t* __restrict__ status)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const uint32_t c = node[i];
    const PRec R = load_prec(V.rec, c);
    const K160 key = keys[i];
    const PAns a = pastry_find_node_dev(V, c, R, key, nsib);
    uint32_t* o = out + i * (uint64_t)max_out;
    for (uint32_t j = 0; j < max_out; ++j) o[j] = NONE;
    sib[i] = a.sib ? 1 : 0;
    status[i] = (uint8_t)((a.err ? 1 : 0) | (a.broken ? 2 : 0));
    uint32_t cnt = 0;
    if (!a.broken) {
        PIter it = iter_start();
        while (cnt < max_out) {
            const uint32_t x = answer_next(V, c, R, key, a, nred, nsib, it);
            if (x == NONE) break;
            o[cnt++] = x;
        }
    }
    count[i] = (uint8_t)cnt;
}

// ---------------------------------------------------------------------------
// the route

constexpr PersistTune KP_TUNE{0.70, 64};

// One lane per semi-recursive route message (BaseOverlay::sendToKey's recursive branch).
//
// ACKS: the route under routeMsgAcks (BaseOverlay.cc:1107-1146): every hop is a NextHopCall around the route message,
// and its receiver sends the NextHopResponse before it forwards (nextHopRpc, 1971-2000), so a forwarder's
// transmit queue holds the ack when the next call enters it (SimpleNodeEntry.cc:164-194: tx.finished =
// max(tx.finished, now) + bits / bandwidth) and the call leaves AC.bwAck late.  The source's queue is idle.  A
// node met twice has drained its queue long before: two hops lie between, each longer than ack plus call.  The
// sender of the call that arrives now forwarded iff hops > 1, so the lane carries only the largest ack round
// trip (sendUdpRpcCall to the response's arrival, the wait in the sender's own queue included) and the first
// hop whose round trip reached rpcUdpTimeout (a tie is a timeout, BaseRpc.cc:191-211).  The route record is the
// first copy's delivery; the re-route after a timeout (BaseOverlay.cc:1697-1757) is the caller's between batches.
// A route that fails part-way has sent, and had acknowledged, the calls of the hops it took: hops counts the
// NextHopCalls sent, each acknowledged by the time the lane ends.  Without ACKS neither AC nor aout is read; the
// two come last, so the plain instantiation finds its arguments where they were before the kernels were folded.
template <bool ACKS>
__global__ __launch_bounds__(256) void k_pastry_route(PView V, DelayConsts DC, int hcm, int nred, const K160* __restrict__ qkeys,
                                                      const uint32_t* __restrict__ qsrc, uint64_t nq, uint64_t chunk, PersistDyn dy,
                                                      ovs_route_out* __restrict__ out, uint32_t* __restrict__ hopseq,
                                                      PastryAckConsts AC, ovs_pastry_ack_out* __restrict__ aout)
{
    PersistFeed<KP_TUNE.dyn_chunk> feed(chunk, dy, nq);
    const uint64_t H = (uint64_t)max(hcm, 1);

    bool active = false, local = true;
    uint64_t q = 0;
    K160 K;
    K.w[0] = K.w[1] = K.w[2] = K.w[3] = K.w[4] = 0;
    uint32_t S = 0, cur = 0, last = NONE;
    double sx = 0, sy = 0;            // the last sender
    int64_t t = 0;
    [[maybe_unused]] int64_t rttmax = -1;       // ACKS: the largest ack round trip
    int hops = 0;
    [[maybe_unused]] uint32_t tohop = 0xFF;     // ACKS: the first hop whose ack timed out
    while (true) {
        if (feed.take(active, dy, nq, q)) {
            active = true;
            local = true;
            K = qkeys[q];
            S = qsrc[q];
            cur = S;
            last = NONE;
            t = 0; hops = 0;
            if constexpr (ACKS) { rttmax = -1; tohop = 0xFF; }
        }
        if (!__any(active)) break;
        if (!active) continue;

        const PRec Rc = load_prec(V.rec, cur);
        const PAns a = pastry_find_node_dev(V, cur, Rc, K, 1);
        uint8_t status = 0xFF;       // 0xFF = still running
        const bool at_src = local;
        if (!local) {
            const int64_t cd = coord_ns(sx, sy, Rc.x, Rc.y, DC.round);
            if constexpr (ACKS) {
                const int64_t d = (hops > 1 ? AC.bwAck : 0) + AC.msgCall + cd;      // the call, behind the sender's own ack
                const int64_t rtt = d + AC.msgAck + cd;                             // the ack leaves an idle queue
                t += d;
                rttmax = rtt > rttmax ? rtt : rttmax;
                if (rtt >= AC.timeout && tohop == 0xFF) tohop = (uint32_t)min(hops - 1, 0xFE);
            } else {
                t += DC.msgRoute + cd;   // sendRouteMessage
            }
        }
        local = false;
        sx = Rc.x; sy = Rc.y;
        // a forwarded message is delivered on receipt where this node is a sibling (BaseOverlay.cc:907-918); at the
        // source sendToKey runs first (1443-1582)
        if (!at_src && a.closest) status = OVS_LOOKUP_OK;
        else {
            const PStep st = pastry_send_to_key(V, cur, Rc, K, a, hops, hcm, nred, last, S);
            status = st.status;
            if (status == PSTEP_FORWARD) {
                if (hopseq) hopseq[q * H + (uint64_t)hops] = st.next;   // hops < hcm here
                ++hops;
                last = cur;
                cur = st.next;
            }
        }
        if (status != 0xFF) {
            ovs_route_out o;
            const bool ok = status == OVS_LOOKUP_OK;
            o.responsible = ok ? cur : NONE;
            o.hops = (uint16_t)(ok ? hops : 0);
            o.status = status;
            o.one_way_hops = (uint8_t)(ok ? hops : 0);
            o.latency_ns = ok ? t : -1;
            out[q] = o;
            if constexpr (ACKS) {
                if (aout) {
                    ovs_pastry_ack_out ao{};
                    ao.max_ack_rtt_ns = rttmax;
                    ao.acks = (uint16_t)hops;
                    ao.timeout_hop = (uint8_t)tohop;
                    aout[q] = ao;
                }
            }
            active = false;
        }
    }
}

// the ack records of routes without acks (routeMsgAcks = false)
__global__ void k_pastry_acks_none(uint64_t n, ovs_pastry_ack_out* __restrict__ aout)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    ovs_pastry_ack_out ao{};
    ao.max_ack_rtt_ns = -1;
    ao.timeout_hop = 0xFF;
    aout[i] = ao;
}

// The ack records of one-way messages under iterative routing: the final sendRouteMessage (BaseOverlay.cc:
// 1254-1257) is one NextHopCall from the source, whose queue the lookup left idle, to getResult()[0]; none where
// that is the source itself or the lookup failed.
__global__ void k_pastry_iter_acks(const ovs_route_out* __restrict__ rout, const uint32_t* __restrict__ src,
                                   const double2* __restrict__ xy, uint32_t nnodes, PastryAckConsts AC, int round, uint64_t n,
                                   ovs_pastry_ack_out* __restrict__ aout)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const ovs_route_out r = rout[i];
    const uint32_t s = src[i];
    ovs_pastry_ack_out ao{};
    ao.max_ack_rtt_ns = -1;
    ao.timeout_hop = 0xFF;
    if (r.status == OVS_LOOKUP_OK && r.responsible != s && r.responsible < nnodes && s < nnodes) {
        const double2 a = xy[s], b = xy[r.responsible];
        const int64_t rtt = AC.msgCall + AC.msgAck + 2 * coord_ns(a.x, a.y, b.x, b.y, round);
        ao.max_ack_rtt_ns = rtt;
        ao.acks = 1;
        if (rtt >= AC.timeout) ao.timeout_hop = 0;
    }
    aout[i] = ao;
}

// ---------------------------------------------------------------------------
// the iterative lookup

// Entry idx of the source's own findNode answer (IterativeLookup.cc:158-160: numRedundantNodes =
// getMaxNumRedundantNodes() = numberOfLeaves), NONE past its end; *seen: probe is among the entries before it.
// The path's start vector is that answer in its own order and unbounded (merge off: IterativePathLookup::add
// push_backs, 1189-1194), so it is walked again here, on the rare paths that look past its first entry,
// rather than kept.
__device__ uint32_t source_entry(const PView& V, uint32_t S, const K160& K, int nsib, int idx, uint32_t probe, bool* seen)
{
    const PRec Rs = load_prec(V.rec, S);
    const PAns as = pastry_find_node_dev(V, S, Rs, K, nsib);
    PIter it = iter_start();
    *seen = false;
    uint32_t x = NONE;
    for (int i = 0; i <= idx; ++i) {
        x = answer_next(V, S, Rs, K, as, V.sh.L, nsib, it);
        if (x == NONE) break;
        if (i < idx && x == probe) *seen = true;
    }
    return x;
}

// One lane per IterativeLookup on Pastry (IterativeLookup.cc with lookupRedundantNodes = lookupParallelPaths =
// lookupParallelRpcs = 1, merge off, visitOnlyOnce, finishOnFirstUnchanged off): one loop iteration is the
// source's local findNode (start, 133-244) or one FindNodeCall with its response or timeout.  lout: a LookupCall
// with nsib siblings (sibs: nq * nsib); rout: the KBRTestApp one-way message under iterative routing (nsib = 1),
// which adds the route message to getResult()[0] (BaseOverlay.cc:1240-1258).  hopseq (nq * hcm, hcm >= 1) holds
// the responders in order and is, with the source, the visited set.  Every call and every response carries the
// PastryFindNodeExtData object (BasePastry.cc:1212-1239, IterativeLookup.cc:385-388, BaseOverlay.cc:1903-1907;
// its bits are in DC); iterativeJoinHook (Pastry.cc:591-614) only counts joinHopCount in it for a lookup that is
// no join and changes no answer, so nothing of it is carried.
__global__ __launch_bounds__(256) void k_pastry_iter(PView V, DelayConsts DC, int hcm, int nsib, const K160* __restrict__ qkeys,
                                                     const uint32_t* __restrict__ qsrc, uint64_t nq, uint64_t chunk, PersistDyn dy,
                                                     ovs_route_out* __restrict__ rout, ovs_lookup_out* __restrict__ lout,
                                                     uint32_t* __restrict__ sibs, uint32_t* __restrict__ hopseq,
                                                     uint32_t* __restrict__ rpcs)
{
    PersistFeed<KP_TUNE.dyn_chunk> feed(chunk, dy, nq);
    const uint64_t H = (uint64_t)hcm;

    bool active = false, local = true, srcvec = false;
    uint64_t q = 0;
    K160 K;
    K.w[0] = K.w[1] = K.w[2] = K.w[3] = K.w[4] = 0;
    uint32_t S = 0, cur = 0, nrpc = 0;
    double sx = 0, sy = 0;            // the source
    int64_t t = 0;
    int hops = 0, ntry = 0, ndead = 0;
    while (true) {
        if (feed.take(active, dy, nq, q)) {
            active = true;
            local = true;
            srcvec = false;
            K = qkeys[q];
            S = qsrc[q];
            cur = S;
            t = 0; hops = 0; ntry = 0; ndead = 0; nrpc = 0;
        }
        if (!__any(active)) break;
        if (!active) continue;

        uint32_t* seq = hopseq + q * H;
        uint32_t* sv = sibs ? sibs + q * (uint64_t)nsib : nullptr;
        const PRec Rc = load_prec(V.rec, cur);
        const PAns a = pastry_find_node_dev(V, cur, Rc, K, nsib);
        uint8_t status = OVS_LOOKUP_OK;
        bool fin = false;
        uint32_t Rn = NONE, nx = NONE;
        int cnt = 0;                  // nodes in this answer
        bool walk = false;            // the path goes on with the start vector's next unused entry
        if (!a.broken) {
            PIter it = iter_start();
            if (a.sib) {
                // the sibling vector: the lookup's result where this answer is accepted (addSibling, 436-440)
                while (true) {
                    const uint32_t x = answer_next(V, cur, Rc, K, a, 1, nsib, it);
                    if (x == NONE) break;
                    if (cnt == 0) Rn = x;
                    if (sv) sv[cnt] = x;
                    ++cnt;
                }
            } else {
                nx = answer_next(V, cur, Rc, K, a, local ? V.sh.L : 1, nsib, it);
                cnt = nx != NONE ? 1 : 0;
            }
        }
        if (local) {
            // IterativeLookup::start (133-244); the source counts as visited (164)
            local = false;
            sx = Rc.x; sy = Rc.y;
            if (a.broken) { fin = true; status = OVS_LOOKUP_BROKEN; }
            else if (a.sib) fin = true;                                                // the key is local (186-195)
            else if (nx == NONE || nx == S) { fin = true; status = OVS_LOOKUP_NO_NEXT; }  // no next hops (167-170);
            else { cur = nx; ntry = 1; srcvec = true; }                                // the first entry is visited (1111)
        } else if (a.broken) {
            ++nrpc;
            fin = true; status = OVS_LOOKUP_BROKEN;    // the responder's findNode errors
        } else {
            // FindNodeCall S -> cur and its FindNodeResponse with cnt NodeHandles
            ++nrpc;
            const int64_t cd = coord_ns(sx, sy, Rc.x, Rc.y, DC.round);
            const int64_t rtt = DC.msgCall + resp_ns(DC, cnt) + 2 * cd;
            if (rtt >= DC.rpcTimeout) {
                // handleTimeout (935-1023): cur is dead; sendRpc goes on with the next unused next hop, and only
                // the start vector holds more than one: every response that names a node replaces them by it
                t += DC.rpcTimeout;
                cnt = 0;
                if (t > DC.lookupTimeout) { fin = true; status = OVS_LOOKUP_TIMEOUT; }
                else if (!srcvec) { fin = true; status = OVS_LOOKUP_RPC_TIMEOUT; }
                else { ++ndead; walk = true; status = OVS_LOOKUP_RPC_TIMEOUT; }
            } else {
                t += rtt;
                if (t > DC.lookupTimeout) { fin = true; status = OVS_LOOKUP_TIMEOUT; cnt = 0; }
                else {
                    // handleResponse (803-921); hops < hcm here: sendRpc checks it before every call
                    seq[hops] = cur;
                    ++hops;
                    if (a.sib) fin = true;                                             // 897-905
                    else if (hops >= hcm) { fin = true; status = OVS_LOOKUP_HOPMAX; }  // sendRpc (1074-1086)
                    else if (cnt == 0) {
                        // no node: the next hops stay as they are (839-846) and sendRpc tries the remaining ones
                        // (1095-1100); a response's single node is used up
                        if (srcvec) { walk = true; status = OVS_LOOKUP_NO_NEXT; }
                        else { fin = true; status = OVS_LOOKUP_NO_NEXT; }
                    } else {
                        // replace mode (841-843); visitOnlyOnce (1111): not the source, no earlier responder; nor
                        // a node that timed out (getNextEntry, 1172-1182): a start-vector entry tried and not visited
                        srcvec = false;
                        bool seen = nx == S;
                        for (int i = 0; i < hops && !seen; ++i) seen = seq[i] == nx;
                        if (seen) { fin = true; status = OVS_LOOKUP_NO_NEXT; }
                        else cur = nx;
                    }
                }
            }
        }
        if (walk || (!fin && ndead > 0 && !srcvec)) {
            bool dead;
            const uint32_t x = source_entry(V, S, K, nsib, ntry, walk ? NONE : cur, &dead);
            if (walk) {
                ++ntry;
                bool seen = x == NONE || x == S;
                for (int i = 0; i < hops && !seen; ++i) seen = seq[i] == x;
                if (seen) fin = true;                  // status: what the path was doing when it ran out
                else { cur = x; status = OVS_LOOKUP_OK; }
            } else if (dead) {
                fin = true; status = OVS_LOOKUP_NO_NEXT;
            }
        }
        if (fin) {
            const bool ok = status == OVS_LOOKUP_OK;
            if (!ok) cnt = 0;
            if (sv)
                for (int j = cnt; j < nsib; ++j) sv[j] = NONE;
            if (rout) {
                // the route message goes to getResult()[0]: the closest node the last responder knows, not always
                // that responder
                double rx = Rc.x, ry = Rc.y;
                if (ok && Rn != S && Rn != cur) {
                    const PRec Rr = load_prec(V.rec, Rn);
                    rx = Rr.x; ry = Rr.y;
                }
                rout[q] = iter_route_out(status, hops, t, Rn, S, sx, sy, rx, ry, DC);
            } else {
                ovs_lookup_out o;
                o.num_siblings = (uint32_t)cnt;
                o.hops = (uint16_t)hops;
                o.status = status;
                o.is_valid = ok ? 1 : 0;
                o.latency_ns = ok ? t : -1;
                lout[q] = o;
            }
            if (rpcs) rpcs[q] = nrpc;
            active = false;
        }
    }
}

hipError_t alloc_tables(uint32_t n, const PastryShape& sh, int rows, PastryTables& t)
{
    pastry_free(t);
    if (n < 2 || sh.b < 1 || sh.b > 4 || sh.L < 2 || sh.L > PASTRY_MAX_LEAVES || (sh.L & 1) || rows < 1 || rows > sh.max_rows())
        return hipErrorInvalidValue;
    t.n = n; t.sh = sh; t.rows = rows;
    hipError_t e = hipMalloc(&t.rec, sizeof(PastryRec) * (uint64_t)n);
    if (e != hipSuccess) return e;
    e = hipMalloc(&t.leaf, sizeof(KeyRec) * (uint64_t)n * (uint64_t)sh.L);
    if (e != hipSuccess) return e;
    return hipMalloc(&t.tab, sizeof(KeyRec) * (uint64_t)n * (uint64_t)rows * (uint64_t)sh.P());
}

hipError_t finish_build(const KeyRec* recs, const double2* xy, PastryTables& t, hipStream_t st)
{
    hipLaunchKernelGGL(k_pastry_rec, dim3(nblk(t.n, 256)), dim3(256), 0, st, recs, xy, t.n, t.rows, t.sh.P(), t.tab, t.rec);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return hipStreamSynchronize(st);
}

hipError_t launch_tab_rule(const KeyRec* recs, PastryTables& t, hipStream_t st)
{
    const uint64_t slots = (uint64_t)t.n * (uint64_t)t.rows * (uint64_t)t.sh.P();
    hipLaunchKernelGGL(k_pastry_tab_rule, dim3(nblk(slots, 256)), dim3(256), 0, st, recs, t.n, t.sh.b, t.rows, t.tab);
    return hipGetLastError();
}

}  // namespace

hipError_t pastry_rule_rows(const KeyRec* recs, uint32_t n, int b, int* rows, hipStream_t st)
{
    int* d = nullptr;
    hipError_t e = hipMalloc(&d, sizeof(int));
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(d, 0, sizeof(int), st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_pastry_max_rows, dim3(nblk(n, 256)), dim3(256), 0, st, recs, n, b, d);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(rows, d, sizeof(int), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    hipFree(d);
    return e;
}

hipError_t pastry_build(const KeyRec* recs, const double2* xy, uint32_t n, const PastryShape& sh, PastryTables& t, hipStream_t st)
{
    if ((uint64_t)n < (uint64_t)sh.L + 1) return hipErrorInvalidValue;
    int rows = 0;
    hipError_t e = pastry_rule_rows(recs, n, sh.b, &rows, st);
    if (e != hipSuccess) return e;
    e = alloc_tables(n, sh, rows, t);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_pastry_leaf_rule, dim3(nblk((uint64_t)n * (uint64_t)sh.L, 256)), dim3(256), 0, st, recs, n, sh.L, t.leaf);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = launch_tab_rule(recs, t, st);
    if (e != hipSuccess) return e;
    return finish_build(recs, xy, t, st);
}

hipError_t pastry_build_explicit(const KeyRec* recs, const double2* xy, uint32_t n, const PastryShape& sh, int rows,
                                 const uint32_t* dleaf, const uint32_t* dtab, PastryTables& t, hipStream_t st)
{
    hipError_t e = alloc_tables(n, sh, rows, t);
    if (e != hipSuccess) return e;
    const uint64_t nl = (uint64_t)n * (uint64_t)sh.L, ns = (uint64_t)n * (uint64_t)rows * (uint64_t)sh.P();
    hipLaunchKernelGGL(k_pastry_slots, dim3(nblk(nl, 256)), dim3(256), 0, st, recs, n, dleaf, nl, t.leaf);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (dtab) {
        hipLaunchKernelGGL(k_pastry_slots, dim3(nblk(ns, 256)), dim3(256), 0, st, recs, n, dtab, ns, t.tab);
        e = hipGetLastError();
    } else {
        e = launch_tab_rule(recs, t, st);
    }
    if (e != hipSuccess) return e;
    return finish_build(recs, xy, t, st);
}

hipError_t pastry_slot_nodes(const PastryTables& t, uint32_t* dleaf, uint32_t* dtab, hipStream_t st)
{
    const uint64_t nl = (uint64_t)t.n * (uint64_t)t.sh.L, ns = (uint64_t)t.n * (uint64_t)t.rows * (uint64_t)t.sh.P();
    hipLaunchKernelGGL(k_pastry_slot_nodes, dim3(nblk(nl, 256)), dim3(256), 0, st, t.leaf, nl, dleaf);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_pastry_slot_nodes, dim3(nblk(ns, 256)), dim3(256), 0, st, t.tab, ns, dtab);
    return hipGetLastError();
}

hipError_t pastry_find_node(const PastryTables& t, const uint32_t* node, const K160* keys, uint64_t nq, int numRedundantNodes,
                            int numSiblings, uint32_t* out_nodes, uint32_t max_out, uint8_t* count, uint8_t* sib,
                            uint8_t* status, hipStream_t st)
{
    if (nq == 0) return hipSuccess;
    hipLaunchKernelGGL(k_pastry_find_node, dim3(nblk(nq, 128)), dim3(128), 0, st, make_view(t), node, keys, nq, numRedundantNodes,
                       numSiblings, out_nodes, max_out, count, sib, status);
    return hipGetLastError();
}

hipError_t pastry_route(const PastryTables& t, const DelayConsts& DC, const PastryAckConsts* AC, int hopCountMax,
                        int recNumRedundantNodes, const K160* keys, const uint32_t* src, uint64_t nq, ovs_route_out* out,
                        ovs_pastry_ack_out* ack_out, uint32_t* hopseq, int num_cu, hipStream_t st, unsigned long long* dyn)
{
    if (nq == 0) return hipSuccess;
    if (!AC && ack_out) return hipErrorInvalidValue;
    auto launch = [&](auto k) {
        using K = decltype(k);
        const PersistLaunch pl = persist_launch<K::fn>(nq, num_cu, dyn, KP_TUNE);
        hipLaunchKernelGGL(K::fn, dim3(pl.blocks), dim3(256), 0, st, make_view(t), DC, hopCountMax, recNumRedundantNodes, keys, src, nq,
                           pl.chunk, pl.dy, out, hopseq, AC ? *AC : PastryAckConsts{}, ack_out);
    };
    if (AC) launch(PersistKernel<k_pastry_route<true>>{}); else launch(PersistKernel<k_pastry_route<false>>{});
    return hipGetLastError();
}

hipError_t pastry_acks_none(uint64_t nq, ovs_pastry_ack_out* ack_out, hipStream_t st)
{
    if (nq == 0) return hipSuccess;
    hipLaunchKernelGGL(k_pastry_acks_none, dim3(nblk(nq, 256)), dim3(256), 0, st, nq, ack_out);
    return hipGetLastError();
}

hipError_t pastry_iter_acks(const ovs_route_out* rout, const uint32_t* src, const double2* xy, uint32_t n, const PastryAckConsts& AC,
                            int round, uint64_t nq, ovs_pastry_ack_out* ack_out, hipStream_t st)
{
    if (nq == 0) return hipSuccess;
    hipLaunchKernelGGL(k_pastry_iter_acks, dim3(nblk(nq, 256)), dim3(256), 0, st, rout, src, xy, n, AC, round, nq, ack_out);
    return hipGetLastError();
}

hipError_t pastry_iter(const PastryTables& t, const DelayConsts& DC, int hopCountMax, int numSiblings, const K160* keys,
                       const uint32_t* src, uint64_t nq, ovs_route_out* rout, ovs_lookup_out* lout, uint32_t* siblings,
                       uint32_t* hopseq, uint32_t* rpcs, int num_cu, hipStream_t st, unsigned long long* dyn)
{
    if (nq == 0) return hipSuccess;
    // the hop list holds hopCountMax responders and is the visitOnlyOnce list: no limit, no list
    if (!hopseq || hopCountMax < 1 || numSiblings < 1 || numSiblings > t.sh.L / 2 || !rout == !lout || (rout && numSiblings != 1))
        return hipErrorInvalidValue;
    using K = PersistKernel<k_pastry_iter>;
    const PersistLaunch pl = persist_launch<K::fn>(nq, num_cu, dyn, KP_TUNE);
    hipLaunchKernelGGL(K::fn, dim3(pl.blocks), dim3(256), 0, st, make_view(t), DC, hopCountMax, numSiblings, keys, src, nq, pl.chunk,
                       pl.dy, rout, lout, siblings, hopseq, rpcs);
    return hipGetLastError();
}

}  // namespace ovs
