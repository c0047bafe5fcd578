// dht.hip -- DHT tier (src/applications/dht/DHT.cc): the replica phase of batched puts and gets on a stable
// network, and the per-node data storage as one open-addressing table in global memory.
//
// Reference: DHT::handleLookupResponse (DHT.cc:832-958), handlePutRequest / handleGetRequest (298-497),
// handlePutResponse / handleGetResponse (553-715), handleRpcTimeout (157-294), the message lengths of
// DHTMessage.msg:30-41 over CommonMessages.msg:28-76, BaseOverlay::route's direct UDP send
// (BaseOverlay.cc:1340-1341), SimpleNodeEntry::calcDelay with its transmit queue (SimpleNodeEntry.cc:155-195),
// SimpleUDP's no-delay delivery to the sending host (SimpleUDP.cc:320-345), DHTDataStorage.cc:155-243.
//
// The lookup phase is ovs_lookup_batch's launch.  Every kernel here runs one lane per operation or per
// (operation, replica) pair, grid-stride or one element per lane; no lane waits for another one and every
// probe loop is bounded by the table's capacity.
//   k_dht_put_plan   per put: the DHTPutCalls back to back through the source's transmit queue, each
//                    replica's arrival and response, the majority rule; counts, reading only, the pairs whose
//                    entry has no slot yet.
//   k_dht_put_claim  per pair: finds or claims the slot (a 64-bit CAS on its tag), atomicMax of the arrival.
//   k_dht_put_op     per pair: among the puts of the latest arrival, atomicMax of the operation index.
//   k_dht_put_write  per pair: the winner writes the payload (plain vector stores).
//   k_dht_put_reset  per pair: clears the arbitration words; k_dht_put_end closes the batch.
//   k_dht_get        per get: the event loop of handleGetResponse / handleRpcTimeout over at most 8 hash and
//                    8 value RPCs, whose per-lane event list lives in LDS ([rpc][lane], dynamically indexed
//                    there, so nothing spills to scratch).
// All stores to memory are ordinary vector stores and atomics.
#include <hip/hip_runtime.h>

#include "dht_dev.hpp"

namespace ovs {

namespace {

constexpr int64_t NEVER = DHT_NEVER;

__global__ __launch_bounds__(256) void k_dht_put_plan(DhtStore st, DhtConsts C, const ovs_lookup_out* __restrict__ look,
                                                      const uint32_t* __restrict__ sib, const K160* __restrict__ keys,
                                                      const uint32_t* __restrict__ src,
                                                      const ovs_dht_op* __restrict__ ops,
                                                      const double2* __restrict__ xy, uint64_t n,
                                                      ovs_dht_put_out* __restrict__ out, long long* __restrict__ pair_t)
{
    uint64_t need = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const ovs_lookup_out L = look[i];
        const ovs_dht_op op = ops[i];
        const uint32_t S = src[i] < C.nnodes ? src[i] : 0u;   // device-pointer calls do not check sources
        ovs_dht_put_out o{};
        o.status = L.status;
        int m = (int)(L.num_siblings < (uint32_t)C.R ? L.num_siblings : (uint32_t)C.R);
        if (!L.is_valid || L.status != OVS_LOOKUP_OK) m = 0;
        if (m == 0) {                                         // DHT.cc:852-864
            o.outcome = OVS_DHT_LOOKUP_FAILED;
            o.latency_ns = -1;
#pragma unroll
            for (int j = 0; j < DHT_MAXR; ++j)
                if (j < C.R) pair_t[i * C.R + j] = -1;
            out[i] = o;
            continue;
        }
        o.hop_count = L.hops;                                 // DHT.cc:866-867
        const int64_t t = op.t0_ns + L.latency_ns;
        const int call_bits = BASERPC_BITS + C.auth + (int)op.vlen + ENTRY_BITS;      // PUTCALL_L
        const int resp_bits = BASERPC_BITS + C.auth + 8;                              // PUTRESPONSE_L
        const K160 key = keys[i];
        int64_t txfin = 0;                                    // the source's queue is idle when the lookup completes
        int64_t ev[DHT_MAXR];                                 // statically indexed: registers
        int nresp = 0;
#pragma unroll
        for (int j = 0; j < DHT_MAXR; ++j) {                  // DHT.cc:876-891
            ev[j] = NEVER;
            if (j >= C.R) continue;
            if (j >= m) { pair_t[i * C.R + j] = -1; continue; }
            uint32_t r = sib[i * C.R + j];
            if (r >= C.nnodes) r = S;
            const int64_t a = dht_send(txfin, S, r, wire_bytes(call_bits), t, xy, C);
            pair_t[i * C.R + j] = a;
            if (dht_find(st, entry_tag(r, key, op.kind, op.id)) == NONE) ++need;
            int64_t rfin = 0;                                 // the replica sends nothing else of this operation
            const int64_t back = dht_send(rfin, r, S, wire_bytes(resp_bits), a, xy, C);
            if (back - t < C.timeout) { ev[j] = back; ++nresp; }      // else: the timeout, scheduled first, at t + timeout
        }
        o.num_sent = (uint8_t)m;
        o.messages = (uint16_t)(2 * m);
        o.bytes = (uint32_t)(m * (bits_bytes(call_bits) + bits_bytes(resp_bits)));
        const int want = m / 2 + 1;                           // numResponses / numSent > 0.5 (DHT.cc:568)
        if (nresp >= want) {
            // the arrival of the want-th response in (time, send order)
            int64_t when = NEVER;
#pragma unroll
            for (int j = 0; j < DHT_MAXR; ++j) {
                int rank = 0;
#pragma unroll
                for (int l = 0; l < DHT_MAXR; ++l)
                    rank += (ev[l] < ev[j] || (ev[l] == ev[j] && l < j)) ? 1 : 0;
                if (ev[j] != NEVER && rank == want - 1) when = ev[j];
            }
            o.outcome = OVS_DHT_SUCCESS;
            o.num_responses = (uint8_t)want;
            o.latency_ns = when - op.t0_ns;
        } else {
            // every response in time came before the timeouts, which all fire at t + timeout: the put fails at
            // the one that makes numFailed / numSent >= 0.5 (DHT.cc:172-180)
            o.outcome = OVS_DHT_FAILED;
            o.num_responses = (uint8_t)nresp;
            o.latency_ns = t + C.timeout - op.t0_ns;
        }
        out[i] = o;
    }
    need = wave_sum_u64(need);
    if ((threadIdx.x & 63) == 0 && need) atomicAdd(&st.hdr->need, (unsigned long long)need);
}

__device__ __forceinline__ bool batch_fits(const DhtStore& st)
{
    return st.hdr->used_prev + st.hdr->need <= st.cap;
}

__global__ __launch_bounds__(256) void k_dht_put_claim(DhtStore st, DhtConsts C, const uint32_t* __restrict__ sib,
                                                       const K160* __restrict__ keys,
                                                       const ovs_dht_op* __restrict__ ops, uint64_t npairs,
                                                       const long long* __restrict__ pair_t,
                                                       uint32_t* __restrict__ pair_slot)
{
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npairs) return;
    pair_slot[p] = NONE;
    const long long a = pair_t[p];
    if (a < 0 || !batch_fits(st)) return;
    const uint64_t i = p / (uint64_t)C.R;
    const uint32_t r = sib[p];
    if (r >= C.nnodes) return;
    const K160 key = keys[i];
    const ovs_dht_op op = ops[i];
    const uint64_t tag = entry_tag(r, key, op.kind, op.id);
    uint64_t q = tag % st.cap;
    for (uint64_t step = 0; step < st.cap; ++step) {
        DhtSlot* sl = &st.slots[q];
        unsigned long long cur = __hip_atomic_load(&sl->tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0) {
            cur = atomicCAS(&sl->tag, 0ull, (unsigned long long)tag);
            if (cur == 0) {
                // this lane claimed the slot: the entry's identity (every later reader is in a later launch)
#pragma unroll
                for (int w = 0; w < 5; ++w) sl->key[w] = key.w[w];
                sl->kind = op.kind; sl->id = op.id; sl->node = r;
                atomicAdd(&st.hdr->used, 1ull);
                cur = tag;
            }
        }
        if (cur == tag) {
            atomicMax(&sl->arb_t, (unsigned long long)a + 1);
            pair_slot[p] = (uint32_t)q;
            return;
        }
        q = q + 1 == st.cap ? 0 : q + 1;
    }
}

__global__ __launch_bounds__(256) void k_dht_put_op(DhtStore st, DhtConsts C, uint64_t npairs,
                                                    const long long* __restrict__ pair_t,
                                                    const uint32_t* __restrict__ pair_slot)
{
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npairs) return;
    const uint32_t q = pair_slot[p];
    if (q == NONE) return;
    DhtSlot* sl = &st.slots[q];
    if (sl->arb_t == (unsigned long long)pair_t[p] + 1) atomicMax(&sl->arb_op, p / (uint64_t)C.R + 1);
}

__global__ __launch_bounds__(256) void k_dht_put_write(DhtStore st, DhtConsts C, const uint32_t* __restrict__ sib,
                                                       const K160* __restrict__ keys,
                                                       const ovs_dht_op* __restrict__ ops, uint64_t npairs,
                                                       const long long* __restrict__ pair_t,
                                                       const uint32_t* __restrict__ pair_slot)
{
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npairs) return;
    const uint32_t q = pair_slot[p];
    if (q == NONE) return;
    const uint64_t i = p / (uint64_t)C.R;
    DhtSlot* sl = &st.slots[q];
    const long long a = pair_t[p];
    if (sl->arb_t != (unsigned long long)a + 1 || sl->arb_op != i + 1) return;
    const ovs_dht_op op = ops[i];
    if (!slot_is(sl, sib[p], keys[i], op.kind, op.id)) {      // another entry with this tag holds the slot
        atomicAdd(&st.hdr->collisions, 1ull);
        return;
    }
    // DHT.cc:399-419: removeData, then addData when the value is not empty; the TTL timer at arrival + ttl
    sl->token = op.vlen ? op.token : 0;
    sl->vlen = op.vlen;
    sl->expiry = op.ttl > 0 ? a + (long long)op.ttl * 1000000000ll : NEVER;
    sl->ins_batch = (uint32_t)st.hdr->batch;
    sl->ins_op = (uint32_t)i;
    sl->ins_t = a;
}

__global__ __launch_bounds__(256) void k_dht_put_reset(DhtStore st, uint64_t npairs,
                                                       const uint32_t* __restrict__ pair_slot)
{
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npairs) return;
    const uint32_t q = pair_slot[p];
    if (q == NONE) return;
    st.slots[q].arb_t = 0;
    st.slots[q].arb_op = 0;
}

__global__ void k_dht_put_end(DhtStore st)
{
    if (blockIdx.x || threadIdx.x) return;
    DhtHeader* h = st.hdr;
    const bool fits = h->used_prev + h->need <= st.cap;
    h->last_refused = fits ? 0 : 1;
    h->refused += fits ? 0 : 1;
    h->last_collisions = h->collisions - h->coll_prev;
    h->coll_prev = h->collisions;
    h->used_prev = h->used;
    h->need = 0;
    h->batch += 1;
}

// ---------------------------------------------------------------- get
constexpr int GET_LANES = 64;
constexpr int GET_RPCS = 2 * DHT_MAXR;

struct GetLds {
    long long ev[GET_RPCS][GET_LANES];              // event time; NEVER once handled
    unsigned long long tok[GET_RPCS][GET_LANES];    // the answering entry's token
    uint32_t vlen[GET_RPCS][GET_LANES];
    uint32_t info[GET_RPCS][GET_LANES];             // bits 0-2 sibling slot, 3 isHash, 4 timeout, 5 entry present
    uint32_t resp[DHT_MAXR][GET_LANES];             // hash responses in arrival order: rpc index, bit 8 popped
};

__global__ __launch_bounds__(GET_LANES) void k_dht_get(DhtStore st, DhtConsts C, const ovs_lookup_out* __restrict__ look,
                                                       const uint32_t* __restrict__ sib, const K160* __restrict__ keys,
                                                       const uint32_t* __restrict__ src,
                                                       const ovs_dht_op* __restrict__ ops,
                                                       const double2* __restrict__ xy, uint64_t n,
                                                       ovs_dht_get_out* __restrict__ out)
{
    __shared__ GetLds M;
    const int ln = threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * GET_LANES;
    for (uint64_t i = (uint64_t)blockIdx.x * GET_LANES + ln; i < n; i += stride) {
        const ovs_lookup_out L = look[i];
        const ovs_dht_op op = ops[i];
        const uint32_t S = src[i] < C.nnodes ? src[i] : 0u;
        ovs_dht_get_out o{};
        o.status = L.status;
        o.server = NONE;
        int m = (int)(L.num_siblings < (uint32_t)C.R ? L.num_siblings : (uint32_t)C.R);
        if (!L.is_valid || L.status != OVS_LOOKUP_OK) m = 0;
        if (m == 0) {                                         // DHT.cc:910-927
            o.outcome = OVS_DHT_LOOKUP_FAILED;
            o.latency_ns = -1;
            out[i] = o;
            continue;
        }
        o.hop_count = L.hops;                                 // DHT.cc:929-930
        const K160 key = keys[i];
        const int64_t t = op.t0_ns + L.latency_ns;
        const uint32_t* row = sib + i * C.R;
        int64_t txfin = 0;                                    // the source's transmit queue
        int nrpc = 0, nr = 0, msgs = 0;
        uint32_t bytes = 0;
        int nreplica = m;                                     // `replica` = row[G, nreplica): back() is row[nreplica - 1]
        bool value_sent = false, chosen_set = false, chosen_has = false;
        unsigned long long chosen_tok = 0;
        int nresp = 0;

        auto node_of = [&](int slot) { const uint32_t r = row[slot]; return r < C.nnodes ? r : S; };
        auto send = [&](int slot, bool is_hash, int64_t now) {
            if (nrpc >= GET_RPCS) return;                     // cannot happen: at most 8 hash and 8 value requests
            const uint32_t r = node_of(slot);
            const int64_t a = dht_send(txfin, S, r, wire_bytes(GETCALL_BITS), now, xy, C);
            const uint32_t q = dht_find(st, entry_tag(r, key, op.kind, op.id));     // DHT.cc:441-443
            bool has = false;
            unsigned long long tk = 0;
            uint32_t vl = 0;
            if (q != NONE) {
                const DhtSlot* sl = &st.slots[q];
                if (slot_is(sl, r, key, op.kind, op.id) && sl->vlen > 0 && sl->expiry > a) {
                    has = true; tk = sl->token; vl = sl->vlen;
                }
            }
            // GETRESPONSE_L: no entry (DHT.cc:462-464), the hash (466-481), the result array (483-487)
            const int bits = BASERPC_BITS + C.auth + 160 + (!has ? 0 : is_hash ? HASH_BITS : (int)vl + ENTRY_BITS);
            int64_t rfin = 0;                                 // the replica's queue: its earlier response reached the source
            const int64_t back = dht_send(rfin, r, S, wire_bytes(bits), a, xy, C);
            msgs += 2;
            bytes += (uint32_t)(bits_bytes(GETCALL_BITS) + bits_bytes(bits));
            const bool tmo = back - now >= C.timeout;         // the timeout was scheduled when the call was sent
            M.ev[nrpc][ln] = tmo ? now + C.timeout : back;
            M.tok[nrpc][ln] = tk;
            M.vlen[nrpc][ln] = vl;
            M.info[nrpc][ln] = (uint32_t)slot | (is_hash ? 8u : 0u) | (tmo ? 16u : 0u) | (has ? 32u : 0u);
            ++nrpc;
        };
        auto same_hash = [&](int k, bool has, unsigned long long tk) {
            const bool h = (M.info[k][ln] & 32u) != 0;
            return h == has && (!h || M.tok[k][ln] == tk);
        };
        auto size_of = [&](bool has, unsigned long long tk) {
            int c = 0;
            for (int x = 0; x < nr; ++x) {
                const uint32_t e = M.resp[x][ln];
                if (!(e & 256u) && same_hash((int)(e & 255u), has, tk)) ++c;
            }
            return c;
        };
        // the first hash in map order (no entry first, then ascending token) with the strictly largest vector
        // (DHT.cc:244-254, 623-633); returns its size, 0: none
        auto majority = [&](bool& bhas, unsigned long long& btok) {
            int best = 0;
            for (int x = 0; x < nr; ++x) {
                const uint32_t e = M.resp[x][ln];
                if (e & 256u) continue;
                const int k = (int)(e & 255u);
                const bool h = (M.info[k][ln] & 32u) != 0;
                const unsigned long long tk = h ? M.tok[k][ln] : 0;
                const int c = size_of(h, tk);
                const bool before = (!h && bhas) || (h == bhas && tk < btok);
                if (c > best || (c == best && best > 0 && before)) { best = c; bhas = h; btok = tk; }
            }
            return best;
        };
        auto pop_back = [&](bool has, unsigned long long tk) {           // hashVector->back(), pop_back()
            for (int x = nr - 1; x >= 0; --x) {
                const uint32_t e = M.resp[x][ln];
                if (!(e & 256u) && same_hash((int)(e & 255u), has, tk)) {
                    M.resp[x][ln] = e | 256u;
                    return (int)(M.info[e & 255u][ln] & 7u);
                }
            }
            return 0;
        };
        auto done = [&](uint8_t outcome, int64_t now) {
            o.outcome = outcome;
            o.latency_ns = now - op.t0_ns;
        };

        const int first = m < C.G ? m : C.G;
        for (int j = 0; j < first; ++j) send(j, true, t);     // DHT.cc:934-946
        o.num_sent = (uint8_t)first;
        bool finished = false;
        for (int guard = 0; guard < GET_RPCS && !finished; ++guard) {
            // the next event: arrival order, ties by send order
            int k = -1;
            long long now = NEVER;
            for (int x = 0; x < nrpc; ++x) {
                const long long e = M.ev[x][ln];
                if (e < now) { now = e; k = x; }
            }
            if (k < 0) break;
            M.ev[k][ln] = NEVER;
            const uint32_t inf = M.info[k][ln];
            const bool is_hash = (inf & 8u) != 0;
            if (inf & 16u) {                                  // DHT.cc:184-294
                if (value_sent) {
                    if (chosen_set && size_of(chosen_has, chosen_tok) > 0) {          // 198-212
                        send(pop_back(chosen_has, chosen_tok), false, now);
                    } else {                                  // 213-221
                        done(OVS_DHT_FAILED, now); finished = true;
                    }
                } else if (nreplica > C.G) {                  // 226-240
                    send(--nreplica, true, now);
                } else {
                    if (nresp > 0) {                          // 243-259
                        bool bh = false; unsigned long long bt = 0;
                        chosen_set = majority(bh, bt) > 0;
                        chosen_has = bh; chosen_tok = bt;
                    }
                    if (chosen_set && size_of(chosen_has, chosen_tok) > 0) {          // 268-282: the state stays
                        send(pop_back(chosen_has, chosen_tok), false, now);
                    } else {                                  // 283-290
                        done(OVS_DHT_FAILED, now); finished = true;
                    }
                }
                continue;
            }
            if (value_sent && !is_hash) {                     // DHT.cc:585-598: also with an empty result array
                done(OVS_DHT_SUCCESS, now); finished = true;
                o.server = node_of((int)(inf & 7u));
                if (inf & 32u) { o.result_count = 1; o.value_token = M.tok[k][ln]; o.value_len = M.vlen[k][ln]; }
                continue;
            }
            if (is_hash) {                                    // DHT.cc:601-684
                if (nr < DHT_MAXR) M.resp[nr++][ln] = (uint32_t)k;
                ++nresp;
                if (value_sent) continue;                     // 617-620
                bool bh = false; unsigned long long bt = 0;
                const int cnt = majority(bh, bt);
                if ((double)cnt / (double)m >= C.ratio) {     // 635-637 (numAvailableReplica = m, 953)
                    chosen_set = cnt > 0; chosen_has = bh; chosen_tok = bt;
                } else if (nresp >= C.G) {                    // 638
                    if (nreplica > C.G) {                     // 640-653
                        send(--nreplica, true, now);
                    } else if (cnt == 0) {                    // 654-678
                        done(OVS_DHT_FAILED, now); finished = true;
                        continue;
                    } else {                                  // 679-682
                        chosen_set = true; chosen_has = bh; chosen_tok = bt;
                    }
                }
            }
            if (!value_sent && chosen_set) {                  // DHT.cc:686-714
                if (size_of(chosen_has, chosen_tok) > 0) {
                    send(pop_back(chosen_has, chosen_tok), false, now);
                    value_sent = true;
                } else {
                    done(OVS_DHT_FAILED, now); finished = true;
                }
            }
        }
        if (!finished) { o.outcome = OVS_DHT_FAILED; o.latency_ns = -1; }   // cannot happen: every pending RPC has an event
        o.num_responses = (uint8_t)nresp;
        o.messages = (uint16_t)msgs;
        o.bytes = bytes;
        out[i] = o;
    }
}

// ---------------------------------------------------------------- DHTTestApp statistics
__device__ __forceinline__ void add_lat(unsigned long long* sum, unsigned long long* lo, unsigned long long* hi,
                                        unsigned long long* mn, unsigned long long* mx, uint64_t l)
{
    atomicAdd(sum, (unsigned long long)l);
    const uint64_t vlo = l * l, vhi = __umul64hi(l, l);
    const unsigned long long old = atomicAdd(lo, (unsigned long long)vlo);
    const unsigned long long carry = old + vlo < old ? 1ull : 0ull;       // this addition wrapped the low word
    if (vhi + carry) atomicAdd(hi, (unsigned long long)(vhi + carry));
    atomicMin(mn, (unsigned long long)l);
    atomicMax(mx, (unsigned long long)l);
}

__global__ __launch_bounds__(256) void k_dhttest_stats(const ovs_dht_put_out* __restrict__ put_out,
                                                       const uint32_t* __restrict__ put_src, uint64_t n_put,
                                                       const ovs_dht_get_out* __restrict__ get_out,
                                                       const ovs_dht_op* __restrict__ get_ops,
                                                       const uint32_t* __restrict__ get_src,
                                                       const ovs_dhttest_expect* __restrict__ expect, uint64_t n_get,
                                                       uint32_t nnodes, DhtStatsDev* __restrict__ S,
                                                       uint32_t* __restrict__ nc)
{
    uint64_t pok = 0, perr = 0, gok = 0, gerr = 0, phn = 0, ph = 0, ghn = 0, gh = 0, msgs = 0, bytes = 0, gln = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_put + n_get; i += stride) {
        if (i < n_put) {
            const ovs_dht_put_out o = put_out[i];
            const uint32_t s = put_src[i];
            msgs += o.messages; bytes += o.bytes;
            if (o.outcome != OVS_DHT_LOOKUP_FAILED) { ++phn; ph += o.hop_count; }     // DHT.cc:866-867
            const bool ok = o.outcome == OVS_DHT_SUCCESS;                             // DHTTestApp.cc:161-167
            if (ok) { ++pok; add_lat(&S->put_lat, &S->put_sq_lo, &S->put_sq_hi, &S->put_min, &S->put_max, (uint64_t)o.latency_ns); }
            else ++perr;
            if (s < nnodes) atomicAdd(&nc[(ok ? 0ull : 1ull) * nnodes + s], 1u);
            continue;
        }
        const uint64_t j = i - n_put;
        const ovs_dht_get_out o = get_out[j];
        const uint32_t s = get_src[j];
        msgs += o.messages; bytes += o.bytes;
        if (o.outcome != OVS_DHT_LOOKUP_FAILED) { ++ghn; gh += o.hop_count; }         // DHT.cc:929-930
        bool ok = false;
        if (o.latency_ns >= 0) {                                                      // DHTTestApp.cc:182-183
            ++gln;
            add_lat(&S->get_lat, &S->get_sq_lo, &S->get_sq_hi, &S->get_min, &S->get_max, (uint64_t)o.latency_ns);
        }
        if (o.outcome == OVS_DHT_SUCCESS) {                                           // DHTTestApp.cc:185-190
            const ovs_dhttest_expect e = expect[j];
            const int64_t now = get_ops[j].t0_ns + o.latency_ns;
            if (!e.known) ok = false;                                                 // 194-200
            else if (now > e.endtime_ns) ok = o.result_count == 0;                    // 202-216
            else ok = o.result_count > 0 && o.value_token == e.token;                 // 219-231
        }
        if (ok) ++gok; else ++gerr;
        if (s < nnodes) atomicAdd(&nc[(ok ? 2ull : 3ull) * nnodes + s], 1u);
    }
    pok = wave_sum_u64(pok); perr = wave_sum_u64(perr); gok = wave_sum_u64(gok); gerr = wave_sum_u64(gerr);
    phn = wave_sum_u64(phn); ph = wave_sum_u64(ph); ghn = wave_sum_u64(ghn); gh = wave_sum_u64(gh);
    msgs = wave_sum_u64(msgs); bytes = wave_sum_u64(bytes); gln = wave_sum_u64(gln);
    if ((threadIdx.x & 63) == 0) {
        if (pok) atomicAdd(&S->put_ok, (unsigned long long)pok);
        if (perr) atomicAdd(&S->put_err, (unsigned long long)perr);
        if (gok) atomicAdd(&S->get_ok, (unsigned long long)gok);
        if (gerr) atomicAdd(&S->get_err, (unsigned long long)gerr);
        if (phn) atomicAdd(&S->put_hop_n, (unsigned long long)phn);
        if (ph) atomicAdd(&S->put_hop, (unsigned long long)ph);
        if (ghn) atomicAdd(&S->get_hop_n, (unsigned long long)ghn);
        if (gh) atomicAdd(&S->get_hop, (unsigned long long)gh);
        if (msgs) atomicAdd(&S->msgs, (unsigned long long)msgs);
        if (bytes) atomicAdd(&S->bytes, (unsigned long long)bytes);
        if (gln) atomicAdd(&S->get_lat_n, (unsigned long long)gln);
    }
}

}  // namespace

hipError_t launch_dht_put_plan(const DhtStore& st, const DhtConsts& C, const ovs_lookup_out* look, const uint32_t* sib,
                               const K160* keys, const uint32_t* src, const ovs_dht_op* ops, const double2* xy, uint64_t n,
                               ovs_dht_put_out* out, long long* pair_t, int num_cu, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    if (!st.slots || !st.cap || C.R < 1 || C.R > DHT_MAXR || C.nnodes == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_dht_put_plan, dim3(capped_grid(n, 256, num_cu, 8)), dim3(256), 0, s, st, C, look, sib, keys, src,
                       ops, xy, n, out, pair_t);
    return hipGetLastError();
}

hipError_t launch_dht_put_apply(const DhtStore& st, const DhtConsts& C, const uint32_t* sib, const K160* keys,
                                const ovs_dht_op* ops, uint64_t n, const long long* pair_t, uint32_t* pair_slot, int num_cu,
                                hipStream_t s)
{
    (void)num_cu;
    if (!st.slots || !st.cap) return hipErrorInvalidValue;
    const uint64_t np = n * (uint64_t)C.R;
    if (np) {
        const uint64_t blocks = blocks256(np);
        if (!grid_ok(blocks)) return hipErrorInvalidValue;
        const dim3 g((unsigned)blocks), b(256);
        hipLaunchKernelGGL(k_dht_put_claim, g, b, 0, s, st, C, sib, keys, ops, np, pair_t, pair_slot);
        hipLaunchKernelGGL(k_dht_put_op, g, b, 0, s, st, C, np, pair_t, pair_slot);
        hipLaunchKernelGGL(k_dht_put_write, g, b, 0, s, st, C, sib, keys, ops, np, pair_t, pair_slot);
        hipLaunchKernelGGL(k_dht_put_reset, g, b, 0, s, st, np, pair_slot);
    }
    hipLaunchKernelGGL(k_dht_put_end, dim3(1), dim3(64), 0, s, st);
    return hipGetLastError();
}

hipError_t launch_dht_get(const DhtStore& st, const DhtConsts& C, const ovs_lookup_out* look, const uint32_t* sib,
                          const K160* keys, const uint32_t* src, const ovs_dht_op* ops, const double2* xy, uint64_t n,
                          ovs_dht_get_out* out, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    if (!st.slots || !st.cap || C.R < 1 || C.R > DHT_MAXR || C.G < 1 || C.G > DHT_MAXR || C.nnodes == 0)
        return hipErrorInvalidValue;
    uint64_t blocks = (n + GET_LANES - 1) / GET_LANES;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(k_dht_get, dim3((unsigned)blocks), dim3(GET_LANES), 0, s, st, C, look, sib, keys, src, ops, xy, n,
                       out);
    return hipGetLastError();
}

hipError_t launch_dhttest_stats(const ovs_dht_put_out* put_out, const uint32_t* put_src, uint64_t n_put,
                                const ovs_dht_get_out* get_out, const ovs_dht_op* get_ops, const uint32_t* get_src,
                                const ovs_dhttest_expect* expect, uint64_t n_get, uint32_t nnodes, DhtStatsDev* S,
                                uint32_t* node_counts, int num_cu, hipStream_t s)
{
    DhtStatsDev init{};
    init.put_min = ~0ull;
    init.get_min = ~0ull;
    const hipError_t e = stats_prelude(node_counts, 4, nnodes, S, init, s);
    if (e != hipSuccess) return e;
    if (n_put + n_get == 0) return hipSuccess;
    hipLaunchKernelGGL(k_dhttest_stats, dim3(capped_grid(n_put + n_get, 256, num_cu, 8)), dim3(256), 0, s, put_out, put_src,
                       n_put, get_out, get_ops, get_src, expect, n_get, nnodes, S, node_counts);
    return hipGetLastError();
}

}  // namespace ovs
