// pastry_dev.hpp -- what the kernels that take a Pastry step share on the device (pastry.hip: the findNode batch
// and the route; scribe.hip: the joins of a Scribe forest): the view of the tables, BasePastry::findNode at one
// node (pastry_find_node_dev, the one restatement), the walk over its answer (answer_next) and what
// BaseOverlay::sendToKey's recursive branch makes of it (pastry_send_to_key, pastry_source_step).  No kernels, no
// state; a findNode answer is never stored: its entries are produced one at a time, each the next in (ring
// distance, insertion order) after the one before, so the callers hold no per-lane arrays.
#pragma once
#include "pastry.hpp"

namespace ovs {

__device__ __forceinline__ KeyRec empty_slot()
{
    KeyRec e;
    e.w[0] = e.w[1] = e.w[2] = e.w[3] = e.w[4] = 0;
    e.aux = NONE;
    return e;
}

// ---------------------------------------------------------------------------
// findNode

struct PView {
    const PastryRec* __restrict__ rec;
    const KeyRec* __restrict__ leaf;
    const KeyRec* __restrict__ tab;
    uint32_t n;
    int rows;
    PastryShape sh;
};

inline PView make_view(const PastryTables& t)
{
    PView V;
    V.rec = t.rec; V.leaf = t.leaf; V.tab = t.tab; V.n = t.n; V.rows = t.rows; V.sh = t.sh;
    return V;
}

struct PRec {
    K160 k;
    int nrows;
    double x, y;
};

__device__ __forceinline__ PRec load_prec(const PastryRec* __restrict__ rec, uint32_t i)
{
    const uint4* p = reinterpret_cast<const uint4*>(rec + i);
    const uint4 q0 = p[0], q1 = p[1], q2 = p[2];
    PRec r;
    r.k.w[0] = q0.x; r.k.w[1] = q0.y; r.k.w[2] = q0.z; r.k.w[3] = q0.w; r.k.w[4] = q1.x;
    r.nrows = (int)q1.y;
    r.x = dbl(q2.x, q2.y);
    r.y = dbl(q2.z, q2.w);
    return r;
}

__device__ __forceinline__ const KeyRec* leaf_row(const PView& V, uint32_t c) { return V.leaf + (uint64_t)c * (uint64_t)V.sh.L; }
__device__ __forceinline__ const KeyRec* tab_row(const PView& V, uint32_t c, int r)
{
    return V.tab + ((uint64_t)c * (uint64_t)V.rows + (uint64_t)r) * (uint64_t)V.sh.P();
}

// PastryStateObject::isCloser (PastryStateObject.cc:134-155) compares keyDist strictly: its two early outs (the
// reference holds the key; test is the reference) are cases of equal or zero distance.  So "closer than ref" is
// a distance below ref's, and every caller below keeps the distance of its current reference in bd.

// specialCloserCondition (157-173) of entry e against a reference at distance bd
__device__ __forceinline__ bool special_closer(const PView& V, const PRec& R, const KeyRec& e, const K160& key, const K160& bd)
{
    const K160 ek = key_of(e);
    if (p_spl_digits(ek, key, V.sh.b) < p_spl_digits(R.k, key, V.sh.b)) return false;
    return k_lt(p_ring_dist(ek, key), bd);
}

// PastryLeafSet::getSmallestNode / getBiggestNode (421-440)
__device__ __forceinline__ KeyRec leaf_smallest(const KeyRec* __restrict__ row, int L)
{
    int i = 0;
    KeyRec e = load_rec(row, 0);
    while (e.aux == NONE && i != L / 2 - 1) e = load_rec(row, (uint32_t)++i);
    return e;
}
__device__ __forceinline__ KeyRec leaf_biggest(const KeyRec* __restrict__ row, int L)
{
    int i = L - 1;
    KeyRec e = load_rec(row, (uint32_t)i);
    while (e.aux == NONE && i != L / 2) e = load_rec(row, (uint32_t)--i);
    return e;
}

// PastryLeafSet::isClosestNode (136-161)
__device__ __forceinline__ bool is_closest(const PView& V, uint32_t c, const PRec& R, const K160& key)
{
    if (k_eq(R.k, key)) return true;
    const KeyRec* row = leaf_row(V, c);
    const KeyRec small = load_rec(row, (uint32_t)(V.sh.L / 2 - 1)), big = load_rec(row, (uint32_t)(V.sh.L / 2));
    if (small.aux == NONE && big.aux == NONE) return true;
    const K160 own = p_ring_dist(R.k, key);
    const bool bc = big.aux != NONE && k_lt(p_ring_dist(key_of(big), key), own);
    const bool sc = small.aux != NONE && k_lt(p_ring_dist(key_of(small), key), own);
    return !bc && !sc;
}

// PastryLeafSet::getDestinationNode (106-134)
__device__ uint32_t leaf_destination(const PView& V, uint32_t c, const PRec& R, const K160& key)
{
    const KeyRec* row = leaf_row(V, c);
    const KeyRec sm = leaf_smallest(row, V.sh.L), bg = leaf_biggest(row, V.sh.L);
    const K160 smk = sm.aux == NONE ? R.k : key_of(sm), bgk = bg.aux == NONE ? R.k : key_of(bg);
    if (!between_LR(key, smk, bgk)) return NONE;
    uint32_t ret = NONE;
    K160 bd = p_ring_dist(R.k, key);
    for (int j = 0; j < V.sh.L; ++j) {
        const KeyRec e = load_rec(row, (uint32_t)j);
        if (e.aux == NONE) continue;
        const K160 d = p_ring_dist(key_of(e), key);
        if (k_lt(d, bd)) { ret = e.aux; bd = d; }
    }
    return ret;
}

// PastryLeafSet::findCloserNode (458-484); *bd: the distance of the node returned
__device__ uint32_t leaf_closer(const PView& V, uint32_t c, const PRec& R, const K160& key, bool optimize, K160* bd)
{
    const KeyRec* row = leaf_row(V, c);
    const KeyRec sm = leaf_smallest(row, V.sh.L), bg = leaf_biggest(row, V.sh.L);
    uint32_t ret = NONE;
    *bd = p_ring_dist(R.k, key);
    if (sm.aux != NONE && special_closer(V, R, sm, key, *bd)) {
        ret = sm.aux; *bd = p_ring_dist(key_of(sm), key);
        if (!optimize) return ret;
    }
    if (bg.aux != NONE && special_closer(V, R, bg, key, *bd)) {
        ret = bg.aux; *bd = p_ring_dist(key_of(bg), key);
    }
    return ret;
}

// PastryRoutingTable::nodeAt (70-76) with its unsigned arguments
__device__ __forceinline__ KeyRec node_at(const PView& V, uint32_t c, const PRec& R, int row, int col)
{
    if (row < 0 || col < 0 || row >= R.nrows || col >= V.sh.P()) return empty_slot();
    return load_rec(tab_row(V, c, row), (uint32_t)col);
}

// PastryRoutingTable::findCloserNode (100-180); the key is not the owner's, (shl + 1) * b <= 160
__device__ uint32_t table_closer(const PView& V, uint32_t c, const PRec& R, const K160& key, bool optimize, K160* bd)
{
    const int P = V.sh.P(), b = V.sh.b;
    uint32_t ret = NONE;
    *bd = p_ring_dist(R.k, key);
    if (!optimize) {
        for (int y = 0; y < R.nrows; ++y)
            for (int x = 0; x < P; ++x) {
                const KeyRec e = load_rec(tab_row(V, c, y), (uint32_t)x);
                if (e.aux != NONE && special_closer(V, R, e, key, *bd)) {
                    *bd = p_ring_dist(key_of(e), key);
                    return e.aux;
                }
            }
        return NONE;
    }
    auto look = [&](int row, int col) {
        const KeyRec e = node_at(V, c, R, row, col);
        if (e.aux != NONE && special_closer(V, R, e, key, *bd)) { ret = e.aux; *bd = p_ring_dist(key_of(e), key); }
    };
    int shl = p_spl_bits(R.k, key) / b;
    const int digit = (int)p_digit(key, shl, b);
    const int x = (int)p_digit(R.k, shl, b);
    int lo = digit - 1, hi = digit + 1;
    while (lo >= 0 || hi < P) {
        if (lo == x) lo = -1;
        if (hi == x) hi = P;
        if (lo >= 0) look(shl, lo--);
        if (hi < P) look(shl, hi++);
    }
    if (shl != 0) {
        --shl;
        look(shl, k_lt(key, R.k) ? digit - 1 : digit + 1);
    }
    return ret;
}

// what BasePastry::findNode decides before it fills a vector
struct PAns {
    uint32_t next;       // nextHops[0]: this node, the leaf, the table entry or the closer node; NONE = none
    bool closest;        // leafSet->isClosestNode(key)
    bool sib, err;       // isSiblingFor(thisNode, key, numSiblings, &err)
    bool sibvec;         // the answer is createSiblingVector(key, numSiblings)
    bool broken;         // the reference throws or dereferences a NULL vector
    uint8_t source;      // 0 this node, 1 leaf set, 2 table slot, 3 closer-node fallback, 4 none
};

// the walk over a sorted vector: the entry last produced, as (distance, insertion order)
struct PIter {
    K160 lo;
    int seq;
    int taken;           // entries produced
    bool started;
    bool first_done;     // the regular next hop went out
};

__device__ __forceinline__ PIter iter_start()
{
    PIter it;
    it.lo.w[0] = it.lo.w[1] = it.lo.w[2] = it.lo.w[3] = it.lo.w[4] = 0;
    it.seq = 0; it.taken = 0; it.started = false; it.first_done = false;
    return it;
}

// The next entry of NodeVector(., KeyDistanceComparator<KeyRingMetric>(key)) after it: the vector filled with
// [this node,] [the table's entries by row and column,] the leaf slots in order (NodeVector.h:381-512: a key once,
// ties in insertion order).  A leaf that is also a table entry sits in its table slot, which is looked at.
__device__ uint32_t next_sorted(const PView& V, uint32_t c, const PRec& R, const K160& key, PIter& it, bool owner_first,
                                bool with_table)
{
    const int P = V.sh.P(), leaf0 = 1 + V.rows * P;
    while (true) {
        uint32_t best = NONE;
        int bseq = 0;
        K160 bd = it.lo, bk = it.lo;
        auto consider = [&](const K160& ek, uint32_t idx, int seq) {
            const K160 d = p_ring_dist(ek, key);
            const bool after = !it.started || k_lt(it.lo, d) || (k_eq(it.lo, d) && seq > it.seq);
            if (after && (best == NONE || k_lt(d, bd))) { best = idx; bd = d; bseq = seq; bk = ek; }
        };
        if (owner_first) consider(R.k, c, 0);
        if (with_table)
            for (int s = 0; s < R.nrows * P; ++s) {
                const KeyRec e = load_rec(tab_row(V, c, 0), (uint32_t)s);
                if (e.aux != NONE) consider(key_of(e), e.aux, 1 + s);
            }
        const KeyRec* row = leaf_row(V, c);
        for (int j = 0; j < V.sh.L; ++j) {
            const KeyRec e = load_rec(row, (uint32_t)j);
            if (e.aux != NONE) consider(key_of(e), e.aux, leaf0 + j);
        }
        if (best == NONE) return NONE;
        it.lo = bd; it.seq = bseq; it.started = true;
        if (with_table && bseq >= leaf0) {
            const int shl = p_spl_bits(R.k, bk) / V.sh.b;
            if (shl < R.nrows && load_rec(tab_row(V, c, shl), p_digit(bk, shl, V.sh.b)).aux == best) continue;
        }
        return best;
    }
}

// PastryLeafSet::createSiblingVector (220-259) returns NULL: the leaf set is valid and full and the vector
// (numSiblings 0: unlimited) holds its biggest or smallest key
__device__ bool sibvec_null(const PView& V, uint32_t c, const PRec& R, const K160& key, int ns)
{
    const KeyRec* row = leaf_row(V, c);
    const int L = V.sh.L;
    if (load_rec(row, (uint32_t)(L / 2 - 1)).aux == NONE || load_rec(row, (uint32_t)(L / 2)).aux == NONE) return false;
    const KeyRec f = load_rec(row, 0), l = load_rec(row, (uint32_t)(L - 1));
    if (f.aux == NONE || l.aux == NONE) return false;
    if (ns == 0) return true;
    const K160 df = p_ring_dist(key_of(f), key), dl = p_ring_dist(key_of(l), key), own = p_ring_dist(R.k, key);
    // entries ordered before the first and before the last slot: this node goes first among equals
    int rf = k_le(own, df) ? 1 : 0, rl = k_le(own, dl) ? 1 : 0;
    for (int j = 0; j < L; ++j) {
        const KeyRec e = load_rec(row, (uint32_t)j);
        if (e.aux == NONE) continue;
        const K160 d = p_ring_dist(key_of(e), key);
        if (j > 0 && k_lt(d, df)) ++rf;
        if (j < L - 1 && k_le(d, dl)) ++rl;
    }
    return rf < ns || rl < ns;
}

// BasePastry::findNode (BasePastry.cc:1100-1211) at node c (record R), state READY, up to the vector
__device__ PAns pastry_find_node_dev(const PView& V, uint32_t c, const PRec& R, const K160& key, int numSiblings)
{
    PAns a;
    a.next = NONE; a.sib = false; a.err = false; a.sibvec = false; a.broken = false; a.source = 4;
    a.closest = is_closest(V, c, R, key);
    if (a.closest) {
        a.next = c;
        a.source = 0;
    } else {
        a.next = leaf_destination(V, c, R, key);
        if (a.next != NONE) a.source = 1;
        else {
            // lookupNextHop (78-98): digitAt reads its digit before the row is checked (83)
            const int shl = p_spl_bits(R.k, key) / V.sh.b;
            if ((shl + 1) * V.sh.b > KEYBITS) { a.broken = true; return a; }
            if (shl < R.nrows) a.next = load_rec(tab_row(V, c, shl), p_digit(key, shl, V.sh.b)).aux;
            if (a.next != NONE) a.source = 2;
        }
        if (a.next == NONE) {
            K160 bd, ld;
            if (V.sh.opt) {
                a.next = table_closer(V, c, R, key, true, &bd);
                const uint32_t tmp = leaf_closer(V, c, R, key, true, &ld);
                if (tmp != NONE && k_lt(ld, bd)) a.next = tmp;        // leafSet->isCloser(*tmp, key, *next) (1146-1151)
            } else {
                a.next = table_closer(V, c, R, key, false, &bd);
                if (a.next == NONE) a.next = leaf_closer(V, c, R, key, false, &ld);
            }
            if (a.next != NONE) a.source = 3;
        }
    }
    // isSiblingFor (919-952)
    if (numSiblings == 1) {
        a.sib = a.closest;
    } else if (sibvec_null(V, c, R, key, numSiblings)) {
        a.err = true;
    } else {
        // this node is in the vector: fewer than numSiblings leaves are strictly closer (0: no limit)
        const KeyRec* row = leaf_row(V, c);
        const K160 own = p_ring_dist(R.k, key);
        int rank = 0;
        for (int j = 0; j < V.sh.L; ++j) {
            const KeyRec e = load_rec(row, (uint32_t)j);
            if (e.aux != NONE && k_lt(p_ring_dist(key_of(e), key), own)) ++rank;
        }
        a.sib = numSiblings == 0 || rank < numSiblings;
        a.err = !a.sib;
    }
    if (a.sib && !a.err) {
        a.sibvec = true;
        if (sibvec_null(V, c, R, key, numSiblings)) a.broken = true;     // findNode returns NULL (1180)
    }
    return a;
}

// the answer's entries in order, one a call; NONE at its end.  numRedundantNodes > 1 (1184-1209): nextHops[0]
// followed by the ring-metric vector without it where useRegularNextHop holds and there is a next hop -- that is
// the vector itself where its first entry is the next hop -- else the vector.
__device__ uint32_t answer_next(const PView& V, uint32_t c, const PRec& R, const K160& key, const PAns& a, int nred, int nsib,
                                PIter& it)
{
    if (a.sibvec) {
        if (nsib && it.taken >= nsib) return NONE;
        const uint32_t x = next_sorted(V, c, R, key, it, true, false);
        if (x != NONE) ++it.taken;
        return x;
    }
    const bool regular = nred > 1 && V.sh.reg && a.next != NONE;
    if (nred <= 1 || (regular && !it.first_done)) {
        if (it.first_done) return NONE;
        it.first_done = true;
        return a.next;
    }
    while (it.taken < nred) {
        const uint32_t x = next_sorted(V, c, R, key, it, false, true);
        if (x == NONE) return NONE;
        ++it.taken;
        if (regular && x == a.next) continue;
        return x;
    }
    return NONE;
}

// ---------------------------------------------------------------------------
// sendToKey

constexpr uint8_t PSTEP_FORWARD = 0xFF;

// What BaseOverlay::sendToKey's recursive branch (BaseOverlay.cc:1443-1582) decides at node cur, which holds a
// message for K that receipt did not deliver, from its findNode answer a (numSiblings = 1).  status
// PSTEP_FORWARD: the message goes to `next`; OVS_LOOKUP_OK: cur is responsible (1558-1568, next = cur); else the
// message is dropped.  hops: the message's hop count, last: the node it came from (NONE at its source), S: its source.
struct PStep {
    uint32_t next;
    uint8_t status;
};

__device__ __forceinline__ PStep pastry_send_to_key(const PView& V, uint32_t cur, const PRec& Rc, const K160& K, const PAns& a,
                                                    int hops, int hcm, int nred, uint32_t last, uint32_t S)
{
    PStep st;
    st.next = NONE;
    // findNode throws "numRedundantNodes or numSiblings too big!" above getMaxNumRedundantNodes() = numberOfLeaves
    // (BasePastry.cc:1095-1098, 1105-1110)
    if (a.broken || nred > V.sh.L) st.status = OVS_LOOKUP_BROKEN;
    else if (!a.sibvec && a.next == NONE && nred <= 1) st.status = OVS_LOOKUP_NO_NEXT;   // "FindNode() returned NULL" (1449)
    else if (hops >= hcm) st.status = OVS_LOOKUP_HOPMAX;                                  // 1464-1489
    else {
        // the candidate loop (1507-1521): not the last hop, not the source (unless here), not this node
        // unless it is a sibling
        PIter it = iter_start();
        while (true) {
            const uint32_t x = answer_next(V, cur, Rc, K, a, nred, 1, it);
            if (x == NONE) break;
            if ((x == last && x != cur) || (x == S && cur != S) || (x == cur && !a.sib)) continue;
            st.next = x;
            break;
        }
        st.status = st.next == NONE ? OVS_LOOKUP_NO_NEXT : st.next == cur ? OVS_LOOKUP_OK : PSTEP_FORWARD;
    }
    return st;
}

// The source step of a route: sendToKey at node c for a message of its own (no last hop, source = c, hop count 0).
// The pick (status PSTEP_FORWARD), c itself (OVS_LOOKUP_OK: c is the sibling for K), or the status the route ends in.
__device__ __forceinline__ PStep pastry_source_step(const PView& V, uint32_t c, const K160& K, int hcm, int nred)
{
    const PRec Rc = load_prec(V.rec, c);
    const PAns a = pastry_find_node_dev(V, c, Rc, K, 1);
    return pastry_send_to_key(V, c, Rc, K, a, 0, hcm, nred, NONE, c);
}

// isSiblingFor(c, K, 1) (BasePastry.cc:919-952): what receipt asks before it delivers (BaseOverlay.cc:907-918)
__device__ __forceinline__ bool pastry_is_sibling(const PView& V, uint32_t c, const K160& K)
{
    return is_closest(V, c, load_prec(V.rec, c), K);
}

}  // namespace ovs
