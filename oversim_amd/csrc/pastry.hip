// pastry.hip -- Pastry routing (src/overlay/pastry/BasePastry.cc, PastryLeafSet.cc, PastryRoutingTable.cc) for
// gfx950 (MI355X).
//
// The build kernels fill the converged tables: a leaf slot is a ring neighbour of the owner, a
// routing-table slot two bisections over the sorted ids.  pastry_find_node_dev is BasePastry::findNode at one
// node: the one restatement, called by the findNode batch kernel and by every hop of k_pastry_route, which runs
// one lane per semi-recursive route message (BaseOverlay::sendToKey's recursive branch) on the persistent-slice
// scheduler of persist.hpp.  A hop reads the node's record, its leaf row and the one table slot the key
// addresses; the table rows are scanned only for the closer-node fallback and when the first candidate of a
// numRedundantNodes > 1 answer is refused.  A findNode answer is never stored: its entries are produced one at a
// time, each the next in (ring distance, insertion order) after the one before, so the kernels hold no per-lane
// arrays.
#include "pastry.hpp"

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

__device__ __forceinline__ K160 rkey(const KeyRec* __restrict__ recs, uint64_t i) { return key_of(load_rec(recs + i, 0)); }

__device__ __forceinline__ KeyRec empty_slot()
{
    KeyRec e;
    e.w[0] = e.w[1] = e.w[2] = e.w[3] = e.w[4] = 0;
    e.aux = NONE;
    return e;
}

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

struct PDyn {
    unsigned long long* ctr;
    uint64_t from;
};
constexpr PersistTune KP_TUNE{0.70, 64};

__global__ __launch_bounds__(256) void k_pastry_route(PView V, DelayConsts DC, int hcm, int nred, const K160* __restrict__ qkeys,
                                                      const uint32_t* __restrict__ qsrc, uint64_t nq, uint64_t chunk, PDyn dy,
                                                      ovs_route_out* __restrict__ out, uint32_t* __restrict__ hopseq)
{
    const int lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    uint64_t cursor = wave * chunk;
    uint64_t end = min(cursor + chunk, dy.ctr ? dy.from : nq);
    bool more = dy.ctr != nullptr;
    const uint64_t lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    const uint64_t H = (uint64_t)max(hcm, 1);

    bool active = false, local = true;
    uint64_t q = 0;
    K160 K;
    K.w[0] = K.w[1] = K.w[2] = K.w[3] = K.w[4] = 0;
    uint32_t S = 0, cur = 0, last = NONE;
    double sx = 0, sy = 0;            // the last sender
    int64_t t = 0;
    int hops = 0;
    while (true) {
        const uint64_t need = __ballot(!active);
        if (more && need != 0 && cursor >= end) {
            const uint64_t nb = persist_claim_chunk<KP_TUNE.dyn_chunk>(dy.ctr, dy.from, lane);
            if (nb < nq) {
                cursor = nb;
                end = min(nb + (uint64_t)KP_TUNE.dyn_chunk, nq);
            } else {
                more = false;
            }
        }
        if (need != 0 && cursor < end) {
            const uint64_t mine = cursor + (uint64_t)__popcll(need & lt_mask);
            if (!active && mine < end) {
                q = mine;
                active = true;
                local = true;
                K = qkeys[q];
                S = qsrc[q];
                cur = S;
                last = NONE;
                t = 0; hops = 0;
            }
            cursor += (uint64_t)__popcll(need);
        }
        if (!__any(active)) break;
        if (!active) continue;

        const PRec Rc = load_prec(V.rec, cur);
        const PAns a = pastry_find_node_dev(V, cur, Rc, K, 1);
        uint8_t status = 0xFF;       // 0xFF = still running
        const bool at_src = local;
        if (!local) t += DC.msgRoute + coord_ns(sx, sy, Rc.x, Rc.y, DC.round);   // sendRouteMessage
        local = false;
        sx = Rc.x; sy = Rc.y;
        // a forwarded message is delivered on receipt where this node is a sibling (BaseOverlay.cc:907-918); at the
        // source sendToKey runs first (1443-1582)
        if (!at_src && a.closest) status = OVS_LOOKUP_OK;
        else if (a.broken) status = OVS_LOOKUP_BROKEN;
        else if (!a.sibvec && a.next == NONE && nred <= 1) status = OVS_LOOKUP_NO_NEXT;   // "FindNode() returned NULL" (1449)
        else if (hops >= hcm) status = OVS_LOOKUP_HOPMAX;                                  // 1464-1489
        else {
            // the candidate loop (1507-1521): not the last hop, not the source (unless here), not this node
            // unless it is a sibling
            PIter it = iter_start();
            uint32_t nx = NONE;
            while (true) {
                const uint32_t x = answer_next(V, cur, Rc, K, a, nred, 1, it);
                if (x == NONE) break;
                if ((x == last && x != cur) || (x == S && cur != S) || (x == cur && !a.sib)) continue;
                nx = x;
                break;
            }
            if (nx == NONE) status = OVS_LOOKUP_NO_NEXT;
            else if (nx == cur) status = OVS_LOOKUP_OK;            // this node is responsible (1558-1568)
            else {
                if (hopseq) hopseq[q * H + (uint64_t)hops] = nx;   // hops < hcm here
                ++hops;
                last = cur;
                cur = nx;
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
            active = false;
        }
    }
}

inline unsigned nblk(uint64_t n, unsigned b) { return (unsigned)((n + b - 1) / b); }

PView make_view(const PastryTables& t)
{
    PView V;
    V.rec = t.rec; V.leaf = t.leaf; V.tab = t.tab; V.n = t.n; V.rows = t.rows; V.sh = t.sh;
    return V;
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

hipError_t pastry_route(const PastryTables& t, const DelayConsts& DC, int hopCountMax, int recNumRedundantNodes, const K160* keys,
                        const uint32_t* src, uint64_t nq, ovs_route_out* out, uint32_t* hopseq, int num_cu, hipStream_t st,
                        unsigned long long* dyn)
{
    if (nq == 0) return hipSuccess;
    using K = PersistKernel<k_pastry_route>;
    const PersistPlan pl = persist_plan(nq, persist_waves<K::fn>(num_cu), dyn != nullptr, KP_TUNE);
    const PDyn dy{pl.dyn ? dyn : nullptr, pl.dyn_from};
    hipLaunchKernelGGL(K::fn, dim3((unsigned)pl.blocks), dim3(256), 0, st, make_view(t), DC, hopCountMax, recNumRedundantNodes, keys,
                       src, nq, pl.chunk, dy, out, hopseq);
    return hipGetLastError();
}

}  // namespace ovs
