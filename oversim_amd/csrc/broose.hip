// broose.hip -- Broose routing (src/overlay/broose/Broose.cc, BrooseBucket.cc) for gfx950 (MI355X).
//
// k_broose_rows builds the ideal snapshot: one thread per (node, bucket) finds the bucket's up to maxSize
// XOR-closest node ids by descending the binary trie that the sorted id array is -- at a split the side
// that shares the bucket key's bit is closer than all of the other side -- and writes them in XOR order.
// k_broose_rec then derives each node's 64 B record from its rows.
//
// broose_find_node_dev is Broose::findNode (574-770) at one node: the one restatement, called by the
// findNode batch kernel and by every hop of K4 k_broose_route, which runs one lane per lookup through
// IterativeLookup's single path (lookupRedundantNodes = lookupParallelRpcs = 1, merge off,
// visitOnlyOnce) on the persistent-slice scheduler of persist.hpp.  A hop reads the responder's record
// and scans one of its rows (24 B entries that carry the ids: broose.hpp) against the route key, or the
// bBucket row against the lookup key for sibling answers and brother lookups.  Nothing is indexed at
// run time but global memory: the kernel holds no per-lane arrays.
#include "broose.hpp"
#include "persist.hpp"

namespace ovs {

void broose_free(BrooseTables& t)
{
    if (t.rec) hipFree(t.rec);
    if (t.rows) hipFree(t.rows);
    t.rec = nullptr;
    t.rows = nullptr;
    t.n = 0;
}

namespace {

__device__ __forceinline__ int kbit(const K160& a, int bit) { return (int)((k_word(a, bit >> 5) >> (bit & 31)) & 1u); }

// ---------------------------------------------------------------------------
// the snapshot

__global__ __launch_bounds__(64) void k_broose_rows(const KeyRec* __restrict__ recs, uint32_t n, BrooseShape sh,
                                                    KeyRec* __restrict__ rows)
{
    // the row under construction, [slot][lane]: node indices in XOR order and the top 64 bits of their
    // distances (an order-preserving code; equal codes fall back to the ids)
    __shared__ uint32_t s_idx[BROOSE_MAX_ROW][64];
    __shared__ uint64_t s_dc[BROOSE_MAX_ROW][64];
    const int t = (int)threadIdx.x;
    const int nr = sh.nrows();
    const uint64_t g = (uint64_t)blockIdx.x * 64 + (uint64_t)t;
    if (g >= (uint64_t)n * (uint64_t)nr) return;
    const uint32_t v = (uint32_t)(g / (uint64_t)nr);
    const int r = (int)(g % (uint64_t)nr);
    const K160 T = broose_bucket_key(sh, rkey(recs, v), r);
    const int m = min(sh.cap(r), BROOSE_MAX_ROW);
    int cnt = 0;
    // chunks arrive closest first, so an insertion never walks back past its own chunk
    auto insert = [&](uint32_t j) {
        if (cnt >= m) return;
        const K160 d = k_xor(rkey(recs, j), T);
        const uint64_t c = top64(d);
        int p = cnt;
        while (p > 0) {
            const uint64_t cp = s_dc[p - 1][t];
            const bool less = c != cp ? c < cp : k_lt(d, k_xor(rkey(recs, s_idx[p - 1][t]), T));
            if (!less) break;
            s_idx[p][t] = s_idx[p - 1][t];
            s_dc[p][t] = cp;
            --p;
        }
        s_idx[p][t] = j;
        s_dc[p][t] = c;
        ++cnt;
    };
    uint32_t lo = 0, hi = n;
    int need = m;
    while (need > 0 && hi > lo) {
        if (hi - lo <= (uint32_t)need) {
            for (uint32_t j = lo; j < hi; ++j) insert(j);
            break;
        }
        // the ids of [lo, hi) agree above `bit` and split at it (they are sorted and distinct)
        const int bit = k_msb(k_xor(rkey(recs, lo), rkey(recs, hi - 1)));
        uint32_t l = lo, h = hi;
        while (l < h) {
            const uint32_t mid = l + ((h - l) >> 1);
            if (kbit(rkey(recs, mid), bit)) h = mid; else l = mid + 1;
        }
        const bool tb = kbit(T, bit);
        const uint32_t nlo = tb ? l : lo, nhi = tb ? hi : l, flo = tb ? lo : l, fhi = tb ? l : hi;
        if (nhi - nlo >= (uint32_t)need) {
            lo = nlo; hi = nhi;              // the far side is never needed
        } else {
            for (uint32_t j = nlo; j < nhi; ++j) insert(j);
            need -= (int)(nhi - nlo);
            lo = flo; hi = fhi;
        }
    }
    KeyRec* row = rows + (uint64_t)v * sh.stride() + sh.at(r);
    for (int j = 0; j < sh.cap(r); ++j) {
        KeyRec e;
        if (j < cnt) {
            e = load_rec(recs, s_idx[j][t]);
            e.aux = s_idx[j][t];
        } else {
            e.w[0] = e.w[1] = e.w[2] = e.w[3] = e.w[4] = 0;
            e.aux = NONE;
        }
        row[j] = e;
    }
}

// explicit tables: row g of the CSR (validated on the host) into the node's fixed row
__global__ void k_broose_rows_csr(const KeyRec* __restrict__ recs, uint32_t n, BrooseShape sh, const uint64_t* __restrict__ off,
                                  const uint32_t* __restrict__ nodes, KeyRec* __restrict__ rows)
{
    const int nr = sh.nrows();
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (uint64_t)n * (uint64_t)nr) return;
    const uint32_t v = (uint32_t)(g / (uint64_t)nr);
    const int r = (int)(g % (uint64_t)nr);
    const uint64_t a = off[g], b = off[g + 1];
    KeyRec* row = rows + (uint64_t)v * sh.stride() + sh.at(r);
    for (int j = 0; j < sh.cap(r); ++j) {
        KeyRec e;
        const uint32_t x = a + (uint64_t)j < b ? nodes[a + (uint64_t)j] : NONE;
        if (x < n) {
            e = load_rec(recs, x);
            e.aux = x;
        } else {
            e.w[0] = e.w[1] = e.w[2] = e.w[3] = e.w[4] = 0;
            e.aux = NONE;
        }
        row[j] = e;
    }
}

__device__ __forceinline__ int row_count(const KeyRec* __restrict__ row, int cap)
{
    int c = 0;
    while (c < cap && load_rec(row, (uint32_t)c).aux != NONE) ++c;
    return c;
}

// BrooseBucket::longestPrefix (202-209): the prefix the closest and the farthest entry share
__device__ __forceinline__ int row_longest_prefix(const KeyRec* __restrict__ row, int cap)
{
    const int c = row_count(row, cap);
    if (c < 2) return 0;
    const K160 d = k_xor(rkey(row, 0), rkey(row, (uint64_t)(c - 1)));
    return k_zero(d) ? KEYBITS : KEYBITS - 1 - k_msb(d);
}

__global__ void k_broose_rec(const KeyRec* __restrict__ recs, const double2* __restrict__ xy, uint32_t n, BrooseShape sh,
                             const KeyRec* __restrict__ rows, BrooseRec* __restrict__ out)
{
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const K160 me = rkey(recs, v);
    const KeyRec* base = rows + (uint64_t)v * sh.stride();
    BrooseRec o;
    for (int i = 0; i < 5; ++i) { o.w[i] = me.w[i]; o.bd[i] = 0; }
    o.lp0 = (uint8_t)row_longest_prefix(base + sh.at(0), sh.kr);
    o.lp1 = (uint8_t)row_longest_prefix(base + sh.at(1), sh.kr);
    // keyInRange on the bBucket (239-260): maxSize / 7 = bucketSize
    const KeyRec* rb = base + sh.at(sh.P() + 1);
    const int cb = row_count(rb, 7 * sh.k);
    if (cb == 0) o.bmode = 2;
    else if (cb <= sh.k) o.bmode = 1;
    else {
        o.bmode = 0;
        const K160 d = k_xor(rkey(rb, (uint64_t)(sh.k - 1)), me);
        for (int i = 0; i < 5; ++i) o.bd[i] = d.w[i];
    }
    o.pad0 = 0; o.pad1 = 0;
    o.x = xy[v].x; o.y = xy[v].y;
    out[v] = o;
}

__global__ void k_broose_row_nodes(const KeyRec* __restrict__ rows, uint64_t total, uint32_t* __restrict__ out)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) out[i] = load_rec(rows + i, 0).aux;
}

// ---------------------------------------------------------------------------
// findNode

struct BView {
    const BrooseRec* __restrict__ rec;
    const KeyRec* __restrict__ rows;
    uint32_t n;
    BrooseShape sh;
};

struct BRec {
    K160 k, bd;
    int lp0, lp1, bmode;
    double x, y;
};

// one record: the four chunks are requested together
__device__ __forceinline__ BRec load_brec(const BrooseRec* __restrict__ rec, uint32_t i)
{
    const uint4* p = reinterpret_cast<const uint4*>(rec + i);
    const uint4 q0 = p[0], q1 = p[1], q2 = p[2], q3 = p[3];
    BRec r;
    r.k.w[0] = q0.x; r.k.w[1] = q0.y; r.k.w[2] = q0.z; r.k.w[3] = q0.w; r.k.w[4] = q1.x;
    r.lp0 = (int)(q1.y & 0xFFu); r.lp1 = (int)((q1.y >> 8) & 0xFFu); r.bmode = (int)((q1.y >> 16) & 0xFFu);
    r.bd.w[0] = q1.z; r.bd.w[1] = q1.w; r.bd.w[2] = q2.x; r.bd.w[3] = q2.y; r.bd.w[4] = q2.z;
    r.x = dbl(q3.x, q3.y);
    r.y = dbl(q3.z, q3.w);
    return r;
}

// The first node of NodeVector(..., KeyDistanceComparator<KeyXorMetric>(tgt)) filled with the row and
// thisNode (fillVector + add): the XOR-closest to tgt of the row's nodes and c.  With has_lo, the closest
// whose distance lies strictly above lo -- the vector's next entry after the one at distance lo (ids are
// distinct, so are the distances).  NONE when there is none; *bd = its distance.
__device__ __forceinline__ uint32_t scan_row(const KeyRec* __restrict__ row, int cap, uint32_t c, const K160& me, const K160& tgt,
                                             bool has_lo, const K160& lo, K160* bd)
{
    uint32_t best = NONE;
    K160 d = k_xor(me, tgt);
    K160 b = d;
    if (!has_lo || k_lt(lo, d)) best = c;
    for (int j = 0; j < cap; ++j) {
        const KeyRec e = load_rec(row, (uint32_t)j);
        if (e.aux == NONE) break;
        d = k_xor(key_of(e), tgt);
        if ((!has_lo || k_lt(lo, d)) && (best == NONE || k_lt(d, b))) { best = e.aux; b = d; }
    }
    *bd = b;
    return best;
}

// Broose::isSiblingFor (823-854), node == thisNode, state READY: numSiblings 0 is key equality, anything
// else bBucket->keyInRange(key) (-1 = getMaxNumSiblings() changes nothing)
__device__ __forceinline__ bool broose_is_sibling(const BRec& R, const K160& key, int numSiblings)
{
    if (numSiblings == 0) return k_eq(R.k, key);
    if (R.bmode) return R.bmode == 1;
    return k_le(k_xor(key, R.k), R.bd);
}

// where findNode's answer comes from: the row scanned and the key it is sorted by
struct BAns {
    const KeyRec* row;
    int cap;
    K160 tgt;
    uint32_t first;      // (*result)[0]
    bool sib;            // isSiblingFor(thisNode, key, numSiblings)
    bool broken;         // the reference errors, reads a bit outside the key, or is undefined
};

// the row and sort key of the answer that leaves extension e (advanced already) at node c: what
// findNode's last round scanned.  brother: the round was the brother lookup (bBucket by the lookup key).
__device__ __forceinline__ void answer_row(const BView& V, uint32_t c, const K160& key, const BExt& e, bool brother, BAns& a)
{
    const KeyRec* base = V.rows + (uint64_t)c * V.sh.stride();
    if (brother) {
        a.row = base + V.sh.at(V.sh.P() + 1); a.cap = 7 * V.sh.k; a.tgt = key;
    } else if (!e.right) {
        a.row = base + V.sh.at(V.sh.P()); a.cap = V.sh.P() * V.sh.kr; a.tgt = e.rk;
    } else {
        // the prefix the round put on top of the route key chose rBucket[prefix] (738-748)
        const int prefix = (int)(e.rk.w[4] >> (32 - V.sh.sb));
        a.row = base + V.sh.at(prefix); a.cap = V.sh.kr; a.tgt = e.rk;
    }
}

// Broose::findNode (574-770) at node c (record R), state READY, for a call that carries extension e
// (e.has = 0: none yet; `right` is then the direction chooseLookup++ (643) would give).  e is advanced in
// place; the caller drops it where the call's answer is not used.  *brother: the answering round was a
// brother lookup.
__device__ BAns broose_find_node_dev(const BView& V, uint32_t c, const BRec& R, const K160& key, BExt& e, bool right,
                                     int numSiblings, bool* brother)
{
    BAns a;
    a.broken = false;
    a.first = NONE;
    a.sib = broose_is_sibling(R, key, numSiblings);
    *brother = false;
    K160 bd;
    if (a.sib) {
        // the closest nodes sorted by XOR distance to the key (597-621); the extension passes through
        answer_row(V, c, key, e, true, a);
        a.first = scan_row(a.row, a.cap, c, R.k, a.tgt, false, a.tgt, &bd);
        return a;
    }
    const int sb = V.sh.sb;
    if (!e.has) {
        // the distance estimate (629-641)
        int dist = max(R.lp0, R.lp1) + 1 + V.sh.userDist;
        if (dist % sb != 0) dist += sb - dist % sb;
        if (dist > KEYBITS) dist = KEYBITS - KEYBITS % sb;
        if (!right) {
            // left shifting (644-656): `int prefix` holds self's top dist bits, defined up to dist = 31
            if (dist > 31) { a.broken = true; return a; }
            e.rk = k_add(b_shr(key, dist), b_shl(b_shr(R.k, KEYBITS - dist), KEYBITS - dist));
            e.step = -dist;
        } else {
            e.rk = R.k;
            e.step = dist;
        }
        e.right = right ? 1 : 0;
        e.has = 1;
    }
    // the tail (765-768): findNode runs again on the same message while the best entry is this node.
    // Right shifting lowers step by shiftingBits a round, left shifting raises it from below 0; at
    // step == 0 the brother lookup answers whatever comes first, so the loop ends within 160 / sb + 1 rounds
    for (int guard = 0; guard <= KEYBITS + 1; ++guard) {
        e.last = c;
        if (e.step == 0) {
            *brother = true;
            answer_row(V, c, key, e, true, a);
            a.first = scan_row(a.row, a.cap, c, R.k, a.tgt, false, a.tgt, &bd);
            return a;
        }
        if (!e.right) {
            if (e.step > 0) break;               // never reaches 0: the reference does not return
            e.rk = b_shl(e.rk, sb);
            e.step += sb;
        } else {
            // key.getBit(160 - dist + i), i < sb, must lie inside the key (737)
            const int dist = e.step;
            if (dist < sb || dist > KEYBITS) break;
            const uint32_t prefix = b_shr(key, KEYBITS - dist).w[0] & ((1u << sb) - 1u);
            K160 pre;
            pre.w[0] = prefix; pre.w[1] = 0; pre.w[2] = 0; pre.w[3] = 0; pre.w[4] = 0;
            e.rk = k_add(b_shr(e.rk, sb), b_shl(pre, KEYBITS - sb));
            e.step = dist - sb;
        }
        answer_row(V, c, key, e, false, a);
        a.first = scan_row(a.row, a.cap, c, R.k, a.tgt, false, a.tgt, &bd);
        if (a.first != c) return a;
    }
    a.broken = true;
    a.first = NONE;
    return a;
}

__global__ void k_broose_find_node(BView V, const uint32_t* __restrict__ node, const K160* __restrict__ keys,
                                   BExt* __restrict__ ext, const uint8_t* __restrict__ right, uint64_t nq, int nred, int nsib,
                                   uint32_t* __restrict__ out, uint32_t max_out, uint8_t* __restrict__ count,
                                   uint8_t* __restrict__ sib, uint8_t* __restrict__ status)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const uint32_t c = node[i];
    const BRec R = load_brec(V.rec, c);
    BExt e = ext[i];
    bool brother;
    const BAns a = broose_find_node_dev(V, c, R, keys[i], e, right[i] != 0, nsib, &brother);
    uint32_t* o = out + i * (uint64_t)max_out;
    for (uint32_t j = 0; j < max_out; ++j) o[j] = NONE;
    sib[i] = a.sib ? 1 : 0;
    status[i] = a.broken ? 1 : 0;
    if (a.broken) { count[i] = 0; return; }
    ext[i] = e;
    // the result size rule (587-595); numSiblings < 0: exhaustive-iterative does not care about siblings
    int size = nsib < 0 ? nred : (a.sib ? (nsib ? nsib : 1) : nred);
    if ((uint32_t)size > max_out) size = (int)max_out;
    int cnt = 0;
    // the vector's entries in order: each the closest beyond the one before
    K160 lo = a.tgt, bd;
    uint32_t x = scan_row(a.row, a.cap, c, R.k, a.tgt, false, lo, &bd);
    while (x != NONE && cnt < size) {
        o[cnt++] = x;
        lo = bd;
        x = scan_row(a.row, a.cap, c, R.k, a.tgt, true, lo, &bd);
    }
    count[i] = (uint8_t)cnt;
}

// ---------------------------------------------------------------------------
// K4: the route

constexpr PersistTune K4_TUNE{0.70, 64};

__global__ __launch_bounds__(256) void k_broose_route(BView V, DelayConsts DC, int hcm, const K160* __restrict__ qkeys,
                                                      const uint32_t* __restrict__ qsrc, const uint8_t* __restrict__ qright,
                                                      uint64_t nq, uint64_t chunk, PersistDyn dy, ovs_route_out* __restrict__ out,
                                                      uint32_t* __restrict__ hopseq, uint32_t* __restrict__ rpcs)
{
    PersistFeed<K4_TUNE.dyn_chunk> feed(chunk, dy, nq);
    const uint64_t H = (uint64_t)hcm;

    bool active = false, local = true, right = false, src_brother = false;
    uint64_t q = 0;
    K160 K;
    uint32_t S = 0, cur = 0;
    double sx = 0, sy = 0;
    int64_t t = 0;
    int hops = 0, ntry = 0;
    uint32_t nrpc = 0;
    uint64_t vis = 0;
    BExt e;
    e.has = 0; e.step = 0; e.right = 0; e.last = NONE;
    e.rk.w[0] = e.rk.w[1] = e.rk.w[2] = e.rk.w[3] = e.rk.w[4] = 0;
    while (true) {
        if (feed.take(active, dy, nq, q)) {
            active = true;
            local = true;
            K = qkeys[q];
            S = qsrc[q];
            right = qright[q] != 0;
            t = 0; hops = 0; ntry = 0; nrpc = 0;
            vis = vis_bit(S);
            e.has = 0; e.step = 0; e.right = 0; e.last = NONE;   // the local FindNodeCall carries no extension
        }
        if (!__any(active)) break;
        if (!active) continue;

        uint32_t* seq = hopseq + q * H;
        uint8_t status = OVS_LOOKUP_OK;
        bool fin = false;
        uint32_t Rn = NONE;
        const uint32_t c = local ? S : cur;
        const BRec Rc = load_brec(V.rec, c);
        BExt e2 = e;
        bool brother;
        const BAns a = broose_find_node_dev(V, c, Rc, K, e2, right, 1, &brother);
        if (local) {
            // IterativeLookup::start (133-244): findNode at the source; the source counts as visited
            local = false;
            sx = Rc.x; sy = Rc.y;
            if (a.broken) { fin = true; status = OVS_LOOKUP_BROKEN; }
            else if (a.sib) { fin = true; Rn = a.first; }
            else if (a.first == S) { fin = true; status = OVS_LOOKUP_NO_NEXT; }   // a brother lookup whose best is the source
            else { cur = a.first; e = e2; src_brother = brother; ntry = 1; }
        } else if (a.broken) {
            ++nrpc;
            fin = true; status = OVS_LOOKUP_BROKEN;    // the responder's findNode errors
        } else {
            // FindNodeCall S -> c and its FindNodeResponse (one NodeHandle), both with the extension
            ++nrpc;
            const int64_t cd = coord_ns(sx, sy, Rc.x, Rc.y, DC.round);
            const int64_t rtt = DC.msgCall + DC.msgResp1 + 2 * cd;
            if (rtt >= DC.rpcTimeout) {
                // handleTimeout (IterativeLookup.cc:935-1023): the path goes on with its next unused next hop.
                // Only the source's local findNode leaves more than one (it asks for getMaxNumRedundantNodes()
                // = bucketSize nodes, 159); every response replaces them by its single node.
                t += DC.rpcTimeout;
                if (t > DC.lookupTimeout) { fin = true; status = OVS_LOOKUP_TIMEOUT; }
                else if (hops == 0 && ntry < V.sh.k) {
                    const BRec Rs = load_brec(V.rec, S);
                    BAns as;
                    answer_row(V, S, K, e, src_brother, as);
                    K160 bd;
                    const uint32_t nx = scan_row(as.row, as.cap, S, Rs.k, as.tgt, true, k_xor(Rc.k, as.tgt), &bd);
                    if (nx == NONE || nx == S) { fin = true; status = OVS_LOOKUP_RPC_TIMEOUT; }
                    else { cur = nx; ++ntry; }
                } else {
                    fin = true; status = OVS_LOOKUP_RPC_TIMEOUT;
                }
            } else {
                t += rtt;
                if (t > DC.lookupTimeout) { fin = true; status = OVS_LOOKUP_TIMEOUT; }
                else {
                    if (hops < hcm) seq[hops] = c;
                    ++hops;
                    vis |= vis_bit(c);
                    if (a.sib) { fin = true; Rn = a.first; }
                    else if (hops >= hcm) { fin = true; status = OVS_LOOKUP_HOPMAX; }
                    else {
                        // visitOnlyOnce: the next hop must not be the source or an earlier responder
                        const uint32_t nx = a.first;
                        bool seen = nx == S;
                        if (!seen && (vis & vis_bit(nx)))
                            for (int i = 0; i < hops && !seen; ++i) seen = seq[i] == nx;
                        if (seen) { fin = true; status = OVS_LOOKUP_NO_NEXT; }
                        else { cur = nx; e = e2; }
                    }
                }
            }
        }
        if (fin) {
            // the route message goes to getResult()[0]: the closest node the sibling knows, not always the
            // sibling itself
            double rx = Rc.x, ry = Rc.y;
            if (status == OVS_LOOKUP_OK && Rn != S && Rn != c) {
                const BRec Rr = load_brec(V.rec, Rn);
                rx = Rr.x; ry = Rr.y;
            }
            out[q] = iter_route_out(status, hops, t, Rn, S, sx, sy, rx, ry, DC);
            if (rpcs) rpcs[q] = nrpc;
            active = false;
        }
    }
}

BView make_view(const BrooseTables& t)
{
    BView V;
    V.rec = t.rec; V.rows = t.rows; V.n = t.n; V.sh = t.sh;
    return V;
}

hipError_t finish_build(const KeyRec* recs, const double2* xy, uint32_t n, BrooseTables& t, hipStream_t st)
{
    hipLaunchKernelGGL(k_broose_rec, dim3(nblk(n, 256)), dim3(256), 0, st, recs, xy, n, t.sh, t.rows, t.rec);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return hipStreamSynchronize(st);
}

hipError_t alloc_tables(uint32_t n, const BrooseShape& sh, BrooseTables& t)
{
    broose_free(t);
    if (n < 2 || sh.P() * sh.kr > BROOSE_MAX_ROW || 7 * sh.k > BROOSE_MAX_ROW || sh.sb < 1) return hipErrorInvalidValue;
    t.n = n;
    t.sh = sh;
    hipError_t e = hipMalloc(&t.rec, sizeof(BrooseRec) * (uint64_t)n);
    if (e != hipSuccess) return e;
    return hipMalloc(&t.rows, sizeof(KeyRec) * (uint64_t)n * sh.stride());
}

}  // namespace

hipError_t broose_build(const KeyRec* recs, const double2* xy, uint32_t n, const BrooseShape& sh, BrooseTables& t, hipStream_t st)
{
    hipError_t e = alloc_tables(n, sh, t);
    if (e != hipSuccess) return e;
    const uint64_t rows = (uint64_t)n * (uint64_t)sh.nrows();
    hipLaunchKernelGGL(k_broose_rows, dim3(nblk(rows, 64)), dim3(64), 0, st, recs, n, sh, t.rows);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return finish_build(recs, xy, n, t, st);
}

hipError_t broose_build_from_csr(const KeyRec* recs, const double2* xy, uint32_t n, const BrooseShape& sh, const uint64_t* doff,
                                 const uint32_t* dnodes, BrooseTables& t, hipStream_t st)
{
    hipError_t e = alloc_tables(n, sh, t);
    if (e != hipSuccess) return e;
    const uint64_t rows = (uint64_t)n * (uint64_t)sh.nrows();
    hipLaunchKernelGGL(k_broose_rows_csr, dim3(nblk(rows, 256)), dim3(256), 0, st, recs, n, sh, doff, dnodes, t.rows);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return finish_build(recs, xy, n, t, st);
}

hipError_t broose_row_nodes(const BrooseTables& t, uint32_t* dout, hipStream_t st)
{
    const uint64_t total = (uint64_t)t.n * t.sh.stride();
    hipLaunchKernelGGL(k_broose_row_nodes, dim3(nblk(total, 256)), dim3(256), 0, st, t.rows, total, dout);
    return hipGetLastError();
}

hipError_t broose_find_node(const BrooseTables& t, const uint32_t* node, const K160* keys, BExt* ext, const uint8_t* right,
                            uint64_t nq, int numRedundantNodes, int numSiblings, uint32_t* out_nodes, uint32_t max_out,
                            uint8_t* count, uint8_t* sib, uint8_t* status, hipStream_t st)
{
    if (nq == 0) return hipSuccess;
    hipLaunchKernelGGL(k_broose_find_node, dim3(nblk(nq, 128)), dim3(128), 0, st, make_view(t), node, keys, ext, right, nq,
                       numRedundantNodes, numSiblings, out_nodes, max_out, count, sib, status);
    return hipGetLastError();
}

hipError_t broose_route(const BrooseTables& t, const DelayConsts& DC, int hopCountMax, const K160* keys, const uint32_t* src,
                        const uint8_t* right, uint64_t nq, ovs_route_out* out, uint32_t* hopseq, uint32_t* rpcs, int num_cu,
                        hipStream_t st, unsigned long long* dyn)
{
    if (nq == 0) return hipSuccess;
    // the hop list holds hopCountMax responders and is the visitOnlyOnce list: no limit, no list
    if (!hopseq || hopCountMax < 1) return hipErrorInvalidValue;
    using K = PersistKernel<k_broose_route>;
    const PersistLaunch pl = persist_launch<K::fn>(nq, num_cu, dyn, K4_TUNE);
    hipLaunchKernelGGL(K::fn, dim3(pl.blocks), dim3(256), 0, st, make_view(t), DC, hopCountMax, keys, src, right, nq, pl.chunk,
                       pl.dy, out, hopseq, rpcs);
    return hipGetLastError();
}

}  // namespace ovs
