// broose_host.hpp -- what Broose's host and device code share and a plain C++ compiler can build: the
// bucket shape, the bucket keys and the validation of explicit tables (tests/broose_tables_driver.cpp
// runs it under the sanitizers without a HIP compiler).
#pragma once
#include <stdint.h>

#include <string>

#include "key160.hpp"

namespace ovs {

constexpr int BROOSE_MAX_ROW = 64;   // the longest row the snapshot build stages (bBucket: 56 at bucketSize 8)

// bucket sizes and places of one node's rows: rBucket[0 .. P-1], lBucket, bBucket (Broose.cc:158-164)
struct BrooseShape {
    int k = 8;           // bucketSize
    int kr = 8;          // rBucketSize
    int userDist = 0;
    int sb = 2;          // brooseShiftingBits
    OVS_HD int P() const { return 1 << sb; }
    OVS_HD int nrows() const { return P() + 2; }
    OVS_HD int cap(int row) const { return row < P() ? kr : (row == P() ? P() * kr : 7 * k); }
    OVS_HD uint32_t at(int row) const { return (uint32_t)(row <= P() ? row * kr : 2 * P() * kr); }
    OVS_HD uint32_t stride() const { return (uint32_t)(2 * P() * kr + 7 * k); }
};

// OverlayKey::operator<< / operator>> (OverlayKey.cc:386-425) trimmed to 160 bits, exact for every count
OVS_HD K160 b_shl(const K160& a, int n)
{
    K160 r;
    const int q = n >> 5, b = n & 31;
    for (int i = 0; i < 5; ++i) {
        const uint32_t hi = k_word(a, i - q), lo = (i - q - 1 >= 0) ? k_word(a, i - q - 1) : 0u;
        r.w[i] = (i - q < 0 || n >= 160) ? 0u : (b ? (hi << b) | (lo >> (32 - b)) : hi);
    }
    return r;
}
OVS_HD K160 b_shr(const K160& a, int n)
{
    K160 r;
    const int q = n >> 5, b = n & 31;
    for (int i = 0; i < 5; ++i) {
        const uint32_t lo = k_word(a, i + q), hi = k_word(a, i + q + 1);
        r.w[i] = (n >= 160) ? 0u : (b ? (lo >> b) | (hi << (32 - b)) : lo);
    }
    return r;
}

// BrooseBucket::initializeBucket (BrooseBucket.cc:49-68) for row `row` of the node with key `me`
OVS_HD K160 broose_bucket_key(const BrooseShape& sh, const K160& me, int row)
{
    if (row == sh.P() + 1) return me;
    if (row == sh.P()) return b_shl(me, sh.sb);
    K160 pre;
    pre.w[0] = (uint32_t)row; pre.w[1] = 0; pre.w[2] = 0; pre.w[3] = 0; pre.w[4] = 0;
    return k_add(b_shr(me, sh.sb), b_shl(pre, 160 - sh.sb));
}

// the parameter ranges the engine implements; false + *err otherwise
inline bool broose_shape_ok(const BrooseShape& sh, std::string* err)
{
    if (sh.sb < 1 || sh.sb > 4) { *err = "brooseShiftingBits must be 1..4"; return false; }
    if (sh.k < 1 || sh.k > 8) { *err = "bucketSize must be 1..8"; return false; }
    if (sh.kr < 1 || sh.kr > 16) { *err = "rBucketSize must be 1..16"; return false; }
    if (sh.userDist < 0 || sh.userDist > 160) { *err = "userDist must be 0..160"; return false; }
    if (sh.P() * sh.kr > BROOSE_MAX_ROW) { *err = "2^brooseShiftingBits * rBucketSize must be <= 64 (the lBucket row)"; return false; }
    return true;
}

// Explicit tables in CSR form: row r of node v = row_nodes[row_off[v * nrows + r] .. row_off[v * nrows + r + 1]).
// Every row must be what a BrooseBucket can hold: offsets from 0 and never decreasing, at most maxSize
// members, members nodes of [0, n), strictly ascending in XOR distance to the bucket key (the map's order;
// this also excludes a node twice).  false + *err naming the node otherwise.
inline bool broose_validate_tables(const K160* ids, uint64_t n, const BrooseShape& sh, const uint64_t* row_off,
                                   const uint32_t* row_nodes, std::string* err)
{
    const uint64_t nr = (uint64_t)sh.nrows();
    if (row_off[0] != 0) { *err = "row_off[0] must be 0"; return false; }
    for (uint64_t v = 0; v < n; ++v) {
        for (uint64_t r = 0; r < nr; ++r) {
            const uint64_t a = row_off[v * nr + r], b = row_off[v * nr + r + 1];
            const std::string where = "node " + std::to_string(v) + " row " + std::to_string(r);
            if (b < a) { *err = where + ": offsets decrease"; return false; }
            if (b - a > (uint64_t)sh.cap((int)r)) { *err = where + ": longer than the bucket's maxSize"; return false; }
            const K160 bk = broose_bucket_key(sh, ids[v], (int)r);
            K160 prev{};
            for (uint64_t j = a; j < b; ++j) {
                if (row_nodes[j] >= n) { *err = where + ": node index out of range"; return false; }
                const K160 d = k_xor(bk, ids[row_nodes[j]]);
                if (j > a && !k_lt(prev, d)) { *err = where + ": not in ascending XOR order to the bucket key"; return false; }
                prev = d;
            }
        }
    }
    return true;
}

}  // namespace ovs
