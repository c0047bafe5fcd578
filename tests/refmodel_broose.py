"""Direct Python reading of Broose (src/overlay/broose/Broose.cc, BrooseBucket.cc) for the tests.

Test infrastructure only, written from the reference, not from the kernel: buckets are sorted maps
fed through BrooseBucket::add, findNode works on a real extension-message object that travels from
call to response to next call, and the lookup is IterativeLookup's single path (lookupParallelRpcs =
lookupRedundantNodes = 1, merge off, visitOnlyOnce) with RPC and lookup timeouts.  Delay helpers are
tests/refmodel.py's.

Cites: BrooseBucket.cc:49-68 (initializeBucket), 70-115 (add), 202-209 (longestPrefix), 239-260
(keyInRange); Broose.cc:145-164, 233-239 (changeState), 574-770 (findNode), 823-854 (isSiblingFor),
1116-1122 (addNode); BrooseMessage.msg:40; IterativeLookup.cc:133-244, 803-921, 935-1023, 1067-1170;
BaseOverlay.cc:1841-1914 (findNodeRpc).
"""
from __future__ import annotations

import bisect
import random

from refmodel import coord_ns, msg_ns, simtime, to_int

KEYLEN = 160
M = 1 << KEYLEN
NONE = 0xFFFFFFFF
# the largest distance estimate for which the left-shifting start's `int prefix` (Broose.cc:647-650)
# is defined: bit << (dist - i - 1) reaches the sign bit of int at dist = 32
MAX_LEFT_DIST = 31

# message lengths in bits (CommonMessages.msg, BrooseMessage.msg:33-40): the extension message is not a
# whole number of bytes, so lengths are summed in bits and rounded up once (cPacket::getByteLength)
FINDNODECALL_BITS = 440
FINDNODERESPONSE_BITS = 264
NODEHANDLE_BITS = 208
AUTHBLOCK_BITS = 800
BROOSE_EXT_BITS = 160 + 8 + 1 + 208      # KEY_L + STEP_L + RIGHTSHIFTING_L + NODEHANDLE_L
UDP_IP_BYTES = 28


class BrooseError(Exception):
    """where the reference calls error(), reads a bit outside the key, or is undefined"""


def shared_prefix_length(a: int, b: int) -> int:
    """OverlayKey::sharedPrefixLength (OverlayKey.cc:530-555), bitsPerDigit = 1"""
    return KEYLEN if a == b else KEYLEN - (a ^ b).bit_length()


def get_bit(key: int, pos: int) -> int:
    if pos < 0 or pos >= KEYLEN:
        raise BrooseError(f"bit position {pos} outside the key")
    return (key >> pos) & 1


def call_bytes(ext=True) -> int:
    return (FINDNODECALL_BITS + (BROOSE_EXT_BITS if ext else 0) + 7) // 8 + UDP_IP_BYTES


def resp_bytes(nodes: int, ext=True, auth=False) -> int:
    bits = FINDNODERESPONSE_BITS + NODEHANDLE_BITS * nodes + (AUTHBLOCK_BITS if auth else 0)
    return (bits + (BROOSE_EXT_BITS if ext else 0) + 7) // 8 + UDP_IP_BYTES


class BrooseBucket:
    """std::map<OverlayKey, BrooseHandle> ordered by bucket key XOR node key"""

    def __init__(self, self_key: int, shifting_bits: int, prefix: int, size: int, is_b=False):
        # initializeBucket (BrooseBucket.cc:49-68)
        self.max_size, self.is_b, self.self_key = size, is_b, self_key
        key = (self_key << -shifting_bits) % M if shifting_bits < 0 else self_key >> shifting_bits
        if prefix != 0:
            key = (key + ((prefix << (KEYLEN - shifting_bits)) % M)) % M
        self.key = key
        self.dist: list[int] = []       # the map's keys, ascending
        self.node: dict[int, int] = {}  # distance -> node index

    def add(self, node: int, node_key: int) -> bool:
        # BrooseBucket.cc:70-115 (lastSeen / rtt bookkeeping carries no routing decision)
        tmp = self.key ^ node_key
        if tmp not in self.node:
            if len(self.dist) >= self.max_size:
                if self.dist[-1] > tmp:
                    del self.node[self.dist.pop()]
                else:
                    return False
            bisect.insort(self.dist, tmp)
            self.node[tmp] = node
        return True

    def nodes(self) -> list[int]:
        return [self.node[d] for d in self.dist]       # fillVector order

    def longest_prefix(self, ids) -> int:
        if len(self.dist) < 2:
            return 0
        return shared_prefix_length(ids[self.node[self.dist[0]]], ids[self.node[self.dist[-1]]])

    def key_in_range(self, key: int) -> bool:
        # BrooseBucket.cc:239-260
        if not self.dist:
            return False
        if self.is_b:
            if len(self.dist) <= self.max_size // 7:
                return True
            d = self.dist[self.max_size // 7 - 1]
        else:
            d = self.dist[-1]
        return (key ^ self.self_key) <= d


class Ext:
    """BrooseFindNodeExtMessage"""

    def __init__(self, route_key=0, step=0, right=False, last_node=NONE):
        self.route_key, self.step, self.right, self.last_node = route_key, step, right, last_node

    def copy(self):
        return Ext(self.route_key, self.step, self.right, self.last_node)

    def tup(self):
        return (self.route_key, self.step, bool(self.right))


def closest_brute(ids, target: int, m: int) -> list[int]:
    return sorted(range(len(ids)), key=lambda j: ids[j] ^ target)[:m]


def closest_fast(ids, target: int, m: int) -> list[int]:
    """the same set by descending the binary trie of the sorted ids: at a split the side that shares the
    target's bit is closer than all of the other side"""
    lo, hi, need, out = 0, len(ids), m, []
    while need > 0 and hi > lo:
        if hi - lo <= need:
            out.extend(range(lo, hi))
            break
        b = (ids[lo] ^ ids[hi - 1]).bit_length() - 1
        thr = ((ids[lo] >> (b + 1)) << (b + 1)) | (1 << b)
        mid = bisect.bisect_left(ids, thr, lo, hi)
        near, far = ((mid, hi), (lo, mid)) if (target >> b) & 1 else ((lo, mid), (mid, hi))
        if near[1] - near[0] >= need:
            lo, hi = near
        else:
            out.extend(range(*near))
            need -= near[1] - near[0]
            lo, hi = far
    return sorted(out, key=lambda j: ids[j] ^ target)


class BrooseNet:
    """A network of READY Broose nodes with fixed tables.

    build = "add": every node's buckets are fed every node of the network through BrooseBucket::add in a
    shuffled order (seeded), the node's own handle included (changeState(READY), Broose.cc:233-239);
    build = "fast": the same contents from closest_fast; rows = explicit tables (row_off, row_nodes) in
    the engine's CSR form, fed through add in the given order."""

    def __init__(self, ids_words, xy, bucket_size=8, r_bucket_size=8, user_dist=0, shifting_bits=2,
                 build="fast", rows=None, rnd=True, seed=1, nodes=None):
        self.ids = [to_int(w) for w in ids_words]
        assert all(self.ids[i] < self.ids[i + 1] for i in range(len(self.ids) - 1))
        self.n, self.xy, self.rnd = len(self.ids), xy, rnd
        self.k, self.kr, self.user_dist, self.sb = bucket_size, r_bucket_size, user_dist, shifting_bits
        self.P = 1 << shifting_bits
        self.nrows = self.P + 2
        self.choose_lookup = [0] * self.n
        self.buckets: dict[int, list[BrooseBucket]] = {}
        rng = random.Random(seed)
        for v in (range(self.n) if nodes is None else nodes):
            bs = self.new_buckets(v)
            if rows is not None:
                off, nd = rows
                for r, b in enumerate(bs):
                    for j in nd[int(off[v * self.nrows + r]):int(off[v * self.nrows + r + 1])]:
                        b.add(int(j), self.ids[int(j)])
            elif build == "add":
                order = list(range(self.n))
                rng.shuffle(order)
                for j in order:
                    self.add_node(bs, j)
            else:
                for b in bs:
                    for j in closest_fast(self.ids, b.key, b.max_size):
                        b.add(j, self.ids[j])
            self.buckets[v] = bs

    # rows of a node: rBucket[0 .. P-1], lBucket, bBucket
    def new_buckets(self, v) -> list[BrooseBucket]:
        me = self.ids[v]
        # changeState(INIT) (Broose.cc:158-164)
        bs = [BrooseBucket(me, self.sb, i, self.kr) for i in range(self.P)]
        bs.append(BrooseBucket(me, -self.sb, 0, self.P * self.kr))
        bs.append(BrooseBucket(me, 0, 0, 7 * self.k, is_b=True))
        return bs

    def add_node(self, bs, j) -> bool:
        """Broose::addNode (1116-1122); True when some bucket's membership changed"""
        changed = False
        for b in bs:
            before = list(b.dist)
            b.add(j, self.ids[j])
            changed |= before != b.dist
        return changed

    def rows(self, v) -> list[list[int]]:
        return [b.nodes() for b in self.buckets[v]]

    def csr(self):
        off, nd = [0], []
        for v in range(self.n):
            for row in self.rows(v):
                nd.extend(row)
                off.append(len(nd))
        return off, nd

    def r_bucket(self, v, i): return self.buckets[v][i]
    def l_bucket(self, v): return self.buckets[v][self.P]
    def b_bucket(self, v): return self.buckets[v][self.P + 1]

    # -- Broose::isSiblingFor (823-854), node == thisNode, state READY
    def is_sibling_for(self, v, key, num_siblings) -> bool:
        if num_siblings > self.k:
            raise BrooseError("numSiblings too big!")
        if num_siblings == -1:
            num_siblings = self.k
        if num_siblings == 0:
            return self.ids[v] == key
        return self.b_bucket(v).key_in_range(key)

    def node_vector(self, cands, target, size) -> list[int]:
        """NodeVector(size) with KeyDistanceComparator<KeyXorMetric>(target): distinct nodes, closest first"""
        return sorted(set(cands), key=lambda j: self.ids[j] ^ target)[:size]

    def distance_estimate(self, v) -> int:
        # Broose.cc:629-641
        dist = max(self.r_bucket(v, 0).longest_prefix(self.ids), self.r_bucket(v, 1).longest_prefix(self.ids)) + 1 + self.user_dist
        if dist % self.sb:
            dist += self.sb - dist % self.sb
        if dist > KEYLEN:
            dist = KEYLEN if KEYLEN % self.sb == 0 else KEYLEN - KEYLEN % self.sb
        return dist

    # -- Broose::findNode (574-770); msg: dict, the call message ("ext" = its findNodeExt object)
    def find_node(self, v, key, num_redundant, num_siblings, msg, right=None, count=None):
        """right: the direction of an extension created here (None: the node's chooseLookup counter).
        count: a one-element list that collects how often findNode ran (the self-recursion included)."""
        me = self.ids[v]
        for _ in range(2 * KEYLEN + 2):
            if count is not None:
                count[0] += 1
            sib = self.is_sibling_for(v, key, num_siblings)
            if num_siblings < 0:
                size = num_redundant
            else:
                size = (num_siblings if num_siblings else 1) if sib else num_redundant
            assert num_siblings or num_redundant
            if sib:
                return self.node_vector(self.b_bucket(v).nodes() + [v], key, size)
            if msg is None:
                raise BrooseError("findNode without a message dereferences a null extension")
            if "ext" not in msg:
                ext = Ext()
                dist = self.distance_estimate(v)
                go_right = (self.choose_lookup[v] % 2 != 0) if right is None else bool(right)
                self.choose_lookup[v] += 1
                if not go_right:
                    if dist > MAX_LEFT_DIST:
                        raise BrooseError("int prefix undefined for dist > 31")
                    prefix = 0
                    for i in range(dist):
                        prefix += get_bit(me, KEYLEN - i - 1) << (dist - i - 1)
                    ext.right = False
                    ext.route_key = ((key >> dist) + ((prefix << (KEYLEN - dist)) % M)) % M
                    dist = -dist
                else:
                    ext.right = True
                    ext.route_key = me
                ext.last_node = v
                ext.step = dist
                msg["ext"] = ext
            ext = msg["ext"]
            # addNode(lastNode) / setLastSeen (675-676): tables are fixed within a batch
            ext.last_node = v
            if ext.step == 0:
                return self.node_vector(self.b_bucket(v).nodes() + [v], key, size)
            if not ext.right:
                if ext.step > 0:
                    raise BrooseError("left-shifting step above 0 never reaches the brother lookup")
                ext.route_key = (ext.route_key << self.sb) % M
                ext.step += self.sb
                res = self.node_vector(self.l_bucket(v).nodes() + [v], ext.route_key, size)
            else:
                dist = ext.step
                rk = ext.route_key >> self.sb
                prefix = 0
                for i in range(self.sb):
                    prefix += get_bit(key, KEYLEN - dist + i) << i
                rk = (rk + ((prefix << (KEYLEN - self.sb)) % M)) % M
                ext.route_key = rk
                ext.step = dist - self.sb
                res = self.node_vector(self.r_bucket(v, prefix).nodes() + [v], rk, size)
            if res[0] != v:
                return res
        raise BrooseError("findNode self-recursion did not end")

    # -- KBRTestApp one-way route over IterativeLookup (iterative, one path, one RPC in flight)
    def lookup(self, kw, S, right, hop_max=50, rpc_to=1.5, lk_to=10.0, auth=False, test_msg=100):
        k = kw if isinstance(kw, int) else to_int(kw)
        rnd = self.rnd
        fail = lambda st, hops, seq, rpcs, fn: dict(responsible=NONE, hops=hops, status=st, one_way_hops=0, latency_ns=-1,
                                                    hop_seq=seq, rpcs=rpcs, find_nodes=fn)
        T_rpc, T_lk = simtime(rpc_to, rnd), simtime(lk_to, rnd)
        m_call = msg_ns(call_bytes(), rnd)
        m_resp = msg_ns(resp_bytes(1, auth=auth), rnd)
        m_route = msg_ns(58 + test_msg + 28, rnd)
        fn = [0]
        # IterativeLookup::start (133-244): the local findNode asks for getMaxNumRedundantNodes() nodes
        msg = {}
        try:
            nxt = self.find_node(S, k, self.k, 1, msg, right, fn)
        except BrooseError:
            return fail(5, 0, [], 0, fn[0])
        t, hops, seq, rpcs, visited = 0, 0, [], 0, {S}
        if self.is_sibling_for(S, k, 1):
            R = nxt[0]
            lat = msg_ns(58 + test_msg + 28, rnd) + coord_ns(self.xy, S, R, rnd) if R != S else 0
            return dict(responsible=R, hops=0, status=0, one_way_hops=int(R != S), latency_ns=lat, hop_seq=[], rpcs=0,
                        find_nodes=fn[0])
        ext = msg["ext"]
        cands, used, after_timeout = list(nxt), 0, False
        while True:
            # IterativePathLookup::sendRpc (1067-1170): one entry is looked at (redundantNodes = 1)
            if hop_max and hops >= hop_max:
                return fail(3, hops, seq, rpcs, fn[0])
            if used >= len(cands) or cands[used] in visited:
                return fail(2 if after_timeout else 4, hops, seq, rpcs, fn[0])
            cur = cands[used]
            used += 1
            rpcs += 1
            call = {"ext": ext.copy()}
            try:
                res = self.find_node(cur, k, 1, 1, call, None, fn)     # findNodeRpc (BaseOverlay.cc:1857)
            except BrooseError:
                return fail(5, hops, seq, rpcs, fn[0])
            sib = self.is_sibling_for(cur, k, 1)
            cd = coord_ns(self.xy, S, cur, rnd)
            rtt = m_call + cd + m_resp + cd
            if rtt >= T_rpc:
                # handleTimeout (935-1023): the next of the source's candidates with the same extension
                t += T_rpc
                if t > T_lk:
                    return fail(1, hops, seq, rpcs, fn[0])
                after_timeout = True
                continue
            t += rtt
            if t > T_lk:
                return fail(1, hops, seq, rpcs, fn[0])
            after_timeout = False
            hops += 1
            seq.append(cur)
            visited.add(cur)
            if sib:
                R = res[0]
                lat = t + (m_route + coord_ns(self.xy, S, R, rnd) if R != S else 0)
                return dict(responsible=R, hops=hops, status=0, one_way_hops=hops + int(R != S), latency_ns=lat, hop_seq=seq,
                            rpcs=rpcs, find_nodes=fn[0])
            cands, used, ext = list(res), 0, call["ext"]     # merge off: the response replaces the next hops


def directions(src, creates, parity=None, n=None):
    """The direction flag per lookup that chooseLookup++ (Broose.cc:643) gives when the batch runs in
    order: lookup i turns right iff its source has created an odd number of extensions before it.
    creates[i]: lookup i creates one (its source is no sibling of its key).  -> (flags, parities after)"""
    par = {} if parity is None else dict(enumerate(parity))
    out = []
    for s, c in zip(src, creates):
        p = par.get(int(s), 0)
        out.append(p % 2 != 0)
        if c:
            par[int(s)] = p + 1
    return out, par
