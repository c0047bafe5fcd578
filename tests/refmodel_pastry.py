"""Pastry with fixed tables, restated line by line in pure Python: the checker of oversim_amd/csrc/pastry.hip.

Test infrastructure only.  Nodes are indices into the sorted id list, None is NodeHandle::UNSPECIFIED_NODE.

Cites: PastryStateObject.cc:107-173 (keyDist, isCloser, specialCloserCondition), OverlayKey.cc:530-555
(sharedPrefixLength), Comparator.h:111-132 (KeyRingMetric), NodeVector.h:381-512 (the sorted add),
PastryLeafSet.cc:58-89, 106-161, 220-484, PastryRoutingTable.cc:28-196, BasePastry.cc:919-952, 1090-1211,
BaseOverlay.cc:907-918 (receipt), 1443-1582 (the recursive branch of sendToKey).
"""
from __future__ import annotations

import bisect

import numpy as np

from refmodel import M, between, between_lr, coord_ns, msg_ns, to_int

NONE = 0xFFFFFFFF
OK, HOPMAX, NO_NEXT, BROKEN = 0, 3, 4, 5


class PastryError(Exception):
    """The reference throws, or dereferences a NULL NodeVector."""


# --- key arithmetic ------------------------------------------------------------------------------
def key_dist(a: int, b: int) -> int:
    """PastryStateObject::keyDist (107-132)."""
    smaller, bigger = (b, a) if a > b else (a, b)
    diff1 = (bigger - smaller) % M
    diff2 = (smaller + ((M - 1) - bigger) + 1) % M
    return diff2 if diff1 > diff2 else diff1


def ring_dist(x: int, y: int) -> int:
    """KeyRingMetric::distance (Comparator.h:121-131)."""
    d1, d2 = (x - y) % M, (y - x) % M
    return d2 if d1 > d2 else d1


def shared_prefix_length(a: int, b: int, bits_per_digit: int = 1) -> int:
    """OverlayKey::sharedPrefixLength (530-555): equal keys give keyLength whatever the digit size."""
    if a == b:
        return 160
    return (160 - (a ^ b).bit_length()) // bits_per_digit


def _btw(x, a, b):
    """isBetween with unspecified keys (OverlayKey.cc:590)."""
    return x is not None and a is not None and b is not None and between(x, a, b)


def sorted_vector(cands, key_of, target, max_size):
    """BaseKeySortedVector::add (NodeVector.h:381-512) of cands in order under KeyDistanceComparator<KeyRingMetric>:
    a key once, before the first strictly farther entry, cut to max_size after every add (0: no limit)."""
    v = []
    for c in cands:
        d = ring_dist(key_of(c), target)
        if max_size and len(v) == max_size and d > ring_dist(key_of(v[-1]), target):
            continue                                            # isAddable
        pos, dup = len(v), False
        for i, e in enumerate(v):
            if key_of(e) == key_of(c):
                dup = True
                break
            if d < ring_dist(key_of(e), target):
                pos = i
                break
        if dup:
            continue
        v.insert(pos, c)
        if max_size and len(v) > max_size:
            del v[max_size:]
    return v


# --- one node's state ----------------------------------------------------------------------------
class PastryNode:
    def __init__(self, net, me: int):
        self.net, self.me = net, me
        L = net.L
        self.leaves = [None] * L                                # initializeSet (58-89)
        self.bigger, self.smaller = L >> 1, (L >> 1) - 1
        self.is_full = False
        self.rows = []                                          # routing table rows of 2^b entries

    def key(self, x):
        return None if x is None else self.net.ids[x]

    # PastryStateObject
    def is_closer(self, test, dest, ref=None):
        """isCloser (134-155); ref None = the owner."""
        if ref is None:
            ref = self.me
        if self.key(ref) == dest or test == ref:
            return False
        return key_dist(self.key(test), dest) < key_dist(self.key(ref), dest)

    def special_closer(self, test, dest, ref=None):
        """specialCloserCondition (157-173)."""
        b = self.net.b
        if shared_prefix_length(self.key(test), dest, b) < shared_prefix_length(self.key(self.me), dest, b):
            return False
        return self.is_closer(test, dest, ref)

    # PastryLeafSet
    def merge_node(self, node):
        """mergeNode (261-327) without callUpdate."""
        lv, nk, own = self.leaves, self.key(node), self.key(self.me)
        last_left = last_right = own
        il, ir = self.smaller, self.bigger
        for x in lv:
            if x is None:
                self.is_full = False
                continue
            if self.key(x) == nk:
                return False
        while True:
            if not self.is_full:
                if lv[il] is None and lv[ir] is None:
                    self._insert(il, node)
                    return True
                if lv[il] is None and not _btw(nk, last_right, self.key(lv[ir])):
                    self._insert(il, node)
                    return True
                if lv[ir] is None and not _btw(nk, self.key(lv[il]), last_left):
                    self._insert(ir, node)
                    return True
            if _btw(nk, self.key(lv[il]), last_left):
                self._insert(il, node)
                return True
            if _btw(nk, last_right, self.key(lv[ir])):
                self._insert(ir, node)
                return True
            last_right = self.key(lv[ir])
            ir += 1
            if ir == len(lv):
                break
            last_left = self.key(lv[il])
            il -= 1
        return False

    def _insert(self, it, node):
        """insertLeaf (329-378)."""
        lv = self.leaves
        if it <= self.smaller:
            lv.insert(it + 1, node)
            if lv[0] is not None and lv[-1] is None:
                lv[-1] = lv[0]
            del lv[0]
        else:
            lv.insert(it, node)
            if lv[-1] is not None and lv[0] is None:
                lv[0] = lv[-1]
            lv.pop()
        self.is_full = lv[0] is not None and lv[-1] is not None
        if not self.is_full:
            self._balance()

    def _balance(self):
        """balanceLeafSet (380-410)."""
        lv = self.leaves
        if self.is_full or (lv[0] is not None and lv[-2] is not None) or (lv[-1] is not None and lv[1] is not None):
            return False
        il, ir = self.smaller, self.bigger
        while ir != len(lv):
            if lv[il] is None:
                if lv[ir] is None or ir + 1 == len(lv) or lv[ir + 1] is None:
                    return False
                lv[il], lv[ir + 1] = lv[ir + 1], None
                return True
            if lv[ir] is None:
                if il == 0 or lv[il - 1] is None:
                    return False
                lv[ir], lv[il - 1] = lv[il - 1], None
                return True
            il -= 1
            ir += 1
        return False

    def smallest_node(self):
        """getSmallestNode (421-427)."""
        i = 0
        while self.leaves[i] is None and i != self.smaller:
            i += 1
        return self.leaves[i]

    def biggest_node(self):
        """getBiggestNode (434-440)."""
        i = len(self.leaves) - 1
        while self.leaves[i] is None and i != self.bigger:
            i -= 1
        return self.leaves[i]

    def destination_node(self, dest):
        """getDestinationNode (106-134)."""
        own = self.key(self.me)
        smallest, biggest = self.key(self.smallest_node()), self.key(self.biggest_node())
        if smallest is None:
            smallest = own
        if biggest is None:
            biggest = own
        if not between_lr(dest, smallest, biggest):
            return None
        ret = None
        for x in self.leaves:
            if x is not None and self.is_closer(x, dest, ret):
                ret = x
        return ret

    def is_closest_node(self, dest):
        """isClosestNode (136-161)."""
        if self.key(self.me) == dest:
            return True
        big, small = self.leaves[self.bigger], self.leaves[self.smaller]
        if big is None and small is None:
            return True
        bc = big is not None and self.is_closer(big, dest)
        sc = small is not None and self.is_closer(small, dest)
        return not bc and not sc

    def sibling_vector(self, key, num_siblings):
        """createSiblingVector (220-259); None = its NULL."""
        lv = self.leaves
        res = sorted_vector([self.me] + [x for x in lv if x is not None], self.key, key, num_siblings)
        if lv[self.smaller] is None or lv[self.bigger] is None:            # !isValid()
            return res
        if lv[0] is None or lv[-1] is None:
            return res
        keys = {self.key(x) for x in res}
        if self.key(self.biggest_node()) in keys or self.key(self.smallest_node()) in keys:
            return None
        return res

    def leaf_closer_node(self, dest, optimize=False):
        """PastryLeafSet::findCloserNode (458-484)."""
        ret = None
        smallest, biggest = self.smallest_node(), self.biggest_node()
        if smallest is not None and self.special_closer(smallest, dest, ret):
            if not optimize:
                return smallest
            ret = smallest
        if biggest is not None and self.special_closer(biggest, dest, ret):
            if not optimize:
                return biggest
            ret = biggest
        return ret

    # PastryRoutingTable
    def digit_at(self, n, key):
        """digitAt (28-32): getBitRange throws outside the key."""
        b = self.net.b
        p = 160 - (n + 1) * b
        if p < 0:
            raise PastryError("OverlayKey::get: Invalid range")
        return (key >> p) & ((1 << b) - 1)

    def node_at(self, row, col):
        """nodeAt (70-76) with the reference's unsigned arguments."""
        if row < 0 or col < 0 or row >= len(self.rows) or col >= (1 << self.net.b):
            return None
        return self.rows[row][col]

    def lookup_next_hop(self, dest):
        """lookupNextHop (78-98)."""
        own = self.key(self.me)
        if dest == own:
            raise PastryError("trying to lookup own key!")
        shl = shared_prefix_length(own, dest) // self.net.b
        digit = self.digit_at(shl, dest)
        return self.node_at(shl, digit)

    def table_closer_node(self, dest, optimize=False):
        """PastryRoutingTable::findCloserNode (100-180)."""
        own = self.key(self.me)
        if dest == own:
            raise PastryError("trying to find closer node to own key!")
        if not optimize:
            for y in range(len(self.rows)):
                for x in range(1 << self.net.b):
                    e = self.node_at(y, x)
                    if e is not None and self.special_closer(e, dest):
                        return e
            return None
        ret = None
        shl = shared_prefix_length(own, dest) // self.net.b
        digit = self.digit_at(shl, dest)
        x = self.digit_at(shl, own)
        n = 1 << self.net.b
        a, b = digit - 1, digit + 1
        while a >= 0 or b < n:
            if a == x:
                a = -1
            if b == x:
                b = n
            if a >= 0:
                e = self.node_at(shl, a)
                if e is not None and self.special_closer(e, dest, ret):
                    ret = e
                a -= 1
            if b < n:
                e = self.node_at(shl, b)
                if e is not None and self.special_closer(e, dest, ret):
                    ret = e
                b += 1
        if shl != 0:
            shl -= 1
            e = self.node_at(shl, digit - 1 if dest < own else digit + 1)
            if e is not None and self.special_closer(e, dest, ret):
                ret = e
        return ret

    def table_nodes(self):
        """PastryRoutingTable::findCloserNodes (182-196): every entry, rows then columns."""
        return [e for row in self.rows for e in row if e is not None]

    # BasePastry
    def is_sibling_for(self, key, num_siblings):
        """isSiblingFor(thisNode, key, numSiblings, &err) (919-952) -> (sibling, err)."""
        if num_siblings == 1:
            return self.is_closest_node(key), False
        res = self.sibling_vector(key, num_siblings)
        if res is None:
            return False, True
        if self.key(self.me) in {self.key(x) for x in res}:
            return True, False
        return False, True

    def find_node(self, key, num_redundant, num_siblings):
        """BasePastry::findNode (1100-1211), state READY -> (nodes, info).  info: sib, err (isSiblingFor's),
        source of the next hop ('self', 'leaf', 'table', 'closer', 'none')."""
        net = self.net
        if num_redundant > net.L or num_siblings > net.L // 2:
            raise PastryError("numRedundantNodes or numSiblings too big!")
        info = dict(sib=False, err=False, source="none")
        hops = []
        if self.is_closest_node(key):
            hops.append(self.me)
            info["source"] = "self"
        else:
            nxt = self.destination_node(key)
            if nxt is not None:
                info["source"] = "leaf"
            else:
                nxt = self.lookup_next_hop(key)
                if nxt is not None:
                    info["source"] = "table"
            if nxt is None:
                if net.optimize:
                    nxt = self.table_closer_node(key, True)
                    tmp = self.leaf_closer_node(key, True)
                    if tmp is not None and self.is_closer(tmp, key, nxt):
                        nxt = tmp
                else:
                    nxt = self.table_closer_node(key)
                    if nxt is None:
                        nxt = self.leaf_closer_node(key)
                if nxt is not None:
                    info["source"] = "closer"
            if nxt is not None:
                hops.append(nxt)
        if num_siblings >= 0:
            sib, err = self.is_sibling_for(key, num_siblings)
            info["sib"], info["err"] = sib, err
            if sib and not err:
                res = self.sibling_vector(key, num_siblings)
                if res is None:
                    raise PastryError("findNode returns the NULL sibling vector")
                return res, info
        if num_redundant > 1:
            add = sorted_vector(self.table_nodes() + [x for x in self.leaves if x is not None], self.key, key,
                                num_redundant)
            if not add:
                raise PastryError("(*additionalHops)[0] of an empty vector")
            if net.regular and hops and add[0] != hops[0]:
                hops = hops + [a for a in add if a != hops[0]]              # push_back: no size limit
            else:
                return add, info
        return hops, info


# --- the network ---------------------------------------------------------------------------------
class PastryNet:
    """READY Pastry nodes on the sorted ids.  tables = (leaf [n][L], table [n][rows][2^b]) node indices with NONE,
    or None for the converged-table rule."""

    def __init__(self, ids_words, xy, bits_per_digit=4, number_of_leaves=16, optimize=False, regular=True, rnd=True,
                 tables=None, nodes=None):
        self.ids = [to_int(w) for w in ids_words] if not isinstance(ids_words[0], int) else list(ids_words)
        assert all(self.ids[i] < self.ids[i + 1] for i in range(len(self.ids) - 1))
        self.n, self.xy = len(self.ids), xy
        self.b, self.L, self.optimize, self.regular, self.rnd = bits_per_digit, number_of_leaves, optimize, regular, rnd
        self.nodes = {}
        for v in (range(self.n) if nodes is None else nodes):
            nd = PastryNode(self, v)
            if tables is None:
                nd.leaves = self.rule_leaves(v)
                nd.rows = self.rule_rows(v)
            else:
                nd.leaves = [None if x == NONE else int(x) for x in tables[0][v]]
                nd.rows = [[None if x == NONE else int(x) for x in row] for row in tables[1][v]]
            nd.is_full = nd.leaves[0] is not None and nd.leaves[-1] is not None
            self.nodes[v] = nd

    # the converged-table rule
    def rule_leaves(self, v):
        n, L = self.n, self.L
        if n - 1 >= L:
            h = L // 2
            return [(v - (h - j)) % n for j in range(h)] + [(v + 1 + j) % n for j in range(h)]
        return self.replay_leaves(v, [(v + 1 + j) % n for j in range(n - 1)])

    def replay_leaves(self, v, order):
        nd = PastryNode(self, v)
        for x in order:
            nd.merge_node(x)
        return nd.leaves

    def rule_entry(self, v, r, c):
        b, me = self.b, self.ids[v]
        p = 160 - (r + 1) * b
        if ((me >> p) & ((1 << b) - 1)) == c:
            return None
        t = (me & ~(((1 << b) - 1) << p)) | (c << p)
        base = (t >> p) << p
        lo = bisect.bisect_left(self.ids, base)
        hi = bisect.bisect_left(self.ids, base + (1 << p))
        if lo == hi:
            return None
        i = bisect.bisect_left(self.ids, t, lo, hi)
        return i if i < hi else lo

    def num_rows(self, v=None):
        """Rows up to the last non-empty one: of node v, or the largest of the network."""
        if v is None:
            return max(self.num_rows(u) for u in range(self.n))
        m = max(shared_prefix_length(self.ids[v], self.ids[u], self.b) for u in ((v - 1) % self.n, (v + 1) % self.n)
                if u != v)
        return m + 1

    def rule_rows(self, v):
        return [[self.rule_entry(v, r, c) for c in range(1 << self.b)] for r in range(self.num_rows(v))]

    def tables(self, rows=None):
        """(leaf [n][L], table [n][rows][2^b]) uint32 arrays, NONE = unspecified."""
        rows = rows or max(len(nd.rows) for nd in self.nodes.values())
        leaf = np.full((self.n, self.L), NONE, dtype=np.uint32)
        tab = np.full((self.n, rows, 1 << self.b), NONE, dtype=np.uint32)
        for v, nd in self.nodes.items():
            for j, x in enumerate(nd.leaves):
                if x is not None:
                    leaf[v, j] = x
            for r, row in enumerate(nd.rows):
                for c, x in enumerate(row):
                    if x is not None:
                        tab[v, r, c] = x
        return leaf, tab

    def owner(self, key):
        """The node with the smallest keyDist to key; ties are reported with both nodes."""
        i = bisect.bisect_left(self.ids, key) % self.n
        a, b = (i - 1) % self.n, i
        da, db = key_dist(self.ids[a], key), key_dist(self.ids[b], key)
        return (a, b) if da == db and a != b else ((a,) if da < db else (b,))

    def route(self, kw, S, rec_num_redundant=3, hop_max=50, route_bytes=186):
        """One semi-recursive route message (BaseOverlay.cc:907-918, 1443-1582) with numSiblings = 1, reported as
        ChordRing.lookup_recursive reports it."""
        k = kw if isinstance(kw, int) else to_int(kw)
        fail = lambda st, seq: dict(responsible=NONE, hops=0, status=st, one_way_hops=0, latency_ns=-1, hop_seq=seq)
        cur, last, t, hops, seq = S, None, 0, 0, []
        while True:
            nd = self.nodes[cur]
            done = lambda: dict(responsible=cur, hops=hops, status=OK, one_way_hops=hops, latency_ns=t, hop_seq=seq)
            if cur != S or hops:
                if nd.is_sibling_for(k, 1)[0]:                              # delivered on receipt (907-918)
                    return done()
            try:
                cands, _ = nd.find_node(k, rec_num_redundant, 1)
            except PastryError:
                return fail(BROKEN, seq)
            if not cands:
                return fail(NO_NEXT, seq)                                   # "FindNode() returned NULL"
            if hops >= hop_max:
                return fail(HOPMAX, seq)                                    # 1464-1489
            sib, err = nd.is_sibling_for(k, 1)
            nxt = None
            for c in cands:                                                 # 1507-1521
                if (last == c and c != cur) or (c == S and cur != S) or (c == cur and not sib):
                    continue
                nxt = c
                break
            if nxt is None:
                return fail(NO_NEXT, seq)
            if nxt == cur:
                return done()
            t += msg_ns(route_bytes, self.rnd) + coord_ns(self.xy, cur, nxt, self.rnd)
            hops += 1
            seq.append(nxt)
            last, cur = cur, nxt


def routes(net, keys, src, **kw):
    """Model routes as arrays, hop_seq padded with NONE to hop_max (at least 1) columns."""
    res = [net.route(k, int(s), **kw) for k, s in zip(keys, src)]
    H = max(kw.get("hop_max", 50), 1)
    out = dict(responsible=np.array([r["responsible"] for r in res], dtype=np.uint32),
               hops=np.array([r["hops"] for r in res], dtype=np.uint16),
               status=np.array([r["status"] for r in res], dtype=np.uint8),
               one_way_hops=np.array([r["one_way_hops"] for r in res], dtype=np.uint8),
               latency_ns=np.array([r["latency_ns"] for r in res], dtype=np.int64),
               hop_seq=np.full((len(res), H), NONE, dtype=np.uint32))
    for i, r in enumerate(res):
        out["hop_seq"][i, :len(r["hop_seq"])] = r["hop_seq"]
    return out
