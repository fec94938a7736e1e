"""Generates kornia_amd/csrc/km_median5_net.h: the min / max network of the register-tiled 5x5 median (csrc/km_median.hip).

    python profiles/gen_median5_network.py            # verify, then write the header
    python profiles/gen_median5_network.py --check    # verify only

A lane holds a 5-row x 8-column piece of the image, x[r][c], and owes the medians of the four 5x5 windows over columns o .. o+4
(o = 0 .. 3).  The network:

  1. sorts each of the 8 columns once (9 exchanges; a column serves up to four windows);
  2. merges the sorted column pairs (1,2), (3,4), (5,6) (Batcher's odd-even merge) and those into the sorted quads (1..4) and (3..6);
     a quad serves two windows - (0..4) = column 0 + quad (1..4), (1..5) = quad (1..4) + column 5, and so on;
  3. takes the element of rank 12 of quad + column by the split formula  min_i max(Q[i-1], C[12-i]): only Q[7..12] are needed,
     so most of the quad merge is never computed - the network is built as a graph and only what the four results depend on is
     emitted, with equal subexpressions shared and min(min(a,b),c) folded into the three-operand form.

Every node is a min or a max, so the 0-1 principle applies: the network is correct on all inputs iff it is on all 2^25 binary ones.
That is checked here exhaustively for each of the four outputs (bit sets: min = AND, max = OR, expected = "at least 13 ones").
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "kornia_amd", "csrc", "km_median5_net.h")


class Net:
    def __init__(self):
        self.nodes = []  # ("in", r, c) | ("min", a, b) | ("max", a, b)
        self.memo = {}

    def inp(self, r, c):
        return self._add(("in", r, c))

    def _add(self, key):
        if key not in self.memo:
            self.memo[key] = len(self.nodes)
            self.nodes.append(key)
        return self.memo[key]

    def op(self, kind, a, b):
        if a == b:
            return a
        return self._add((kind, min(a, b), max(a, b)))

    def cex(self, v, i, j):
        v[i], v[j] = self.op("min", v[i], v[j]), self.op("max", v[i], v[j])

    def sort5(self, v):
        v = list(v)
        for i, j in ((0, 1), (3, 4), (2, 4), (2, 3), (0, 3), (0, 2), (1, 4), (1, 3), (1, 2)):
            self.cex(v, i, j)
        return v

    def merge(self, a, b):
        """Batcher's odd-even merge of two sorted lists of any lengths."""
        if not a:
            return list(b)
        if not b:
            return list(a)
        if len(a) == 1 and len(b) == 1:
            return [self.op("min", a[0], b[0]), self.op("max", a[0], b[0])]
        v = self.merge(a[0::2], b[0::2])
        w = self.merge(a[1::2], b[1::2])
        out = [v[0]]
        vi, wi = 1, 0
        while vi < len(v) and wi < len(w):
            out += [self.op("min", w[wi], v[vi]), self.op("max", w[wi], v[vi])]
            vi += 1
            wi += 1
        out += v[vi:] + w[wi:]
        return out

    def rank(self, a, b, k):
        """element of rank k (0-based) of the union of the sorted lists a and b:  min over i of max(a[i-1], b[k-i])"""
        terms = []
        for i in range(0, k + 2):
            j = k + 1 - i  # i elements of a and j of b are the k + 1 smallest
            if i > len(a) or j > len(b):
                continue
            if i == 0:
                terms.append(b[j - 1])
            elif j == 0:
                terms.append(a[i - 1])
            else:
                terms.append(self.op("max", a[i - 1], b[j - 1]))
        r = terms[0]
        for t in terms[1:]:
            r = self.op("min", r, t)
        return r


def build():
    n = Net()
    col = [n.sort5([n.inp(r, c) for r in range(5)]) for c in range(8)]
    pair = {c: n.merge(col[c], col[c + 1]) for c in (1, 3, 5)}
    quad = {1: n.merge(pair[1], pair[3]), 3: n.merge(pair[3], pair[5])}
    outs = [n.rank(quad[1], col[0], 12), n.rank(quad[1], col[5], 12), n.rank(quad[3], col[2], 12), n.rank(quad[3], col[7], 12)]
    return n, outs


def live(n, outs):
    need = set()
    stack = list(outs)
    while stack:
        i = stack.pop()
        if i in need:
            continue
        need.add(i)
        if n.nodes[i][0] != "in":
            stack += [n.nodes[i][1], n.nodes[i][2]]
    return sorted(need)


def verify(n, outs):
    N = 1 << 25
    idx = np.arange(N, dtype=np.uint32)
    pc = np.zeros(N, dtype=np.uint8)
    for b in range(25):
        pc += ((idx >> b) & 1).astype(np.uint8)
    want = np.packbits(pc >= 13, bitorder="little")
    del pc
    for o, root in enumerate(outs):
        order = live(n, [root])
        last = {}
        for i in order:
            if n.nodes[i][0] != "in":
                last[n.nodes[i][1]] = i
                last[n.nodes[i][2]] = i
        val = {}
        for i in order:
            kind, a, b = n.nodes[i]
            if kind == "in":
                assert o <= b <= o + 4, "an output may depend on its own window only"
                val[i] = np.packbits(((idx >> (a * 5 + (b - o))) & 1).astype(np.bool_), bitorder="little")
            else:
                val[i] = (val[a] & val[b]) if kind == "min" else (val[a] | val[b])
                for s in (a, b):
                    if last.get(s) == i:
                        del val[s]
        assert np.array_equal(val[root], want), f"output {o}: the network is not a median of its 25 inputs"
        print(f"output {o}: {sum(n.nodes[i][0] != 'in' for i in order)} nodes, median on all 2^25 binary inputs", flush=True)


def emit(n, outs):
    order = live(n, outs)
    uses = {}
    for i in order:
        if n.nodes[i][0] != "in":
            uses[n.nodes[i][1]] = uses.get(n.nodes[i][1], 0) + 1
            uses[n.nodes[i][2]] = uses.get(n.nodes[i][2], 0) + 1
    for o in outs:
        uses[o] = uses.get(o, 0) + 1
    # fold  op(op(a, b), c)  into the three-operand form where the inner node has no other use
    folded = set()
    expr = {}
    for i in order:
        kind, a, b = n.nodes[i]
        if kind == "in":
            continue
        done = False
        for inner, other in ((a, b), (b, a)):
            if n.nodes[inner][0] == kind and uses.get(inner, 0) == 1 and inner not in outs and len(expr[inner]) == 3:
                expr[i] = (kind + "3", expr[inner][1], expr[inner][2], other)
                folded.add(inner)
                done = True
                break
        if not done:
            expr[i] = (kind, a, b)

    def name(i):
        kind, a, b = n.nodes[i]
        return f"x[{a}][{b}]" if kind == "in" else f"t{i}"

    lines = []
    count = 0
    for i in order:
        if n.nodes[i][0] == "in" or i in folded:
            continue
        e = expr[i]
        fn = {"min": "kmm_min", "max": "kmm_max", "min3": "km_min3", "max3": "km_max3"}[e[0]]
        lines.append(f"    const float t{i} = {fn}({', '.join(name(k) for k in e[1:])});")
        count += 1
    for o, root in enumerate(outs):
        lines.append(f"    out[{o}] = {name(root)};")
    head = f"""// kornia_amd - GENERATED by profiles/gen_median5_network.py (do not edit): the min / max network of the register-tiled 5x5 median.
// x[r][c]: 5 rows (in any order) x 8 adjacent columns; out[o] = median of the 25 values of columns o .. o + 4.
// Columns sorted once (9 exchanges each), sorted pairs (1,2) (3,4) (5,6) and quads (1..4) (3..6) shared between the windows, rank 12 of
// quad + remaining column by the split formula; only what the four results depend on is computed: {count} operations for 4 pixels.
// Verified by the generator on all 2^25 binary inputs of every output (the 0-1 principle: every node is a min or a max).
#pragma once

#define KMM_MEDIAN5_OPS {count}

__device__ __forceinline__ void kmm_median5x4(const float (&x)[5][8], float (&out)[4]) {{
"""
    return head + "\n".join(lines) + "\n}\n", count


def main():
    n, outs = build()
    verify(n, outs)
    text, count = emit(n, outs)
    print(f"{count} operations for 4 pixels ({count / 4:.1f} per pixel)")
    if "--check" not in sys.argv:
        open(OUT, "w").write(text)
        print(OUT)


if __name__ == "__main__":
    main()
