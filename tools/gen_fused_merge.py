#!/usr/bin/env python3
"""Generator of sketchml_amd/csrc/skml_fused_merge.hpp: the merge phases of the leaf's in-register
odd-even merge sort (OddEvenNet<R>, skml_device.hpp) rewritten with gfx950's 3-input
v_min3 / v_med3 / v_max3_f32.

A p+p merge phase of Batcher's network joins two sorted runs.  Where a comparator's input is
P = min(a, b) of an earlier comparator and q its other input, min(P, q) = min3(a, b, q), and
max(P, q) = med3(a, b, q) whenever the runs' order implies q <= a or q <= b; dually for max.
If every consumer of P can be written in one op without P, P is never computed.  Whether a
replacement is valid is decided by the 0-1 principle over the (p+1)^2 inputs made of two sorted
0-1 runs: min / max / med3 commute with every monotone map, so two expressions over them that agree
on every threshold image agree on every input.

Per phase the script
  * rebuilds the comparators of OddEvenNet<R>::table() for that p (one block of 2p registers),
  * walks the values (from the inputs on, or backwards from the outputs) and drops every value whose consumers all have a
    1-op form over the value's own operands (a limit on how many comparator layers an operand may
    lie behind the value it feeds gives the points with fewer fusions and shorter live ranges),
  * orders the remaining ops with a list scheduler that keeps the number of live values low,
  * and, given --cap, takes per phase the fewest ops among those limits and walks whose peak of live
    values over the whole register file (R - 2p registers of the other blocks included) fits.
The ops then get explicit value slots: slots [0, R) are the registers on entry, a destination takes
the lowest free slot.  The header carries the op list of every block of every phase, the slot of
each sorted position at the end, and the op count and live peak of each phase.

    python tools/gen_fused_merge.py                  # write the header with the committed arguments
    python tools/gen_fused_merge.py --stdout --cap 80  # another point, to stdout

Deterministic: the same arguments give the same bytes."""
import argparse
import itertools
import os
import sys

K_MIN, K_MAX, K_MIN3, K_MED3, K_MAX3 = range(5)
DEFAULT_CAP = 0       # 0: no cap
DEFAULT_BARRIER = 16  # ops between scheduling barriers
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "sketchml_amd", "csrc",
                      "skml_fused_merge.hpp")


def batcher_table(n):
    """OddEvenNet<N>::table() (skml_device.hpp), in the same loop order, with each comparator's p."""
    out = []
    p = 1
    while p < n:
        k = p
        while k >= 1:
            j = k % p
            while j < n - k:
                for i in range(min(k, n - j - k)):
                    if (i + j) // (2 * p) == (i + j + k) // (2 * p):
                        out.append((p, i + j, i + j + k))
                j += 2 * k
            k //= 2
        p *= 2
    return out


def phase_comparators(R, p):
    """The comparators of the p+p phase inside block 0 (registers [0, 2p)), in table order."""
    return [(a, b) for q, a, b in batcher_table(R) if q == p and a < 2 * p]


def truth(kind, t):
    if kind == K_MIN:
        return t[0] & t[1]
    if kind == K_MAX:
        return t[0] | t[1]
    if kind == K_MIN3:
        return t[0] & t[1] & t[2]
    if kind == K_MAX3:
        return t[0] | t[1] | t[2]
    return (t[0] & t[1]) | (t[0] & t[2]) | (t[1] & t[2])


class Phase:
    """The value graph of one p+p merge: nodes [0, 2p) are the inputs (two sorted runs), every
    other node is one op.  expr[n] = (kind, sources); tt[n] = the node's value on each of the
    (p+1)^2 zero-one inputs, as a bit mask; layer[n] = comparator depth."""

    def __init__(self, R, p):
        self.p = p
        n_in = 2 * p
        self.n_in = n_in
        self.expr = {}
        self.tt = []
        self.layer = [0] * n_in
        for i in range(n_in):
            run, pos = divmod(i, p)
            m = 0
            for za in range(p + 1):
                for zb in range(p + 1):
                    zeros = za if run == 0 else zb
                    if pos >= zeros:
                        m |= 1 << (za * (p + 1) + zb)
            self.tt.append(m)
        cur = list(range(n_in))
        for a, b in phase_comparators(R, p):
            x, y = cur[a], cur[b]
            lay = max(self.layer[x], self.layer[y]) + 1
            for kind, pos in ((K_MIN, a), (K_MAX, b)):
                n = len(self.tt)
                self.expr[n] = (kind, (x, y))
                self.tt.append(truth(kind, (self.tt[x], self.tt[y])))
                self.layer.append(lay)
                cur[pos] = n
        self.out = cur
        self.plain_ops = len(self.expr)

    def consumers(self, x):
        return [v for v, (_, src) in self.expr.items() if x in src]

    def replacement(self, v, x, back):
        """A 1-op form of v over its other operands and x's operands, or None."""
        _, vsrc = self.expr[v]
        pool = sorted((set(vsrc) - {x}) | set(self.expr[x][1]))
        if any(self.layer[v] - self.layer[s] > back + 1 for s in pool):
            return None
        want = self.tt[v]
        for k in (2, 3):
            # later nodes first: the nearer operand keeps live ranges short
            for src in itertools.combinations(reversed(pool), k):
                for kind in ((K_MIN, K_MAX) if k == 2 else (K_MIN3, K_MED3, K_MAX3)):
                    if truth(kind, [self.tt[s] for s in src]) == want:
                        return kind, tuple(sorted(src))
        return None

    def fuse(self, back, forward):
        """forward: try the values nearest the inputs first.  That finds more fusions (its consumers
        still have two operands each when a value is tried) at longer live ranges."""
        outs = set(self.out)
        changed = True
        while changed:  # a dropped value hands its operands to its consumers: walk again
            changed = False
            for x in sorted(self.expr, reverse=not forward):
                if x in outs or x not in self.expr:
                    continue
                cons = self.consumers(x)
                rep = [self.replacement(v, x, back) for v in cons]
                if all(r is not None for r in rep):
                    for v, r in zip(cons, rep):
                        self.expr[v] = r
                    del self.expr[x]
                    changed = True

    def schedule(self):
        """Order of the ops and the peak number of live values (inputs and outputs included)."""
        best = None
        for tie in range(3):
            order, peak = self._list_schedule(tie)
            if best is None or peak < best[1]:
                best = (order, peak)
        return best

    def _list_schedule(self, tie):
        uses = {}
        for v, (_, src) in self.expr.items():
            for s in set(src):
                uses[s] = uses.get(s, 0) + 1
        for o in self.out:
            uses[o] = uses.get(o, 0) + 1  # an output never dies
        done = set(range(self.n_in))
        todo = set(self.expr)
        live = self.n_in
        peak = live
        order = []
        while todo:
            pick = None
            for v in sorted(todo):
                src = set(self.expr[v][1])
                if not src <= done:
                    continue
                kills = sum(1 for s in src if uses[s] == 1)
                # fewest new live values; then (0) table order, (1) the op whose operands are
                # nearest to dying, (2) the oldest operands
                if tie == 0:
                    t = v
                elif tie == 1:
                    t = sum(uses[s] for s in src)
                else:
                    t = min(src)
                key = (1 - kills, t, v)
                if pick is None or key < pick[0]:
                    pick = (key, v)
            v = pick[1]
            live += 1
            peak = max(peak, live)
            for s in set(self.expr[v][1]):
                uses[s] -= 1
                if uses[s] == 0:
                    live -= 1
            todo.remove(v)
            done.add(v)
            order.append(v)
        return order, peak


def build_phase(R, p, cap):
    """The fewest ops whose live peak (with the R - 2p registers outside the block) fits the cap."""
    best = None
    limits = list(range(0, 2 * p.bit_length() + 2))
    for back in reversed(limits):
        for forward in (True, False):
            ph = Phase(R, p)
            if back > 0:
                ph.fuse(back, forward)
            order, peak = ph.schedule()
            total = peak + R - 2 * p
            if cap and total > cap and back > 0:
                continue
            if best is None or (len(order), total) < (best[2], best[3]):
                best = (ph, order, len(order), total)
    return best


def generate(R, cap, barrier):
    """-> (ops, out_slot, phases, nslots): ops = [(kind, dst, a, b, c) or None for a barrier]."""
    where = list(range(R))  # slot of each register position
    free = []
    nslots = R
    ops = []
    phases = []
    count = 0
    p = 4
    while p < R:
        ph, order, nops, total = build_phase(R, p, cap)
        kinds = [0] * 5
        for v in order:
            kinds[ph.expr[v][0]] += 1
        last_use = {}
        for i, v in enumerate(order):
            for s in ph.expr[v][1]:
                last_use[s] = i
        outs = set(ph.out)
        for blk in range(R // (2 * p)):
            slot = {i: where[blk * 2 * p + i] for i in range(2 * p)}
            for i, v in enumerate(order):
                kind, src = ph.expr[v]
                ss = [slot[s] for s in src]
                # the sources that die here free their slots before the destination is chosen:
                # an op may write the slot of one of its own operands
                for s in sorted(set(src)):
                    if last_use[s] == i and s not in outs:
                        free.append(slot[s])
                if free:
                    free.sort()
                    d = free.pop(0)
                else:
                    d = nslots
                    nslots += 1
                slot[v] = d
                ops.append((kind, d, ss[0], ss[1], ss[2] if len(ss) > 2 else ss[1]))
                count += 1
                if barrier and count % barrier == 0:
                    ops.append(None)
            for i, o in enumerate(ph.out):
                where[blk * 2 * p + i] = slot[o]
        phases.append((p, R // (2 * p), ph.plain_ops, nops, total, kinds, list(where)))
        p *= 2
    return ops, where, phases, nslots


def emit(cap, barrier):
    L = []
    L.append("// Generated by tools/gen_fused_merge.py --cap %d --barrier %d; do not edit." % (cap, barrier))
    L.append("// The merge phases of sort_regs_oddeven<R> for float after the 4-sorters, with 3-input ops:")
    L.append("// X(kind, dst, a, b, c) over value slots (slots [0, R) are the registers on entry; kind 0 min,")
    L.append("// 1 max, 2 min3, 3 med3, 4 max3; c repeats b for the 2-input kinds), B() a scheduling barrier,")
    L.append("// O(position, slot) where each sorted position ends.")
    L.append("#pragma once")
    for R in (32, 64):
        ops, where, phases, nslots = generate(R, cap, barrier)
        nops = sum(1 for o in ops if o is not None)
        plain = sum(ph[1] * ph[2] for ph in phases)
        L.append("")
        L.append("// R = %d: %d ops (plain network: %d), %d slots" % (R, nops, plain, nslots))
        L.append("// phase p+p x merges: plain ops, fused ops, peak live values, min max min3 med3 max3;")
        L.append("// then the slot of each sorted position after the phase")
        for p, n, pl, fu, total, kinds, wh in phases:
            L.append("//   %2d+%-2d x %d: %3d %3d %3d  %s" % (p, p, n, pl, fu, total, " ".join(map(str, kinds))))
            L.append("//   slots after %d+%d: %s" % (p, p, " ".join(map(str, wh))))
        L.append("#define SKML_FM%d_SLOTS %d" % (R, nslots))
        L.append("#define SKML_FM%d_OPS %d" % (R, nops))
        L.append("#define SKML_FM%d_PEAK %d" % (R, max(ph[4] for ph in phases)))
        L.append("#define SKML_FM%d_LIST(X, B) \\" % R)
        for o in ops:
            L.append("    B() \\" if o is None else "    X(%d, %d, %d, %d, %d) \\" % o)
        L.append("    /* end */")
        L.append("#define SKML_FM%d_OUT(O) \\" % R)
        for i, s in enumerate(where):
            L.append("    O(%d, %d) \\" % (i, s))
        L.append("    /* end */")
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cap", type=int, default=DEFAULT_CAP, help="most live values at any point (0: no cap)")
    ap.add_argument("--barrier", type=int, default=DEFAULT_BARRIER, help="ops between scheduling barriers (0: none)")
    ap.add_argument("--stdout", action="store_true", help="print the header instead of writing it")
    ap.add_argument("--report", action="store_true", help="print op count and live peak per phase only")
    a = ap.parse_args()
    if a.report:
        for R in (32, 64):
            ops, _, phases, nslots = generate(R, a.cap, a.barrier)
            print("R=%d: %d ops, %d slots" % (R, sum(1 for o in ops if o is not None), nslots))
            for p, n, pl, fu, total, kinds, _ in phases:
                print("  %2d+%-2d x %d: plain %3d fused %3d peak live %3d  kinds %s" % (p, p, n, pl, fu, total, kinds))
        return
    text = emit(a.cap, a.barrier)
    if a.stdout:
        sys.stdout.write(text)
    else:
        with open(HEADER, "w") as f:
            f.write(text)
        for line in text.splitlines():
            if (line.startswith("//  ") and "slots after" not in line) or line.startswith("// R ="):
                print(line[3:])


if __name__ == "__main__":
    main()
