"""Host-side check of the sparse field stream's arithmetic (no GPU): sketchml_amd/csrc/skml_sparse_wire.hpp
as a stand-alone program (tests/sparse_wire_check.cpp) under the address and undefined-behaviour
sanitizers, against the CPU oracle.

The stream is assembled here from the oracle alone (tests/sparse_wire_fixtures.py), in
GroupedMinMaxSketch.writeObject order.  The program must parse it into the oracle's fields, refuse every
proper prefix and every single mutation with SKML_E_ARG, build HuffmanEncoder's items as the oracle does,
decode the oracle's Huffman words back through huff_tables (codes longer than the LUT's 12 bits
included), refuse malformed code tables with the library's messages, and agree with the oracle's hash
choice and calGroupEdges."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import sparse_wire_fixtures as FX
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (dim, bins, groups, rows, values); test_the_cases_cover_what_they_are_for holds them to the comments
CASES = [
    (12000, 256, 8, 2, "normal"),  # fixed and unary flag kinds mixed, numIntervals 4 and 8
    (12000, 16, 4, 3, "dups"),     # group 0 empty (presence byte 0), numIntervals 16: the smallest stream
    (12000, 1024, 2, 1, "normal"), # one row
    (4000, 256, 2, 2, "const"),    # bin_num 2, one empty group, a two-symbol table
]
FIB20 = [1, 1]
while len(FIB20) < 20:
    FIB20.append(FIB20[-1] + FIB20[-2])


@pytest.fixture(scope="module")
def cases():
    out = []
    for dim, bins, groups, rows, kind in CASES:
        _, _, osp = FX.compress(dim, bins, groups, rows, kind)
        stream, huff = FX.assemble(osp, rows)
        out.append((osp, rows, stream, huff))
    return out


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """Builds the program once; returns run(lines) -> the number of checks it made."""
    d = tmp_path_factory.mktemp("sparse_wire")
    exe = str(d / "sparse_wire_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "sparse_wire_check.cpp")],
                   check=True)
    with open(os.path.join(ROOT, "sketchml_amd", "csrc", "skml_sparse.h")) as f:
        text = f.read()
    limits = [re.search(r"constexpr int %s = (\d+);" % n, text).group(1)
              for n in ("kMaxGroups", "kMaxRows", "kHuffLutBits")]
    assert limits == ["64", "8", "12"]
    count = [0]

    def run(lines):
        count[0] += 1
        script = str(d / f"script{count[0]}.txt")
        with open(script, "w") as f:
            f.write("\n".join(lines) + "\n")
        out = subprocess.run([exe, script] + limits, capture_output=True, text=True, timeout=300)
        m = re.fullmatch(r"ok (\d+) checks\n", out.stdout)
        assert out.returncode == 0 and m and not out.stderr, out.stdout + out.stderr
        return int(m.group(1))

    return run


def _hex(b):
    return b.hex() if b else "-"


def _items(items):
    return [len(items)] + [int(v) for it in items for v in it]


def _words(w):
    return [len(w)] + [int(x) for x in w]


def _line(*parts):
    out = []
    for p in parts:
        out.extend(p if isinstance(p, (list, tuple)) else [p])
    return " ".join(str(x) for x in out)


def _syms(table):
    values, counts = np.unique(np.asarray(table, dtype=np.int32), return_counts=True)  # ascending signed order
    return [len(values)] + [int(x) for vc in zip(values, counts) for x in vc]


def test_the_cases_cover_what_they_are_for(cases):
    (a, _, sa, _), (b, _, sb, _), (c, _, sc, _), (d, _, _, _) = cases
    assert len(FX.data(12000, 0.25, 7)[0]) == 3012
    kinds = {x["flag_kind"] for x in a.deltas if x}
    ms = {x["num_intervals"] for x in a.deltas if x}
    assert kinds == {False, True} and {4, 8} <= ms
    assert b.tables[0] is None and 16 in {x["num_intervals"] for x in b.deltas if x}
    assert d.q.bin_num == 2 and sum(t is None for t in d.tables) == 1
    assert any(len(np.unique(t)) == 2 for t in d.tables if t is not None)
    assert 6500 < len(sa) < 8000 and 3000 < len(sb) < 4000 and 5500 < len(sc) < 7500
    assert len(sb) == min(len(s) for _, _, s, _ in cases[:3])


def test_parse_equals_the_oracle(cases, checker):
    lines = []
    for osp, rows, stream, huff in cases:
        G = osp.group_num
        sizes = [0 if d is None else d["size"] for d in osp.deltas]
        assert sizes == [int(x) for x in osp.group_size]
        cells = [0 if t is None else rows * int(osp.col_num[g]) for g, t in enumerate(osp.tables)]
        ratio = struct.unpack(">Q", struct.pack(">d", 0.3))[0]
        lines.append(_line("parse", _hex(stream), G, rows, ratio, osp.q.bin_num, osp.q.zero_idx, sum(sizes),
                           sum(cells)))
        gstart = k1 = tab = 0
        for g in range(G):
            d = osp.deltas[g]
            if d is None:
                lines.append(_line("sk", g, 0))
                lines.append(_line("en", g, gstart, k1, 0))
                continue
            lines.append(_line("sk", g, 1, int(osp.col_num[g]), tab, cells[g], rows, [int(h) for h in osp.hash_ids[g]],
                               _items(huff[g]["items"]), _words(huff[g]["words"])))
            lines.append(_line("en", g, gstart, k1, 1, d["size"], d["num_intervals"], int(d["flag_kind"]),
                               _words(d["flag_words"]), _words(d["delta_words"])))
            gstart += d["size"]
            k1 += d["size"] if d["flag_kind"] else 0
            tab += cells[g]
    assert checker(lines) > 200


def test_every_proper_prefix_is_refused(cases, checker):
    stream = cases[1][2]
    assert checker([_line("prefixes", _hex(stream))]) == len(stream)


def test_single_mutations_are_refused(cases, checker):
    muts = FX.mutations(cases[1][2])
    assert len(muts) == 15 and len({m for _, m in muts}) == 15 and all(m != cases[1][2] for _, m in muts)
    for what, m in muts:  # one run each: a failure names the mutation
        assert checker([_line("reject", _hex(m))]) == 1, what


def test_huffman_items_equal_the_oracle(cases, checker):
    tables = [t for osp, _, _, _ in cases for t in osp.tables if t is not None]
    tables.append(np.full(10, 5, dtype=np.int32))
    tables.append(np.array([2**31 - 1, -2**31, 7, 7], dtype=np.int32))  # signed order of the fill values
    fib = np.repeat(np.arange(20, dtype=np.int32), FIB20)
    assert len(fib) == 17710
    tables.append(fib)
    lines = []
    for t in tables:
        want = O.huffman_encode(t)
        lines.append(_line("huff", _syms(t), _items(want["items"])))
    assert O.huffman_encode(tables[-3])["items"] == [(5, 0, 1)]
    assert max(it[2] for it in O.huffman_encode(fib)["items"]) == 19
    assert checker(lines) == 2 * len(tables)


def test_huff_tables_decode_the_oracles_words_and_refuse_bad_codes(cases, checker):
    fib = np.repeat(np.arange(20, dtype=np.int32), FIB20)
    rng = np.random.default_rng(5)
    rng.shuffle(fib)
    a = cases[0][0]
    lines = []
    for t in (fib, next(t for t in a.tables if t is not None)):
        h = O.huffman_encode(t)
        assert np.array_equal(h["decoded"], t) and len(h["items"]) > 2
        lines.append(_line("tables", _items(h["items"]), _words(h["words"]), len(t), [int(x) for x in t]))
    assert checker(lines) == 4
    items = [tuple(int(v) for v in it) for it in O.huffman_encode(fib)["items"]]
    by_len = sorted(items, key=lambda it: it[2])
    short, long_ = by_len[1], by_len[-1]  # a LUT code (2 bits) and a tree code (19 bits)
    assert 2 <= short[2] <= 12 < long_[2]

    def swap(old, new):
        return [new if it == old else it for it in items]

    free, full = "Huffman codes are not prefix-free", "Huffman tree is not full"
    wide = "Huffman code wider than its length"
    bad = [
        (items + [(99, short[1], short[2])], free),             # a duplicated code, in the LUT ...
        (items + [(99, long_[1], long_[2])], free),             # ... and in the tree
        (items + [(99, short[1] >> 1, short[2] - 1)], free),    # a prefix of a LUT code
        (items + [(99, long_[1] >> 1, long_[2] - 1)], free),    # a prefix of a tree code, itself in the tree
        (items + [(99, long_[1] >> 9, long_[2] - 9)], free),    # ... and in the LUT
        ([it for it in items if it != short], full),            # a dropped item: a LUT range stays empty
        ([it for it in items if it != long_], full),            # ... a tree node keeps one child
        (swap(short, (short[0], short[1], 0)), "Huffman code of 0 bits"),
        (swap(short, (short[0], short[1], 32)), "Huffman code of 32 bits"),
        (swap(short, (short[0], 1 << short[2], short[2])), wide),
        (swap(long_, (long_[0], 1 << long_[2], long_[2])), wide),
    ]
    for its, msg in bad:
        assert checker([_line("tables_bad", _items(its), "|", msg)]) == 1, msg


def test_hash_choice_and_group_edges_equal_the_oracle(checker):
    lines = []
    for seed in (0, 1, -1, 2**31):
        for rows in range(1, 9):
            lines.append(_line("hashes", seed, rows, [int(h) for h in O.pick_hashes(seed, rows)]))
    for zero, bins, groups in [(0, 256, 8), (128, 256, 8), (255, 256, 8), (3, 16, 4), (9, 16, 4), (1, 2, 2),
                               (100, 1000, 7), (17, 50, 64), (5, 8, 16), (0, 3, 4)]:
        e = np.zeros(groups, dtype=np.int32)
        status = O.lib().orc_group_edges(zero, bins, groups, e.ctypes.data_as(O.i32p))
        assert (status != 0) == (groups > bins)  # the oracle refuses Java's division by zero
        lines.append(_line("edges", zero, bins, groups, status, [] if status else [int(x) for x in e]))
    assert checker(lines) > 100
