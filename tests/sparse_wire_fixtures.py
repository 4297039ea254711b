"""The field stream of GroupedMinMaxSketch.writeObject assembled from the CPU oracle alone, its field
offsets, and the single mutations a reader must refuse: shared by tests/test_sparse_wire_cpu.py (the
host parse as a stand-alone program) and tests/test_gpu_sparse_readobject.py (the same bytes through
SparsePayload.deserialize)."""
import struct

import numpy as np

from oracle import oracle as O

BKDR_SEED = {3: 31, 4: 131, 5: 267, 6: 1313, 7: 13131}  # Int2IntHash objects: the BKDR hashes carry a seed


def data(dim, density, seed, kind="normal"):
    rng = np.random.default_rng(seed)
    keys = np.nonzero(rng.random(dim) < density)[0].astype(np.int32)
    if kind == "normal":
        vals = rng.standard_normal(len(keys)).astype(np.float32)
    elif kind == "dups":
        vals = rng.integers(-3, 4, len(keys)).astype(np.float32)
    elif kind == "const":
        vals = np.full(len(keys), 0.5, dtype=np.float32)
    else:
        raise ValueError(kind)
    return keys, vals


def compress(dim, bins, groups, rows, kind):
    """The oracle's SparseVectorCompressor.compressSparse of the shared input (density 0.25, seed 7,
    colRatio 0.3, seed 3, hashSeed 4)."""
    keys, vals = data(dim, 0.25, 7, kind)
    return keys, vals, O.sparse_compress(keys, vals.astype(np.float64), bins, groups, rows, 0.3, 3, 4)


def assemble(osp, rows, col_ratio=0.3):
    """(stream, huffman): the bytes in writeObject order (the layout tests/test_gpu_sparse.py's
    _parse_sparse_stream reads), and O.huffman_encode of every present group's table."""
    out = bytearray()
    out += struct.pack(">iidii", osp.group_num, rows, col_ratio, osp.q.bin_num, osp.q.zero_idx)
    huff = [None if t is None else O.huffman_encode(t) for t in osp.tables]
    for g in range(osp.group_num):  # MinMaxSketch objects
        if osp.tables[g] is None:
            out += b"\0"
            continue
        cols = int(osp.col_num[g])
        out += struct.pack(">Biii", 1, rows, cols, osp.q.zero_idx)
        for h in osp.hash_ids[g]:
            out += struct.pack(">iii", int(h), cols, BKDR_SEED.get(int(h), 0))
        items = huff[g]["items"]
        out += struct.pack(">i", len(items))
        for it in items:
            out += struct.pack(">iii", *(int(v) for v in it))
        out += struct.pack(">i", len(huff[g]["words"])) + huff[g]["words"].astype(">u8").tobytes()
        out += struct.pack(">i", rows * cols)
    for g in range(osp.group_num):  # DeltaAdaptiveEncoder objects
        d = osp.deltas[g]
        if d is None:
            out += b"\0"
            continue
        out += struct.pack(">BiiB", 1, d["size"], d["num_intervals"], 1 if d["flag_kind"] else 0)
        for words in (d["flag_words"], d["delta_words"]):
            out += struct.pack(">i", len(words)) + words.astype(">u8").tobytes()
    return bytes(out), huff


def offsets(stream):
    """Byte offsets of the fields the mutations touch, found by walking the stream: the first present
    sketch's rows, zero, first hash id, item count, long count and size; the first encoder's presence
    byte; the first present encoder's size and numIntervals."""
    at = {}
    G, rows = struct.unpack_from(">ii", stream, 0)
    off = 24  # the head: groupNum, rowNum, colRatio, binNum, zero
    for _ in range(G):
        pres = stream[off]
        off += 1
        if not pres:
            continue
        first = "sk_rows" not in at
        if first:
            at.update(sk_rows=off, sk_zero=off + 8, hash_id=off + 12)
        off += 12 + 12 * rows
        ni = struct.unpack_from(">i", stream, off)[0]
        if first:
            at["item_count"] = off
        off += 4 + 12 * ni
        nl = struct.unpack_from(">i", stream, off)[0]
        if first:
            at["long_count"] = off
        off += 4 + 8 * nl
        if first:
            at["sk_size"] = off
        off += 4
    for g in range(G):
        if g == 0:
            at["enc_presence"] = off
        pres = stream[off]
        off += 1
        if not pres:
            continue
        if "enc_size" not in at:
            at.update(enc_size=off, enc_m=off + 4)
        off += 9
        for _ in range(2):
            off += 4 + 8 * struct.unpack_from(">i", stream, off)[0]
    assert off == len(stream)
    return at


def mutations(stream):
    """[(what, bytes)]: each a valid stream with one field changed."""
    at = offsets(stream)

    def with_i32(off, v):
        b = bytearray(stream)
        b[off:off + 4] = struct.pack(">i", v)
        return bytes(b)

    def i32(off):
        return struct.unpack_from(">i", stream, off)[0]

    flipped = bytearray(stream)
    flipped[at["enc_presence"]] ^= 1
    return [
        ("groupNum 1000", with_i32(0, 1000)),
        ("groupNum 0", with_i32(0, 0)),
        ("rows 9", with_i32(4, 9)),
        ("bin_num 0", with_i32(16, 0)),
        ("a sketch's rows differ from the head's", with_i32(at["sk_rows"], i32(at["sk_rows"]) + 1)),
        ("a sketch's zero differs from the head's", with_i32(at["sk_zero"], i32(at["sk_zero"]) + 1)),
        ("hash id 8", with_i32(at["hash_id"], 8)),
        ("hash id -1", with_i32(at["hash_id"], -1)),
        ("item count -1", with_i32(at["item_count"], -1)),
        ("item count past the stream", with_i32(at["item_count"], len(stream) // 12 + 1)),
        ("long count past the bytes left", with_i32(at["long_count"], len(stream) // 8 + 1)),
        ("size differs from rows * cols", with_i32(at["sk_size"], i32(at["sk_size"]) + 1)),
        ("encoder presence differs from the sketch's", bytes(flipped)),
        ("numIntervals 3", with_i32(at["enc_m"], 3)),
        ("encoder size -1", with_i32(at["enc_size"], -1)),
    ]
