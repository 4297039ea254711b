// skml_sparse_wire.hpp -- the Java-side host arithmetic of the sparse path, shared by the sparse
// host files and by the host check tests/sparse_wire_check.cpp: java.util.Random and the hash
// choice, calGroupEdges, MinMaxSketch.compare, HuffmanEncoder's tree (the JDK priority queue), the
// field stream's writer and reader, and the Huffman decode tables.  Plain C++ (no HIP types) so
// that the host compiler builds it alone.  Nothing here sets the library's error state: a check
// that fails returns its status and message (WireStatus), and the caller reports them.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <tuple>
#include <utility>
#include <vector>

#include "../../include/skml.h"

namespace skml {

// A status of include/skml.h and, unless it is SKML_OK, the text for skml_last_error.
struct WireStatus {
    int code = SKML_OK;
    char msg[160] = {0};
    explicit operator bool() const { return code != SKML_OK; }
};
__attribute__((format(printf, 2, 3))) inline WireStatus wire_fail(int code, const char* fmt, ...) {
    WireStatus st;
    st.code = code;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(st.msg, sizeof(st.msg), fmt, ap);
    va_end(ap);
    return st;
}

// java.util.Random (JDK 8 spec): seed scramble, next(bits), nextInt(bound).
struct JavaRandom {
    uint64_t s;
    explicit JavaRandom(int64_t seed) : s(((uint64_t)seed ^ 0x5DEECE66DULL) & ((1ULL << 48) - 1)) {}
    int32_t next(int bits) {
        s = (s * 0x5DEECE66DULL + 0xBULL) & ((1ULL << 48) - 1);
        return (int32_t)(s >> (48 - bits));
    }
    int32_t next_int(int32_t bound) {
        if ((bound & -bound) == bound) return (int32_t)(((int64_t)bound * (int64_t)next(31)) >> 31);
        int32_t bits, val;
        do {
            bits = next(31);
            val = bits % bound;
        } while ((int32_t)((uint32_t)bits - (uint32_t)val + (uint32_t)(bound - 1)) < 0);  // int overflow test
        return val;
    }
};

// HashFactory.getRandomInt2IntHashes (hash/HashFactory.java:23-38) with Maths.shuffle
// (util/Maths.java:41-49): Fisher-Yates from the end over the 8 hash ids; rows take the first.
inline void pick_hashes(int64_t seed, int rows, int32_t* ids) {
    int32_t idx[8];
    for (int i = 0; i < 8; i++) idx[i] = i;
    JavaRandom r(seed);
    for (int i = 7; i > 0; i--) {
        const int32_t j = r.next_int(i + 1);
        std::swap(idx[i], idx[j]);
    }
    for (int i = 0; i < rows; i++) ids[i] = idx[i];
}

// FSketchUtils.calGroupEdges (frequency/FSketchUtils.java:9-28)
inline WireStatus group_edges(int32_t zero, int32_t bins, int32_t G, int32_t* edges) {
    if (G == 2) {
        edges[0] = zero;
        edges[1] = bins;
        return WireStatus{};
    }
    const int32_t bpg = bins / G;
    if (zero < bpg) edges[0] = zero;
    else if (bpg == 0) return wire_fail(SKML_E_ARG, "calGroupEdges: / by zero (bin_num %d < group_num %d)", bins, G);
    else if ((zero % bpg) < (bpg / 2)) edges[0] = bpg + zero % bpg;
    else edges[0] = zero % bpg;
    for (int32_t i = 1; i < G - 1; i++) edges[i] = edges[i - 1] + bpg;
    edges[G - 1] = bins;
    return WireStatus{};
}

inline int32_t log2nlz(int32_t k) { return 31 - __builtin_clz((uint32_t)k); }

// MinMaxSketch.compare with Java int wrap (MinMaxSketch.java:80-86)
inline int32_t mm_dist(int32_t v, int32_t zero) {
    const int32_t d = (int32_t)((uint32_t)v - (uint32_t)zero);
    return d < 0 ? (int32_t)(0u - (uint32_t)d) : d;
}
inline int32_t mm_cmp(int32_t a, int32_t b, int32_t zero) {
    return (int32_t)((uint32_t)mm_dist(a, zero) - (uint32_t)mm_dist(b, zero));
}

// HuffmanEncoder.encode's tree (binary/HuffmanEncoder.java:88-111): leaves fed in ascending
// value order (Int2ObjectRBTreeMap) into a JDK 8 java.util.PriorityQueue ordered by occurrence
// (binary heap, siftUp / siftDown as in the JDK), two polls per merge, the merged node offered
// back; codes from the traversal (left 0, right 1; a lone leaf gets one bit).
struct HuffItem {
    int32_t value, bits, nbits;
};
struct HuffBuilder {
    struct Node {
        int32_t value;
        int64_t occ;
        int32_t left, right;
        bool leaf;
    };
    std::vector<Node> pool;
    std::vector<int32_t> heap;
    bool less_than(int32_t a, int32_t b) const { return pool[(size_t)a].occ < pool[(size_t)b].occ; }
    void sift_up(size_t k, int32_t x) {
        while (k > 0) {
            const size_t parent = (k - 1) >> 1;
            const int32_t e = heap[parent];
            if (!less_than(x, e)) break;  // comparator(x, e) >= 0
            heap[k] = e;
            k = parent;
        }
        heap[k] = x;
    }
    void sift_down(size_t k, int32_t x) {
        const size_t n = heap.size(), half = n >> 1;
        while (k < half) {
            size_t child = 2 * k + 1;
            int32_t c = heap[child];
            const size_t right = child + 1;
            if (right < n && less_than(heap[right], c)) c = heap[child = right];  // cmp(c, right) > 0
            if (!less_than(c, x)) break;                                          // cmp(x, c) <= 0
            heap[k] = c;
            k = child;
        }
        heap[k] = x;
    }
    void offer(int32_t x) {
        heap.push_back(x);
        sift_up(heap.size() - 1, x);
    }
    int32_t poll() {
        const int32_t res = heap[0];
        const int32_t x = heap.back();
        heap.pop_back();
        if (!heap.empty()) sift_down(0, x);
        return res;
    }
    // symbols: (value, count) in ascending signed value order, counts > 0
    bool build(const std::vector<std::pair<int32_t, int64_t>>& syms, std::vector<HuffItem>& items) {
        pool.clear();
        heap.clear();
        for (const auto& sv : syms) {
            pool.push_back(Node{sv.first, sv.second, -1, -1, true});
            offer((int32_t)pool.size() - 1);
        }
        while (heap.size() > 1) {
            const int32_t x = poll(), y = poll();
            pool.push_back(Node{-1, pool[(size_t)x].occ + pool[(size_t)y].occ, x, y, false});
            offer((int32_t)pool.size() - 1);
        }
        items.clear();
        if (heap.empty()) return true;
        bool ok = true;
        // iterative traversal (left first), collecting leaves
        std::vector<std::tuple<int32_t, uint32_t, int>> st{{heap[0], 0u, 0}};
        while (!st.empty()) {
            auto [nd, bits, depth] = st.back();
            st.pop_back();
            const Node& n = pool[(size_t)nd];
            if (n.leaf) {
                items.push_back(HuffItem{n.value, (int32_t)bits, depth == 0 ? 1 : depth});
                if (depth > 32) ok = false;
            } else {
                st.emplace_back(n.right, (bits << 1) | 1u, depth + 1);
                st.emplace_back(n.left, bits << 1, depth + 1);
            }
        }
        std::sort(items.begin(), items.end(), [](const HuffItem& a, const HuffItem& b) { return a.value < b.value; });
        return ok;
    }
};

// Host layout of the field stream: small fields are appended to `small` and form pieces of the
// stream; a long array leaves a gap of 8 * nwords bytes that k_wire_longs fills on the device.
struct WireBuilder {
    std::vector<uint8_t> small;
    std::vector<int64_t> pieces;  // {small offset, stream offset, length} triples
    int64_t total = 0;
    bool open = false;
    void put(uint64_t v, int n) {
        if (!open) {
            pieces.push_back((int64_t)small.size());
            pieces.push_back(total);
            pieces.push_back(0);
            open = true;
        }
        for (int i = n - 1; i >= 0; i--) small.push_back((uint8_t)(v >> (8 * i)));
        pieces.back() += n;
        total += n;
    }
    void i32(int32_t v) { put((uint32_t)v, 4); }
    void f64(double d) {
        uint64_t x;
        std::memcpy(&x, &d, 8);
        put(x, 8);
    }
    void byte(int v) { put((uint8_t)v, 1); }
    int64_t gap(int64_t bytes) {  // returns the gap's stream offset
        open = false;
        const int64_t at = total;
        total += bytes;
        return at;
    }
};

struct BeReader {
    const uint8_t* p;
    size_t n, i = 0;
    bool bad = false;
    uint64_t u(int k) {
        if (i + (size_t)k > n) {
            bad = true;
            i = n;
            return 0;
        }
        uint64_t v = 0;
        for (int j = 0; j < k; j++) v = (v << 8) | p[i++];
        return v;
    }
    int32_t i32() { return (int32_t)(uint32_t)u(4); }
    int64_t i64() { return (int64_t)u(8); }
    double f64() {
        const uint64_t x = u(8);
        double d;
        std::memcpy(&d, &x, 8);
        return d;
    }
    int byte() { return (int)u(1); }
    // a long[] body: its byte position, the contents stay in the stream (read on the device)
    bool skip_longs(size_t count, int64_t* pos) {
        if (count > (n - i) / 8) {
            bad = true;
            i = n;
            return false;
        }
        *pos = (int64_t)i;
        i += 8 * count;
        return true;
    }
};

// What GroupedMinMaxSketch.readObject (GroupedMinMaxSketch.java:161-172) finds in a field stream
// before any of it is decoded: the small fields, and where the long arrays lie.
struct WireSketchIn {  // MinMaxSketch.readObject + HuffmanEncoder.readObject of one group
    char present = 0;  // the presence byte as read; the encoder's byte must equal it
    int32_t cols = 0;
    std::vector<int32_t> hash_ids;  // rows of them
    std::vector<HuffItem> items;
    int64_t pos = 0, nlongs = 0;  // the HuffmanEncoder's long[] in the stream
    int64_t size = 0;
    int64_t tab_off = 0;  // cells of the groups before this one
};
struct WireEncoderIn {  // DeltaAdaptiveEncoder.readObject of one group (absent: one interval, fixed)
    int32_t size = 0, m = 1, kind = 0;
    int32_t nf = 0, bpi = 0;  // floor(log2 m) flag bits, 32 / m delta bits per interval
    int64_t fpos = 0, fn = 0, dpos = 0, dn = 0;  // the flag and delta long[]s in the stream
    int64_t gstart = 0;        // keys of the groups before this one
    int32_t kind1_before = 0;  // those of them in unary-flag groups
};
struct WireParse {
    int32_t G = 0, rows = 0, bin_num = 0, zero = 0;
    double col_ratio = 0.0;
    std::vector<WireSketchIn> sketches;
    std::vector<WireEncoderIn> encoders;
    int64_t nnz = 0, cells = 0;  // all groups' keys and table cells
};

// The parse of a field stream (the one skml_sparse_serialize writes).  DeltaAdaptiveEncoder
// objects: the small fields here, the BitSets' positions in the stream.  toLongArray dropped each
// BitSet's trailing zero words, but the decode kernels index one contiguous stream per kind, so
// every group's exact bit lengths are recovered on the device afterwards.
inline WireStatus parse_wire(const uint8_t* buf, size_t len, int max_groups, int max_rows, WireParse* out) {
    BeReader r{buf, len};
    WireParse& w = *out;
    w = WireParse{};
    w.G = r.i32();
    w.rows = r.i32();
    w.col_ratio = r.f64();
    w.bin_num = r.i32();
    w.zero = r.i32();
    if (r.bad || w.G < 1 || w.G > max_groups || w.rows < 0 || w.rows > max_rows || w.bin_num < 1)
        return wire_fail(SKML_E_ARG, "malformed GroupedMinMaxSketch stream (groups %d rows %d bins %d)", w.G, w.rows,
                         w.bin_num);
    w.sketches.resize((size_t)w.G);
    w.encoders.resize((size_t)w.G);
    for (int g = 0; g < w.G; g++) {  // MinMaxSketch objects
        WireSketchIn& h = w.sketches[(size_t)g];
        h.present = (char)r.byte();
        if (!h.present) continue;
        const int32_t rows = r.i32(), cols = r.i32(), zero = r.i32();
        if (rows != w.rows || cols < 0 || zero != w.zero) return wire_fail(SKML_E_ARG, "malformed MinMaxSketch %d", g);
        h.cols = cols;
        h.hash_ids.resize((size_t)rows);
        for (int k = 0; k < rows; k++) {
            h.hash_ids[(size_t)k] = r.i32();
            (void)r.i32();  // hash size (= cols)
            (void)r.i32();  // BKDR seed (a function of the hash id)
            if (h.hash_ids[(size_t)k] < 0 || h.hash_ids[(size_t)k] > 7) return wire_fail(SKML_E_ARG, "bad hash id");
        }
        const int32_t ni = r.i32();
        if (ni < 0 || (size_t)ni * 12 > len) return wire_fail(SKML_E_ARG, "malformed Huffman items");
        h.items.resize((size_t)ni);
        for (auto& it : h.items) {
            it.value = r.i32();
            it.bits = r.i32();
            it.nbits = r.i32();
        }
        const int32_t nl = r.i32();
        if (nl < 0 || !r.skip_longs((size_t)nl, &h.pos)) return wire_fail(SKML_E_ARG, "malformed Huffman bit set");
        h.nlongs = nl;
        h.size = r.i32();
        if (h.size != (int64_t)rows * cols) return wire_fail(SKML_E_ARG, "Huffman size %lld != rows*cols", (long long)h.size);
        h.tab_off = w.cells;
        w.cells += h.size;
    }
    int64_t n = 0;
    int32_t k1 = 0;
    for (int g = 0; g < w.G; g++) {  // DeltaAdaptiveEncoder objects
        WireEncoderIn& e = w.encoders[(size_t)g];
        e.gstart = n;
        e.kind1_before = k1;
        const int pres = r.byte();
        if (pres != w.sketches[(size_t)g].present)
            return wire_fail(SKML_E_ARG, "sketch / encoder presence mismatch in group %d", g);
        if (!pres) continue;
        e.size = r.i32();
        e.m = r.i32();
        e.kind = r.byte() ? 1 : 0;
        if (e.size < 0 || (e.m != 1 && e.m != 2 && e.m != 4 && e.m != 8 && e.m != 16))
            return wire_fail(SKML_E_ARG, "malformed DeltaAdaptiveEncoder %d (numIntervals %d)", g, e.m);
        const int32_t nfl = r.i32();
        if (nfl < 0 || !r.skip_longs((size_t)nfl, &e.fpos)) return wire_fail(SKML_E_ARG, "malformed BitSet");
        const int32_t ndl = r.i32();
        if (ndl < 0 || !r.skip_longs((size_t)ndl, &e.dpos)) return wire_fail(SKML_E_ARG, "malformed BitSet");
        e.fn = nfl;
        e.dn = ndl;
        e.bpi = 32 / e.m;
        while ((1 << (e.nf + 1)) <= e.m) e.nf++;  // floor(log2 m)
        if (e.kind) k1 += e.size;
        n += e.size;
    }
    w.nnz = n;
    if (r.bad) return wire_fail(SKML_E_ARG, "truncated GroupedMinMaxSketch stream");
    return WireStatus{};
}

// Elements of the Huffman decode tables, laid out as the device's int2 / int4.
struct HuffLutCell {
    int32_t value, nbits;  // {value, length}, or {tree node, -1} for a long code's prefix
};
struct HuffNodeCell {
    int32_t left, right, value, pad;  // left < 0 for a leaf
};

// Decode tables of one group's HuffmanEncoder items (HuffmanEncoder.java:131-152 builds the same
// tree): codes of <= lut_bits bits fill their LUT ranges, longer codes end in tree nodes.
inline WireStatus huff_tables(const std::vector<HuffItem>& items, int node_base, int lut_bits,
                              std::vector<HuffLutCell>& lut, std::vector<HuffNodeCell>& nodes) {
    struct N {
        int left = -1, right = -1, value = 0;
        bool leaf = false;
    };
    const int lut_size = 1 << lut_bits;
    const size_t l0 = lut.size();
    lut.resize(l0 + (size_t)lut_size, HuffLutCell{0, 0});
    std::vector<char> set((size_t)lut_size, 0);
    std::vector<int> prefix_node((size_t)lut_size, -1);  // subtree root of a long-code prefix
    std::vector<N> t;
    for (const HuffItem& it : items) {
        if (it.nbits <= 0 || it.nbits > 31) return wire_fail(SKML_E_ARG, "Huffman code of %d bits", it.nbits);
        const uint32_t code = (uint32_t)it.bits;
        if (it.nbits <= lut_bits) {
            const uint32_t lo = code << (lut_bits - it.nbits), hi = (code + 1) << (lut_bits - it.nbits);
            if (hi > (uint32_t)lut_size) return wire_fail(SKML_E_ARG, "Huffman code wider than its length");
            for (uint32_t k = lo; k < hi; k++) {
                if (set[k]) return wire_fail(SKML_E_ARG, "Huffman codes are not prefix-free");
                set[k] = 1;
                lut[l0 + k] = HuffLutCell{it.value, it.nbits};
            }
            continue;
        }
        const uint32_t pre = code >> (it.nbits - lut_bits);
        if (pre >= (uint32_t)lut_size) return wire_fail(SKML_E_ARG, "Huffman code wider than its length");
        int node = prefix_node[pre];
        if (node < 0) {
            if (set[pre]) return wire_fail(SKML_E_ARG, "Huffman codes are not prefix-free");
            node = (int)t.size();
            t.push_back(N());
            prefix_node[pre] = node;
            set[pre] = 1;
            lut[l0 + pre] = HuffLutCell{node_base + node, -1};
        }
        for (int b = it.nbits - lut_bits - 1; b >= 0; b--) {
            if (t[(size_t)node].leaf) return wire_fail(SKML_E_ARG, "Huffman codes are not prefix-free");
            const bool one = (code >> b) & 1u;
            int child = one ? t[(size_t)node].right : t[(size_t)node].left;
            if (child < 0) {
                child = (int)t.size();
                t.push_back(N());
                if (one) t[(size_t)node].right = child;
                else t[(size_t)node].left = child;
            }
            node = child;
        }
        N& leaf = t[(size_t)node];
        if (leaf.leaf || leaf.left >= 0 || leaf.right >= 0) return wire_fail(SKML_E_ARG, "Huffman codes are not prefix-free");
        leaf.leaf = true;
        leaf.value = it.value;
    }
    for (int k = 0; k < lut_size; k++)
        if (!set[(size_t)k]) return wire_fail(SKML_E_ARG, "Huffman tree is not full");
    for (const N& nd : t) {
        if (nd.leaf) {
            nodes.push_back(HuffNodeCell{-1, -1, nd.value, 0});
        } else {
            if (nd.left < 0 || nd.right < 0) return wire_fail(SKML_E_ARG, "Huffman tree is not full");
            nodes.push_back(HuffNodeCell{node_base + nd.left, node_base + nd.right, 0, 0});
        }
    }
    return WireStatus{};
}

}  // namespace skml
