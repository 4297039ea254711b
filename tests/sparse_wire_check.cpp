// sparse_wire_check.cpp -- the Java-side host arithmetic of sketchml_amd/csrc/skml_sparse_wire.hpp
// against the CPU oracle's records: the parse of a field stream (every field, every truncation,
// single mutations), HuffmanEncoder's tree, the Huffman decode tables (walked by a scalar decoder
// over the oracle's words), the hash choice and calGroupEdges.  A stand-alone program: built with
// g++ by tests/test_sparse_wire_cpu.py (with -fsanitize=address,undefined), it reads the script
// that test writes and prints "ok <checks> checks".
//
//   sparse_wire_check <script> <max groups> <max rows> <LUT bits>
//
// One command a line, numbers in decimal, a stream as one hexadecimal word:
//   parse HEX G rows colRatioBits bins zero nnz cells      the head and totals of the parse
//   sk g present [cols tab_off size | nh ids | ni (value bits nbits)* | nl words*]
//   en g gstart kind1_before present [size m kind | nf words* | nd words*]
//   prefixes HEX                                           every proper prefix -> SKML_E_ARG
//   reject HEX                                             -> SKML_E_ARG
//   huff ns (value count)* ni (value bits nbits)*          HuffBuilder
//   tables ni (value bits nbits)* nw words* nc cells*      huff_tables, decoded back
//   tables_bad ni (value bits nbits)* | message            huff_tables refuses with the message
//   hashes seed rows ids*                                  pick_hashes
//   edges zero bins groups status edges*                   group_edges (edges when status is 0)
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../sketchml_amd/csrc/skml_sparse_wire.hpp"

using namespace skml;

namespace {

int g_line = 0, g_checks = 0;

[[noreturn]] void die(const std::string& what) {
    std::printf("line %d: %s\n", g_line, what.c_str());
    std::exit(1);
}
void expect(bool ok, const char* what) {
    g_checks++;
    if (!ok) die(what);
}

struct Tokens {
    std::istringstream in;
    explicit Tokens(const std::string& s) : in(s) {}
    std::string word() {
        std::string t;
        if (!(in >> t)) die("the script line ends early");
        return t;
    }
    int64_t num() { return std::strtoll(word().c_str(), nullptr, 10); }
    uint64_t u64() { return std::strtoull(word().c_str(), nullptr, 10); }
    std::vector<uint8_t> hex() {
        const std::string t = word();
        std::vector<uint8_t> b;
        if (t == "-") return b;  // the empty stream
        for (size_t i = 0; i + 1 < t.size(); i += 2) b.push_back((uint8_t)std::strtoul(t.substr(i, 2).c_str(), nullptr, 16));
        return b;
    }
    std::vector<HuffItem> items() {
        std::vector<HuffItem> v((size_t)num());
        for (auto& it : v) {
            it.value = (int32_t)num();
            it.bits = (int32_t)num();
            it.nbits = (int32_t)num();
        }
        return v;
    }
};

bool same_items(const std::vector<HuffItem>& a, const std::vector<HuffItem>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++)
        if (a[i].value != b[i].value || a[i].bits != b[i].bits || a[i].nbits != b[i].nbits) return false;
    return true;
}

// the stream's big-endian long at byte `pos`
uint64_t be64(const std::vector<uint8_t>& s, int64_t pos) {
    uint64_t v = 0;
    for (int i = 0; i < 8; i++) v = (v << 8) | s[(size_t)pos + (size_t)i];
    return v;
}
// `n` longs of the script against the stream's at `pos`
void expect_longs(Tokens& t, const std::vector<uint8_t>& s, int64_t pos, int64_t n, const char* what) {
    expect(t.num() == n, what);
    expect(pos >= 0 && (uint64_t)pos + 8 * (uint64_t)n <= s.size(), what);
    for (int64_t i = 0; i < n; i++) expect(t.u64() == be64(s, pos + 8 * i), what);
}

// bit `pos` of BitSet words (bit 0 is the lowest bit of word 0); 0 past the stored words
int bit_at(const std::vector<uint64_t>& w, int64_t pos) {
    const size_t wi = (size_t)(pos >> 6);
    return wi < w.size() ? (int)((w[wi] >> (pos & 63)) & 1u) : 0;
}

// HuffmanEncoder.decode over the tables of huff_tables: a code's first bit is its highest
std::vector<int32_t> decode(const std::vector<HuffLutCell>& lut, const std::vector<HuffNodeCell>& nodes, int lut_bits,
                            const std::vector<uint64_t>& words, size_t count) {
    std::vector<int32_t> out;
    int64_t pos = 0;
    while (out.size() < count) {
        uint32_t win = 0;
        for (int i = 0; i < lut_bits; i++) win = (win << 1) | (uint32_t)bit_at(words, pos + i);
        const HuffLutCell c = lut[win];
        if (c.nbits > 0) {
            out.push_back(c.value);
            pos += c.nbits;
            continue;
        }
        if (c.nbits != -1) die("a LUT cell that is neither a code nor a tree node");
        pos += lut_bits;
        int32_t nd = c.value;
        for (;;) {
            if (nd < 0 || (size_t)nd >= nodes.size()) die("a tree node outside the table");
            if (nodes[(size_t)nd].left < 0) break;
            nd = bit_at(words, pos++) ? nodes[(size_t)nd].right : nodes[(size_t)nd].left;
        }
        out.push_back(nodes[(size_t)nd].value);
    }
    return out;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 5) {
        std::printf("usage: sparse_wire_check <script> <max groups> <max rows> <LUT bits>\n");
        return 2;
    }
    const int max_groups = std::atoi(argv[2]), max_rows = std::atoi(argv[3]), lut_bits = std::atoi(argv[4]);
    std::ifstream script(argv[1]);
    if (!script) die("cannot read the script");
    std::vector<uint8_t> stream;  // of the last `parse`
    WireParse w;
    std::string line;
    while (std::getline(script, line)) {
        g_line++;
        if (line.empty()) continue;
        Tokens t(line);
        const std::string cmd = t.word();
        if (cmd == "parse") {
            stream = t.hex();
            const WireStatus st = parse_wire(stream.data(), stream.size(), max_groups, max_rows, &w);
            if (st) die(std::string("the parse refuses a valid stream: ") + st.msg);
            g_checks++;
            expect(w.G == t.num() && w.rows == t.num(), "head: groups, rows");
            uint64_t ratio;
            std::memcpy(&ratio, &w.col_ratio, 8);
            expect(ratio == t.u64(), "head: colRatio");
            expect(w.bin_num == t.num() && w.zero == t.num(), "head: bins, zero");
            expect(w.nnz == t.num() && w.cells == t.num(), "totals: keys, cells");
            expect(w.sketches.size() == (size_t)w.G && w.encoders.size() == (size_t)w.G, "one record per group");
        } else if (cmd == "sk") {
            const WireSketchIn& h = w.sketches.at((size_t)t.num());
            const bool present = t.num() != 0;
            expect((h.present != 0) == present, "sketch presence");
            if (!present) {
                expect(h.cols == 0 && h.size == 0 && h.nlongs == 0 && h.items.empty(), "an absent sketch holds nothing");
                continue;
            }
            expect(h.cols == t.num() && h.tab_off == t.num() && h.size == t.num(), "sketch cols, tab_off, size");
            expect((int64_t)h.hash_ids.size() == t.num(), "hash count");
            for (int32_t id : h.hash_ids) expect(id == t.num(), "hash id");
            expect(same_items(h.items, t.items()), "Huffman items");
            expect_longs(t, stream, h.pos, h.nlongs, "Huffman longs");
        } else if (cmd == "en") {
            const WireEncoderIn& e = w.encoders.at((size_t)t.num());
            expect(e.gstart == t.num() && e.kind1_before == t.num(), "gstart, kind1_before");
            if (t.num() == 0) {
                expect(e.size == 0 && e.m == 1 && e.kind == 0 && e.fn == 0 && e.dn == 0, "an absent encoder: one interval, fixed");
                continue;
            }
            expect(e.size == t.num() && e.m == t.num() && e.kind == t.num(), "encoder size, m, kind");
            expect(e.bpi == 32 / e.m && (1 << e.nf) == e.m, "bits per interval, flag bits");
            expect_longs(t, stream, e.fpos, e.fn, "flag longs");
            expect_longs(t, stream, e.dpos, e.dn, "delta longs");
        } else if (cmd == "prefixes") {
            const std::vector<uint8_t> s = t.hex();
            for (size_t len = 0; len < s.size(); len++) {
                // an exact-size copy: a read past the prefix is a read past the allocation
                std::vector<uint8_t> cut(s.begin(), s.begin() + (ptrdiff_t)len);
                WireParse p;
                const WireStatus st = parse_wire(cut.data(), cut.size(), max_groups, max_rows, &p);
                if (st.code != SKML_E_ARG || !st.msg[0]) die("a prefix of " + std::to_string(len) + " bytes is not refused");
                g_checks++;
            }
        } else if (cmd == "reject") {
            const std::vector<uint8_t> s = t.hex();
            WireParse p;
            const WireStatus st = parse_wire(s.data(), s.size(), max_groups, max_rows, &p);
            expect(st.code == SKML_E_ARG && st.msg[0], "a mutated stream is not refused");
        } else if (cmd == "huff") {
            std::vector<std::pair<int32_t, int64_t>> syms((size_t)t.num());
            for (auto& sv : syms) {
                sv.first = (int32_t)t.num();
                sv.second = t.num();
            }
            std::vector<HuffItem> got;
            HuffBuilder hb;
            expect(hb.build(syms, got), "HuffBuilder: a code longer than 32 bits");
            expect(same_items(got, t.items()), "HuffBuilder items");
        } else if (cmd == "tables") {
            const std::vector<HuffItem> items = t.items();
            std::vector<uint64_t> words((size_t)t.num());
            for (auto& x : words) x = t.u64();
            std::vector<int32_t> cells((size_t)t.num());
            for (auto& x : cells) x = (int32_t)t.num();
            std::vector<HuffLutCell> lut;
            std::vector<HuffNodeCell> nodes;
            const WireStatus st = huff_tables(items, 0, lut_bits, lut, nodes);
            if (st) die(std::string("huff_tables refuses valid items: ") + st.msg);
            expect(lut.size() == (size_t)1 << lut_bits, "one LUT row");
            expect(decode(lut, nodes, lut_bits, words, cells.size()) == cells, "the decoded table");
        } else if (cmd == "tables_bad") {
            const std::vector<HuffItem> items = t.items();
            if (t.word() != "|") die("tables_bad: the message follows a |");
            std::string msg;
            std::getline(t.in >> std::ws, msg);
            std::vector<HuffLutCell> lut;
            std::vector<HuffNodeCell> nodes;
            const WireStatus st = huff_tables(items, 0, lut_bits, lut, nodes);
            if (st.code != SKML_E_ARG || msg != st.msg) die("huff_tables: wanted \"" + msg + "\", got \"" + st.msg + "\"");
            g_checks++;
        } else if (cmd == "hashes") {
            const int64_t seed = t.num();
            const int rows = (int)t.num();
            int32_t ids[8];
            pick_hashes(seed, rows, ids);
            for (int i = 0; i < rows; i++) expect(ids[i] == t.num(), "pick_hashes");
        } else if (cmd == "edges") {
            const int32_t zero = (int32_t)t.num(), bins = (int32_t)t.num(), groups = (int32_t)t.num();
            const bool refused = t.num() != 0;
            std::vector<int32_t> e((size_t)groups, 0);
            const WireStatus st = group_edges(zero, bins, groups, e.data());
            expect((st.code != SKML_OK) == refused && (!refused || st.code == SKML_E_ARG), "group_edges status");
            if (!refused)
                for (int32_t x : e) expect(x == t.num(), "group_edges");
        } else {
            die("unknown command " + cmd);
        }
    }
    std::printf("ok %d checks\n", g_checks);
    return 0;
}
