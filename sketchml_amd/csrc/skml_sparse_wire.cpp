// skml_sparse_wire.cpp -- the Java field stream of a sparse payload (include/skml.h, "Sparse
// path"): GroupedMinMaxSketch.writeObject / readObject with the HuffmanEncoder of the MinMaxSketch
// tables.  The stream's arithmetic (Huffman trees, layout, parse, decode tables) is
// skml_sparse_wire.hpp; the bytes are assembled and taken apart on the device (skml_wire.hip,
// skml_sparse_huffman.hip), and this file plans those launches.
#include <algorithm>
#include <cstddef>
#include <cstring>
#include <vector>

#include "skml_sparse_host.hpp"

using namespace skml;

// the decode tables go to the launchers as the device's vector types
static_assert(sizeof(HuffLutCell) == sizeof(int2) && offsetof(HuffLutCell, value) == offsetof(int2, x) &&
                  offsetof(HuffLutCell, nbits) == offsetof(int2, y),
              "HuffLutCell is int2");
static_assert(sizeof(HuffNodeCell) == sizeof(int4) && offsetof(HuffNodeCell, left) == offsetof(int4, x) &&
                  offsetof(HuffNodeCell, right) == offsetof(int4, y) && offsetof(HuffNodeCell, value) == offsetof(int4, z) &&
                  offsetof(HuffNodeCell, pad) == offsetof(int4, w),
              "HuffNodeCell is int4");

namespace {

// Per-group HuffmanEncoder of the MinMaxSketch tables: device histograms, host trees, device
// code stream (cached in the payload).
int build_huffman(skml_ctx* c, skml_sparse* s) {
    if (s->huff_done) return SKML_OK;
    hipStream_t st = c->stream;
    const SpGroups& G = s->g;
    const int B = G.bin_num;
    const size_t nsym = (size_t)B + 1;
    s->huff_items.assign((size_t)G.G, {});
    s->huff_bit0.assign((size_t)G.G + 1, 0);
    s->huff_bits.assign((size_t)G.G, 0);
    if (s->ncells > 0) {
        int64_t max_cells = 0;
        for (int g = 0; g < G.G; g++)
            if (G.gstart[g + 1] > G.gstart[g]) max_cells = std::max<int64_t>(max_cells, (int64_t)G.rows * G.cols[g]);
        uint32_t* hist = scratch<uint32_t>(c, kSlotDelta, (size_t)G.G * nsym);
        uint64_t* lut = scratch<uint64_t>(c, kSlotCells, (size_t)G.G * nsym);
        if (!hist || !lut) return fail(SKML_E_OOM, "huffman scratch");
        HIP_TRY(hipMemsetAsync(hist, 0, sizeof(uint32_t) * (size_t)G.G * nsym, st));
        HIP_TRY(launch_huff_hist(st, s->tables, s->g_dev, G.G, B, max_cells, hist));
        std::vector<uint32_t> hh((size_t)G.G * nsym);
        if (int e = sync_to_host(c, hh.data(), hist, sizeof(uint32_t) * hh.size())) return e;
        std::vector<uint64_t> lh((size_t)G.G * nsym, 0);
        HuffBuilder hb;
        int64_t bit = 0;
        for (int g = 0; g < G.G; g++) {
            s->huff_bit0[(size_t)g] = bit;
            if (G.gstart[g + 1] == G.gstart[g]) continue;
            std::vector<std::pair<int32_t, int64_t>> syms;
            const uint32_t* h = hh.data() + (size_t)g * nsym;
            if (G.fill < 0 && h[B]) syms.emplace_back(G.fill, h[B]);  // ascending signed order
            for (int v = 0; v < B; v++)
                if (h[v]) syms.emplace_back(v, h[v]);
            if (G.fill >= 0 && h[B]) syms.emplace_back(G.fill, h[B]);
            if (!hb.build(syms, s->huff_items[(size_t)g]))
                return fail(SKML_E_STATE, "Huffman code longer than 32 bits (group %d)", g);
            for (const HuffItem& it : s->huff_items[(size_t)g]) {
                const int sym = (it.value >= 0 && it.value < B) ? it.value : B;
                lh[(size_t)g * nsym + sym] = ((uint64_t)it.nbits << 32) | (uint32_t)it.bits;
                s->huff_bits[(size_t)g] += (int64_t)it.nbits * h[sym];
            }
            bit += s->huff_bits[(size_t)g];
        }
        s->huff_bit0[(size_t)G.G] = bit;
        HIP_TRY(hipMemcpyAsync(lut, lh.data(), sizeof(uint64_t) * lh.size(), hipMemcpyHostToDevice, st));
        const int64_t tiles = sp_tiles(s->ncells, kSpTile);
        uint64_t* ts = scratch<uint64_t>(c, kSlotTiles, (size_t)tiles + 1);
        int64_t* gbit = scratch<int64_t>(c, kSlotSmall, kMaxGroups + 1);
        if (!ts || !gbit) return fail(SKML_E_OOM, "huffman scratch");
        HIP_TRY(launch_huff_lens(st, s->tables, s->ncells, s->g_dev, B, lut, ts));
        uint64_t total = 0;
        if (int e = scan_tiles(c, ts, tiles, 1, &total)) return e;
        if ((int64_t)total != bit) return fail(SKML_E_STATE, "huffman bit count mismatch");
        s->n_huff_words = (bit + 63) / 64 + 1;
        HIP_TRY(hipMalloc(&s->huff_words, sizeof(uint64_t) * (size_t)s->n_huff_words));
        HIP_TRY(hipMemsetAsync(s->huff_words, 0, sizeof(uint64_t) * (size_t)s->n_huff_words, st));
        HIP_TRY(launch_huff_write(st, s->tables, s->ncells, s->g_dev, B, lut, ts, s->huff_words, gbit));
        HIP_TRY(hipStreamSynchronize(st));
    }
    s->huff_done = true;
    return SKML_OK;
}

// The device field stream of a payload (cached in s->wire_dev): Huffman codes of the tables,
// the trims of every long array (one small read-back), the layout on the host, then two kernels.
int build_wire(skml_ctx* c, skml_sparse* s) {
    if (int e = build_huffman(c, s)) return e;
    hipStream_t st = c->stream;
    const SpGroups& G = s->g;
    static const int32_t kBkdrSeed[8] = {0, 0, 0, 31, 131, 267, 1313, 13131};
    // the long arrays in stream order: every present sketch's Huffman words, then every present
    // encoder's flag and delta words
    std::vector<WireSec> secs;
    std::vector<int> present;
    for (int g = 0; g < G.G; g++)
        if (G.gstart[g + 1] > G.gstart[g]) present.push_back(g);
    for (int g : present) secs.push_back(WireSec{0, s->huff_bit0[(size_t)g], s->huff_bits[(size_t)g], 0, 2, 0});
    for (int g : present) {
        secs.push_back(WireSec{0, G.fb[g], G.fb[g + 1] - G.fb[g], 0, 0, 0});
        secs.push_back(WireSec{0, G.db[g], G.db[g + 1] - G.db[g], 0, 1, 0});
    }
    const int nsec = (int)secs.size();
    std::vector<int64_t> wpre((size_t)nsec + 1, 0);
    for (int k = 0; k < nsec; k++) wpre[(size_t)k + 1] = wpre[(size_t)k] + (secs[(size_t)k].nbits + 63) / 64;
    const WireSrc src{s->flag_words, s->delta_words, s->huff_words};
    // section tables and the trims in one scratch block: secs | wpre | nz | npre
    const size_t o_pre = align_up(sizeof(WireSec) * (size_t)std::max(nsec, 1), 256);
    const size_t o_nz = o_pre + align_up(sizeof(int64_t) * ((size_t)nsec + 1), 256);
    const size_t o_npre = o_nz + align_up(sizeof(uint64_t) * (size_t)std::max(nsec, 1), 256);
    const size_t meta_bytes = o_npre + sizeof(int64_t) * ((size_t)nsec + 1);
    uint8_t* meta = scratch<uint8_t>(c, kSlotWireMeta, meta_bytes);
    if (!meta) return fail(SKML_E_OOM, "wire scratch");
    WireSec* d_secs = reinterpret_cast<WireSec*>(meta);
    int64_t* d_pre = reinterpret_cast<int64_t*>(meta + o_pre);
    uint64_t* d_nz = reinterpret_cast<uint64_t*>(meta + o_nz);
    int64_t* d_npre = reinterpret_cast<int64_t*>(meta + o_npre);
    std::vector<uint64_t> nz((size_t)nsec, 0);
    if (nsec > 0) {
        HIP_TRY(hipMemcpyAsync(d_secs, secs.data(), sizeof(WireSec) * (size_t)nsec, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_pre, wpre.data(), sizeof(int64_t) * wpre.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(d_nz, 0, sizeof(uint64_t) * (size_t)nsec, st));
        HIP_TRY(launch_wire_lastnz(st, src, d_secs, nsec, d_nz));
        if (int e = sync_to_host(c, nz.data(), d_nz, sizeof(uint64_t) * (size_t)nsec)) return e;
    }
    // the layout (GroupedMinMaxSketch.writeObject field order, see skml_sparse_serialize)
    WireBuilder w;
    w.i32(G.G);
    w.i32(G.rows);
    w.f64(s->params.col_ratio);
    w.i32(G.bin_num);
    w.i32(G.zero);
    int k = 0;
    for (int g = 0; g < G.G; g++) {  // sketches
        const bool pres = G.gstart[g + 1] > G.gstart[g];
        w.byte(pres ? 1 : 0);
        if (!pres) continue;
        w.i32(G.rows);
        w.i32(G.cols[g]);
        w.i32(G.zero);
        for (int r = 0; r < G.rows; r++) {
            w.i32(G.hash_ids[g][r]);
            w.i32(G.cols[g]);
            w.i32(kBkdrSeed[G.hash_ids[g][r] & 7]);
        }
        const auto& items = s->huff_items[(size_t)g];
        w.i32((int32_t)items.size());
        for (const HuffItem& it : items) {
            w.i32(it.value);
            w.i32(it.bits);
            w.i32(it.nbits);
        }
        WireSec& sc = secs[(size_t)k++];
        sc.nwords = (int64_t)nz[(size_t)(&sc - secs.data())];
        w.i32((int32_t)sc.nwords);
        sc.dst = w.gap(8 * sc.nwords);
        w.i32(G.rows * G.cols[g]);
    }
    for (int g = 0; g < G.G; g++) {  // encoders
        const bool pres = G.gstart[g + 1] > G.gstart[g];
        w.byte(pres ? 1 : 0);
        if (!pres) continue;
        w.i32((int32_t)(G.gstart[g + 1] - G.gstart[g]));
        w.i32(G.m[g]);
        w.byte(G.kind[g] ? 1 : 0);
        for (int t = 0; t < 2; t++) {
            WireSec& sc = secs[(size_t)k];
            sc.nwords = (int64_t)nz[(size_t)k];
            k++;
            w.i32((int32_t)sc.nwords);
            sc.dst = w.gap(8 * sc.nwords);
        }
    }
    std::vector<int64_t> npre((size_t)nsec + 1, 0);
    for (int q = 0; q < nsec; q++) npre[(size_t)q + 1] = npre[(size_t)q] + secs[(size_t)q].nwords;
    // the stream: the small fields' pieces, then the long arrays
    DevTemp wire(st);  // freed on every failing return below, after the stream has drained
    HIP_TRY(hipMalloc(&wire.p, (size_t)std::max<int64_t>(w.total, 1)));
    const int npieces = (int)(w.pieces.size() / 3);
    const size_t o_pcs = align_up(w.small.size(), 256);
    uint8_t* sm = scratch<uint8_t>(c, kSlotSmall, o_pcs + sizeof(int64_t) * w.pieces.size() + 8);
    if (!sm) return fail(SKML_E_OOM, "wire scratch");
    if (!w.small.empty()) SP_TRY(hipMemcpyAsync(sm, w.small.data(), w.small.size(), hipMemcpyHostToDevice, st));
    if (npieces > 0)
        SP_TRY(hipMemcpyAsync(sm + o_pcs, w.pieces.data(), sizeof(int64_t) * w.pieces.size(), hipMemcpyHostToDevice, st));
    if (nsec > 0) {
        SP_TRY(hipMemcpyAsync(d_secs, secs.data(), sizeof(WireSec) * (size_t)nsec, hipMemcpyHostToDevice, st));
        SP_TRY(hipMemcpyAsync(d_npre, npre.data(), sizeof(int64_t) * npre.size(), hipMemcpyHostToDevice, st));
    }
    SP_TRY(launch_wire_pieces(st, sm, reinterpret_cast<const int64_t*>(sm + o_pcs), npieces, static_cast<uint8_t*>(wire.p)));
    if (nsec > 0) SP_TRY(launch_wire_longs(st, src, d_secs, d_npre, nsec, npre.back(), static_cast<uint8_t*>(wire.p)));
    SP_TRY(hipStreamSynchronize(st));  // the host vectors above are the copies' sources
    s->wire_dev = wire.release();
    s->wire_bytes = (size_t)w.total;
    return SKML_OK;
}

// ---- readObject, stage 2: every group's exact flag and delta bit lengths ----
// toLongArray dropped each BitSet's trailing zero words, so the lengths are recovered from the
// contents: fixed-width flags take size * nf bits, and the deltas bpi * (size + the flags' field
// sum); unary flags end at the size-th zero, and the deltas take bpi * (that length - size).  The
// field sums and zero selects run on the device (one read-back); the stream offsets G.fb / G.db
// and the payload's totals follow on the host.
int read_flag_lengths(skml_ctx* c, const WireParse& w, const uint8_t* dstream, skml_sparse* s) {
    hipStream_t st = c->stream;
    SpGroups& G = s->g;
    std::vector<RdFlagSec> fx, un;
    std::vector<int> fx_g, un_g;
    for (int g = 0; g < G.G; g++) {
        if (!w.sketches[(size_t)g].present) continue;
        const WireEncoderIn& e = w.encoders[(size_t)g];
        RdFlagSec sc{e.fpos, e.fn, (int64_t)e.size * e.nf, e.size, e.nf, 0};
        if (G.kind[g]) {
            un.push_back(sc);
            un_g.push_back(g);
        } else if (e.nf > 0) {
            fx.push_back(sc);
            fx_g.push_back(g);
        }
    }
    std::vector<int64_t> fx_pre(fx.size() + 1, 0), un_pre(un.size() + 1, 0);
    for (size_t q = 0; q < fx.size(); q++) fx_pre[q + 1] = fx_pre[q] + (fx[q].nbits + 63) / 64;
    for (size_t q = 0; q < un.size(); q++) un_pre[q + 1] = un_pre[q] + (un[q].nstored + kRdTileWords - 1) / kRdTileWords;
    const size_t nfx = fx.size(), nun = un.size();
    const size_t o_un = align_up(sizeof(RdFlagSec) * std::max<size_t>(nfx, 1), 256);
    const size_t o_fxp = o_un + align_up(sizeof(RdFlagSec) * std::max<size_t>(nun, 1), 256);
    const size_t o_unp = o_fxp + align_up(sizeof(int64_t) * (nfx + 1), 256);
    const size_t o_res = o_unp + align_up(sizeof(int64_t) * (nun + 1), 256);  // sums[nfx] | flen[nun]
    const size_t o_tz = o_res + align_up(sizeof(int64_t) * (nfx + nun + 1), 256);
    uint8_t* meta = scratch<uint8_t>(c, kSlotWireMeta, o_tz + sizeof(uint32_t) * (size_t)std::max<int64_t>(un_pre.back(), 1));
    if (!meta) return fail(SKML_E_OOM, "readObject scratch");
    int64_t* d_res = reinterpret_cast<int64_t*>(meta + o_res);
    std::vector<int64_t> res(nfx + nun, 0);
    if (nfx + nun > 0) {
        if (nfx) HIP_TRY(hipMemcpyAsync(meta, fx.data(), sizeof(RdFlagSec) * nfx, hipMemcpyHostToDevice, st));
        if (nun) HIP_TRY(hipMemcpyAsync(meta + o_un, un.data(), sizeof(RdFlagSec) * nun, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(meta + o_fxp, fx_pre.data(), sizeof(int64_t) * fx_pre.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(meta + o_unp, un_pre.data(), sizeof(int64_t) * un_pre.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(d_res, 0, sizeof(int64_t) * (nfx + nun), st));
        HIP_TRY(launch_rd_fixed_sum(st, dstream, reinterpret_cast<const RdFlagSec*>(meta),
                                    reinterpret_cast<const int64_t*>(meta + o_fxp), (int)nfx, fx_pre.back(),
                                    reinterpret_cast<uint64_t*>(d_res)));
        HIP_TRY(launch_rd_unary(st, dstream, reinterpret_cast<const RdFlagSec*>(meta + o_un),
                                reinterpret_cast<const int64_t*>(meta + o_unp), (int)nun, un_pre.back(),
                                reinterpret_cast<uint32_t*>(meta + o_tz), d_res + nfx));
        if (int e = sync_to_host(c, res.data(), d_res, sizeof(int64_t) * res.size())) return e;
    }
    std::vector<int64_t> flen((size_t)G.G, 0), dlen((size_t)G.G, 0);
    for (size_t q = 0; q < nfx; q++) {
        const WireEncoderIn& e = w.encoders[(size_t)fx_g[q]];
        flen[(size_t)fx_g[q]] = fx[q].nbits;
        dlen[(size_t)fx_g[q]] = (int64_t)e.bpi * ((int64_t)e.size + res[q]);
    }
    for (size_t q = 0; q < nun; q++) {
        const int g = un_g[q];
        const WireEncoderIn& e = w.encoders[(size_t)g];
        flen[(size_t)g] = res[nfx + q];
        if (flen[(size_t)g] < e.size) return fail(SKML_E_ARG, "unary flags of group %d do not end", g);
        dlen[(size_t)g] = (int64_t)e.bpi * (flen[(size_t)g] - e.size);
    }
    int64_t fbits = 0, dbits = 0;
    for (int g = 0; g < G.G; g++) {
        G.fb[g] = fbits;
        G.db[g] = dbits;
        if (!w.sketches[(size_t)g].present) continue;
        const WireEncoderIn& e = w.encoders[(size_t)g];
        if (!G.kind[g] && e.nf == 0) {  // one interval per key: no flag bits, 32-bit deltas
            flen[(size_t)g] = 0;
            dlen[(size_t)g] = (int64_t)e.bpi * e.size;
        }
        if (e.fn > (flen[(size_t)g] + 63) / 64 || e.dn > (dlen[(size_t)g] + 63) / 64)
            return fail(SKML_E_ARG, "DeltaAdaptiveEncoder %d holds bits past its stream", g);
        fbits += flen[(size_t)g];
        dbits += dlen[(size_t)g];
    }
    G.fb[G.G] = fbits;
    G.db[G.G] = dbits;
    s->flag_bits = fbits;
    s->delta_bits = dbits;
    s->n_flag_words = (fbits + 63) / 64 + 1;
    s->n_delta_words = (dbits + 63) / 64 + 1;
    return SKML_OK;
}

// ---- readObject, stage 3: the DeltaAdaptive BitSets into the payload's two contiguous streams,
// then the group table ----
int copy_streams(skml_ctx* c, const WireParse& w, const uint8_t* dstream, skml_sparse* s) {
    hipStream_t st = c->stream;
    SpGroups& G = s->g;
    std::vector<RdBitSec> fsec((size_t)G.G), dsec((size_t)G.G);
    for (int g = 0; g < G.G; g++) {
        fsec[(size_t)g] = RdBitSec{w.encoders[(size_t)g].fpos, w.encoders[(size_t)g].fn};
        dsec[(size_t)g] = RdBitSec{w.encoders[(size_t)g].dpos, w.encoders[(size_t)g].dn};
    }
    const size_t o_d = align_up(sizeof(RdBitSec) * (size_t)G.G, 256);
    const size_t o_fo = 2 * o_d, o_do = o_fo + align_up(sizeof(int64_t) * (size_t)(G.G + 1), 256);
    uint8_t* m2 = scratch<uint8_t>(c, kSlotStatus, o_do + sizeof(int64_t) * (size_t)(G.G + 1));
    if (!m2) return fail(SKML_E_OOM, "readObject scratch");
    HIP_TRY(hipMemcpyAsync(m2, fsec.data(), sizeof(RdBitSec) * fsec.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(m2 + o_d, dsec.data(), sizeof(RdBitSec) * dsec.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(m2 + o_fo, G.fb, sizeof(int64_t) * (size_t)(G.G + 1), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(m2 + o_do, G.db, sizeof(int64_t) * (size_t)(G.G + 1), hipMemcpyHostToDevice, st));
    HIP_TRY(launch_rd_stream(st, dstream, reinterpret_cast<const RdBitSec*>(m2),
                             reinterpret_cast<const int64_t*>(m2 + o_fo), G.G, s->n_flag_words, s->flag_words));
    HIP_TRY(launch_rd_stream(st, dstream, reinterpret_cast<const RdBitSec*>(m2 + o_d),
                             reinterpret_cast<const int64_t*>(m2 + o_do), G.G, s->n_delta_words, s->delta_words));
    HIP_TRY(hipStreamSynchronize(st));  // the host tables above are the copies' sources
    return upload_groups(c, s);
}

// ---- readObject, stage 4: HuffmanEncoder.decode of every group's table (HuffmanEncoder.java:
// 193-207) by the speculative parallel decoder: every 2048-bit segment decodes from its nominal
// start, then the starts are moved until every segment begins where its predecessor ends ----
int decode_tables(skml_ctx* c, const WireParse& w, const uint8_t* dstream, skml_sparse* s) {
    hipStream_t st = c->stream;
    const SpGroups& G = s->g;
    std::vector<HuffDecGroup> dg;
    std::vector<HuffSeg> segs;
    std::vector<int64_t> starts;
    std::vector<HuffLutCell> lut;
    std::vector<HuffNodeCell> nodes;
    std::vector<int64_t> wpos, wpre{0};  // the groups' Huffman long[]s: stream positions, word prefix
    for (int g = 0; g < G.G; g++) {
        const WireSketchIn& h = w.sketches[(size_t)g];
        if (!h.present || h.size == 0) continue;
        if (h.items.empty()) return fail(SKML_E_ARG, "Huffman items missing in group %d", g);
        if (h.items.size() == 1) {  // a one-symbol tree: zero-bit codes
            HIP_TRY(launch_fill_i32(st, s->tables + G.tab_off[g], h.size, h.items[0].value));
            continue;
        }
        HuffDecGroup d;
        d.word0 = wpre.back();
        d.nwords = h.nlongs;
        d.tab_off = G.tab_off[g];
        d.size = h.size;
        d.lut_row = (int32_t)(lut.size() / kHuffLutSize);
        d.seg0 = (int32_t)segs.size();
        std::vector<HuffNodeCell> gn;
        if (int e = report(huff_tables(h.items, (int)nodes.size(), kHuffLutBits, lut, gn))) return e;
        nodes.insert(nodes.end(), gn.begin(), gn.end());
        wpos.push_back(h.pos);
        wpre.push_back(wpre.back() + h.nlongs);
        const int64_t bits = d.nwords * 64;
        const int64_t nseg = std::max<int64_t>(1, (bits + kHuffSeg - 1) / kHuffSeg);
        for (int64_t k = 0; k < nseg; k++) {
            HuffSeg sg;
            sg.g = (int32_t)dg.size();
            sg.first = k == 0;
            sg.last = k == nseg - 1;
            sg.lim = (k + 1) * kHuffSeg;
            segs.push_back(sg);
            starts.push_back(k * kHuffSeg);
        }
        dg.push_back(d);
    }
    const int ns = (int)segs.size();
    if (ns == 0) return SKML_OK;
    if (nodes.empty()) nodes.push_back(HuffNodeCell{-1, -1, 0, 0});
    const size_t nwords_all = (size_t)wpre.back() + 1;  // + a zero word read past the last one
    // one device block: groups, segments, starts, 2 x ends, counts (+1 for the scan total),
    // flags, LUT, nodes, words
    const size_t b_grp = align_up(sizeof(HuffDecGroup) * dg.size(), 256);
    const size_t b_seg = align_up(sizeof(HuffSeg) * (size_t)ns, 256);
    const size_t b_i64 = align_up(sizeof(int64_t) * (size_t)ns, 256);
    const size_t b_cnt = align_up(sizeof(uint64_t) * (size_t)(ns + 1), 256);
    const size_t b_lut = align_up(sizeof(int2) * lut.size(), 256);
    const size_t b_nod = align_up(sizeof(int4) * nodes.size(), 256);
    const size_t b_wrd = align_up(sizeof(uint64_t) * nwords_all, 256);
    const size_t b_wp = align_up(sizeof(int64_t) * (wpos.size() + wpre.size()), 256);
    const size_t total = b_grp + b_seg + 3 * b_i64 + b_cnt + 256 + b_lut + b_nod + b_wrd + b_wp;
    DevTemp blk(st);  // freed on every return below, after the stream has drained
    HIP_TRY(hipMalloc(&blk.p, total));
    char* q = static_cast<char*>(blk.p);
    auto* d_grp = (HuffDecGroup*)q; q += b_grp;
    auto* d_seg = (HuffSeg*)q; q += b_seg;
    auto* d_start = (int64_t*)q; q += b_i64;
    auto* d_ea = (int64_t*)q; q += b_i64;
    auto* d_eb = (int64_t*)q; q += b_i64;
    auto* d_cnt = (uint64_t*)q; q += b_cnt;
    auto* d_flag = (unsigned*)q; q += 256;
    auto* d_lut = (int2*)q; q += b_lut;
    auto* d_nod = (int4*)q; q += b_nod;
    auto* d_wrd = (uint64_t*)q; q += b_wrd;
    auto* d_wp = (int64_t*)q;
    HIP_TRY(hipMemcpyAsync(d_wp, wpos.data(), sizeof(int64_t) * wpos.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_wp + wpos.size(), wpre.data(), sizeof(int64_t) * wpre.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d_wrd + wpre.back(), 0, sizeof(uint64_t), st));
    HIP_TRY(launch_rd_words(st, dstream, d_wp, d_wp + wpos.size(), (int)wpos.size(), wpre.back(), d_wrd));
    HIP_TRY(hipMemcpyAsync(d_grp, dg.data(), sizeof(HuffDecGroup) * dg.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_seg, segs.data(), sizeof(HuffSeg) * segs.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_start, starts.data(), sizeof(int64_t) * starts.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_lut, lut.data(), sizeof(int2) * lut.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_nod, nodes.data(), sizeof(int4) * nodes.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d_cnt, 0, b_cnt, st));
    HIP_TRY(launch_huff_spec(st, ns, d_seg, d_grp, d_wrd, d_lut, d_nod, d_start, d_ea, d_cnt));
    // resynchronise until every segment starts where its predecessor ends
    for (int round = 0;; round++) {
        if (round > ns + 1) return fail(SKML_E_ARG, "Huffman stream does not resynchronise");
        HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(unsigned), st));
        HIP_TRY(launch_huff_sync(st, ns, d_seg, d_grp, d_wrd, d_lut, d_nod, d_start, d_ea, d_eb, d_cnt, d_flag));
        unsigned changed = 0;
        if (int e = sync_to_host(c, &changed, d_flag, sizeof(unsigned))) return e;
        std::swap(d_ea, d_eb);
        if (!changed) break;
    }
    HIP_TRY(launch_scan_cols(st, d_cnt, ns, 1));  // exclusive scan: symbol offsets
    HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(unsigned), st));
    HIP_TRY(launch_huff_decode_write(st, ns, d_seg, d_grp, d_wrd, d_lut, d_nod, d_start, d_cnt, s->tables, d_flag));
    unsigned err = 0;
    if (int e = sync_to_host(c, &err, d_flag, sizeof(unsigned))) return e;
    if (err) return fail(SKML_E_ARG, "Huffman stream holds a different number of symbols than size");
    return SKML_OK;
}

}  // namespace

extern "C" {

// GroupedMinMaxSketch.writeObject field order (GroupedMinMaxSketch.java:148-158) with
// MinMaxSketch.writeObject (MinMaxSketch.java:88-97), HuffmanEncoder.writeObject
// (HuffmanEncoder.java:168-190) and DeltaAdaptiveEncoder.writeObject (:148-170); big-endian
// DataOutput primitives; a 1-byte presence flag stands where Java writes a null object, and each
// Int2IntHash object is (int HashFactory index, int size, int BKDR seed or 0).  Assembled on the
// device (skml_wire.hip) and copied out once.
int skml_sparse_serialize(skml_ctx* c, const skml_sparse* cs, uint8_t* buf, size_t cap, size_t* written) {
    if (!c || !cs) return fail(SKML_E_ARG, "bad serialise arguments");
    HIP_TRY(hipSetDevice(c->device));
    skml_sparse* s = const_cast<skml_sparse*>(cs);  // the Huffman streams and the wire are lazily built caches
    if (!s->wire_dev)
        if (int e = build_wire(c, s)) return e;
    if (written) *written = s->wire_bytes;
    if (!buf) return SKML_OK;
    if (cap < s->wire_bytes) return fail(SKML_E_ARG, "buffer capacity %zu < %zu", cap, s->wire_bytes);
    HIP_TRY(hipMemcpyAsync(buf, s->wire_dev, s->wire_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SKML_OK;
}

// GroupedMinMaxSketch.readObject (GroupedMinMaxSketch.java:161-172), MinMaxSketch.readObject
// (MinMaxSketch.java:99-108), HuffmanEncoder.readObject + decode (HuffmanEncoder.java:127-166,
// 193-207) and DeltaAdaptiveEncoder.readObject (DeltaAdaptiveEncoder.java:172-188): the stream
// skml_sparse_serialize writes, back into a device payload that restore/decode accept.  Four
// stages: the parse (parse_wire, host only), the flag lengths, the stream copy, the table decode.
int skml_sparse_deserialize(skml_ctx* c, const uint8_t* buf, size_t len, const double* qvalues, int32_t nvalues,
                            skml_sparse** out) {
    if (!c || !buf || !out || nvalues < 0 || (nvalues > 0 && !qvalues))
        return fail(SKML_E_ARG, "bad deserialise arguments");
    *out = nullptr;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    WireParse w;
    if (int e = report(parse_wire(buf, len, kMaxGroups, kMaxRows, &w))) return e;
    skml_sparse* s = new skml_sparse();
    PayloadOwner own(s, st);
    s->device = c->device;
    SpGroups& G = s->g;
    G.G = w.G;
    G.rows = w.rows;
    G.bin_num = w.bin_num;
    G.zero = w.zero;
    G.fill = mm_cmp(INT32_MIN, INT32_MAX, G.zero) <= 0 ? INT32_MIN : INT32_MAX;
    for (int g = 0; g < G.G; g++) {
        const WireSketchIn& h = w.sketches[(size_t)g];
        const WireEncoderIn& e = w.encoders[(size_t)g];
        G.cols[g] = h.cols;
        for (size_t k = 0; k < h.hash_ids.size(); k++) G.hash_ids[g][k] = h.hash_ids[k];
        G.tab_off[g] = h.tab_off;
        G.gstart[g] = e.gstart;
        G.kind1_before[g] = e.kind1_before;
        G.m[g] = e.m;
        G.kind[g] = e.kind;
    }
    G.gstart[G.G] = w.nnz;
    s->params.col_ratio = w.col_ratio;
    s->params.group_num = G.G;
    s->params.row_num = G.rows;
    s->params.bin_num = G.bin_num;
    // the stream on the device, once
    // 16 bytes of slack: be64_at reads the aligned word after an unaligned long
    uint8_t* dstream = scratch<uint8_t>(c, kSlotWire, std::max<size_t>(len + 16, 64));
    if (!dstream) return fail(SKML_E_OOM, "device copy of the stream");
    HIP_TRY(hipMemcpyAsync(dstream, buf, len, hipMemcpyHostToDevice, st));
    if (int e = read_flag_lengths(c, w, dstream, s)) return e;
    s->nnz = w.nnz;
    s->ncells = w.cells;
    G.ncells = w.cells;  // the group table's total as the encoder's plan leaves it (exported blobs check it)
    s->hdr.magic = SKML_DENSE_MAGIC;
    s->hdr.status = SKML_OK;
    s->hdr.n = w.nnz;
    s->hdr.bin_num = G.bin_num;
    s->hdr.zero_idx = G.zero;
    s->hdr.req_bins = G.bin_num;
    s->hdr.code_bits = code_bits_for(G.bin_num);
    s->qvalues.assign(qvalues, qvalues + nvalues);
    // device: group table, the contiguous DeltaAdaptive streams, MinMax tables
    if (hipMalloc(&s->g_dev, sizeof(SpGroups)) != hipSuccess ||
        hipMalloc(&s->flag_words, sizeof(uint64_t) * (size_t)s->n_flag_words) != hipSuccess ||
        hipMalloc(&s->delta_words, sizeof(uint64_t) * (size_t)s->n_delta_words) != hipSuccess ||
        hipMalloc(&s->tables, sizeof(int32_t) * (size_t)std::max<int64_t>(w.cells, 1)) != hipSuccess)
        return fail(SKML_E_OOM, "deserialised payload");
    if (int e = copy_streams(c, w, dstream, s)) return e;
    if (int e = decode_tables(c, w, dstream, s)) return e;
    HIP_TRY(hipStreamSynchronize(st));
    own.release(out);
    return SKML_OK;
}

}  // extern "C"
