// skml_internal.h -- constants and launch interfaces shared by the host files (*.cpp) and the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/skml.h"

namespace skml {

// The kernel form selected by skml_debug_form (SKML_FORM_*): 0 = the library's own choice.
int form(int id);

// Storage type of a dense input or output buffer.  The sketch sorts and merges float whatever the
// storage: bf16 and fp16 widen to float exactly, so a 16-bit encode is the fp32 encode of the
// widened buffer, byte for byte.
enum XType : int { kXF32 = 0, kXBF16 = 1, kXF16 = 2 };
struct bf16_t { uint16_t bits; };
struct f16_t { uint16_t bits; };

constexpr uint64_t kLcgMult = 0x5DEECE66DULL;  // java.util.Random
constexpr uint64_t kLcgAdd = 0xBULL;
constexpr uint64_t kLcgMask = (1ULL << 48) - 1;

constexpr int kK = 128;                 // HeapQuantileSketch.DEFAULT_K (HeapQuantileSketch.java:13)
constexpr int kChunk = 2 * kK;          // base buffer size: 256 values per leaf
constexpr int kLeafWaves = 8;           // waves per leaf workgroup
constexpr int kChunksPerWave = 8;       // 32 keys per lane, 8 lanes per chunk
constexpr int kLeafChunks = kLeafWaves * kChunksPerWave;  // 64 chunks -> one level-6 node
constexpr int kLeafTopLevel = 6;
constexpr int kMergeGroupLog = 6;       // upper merge: 64 nodes per workgroup
constexpr int kMaxLevels = 24;     // n < 2^31 -> fewer than 2^23 chunks
constexpr int kHeaderBytes = 64;
// Quantize bucket LUT: the top kLutBits of a value's total-order key select a bucket whose entry
// is the number of splits below the bucket; at most `cmax` splits fall inside any bucket.
constexpr int kLutBits = 14;
constexpr int kLutSize = 1 << kLutBits;
constexpr int kLutMaxNeed = 15;    // <= 4 bisection steps after the lookup; else Eytzinger
constexpr int kLutMaxSplits = 4096;  // split table must fit the quantize kernel's LDS
constexpr int kLutPad = 16;          // NaN padding after the last split (2^4 bisection reach)
struct QuantLut {
    uint16_t base[kLutSize];
    int32_t cmax;  // -1: LUT unusable (too many splits per bucket); kLutJavaMode: see below
    int32_t pad[15];
};
// cmax value asking the quantize pass for Quantizer.indexOf literally (a degenerate uniform split
// table: NaN or descending splits, on which indexOf is not an upper bound).
constexpr int32_t kLutJavaMode = -2;

// fp64 leaf partials (one per 64-chunk tile): min / max total-order key, flags (bit0 NaN).
struct LeafPartial64 {
    uint64_t min_key;
    uint64_t max_key;
    uint32_t flags;
    uint32_t pad;
};
// Uniform quantizer partials (one per workgroup): IEEE min / max of the non-NaN values and the
// index of the first zero.
struct UniPartial {
    double mn, mx;
    int64_t zidx;
    int64_t pad;
};
constexpr int kUniMaxParts = 1024;

// Per leaf workgroup partial results: min key, max key, flags (bit0 NaN, bit1 -0, bit2 +0).
struct LeafPartial {
    uint32_t min_key;
    uint32_t max_key;
    uint32_t flags;
    uint32_t pad;
};

// One HeapQuantileSketch's state (a parallelQuantize slice sketch, QuantileQuantizer.java:63-75),
// fixed size so that P of them all-gather as one buffer.  Levels are the bits of n / 256.
struct SketchRecord {
    int64_t n;
    LeafPartial mm;               // min / max total-order keys, flags (bit0 NaN)
    int64_t pad;
    float tail[kChunk];           // base buffer in insertion order (n % 256 used)
    float level[kMaxLevels][kK];  // level l: 128 samples, IEEE-sorted
};

// fp64 counterpart of SketchRecord.
struct SketchRecord64 {
    int64_t n;
    LeafPartial64 mm;
    double tail[kChunk];
    double level[kMaxLevels][kK];
};
// fp64 leaf in the fp32 leaf's layout (8 lanes x 32 values per chunk), skml_sketch.hip
hipError_t launch_leaf2_f64(hipStream_t st, const double* x, int64_t chunks, uint64_t s0, const uint64_t* jump_tab,
                            LeafPartial64* part, double* nodes6, double* roots, uint8_t* ubits);
hipError_t launch_sketch_record64(hipStream_t st, const double* x, int64_t n, const LeafPartial64* part,
                                  int64_t nparts, const double* roots, SketchRecord64* rec);
// Merge of fp64 records into (roots, tail, part) for launch_summary64 (tail, sharded = 1).
hipError_t launch_sketch_merge64(hipStream_t st, const SketchRecord64* recs, int nrec, uint64_t s0, uint64_t bit0,
                                 const uint64_t* jump_tab, double* roots, double* tail, LeafPartial64* part);

struct MergeJob {
    int64_t src_node;      // first input node index (in src buffer)
    int64_t dst_node;      // first output node index (in dst buffer), or -1 -> root slot
    int64_t chunk_base;    // first chunk covered by the job's first input node
    int32_t level_in;      // level of the input nodes
    int32_t group_log;     // each workgroup merges 2^group_log consecutive nodes
    int32_t groups;        // number of workgroups for this job
    int32_t root_level;    // >= 0: the single output is the tree root of this level
};
constexpr int kMaxJobs = 24;
struct MergePass {
    MergeJob job[kMaxJobs];
    int32_t njobs;
    int32_t fuse_summary;  // last pass: its last workgroup also runs the summary
    int32_t wg_prefix[kMaxJobs + 1];
};

__host__ __device__ inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
// Packed code width: smallest of 1, 2, 4, 8, 16 bits holding bin_num codes.
__host__ __device__ inline int code_bits_for(int bins) {
    int b = 1;
    while ((1LL << b) < bins) b <<= 1;
    return b;
}
__host__ __device__ inline size_t dense_codes_offset(int req_bins) {
    return align_up(kHeaderBytes + 8 * (size_t)(req_bins - 1), 256);
}

// Upper merge nodes (tree levels >= kLeafTopLevel + 1) of the fixed merge tree over C chunks,
// numbered level by level: node i of level L covers chunks [i 2^L, (i+1) 2^L), and its number is
// upper_level_offset(C, L) + i.  The leaf kernel draws their compaction bits (one per wave) into
// a byte array so the merge passes look them up instead of jumping the LCG themselves.
__host__ __device__ inline int64_t upper_level_offset(int64_t C, int L) {
    int64_t o = 0;
    for (int l = kLeafTopLevel + 1; l < L; l++) o += C >> l;
    return o;
}
__host__ __device__ inline int64_t upper_node_count(int64_t C) { return upper_level_offset(C, kMaxLevels); }

// ---- kernel launchers (skml_sketch.hip) ----
// ubits: upper_node_count(full tiles * 64) bytes; the leaf draws the upper merge tree's bits into it
// x: `chunks` x 256 values of storage type xtype (launch_leaf, launch_merge_pass, launch_summary
// and launch_quantize alike)
hipError_t launch_leaf(hipStream_t st, const void* x, int64_t chunks, uint64_t s0,
                       const uint64_t* jump_tab, LeafPartial* part, float* nodes6, float* roots, uint8_t* ubits,
                       int xtype = kXF32);
hipError_t launch_leaf_stage(hipStream_t st, int stage, const float* x, int64_t chunks, uint64_t s0,
                             const uint64_t* jump_tab, LeafPartial* part, float* scratch, float* roots);
// fp64 merge pass over double nodes (no summary; `next` as in launch_merge_pass).
hipError_t launch_merge_pass64(hipStream_t st, const MergePass& pass, const MergePass* next, const double* src,
                               double* dst, double* next_dst, double* roots, uint64_t s0, const uint64_t* jump_tab,
                               unsigned* done, const uint8_t* ubits, int64_t uchunks);
// Slice sketch -> record (after the leaf and the merge passes without a summary).
hipError_t launch_sketch_record(hipStream_t st, const float* x, int64_t n, const LeafPartial* part, int64_t nparts,
                                const float* roots, SketchRecord* rec);
// HeapQuantileSketch.merge of recs[0..nrec) in order (compaction bits from stream index bit0
// on), then the summary of the merged sketch (n_total values) into payload's header, splits and
// the quantize LUT; the header's n is n_local.  scratch: kMaxLevels*kK + kChunk floats and nrec
// LeafPartials (device).
hipError_t launch_sketch_merge(hipStream_t st, const SketchRecord* recs, int nrec, uint64_t s0, uint64_t bit0,
                               const uint64_t* jump_tab, int64_t n_total, int64_t n_local, const int64_t* ranks,
                               int req_bins, int dedup, void* payload, double* scratch_raw, QuantLut* lut,
                               float* scratch_roots, float* scratch_tail, LeafPartial* scratch_part);
// `next` (may be null): a one-workgroup pass run by this pass's last workgroup (its src is `dst`,
// its output `next_dst`), saving a launch.
hipError_t launch_merge_pass(hipStream_t st, const MergePass& pass, const MergePass* next, const float* src,
                             float* dst, float* next_dst, float* roots, uint64_t s0, const uint64_t* jump_tab,
                             unsigned* done, const void* x, int64_t n, const LeafPartial* part, int64_t nparts,
                             const int64_t* ranks, int req_bins, int dedup, void* payload,
                             double* scratch_raw, QuantLut* lut, const uint8_t* ubits, LeafPartial* part_red,
                             int64_t nred, int64_t part_from, int xtype = kXF32);
hipError_t launch_summary(hipStream_t st, const void* x, int64_t n, const LeafPartial* part,
                          int64_t nparts, const float* roots, const int64_t* ranks, int req_bins,
                          int dedup, void* payload, double* scratch_raw, QuantLut* lut, int xtype = kXF32);
// getQuantiles' rank table for (n, bins) written on the device (bins - 1 int64)
hipError_t launch_set_ranks(hipStream_t st, int64_t n, int bins, int64_t* ranks);
hipError_t launch_set_splits(hipStream_t st, void* payload, int64_t n, const double* splits_dev,
                             int nsplits, double mn, double mx, int req_bins, QuantLut* lut);
// ---- kernel launchers (skml_dense.hip) ----
// The quantize pass's resident workgroups per CU, one entry per (instantiation, dynamic LDS bytes)
// asked of the runtime so far; lives in the context (skml_ctx::qres).
struct QuantResidency {
    static constexpr int kSlots = 16;
    struct Entry {
        int inst;
        size_t lds;
        int wgs;
    } e[kSlots];
    int used = 0, next = 0;
    int cus = 0;  // the device's CU count
};
// lut == nullptr: every workgroup builds the bucket table itself from the payload's splits (the
// quantile encodes); otherwise the caller's table (set-splits, uniform and ZipML encodes, whose
// cmax may ask for the literal indexOf).  req_bins sizes the kernel's LDS tables.  wgs_out (debug):
// report the resident workgroups per CU of the selected form and launch nothing.
hipError_t launch_quantize(hipStream_t st, QuantResidency* res, const void* x, int64_t n, void* payload,
                           const QuantLut* lut, int req_bins, int xtype = kXF32, int* wgs_out = nullptr);
// The table the summary builds for the quantile encodes' quantize pass: none (the pass builds its
// own).  -DSKML_Q_GLOBAL_LUT=1 (A/B builds) restores the summary-built global 16-bit table.
#ifndef SKML_Q_GLOBAL_LUT
#define SKML_Q_GLOBAL_LUT 0
#endif
inline QuantLut* summary_lut(QuantLut* lut) { return SKML_Q_GLOBAL_LUT ? lut : nullptr; }
// out: n values of storage type otype; a 16-bit `out` needs 2-byte alignment only (16-byte stores
// when it is 16-byte aligned, element stores otherwise), a float `out` 16-byte alignment
hipError_t launch_decode(hipStream_t st, const void* payload, void* out, int64_t n, int otype = kXF32);
hipError_t launch_decode_sum(hipStream_t st, const void* payloads, int P, size_t stride, void* out,
                             int64_t n, double scale, int common_bits,
                             int max_bins, int otype = kXF32);  // common_bits 0: mixed widths
hipError_t launch_bins(hipStream_t st, const void* payload, int32_t* bins, int64_t n);
hipError_t launch_ref_body(hipStream_t st, const void* payload, uint8_t* out, int64_t n, int width);
hipError_t launch_times_by(hipStream_t st, void* payload, double x);
// ---- FixedPointGradient (skml_fixed.hip) ----
constexpr int kFxHeaderBytes = 256;   // the 64-byte header padded: the words start here
constexpr int kFxMinBits = 2, kFxMaxBits = 29;
constexpr int kFxMaxParts = 1024;     // workgroup partials of the sum of squares
// One workgroup's part of the sum of squares; flags bit 0: a value that is not zero.
struct FxPartial {
    double sum;
    uint32_t flags;
    uint32_t pad;
};
static_assert(sizeof(skml_fixed_header) == 64, "the fixed-point header is 64 bytes");
__host__ __device__ inline int64_t fixed_words(int64_t n, int bits) { return (n * bits + 63) >> 6; }
// x: n values, float (wide = 0) or double; part: kFxMaxParts partials.  The norm's two launches
// write the header (and zero its padding and the words' tail padding), the quantize pass the words.
hipError_t launch_fixed_norm(hipStream_t st, const void* x, int wide, int64_t n, int bits, int64_t seed,
                             FxPartial* part, void* payload);
hipError_t launch_fixed_quantize(hipStream_t st, const void* x, int wide, int64_t n, void* payload,
                                 const uint64_t* jump_tab);
hipError_t launch_fixed_decode(hipStream_t st, const void* payload, void* out, int wide, int64_t n);
// bits: the payloads' common width (checked by the caller)
hipError_t launch_fixed_decode_sum(hipStream_t st, const void* payloads, int P, size_t stride, float* out,
                                   int64_t n, double scale, int bits);
hipError_t launch_fixed_codes(hipStream_t st, const void* payload, int32_t* codes, int64_t n);
hipError_t launch_fixed_times_by(hipStream_t st, void* payload, double x);
// ---- optimiser update (skml_optim.hip; ml/objective/GradientDescent.scala, Adam.scala) ----
// What the update kernels take by value: the step's constants, computed once on the host in the
// reference's double arithmetic (Adam.scala:54-57).
struct OptConsts {
    double lr;
    double beta1, beta2;
    double omb1, omb2;  // 1 - beta1, 1 - beta2
    double c_m;         // Math.sqrt(1 - beta2_t)
    double c_d;         // 1 - beta1_t
    double eps;
    int32_t live;       // 1: only elements with |g| > 1e-8 are touched
    int32_t adam;
};
constexpr int kOptPer = 8;  // elements per lane and step of the dense update kernels
// w / m / v: n values of float (wide = 0) or double, 16-byte aligned; m, v null for SGD.
// common_bits / max_bins as launch_decode_sum.
hipError_t launch_decode_sum_step(hipStream_t st, const void* payloads, int P, size_t stride, int64_t n, double scale,
                                  int common_bits, int max_bins, const OptConsts& k, int wide, void* w, void* m,
                                  void* v);
// *count (zeroed by the caller on the same stream) += #{i : |scale * sum_p v_p[i]| > 1e-8}
hipError_t launch_decode_sum_live(hipStream_t st, const void* payloads, int P, size_t stride, int64_t n, double scale,
                                  unsigned long long* count);
// g: n values of float (g_wide = 0) or double, 16-byte aligned
hipError_t launch_opt_step(hipStream_t st, const void* g, int g_wide, int64_t n, double scale, const OptConsts& k,
                           int wide, void* w, void* m, void* v);
hipError_t launch_opt_count(hipStream_t st, const void* g, int g_wide, int64_t n, double scale,
                            unsigned long long* count);
// keys strictly increasing (not verified; a key outside [0, dim) is skipped)
hipError_t launch_opt_step_kv(hipStream_t st, const int32_t* keys, const void* vals, int v_wide, int64_t nnz,
                              int64_t dim, double scale, const OptConsts& k, int wide, void* w, void* m, void* v);
// launch_decode_sum_step and launch_decode_sum_live for P fixed-point payloads of one width `bits`
// (skml_fixed.hip): k_fixed_decode_sum's walk with the update, or the count, in place of the store.
hipError_t launch_fixed_decode_sum_step(hipStream_t st, const void* payloads, int P, size_t stride, int64_t n,
                                        double scale, int bits, const OptConsts& k, int wide, void* w, void* m, void* v);
hipError_t launch_fixed_decode_sum_live(hipStream_t st, const void* payloads, int P, size_t stride, int64_t n,
                                        double scale, int bits, unsigned long long* count);
// ---- mini-batch gradient (skml_glm.hip; ml/objective/GradientDescent.scala:23-87, Loss.scala:56-137) ----
// `wide`: w holds doubles (else floats, widened exactly).  lanes: 1, 8 or 64 lanes per row
// (glm_lanes_per_row picks from the data set's mean row length).  pre / loss may be null.
int glm_lanes_per_row(int64_t nnz, int64_t rows);
hipError_t launch_glm_predict(hipStream_t st, const skml_glm_data& d, int64_t row0, int64_t batch, int loss_kind,
                              const void* w, int wide, int lanes, double* pre, double* coef, double* loss);
// *obj = the sum of loss[0 .. batch) by one workgroup: 256 strided sequential sums, then a fixed tree
hipError_t launch_glm_loss_sum(hipStream_t st, const double* loss, int64_t batch, double* obj);
// g[k] for every k in [0, dim) in plusBy's order; *count (zeroed by the caller) += #{|g[k]| > 1e-8}
hipError_t launch_glm_plus_by(hipStream_t st, const skml_glm_data& d, int64_t row0, int64_t batch, const double* coef,
                              double* g, unsigned long long* count);
// timesBy(times), then the regulariser, in place; keys null: the dense form over dim values
hipError_t launch_glm_finish(hipStream_t st, const int32_t* keys, double* vals, int64_t n, int64_t dim, double times,
                             int reg_kind, double reg_param, const void* w, int wide);
// ---- validation pass (skml_glm.hip, skml_valid.hip; ml/util/ValidationUtil.scala:12-93) ----
// Every row of d: pre (may be null), loss, and cnt[0 .. 5) += truePos, trueNeg, falsePos, falseNeg, NaN
// scores (zeroed by the caller on the same stream).  d's column-order arrays are not read.
hipError_t launch_glm_valid(hipStream_t st, const skml_glm_data& d, int loss_kind, const void* w, int wide, int lanes,
                            double* pre, double* loss, unsigned long long* cnt);
// *out = ((0.0 + x[0]) + x[1]) + ... + x[n - 1] by one wave
hipError_t launch_glm_seq_sum(hipStream_t st, const double* x, int64_t n, double* out);
// Scratch of the key-and-payload sort over n scores; the sorted permutation ends in idx_a.
struct ValidAucScratch {
    uint64_t *keys_a, *keys_b;
    uint32_t *idx_a, *idx_b;
    uint32_t *hist, *hist_tmp;
};
size_t valid_auc_layout(int64_t n, ValidAucScratch* out, char* base);
// *nan_count (zeroed by the caller) += the NaN scores
hipError_t launch_valid_keys(hipStream_t st, const double* score, int64_t n, const ValidAucScratch& s,
                             unsigned long long* nan_count);
// pass 0 .. 7 in order
hipError_t launch_valid_sort_pass(hipStream_t st, int64_t n, int pass, const ValidAucScratch& s);
// res[0] += sigma, res[1] += M (zeroed by the caller); order (may be null): the permutation as int32
hipError_t launch_valid_rank_sum(hipStream_t st, const ValidAucScratch& s, const double* label, int64_t n, int32_t* order,
                                 unsigned long long* res);
// ---- ZipMLQuantizer (skml_zip.hip) ----
constexpr int kZipMinBins = 4;  // bin_num 2 and 3 reach thrNum = 0 (selectKthLargest of nothing)
constexpr int kZipTail = 4096;   // splitNum at which the rounds move into one workgroup's LDS
enum : int { kZipOk = 0, kZipThrZero = 1, kZipNoProgress = 2 };
// Device state of one call: the select's walk, the round's result, the search's outcome.
struct ZipState {
    uint64_t prefix;  // digits of the threshold's key fixed so far
    int64_t k;        // rank (from the largest) still looked for among the candidates
    double thr;       // the round's threshold
    int64_t kept;     // pairs the round kept
    int32_t bad;      // a NaN or an infinity in the input
    int32_t status;   // kZipOk / kZipThrZero / kZipNoProgress (k_zip_finish)
    int32_t bin_num;  // the final splitNum
    int32_t rounds;   // rounds run by k_zip_finish
    double mn, mx;
    uint32_t hist[256];
};
struct ZipScratch {
    ZipState* state;
    void* keys_a;  // uint32 (fp32 input) or uint64 keys, ping-pong
    void* keys_b;
    int32_t* idx_a;  // splitIndex ping-pong, over the keys
    int32_t* idx_b;
    double* sorted;
    double* r;
    double* t;
    double* err;
    uint32_t* hist;  // sort: 256 x tiles digit counts, scanned in place
    uint32_t* hist_tmp;
    uint32_t* blockcnt;
    uint32_t* blockcnt_tmp;
    double* tot_a;  // prefix sums: workgroup totals of every tree level
    double* tot_b;
    double* splits;
};
size_t zip_scratch_layout(int64_t n, int wide, int own_prefix, ZipScratch* out, char* base);
// s.state zeroed by the caller; its `bad` flag reports a NaN or an infinity
hipError_t launch_zip_sort(hipStream_t st, const void* x, int wide, int64_t n, const ZipScratch& s, double* sorted);
hipError_t launch_zip_scan(hipStream_t st, const double* sorted, int64_t n, double* r, double* t, const ZipScratch& s);
// one round over idx (null: the identity) into idx_out; s.state->kept then holds the kept pairs
hipError_t launch_zip_round(hipStream_t st, const int32_t* idx, int32_t* idx_out, int64_t split_num, int64_t n,
                            int bins, const double* r, const double* t, const ZipScratch& s);
// the rounds from split_num <= kZipTail on (or none), then s.splits and s.state's outcome
hipError_t launch_zip_finish(hipStream_t st, const int32_t* idx, int64_t split_num, int64_t n, int bins,
                             const double* r, const double* t, const double* sorted, const ZipScratch& s);
// The sort's pieces that the validation pass's key-and-payload sort (skml_valid.hip) runs as they are:
// the digit counts of the kZsTile-key tiles of uint64 keys, digit-major (hist[d * nblocks + b]), and the
// exclusive scan of uint32 in place (tmp: zip_scan_u32_tmp(n) entries).
hipError_t launch_zip_hist64(hipStream_t st, const uint64_t* keys, int64_t n, int pass, uint32_t* hist, int nblocks);
hipError_t zip_scan_u32(hipStream_t st, uint32_t* data, int64_t n, uint32_t* tmp);
size_t zip_scan_u32_tmp(int64_t n);
// ---- kernel launchers (skml_f64.hip) ----
hipError_t launch_summary64(hipStream_t st, const double* x, int64_t n, const LeafPartial64* part, int64_t nparts,
                            const double* roots, const int64_t* ranks, int req_bins, int dedup, void* payload,
                            double* g_raw, QuantLut* lut,
                            const double* tail = nullptr, int sharded = 0, int64_t n_local = 0);
// `lut` may be null; fp64 values are looked up by their round-down fp32 image, then corrected
// by exact double compares.
hipError_t launch_quantize64(hipStream_t st, const double* x, int64_t n, void* payload, const QuantLut* lut,
                             const int* qflags, int req_bins);
hipError_t launch_decode64(hipStream_t st, const void* payload, double* out, int64_t n);
int uniform_partials(int64_t n);
hipError_t launch_uniform(hipStream_t st, const float* x, int64_t n, int bin_num, UniPartial* part, void* payload,
                          QuantLut* lut, int* qflags);
hipError_t launch_uniform64(hipStream_t st, const double* x, int64_t n, int bin_num, UniPartial* part,
                            void* payload, QuantLut* lut, int* qflags);
// *bad (device int, zeroed by the caller) counts waves that met a bin outside [0, binNum)
hipError_t launch_pack_ref(hipStream_t st, const uint8_t* body, int width, int64_t n, void* payload, int* bad);

}  // namespace skml
