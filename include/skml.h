/*
 * skml.h -- C ABI of the MI355X SketchML gradient codec (libskml.so, sketchml_amd/lib/).
 *
 * This is the drop-in boundary for the reference's `sketch` module hot path.  Every entry point
 * takes plain pointers and sizes (no torch / no C++ types) so the reference's Java host can bind
 * it through JNI.  Each function below names the reference interface it
 * replaces; paths are relative to
 *   /root/reference/sketch/src/main/java/org/dma/sketchml/sketch/
 *
 * Execution model: a context owns one HIP stream on one device.  Encode / decode calls enqueue
 * device work and return without synchronising; errors detected on the device (NaN input, as
 * HeapQuantileSketch.update throws, HeapQuantileSketch.java:75-76) are recorded in the payload
 * header and reported by skml_dense_info() / skml_ctx_sync().
 *
 * RNG model: the reference draws compaction bits from an unseeded JVM-global java.util.Random
 * (QSketchUtils.java:9,47).  Here the stream is java.util.Random(params.seed), consumed in exactly
 * the order the sequential Java sketch would consume it, so results are reproducible and equal
 * to the reference algorithm driven by that stream.
 */
#ifndef SKML_H
#define SKML_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes; the JNI shim maps them to the reference's exceptions ---- */
#define SKML_OK 0
#define SKML_E_ARG 1   /* SketchMLException / QuantileSketchException (argument checks) */
#define SKML_E_NAN 2   /* QuantileSketchException("Encounter NaN value") */
#define SKML_E_ORDER 3 /* SketchMLException("Log for ...") on non-increasing keys */
#define SKML_E_HIP 4
#define SKML_E_RCCL 5
#define SKML_E_OOM 6
#define SKML_E_STATE 7

#define SKML_DENSE_MAGIC 0x444D4B53u /* "SKMD" */
#define SKML_MAX_BINS 65536          /* Quantizer.writeObject's short-code limit */

typedef struct skml_ctx skml_ctx;

/* Codec knobs (ml/conf/MLConf.scala:35-42; Quantizer.java:29; GroupedMinMaxSketch.java:35-36;
 * MinMaxSketch.java:25).  The sketch's k is fixed at 128 (HeapQuantileSketch.java:13). */
typedef struct skml_params {
    int32_t bin_num;   /* requested bins, 2..65536, default 256 */
    int32_t group_num; /* sparse: MinMax groups, default 8 */
    int32_t row_num;   /* sparse: MinMax rows, default 2 */
    int32_t dedup;     /* 1: QuantileQuantizer.quantize (Maths.unique); 0: parallelQuantize */
    double col_ratio;  /* sparse: MinMax columns / group size, default 0.3 */
    int64_t seed;      /* java.util.Random seed of the sketch's compaction stream */
    int64_t hash_seed; /* sparse: group g's hashes are drawn from Random(hash_seed + g) */
    int32_t quant_type; /* sparse: the values' quantizer, SKML_QUANTILE (default) or SKML_UNIFORM
                           (Quantizer.newQuantizer, base/Quantizer.java:126-136); the dense path
                           has separate entry points per quantizer */
    int32_t parallelism; /* sparse path: slice sketches of the values' parallelQuantize when > 1
                            (Constants.Parallel, SparseVectorCompressor.java:90-91); 0 or 1: one.
                            The dense path takes T as an argument
                            (skml_dense_encode_parallel_f32) */
} skml_params;
#define SKML_QUANTILE 0
#define SKML_UNIFORM 1

/* Device payload header (little-endian, 64 bytes) followed by double splits[req_bins-1],
 * padded to 256 bytes, then the packed codes (code_bits per element, LSB-first). */
typedef struct skml_dense_header {
    uint32_t magic;
    int32_t status;    /* SKML_OK or SKML_E_NAN */
    int64_t n;
    int32_t bin_num;   /* effective bins (after Maths.unique), Quantizer.binNum */
    int32_t zero_idx;  /* Quantizer.zeroIdx */
    int32_t code_bits; /* 1, 2, 4, 8 or 16 */
    int32_t req_bins;  /* capacity of the splits array + 1 */
    double min;        /* Quantizer.min (Double.MAX_VALUE-initialised quirk kept) */
    double max;        /* Quantizer.max (Double.MIN_VALUE-initialised quirk kept) */
    int64_t codes_offset;
    int64_t reserved;
} skml_dense_header;

void skml_params_default(skml_params* p);
const char* skml_last_error(void); /* thread-local message of the last failing call */
const char* skml_version(void);

/* Context: one HIP stream on one device.  `hip_stream` is an existing hipStream_t (e.g.
 * torch.cuda.current_stream().cuda_stream; NULL is the device's default stream) or
 * SKML_STREAM_OWN, in which case the library creates and owns a non-blocking stream. */
#define SKML_STREAM_OWN ((void*)(intptr_t)-1)
int skml_ctx_create(int device, void* hip_stream, skml_ctx** out);
int skml_ctx_destroy(skml_ctx* ctx);
int skml_ctx_sync(skml_ctx* ctx);
int skml_ctx_set_stream(skml_ctx* ctx, void* hip_stream);

/* Per-kernel timing with HIP events recorded on the context stream around the launches of the
 * selected kernels (profiling aid for bench.py's roofline; off by default).  `mask`: bit k
 * times kernel id k; SKML_TIMING_ALL times every kernel; 0 turns timing off. */
#define SKML_K_LEAF 0
#define SKML_K_MERGE 1
#define SKML_K_SUMMARY 2
#define SKML_K_QUANTIZE 3
#define SKML_K_DECODE 4
#define SKML_K_DECODE_SUM 5
#define SKML_K_SPARSE 6
#define SKML_K_GLM_PREDICT 7 /* k_glm_predict and the reduction of loss_j */
#define SKML_K_GLM_PLUS_BY 8
#define SKML_K_GLM_FINISH 9
#define SKML_K_GLM_VALID 10  /* k_glm_valid */
#define SKML_K_SEQ_SUM 11    /* the ordered sum (or, with SKML_VALID_TREE_SUM, the tree sum) */
#define SKML_K_VALID_SORT 12 /* the keys and one launch per pass of the key-and-payload sort */
#define SKML_K_VALID_RANK 13 /* the rank sum */
#define SKML_K_COUNT 14
#define SKML_TIMING_ALL (-1)
int skml_ctx_set_timing(skml_ctx* ctx, int mask);
/* Synchronises; total device milliseconds and launch count of kernel `kid` since the reset. */
int skml_ctx_kernel_stats(skml_ctx* ctx, int kid, int64_t* launches, double* total_ms);
int skml_ctx_reset_stats(skml_ctx* ctx);
/* Profiling ablation of the sketch leaf kernel (stage 0 load, 1 + leaf sort, 2 + in-wave merges,
 * 3 full): average device ms over `iters` launches on n values.  Not part of the codec. */
int skml_debug_leaf_stage(skml_ctx* ctx, const float* x_dev, int64_t n, int stage, int iters,
                          double* avg_ms);
/* Test hook: while `on` is non-zero, the sparse encode treats its two MinMax staging scratch
 * buffers (the hashed cells and the per-(tile, bucket) reservations) as failed allocations, so
 * the fallback path (key-carrying pairs, rehashing scatter) is exercised.  Not part of the codec. */
int skml_debug_sparse_scratch_fail(int on);

/* Test hook: how the calling thread's last restore / decode merged the groups' runs (Sort.merge):
 * 0 none (fewer than two groups or no keys), 1 the one-pass key-range merge, 2 the pairwise merge
 * rounds (forced by SKML_FORM_RS_ROUNDS), 3 the one-pass merge found the input irregular (a run
 * that does not ascend, a repeated key, a key outside [0, INT32_MAX)) and the rounds ran instead. */
int skml_debug_sparse_merge_path(void);

/* Test hook: the scratch budget of one batch of skml_sparse_decode_sum_*, process-wide.  The sum
 * restores its payloads in batches whose keys, bins and run bounds fit 3 GiB of scratch; a later
 * batch continues the sum of the earlier ones.  `bytes` > 0 replaces the 3 GiB for the calls that
 * follow (a value above 3 GiB is taken as 3 GiB: the batch's offsets are 32-bit), so that small
 * payloads reach the continuation; 0 restores it.  A batch always takes at least one payload.
 * Returns the previous setting (0: the 3 GiB).  Not part of the codec. */
int64_t skml_debug_sparse_sum_budget(int64_t bytes);

/* Test hook: how many scratch batches and how many tile launches the calling thread's last
 * skml_sparse_decode_sum_* made (up to where it stopped, if it failed).  Not part of the codec. */
int skml_debug_sparse_sum_path(int32_t* batches, int32_t* launches);

/* Test hook: force one of the library's alternative kernel forms, process-wide.  Every form gives
 * the same results (the tests run each one against the oracle); 0 is the library's own choice.
 * Returns the previous value, -1 for an unknown id, or -2 (nothing changed) for a form whose
 * kernels only the A/B build carries (built with -DSKML_AB into sketchml_amd/lib_ab/: the forms
 * measured slower than the default, kept for A/B runs).  Not part of the codec. */
#define SKML_FORM_LEAF_SPLIT 0      /* 2: the split leaf always (the default at every size); A/B build: 1 one wave per 64-chunk tile, 3 / 4 / 5 the last 25 / 12.5 / 50 % split */
#define SKML_FORM_DECODE_SUM 1      /* 1: the per-payload kernel (the form for > 8 payloads, mixed widths or wide tables); A/B build: 2 the occupancy form without prefetch */
#define SKML_FORM_PART_BALLOT 2     /* 1: the ballot-ranked partition scatter */
#define SKML_FORM_RS_ROUNDS 3       /* 1: Sort.merge by the pairwise merge rounds always (the fallback for irregular runs); A/B build: 2 the one-pass merge without prefetch */
#define SKML_FORM_DEC_ROWS_SERIAL 4 /* 1: the generic MinMax query (rows one by one; the form for edge tiles and rows != 2) for every tile; A/B build: 2 persistent workgroups */
#define SKML_FORM_AGG_TILES 5       /* 0: Gradient.sum's sum tile in LDS (the default), 1: the 4,096-key wave-per-payload tiles (the form for > 8 groups or > 256 quantValues); A/B build: 2 / 3 staged tiles four / two per round, 4 staged tiles with the next tile prefetched, 5 staged tiles without */
#define SKML_FORM_AGG_ONE_LANE 6    /* 1: Gradient.sum restores every payload on the caller's stream */
#define SKML_FORM_RUN_BOUNDS 7      /* A/B build: 1 the runs' tile / key-range bounds (Gradient.sum, the one-pass Sort.merge) in passes of their own (k_agg_bounds, k_rs_bounds) instead of by the key query */
#define SKML_FORM_DEC_LOOKBACK 8    /* A/B build: 1 the restore's bit lengths and deltas in one pass with decoupled look-backs for the bit offsets and the deltas' prefixes, 2 the same pass with the deltas' tile scan after it */
#define SKML_FORM_COUNT 9
int skml_debug_form(int id, int value);
/* Build flags of the loaded library: SKML_BUILD_AB when it carries the A/B-only forms. */
#define SKML_BUILD_AB 1
int skml_build_flags(void);

/* ---- Dense path: QuantileQuantizer.quantize + Quantizer.getBins/getValues ---- */

/* Bytes of a device payload able to hold n codes for `bin_num` requested bins. */
size_t skml_dense_payload_bytes(int64_t n, int32_t bin_num);

/* QuantileQuantizer.quantize(double[]) (quantization/QuantileQuantizer.java:27-50) on fp32
 * input: k=128 quantile sketch (HeapQuantileSketch.update), getQuantiles(bin_num), Maths.unique,
 * findZeroIdx, then bins[i] = indexOf(x[i]) (Quantizer.java:49-92), packed into the payload.
 * params->dedup = 0 gives parallelQuantize's no-dedup split table (QuantileQuantizer.java:85).
 * x_dev and payload_dev are device pointers.  Asynchronous. */
int skml_dense_encode_f32(skml_ctx* ctx, const float* x_dev, int64_t n, const skml_params* params,
                          void* payload_dev, size_t payload_cap);

/* The same on fp64 input (the reference's own double[] path): the sketch
 * sorts and merges 64-bit keys, indexOf compares in double.  Asynchronous. */
int skml_dense_encode_f64(skml_ctx* ctx, const double* x_dev, int64_t n, const skml_params* params,
                          void* payload_dev, size_t payload_cap);

/* The same on bf16 / fp16 input (torch.bfloat16 / torch.float16 gradients; 16-bit values travel
 * as uint16_t).  Widening a 16-bit float to fp32 is exact for every bit pattern, so the result is
 * defined as skml_dense_encode_f32 of the widened buffer and the payload is byte for byte the
 * same; the kernels widen in registers and no fp32 copy is made.  Arguments, params->dedup /
 * seed and status codes as skml_dense_encode_f32 (x_dev 16-byte aligned).  Asynchronous. */
int skml_dense_encode_bf16(skml_ctx* ctx, const uint16_t* x_dev, int64_t n, const skml_params* params,
                           void* payload_dev, size_t payload_cap);
int skml_dense_encode_f16(skml_ctx* ctx, const uint16_t* x_dev, int64_t n, const skml_params* params,
                          void* payload_dev, size_t payload_cap);

/* UniformQuantizer.quantize(double[]) (quantization/UniformQuantizer.java:21-45): min / max
 * (Double.MAX_VALUE / Double.MIN_VALUE initialised, NaN values skipped), bin_num-1 splits by
 * repeated `+= (max-min)/bin_num`, findZeroIdx, bins[i] = indexOf(x[i]).  No Maths.unique; NaN
 * values are binned, not rejected.  parallelQuantize is the same computation
 * (UniformQuantizer.java:48-70).  params->seed / dedup are ignored.  Asynchronous. */
int skml_dense_encode_uniform_f32(skml_ctx* ctx, const float* x_dev, int64_t n,
                                  const skml_params* params, void* payload_dev, size_t payload_cap);
int skml_dense_encode_uniform_f64(skml_ctx* ctx, const double* x_dev, int64_t n,
                                  const skml_params* params, void* payload_dev, size_t payload_cap);

/* Several independent buckets (QuantileQuantizer.quantize of each, e.g. the gradient buckets of
 * one DDP step): results identical to skml_dense_encode_f32 per bucket.  The buckets run on two
 * internal streams so that one bucket's sketch (VALU-bound) overlaps the previous bucket's
 * quantize pass (HBM-bound).  xs / ns / payloads / caps: host arrays of nbuckets entries
 * (device pointers).  Ordered after, and waited for by, the context's stream.  Asynchronous. */
int skml_dense_encode_batch_f32(skml_ctx* ctx, int32_t nbuckets, const float* const* xs_dev, const int64_t* ns,
                                const skml_params* params, void* const* payloads_dev, const size_t* payload_caps);

/* QuantileQuantizer.parallelQuantize (QuantileQuantizer.java:53-92) with `threads` slices
 * (Constants.Parallel.getParallelism): slice t = [t*(n/T), ...), the last slice takes the
 * remainder; each slice is sketched, the sketches merged in slice order (HeapQuantileSketch.merge,
 * HeapQuantileSketch.java:186-228), no Maths.unique unless params->dedup (default params: 0).
 * The reference draws every compaction bit from one static Random (QSketchUtils.java:9) in a
 * thread-interleaved order; this is the schedule that runs the slice sketches one after another
 * and then the merges, with Random(params->seed).  threads = 1 equals skml_dense_encode_f32 with
 * dedup = 0.  Asynchronous. */
int skml_dense_encode_parallel_f32(skml_ctx* ctx, const float* x_dev, int64_t n, int32_t threads,
                                   const skml_params* params, void* payload_dev, size_t payload_cap);

/* The same split table over P devices (SURVEY §8e single-split-table mode): shard s holds
 * shard_n[s] consecutive values of one logical gradient.  Each rank sketches its shard into a
 * fixed-size device record (skml_sketch_record_bytes(0)), the records are all-gathered in shard
 * order (skml_allgather), and every rank merges them identically and quantises its own shard.
 * The result equals skml_dense_encode_parallel_f32 over the concatenation when the shards follow
 * its slicing; any shard sizes are accepted (merge order = shard order).  The payload header
 * carries the global splits / min / max / zeroIdx and n = shard_n[shard]. */
size_t skml_sketch_record_bytes(int32_t fp64);
int skml_dense_sketch_shard_f32(skml_ctx* ctx, const float* x_dev, int64_t n, const int64_t* shard_n,
                                int32_t nshards, int32_t shard, int64_t seed, void* record_dev);
int skml_dense_encode_sharded_f32(skml_ctx* ctx, const float* x_dev, int64_t n, const int64_t* shard_n,
                                  int32_t nshards, int32_t shard, const void* records_dev,
                                  const skml_params* params, void* payload_dev, size_t payload_cap);
/* fp64 input (the reference's double[] itself): records of skml_sketch_record_bytes(1) bytes. */
int skml_dense_encode_parallel_f64(skml_ctx* ctx, const double* x_dev, int64_t n, int32_t threads,
                                   const skml_params* params, void* payload_dev, size_t payload_cap);
int skml_dense_sketch_shard_f64(skml_ctx* ctx, const double* x_dev, int64_t n, const int64_t* shard_n,
                                int32_t nshards, int32_t shard, int64_t seed, void* record_dev);
int skml_dense_encode_sharded_f64(skml_ctx* ctx, const double* x_dev, int64_t n, const int64_t* shard_n,
                                  int32_t nshards, int32_t shard, const void* records_dev,
                                  const skml_params* params, void* payload_dev, size_t payload_cap);

/* Split-injected parity mode: quantise against a caller-given split table (host doubles,
 * sorted ascending), min and max, exactly as Quantizer.quantizeToBins would.  Asynchronous. */
int skml_dense_encode_with_splits_f32(skml_ctx* ctx, const float* x_dev, int64_t n,
                                      const double* splits_host, int32_t nsplits, double min,
                                      double max, void* payload_dev, size_t payload_cap);

/* DenseVectorCompressor.decompressDense (sample/DenseVectorCompressor.java:84-91):
 * out[i] = (float) Quantizer.getValues()[bin[i]].  Asynchronous. */
int skml_dense_decode_f32(skml_ctx* ctx, const void* payload_dev, float* out_dev, int64_t n);

/* decompressDense into bf16 / fp16: skml_dense_decode_f32's float rounded to nearest even.  Any
 * payload decodes to any output type.  out_dev needs 2-byte alignment only (16-byte stores when it
 * is 16-byte aligned, element stores otherwise).  Asynchronous. */
int skml_dense_decode_bf16(skml_ctx* ctx, const void* payload_dev, uint16_t* out_dev, int64_t n);
int skml_dense_decode_f16(skml_ctx* ctx, const void* payload_dev, uint16_t* out_dev, int64_t n);

/* decompressDense into double[] (the reference's return type): out[i] = getValues()[bin[i]]
 * without the float rounding.  Asynchronous. */
int skml_dense_decode_f64(skml_ctx* ctx, const void* payload_dev, double* out_dev, int64_t n);

/* Fused decode of P payloads into one sum: out[i] = scale * sum_p values_p[bin_p[i]], the
 * decode half of Gradient.sum + timesBy(1/P) (ml/gradient/Gradient.scala:44-49,
 * ml/algorithm/GeneralizedLinearModel.scala:145-150).  payloads_dev points to P payloads laid
 * out `stride` bytes apart.  Asynchronous. */
int skml_dense_decode_sum_f32(skml_ctx* ctx, const void* payloads_dev, int32_t P, size_t stride,
                              float* out_dev, int64_t n, double scale);

/* The same sum (in double, payload order, times scale, cast to float) rounded to nearest even
 * into a bf16 / fp16 output; out_dev as in skml_dense_decode_bf16.  Asynchronous. */
int skml_dense_decode_sum_bf16(skml_ctx* ctx, const void* payloads_dev, int32_t P, size_t stride,
                               uint16_t* out_dev, int64_t n, double scale);
int skml_dense_decode_sum_f16(skml_ctx* ctx, const void* payloads_dev, int32_t P, size_t stride,
                              uint16_t* out_dev, int64_t n, double scale);

/* Quantizer.getBins() (Quantizer.java:168-170): materialise int32 bins on the device. */
int skml_dense_bins_i32(skml_ctx* ctx, const void* payload_dev, int32_t* bins_dev, int64_t n);

/* Synchronise and read the header + splits (Quantizer.getBinNum/getSplits/getZeroIdx/getMin/
 * getMax/getN).  splits_host may be NULL; otherwise it receives bin_num-1 doubles.  Returns the
 * header's status (SKML_E_NAN if the input held a NaN). */
int skml_dense_info(skml_ctx* ctx, const void* payload_dev, skml_dense_header* hdr_host,
                    double* splits_host, int32_t splits_cap);

/* Quantizer.timesBy (Quantizer.java:119-124): scale min, max and splits in place. */
int skml_dense_times_by(skml_ctx* ctx, void* payload_dev, double x);

/* Quantizer.writeObject field stream (Quantizer.java:184-203): big-endian binNum, n,
 * splits[binNum-1], zeroIdx, min, max, bins.length, then bins as (bin-128) bytes / (bin-32768)
 * shorts / ints.  Synchronising.  *written receives the byte count (also when buf is NULL). */
int skml_dense_serialize_ref(skml_ctx* ctx, const void* payload_dev, uint8_t* buf_host,
                             size_t cap, size_t* written);
/* Quantizer.readObject (Quantizer.java:205-226) into a device payload.  Synchronising. */
int skml_dense_deserialize_ref(skml_ctx* ctx, const uint8_t* buf_host, size_t len,
                               void* payload_dev, size_t payload_cap);

/* ---- FixedPointGradient (ml/gradient/FixedPointGradient.scala:39-75): the norm-scaled
 * sign + (b-1)-bit magnitude baseline codec that Gradient.compress switches to beside the sketch
 * (ml/gradient/Gradient.scala:18-36) ---- */

#define SKML_FIXED_MAGIC 0x584D4B53u /* "SKMX" */

/* Device payload: this header (little-endian, 64 bytes) padded with zeros to 256 bytes, then
 * ceil(n * num_bits / 64) 64-bit words, padded with zero words to a multiple of 256 bytes.  Code i
 * occupies stream bits [i * num_bits, (i + 1) * num_bits), its most significant bit first
 * (BinaryUtils.setBits, sketch/binary/BinaryUtils.java:6-14); stream bit k is bit k & 63 of word
 * k >> 6 (java.util.BitSet.toLongArray).  Caller-owned and relocatable: skml_allgather moves it
 * as it is. */
typedef struct skml_fixed_header {
    uint32_t magic;
    int32_t status;   /* SKML_OK, or SKML_E_NAN: a NaN or infinite value, a norm that is not finite,
                         or a zero norm over a nonzero value (fp64 underflow) */
    int64_t n;        /* FixedPointGradient.size */
    int32_t num_bits; /* 2..29 */
    int32_t reserved0;
    double norm;      /* sqrt(sum v_i^2) times every timesBy factor */
    int64_t words_offset; /* 256 */
    int64_t seed;     /* the sigma stream: sigma_i = the i-th nextBoolean() of java.util.Random(seed) */
    int64_t reserved[2];
} skml_fixed_header;

/* Bytes of a device payload for n codes of num_bits; 0 for arguments the encode refuses. */
size_t skml_fixed_payload_bytes(int64_t n, int32_t num_bits);

/* FixedPointGradient.fromArray (FixedPointGradient.scala:39-53): norm = sqrt(sum v_i^2) in double;
 * code_i = floor(|v_i| / norm * (2^(b-1) - 1)).toInt + sigma_i, or-ed with 2^(b-1) when v_i < 0,
 * all in double in that order (fp32 input is widened first).  sigma_i is added unconditionally, so
 * |v_i| = norm with sigma_i = 1 gives the code 2^(b-1), which decodes as -0.0; an all-zero input
 * (norm 0, NaN quotient, .toInt = 0) gives code_i = sigma_i.  The reference draws sigma from an
 * unseeded global Bernoulli(0.5); here it is the i-th nextBoolean() of java.util.Random(seed),
 * i from 0.  The sum of squares is a fixed tree (no atomics): the same input gives the same bytes
 * on every run, and its relative error is below 2^-40.  num_bits outside 2..29 (the reference
 * requires < 30; 1 divides by zero) and n outside 1..2^31-1 return SKML_E_ARG.  x_dev 16-byte
 * aligned, payload_dev 256-byte aligned.  Asynchronous; the header's status reports the input.
 * Timed (skml_ctx_set_timing) as SKML_K_SUMMARY for the norm and header launches and
 * SKML_K_QUANTIZE for the quantize + pack pass; the decodes as SKML_K_DECODE / SKML_K_DECODE_SUM. */
int skml_fixed_encode_f32(skml_ctx* ctx, const float* x_dev, int64_t n, int32_t num_bits, int64_t seed,
                          void* payload_dev, size_t payload_cap);
int skml_fixed_encode_f64(skml_ctx* ctx, const double* x_dev, int64_t n, int32_t num_bits, int64_t seed,
                          void* payload_dev, size_t payload_cap);

/* FixedPointGradient.toArray (FixedPointGradient.scala:63-75): v_i = (double)(code_i & max) / max *
 * norm, negated when the sign bit is set; the f32 form stores (float)v_i.  out_dev 16-byte
 * aligned.  Asynchronous. */
int skml_fixed_decode_f32(skml_ctx* ctx, const void* payload_dev, float* out_dev, int64_t n);
int skml_fixed_decode_f64(skml_ctx* ctx, const void* payload_dev, double* out_dev, int64_t n);

/* Gradient.sum + timesBy over P fixed-point payloads `stride` bytes apart, skml_dense_decode_sum_f32's
 * contract: out[i] = (float)(scale * sum_p v_p[i]), the sum in double from +0.0 in payload order.
 * Every payload must hold n codes of one num_bits (else SKML_E_ARG) and fit its stride; P in
 * [1, 16].  Reads the headers back first (synchronises), then queues the sum. */
int skml_fixed_decode_sum_f32(skml_ctx* ctx, const void* payloads_dev, int32_t P, size_t stride,
                              float* out_dev, int64_t n, double scale);

/* The codes as int32 (BinaryUtils.getBits of every field).  Asynchronous. */
int skml_fixed_codes_i32(skml_ctx* ctx, const void* payload_dev, int32_t* codes_dev, int64_t n);

/* FixedPointGradient.timesBy (FixedPointGradient.scala:55): norm *= x, nothing else.  Asynchronous. */
int skml_fixed_times_by(skml_ctx* ctx, void* payload_dev, double x);

/* Synchronise and read the header; returns its status (SKML_E_NAN as described above). */
int skml_fixed_info(skml_ctx* ctx, const void* payload_dev, skml_fixed_header* hdr_host);

/* ---- ZipGradient's ZipMLQuantizer (ml/gradient/ZipGradient.scala:61-139): the error-minimising
 * quantizer that Gradient.compress switches to beside the sketch (ml/gradient/Gradient.scala:18-36).
 * quantize (ZipGradient.scala:70-129): sort a copy, prefix sums r of the sorted values and t of their
 * squares, then halve the split list round by round -- a pair of neighbouring ranges stays split
 * when the squared error of joining it is among the thrNum largest (Sort.selectKthLargest over the
 * errors and the zeros behind them, ties kept; an odd list's last singleton is dropped) -- until at
 * most bin_num splits are left; splits[i] = sorted[splitIndex[i + 1]] without dedup, min / max the
 * first / last sorted value, findZeroIdx, bins[i] = indexOf(x[i]).  The result is an ordinary dense
 * payload (SKML_DENSE_MAGIC, skml_dense_payload_bytes(n, bin_num) bytes, req_bins = bin_num, the
 * header's bin_num = the effective count, bin_num or bin_num - 1): decode, decode-sum, timesBy,
 * getBins, the writeObject stream and the all-gather work on it unchanged.
 *
 * The sort is Arrays.sort(double[])'s total order (-0.0 before +0.0) and so bit-exact; the prefix
 * sums are a fixed tree (DESIGN.md "ZipML"), equal on every run but rounded unlike the reference's
 * sequential loop in the last bits; given r and t, the split search is the reference's, bit for bit.
 * n in [2, 2^31 - 1], bin_num in [4, 65536] (2 and 3 always reach thrNum = 0, on which the
 * reference throws); n <= bin_num runs no round: binNum = n, splits = sorted[1..n-1].  Status:
 * SKML_E_NAN for a NaN or an infinity in the input (the reference returns garbage); SKML_E_ARG for
 * the arguments above, a short payload, and an input on which a round keeps every split -- the
 * reference's loop does not terminate there (an all-equal vector of even length > bin_num, a vector
 * of mostly exact zeros); SKML_E_OOM when the scratch cannot be allocated (the context stays usable).
 * The scratch is the context's ZipML workspace, allocated by the call that first needs its size and
 * kept (grow-only, freed with the context, like the context's other workspaces: allocating 9.7 GB
 * afresh costs the driver about half a second): skml_zip_workspace_bytes(n, fp64) bytes, about 36
 * bytes per value for fp32 input and 44 for fp64 (0 for an n the encode refuses).  x_dev 16-byte
 * aligned, payload_dev 256-byte aligned.  Synchronising (the loop's trip count depends on the data).
 * Timed (skml_ctx_set_timing) as SKML_K_SUMMARY for sort, prefix sums and split search (the rounds'
 * host read-backs included) and SKML_K_QUANTIZE for the quantize pass. */
size_t skml_zip_workspace_bytes(int64_t n, int32_t fp64); /* scratch a call over n values needs */
int skml_zip_encode_f32(skml_ctx* ctx, const float* x_dev, int64_t n, int32_t bin_num, void* payload_dev,
                        size_t payload_cap);
int skml_zip_encode_f64(skml_ctx* ctx, const double* x_dev, int64_t n, int32_t bin_num, void* payload_dev,
                        size_t payload_cap);
/* Test hooks, not part of the codec: the sorted copy (n doubles) and the two prefix sums exactly as
 * the encode computes them (the same code).  r_dev and t_dev may both be NULL: the sort alone.
 * Synchronising; SKML_E_NAN as the encode. */
int skml_debug_zip_prefix_f32(skml_ctx* ctx, const float* x_dev, int64_t n, double* sorted_dev, double* r_dev,
                              double* t_dev);
int skml_debug_zip_prefix_f64(skml_ctx* ctx, const double* x_dev, int64_t n, double* sorted_dev, double* r_dev,
                              double* t_dev);
/* Frees the context's ZipML workspace (waits for the stream first); the next encode allocates it
 * again.  For a caller that encoded one large gradient and wants the memory back. */
int skml_zip_release_workspace(skml_ctx* ctx);
/* Test hook: the halving rounds of the context's last successful skml_zip_encode_* (-1: no context). */
int skml_debug_zip_rounds(skml_ctx* ctx);

/* ---- Optimiser update (ml/objective/GradientDescent.scala:89-117, ml/objective/Adam.scala:27-77):
 * the consumer of Gradient.sum, optimizer.update(bcGrad.value, weights)
 * (ml/algorithm/GeneralizedLinearModel.scala:156) ----
 *
 * The gradient of element i is g_i = scale * x_i in double, where x_i is the sum of the P decoded
 * payload values (from +0.0, in payload order, as the decode-sum kernels hold it before their float
 * cast; the fused entries never round it to float), an array element, or a key's value.
 *   SGD:   w_i -= g_i * lr                                   (the caller decays lr)
 *   Adam:  m_t = beta1*m + (1-beta1)*g ;  v_t = beta2*v + ((1-beta2)*g)*g
 *          w -= ((sqrt(1-beta2_t)*m_t) / ((1-beta1_t)*(sqrt(v_t)+eps))) * lr ;  m = m_t ;  v = v_t
 * in double in exactly this order, without contraction; sqrt and / are correctly rounded.  The state
 * w, m, v shares one type, the entry's suffix: _f64 is the reference's; _f32 state is widened on
 * load, the update runs in double on the unrounded m_t and v_t, and each of w, m, v is rounded to
 * float once, at its store.
 * select: SKML_OPT_ALL updates every element (update(DenseDoubleGradient): with g = 0, m and v
 * still decay and w still moves); SKML_OPT_LIVE only those with fabs(g_i) > 1e-8, every other
 * element keeps w, m, v bit for bit (what toSparse hands update(SparseDoubleGradient));
 * SKML_OPT_AUTO is toAuto (DenseDoubleGradient.scala:64-95): it counts the live elements first and
 * takes ALL when nnz > dim * 2 / 3 in Java int arithmetic, LIVE otherwise; it costs a second pass
 * over the input and synchronises for the count.  ALL and LIVE are one pass. */
#define SKML_OPT_SGD 0
#define SKML_OPT_ADAM 1
#define SKML_OPT_ALL 0
#define SKML_OPT_LIVE 1
#define SKML_OPT_AUTO 2
typedef struct skml_opt_params {
    int32_t kind;   /* SKML_OPT_SGD | SKML_OPT_ADAM */
    int32_t select; /* SKML_OPT_ALL | SKML_OPT_LIVE | SKML_OPT_AUTO */
    double lr;
    double beta1, beta2;     /* Adam.scala:20-21 */
    double beta1_t, beta2_t; /* Adam.scala:22-23, advanced by the caller (Adam.scala:29-32) */
    double eps;              /* Maths.EPS */
} skml_opt_params;
/* Adam, ALL, beta1 = beta1_t = 0.9, beta2 = beta2_t = 0.999, eps = 1e-8, lr = 0. */
void skml_opt_params_default(skml_opt_params* p);

/* Gradient.sum + timesBy + optimizer.update in one pass over P gathered dense payloads (a ZipML
 * payload is one): the decode-sum's kernel forms with the update of w / m / v in place of the
 * fp32 store.  payloads_dev / P / stride / n / scale and the header checks (read back first:
 * magic, status with SKML_E_NAN, n, code width, stride) are skml_dense_decode_sum_f32's.  w_dev, m_dev,
 * v_dev: n values each, 16-byte aligned, overlapping neither each other nor the payloads; m_dev and
 * v_dev must be NULL for SGD.  SKML_E_ARG for a NULL context, misaligned or overlapping state, P
 * outside [1, 16], n < 1, or lr / betas / eps that are not finite.  ALL and LIVE return with the
 * update queued on the context's stream.  Timed under SKML_K_DECODE_SUM. */
int skml_dense_decode_sum_step_f32(skml_ctx* ctx, const void* payloads_dev, int32_t P, size_t stride, int64_t n,
                                   double scale, const skml_opt_params* params, float* w_dev, float* m_dev,
                                   float* v_dev);
int skml_dense_decode_sum_step_f64(skml_ctx* ctx, const void* payloads_dev, int32_t P, size_t stride, int64_t n,
                                   double scale, const skml_opt_params* params, double* w_dev, double* m_dev,
                                   double* v_dev);
/* The same for P gathered FixedPointGradient payloads: skml_fixed_decode_sum_f32's walk with the update
 * of w / m / v in place of its (float)(scale * sum) store, so the gradient is the double the
 * reference's update(fpGrad.toAuto, weight) sees.  payloads_dev / P / stride / n / scale and the
 * header checks (read back first: magic, status with SKML_E_NAN, n, one num_bits, stride) are
 * skml_fixed_decode_sum_f32's; params, the state and their checks are skml_dense_decode_sum_step_*'s,
 * the payloads' range being [payloads_dev, payloads_dev + (P - 1) * stride + skml_fixed_payload_bytes(n,
 * num_bits)).  LIVE and AUTO as above (AUTO's count pass walks the payloads once more and
 * synchronises).  Timed under SKML_K_DECODE_SUM. */
int skml_fixed_decode_sum_step_f32(skml_ctx* ctx, const void* payloads_dev, int32_t P, size_t stride, int64_t n,
                                   double scale, const skml_opt_params* params, float* w_dev, float* m_dev,
                                   float* v_dev);
int skml_fixed_decode_sum_step_f64(skml_ctx* ctx, const void* payloads_dev, int32_t P, size_t stride, int64_t n,
                                   double scale, const skml_opt_params* params, double* w_dev, double* m_dev,
                                   double* v_dev);
/* The same update from a dense device array of n floats (g_fp64 = 0) or doubles, 16-byte aligned:
 * the output of skml_sparse_decode_sum_f64 or skml_fixed_decode_sum_f32, or an uncompressed
 * gradient.  Asynchronous unless AUTO. */
int skml_opt_step_f32(skml_ctx* ctx, const void* g_dev, int32_t g_fp64, int64_t n, double scale,
                      const skml_opt_params* params, float* w_dev, float* m_dev, float* v_dev);
int skml_opt_step_f64(skml_ctx* ctx, const void* g_dev, int32_t g_fp64, int64_t n, double scale,
                      const skml_opt_params* params, double* w_dev, double* m_dev, double* v_dev);
/* update(SparseDoubleGradient, ...) (Adam.scala:63-77, GradientDescent.scala:111-117): nnz int32 keys
 * and their values (floats, or doubles when vals_fp64) update w / m / v (dim values each) at the
 * keys.  Precondition, not verified: the keys are strictly increasing (SparseDoubleGradient's
 * invariant), so that no element has two owners; a key outside [0, dim) is skipped.  ALL updates
 * every key, LIVE those with fabs(g) > 1e-8; AUTO is refused (SKML_E_ARG): the caller that built
 * the key list has made toAuto's choice.  Asynchronous. */
int skml_opt_step_kv_f32(skml_ctx* ctx, const int32_t* keys_dev, const void* vals_dev, int32_t vals_fp64, int64_t nnz,
                         int64_t dim, double scale, const skml_opt_params* params, float* w_dev, float* m_dev,
                         float* v_dev);
int skml_opt_step_kv_f64(skml_ctx* ctx, const int32_t* keys_dev, const void* vals_dev, int32_t vals_fp64, int64_t nnz,
                         int64_t dim, double scale, const skml_opt_params* params, double* w_dev, double* m_dev,
                         double* v_dev);

/* ---- Mini-batch gradient: optimizer.miniBatchGradientDescent(weights, trainData, loss)
 * (ml/objective/GradientDescent.scala:23-87, ml/objective/Loss.scala:56-137) ----
 *
 * The data set lives on the device, caller-owned and read-only: its CSR (row_ptr[rows + 1], col[nnz],
 * val[nnz], label[rows]) and the same entries in (column, row) order (col_ptr[dim + 1], csc_row[nnz],
 * csc_val[nnz]).  Every pointer is 8-byte aligned; rows and dim fit a Java int.  Preconditions, not
 * verified (sketchml_amd/data.py verifies them): row_ptr and col_ptr ascend from 0 to nnz, the
 * columns of a row ascend strictly inside [0, dim), csc_row ascends inside a column.  The kernels
 * skip an entry whose column or batch position is out of range; they never read or write through it. */
typedef struct skml_glm_data {
    int64_t rows, dim, nnz;
    const int64_t* row_ptr;
    const int32_t* col;
    const double* val;
    const double* label;
    const int64_t* col_ptr;
    const int32_t* csc_row;
    const double* csc_val;
} skml_glm_data;
#define SKML_LOSS_L1_LOG 0
#define SKML_LOSS_L2_HINGE 1
#define SKML_LOSS_L2_LOG 2
#define SKML_LOSS_L2_SQUARE 3
#define SKML_REG_NONE 0
#define SKML_REG_L1 1
#define SKML_REG_L2 2
/* The loop of miniBatchGradientDescent over `batch` instances; instance j is row (row0 + j) mod rows
 * (DataSet.loopingRead).  All in double, without contraction:
 *   pre_j  = Maths.dot(w, x_j): from +0.0, w[col] * val (rounded) added in stored order
 *   loss_j = loss.loss(pre_j, y_j),  coef_j = -1.0 * loss.grad(pre_j, y_j), branches as written
 *            (exp and log are the device's, within 1 ulp as Java's: not bit-pinned)
 *   grad_out[k] = from +0.0, val * coef_j (rounded) added for j = 0 .. batch - 1 in that order; +0.0
 *            for a feature without an entry in the batch.  No atomics, no tree.  Unscaled.
 *   *nnz_out = #{k : |grad_out[k]| > 1e-8} (toAuto's count),  *obj_loss_out = sum of loss_j by a
 *            fixed-shape reduction (256 strided sequential sums, then a tree): deterministic, not the
 *            reference's sequential sum; loss_out has the terms.
 * w_dev: dim doubles (_f64) or floats (_f32, widened exactly).  pre_out, loss_out (batch doubles each)
 * may be NULL; coef_out (batch doubles) may be NULL, a context buffer then stands in.  grad_out: dim
 * doubles.  Synchronises once, for the two scalars, through pinned staging.  SKML_E_ARG, with nothing
 * written: a NULL or misaligned pointer, row0 outside [0, rows), batch outside [1, rows], rows or dim
 * outside [1, 2^31 - 1], nnz < 0, an unknown loss, grad_out overlapping an input or another output.
 * Timed as SKML_K_GLM_PREDICT and SKML_K_GLM_PLUS_BY. */
int skml_glm_gradient_f64(skml_ctx* ctx, const skml_glm_data* data, int64_t row0, int64_t batch, int32_t loss_kind,
                          const double* w_dev, double* pre_out, double* coef_out, double* loss_out, double* grad_out,
                          int64_t* nnz_out, double* obj_loss_out);
int skml_glm_gradient_f32(skml_ctx* ctx, const skml_glm_data* data, int64_t row0, int64_t batch, int32_t loss_kind,
                          const float* w_dev, double* pre_out, double* coef_out, double* loss_out, double* grad_out,
                          int64_t* nnz_out, double* obj_loss_out);
/* grad.timesBy(times), then the regulariser (GradientDescent.scala:53-87), in place, on the form toAuto
 * chose.  SKML_REG_L1 is l1Reg(grad, 0, reg_param) as written: v in [0, theta] -> Math.max(v - 0, 0),
 * v < 0 && v >= -theta -> Math.min(v - 0, 0) (Java's max / min: -0.0 becomes +0.0).  SKML_REG_L2 is
 * v += w[k] * reg_param (product rounded, then added); on keys and values it touches the kept keys
 * only, as the reference does.  w_dev: dim doubles, or floats when w_fp32; may be NULL unless L2.
 * keys_dev: strictly increasing (not verified; a key outside [0, dim) keeps timesBy and skips L2).
 * Asynchronous.  SKML_E_ARG: NULL or misaligned pointers, dim outside [1, 2^31 - 1], nnz outside
 * [0, dim], an unknown regulariser, values overlapping w or the keys.  Timed as SKML_K_GLM_FINISH. */
int skml_glm_finish_dense_f64(skml_ctx* ctx, double* g_dev, int64_t dim, double times, int32_t reg_kind,
                              double reg_param, const void* w_dev, int32_t w_fp32);
int skml_glm_finish_kv_f64(skml_ctx* ctx, const int32_t* keys_dev, double* vals_dev, int64_t nnz, int64_t dim,
                           double times, int32_t reg_kind, double reg_param, const void* w_dev, int32_t w_fp32);

/* ---- Validation pass: ValidationUtil.calLossPrecision / calLossAucPrecision
 * (ml/util/ValidationUtil.scala:12-93, sketch/util/Sort.java:168-259) ----
 *
 * For every instance i of the data set, in order, all in double without contraction:
 *   pre_i  = Maths.dot(w, x_i), the bits of skml_glm_gradient_*'s pre
 *   z      = pre_i * label_i (one rounded product): z > 0 -> truePos if pre_i > 0 else trueNeg;
 *            z < 0 -> falsePos if pre_i > 0 else falseNeg; z == 0 (an underflow, a zero label, an
 *            empty row) or NaN -> no counter moves
 *   loss_i = loss.loss(pre_i, label_i)
 *   loss   = ((0.0 + loss_0) + loss_1) + ..., one rounded add after the other: the reference's bits
 *            given the loss_i.  With SKML_VALID_TREE_SUM the fixed-shape sum of skml_glm_gradient_*'s
 *            objLoss instead (deterministic and faster, not the reference's order).
 * With SKML_VALID_AUC also the sort of (score, label) ascending by score and
 *   pos = #{label == 1.0} (M),  neg = num - pos (N),
 *   rank_sum = the sum of the 0-based sorted positions that hold a label == 1.0 (sigma), an exact integer;
 * the caller forms auc = (sigma - (M + 1) * M / 2) / M / N as the reference writes it.
 *
 * The order of the sort -- the tie rule.  The reference sorts with a quicksort whose comparator calls two
 * scores equal when they differ by less than 1e-11; that relation is not transitive and the order
 * inside a group of near-equal scores depends on the pivots (its output need not even ascend).  Here
 * scores are ordered by their IEEE total-order key: -0.0 before +0.0, infinities are ordinary values,
 * and equal scores keep instance order (a stable sort).  rank_sum equals the reference's whenever all
 * gaps between distinct sorted scores exceed 1e-11 and no score repeats; otherwise it is this rule's.
 * A NaN score is counted in nan_scores and makes the AUC undefined (the caller reports NaN).
 * The reference accumulates sigma in double, exact while n (n - 1) / 2 < 2^53 (n <= 2^27); above that
 * the integer rank_sum converted once is the documented deviation. */
#define SKML_VALID_AUC 1
#define SKML_VALID_TREE_SUM 2
typedef struct skml_valid_result {
    double loss;        /* validLoss: the sum, not the mean */
    int64_t true_pos, true_neg, false_pos, false_neg;
    int64_t num;        /* validNum = rows */
    int64_t pos, neg;   /* M, N; 0 without SKML_VALID_AUC */
    uint64_t rank_sum;  /* sigma; 0 without SKML_VALID_AUC */
    int64_t nan_scores; /* the NaN predictions */
} skml_valid_result;
/* data: as skml_glm_gradient_*, except that col_ptr, csc_row and csc_val are not read and may be NULL.
 * w_dev: dim doubles (_f64) or floats (_f32, widened exactly).  pre_out, loss_out (rows doubles each)
 * may be NULL; the context's buffer then stands in.  One read-back through pinned staging after one
 * synchronisation.  SKML_E_ARG, with nothing written: a NULL or misaligned pointer, rows or dim
 * outside [1, 2^31 - 1], nnz < 0, an unknown loss or flag bit, an output overlapping an input or the
 * other output.  Timed as SKML_K_GLM_VALID, SKML_K_SEQ_SUM, SKML_K_VALID_SORT, SKML_K_VALID_RANK. */
int skml_glm_validate_f64(skml_ctx* ctx, const skml_glm_data* data, int32_t loss_kind, const double* w_dev, int32_t flags,
                          double* pre_out, double* loss_out, skml_valid_result* out);
int skml_glm_validate_f32(skml_ctx* ctx, const skml_glm_data* data, int32_t loss_kind, const float* w_dev, int32_t flags,
                          double* pre_out, double* loss_out, skml_valid_result* out);
/* The AUC stage alone over n scores and labels on the device (n in [1, 2^31 - 1], 8-byte aligned):
 * *pos, *neg, *rank_sum and *nan_scores as above; order_out (optional, n int32 on the device, 4-byte
 * aligned, not overlapping the inputs) receives the sorted permutation: order_out[p] = the instance at
 * sorted position p.  Synchronises once.  skml_glm_validate_* runs the same code. */
int skml_auc_rank_sum(skml_ctx* ctx, const double* scores_dev, const double* labels_dev, int64_t n, int32_t* order_out,
                      int64_t* pos, int64_t* neg, uint64_t* rank_sum, int64_t* nan_scores);
/* *sum = ((0.0 + x[0]) + x[1]) + ... + x[n - 1], one rounded add after the other (the reference's
 * `objLoss += ...` and `validLoss += ...`): n in [1, 2^31 - 1] doubles on the device, 8-byte aligned.
 * A chain of n dependent additions run by one wave.  Synchronises once. */
int skml_glm_seq_sum(skml_ctx* ctx, const double* x_dev, int64_t n, double* sum);

/* ---- Host memory in and out (the JNI path: a JVM float[] on its way to a socket) ---- */

/* Pinned host memory (hipHostMalloc): a Java direct ByteBuffer over it (JNI NewDirectByteBuffer)
 * lets the host entry points DMA the gradient without the staging copy. */
int skml_host_alloc(size_t bytes, void** out);
int skml_host_free(void* p);

/* DenseVectorCompressor.compressDense (sample/DenseVectorCompressor.java:34-41) from host memory:
 * x_host (pageable or pinned) -> device -> QuantileQuantizer.quantize (as skml_dense_encode_f32)
 * -> the payload (header, splits, packed codes) back in payload_host.  Pageable input is staged
 * through library-owned pinned buffers, the host copy of one piece overlapping the DMA of the
 * previous one.  payload_host NULL: *written = an upper bound of the payload size.  Otherwise
 * *written = the bytes written (codes_offset + ceil(n * code_bits / 8)).  params->parallelism > 1
 * selects parallelQuantize (QuantileQuantizer.java:53-92) with that many slices, as on the sparse
 * path (params->dedup then applies as given); params->quant_type = SKML_UNIFORM selects
 * UniformQuantizer instead (skml_dense_encode_uniform_f32/_f64).  Synchronising. */
int skml_dense_encode_host_f32(skml_ctx* ctx, const float* x_host, int64_t n, const skml_params* params,
                               void* payload_host, size_t payload_cap, size_t* written);
/* The reference's own double[] input (QuantileQuantizer.quantize(double[]), no fp32 rounding):
 * as skml_dense_encode_host_f32 over skml_dense_encode_f64. */
int skml_dense_encode_host_f64(skml_ctx* ctx, const double* x_host, int64_t n, const skml_params* params,
                               void* payload_host, size_t payload_cap, size_t* written);
/* DenseVectorCompressor.decompressDense (DenseVectorCompressor.java:84-91) from a host payload
 * (as written above) into a host float[n] / double[n].  Synchronising. */
int skml_dense_decode_host_f32(skml_ctx* ctx, const void* payload_host, size_t payload_len, float* out_host,
                               int64_t n);
int skml_dense_decode_host_f64(skml_ctx* ctx, const void* payload_host, size_t payload_len, double* out_host,
                               int64_t n);
/* Host payloads without a device (pure host code):
 *   skml_dense_info_host     Quantizer.getBinNum/getSplits/getZeroIdx/getMin/getMax/getN
 *   skml_dense_bins_host     Quantizer.getBins() (Quantizer.java:163-165): unpacked int32 bins
 *   skml_dense_times_by_host Quantizer.timesBy (Quantizer.java:119-124), in place */
int skml_dense_info_host(const void* payload_host, size_t payload_len, skml_dense_header* hdr, double* splits_host,
                         int32_t splits_cap);
int skml_dense_bins_host(const void* payload_host, size_t payload_len, int32_t* bins_host, int64_t n);
int skml_dense_times_by_host(void* payload_host, size_t payload_len, double x);

/* ---- Sparse path: SketchGradient.fromSparse / SparseVectorCompressor ---- */

typedef struct skml_sparse skml_sparse; /* library-owned; free with skml_sparse_free */

/* DenseDoubleGradient.countNNZ + toSparse (ml/gradient/DenseDoubleGradient.scala:64-89):
 * keep |x| > 1e-8 with ascending int32 keys.  keys_dev / vals_dev need dim capacity.
 * Synchronising (returns nnz through *nnz_out). */
int skml_sparse_compact_f32(skml_ctx* ctx, const float* dense_dev, int64_t dim, int32_t* keys_dev,
                            float* vals_dev, int64_t* nnz_out);
/* The same over the reference's own double[] (DenseDoubleGradient.values): |x| > 1e-8 in double. */
int skml_sparse_compact_f64(skml_ctx* ctx, const double* dense_dev, int64_t dim, int32_t* keys_dev,
                            double* vals_dev, int64_t* nnz_out);
/* bf16 / fp16 gradients (no reference call: Java has no 16-bit float), the 16 bits travelling as
 * uint16_t as in the dense entries.  Widening to float is exact for every bit pattern, so these are
 * defined as skml_sparse_compact_f32 of the widened buffer: the same ascending keys and, bit for
 * bit, the same fp32 values (|x| > 1e-8 on the widened value, NaN dropped, +-inf kept).  The kernels
 * read the 16-bit buffer itself; no fp32 copy of it exists.  dense_dev needs only 2-byte alignment
 * (16-byte aligned buffers take 16-byte loads).  Synchronising. */
int skml_sparse_compact_bf16(skml_ctx* ctx, const uint16_t* dense_dev, int64_t dim, int32_t* keys_dev,
                             float* vals_dev, int64_t* nnz_out);
int skml_sparse_compact_f16(skml_ctx* ctx, const uint16_t* dense_dev, int64_t dim, int32_t* keys_dev,
                            float* vals_dev, int64_t* nnz_out);

/* SparseVectorCompressor.compressSparse (sample/SparseVectorCompressor.java:52-67):
 * QuantileQuantizer.quantize(values) then GroupedMinMaxSketch.create(keys, bins)
 * (frequency/GroupedMinMaxSketch.java:51-70): group partition, MinMax insert, DeltaAdaptive key
 * encoding (binary/DeltaAdaptiveEncoder.java:54-112).  Synchronising. */
int skml_sparse_encode_kv_f32(skml_ctx* ctx, const int32_t* keys_dev, const float* vals_dev,
                              int64_t nnz, const skml_params* params, skml_sparse** out);
/* SparseVectorCompressor.compressSparse(int[], double[]) / SketchGradient.fromSparse on the
 * reference's own double values (SketchGradient.scala:35-48, SparseVectorCompressor.java:52-67):
 * the values' quantizer sketches and bins the doubles themselves (skml_dense_encode_f64, or the
 * uniform / parallel f64 forms), so split samples and bins equal the Java double[] path even for
 * values that are not fp32-representable.  Synchronising. */
int skml_sparse_encode_kv_f64(skml_ctx* ctx, const int32_t* keys_dev, const double* vals_dev,
                              int64_t nnz, const skml_params* params, skml_sparse** out);
/* SketchGradient.fromSparse after toAuto's compaction: compact + encode_kv. */
int skml_sparse_encode_f32(skml_ctx* ctx, const float* dense_dev, int64_t dim,
                           const skml_params* params, skml_sparse** out);
/* skml_sparse_encode_f32 of the widened bf16 / fp16 buffer (the payload is byte for byte the
 * same): the 16-bit compaction above, then the fp32 key/value encode. */
int skml_sparse_encode_bf16(skml_ctx* ctx, const uint16_t* dense_dev, int64_t dim,
                            const skml_params* params, skml_sparse** out);
int skml_sparse_encode_f16(skml_ctx* ctx, const uint16_t* dense_dev, int64_t dim,
                           const skml_params* params, skml_sparse** out);
/* The ml path itself: DenseDoubleGradient.toAuto / toSparse (DenseDoubleGradient.scala:64-95) of a
 * double[] gradient, then SketchGradient.fromSparse on the double values. */
int skml_sparse_encode_f64(skml_ctx* ctx, const double* dense_dev, int64_t dim,
                           const skml_params* params, skml_sparse** out);
/* GroupedMinMaxSketch.restore + Sort.merge (GroupedMinMaxSketch.java:123-146,
 * util/Sort.java:362-379) and SparseVectorCompressor.decompressSparse's value lookup
 * (SparseVectorCompressor.java:118-126).  keys/vals device buffers of nnz capacity.  A restored
 * bin outside quantValues returns SKML_E_ARG (Java: ArrayIndexOutOfBoundsException). */
int skml_sparse_decode_f32(skml_ctx* ctx, const skml_sparse* s, int32_t* keys_dev,
                           float* vals_dev);
/* The same with the values as the reference's doubles (quantValues[bin], no fp32 rounding). */
int skml_sparse_decode_f64(skml_ctx* ctx, const skml_sparse* s, int32_t* keys_dev,
                           double* vals_dev);
int skml_sparse_nnz(const skml_sparse* s, int64_t* nnz);
/* SparseVectorCompressor.timesBy (sample/SparseVectorCompressor.java:128-134): scales the
 * double quantValues table in place (the scaled values are what decode returns, as fp32). */
int skml_sparse_times_by(skml_sparse* s, double x);
/* quantValues (Quantizer.getValues times every timesBy factor): min(bin_num, cap) doubles. */
int skml_sparse_values(const skml_sparse* s, double* out, int32_t cap);
/* Header of the quantizer inside the sparse payload (bins, zero index, splits). */
int skml_sparse_quant_info(const skml_sparse* s, skml_dense_header* hdr, double* splits_host,
                           int32_t splits_cap);
/* Per-group view for parity checks: size, colNum, hash ids, DeltaAdaptive choice and bit
 * lengths; tables/words are copied to host buffers when non-NULL. */
typedef struct skml_sparse_group {
    int32_t size;
    int32_t col_num;
    int32_t hash_ids[8];
    int32_t num_intervals;
    int32_t flag_kind;
    int64_t n_flag_bits;
    int64_t n_delta_bits;
} skml_sparse_group;
int skml_sparse_group_info(skml_ctx* ctx, const skml_sparse* s, int32_t g, skml_sparse_group* info,
                           int32_t* table_host, uint64_t* flag_words_host,
                           uint64_t* delta_words_host);
/* GroupedMinMaxSketch.writeObject-ordered field stream (GroupedMinMaxSketch.java:148-158),
 * without Java object-stream framing; see DESIGN.md for the exact layout. */
int skml_sparse_serialize(skml_ctx* ctx, const skml_sparse* s, uint8_t* buf_host, size_t cap,
                          size_t* written);
/* GroupedMinMaxSketch.readObject (GroupedMinMaxSketch.java:161-172) with its MinMaxSketch,
 * HuffmanEncoder and DeltaAdaptiveEncoder readObjects: parses the stream skml_sparse_serialize
 * writes and rebuilds a device payload (the Huffman tables are decoded on the device).
 * quant_values (SparseVectorCompressor.quantValues, may be NULL with nvalues 0) enable
 * skml_sparse_decode_f32; without them only skml_sparse_restore_bins applies.  Synchronising. */
int skml_sparse_deserialize(skml_ctx* ctx, const uint8_t* buf_host, size_t len, const double* quant_values,
                            int32_t nvalues, skml_sparse** out);
/* GroupedMinMaxSketch.restore (GroupedMinMaxSketch.java:123-146): keys in Sort.merge order and
 * their int32 bins, on the device.  Synchronising. */
int skml_sparse_restore_bins(skml_ctx* ctx, const skml_sparse* s, int32_t* keys_dev, int32_t* bins_dev);
int skml_sparse_free(skml_sparse* s);

/* ---- Sparse payloads between GPUs (the ml path's exchange) ----
 * A payload exported as one contiguous, relocatable device blob: a 256-byte header (magic "SKSP",
 * section offsets), the group table, the quantizer header + splits, quantValues (doubles, timesBy
 * applied), the MinMaxSketch tables and the two DeltaAdaptive word streams.  It is what the RCCL
 * all-gather moves (sizes first, then the blobs padded to the largest: skml_allgather), with no
 * host round trip.  The blob replaces the Java-serialised SketchGradient that Spark's collect /
 * broadcast ship (ml/algorithm/GeneralizedLinearModel.scala:145-156). */
int skml_sparse_export_bytes(const skml_sparse* s, size_t* bytes);
/* dst_dev: 256-byte aligned device memory of at least export_bytes.  Asynchronous. */
int skml_sparse_export(skml_ctx* ctx, const skml_sparse* s, void* dst_dev, size_t cap);
/* A library-owned copy of the blob at blob_dev (len bytes available there); the blob is checked
 * (magic, section offsets, group-table invariants) before anything runs on it.  Synchronising. */
int skml_sparse_import(skml_ctx* ctx, const void* blob_dev, size_t len, skml_sparse** out);
/* Gradient.sum (ml/gradient/Gradient.scala:44-49) of P blobs laid out `stride` bytes apart (the
 * all-gather output): out[0, dim) = +0.0, then payload by payload, in order,
 * DenseDoubleGradient.plusBy(SketchGradient.toAuto) (DenseDoubleGradient.scala:38) -- every restored
 * key adds quantValues[bin] in double (the live values only, plus the dense form's +0.0, when the
 * payload's live count exceeds dim * 2 / 3: SparseDoubleGradient.toAuto); then out *= scale when
 * scale != 1 (the 1/P average, one double multiply per element).  A key outside [0, dim) fails
 * with SKML_E_ARG (SparseDoubleGradient's bound check), and so do a key repeated across one
 * payload's groups (its constructor requires strictly increasing keys) and a payload that restores
 * no keys (its constructor reads indices.head).  Synchronising. */
int skml_sparse_decode_sum_f64(skml_ctx* ctx, const void* blobs_dev, int32_t P, size_t stride, int64_t dim,
                               double scale, double* out_dev);
/* The same sum returned as float, bf16 or fp16 (the 16 bits as uint16_t): exactly
 * skml_sparse_decode_sum_f64's double sum, x scale included, then cast to float (round to nearest
 * even) and, for the 16-bit types, that float rounded to nearest even again -- the definition of
 * skml_dense_decode_sum_bf16.  No partial sum passes through the narrow type: when the sum takes
 * more than one tile launch (more than 8 payloads, or more than one scratch batch) it is kept in a
 * dim-double accumulator of the context's scratch and only the last launch writes out_dev.  out_dev
 * needs only its element's alignment.  Every refusal of the f64 entry is refused the same way
 * (out_dev's contents are unspecified on error).  Synchronising. */
int skml_sparse_decode_sum_f32(skml_ctx* ctx, const void* blobs_dev, int32_t P, size_t stride, int64_t dim,
                               double scale, float* out_dev);
int skml_sparse_decode_sum_bf16(skml_ctx* ctx, const void* blobs_dev, int32_t P, size_t stride, int64_t dim,
                                double scale, uint16_t* out_dev);
int skml_sparse_decode_sum_f16(skml_ctx* ctx, const void* blobs_dev, int32_t P, size_t stride, int64_t dim,
                               double scale, uint16_t* out_dev);
/* Host-memory forms of encode_kv / decode (int[] keys and float[] values in JVM arrays). */
int skml_sparse_encode_kv_host_f32(skml_ctx* ctx, const int32_t* keys_host, const float* vals_host, int64_t nnz,
                                   const skml_params* params, skml_sparse** out);
/* int[] keys and double[] values (SparseVectorCompressor.compressSparse(int[], double[])). */
int skml_sparse_encode_kv_host_f64(skml_ctx* ctx, const int32_t* keys_host, const double* vals_host, int64_t nnz,
                                   const skml_params* params, skml_sparse** out);
int skml_sparse_decode_host_f32(skml_ctx* ctx, const skml_sparse* s, int32_t* keys_host, float* vals_host);
/* keys into an int[] and quantValues[bin] into a double[] (SparseVectorCompressor.decompressSparse). */
int skml_sparse_decode_host_f64(skml_ctx* ctx, const skml_sparse* s, int32_t* keys_host, double* vals_host);

/* ---- DeltaAdaptiveEncoder as a standalone BinaryEncoder (base/BinaryEncoder.java:6-11) ---- */
/* encode(int[]): keys strictly increasing (keys[0] >= 0).  Outputs the choice and the two
 * BitSet word streams (BitSet.toLongArray layout).  Synchronising. */
int skml_delta_encode(skml_ctx* ctx, const int32_t* keys_dev, int64_t n, int32_t* num_intervals,
                      int32_t* flag_kind, int64_t* n_flag_bits, int64_t* n_delta_bits,
                      uint64_t* flag_words_dev, uint64_t* delta_words_dev, int64_t words_cap);
/* decode(): keys_dev receives n keys.  Asynchronous. */
int skml_delta_decode(skml_ctx* ctx, int64_t n, int32_t num_intervals, int32_t flag_kind,
                      const uint64_t* flag_words_dev, int64_t n_flag_words,
                      const uint64_t* delta_words_dev, int64_t n_delta_words, int32_t* keys_dev);

/* Host-memory forms (a JVM int[] in, BitSet.toLongArray long[]s out, and back): words_cap is the
 * capacity of each word array; NULL word arrays query the bit counts only. */
int skml_delta_encode_host(skml_ctx* ctx, const int32_t* keys_host, int64_t n, int32_t* num_intervals,
                           int32_t* flag_kind, int64_t* n_flag_bits, int64_t* n_delta_bits, uint64_t* flag_words_host,
                           uint64_t* delta_words_host, int64_t words_cap);
int skml_delta_decode_host(skml_ctx* ctx, int64_t n, int32_t num_intervals, int32_t flag_kind,
                           const uint64_t* flag_words_host, int64_t n_flag_words, const uint64_t* delta_words_host,
                           int64_t n_delta_words, int32_t* keys_host);

/* ---- Multi-GPU: RCCL all-gather of payloads over xGMI ---- */
typedef struct skml_comm skml_comm;
#define SKML_UNIQUE_ID_BYTES 128
int skml_comm_unique_id(uint8_t id_out[SKML_UNIQUE_ID_BYTES]);
int skml_comm_init_rank(skml_ctx* ctx, const uint8_t id[SKML_UNIQUE_ID_BYTES], int32_t nranks,
                        int32_t rank, skml_comm** out);
int skml_comm_destroy(skml_comm* comm);
/* ncclAllGather of `bytes` from each rank's payload into all_dev (nranks * bytes). Async. */
int skml_allgather(skml_ctx* ctx, skml_comm* comm, const void* payload_dev, size_t bytes,
                   void* all_dev);

#ifdef __cplusplus
}
#endif
#endif /* SKML_H */
