// skml_valid.hip -- the AUC stage of the validation pass (ml/util/ValidationUtil.scala:43-93) on the
// device: the scores sorted ascending with their instance index as payload, then the rank sum.
//   k_valid_keys       score -> order-preserving 64-bit key (zip_key64), payload = instance index, NaN count
//   k_valid_scatter    one LSD pass of 8-bit digits: k_zip_scatter's stable scheme with the payload carried
//                      alongside the key; the tile histogram and the scan are skml_zip.hip's own launchers
//   k_valid_rank_sum   sigma = sum of the 0-based positions p with label[idx[p]] == 1.0, M = their number
// The order is the keys': -0.0 before +0.0, infinities ordinary values, equal keys in instance order (an
// LSD sort of stable passes).  Integer atomics only: the results do not depend on the order.
#include <algorithm>

#include "skml_device.hpp"
#include "skml_valid.hpp"

namespace skml {

__global__ __launch_bounds__(kZsThreads) void k_valid_keys(const double* __restrict__ score, int64_t n,
                                                           uint64_t* __restrict__ keys, uint32_t* __restrict__ idx,
                                                           unsigned long long* __restrict__ nan_count) {
    // the trip count is the wave's: the ballot needs every lane
    const int lane = threadIdx.x & 63;
    for (int64_t base = (int64_t)blockIdx.x * kZsThreads + (threadIdx.x - lane); base < n;
         base += (int64_t)gridDim.x * kZsThreads) {
        const int64_t i = base + lane;
        bool nan = false;
        if (i < n) {
            const double v = score[i];
            nan = v != v;
            keys[i] = zip_key64(v);
            idx[i] = (uint32_t)i;
        }
        const unsigned long long m = __ballot(nan);
        if (m != 0 && lane == 0) atomicAdd(nan_count, (unsigned long long)__popcll(m));
    }
}

// Stable scatter of workgroup b's tile (the tile k_zip_hist counted) to offs[d * nblocks + b] on, keys
// and payloads together, kZsRows * kZsThreads keys at a time in input order.  A key's rank among its
// wave's equal digits of its row comes from eight ballots; the (row, wave) counts of a digit are turned
// into offsets by that digit's thread (valid_slot_offsets), which also moves the digit's base on.  Two
// workgroup barriers per step.  Every position is below n because the offsets are the exclusive scan of
// the counts of these same tiles; the store checks it all the same.
__global__ __launch_bounds__(kZsThreads) void k_valid_scatter(const uint64_t* __restrict__ in, const uint32_t* __restrict__ pin,
                                                              uint64_t* __restrict__ out, uint32_t* __restrict__ pout,
                                                              int64_t n, int pass, const uint32_t* __restrict__ offs,
                                                              int nblocks) {
    static_assert(kZipDigits == kZsThreads, "a thread per digit");
    __shared__ uint32_t s_base[kZipDigits];
    __shared__ uint32_t s_cnt[kValidSlots][kZipDigits];
    __shared__ uint32_t s_off[kValidSlots][kZipDigits];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    s_base[tid] = offs[(size_t)tid * nblocks + blockIdx.x];
    for (int q = 0; q < kValidSlots; q++) s_cnt[q][tid] = 0u;
    __syncthreads();
    int64_t b0, e;
    valid_tile(blockIdx.x, n, &b0, &e);
    for (int64_t s0 = b0; s0 < e; s0 += kZsRows * kZsThreads) {
        uint64_t key[kZsRows];
        uint32_t pay[kZsRows];
        int d[kZsRows], rank[kZsRows];
        bool valid[kZsRows];
#pragma unroll
        for (int j = 0; j < kZsRows; j++) {
            const int64_t i = valid_step_index(s0, j, tid);
            valid[j] = i < e;
            key[j] = valid[j] ? in[i] : 0ull;
            pay[j] = valid[j] ? pin[i] : 0u;
        }
#pragma unroll
        for (int j = 0; j < kZsRows; j++) {
            d[j] = valid[j] ? zip_digit(key[j], pass) : 0;
            uint64_t peers = __ballot(valid[j]);
#pragma unroll
            for (int b = 0; b < kZipDigitBits; b++) {
                const bool bit = (d[j] >> b) & 1;
                const uint64_t m = __ballot(valid[j] && bit);
                peers &= bit ? m : ~m;
            }
            rank[j] = __popcll(peers & ((1ull << lane) - 1ull));
            if (valid[j] && rank[j] == 0) s_cnt[valid_slot(j, wave)][d[j]] = (uint32_t)__popcll(peers);
        }
        __syncthreads();
        s_base[tid] = valid_slot_offsets(s_base[tid], &s_cnt[0][tid], &s_off[0][tid], kZipDigits);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kZsRows; j++)
            if (valid[j]) {
                const uint32_t pos = s_off[valid_slot(j, wave)][d[j]] + (uint32_t)rank[j];
                if ((int64_t)pos < n) {
                    out[pos] = key[j];
                    pout[pos] = pay[j];
                }
            }
        // the next step writes s_cnt (cleared above) before its first barrier and s_off only after it
    }
}

// res[0] += sigma, res[1] += M over the sorted positions [0, n): a lane's own sums, a wave reduction,
// one LDS add per wave, one pair of 64-bit integer atomics per workgroup.  Exact for every n < 2^32:
// sigma < 2^63.  order (optional): the permutation as int32.
__global__ __launch_bounds__(256) void k_valid_rank_sum(const uint32_t* __restrict__ idx, const double* __restrict__ label,
                                                        int64_t n, int32_t* __restrict__ order,
                                                        unsigned long long* __restrict__ res) {
    __shared__ unsigned long long s_res[2];
    unsigned long long sigma = 0, m = 0;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
        const uint32_t i = idx[p];
        if (order) order[p] = (int32_t)i;
        if ((int64_t)i < n && label[i] == 1.0) {
            sigma += (unsigned long long)p;
            m += 1;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sigma += __shfl_xor(sigma, o, 64);
        m += __shfl_xor(m, o, 64);
    }
    if (threadIdx.x < 2) s_res[threadIdx.x] = 0;
    __syncthreads();
    if ((threadIdx.x & 63) == 0 && m) {
        atomicAdd(&s_res[0], sigma);
        atomicAdd(&s_res[1], m);
    }
    __syncthreads();
    if (threadIdx.x < 2 && s_res[threadIdx.x]) atomicAdd(&res[threadIdx.x], s_res[threadIdx.x]);
}

static int valid_tiles(int64_t n) { return (int)((n + kZsTile - 1) / kZsTile); }

size_t valid_auc_layout(int64_t n, ValidAucScratch* out, char* base) {
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t o = off;
        off = align_up(off + bytes, 256);
        return base ? (void*)(base + o) : nullptr;
    };
    const size_t nn = (size_t)std::max<int64_t>(n, 1);
    const int64_t cells = (int64_t)kZipDigits * valid_tiles((int64_t)nn);
    ValidAucScratch s;
    s.keys_a = (uint64_t*)take(8 * nn);
    s.keys_b = (uint64_t*)take(8 * nn);
    s.idx_a = (uint32_t*)take(4 * nn);
    s.idx_b = (uint32_t*)take(4 * nn);
    s.hist = (uint32_t*)take(4 * (size_t)cells);
    s.hist_tmp = (uint32_t*)take(4 * zip_scan_u32_tmp(cells));
    if (out) *out = s;
    return off;
}

hipError_t launch_valid_keys(hipStream_t st, const double* score, int64_t n, const ValidAucScratch& s,
                             unsigned long long* nan_count) {
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((n + kZsThreads - 1) / kZsThreads, 4096));
    hipLaunchKernelGGL(k_valid_keys, dim3(grid), dim3(kZsThreads), 0, st, score, n, s.keys_a, s.idx_a, nan_count);
    return hipGetLastError();
}

hipError_t launch_valid_sort_pass(hipStream_t st, int64_t n, int pass, const ValidAucScratch& s) {
    const int nblocks = valid_tiles(n);
    const bool odd = pass & 1;  // an even number of passes: the sorted keys end in keys_a / idx_a
    const uint64_t* ka = odd ? s.keys_b : s.keys_a;
    uint64_t* kb = odd ? s.keys_a : s.keys_b;
    const uint32_t* ia = odd ? s.idx_b : s.idx_a;
    uint32_t* ib = odd ? s.idx_a : s.idx_b;
    hipError_t e = launch_zip_hist64(st, ka, n, pass, s.hist, nblocks);
    if (e != hipSuccess) return e;
    if ((e = zip_scan_u32(st, s.hist, (int64_t)kZipDigits * nblocks, s.hist_tmp)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_valid_scatter, dim3(nblocks), dim3(kZsThreads), 0, st, ka, ia, kb, ib, n, pass, s.hist, nblocks);
    return hipGetLastError();
}

hipError_t launch_valid_rank_sum(hipStream_t st, const ValidAucScratch& s, const double* label, int64_t n, int32_t* order,
                                 unsigned long long* res) {
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 2048));
    hipLaunchKernelGGL(k_valid_rank_sum, dim3(grid), dim3(256), 0, st, s.idx_a, label, n, order, res);
    return hipGetLastError();
}

}  // namespace skml
