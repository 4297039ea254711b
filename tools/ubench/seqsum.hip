// Probe (gfx950): what bounds k_glm_seq_sum (skml_glm.hip), the sum of n doubles in index order by one
// wave?  The same staging through LDS with every lane adding (mode 0) and with lane 0 alone adding
// (mode 1), 2^18 values, 20 launches per window.  Prints ms per run and ns per element and checks the
// bits against the host's forward sum.  Measured on an MI355X: 7.50 ns per element with every lane,
// 7.75 ns with one: the time is the dependent v_add_f64 itself, not the width of the wave
// (DESIGN.md section 4 "Validation").
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -o seqsum seqsum.hip
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>
#include <cmath>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::printf("%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

template <int MODE>
__global__ __launch_bounds__(64) void k_sum(const double* __restrict__ x, int64_t n, double* __restrict__ out) {
    __shared__ double slots[256];
    const int lane = threadIdx.x;
    double acc = 0.0;
    double nxt[4];
    for (int u = 0; u < 4; u++) { const int64_t i = u * 64 + lane; nxt[u] = i < n ? x[i] : 0.0; }
    for (int64_t b = 0; b < n; b += 256) {
        for (int u = 0; u < 4; u++) slots[u * 64 + lane] = nxt[u];
        if (b + 256 < n)
            for (int u = 0; u < 4; u++) { const int64_t i = b + 256 + u * 64 + lane; nxt[u] = i < n ? x[i] : 0.0; }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const int64_t rem = n - b;
        const int cnt = rem < 256 ? (int)rem : 256;
        if (MODE == 0 || lane == 0) {
            if (cnt == 256) {
#pragma unroll
                for (int i = 0; i < 256; i++) acc += slots[i];
            } else {
                for (int i = 0; i < cnt; i++) acc += slots[i];
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    if (lane == 0) *out = acc;
}

int main() {
    const int64_t n = 1 << 18;
    std::vector<double> h(n);
    uint64_t s = 88172645463325252ull;
    for (auto& v : h) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; v = std::ldexp((double)(int64_t)(s >> 11) / 9007199254740992.0 - 0.5, (int)(s % 41) - 20); }
    double fwd = 0.0;
    for (double v : h) fwd += v;
    double *d, *o;
    CK(hipMalloc(&d, n * 8));
    CK(hipMalloc(&o, 16));
    hipStream_t st;
    CK(hipStreamCreate(&st));
    CK(hipMemcpyAsync(d, h.data(), n * 8, hipMemcpyHostToDevice, st));
    hipEvent_t a, b;
    CK(hipEventCreate(&a));
    CK(hipEventCreate(&b));
    for (int mode = 0; mode < 2; mode++) {
        for (int rep = 0; rep < 3; rep++) {
            for (int w = 0; w < 5; w++) {
                if (mode == 0) hipLaunchKernelGGL(k_sum<0>, dim3(1), dim3(64), 0, st, d, n, o);
                else hipLaunchKernelGGL(k_sum<1>, dim3(1), dim3(64), 0, st, d, n, o);
            }
            CK(hipEventRecord(a, st));
            for (int w = 0; w < 20; w++) {
                if (mode == 0) hipLaunchKernelGGL(k_sum<0>, dim3(1), dim3(64), 0, st, d, n, o);
                else hipLaunchKernelGGL(k_sum<1>, dim3(1), dim3(64), 0, st, d, n, o);
            }
            CK(hipEventRecord(b, st));
            CK(hipEventSynchronize(b));
            float ms = 0;
            CK(hipEventElapsedTime(&ms, a, b));
            double got = 0;
            CK(hipMemcpyAsync(&got, o, 8, hipMemcpyDeviceToHost, st));
            CK(hipStreamSynchronize(st));
            std::printf("mode %d (%s): %.4f ms per run, %.3f ns per element, bits %s\n", mode, mode ? "one lane adds" : "every lane adds",
                        ms / 20, ms / 20 * 1e6 / n, std::memcmp(&got, &fwd, 8) == 0 ? "equal" : "DIFFER");
        }
    }
    return 0;
}
