// skml_opt.hpp -- the optimiser update of one element and the state accesses around it: what the
// update kernels of skml_optim.hip and the fused fixed-point step of skml_fixed.hip share
// (ml/objective/GradientDescent.scala:104-117, ml/objective/Adam.scala:50-77).
#pragma once
#include "skml_device.hpp"

namespace skml {

typedef float of32x4 __attribute__((ext_vector_type(4)));
typedef double of64x2 __attribute__((ext_vector_type(2)));

// N (8 or 4) consecutive values from / to p + e0 as 16-byte accesses (p 16-byte aligned, e0 a
// multiple of N).
template <typename T, int N>
__device__ __forceinline__ void load_state(const T* __restrict__ p, int64_t e0, T (&x)[N]) {
    if constexpr (sizeof(T) == 4) {
        const of32x4* s = reinterpret_cast<const of32x4*>(p + e0);
#pragma unroll
        for (int j = 0; j < N / 4; j++) {
            const of32x4 a = s[j];
            x[4 * j] = a.x; x[4 * j + 1] = a.y; x[4 * j + 2] = a.z; x[4 * j + 3] = a.w;
        }
    } else {
        const of64x2* s = reinterpret_cast<const of64x2*>(p + e0);
#pragma unroll
        for (int j = 0; j < N / 2; j++) {
            const of64x2 a = s[j];
            x[2 * j] = a.x; x[2 * j + 1] = a.y;
        }
    }
}
template <typename T, int N>
__device__ __forceinline__ void store_state(T* __restrict__ p, int64_t e0, const T (&x)[N]) {
    if constexpr (sizeof(T) == 4) {
        of32x4* d = reinterpret_cast<of32x4*>(p + e0);
#pragma unroll
        for (int j = 0; j < N / 4; j++) d[j] = of32x4{x[4 * j], x[4 * j + 1], x[4 * j + 2], x[4 * j + 3]};
    } else {
        of64x2* d = reinterpret_cast<of64x2*>(p + e0);
#pragma unroll
        for (int j = 0; j < N / 2; j++) d[j] = of64x2{x[2 * j], x[2 * j + 1]};
    }
}

// The update of one element, in double in the reference's operation order (Adam.scala:54-59,
// GradientDescent.scala:108; the build has -ffp-contract=off, sqrt and / are correctly rounded).
// fp32 state is widened on load; ng uses the unrounded m_t and v_t; each of w, m, v is rounded once,
// at its store.  An element that the LIVE selection leaves out keeps its bits.
template <bool ADAM, typename W>
__device__ __forceinline__ void opt_apply(double g, W& w, W& m, W& v, const OptConsts& k) {
    const bool upd = !k.live || fabs(g) > 1e-8;  // DenseDoubleGradient.toSparse's Math.abs(x) > Maths.EPS
    if constexpr (ADAM) {
        const double m_t = k.beta1 * (double)m + k.omb1 * g;
        const double v_t = k.beta2 * (double)v + (k.omb2 * g) * g;
        const double ng = (k.c_m * m_t) / (k.c_d * (sqrt(v_t) + k.eps));
        const double w_t = (double)w - ng * k.lr;
        w = upd ? (W)w_t : w;
        m = upd ? (W)m_t : m;
        v = upd ? (W)v_t : v;
    } else {
        const double w_t = (double)w - g * k.lr;
        w = upd ? (W)w_t : w;
    }
}

// A lane's N consecutive elements at e0: state in, update, state out.
template <bool ADAM, typename W, int N>
struct StateN {
    W w[N], m[N], v[N];
    __device__ __forceinline__ void load(const W* __restrict__ pw, const W* __restrict__ pm, const W* __restrict__ pv,
                                         int64_t e0) {
        load_state(pw, e0, w);
        if constexpr (ADAM) {
            load_state(pm, e0, m);
            load_state(pv, e0, v);
        }
    }
    __device__ __forceinline__ void apply(const double (&g)[N], const OptConsts& k) {
#pragma unroll
        for (int e = 0; e < N; e++) opt_apply<ADAM>(g[e], w[e], m[e], v[e], k);
    }
    __device__ __forceinline__ void store(W* __restrict__ pw, W* __restrict__ pm, W* __restrict__ pv, int64_t e0) {
        store_state(pw, e0, w);
        if constexpr (ADAM) {
            store_state(pm, e0, m);
            store_state(pv, e0, v);
        }
    }
};
// One element (the last elements of a partial step, and the key / value form).
template <bool ADAM, typename W>
__device__ __forceinline__ void opt_apply_at(double g, W* __restrict__ pw, W* __restrict__ pm, W* __restrict__ pv,
                                             int64_t i, const OptConsts& k) {
    W w = pw[i], m = W(0), v = W(0);
    if constexpr (ADAM) {
        m = pm[i];
        v = pv[i];
    }
    opt_apply<ADAM>(g, w, m, v, k);
    pw[i] = w;
    if constexpr (ADAM) {
        pm[i] = m;
        pv[i] = v;
    }
}

// A workgroup's live count into *count: a ballot and a popcount per wave and element slot, one LDS
// add per wave, one global atomic per workgroup.  Every lane of a wave reaches every call.
struct LiveCount {
    unsigned long long wave = 0;  // wave-uniform
    __device__ __forceinline__ void add(bool live) { wave += (unsigned long long)__popcll(__ballot(live)); }
    __device__ __forceinline__ void finish(unsigned long long* s_cnt, unsigned long long* count) {
        if (threadIdx.x == 0) *s_cnt = 0;
        __syncthreads();
        if ((threadIdx.x & 63) == 0 && wave) atomicAdd(s_cnt, wave);
        __syncthreads();
        if (threadIdx.x == 0 && *s_cnt) atomicAdd(count, *s_cnt);
    }
};

}  // namespace skml
