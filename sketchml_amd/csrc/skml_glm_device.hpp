// skml_glm_device.hpp -- the device functions the sparse kernels of skml_glm.hip and the dense ones of
// skml_glm_dense.hip share, so that both data layouts run the same arithmetic: loss.loss / loss.grad
// (ml/objective/Loss.scala:56-137) and the confusion counts of the validation pass
// (ml/util/ValidationUtil.scala:21-31).  The other two shared pieces are already common: the loss sum
// is a launch of its own (launch_glm_loss_sum, skml_internal.h) and toAuto's live count is LiveCount
// (skml_opt.hpp).
#pragma once
#include "skml_device.hpp"
#include "skml_valid.hpp"

namespace skml {

constexpr int kGlmLog = 0, kGlmHinge = 1, kGlmSquare = 2;

// loss.loss(pre, y) and loss.grad(pre, y), the branches as Loss.scala writes them.  L1LogLoss and
// L2LogLoss share their arithmetic.
template <int LOSS>
__device__ __forceinline__ void glm_loss(double pre, double y, double& loss, double& grad) {
    if constexpr (LOSS == kGlmLog) {
        const double z = pre * y;
        if (z > 18) {
            const double e = exp(-z);
            loss = e;
            grad = y * e;
        } else if (z < -18) {
            loss = -z;
            grad = y;
        } else {
            loss = log(1.0 + exp(-z));
            grad = y / (1.0 + exp(z));
        }
    } else if constexpr (LOSS == kGlmHinge) {
        const double z = pre * y;
        loss = z < 1.0 ? 1.0 - z : 0.0;
        grad = z <= 1.0 ? y : 0.0;
    } else {
        const double d = pre - y;
        loss = (0.5 * d) * d;
        grad = y - pre;
    }
}

// A workgroup's confusion counts into cnt[0 .. 4) += truePos, trueNeg, falsePos, falseNeg and cnt[4] +=
// the NaN scores: a ballot and a popcount per wave and instance slot, one LDS add per wave, one global
// atomic per workgroup and counter (integer sums: no order to depend on).  Every lane of a wave
// reaches every add, every wave of the workgroup finish; s_cnt is kValidCounters words of LDS.
constexpr int kValidCounters = 5;
struct ValidCount {
    unsigned long long wave[kValidCounters] = {0, 0, 0, 0, 0};  // wave-uniform
    // cls: valid_class of the lane's instance, kValidNone for a lane without one
    __device__ __forceinline__ void add(int cls, bool nan) {
#pragma unroll
        for (int k = 0; k < 4; k++) wave[k] += (unsigned long long)__popcll(__ballot(cls == k + 1));
        wave[4] += (unsigned long long)__popcll(__ballot(nan));
    }
    __device__ __forceinline__ void finish(unsigned long long* s_cnt, unsigned long long* cnt) {
        if (threadIdx.x < kValidCounters) s_cnt[threadIdx.x] = 0;
        __syncthreads();
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int k = 0; k < kValidCounters; k++)
                if (wave[k]) atomicAdd(&s_cnt[k], wave[k]);
        }
        __syncthreads();
        if (threadIdx.x < kValidCounters && s_cnt[threadIdx.x]) atomicAdd(&cnt[threadIdx.x], s_cnt[threadIdx.x]);
    }
};

}  // namespace skml
