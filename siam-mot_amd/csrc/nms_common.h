// Shared by nms.hip and rpn_proposals.hip: the 64-box tile of the NMS bitmask and the IoU both compare against the threshold.
#pragma once
#include "smot_common.h"

namespace smot {

constexpr int NMS_T = 64;

__device__ __forceinline__ float iou_plus1(const float* a, const float* b) {
    const float left = fmaxf(a[0], b[0]), right = fminf(a[2], b[2]);
    const float top = fmaxf(a[1], b[1]), bottom = fminf(a[3], b[3]);
    const float w = fmaxf(right - left + 1.0f, 0.0f), h = fmaxf(bottom - top + 1.0f, 0.0f);
    const float inter = w * h;
    const float sa = (a[2] - a[0] + 1.0f) * (a[3] - a[1] + 1.0f);
    const float sb = (b[2] - b[0] + 1.0f) * (b[3] - b[1] + 1.0f);
    return inter / (sa + sb - inter);
}

}  // namespace smot
