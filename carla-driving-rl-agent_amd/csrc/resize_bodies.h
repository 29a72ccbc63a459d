// The bilinear resize rule shared by the contrastive views (views.hip) and the display maps of the occlusion saliency (explain.hip).
#pragma once
#include "cdrl_common.h"

namespace cdrl {

// Source position of destination index d when `crop` source pixels are resized to `full`: (d + 0.5) * crop / full - 0.5 clamped to
// [0, crop - 1], in exact integer arithmetic (numerator over 2 * full), so the taps never depend on float rounding of the coordinate
// and a full-size crop has fraction 0.  -> lower tap i0, upper tap i1 = min(i0 + 1, crop - 1), fraction in [0, 1)
__device__ __forceinline__ void resize_src(int d, int crop, int full, int& i0, int& i1, float& frac) {
    const int den = 2 * full;
    int num = (2 * d + 1) * crop - full;
    num = num < 0 ? 0 : num;
    const int top = (crop - 1) * den;
    num = num > top ? top : num;
    i0 = num / den;
    frac = (float)(num - i0 * den) / (float)den;
    i1 = i0 + 1 < crop ? i0 + 1 : crop - 1;
}

}  // namespace cdrl
