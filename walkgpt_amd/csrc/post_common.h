// Shared by misc.hip (wg_postprocess_kernel) and amg.hip (wg_amg_mask_stats_kernel): the arithmetic of Sam.postprocess_masks (sam.py:137-172),
// i.e. the source-index rule of the two bilinear resamples and the 16-tap evaluation of one output pixel, operation by operation as PyTorch's
// CPU kernel does it.  One copy, so that both kernels produce the very same float for a pixel.
#pragma once
#include "wg_common.h"

// The four source-index scales of the two resamples (torch: input size / output size in fp32), divided on the host: a device-side `/` under
// -ffast-math is a reciprocal approximation times the numerator.  (Through double: a ratio of two small integers is never a rounding tie.)
struct PostScales { float s1y, s1x, s2y, s2x; };
static inline PostScales wg_post_scales(int lh, int lw, int img, int in_h, int in_w, int out_h, int out_w) {
    return PostScales{(float)((double)lh / (double)img), (float)((double)lw / (double)img), (float)((double)in_h / (double)out_h),
                      (float)((double)in_w / (double)out_w)};
}

// One IEEE operation, one rounding, whatever the translation unit's floating-point mode: HIP's __fmul_rn / __fadd_rn are plain `*` / `+` unless
// OCML_BASIC_ROUNDED_OPERATIONS is defined, and under -ffast-math the back end fuses and re-associates them (differently from one
// instantiation of a kernel to the next: the fused-score form of the postprocess kernel differed from the plain one by an ulp in column 0).
__device__ __forceinline__ float wg_mul_rn(float a, float b) { float r; asm("v_mul_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float wg_add_rn(float a, float b) { float r; asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float wg_sub_rn(float a, float b) { float r; asm("v_sub_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ void wg_src_index(int dst, float scale, int in_size, int& i0, int& i1, float& l1) {
    // separate roundings (no FMA contraction) so the source index and weight match PyTorch's CPU kernel bit for bit
    float s = wg_sub_rn(wg_mul_rn(scale, (float)dst + 0.5f), 0.5f);
    s = s < 0.f ? 0.f : s;
    i0 = (int)s;
    i0 = i0 < in_size - 1 ? i0 : in_size - 1;
    i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
    l1 = wg_sub_rn(s, (float)i0);
}

// The column half of a pixel's taps: the same for every row of an output column, so a thread that owns a column forms it once.
struct PostCol {
    int xa[2][2];        // [second-resample tap][first-resample tap]
    float lx, lxa[2];
};
__device__ __forceinline__ PostCol wg_post_col(int ox, const PostScales& sc, int in_w, int lw) {
    PostCol c;
    int x0, x1;
    wg_src_index(ox, sc.s2x, in_w, x0, x1, c.lx);
    wg_src_index(x0, sc.s1x, lw, c.xa[0][0], c.xa[0][1], c.lxa[0]);
    wg_src_index(x1, sc.s1x, lw, c.xa[1][0], c.xa[1][1], c.lxa[1]);
    return c;
}

// The sixteen low-res taps of output pixel (oy, column c) of mask `m` and the row weights; loads only, so a caller can request several rows' taps
// before it uses the first.
__device__ __forceinline__ void wg_post_taps(const float* __restrict__ m, int oy, const PostScales& sc, int in_h, int lh, int lw, const PostCol& c,
                                             float (&tap)[2][2][4], float& ly, float (&lya)[2]) {
    int y0, y1, ya[2][2];
    wg_src_index(oy, sc.s2y, in_h, y0, y1, ly);
    wg_src_index(y0, sc.s1y, lh, ya[0][0], ya[0][1], lya[0]);
    wg_src_index(y1, sc.s1y, lh, ya[1][0], ya[1][1], lya[1]);
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            tap[j][i][0] = m[ya[j][0] * lw + c.xa[i][0]]; tap[j][i][1] = m[ya[j][0] * lw + c.xa[i][1]];
            tap[j][i][2] = m[ya[j][1] * lw + c.xa[i][0]]; tap[j][i][3] = m[ya[j][1] * lw + c.xa[i][1]];
        }
}

// The pixel from its taps: the img^2 intermediate at (y0|y1, x0|x1) as torch's first resample forms it, then the second resample.
__device__ __forceinline__ float wg_post_eval(const float (&tap)[2][2][4], float ly, const float (&lya)[2], const PostCol& c) {
    float up[2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const float wy = wg_sub_rn(1.f, lya[j]), wx = wg_sub_rn(1.f, c.lxa[i]);
            up[j][i] = wg_add_rn(wg_mul_rn(wy, wg_add_rn(wg_mul_rn(wx, tap[j][i][0]), wg_mul_rn(c.lxa[i], tap[j][i][1]))),
                                 wg_mul_rn(lya[j], wg_add_rn(wg_mul_rn(wx, tap[j][i][2]), wg_mul_rn(c.lxa[i], tap[j][i][3]))));
        }
    const float vy = wg_sub_rn(1.f, ly), vx = wg_sub_rn(1.f, c.lx);
    return wg_add_rn(wg_mul_rn(vy, wg_add_rn(wg_mul_rn(vx, up[0][0]), wg_mul_rn(c.lx, up[0][1]))),
                     wg_mul_rn(ly, wg_add_rn(wg_mul_rn(vx, up[1][0]), wg_mul_rn(c.lx, up[1][1]))));
}
