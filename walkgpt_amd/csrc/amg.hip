// What SamAutomaticMaskGenerator does behind the mask decoder (automatic_mask_generator.py:260-321, utils/amg.py), without ever writing a
// full-resolution float: per-mask statistics and the bit-packed binary mask from the low-res logits in one pass, the change positions of the
// run-length code of selected masks, and greedy box NMS.  No atomics and no hand-over between workgroups anywhere: every reduction is
// partials -> a second small kernel that folds them in a fixed order, and everything folded is an integer, so two runs give the same bits.
#include "wg_common.h"
#include "post_common.h"

// ------------------------------------------------------------------------------------------------------------
// (a) Mask statistics.  The pixel is the very float wg_postprocess_masks_f32 writes (post_common.h).  Per mask n:
//   stats[n] = {count(x > thr + off), count(x > thr - off), count(x > thr), x_min, y_min, x_max, y_max, 0}      (int32; the box is that of
//              x > thr in inclusive pixel indices, 0,0,0,0 for an empty mask: batched_mask_to_box, amg.py:303-346)
//   bits[n, yb, x] bit r = (pixel (32 yb + r, x) > thr), rows past out_h are 0                                   (uint32 [N, ceil(out_h/32), out_w])
// grid (column blocks of 256, row blocks of 32, masks); a thread owns one output column and assembles one whole word, so a wave's store is 256
// contiguous bytes.  Algorithmic bytes per mask: read lh*lw*4, write out_h*out_w/8.
// ------------------------------------------------------------------------------------------------------------
#define AMG_ROWS 32
#define AMG_EMPTY_MIN (1 << 30)      // x_min / y_min of a workgroup (mask) without a set pixel; x_max / y_max are -1

__global__ __launch_bounds__(256) void wg_amg_mask_stats_kernel(const float* __restrict__ low, int* __restrict__ partial, unsigned* __restrict__ bits, int lh,
                                                                int lw, PostScales sc, int in_h, int in_w, int out_h, int out_w, float t_hi, float t_lo,
                                                                float t_mid) {
    __shared__ float red[4][7];
    const int ox = blockIdx.x * 256 + threadIdx.x, n = blockIdx.z;
    const int hb = (int)gridDim.y;
    unsigned word = 0u;
    int c_hi = 0, c_lo = 0;
    if (ox < out_w) {
        const float* m = low + (long)n * lh * lw;
        const PostCol col = wg_post_col(ox, sc, in_w, lw);
        // rows in chunks of four, all 64 taps of a chunk requested before the first is used (as wg_postprocess_kernel); rows past the image
        // repeat the last one and count for nothing
#pragma unroll 1
        for (int r0 = 0; r0 < AMG_ROWS; r0 += 4) {
            float tap[4][2][2][4], ly[4], lya[4][2];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int oy = blockIdx.y * AMG_ROWS + r0 + r;
                wg_post_taps(m, oy < out_h ? oy : out_h - 1, sc, in_h, lh, lw, col, tap[r], ly[r], lya[r]);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int oy = blockIdx.y * AMG_ROWS + r0 + r;
                const float res = wg_post_eval(tap[r], ly[r], lya[r], col);
                if (oy < out_h) {
                    c_hi += res > t_hi ? 1 : 0;
                    c_lo += res > t_lo ? 1 : 0;
                    word |= res > t_mid ? (1u << (r0 + r)) : 0u;
                }
            }
        }
        bits[((long)n * hb + blockIdx.y) * out_w + ox] = word;
    }
    // the workgroup's record: three sums, two minima (as maxima of the negated value), two maxima.  Every value is an integer below 2^24 in
    // magnitude or the empty marker 2^30, all exact in fp32, so the float reductions of wg_common.h return exact results
    const int first = word ? __builtin_ctz(word) : 0, last = word ? 31 - __builtin_clz(word) : 0;
    float v[7];
    v[0] = (float)c_hi;
    v[1] = (float)c_lo;
    v[2] = (float)__builtin_popcount(word);
    v[3] = word ? -(float)ox : -(float)AMG_EMPTY_MIN;
    v[4] = word ? -(float)(blockIdx.y * AMG_ROWS + first) : -(float)AMG_EMPTY_MIN;
    v[5] = word ? (float)ox : -1.f;
    v[6] = word ? (float)(blockIdx.y * AMG_ROWS + last) : -1.f;
#pragma unroll
    for (int k = 0; k < 7; ++k) v[k] = k < 3 ? wg_wave_sum(v[k]) : wg_wave_max(v[k]);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < 7; ++k) red[threadIdx.x >> 6][k] = v[k];
    __syncthreads();
    if (threadIdx.x < 8) {
        const int k = threadIdx.x;
        float r = 0.f;
        if (k < 3) r = red[0][k] + red[1][k] + red[2][k] + red[3][k];
        else if (k < 7) r = fmaxf(fmaxf(red[0][k], red[1][k]), fmaxf(red[2][k], red[3][k]));
        const int iv = (k == 3 || k == 4) ? (int)(-r) : (int)r;
        const long blk = ((long)n * hb + blockIdx.y) * gridDim.x + blockIdx.x;
        partial[blk * 8 + k] = iv;
    }
}

// one wave per mask folds the workgroups' records in a fixed order (integers: the order does not even matter for the value)
__global__ __launch_bounds__(64) void wg_amg_mask_stats_final_kernel(const int* __restrict__ partial, int* __restrict__ stats, int nblk) {
    const int n = blockIdx.x;
    int c[3] = {0, 0, 0}, lo[2] = {AMG_EMPTY_MIN, AMG_EMPTY_MIN}, hi[2] = {-1, -1};
    for (int i = threadIdx.x; i < nblk; i += 64) {
        const int* p = partial + ((long)n * nblk + i) * 8;
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] += p[k];
        lo[0] = min(lo[0], p[3]); lo[1] = min(lo[1], p[4]);
        hi[0] = max(hi[0], p[5]); hi[1] = max(hi[1], p[6]);
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] += __shfl_xor(c[k], s, 64);
#pragma unroll
        for (int k = 0; k < 2; ++k) { lo[k] = min(lo[k], __shfl_xor(lo[k], s, 64)); hi[k] = max(hi[k], __shfl_xor(hi[k], s, 64)); }
    }
    if (threadIdx.x == 0) {
        const bool empty = hi[0] < lo[0] || hi[1] < lo[1];
        int* o = stats + (long)n * 8;
        o[0] = c[0]; o[1] = c[1]; o[2] = c[2];
        o[3] = empty ? 0 : lo[0]; o[4] = empty ? 0 : lo[1]; o[5] = empty ? 0 : hi[0]; o[6] = empty ? 0 : hi[1];
        o[7] = 0;
    }
}

static long wg_amg_blocks(int out_h, int out_w) { return (long)((out_h + AMG_ROWS - 1) / AMG_ROWS) * ((out_w + 255) / 256); }

extern "C" long wg_amg_mask_stats_workspace_ints(int N, int out_h, int out_w) {
    if (N <= 0 || out_h <= 0 || out_w <= 0) return 0;
    return (long)N * wg_amg_blocks(out_h, out_w) * 8;
}

extern "C" int wg_amg_mask_stats_f32(const float* low_res, int* stats, unsigned* bits, int* workspace, long workspace_ints, int N, int low_h, int low_w,
                                     int img_size, int in_h, int in_w, int out_h, int out_w, float mask_threshold, float stability_offset, void* stream) {
    WG_REQUIRE(low_res && stats && bits && workspace && N > 0 && low_h > 0 && low_w > 0 && img_size > 0, "amg_mask_stats: bad arguments");
    WG_REQUIRE(in_h > 0 && in_w > 0 && in_h <= img_size && in_w <= img_size && out_h > 0 && out_w > 0,
               "amg_mask_stats: crop (%d,%d) must lie inside the %d^2 padded image", in_h, in_w, img_size);
    WG_REQUIRE((long)low_h * low_w < (1L << 31), "amg_mask_stats: low-res masks of 2^31 pixels or more");
    // grid limits: 65535 masks and 65535 row blocks of 32 per call; the counts are int32 and the box goes through fp32 exactly below 2^24
    WG_REQUIRE(N <= 65535 && out_h < (1 << 21) && out_w < (1 << 24) && (long)out_h * out_w < (1L << 31),
               "amg_mask_stats: more than 65535 masks, or an output of 2^31 pixels or more, per call");
    const long nblk = wg_amg_blocks(out_h, out_w);
    WG_REQUIRE(workspace_ints >= (long)N * nblk * 8, "amg_mask_stats: workspace too small (need %ld ints)", (long)N * nblk * 8);
    const int gx = (out_w + 255) / 256, gy = (out_h + AMG_ROWS - 1) / AMG_ROWS;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(wg_amg_mask_stats_kernel, dim3((unsigned)gx, (unsigned)gy, (unsigned)N), dim3(256), 0, st, low_res, workspace, bits, low_h, low_w,
                       wg_post_scales(low_h, low_w, img_size, in_h, in_w, out_h, out_w), in_h, in_w, out_h, out_w,
                       (float)((double)mask_threshold + (double)stability_offset), (float)((double)mask_threshold - (double)stability_offset), mask_threshold);
    hipLaunchKernelGGL(wg_amg_mask_stats_final_kernel, dim3((unsigned)N), dim3(64), 0, st, (const int*)workspace, stats, (int)nblk);
    return wg_check_launch("wg_amg_mask_stats_f32");
}

// ------------------------------------------------------------------------------------------------------------
// (b) Change positions of the run-length code (mask_to_rle_pytorch, amg.py:107-135, of uncrop_masks, amg.py:255-264).  The mask keep[k] occupies
// rows y0 .. y0 + out_h - 1 and columns x0 .. x0 + out_w - 1 of an H x W frame that is zero elsewhere; its change positions are every p in
// 1 .. H W - 1 with bit[p] != bit[p - 1] in the column-major flattening p = x H + y.  One thread owns one (mask, column) and walks its words:
// within a word the transitions are w ^ ((w << 1) | carry).  The bit before a column's first row is the previous column's last bit only when the
// mask spans the frame's height (otherwise a zero row lies between), and a column that ends in 1 is closed at the row behind it when a zero
// follows there: below the crop, or, for the crop's last column, in the frame's next column.
// MODE 0 counts (int32 [K, out_w]); MODE 1 stores the positions of (k, x) from offsets[k out_w + x - 1] on (the inclusive running sum of the
// counts; positions therefore come out sorted per mask) and first[k] = the frame's bit 0.
// ------------------------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(256) void wg_amg_rle_kernel(const unsigned* __restrict__ bits, const int* __restrict__ keep, int n_masks, int* __restrict__ counts,
                                                         const long* __restrict__ offsets, int* __restrict__ positions, long total, int* __restrict__ first,
                                                         int out_h, int out_w, int x0, int y0, int H, int W) {
    const int x = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    if (x >= out_w) return;
    int n = keep[k];
    n = n < 0 ? 0 : (n >= n_masks ? n_masks - 1 : n);      // (an index outside the bit planes must not become an address: clamped; ops.amg_rle refuses such a list)
    const int hb = (out_h + 31) >> 5;
    const unsigned* col = bits + (long)n * hb * out_w + x;
    const bool full = out_h == H;
    unsigned carry = 0u;
    if (full && x > 0) carry = (col[(long)(hb - 1) * out_w - 1] >> ((out_h - 1) & 31)) & 1u;
    const long base = (long)(x0 + x) * H + y0;              // position of this column's row 0
    const long i = (long)k * out_w + x;
    long at = 0;
    if (MODE == 1) {
        at = i > 0 ? offsets[i - 1] : 0;
        if (x == 0) first[k] = (x0 == 0 && y0 == 0) ? (int)(col[0] & 1u) : 0;
    }
    int cnt = 0;
    unsigned w = 0u;
    for (int b = 0; b < hb; ++b) {
        w = col[(long)b * out_w];
        unsigned t = w ^ ((w << 1) | carry);
        if (b == hb - 1 && (out_h & 31)) t &= (1u << (out_h & 31)) - 1u;   // rows past out_h are not this column's
        if (b == 0 && base == 0) t &= ~1u;                                  // p = 0 has no predecessor
        carry = w >> 31;
        if (MODE == 0) {
            cnt += __builtin_popcount(t);
        } else {
            while (t) {
                const int r = __builtin_ctz(t);
                t &= t - 1u;
                if (at < total) positions[at] = (int)(base + 32 * b + r);
                ++at;
            }
        }
    }
    const unsigned last_bit = (w >> ((out_h - 1) & 31)) & 1u;
    const long close = base + out_h;
    if (last_bit && (!full || x == out_w - 1) && close < (long)H * W) {
        if (MODE == 0) ++cnt;
        else if (at < total) positions[at] = (int)close;
    }
    if (MODE == 0) counts[i] = cnt;
}

static int wg_amg_rle_check(const char* what, const void* bits, const void* keep, int N, int K, int out_h, int out_w, int x0, int y0, int H, int W) {
    WG_REQUIRE(bits && keep && N > 0 && K > 0 && out_h > 0 && out_w > 0 && H > 0 && W > 0, "%s: bad arguments", what);
    WG_REQUIRE(x0 >= 0 && y0 >= 0 && (long)x0 + out_w <= W && (long)y0 + out_h <= H, "%s: the %dx%d mask at (%d,%d) does not lie inside the %dx%d frame", what,
               out_h, out_w, x0, y0, H, W);
    WG_REQUIRE((long)H * W < (1L << 31), "%s: frames of 2^31 pixels or more are not supported (positions are int32)", what);
    WG_REQUIRE(K <= 65535, "%s: more than 65535 selected masks per call", what);
    return WG_OK;
}

extern "C" int wg_amg_rle_count_i32(const unsigned* bits, const int* keep, int* counts, int N, int K, int out_h, int out_w, int x0, int y0, int H, int W,
                                    void* stream) {
    const int rc = wg_amg_rle_check("amg_rle_count", bits, keep, N, K, out_h, out_w, x0, y0, H, W);
    if (rc != WG_OK) return rc;
    WG_REQUIRE(counts, "amg_rle_count: null output");
    hipLaunchKernelGGL(wg_amg_rle_kernel<0>, dim3((unsigned)((out_w + 255) / 256), (unsigned)K), dim3(256), 0, (hipStream_t)stream, bits, keep, N, counts,
                       (const long*)nullptr, (int*)nullptr, 0L, (int*)nullptr, out_h, out_w, x0, y0, H, W);
    return wg_check_launch("wg_amg_rle_count_i32");
}

extern "C" int wg_amg_rle_write_i32(const unsigned* bits, const int* keep, const long* offsets, int* positions, long total, int* first, int N, int K, int out_h,
                                    int out_w, int x0, int y0, int H, int W, void* stream) {
    const int rc = wg_amg_rle_check("amg_rle_write", bits, keep, N, K, out_h, out_w, x0, y0, H, W);
    if (rc != WG_OK) return rc;
    WG_REQUIRE(offsets && first && total >= 0 && (positions || total == 0), "amg_rle_write: null output or negative total");
    hipLaunchKernelGGL(wg_amg_rle_kernel<1>, dim3((unsigned)((out_w + 255) / 256), (unsigned)K), dim3(256), 0, (hipStream_t)stream, bits, keep, N, (int*)nullptr,
                       offsets, positions, total, first, out_h, out_w, x0, y0, H, W);
    return wg_check_launch("wg_amg_rle_write_i32");
}

// ------------------------------------------------------------------------------------------------------------
// (c) Greedy box NMS (torchvision.ops.nms as automatic_mask_generator.py:206-211, :245-250, :357-362 call it, one category).  boxes [N, 4] fp32
// XYXY, order [N] = box indices by descending score.  Kernel 1: the suppression matrix, uint64 [N, ceil(N/64)]; bit j of row i (both positions
// in `order`) is set when j > i and inter / (area_i + area_j - inter) > iou_threshold, in torchvision's arithmetic: area (x2-x1)(y2-y1), the
// intersection's extents clamped at 0, every operation rounded once and the division correctly rounded (wg_div_rn below), so the decision is the
// one torch makes on the same boxes.  Kernel 2: one workgroup walks `order` and ORs the rows of kept boxes into a removed-set held in LDS.
// ------------------------------------------------------------------------------------------------------------
#define NMS_MAX 8192

// a / b correctly rounded: this file is built with -ffast-math, under which `/` is a reciprocal approximation times the numerator.  The IEEE
// sequence of the ISA manual, written out in builtins: scale both operands, a reciprocal refined by one Newton step, the quotient refined twice
// in fma, then v_div_fmas / v_div_fixup undo the scaling and settle the special cases.
__device__ __forceinline__ float wg_div_rn(float a, float b) {
    bool vcc_d, vcc_n;
    const float ds = __builtin_amdgcn_div_scalef(a, b, false, &vcc_d);     // the denominator, scaled
    const float ns = __builtin_amdgcn_div_scalef(a, b, true, &vcc_n);      // the numerator, scaled
    float r = __builtin_amdgcn_rcpf(ds);
    const float e0 = __builtin_fmaf(-ds, r, 1.0f);
    r = __builtin_fmaf(e0, r, r);
    float q = wg_mul_rn(ns, r);
    const float e1 = __builtin_fmaf(-ds, q, ns);
    q = __builtin_fmaf(e1, r, q);
    const float e2 = __builtin_fmaf(-ds, q, ns);
    return __builtin_amdgcn_div_fixupf(__builtin_amdgcn_div_fmasf(e2, r, q, vcc_n), b, a);
}

__global__ __launch_bounds__(64) void wg_nms_matrix_kernel(const float* __restrict__ boxes, const int* __restrict__ order, unsigned long long* __restrict__ matrix,
                                                           int N, int words, float thr) {
    __shared__ float cb[64][5];
    const int w = blockIdx.x, i = blockIdx.y * 64 + threadIdx.x;
    const int j0 = w * 64 + threadIdx.x;
    if (j0 < N) {
        int idx = order[j0];
        idx = idx < 0 ? 0 : (idx >= N ? N - 1 : idx);
        const f32x4 b = *(const f32x4*)(boxes + 4L * idx);
        cb[threadIdx.x][0] = b[0]; cb[threadIdx.x][1] = b[1]; cb[threadIdx.x][2] = b[2]; cb[threadIdx.x][3] = b[3];
        cb[threadIdx.x][4] = wg_mul_rn(wg_sub_rn(b[2], b[0]), wg_sub_rn(b[3], b[1]));
    }
    __syncthreads();
    if (i >= N) return;
    unsigned long long word = 0ull;
    if (w * 64 + 63 > i) {      // (a word wholly at or before i holds no j > i)
        int idx = order[i];
        idx = idx < 0 ? 0 : (idx >= N ? N - 1 : idx);
        const f32x4 a = *(const f32x4*)(boxes + 4L * idx);
        const float area = wg_mul_rn(wg_sub_rn(a[2], a[0]), wg_sub_rn(a[3], a[1]));
        const int nj = N - w * 64 < 64 ? N - w * 64 : 64;
        for (int t = 0; t < nj; ++t) {
            if (w * 64 + t <= i) continue;
            const float xx1 = fmaxf(a[0], cb[t][0]), yy1 = fmaxf(a[1], cb[t][1]), xx2 = fminf(a[2], cb[t][2]), yy2 = fminf(a[3], cb[t][3]);
            const float iw = fmaxf(wg_sub_rn(xx2, xx1), 0.f), ih = fmaxf(wg_sub_rn(yy2, yy1), 0.f);
            const float inter = wg_mul_rn(iw, ih);
            const float iou = wg_div_rn(inter, wg_sub_rn(wg_add_rn(area, cb[t][4]), inter));
            if (iou > thr) word |= 1ull << t;
        }
    }
    matrix[(long)i * words + w] = word;
}

__global__ __launch_bounds__(128) void wg_nms_walk_kernel(const unsigned long long* __restrict__ matrix, const int* __restrict__ order, int* __restrict__ keep,
                                                          int* __restrict__ n_keep, int N, int words) {
    __shared__ unsigned long long removed[NMS_MAX / 64];
    const int t = threadIdx.x;
    removed[t] = 0ull;
    __syncthreads();
    int nk = 0;
    // thread t owns word t of the removed-set; row i + 1 is requested while row i is decided.  One barrier per step is enough: a kept row i only
    // sets bits j > i, so the bit a slower thread still reads for step i cannot change under it.  (Formally the owner's read-modify-write of
    // word i >> 6 and the other threads' read of it in the same step are unordered: this rests on an aligned 64-bit LDS access being one
    // ds_read_b64 / ds_write_b64 that does not tear, which holds on this hardware; the read goes through a volatile pointer so that it stays
    // one such access per step.)
    const volatile unsigned long long* removed_now = removed;
    unsigned long long nxt = t < words ? matrix[t] : 0ull;
    for (int i = 0; i < N; ++i) {
        const unsigned long long cur = nxt;
        if (i + 1 < N && t < words) nxt = matrix[(long)(i + 1) * words + t];
        const bool alive = !((removed_now[i >> 6] >> (i & 63)) & 1ull);
        if (alive) {
            removed[t] |= cur;
            if (t == 0) keep[nk++] = order[i];
        }
        __syncthreads();
    }
    if (t == 0) n_keep[0] = nk;
}

extern "C" long wg_nms_workspace_words(int N) { return N > 0 ? (long)N * ((N + 63) / 64) : 0; }

extern "C" int wg_nms_f32(const float* boxes, const int* order, float iou_threshold, int* keep, int* n_keep, unsigned long long* workspace, long workspace_words,
                          int N, void* stream) {
    WG_REQUIRE(boxes && order && keep && n_keep && workspace && N > 0, "nms: bad arguments");
    WG_REQUIRE(N <= NMS_MAX, "nms: %d boxes (at most %d per call: an 8 MB suppression matrix and a 1 KB removed-set)", N, NMS_MAX);
    WG_REQUIRE(((uintptr_t)boxes & 15) == 0, "nms: boxes must be 16-byte aligned");
    const int words = (N + 63) / 64;
    WG_REQUIRE(workspace_words >= (long)N * words, "nms: workspace too small (need %ld 64-bit words)", (long)N * words);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(wg_nms_matrix_kernel, dim3((unsigned)words, (unsigned)words), dim3(64), 0, st, boxes, order, workspace, N, words, iou_threshold);
    hipLaunchKernelGGL(wg_nms_walk_kernel, dim3(1), dim3(128), 0, st, (const unsigned long long*)workspace, order, keep, n_keep, N, words);
    return wg_check_launch("wg_nms_f32");
}
