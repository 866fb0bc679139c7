// SAM's prompt side for point / box / mask prompts and Sam.preprocess (0.3.0).
//
//   wg_prompt_sparse_f32   PromptEncoder._embed_points / _embed_boxes / forward's concatenation (prompt_encoder.py:80-112, 150-186) and
//                          PositionEmbeddingRandom.forward_with_coords / _pe_encoding (:196-214, :231-240): every sparse row in one launch
//   wg_mask_embed_bf16     PromptEncoder.mask_downscaling (:57-65) on `masks` (_embed_masks :114-117; LayerNorm2d common.py:31-43): one
//                          kernel, each output pixel from its own 4x4 input patch, no intermediate in memory
//   wg_normalize_pad_bf16  Sam.preprocess (sam.py:174-186)
#include "wg_common.h"

// ------------------------------------------------------------------------------------------------------------
// Sparse rows.  Row r of batch b (R = Np + 2*has_box + T rows, Np = N + pad): points, then the two box corners, then text rows.
// The positional term is [sin(2 pi t) | cos(2 pi t)] with t = (2 x / W - 1) G[0, f] + (2 y / H - 1) G[1, f] in turns; t reaches ~6
// turns (40 rad), so it is reduced to [-1/2, 1/2] here (t - rint(t)) and sinpi / cospi see |2r| <= 1: the build's -ffast-math may
// not be trusted with the reduction of a 40-rad argument.  One block per (row, batch), the C/2 features over the threads.
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(128) void wg_prompt_sparse_kernel(const float* coords, const int* labels, int N, int pad, const float* boxes,
                                                               const void* text, int T, int text_bf16, const float* G, const float* table,
                                                               int C, float inv_h, float inv_w, float img_h, float img_w, float* out, int R) {
    const int r = blockIdx.x, b = blockIdx.y;
    const int F = C / 2;
    const int Np = coords ? N + pad : 0;
    const int nbox = boxes ? 2 : 0;
    float* o = out + ((long)b * R + r) * C;
    if (r >= Np + nbox) {                                   // text rows: copied (prompt_encoder.py:175-176)
        const long src = ((long)b * T + (r - Np - nbox)) * C;
        for (int c = threadIdx.x; c < C; c += blockDim.x)
            o[c] = text_bf16 ? (float)((const bf16*)text)[src + c] : ((const float*)text)[src + c];
        return;
    }
    float x, y;
    int add;                                                // row of `table` added: 0..3 point_embeddings, 4 not_a_point, -1 none
    bool zero_pe = false;
    if (r < Np) {
        int label;
        if (r < N) {
            x = coords[((long)b * N + r) * 2] + 0.5f;      // :86 shift to the pixel centre
            y = coords[((long)b * N + r) * 2 + 1] + 0.5f;
            label = labels[(long)b * N + r];
        } else {                                            // :87-91 the padding point, appended after the shift
            x = 0.f; y = 0.f; label = -1;
        }
        zero_pe = label == -1;                              // :95-98
        add = label == -1 ? 4 : (label == 0 ? 0 : (label == 1 ? 1 : -1));
    } else {
        const int k = r - Np;                               // :104-109 corner k adds point_embeddings[2 + k]
        x = boxes[(long)b * 4 + 2 * k] + 0.5f;
        y = boxes[(long)b * 4 + 2 * k + 1] + 0.5f;
        add = 2 + k;
    }
    // forward_with_coords divides x by W and y by H; under -ffast-math a division may become a reciprocal multiply: the host passes both
    // and the true quotient is formed with one correction step (x - q W is exact enough in fp32 to land on the IEEE quotient)
    float qx = x * inv_w, qy = y * inv_h;
    qx = fmaf(fmaf(-qx, img_w, x), inv_w, qx);
    qy = fmaf(fmaf(-qy, img_h, y), inv_h, qy);
    const float cx = 2.f * qx - 1.f, cy = 2.f * qy - 1.f;
    const float* e = add >= 0 ? table + (long)add * C : nullptr;
    for (int f = threadIdx.x; f < F; f += blockDim.x) {
        float s = 0.f, co = 0.f;
        if (!zero_pe) {
            const float t = fmaf(cy, G[F + f], cx * G[f]);
            const float red = t - rintf(t);
            s = sinpif(2.f * red);
            co = cospif(2.f * red);
        }
        if (e) { s += e[f]; co += e[F + f]; }
        o[f] = s;
        o[F + f] = co;
    }
}

extern "C" int wg_prompt_sparse_f32(const float* coords, const int* labels, int B, int N, int pad, const float* boxes, const void* text, int T,
                                    int text_bf16, const float* gaussian, const float* embed_table, int C, int img_h, int img_w, float* out,
                                    void* stream) {
    WG_REQUIRE(gaussian && embed_table && out && B > 0 && C > 0 && C % 2 == 0 && img_h > 0 && img_w > 0, "prompt_sparse: bad arguments");
    WG_REQUIRE(!coords || (labels && N > 0 && (pad == 0 || pad == 1)), "prompt_sparse: points need labels and N > 0");
    WG_REQUIRE(!text || T > 0, "prompt_sparse: text rows need T > 0");
    WG_REQUIRE(coords || boxes, "prompt_sparse: neither points nor boxes");
    const int R = (coords ? N + pad : 0) + (boxes ? 2 : 0) + (text ? T : 0);
    hipLaunchKernelGGL(wg_prompt_sparse_kernel, dim3(R, B), dim3(128), 0, (hipStream_t)stream, coords, labels, coords ? N : 0, coords ? pad : 0,
                       boxes, text, text ? T : 0, text_bf16, gaussian, embed_table, C, 1.0f / (float)img_h, 1.0f / (float)img_w, (float)img_h,
                       (float)img_w, out, R);
    return wg_check_launch("wg_prompt_sparse_f32");
}

// ------------------------------------------------------------------------------------------------------------
// mask_downscaling, fused per output pixel.  params (fp32, WG_MASK_PARAMS floats):
//   w1 [4][2][2] | b1 [4] | ln1 gain [4] | ln1 bias [4] | w2 [16][4][2][2] | b2 [16] | ln2 gain [16] | ln2 bias [16] | w3 [256][16] | b3 [256]
// Each wave takes 64 output pixels: lane l runs stages 1-4 (conv 2x2 s2 -> LN -> GELU -> conv 2x2 s2 -> LN -> GELU) on pixel l's 4x4 patch
// in fp32 and leaves the 16-vector in LDS; then, pixel by pixel, lane l forms output channels 4l..4l+3 from the broadcast 16-vector
// with their 16x4 weights in registers, so the wave writes one pixel's 256 bf16 (512 B) contiguously.
// ------------------------------------------------------------------------------------------------------------
#define WG_MASK_PARAMS (16 + 12 + 256 + 48 + 4096 + 256)

__device__ __forceinline__ float wg_gelu_erf(float x) { return 0.5f * x * (1.0f + wg_erf(x * 0.70710678118654752440f)); }

__global__ __launch_bounds__(256) void wg_mask_embed_kernel(const float* masks, const float* prm, float eps1, float eps2, bf16* out,
                                                            long npix, int h, int w) {
    __shared__ float vec[4][64][17];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long base = ((long)blockIdx.x * 4 + wave) * 64;
    const long p = base + lane;
    const float *w1 = prm, *b1 = prm + 16, *g1 = prm + 20, *be1 = prm + 24, *w2 = prm + 28, *b2 = prm + 284, *g2 = prm + 300,
                *be2 = prm + 316, *w3 = prm + 332, *b3 = prm + 4428;
    if (p < npix) {
        const int x = (int)(p % w);
        const long by = p / w;                              // b * h + y
        const long W4 = 4L * w;
        const float* src = masks + by * 4 * W4 + 4L * x;    // row 4y of image b (H = 4h rows of 4w)
        float in[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const f32x4 v = *(const f32x4*)(src + i * W4);
            in[i][0] = v[0]; in[i][1] = v[1]; in[i][2] = v[2]; in[i][3] = v[3];
        }
        float a1[4][2][2];                                  // [channel][sy][sx] after conv1 + LN + GELU
#pragma unroll
        for (int sy = 0; sy < 2; ++sy)
#pragma unroll
            for (int sx = 0; sx < 2; ++sx) {
                float v[4], mean = 0.f;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    v[c] = b1[c] + w1[4 * c] * in[2 * sy][2 * sx] + w1[4 * c + 1] * in[2 * sy][2 * sx + 1] + w1[4 * c + 2] * in[2 * sy + 1][2 * sx] +
                           w1[4 * c + 3] * in[2 * sy + 1][2 * sx + 1];
                    mean += v[c];
                }
                mean *= 0.25f;
                float var = 0.f;
#pragma unroll
                for (int c = 0; c < 4; ++c) var += (v[c] - mean) * (v[c] - mean);
                const float rs = 1.0f / sqrtf(var * 0.25f + eps1);
#pragma unroll
                for (int c = 0; c < 4; ++c) a1[c][sy][sx] = wg_gelu_erf(g1[c] * ((v[c] - mean) * rs) + be1[c]);
            }
        float v2[16], mean = 0.f;
#pragma unroll
        for (int o = 0; o < 16; ++o) {
            float s = b2[o];
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int k = 0; k < 4; ++k) s += w2[o * 16 + c * 4 + k] * a1[c][k >> 1][k & 1];
            v2[o] = s;
            mean += s;
        }
        mean *= 1.0f / 16.0f;
        float var = 0.f;
#pragma unroll
        for (int o = 0; o < 16; ++o) var += (v2[o] - mean) * (v2[o] - mean);
        const float rs = 1.0f / sqrtf(var * (1.0f / 16.0f) + eps2);
#pragma unroll
        for (int o = 0; o < 16; ++o) vec[wave][lane][o] = wg_gelu_erf(g2[o] * ((v2[o] - mean) * rs) + be2[o]);
    }
    float wr[4][16], br[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        br[j] = b3[4 * lane + j];
#pragma unroll
        for (int i = 0; i < 16; ++i) wr[j][i] = w3[(4 * lane + j) * 16 + i];
    }
    __syncthreads();
    const int n = npix - base < 64 ? (int)(npix - base) : 64;
    for (int q = 0; q < n; ++q) {
        float acc[4] = {br[0], br[1], br[2], br[3]};
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float a = vec[wave][q][i];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = fmaf(wr[j][i], a, acc[j]);
        }
        bf16x4 ov;
#pragma unroll
        for (int j = 0; j < 4; ++j) ov[j] = (bf16)acc[j];
        *(bf16x4*)(out + (base + q) * 256 + 4 * lane) = ov;
    }
}

extern "C" int wg_mask_embed_bf16(const float* masks, const float* params, float eps1, float eps2, void* out, int B, int h, int w, int mask_in_chans,
                                  int embed_dim, void* stream) {
    if (mask_in_chans != 16 || embed_dim != 256) {
        wg_set_error("mask_embed: built for mask_in_chans 16, embed_dim 256 (got %d, %d)", mask_in_chans, embed_dim);
        return WG_ERR_UNSUPPORTED;
    }
    WG_REQUIRE(masks && params && out && B > 0 && h > 0 && w > 0, "mask_embed: bad arguments");
    WG_REQUIRE(((unsigned long)masks & 15) == 0 && ((unsigned long)out & 7) == 0, "mask_embed: masks must be 16-byte, out 8-byte aligned");
    const long npix = (long)B * h * w;
    const long blocks = (npix + 255) / 256;
    WG_REQUIRE(blocks < (1L << 31), "mask_embed: too many pixels");
    hipLaunchKernelGGL(wg_mask_embed_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, masks, params, eps1, eps2, (bf16*)out, npix,
                       h, w);
    return wg_check_launch("wg_mask_embed_bf16");
}

// ------------------------------------------------------------------------------------------------------------
// Sam.preprocess: x [B,3,H,W] (uint8 or fp32) -> out [B,3,S,S] bf16 = pad((x - mean_c) / std_c), zeros outside H x W.
// ------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void wg_normalize_pad_kernel(const T* x, const float* mean, const float* stdv, bf16* out, int H, int W, int S,
                                                               long total) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int xo = (int)(i % S);
        const int yo = (int)((i / S) % S);
        const long bc = i / ((long)S * S);                  // b * 3 + c
        float v = 0.f;
        if (yo < H && xo < W) {
            const int c = (int)(bc % 3);
            v = ((float)x[(bc * H + yo) * W + xo] - mean[c]) / stdv[c];
        }
        out[i] = (bf16)v;
    }
}

extern "C" int wg_normalize_pad_bf16(const void* x, int x_u8, const float* mean, const float* stdv, void* out, int B, int H, int W, int S,
                                     void* stream) {
    WG_REQUIRE(x && mean && stdv && out && B > 0 && H > 0 && W > 0 && H <= S && W <= S, "normalize_pad: bad arguments");
    const long total = (long)B * 3 * S * S;
    const int blocks = (int)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
    if (x_u8)
        hipLaunchKernelGGL(wg_normalize_pad_kernel<unsigned char>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const unsigned char*)x, mean,
                           stdv, (bf16*)out, H, W, S, total);
    else
        hipLaunchKernelGGL(wg_normalize_pad_kernel<float>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const float*)x, mean, stdv,
                           (bf16*)out, H, W, S, total);
    return wg_check_launch("wg_normalize_pad_bf16");
}
