// The LLaMA generate path (walkgpt_amd/llama_hip.py): RMSNorm, RoPE + KV-cache write, causal prefill attention, split-key decode
// attention, the decode GEMV -- on bf16 weights and, for the e4m3 weight-only mode, on e4m3 bytes with a scale per row (section e2, with
// its quantiser and dequantiser) -- and the device-side token pick.  bf16 data, fp32 arithmetic, no float atomics, every sum in a fixed
// order (a run repeats bit for bit).  No launch function allocates or synchronises: all of them run inside a graph capture.
//
// Device state of a generation (int32, read by the kernels so that a captured decode step bakes in no length):
//   past_len   prefill / rope_cache: the number of tokens already in the cache (token j of the call sits at position past_len + j);
//              decode attention and the pick: the position of the CURRENT token -- its query sees keys 0 .. past_len.  The pick sets
//              mask[row][past_len + 1] and increments it, so the next step's token lands on the next slot.
//   n_new      how many tokens the pick has emitted.
// Every index derived from that state is clamped to the cache capacity `cap` (or to the table it indexes) inside the kernel: a stale
// or garbage state gives wrong numbers, never an access outside the buffers.
//
// Cache layout: K and V are [rows, cap, H] bf16 (H = heads * 128), position-major, one pair per layer; cap % 64 == 0.
// Key mask: uint8 [rows, cap], 1 = attend, the same for every query of a row.
#include "wg_common.h"

#define WG_LLAMA_HD 128
#define WG_LLAMA_SPLITS 8        // key splits of the decode attention (fixed: the combine order must not depend on the shape)
#define WG_LLAMA_PART 132        // floats per decode partial: o[128], m, l, 2 pad (keeps rows 16-byte aligned)
#define WG_NEG_BIG (-1.0e30f)

__device__ __forceinline__ int wg_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ long wg_clampl(long v, long lo, long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- a. RMSNorm ---------------------------------------------------------------------------------------------------------------------
// y = x * rsqrt(mean(x^2) + eps) * w, one rounding (to bf16) at the end.  One 256-thread block per row.
// slot != null: row r is written to y + r * y_bs + clamp(*slot + slot_add, 0, slot_cap - 1) * ldy (the decode step's hidden-state slot).
__global__ __launch_bounds__(256) void wg_rmsnorm_rows_kernel(const bf16* x, long ldx, const bf16* w, bf16* y, long ldy, int D, float eps,
                                                              const int* slot, int slot_add, int slot_cap, long y_bs) {
    __shared__ float red[4];
    const int row = blockIdx.x, tid = threadIdx.x;
    const bf16* xr = x + (long)row * ldx;
    float ss = 0.f;
    for (int k = tid * 8; k < D; k += 2048) {
        const bf16x8 t = *(const bf16x8*)(xr + k);
#pragma unroll
        for (int e = 0; e < 8; ++e) ss += (float)t[e] * (float)t[e];
    }
    ss = wg_wave_sum(ss);
    if ((tid & 63) == 0) red[tid >> 6] = ss;
    __syncthreads();
    const float rstd = 1.0f / sqrtf(((red[0] + red[1]) + (red[2] + red[3])) / (float)D + eps);
    bf16* yr = slot ? y + (long)row * y_bs + wg_clampl((long)*slot + slot_add, 0, slot_cap - 1) * ldy : y + (long)row * ldy;
    for (int k = tid * 8; k < D; k += 2048) {
        const bf16x8 t = *(const bf16x8*)(xr + k), g = *(const bf16x8*)(w + k);
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (bf16)((float)t[e] * rstd * (float)g[e]);
        *(bf16x8*)(yr + k) = o;
    }
}

extern "C" int wg_rmsnorm_rows_bf16(const void* x, long ldx, const void* w, void* y, long ldy, int M, int D, float eps, const int* slot,
                                    int slot_add, int slot_cap, long y_batch_stride, void* stream) {
    WG_REQUIRE(x && w && y, "rmsnorm: null operand");
    WG_REQUIRE(M > 0 && D > 0 && D % 8 == 0, "rmsnorm: bad shape (M %d, D %d; D must be a multiple of 8)", M, D);
    WG_REQUIRE(ldx >= D && ldy >= D && ldx % 8 == 0 && ldy % 8 == 0, "rmsnorm: leading dimensions must be multiples of 8 and >= D");
    WG_REQUIRE((((uintptr_t)x | (uintptr_t)w | (uintptr_t)y) & 15) == 0, "rmsnorm: misaligned operand");
    WG_REQUIRE(!slot || (slot_cap > 0 && y_batch_stride >= (long)slot_cap * ldy), "rmsnorm: slot output needs slot_cap rows inside y_batch_stride");
    hipLaunchKernelGGL(wg_rmsnorm_rows_kernel, dim3(M), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, ldx, (const bf16*)w, (bf16*)y, ldy, D, eps,
                       slot, slot_add, slot_cap, y_batch_stride);
    return wg_check_launch("wg_rmsnorm_rows_bf16");
}

// ---- b. RoPE + cache write ----------------------------------------------------------------------------------------------------------
// One thread per (token, head, 8 of the 64 rotation pairs): pair (i, i + 64) as transformers' rotate_half,
//   out[i] = x[i] cos[i] - x[i + 64] sin[i],   out[i + 64] = x[i + 64] cos[i] + x[i] sin[i]      (fp32, one rounding)
// q -> q_out [rows L, H]; rotated k and plain v -> the cache slot of position past_len + j.  A position outside [0, cap) writes no cache
// slot (and reads the table's last row).
// LoRA form (wg_llama_rope_cache_lora_bf16): the up-projection of unmerged adapters rides in here.  Before the rotation (for v: before
// the copy) the adapted ones of q, k, v become, in fp32,  x[n] + s * sum_j B[n][j] t[tok][seg * rank + j]  (j ascending; B [H, rank]
// bf16, its row rank / 8 16-byte loads; t fp32 [rows L, 3 rank], the down-projections the q | k | v GEMV left):
//   q = bf16(rope(bf16(W_q xh) + s B_q t_q)), the same for k;  v = bf16(bf16(W_v xh) + s B_v t_v).
// An unadapted v stays a copy and an unadapted q / k takes the arithmetic above.
struct RopeArgs {
    const bf16* qkv; long ldqkv;
    const float* cos; const float* sin; int max_pos;
    const int* past_len;
    bf16* q_out; long ldq;
    bf16* kc; bf16* vc;
    int rows, L, heads, cap;
};

__device__ __forceinline__ void wg_rope8(const bf16x8 lo, const bf16x8 hi, const float* c, const float* s, bf16x8& olo, bf16x8& ohi) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float a = (float)lo[e], b = (float)hi[e];
        olo[e] = (bf16)(a * c[e] - b * s[e]);
        ohi[e] = (bf16)(b * c[e] + a * s[e]);
    }
}

struct RopeLoraArgs : RopeArgs {
    const float* t; long ldt;
    const bf16* b[3]; float s[3];
    int rank;
};

// d[0 .. 7] / d[8 .. 15] = s * B[col + e] . t / s * B[col + 64 + e] . t, the adapter's term of this thread's 16 elements of projection `seg`
// (j ascending).  The 16 rows of B are loaded together (16 bytes each per 8 columns of B) and the t slice once per thread.
__device__ __forceinline__ void wg_lora_up16(const RopeLoraArgs& a, int seg, long tok, int col, float* d) {
#pragma unroll
    for (int e = 0; e < 16; ++e) d[e] = 0.f;
    const bf16* b = a.b[seg] + (long)col * a.rank;
    const float* t = a.t + tok * a.ldt + seg * a.rank;
    for (int j = 0; j < a.rank; j += 8) {
        bf16x8 bv[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) bv[e] = *(const bf16x8*)(b + (long)((e & 7) + (e >> 3) * 64) * a.rank + j);
        const f32x4 t0 = *(const f32x4*)(t + j), t1 = *(const f32x4*)(t + j + 4);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
#pragma unroll
            for (int u = 0; u < 4; ++u) d[e] += (float)bv[e][u] * t0[u];
#pragma unroll
            for (int u = 0; u < 4; ++u) d[e] += (float)bv[e][4 + u] * t1[u];
        }
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) d[e] *= a.s[seg];
}

// The LoRA form's rotation: the operations are spelled out as the plain kernel's wg_rope8 compiles (one product, one fma each, in this
// pairing), so a projection without an adapter -- or with B = 0 -- gives the plain kernel's bits.  That rests on how the compiler contracts
// a * c - b * s in wg_rope8; what pins it are the GPU tests (tests/test_gpu_lora.py: all B null against the plain entry point, B = 0
// against the plain model): if a compiler pairs wg_rope8 differently, they fail and this function follows it.
__device__ __forceinline__ void wg_rope8f(const float* lo, const float* hi, const float* c, const float* s, bf16x8& olo, bf16x8& ohi) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        olo[e] = (bf16)__builtin_fmaf(lo[e], c[e], -(hi[e] * s[e]));
        ohi[e] = (bf16)__builtin_fmaf(hi[e], c[e], lo[e] * s[e]);
    }
}

// q or k of the LoRA form: lo / hi are this thread's two 8-element pieces of the projection, d is wg_lora_up16's, added where the projection has an adapter
__device__ __forceinline__ void wg_rope8_lora(const bf16x8 lo, const bf16x8 hi, const float* d, bool adapted, const float* c, const float* s,
                                              bf16x8& olo, bf16x8& ohi) {
    float fl[8], fh[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { fl[e] = (float)lo[e]; fh[e] = (float)hi[e]; }
    if (adapted) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { fl[e] += d[e]; fh[e] += d[8 + e]; }
    }
    wg_rope8f(fl, fh, c, s, olo, ohi);
}

// The LoRA form runs one thread per (token, head, 8 pairs, projection): blockIdx.y = 0 / 1 / 2 takes q / k / v alone.  The decode step has
// rows * heads * 8 such threads per projection -- one workgroup -- so what the kernel costs there is its chain of dependent trips to
// memory, not bytes; with a projection per workgroup the B rows, the t slice and the x pieces of a thread are all in flight at once and
// the chain is as long as the plain kernel's.
template <bool LORA>
__global__ __launch_bounds__(256) void wg_llama_rope_cache_kernel(std::conditional_t<LORA, RopeLoraArgs, RopeArgs> a) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long total = (long)a.rows * a.L * a.heads * 8;
    if (i >= total) return;
    const int c8 = (int)(i & 7);
    const int head = (int)((i >> 3) % a.heads);
    const long tok = (i >> 3) / a.heads;            // row * L + j
    const int j = (int)(tok % a.L), row = (int)(tok / a.L);
    const int H = a.heads * WG_LLAMA_HD;
    const long pos = (long)*a.past_len + j;
    const int tp = (int)(pos < 0 ? 0 : (pos > a.max_pos - 1 ? a.max_pos - 1 : pos));
    float c[8], s[8];
    {
        const f32x4* cp = (const f32x4*)(a.cos + (long)tp * 64 + c8 * 8);
        const f32x4* sp = (const f32x4*)(a.sin + (long)tp * 64 + c8 * 8);
        const f32x4 c0 = cp[0], c1 = cp[1], s0 = sp[0], s1 = sp[1];
#pragma unroll
        for (int e = 0; e < 4; ++e) { c[e] = c0[e]; c[4 + e] = c1[e]; s[e] = s0[e]; s[4 + e] = s1[e]; }
    }
    const bf16* src = a.qkv + tok * a.ldqkv + head * WG_LLAMA_HD + c8 * 8;
    bf16x8 olo, ohi;
    if constexpr (LORA) {
        const int seg = blockIdx.y;
        const bool adapted = a.b[seg] != nullptr;
        const bf16x8 lo = *(const bf16x8*)(src + seg * H), hi = *(const bf16x8*)(src + seg * H + 64);
        float d[16];
        if (adapted) wg_lora_up16(a, seg, tok, head * WG_LLAMA_HD + c8 * 8, d);
        if (seg == 0) {
            wg_rope8_lora(lo, hi, d, adapted, c, s, olo, ohi);
            bf16* qo = a.q_out + tok * a.ldq + head * WG_LLAMA_HD + c8 * 8;
            *(bf16x8*)qo = olo;
            *(bf16x8*)(qo + 64) = ohi;
            return;
        }
        if (pos < 0 || pos >= a.cap) return;
        const long slot = ((long)row * a.cap + pos) * H + head * WG_LLAMA_HD + c8 * 8;
        if (seg == 1) {
            wg_rope8_lora(lo, hi, d, adapted, c, s, olo, ohi);
            *(bf16x8*)(a.kc + slot) = olo;
            *(bf16x8*)(a.kc + slot + 64) = ohi;
            return;
        }
        olo = lo; ohi = hi;
        if (adapted) {
#pragma unroll
            for (int e = 0; e < 8; ++e) { olo[e] = (bf16)((float)lo[e] + d[e]); ohi[e] = (bf16)((float)hi[e] + d[8 + e]); }
        }
        *(bf16x8*)(a.vc + slot) = olo;
        *(bf16x8*)(a.vc + slot + 64) = ohi;
        return;
    }
    wg_rope8(*(const bf16x8*)src, *(const bf16x8*)(src + 64), c, s, olo, ohi);
    bf16* qo = a.q_out + tok * a.ldq + head * WG_LLAMA_HD + c8 * 8;
    *(bf16x8*)qo = olo;
    *(bf16x8*)(qo + 64) = ohi;
    if (pos < 0 || pos >= a.cap) return;
    const long slot = ((long)row * a.cap + pos) * H + head * WG_LLAMA_HD + c8 * 8;
    wg_rope8(*(const bf16x8*)(src + H), *(const bf16x8*)(src + H + 64), c, s, olo, ohi);
    *(bf16x8*)(a.kc + slot) = olo;
    *(bf16x8*)(a.kc + slot + 64) = ohi;
    *(bf16x8*)(a.vc + slot) = *(const bf16x8*)(src + 2 * H);
    *(bf16x8*)(a.vc + slot + 64) = *(const bf16x8*)(src + 2 * H + 64);
}

static int wg_llama_rope_cache_check(const char* word, const void* qkv, long ldqkv, const float* cos_table, const float* sin_table, int max_pos,
                                     const int* past_len, const void* q_out, long ldq, const void* k_cache, const void* v_cache, int rows, int L,
                                     int heads, int cap) {
    WG_REQUIRE(qkv && cos_table && sin_table && past_len && q_out && k_cache && v_cache, "%s: null operand", word);
    WG_REQUIRE(rows > 0 && L > 0 && heads > 0 && max_pos > 0, "%s: bad shape", word);
    WG_REQUIRE(cap > 0 && cap % 64 == 0, "%s: cache capacity %d must be a positive multiple of 64", word, cap);
    const long H = (long)heads * WG_LLAMA_HD;
    WG_REQUIRE(ldqkv >= 3 * H && ldq >= H && ldqkv % 8 == 0 && ldq % 8 == 0, "%s: leading dimensions too small or not multiples of 8", word);
    WG_REQUIRE((((uintptr_t)qkv | (uintptr_t)cos_table | (uintptr_t)sin_table | (uintptr_t)q_out | (uintptr_t)k_cache | (uintptr_t)v_cache) & 15) == 0,
               "%s: misaligned operand", word);
    return 0;
}

extern "C" int wg_llama_rope_cache_bf16(const void* qkv, long ldqkv, const float* cos_table, const float* sin_table, int max_pos,
                                        const int* past_len, void* q_out, long ldq, void* k_cache, void* v_cache, int rows, int L, int heads,
                                        int cap, void* stream) {
    if (const int rc = wg_llama_rope_cache_check("llama_rope_cache", qkv, ldqkv, cos_table, sin_table, max_pos, past_len, q_out, ldq, k_cache,
                                                 v_cache, rows, L, heads, cap)) return rc;
    RopeArgs a{(const bf16*)qkv, ldqkv, cos_table, sin_table, max_pos, past_len, (bf16*)q_out, ldq, (bf16*)k_cache, (bf16*)v_cache, rows, L, heads, cap};
    const long total = (long)rows * L * heads * 8;
    hipLaunchKernelGGL(wg_llama_rope_cache_kernel<false>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return wg_check_launch("wg_llama_rope_cache_bf16");
}

extern "C" int wg_llama_rope_cache_lora_bf16(const void* qkv, long ldqkv, const float* cos_table, const float* sin_table, int max_pos,
                                             const int* past_len, void* q_out, long ldq, void* k_cache, void* v_cache, int rows, int L, int heads,
                                             int cap, const float* t, long ldt, const void* b_q, const void* b_k, const void* b_v, float s_q,
                                             float s_k, float s_v, int rank, void* stream) {
    if (const int rc = wg_llama_rope_cache_check("llama_rope_cache_lora", qkv, ldqkv, cos_table, sin_table, max_pos, past_len, q_out, ldq, k_cache,
                                                 v_cache, rows, L, heads, cap)) return rc;
    WG_REQUIRE(rank >= 8 && rank <= 64 && rank % 8 == 0, "llama_rope_cache_lora: rank %d must be a multiple of 8, at most 64", rank);
    if (b_q || b_k || b_v) {
        WG_REQUIRE(t, "llama_rope_cache_lora: null operand (t, with an adapter given)");
        WG_REQUIRE(ldt >= 3L * rank && ldt % 4 == 0, "llama_rope_cache_lora: ldt %ld too small for [rows L, 3 rank] (or not a multiple of 4)", ldt);
        WG_REQUIRE((((uintptr_t)t | (uintptr_t)b_q | (uintptr_t)b_k | (uintptr_t)b_v) & 15) == 0, "llama_rope_cache_lora: misaligned B / t");
    }
    RopeLoraArgs a{{(const bf16*)qkv, ldqkv, cos_table, sin_table, max_pos, past_len, (bf16*)q_out, ldq, (bf16*)k_cache, (bf16*)v_cache, rows, L, heads,
                    cap}, t, ldt, {(const bf16*)b_q, (const bf16*)b_k, (const bf16*)b_v}, {s_q, s_k, s_v}, rank};
    const long total = (long)rows * L * heads * 8;
    hipLaunchKernelGGL(wg_llama_rope_cache_kernel<true>, dim3((unsigned)((total + 255) / 256), 3), dim3(256), 0, (hipStream_t)stream, a);
    return wg_check_launch("wg_llama_rope_cache_lora_bf16");
}

// ---- c. prefill attention -----------------------------------------------------------------------------------------------------------
// Flash-style, one wave per (32 queries, head, row), 32 keys per step.  The score product is taken swapped, S^T = K Q^T
// (mfma_f32_32x32x16_bf16, A = K rows and B = Q rows, both 16-byte loads straight from memory), so a lane holds 16 scores of ONE query
// (column = lane & 31; the other 16 keys sit in lane ^ 32) and the running max / sum are per lane.  P is rounded to bf16 and is, as it
// stands in the accumulator registers, the B operand of O^T = V^T P^T; the V^T fragments are gathered from a [32][128] LDS image of
// the V tile.  The row sum is taken from the unrounded P.  Query j sits at position past + j and sees keys <= its position whose mask
// byte is set.  V rows beyond the block's last visible key are staged as zeros (an unwritten cache slot may hold anything).
struct PrefillArgs {
    const bf16* q; long ldq;
    const bf16* kc; const bf16* vc;
    const unsigned char* mask;
    bf16* out; long ldo;
    const int* past_len;
    int rows, L, heads, cap;
    float scale2;             // softmax scale * log2(e)
};

__global__ __launch_bounds__(64) void wg_llama_attn_prefill_kernel(PrefillArgs a) {
    __shared__ __attribute__((aligned(16))) bf16 Vs[32][136];
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const int qb = blockIdx.x, head = blockIdx.y, row = blockIdx.z;
    const int H = a.heads * WG_LLAMA_HD;
    const int past = wg_clampi(*a.past_len, 0, a.cap - a.L);
    const int qi = qb * 32 + r;
    const int qc = qi < a.L ? qi : a.L - 1;
    const int qpos = past + qc;
    const int qlast = qb * 32 + 31 < a.L ? qb * 32 + 31 : a.L - 1;
    const int kmax = past + qlast;                      // the block's last visible key; < cap
    bf16x8 qf[8];
    {
        const bf16* qp = a.q + ((long)row * a.L + qc) * a.ldq + head * WG_LLAMA_HD + 8 * h;
#pragma unroll
        for (int s = 0; s < 8; ++s) qf[s] = *(const bf16x8*)(qp + 16 * s);
    }
    f32x16 ot[4];
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int e = 0; e < 16; ++e) ot[d][e] = 0.f;
    float m = WG_NEG_BIG, l = 0.f;
    const bf16* kb = a.kc + (long)row * a.cap * H + head * WG_LLAMA_HD;
    const bf16* vb = a.vc + (long)row * a.cap * H + head * WG_LLAMA_HD;
    const unsigned char* mk = a.mask + (long)row * a.cap;

    for (int key0 = 0; key0 <= kmax; key0 += 32) {
        __syncthreads();                                 // the previous step's fragment reads are done
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const int kr = p * 4 + (lane >> 4), key = key0 + kr, d = (lane & 15) * 8;
            bf16x8 v;
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (bf16)0.f;
            if (key <= kmax) v = *(const bf16x8*)(vb + (long)key * H + d);
            *(bf16x8*)&Vs[kr][d] = v;
        }
        f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
        {
            const int kk = key0 + r <= kmax ? key0 + r : kmax;
            const bf16* kp = kb + (long)kk * H + 8 * h;
#pragma unroll
            for (int s = 0; s < 8; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const bf16x8*)(kp + 16 * s), qf[s], acc, 0, 0, 0);
        }
        __syncthreads();                                 // the V image is complete
        float sc[16], tmax = WG_NEG_BIG;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int kbase = key0 + 8 * g + 4 * h;      // key0 + 31 < cap: cap is a multiple of 64 and key0 <= kmax < cap
            const unsigned mw = *(const unsigned*)(mk + kbase);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool ok = kbase + e <= qpos && ((mw >> (8 * e)) & 0xffu) != 0;
                sc[4 * g + e] = ok ? acc[4 * g + e] * a.scale2 : WG_NEG_BIG;
                tmax = fmaxf(tmax, sc[4 * g + e]);
            }
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
        const float mn = fmaxf(m, tmax);
        const float alpha = exp2f(m - mn);
        m = mn;
        bf16x8 pf[2];
        float ps = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float p = sc[e] > -1.0e29f ? exp2f(sc[e] - mn) : 0.f;
            ps += p;
            pf[e >> 3][e & 7] = (bf16)p;
        }
        l = l * alpha + ps;
#pragma unroll
        for (int d = 0; d < 4; ++d)
#pragma unroll
            for (int e = 0; e < 16; ++e) ot[d][e] *= alpha;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                bf16x8 vf;
#pragma unroll
                for (int j = 0; j < 8; ++j) vf[j] = Vs[16 * ks + 8 * (j >> 2) + 4 * h + (j & 3)][32 * d + r];
                ot[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf[ks], ot[d], 0, 0, 0);
            }
    }
    l += __shfl_xor(l, 32, 64);
    const float inv = l > 0.f ? 1.0f / l : 0.f;
    if (qi < a.L) {
        bf16* op = a.out + ((long)row * a.L + qi) * a.ldo + head * WG_LLAMA_HD + 4 * h;
#pragma unroll
        for (int d = 0; d < 4; ++d)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                bf16x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = (bf16)(ot[d][4 * g + e] * inv);
                *(bf16x4*)(op + 32 * d + 8 * g) = o;
            }
    }
}

extern "C" int wg_llama_attn_prefill_bf16(const void* q, long ldq, const void* k_cache, const void* v_cache, const unsigned char* mask, void* out,
                                          long ldo, const int* past_len, int rows, int L, int heads, int cap, float scale, void* stream) {
    WG_REQUIRE(q && k_cache && v_cache && mask && out && past_len, "llama_attn_prefill: null operand");
    WG_REQUIRE(rows > 0 && rows <= 65535 && L > 0 && heads > 0 && heads <= 65535, "llama_attn_prefill: bad shape");
    WG_REQUIRE(cap > 0 && cap % 64 == 0 && L <= cap, "llama_attn_prefill: capacity %d must be a multiple of 64 and >= L = %d", cap, L);
    const long H = (long)heads * WG_LLAMA_HD;
    WG_REQUIRE(ldq >= H && ldo >= H && ldq % 8 == 0 && ldo % 8 == 0, "llama_attn_prefill: leading dimensions too small or not multiples of 8");
    WG_REQUIRE((((uintptr_t)q | (uintptr_t)k_cache | (uintptr_t)v_cache | (uintptr_t)out) & 15) == 0 && ((uintptr_t)mask & 3) == 0,
               "llama_attn_prefill: misaligned operand");
    PrefillArgs a{(const bf16*)q, ldq, (const bf16*)k_cache, (const bf16*)v_cache, mask, (bf16*)out, ldo, past_len, rows, L, heads, cap,
                  scale * 1.4426950408889634f};
    hipLaunchKernelGGL(wg_llama_attn_prefill_kernel, dim3((unsigned)((L + 31) / 32), heads, rows), dim3(64), 0, (hipStream_t)stream, a);
    return wg_check_launch("wg_llama_attn_prefill_bf16");
}

// ---- d. decode attention ------------------------------------------------------------------------------------------------------------
// One query per (row, head) over keys 0 .. past_len.  WG_LLAMA_SPLITS one-wave workgroups per (row, head): split s takes the 16-key
// groups s, s + SPLITS, ...  A lane owns 32 head dims of one key per step (K and V rows by 16-byte loads straight to registers) and a
// private online-softmax state; the wave merges its 16 key slots by a butterfly and leaves (o[128], m, l) in fp32.  The combine kernel
// adds the SPLITS partials of a (row, head) in index order.  P stays fp32 here.
struct DecodeArgs {
    const bf16* q; long ldq;
    const bf16* kc; const bf16* vc;
    const unsigned char* mask;
    float* part;
    bf16* out; long ldo;
    const int* past_len;
    int rows, heads, cap;
    float scale2;
};

__global__ __launch_bounds__(64) void wg_llama_attn_decode_kernel(DecodeArgs a) {
    const int lane = threadIdx.x, slot = lane >> 2, ds = lane & 3;
    const int split = blockIdx.x, head = blockIdx.y, row = blockIdx.z;
    const int H = a.heads * WG_LLAMA_HD;
    const int nkeys = (int)wg_clampl((long)*a.past_len + 1, 1, a.cap);
    const int dcol = head * WG_LLAMA_HD + ds * 32;
    float q[32], o[32];
    {
        const bf16* qp = a.q + (long)row * a.ldq + dcol;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const bf16x8 t = *(const bf16x8*)(qp + 8 * c);
#pragma unroll
            for (int e = 0; e < 8; ++e) q[8 * c + e] = (float)t[e] * a.scale2;
        }
    }
#pragma unroll
    for (int d = 0; d < 32; ++d) o[d] = 0.f;
    float m = WG_NEG_BIG, l = 0.f;
    const bf16* kb = a.kc + (long)row * a.cap * H + dcol;
    const bf16* vb = a.vc + (long)row * a.cap * H + dcol;
    const unsigned char* mk = a.mask + (long)row * a.cap;
    for (int j0 = split * 16; j0 < nkeys; j0 += 16 * WG_LLAMA_SPLITS) {
        const int j = j0 + slot;
        const int jc = j < nkeys ? j : nkeys - 1;
        const bool ok = j < nkeys && mk[jc] != 0;
        const bf16* kp = kb + (long)jc * H;
        const bf16* vp = vb + (long)jc * H;
        bf16x8 kk[4], vv[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) { kk[c] = *(const bf16x8*)(kp + 8 * c); vv[c] = *(const bf16x8*)(vp + 8 * c); }
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int e = 0; e < 8; ++e) s += q[8 * c + e] * (float)kk[c][e];
        s += __shfl_xor(s, 1, 64);
        s += __shfl_xor(s, 2, 64);
        if (ok) {
            const float mn = fmaxf(m, s);
            const float alpha = exp2f(m - mn), p = exp2f(s - mn);
            m = mn;
            l = l * alpha + p;
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int e = 0; e < 8; ++e) o[8 * c + e] = o[8 * c + e] * alpha + p * (float)vv[c][e];
        }
    }
#pragma unroll
    for (int w = 4; w < 64; w <<= 1) {
        const float m2 = __shfl_xor(m, w, 64), l2 = __shfl_xor(l, w, 64);
        const float mn = fmaxf(m, m2);
        const float a1 = exp2f(m - mn), a2 = exp2f(m2 - mn);
        l = l * a1 + l2 * a2;
#pragma unroll
        for (int d = 0; d < 32; ++d) {
            const float o2 = __shfl_xor(o[d], w, 64);
            o[d] = o[d] * a1 + o2 * a2;
        }
        m = mn;
    }
    if (slot == 0) {
        float* pp = a.part + (((long)row * a.heads + head) * WG_LLAMA_SPLITS + split) * WG_LLAMA_PART;
#pragma unroll
        for (int c = 0; c < 8; ++c) *(f32x4*)(pp + ds * 32 + 4 * c) = (f32x4){o[4 * c], o[4 * c + 1], o[4 * c + 2], o[4 * c + 3]};
        if (ds == 0) { pp[128] = m; pp[129] = l; }
    }
}

__global__ __launch_bounds__(128) void wg_llama_attn_combine_kernel(DecodeArgs a) {
    const int d = threadIdx.x, head = blockIdx.x, row = blockIdx.y;
    const float* pp = a.part + ((long)row * a.heads + head) * WG_LLAMA_SPLITS * WG_LLAMA_PART;
    float mx = WG_NEG_BIG;
#pragma unroll
    for (int s = 0; s < WG_LLAMA_SPLITS; ++s) mx = fmaxf(mx, pp[s * WG_LLAMA_PART + 128]);
    float l = 0.f, o = 0.f;
#pragma unroll
    for (int s = 0; s < WG_LLAMA_SPLITS; ++s) {
        const float w = exp2f(pp[s * WG_LLAMA_PART + 128] - mx);
        l += pp[s * WG_LLAMA_PART + 129] * w;
        o += pp[s * WG_LLAMA_PART + d] * w;
    }
    a.out[(long)row * a.ldo + head * WG_LLAMA_HD + d] = (bf16)(l > 0.f ? o / l : 0.f);
}

extern "C" long wg_llama_attn_decode_workspace_floats(int rows, int heads) {
    return (long)(rows > 0 ? rows : 0) * (heads > 0 ? heads : 0) * WG_LLAMA_SPLITS * WG_LLAMA_PART;
}

extern "C" int wg_llama_attn_decode_bf16(const void* q, long ldq, const void* k_cache, const void* v_cache, const unsigned char* mask,
                                         float* workspace, long workspace_floats, void* out, long ldo, const int* past_len, int rows, int heads,
                                         int cap, float scale, void* stream) {
    WG_REQUIRE(q && k_cache && v_cache && mask && workspace && out && past_len, "llama_attn_decode: null operand");
    WG_REQUIRE(rows > 0 && rows <= 65535 && heads > 0 && heads <= 65535, "llama_attn_decode: bad shape");
    WG_REQUIRE(cap > 0 && cap % 64 == 0, "llama_attn_decode: cache capacity %d must be a positive multiple of 64", cap);
    const long H = (long)heads * WG_LLAMA_HD;
    WG_REQUIRE(ldq >= H && ldo >= H && ldq % 8 == 0, "llama_attn_decode: leading dimensions too small or not multiples of 8");
    WG_REQUIRE(workspace_floats >= wg_llama_attn_decode_workspace_floats(rows, heads), "llama_attn_decode: workspace too small");
    WG_REQUIRE((((uintptr_t)q | (uintptr_t)k_cache | (uintptr_t)v_cache | (uintptr_t)workspace) & 15) == 0, "llama_attn_decode: misaligned operand");
    DecodeArgs a{(const bf16*)q, ldq, (const bf16*)k_cache, (const bf16*)v_cache, mask, workspace, (bf16*)out, ldo, past_len, rows, heads, cap,
                 scale * 1.4426950408889634f};
    hipLaunchKernelGGL(wg_llama_attn_decode_kernel, dim3(WG_LLAMA_SPLITS, heads, rows), dim3(64), 0, (hipStream_t)stream, a);
    int rc = wg_check_launch("wg_llama_attn_decode_bf16");
    if (rc != 0) return rc;
    hipLaunchKernelGGL(wg_llama_attn_combine_kernel, dim3(heads, rows), dim3(128), 0, (hipStream_t)stream, a);
    return wg_check_launch("wg_llama_attn_decode_bf16(combine)");
}

// ---- e. decode GEMV -----------------------------------------------------------------------------------------------------------------
// out[m][n] = sum_k xh[m][k] W[n][k] for M <= 8 rows; every weight element is read once, by non-temporal 16-byte loads straight to
// registers (no LDS on the weight path).  A wave owns 4 weight rows at a time (pair mode: 2 gate + 2 up rows); lane l takes the
// 8-element pieces l, l + 64, ... of each row, multiplies them with the matching pieces of the M input rows (those come from L2)
// and the wave adds its 64 lane sums by a fixed butterfly.  (Fewer rows per wave where N is small, i.e. more waves per CU, was
// measured on the 7B shapes: within 4 % for o_proj, down_proj and the SwiGLU pair, and 30 % slower for the q | k | v launch, whose
// every workgroup repeats the RMSNorm prologue; profiles/llm_generate.md.)  fp32 throughout; the only rounding is that of the output.
//   segments   up to three weight matrices (W_i [N_i, K]) are the column ranges [0, N_0), [N_0, N_0 + N_1), ... of one output
//   norm       xh = x * rstd(x row) * gamma, not rounded; every workgroup recomputes the M values of rstd (M K reads from L2)
//   residual   out = res + acc (res may be out)
//   pair       out[n] = silu(W_0[n] . xh) * (W_1[n] . xh)
//   out_f32    fp32 output (the logits)
//   lora       (wg_llama_gemv_lora_bf16) the rows of up to three adapter down-projections A_i [rank, K], A_i belonging to segment i, are
//              further weight rows of the same launch, after the last W row and in segment order: t[m][i * rank + j] = A_i[j] . xh[m],
//              fp32, not rounded (t [M, 3 rank]; the column block of an absent adapter is not written).  They take no residual.
struct GemvArgs {
    const bf16* x; long ldx;
    const bf16* w[3]; int n[3];
    int K;
    const bf16* gamma; float eps;
    const bf16* res; long ldr;
    void* out; long ldo;
    int out_f32;
};
struct GemvLoraArgs : GemvArgs {
    const bf16* la[3]; int rank;
    float* t; long ldt;
};

// LoRA row j (0 .. adapters * rank - 1, present adapters in segment order) -> its segment; j becomes the row inside that adapter
__device__ __forceinline__ int wg_lora_row_segment(const GemvLoraArgs& a, int& j) {
    int sgm = 0;
    if (!a.la[0] || j >= a.rank) {
        if (a.la[0]) j -= a.rank;
        sgm = 1;
        if (!a.la[1] || j >= a.rank) {
            if (a.la[1]) j -= a.rank;
            sgm = 2;
        }
    }
    return sgm;
}

template <int M, bool PAIR, bool LORA = false>
__global__ __launch_bounds__(256) void wg_llama_gemv_kernel(std::conditional_t<LORA, GemvLoraArgs, GemvArgs> a) {
    static_assert(!(PAIR && LORA), "pair mode takes no adapters");
    constexpr int R = 4;                    // weight rows in flight per wave
    constexpr int RO = PAIR ? 2 : 4;        // output columns per wave
    __shared__ float red[4][8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = a.K;
    float rstd[M];
#pragma unroll
    for (int m = 0; m < M; ++m) rstd[m] = 1.f;
    if (a.gamma) {
        float ss[M];
#pragma unroll
        for (int m = 0; m < M; ++m) ss[m] = 0.f;
        for (int k = tid * 8; k < K; k += 2048) {
#pragma unroll
            for (int m = 0; m < M; ++m) {
                const bf16x8 t = *(const bf16x8*)(a.x + (long)m * a.ldx + k);
#pragma unroll
                for (int e = 0; e < 8; ++e) ss[m] += (float)t[e] * (float)t[e];
            }
        }
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const float t = wg_wave_sum(ss[m]);
            if (lane == 0) red[wave][m] = t;
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < M; ++m) rstd[m] = 1.0f / sqrtf(((red[0][m] + red[1][m]) + (red[2][m] + red[3][m])) / (float)K + a.eps);
    }
    const int nw = PAIR ? a.n[0] : a.n[0] + a.n[1] + a.n[2];      // output columns of W; ntot: those plus the adapter rows
    int ntot = nw;
    if constexpr (LORA) ntot += ((a.la[0] != nullptr) + (a.la[1] != nullptr) + (a.la[2] != nullptr)) * a.rank;
    const int n0 = (blockIdx.x * 4 + wave) * RO;
    if (n0 >= ntot) return;                 // (after the only barrier)
    const bf16* wp[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if constexpr (PAIR) {
            const int n = n0 + (r & 1) < ntot ? n0 + (r & 1) : ntot - 1;
            wp[r] = a.w[r >> 1] + (long)n * K;
        } else {
            int n = n0 + r < ntot ? n0 + r : ntot - 1;
            bool lora_row = false;
            if constexpr (LORA) {
                if (n >= nw) {
                    int j = n - nw;
                    const int sgm = wg_lora_row_segment(a, j);
                    wp[r] = a.la[sgm] + (long)j * K;
                    lora_row = true;
                }
            }
            if (!lora_row) {
                int sgm = 0;
                if (n >= a.n[0]) { n -= a.n[0]; sgm = 1; if (n >= a.n[1]) { n -= a.n[1]; sgm = 2; } }
                wp[r] = a.w[sgm] + (long)n * K;
            }
        }
    }
    float acc[R][M];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int m = 0; m < M; ++m) acc[r][m] = 0.f;
#pragma unroll 2
    for (int k = lane * 8; k < K; k += 512) {
        u32x4 wv[R];
#pragma unroll
        for (int r = 0; r < R; ++r) wv[r] = __builtin_nontemporal_load((const u32x4*)(wp[r] + k));
        float g[8];
        if (a.gamma) {
            const bf16x8 t = *(const bf16x8*)(a.gamma + k);
#pragma unroll
            for (int e = 0; e < 8; ++e) g[e] = (float)t[e];
        }
        float xf[M][8];
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const bf16x8 t = *(const bf16x8*)(a.x + (long)m * a.ldx + k);
#pragma unroll
            for (int e = 0; e < 8; ++e) xf[m][e] = a.gamma ? (float)t[e] * rstd[m] * g[e] : (float)t[e];
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const bf16x8 wb = __builtin_bit_cast(bf16x8, wv[r]);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float wf = (float)wb[e];
#pragma unroll
                for (int m = 0; m < M; ++m) acc[r][m] += xf[m][e] * wf;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int m = 0; m < M; ++m) acc[r][m] = wg_wave_sum(acc[r][m]);
    if (lane != 0) return;
#pragma unroll
    for (int c = 0; c < RO; ++c) {
        const int n = n0 + c;
        if (n >= ntot) break;
        if constexpr (LORA) {
            if (n >= nw) {
                int j = n - nw;
                const int sgm = wg_lora_row_segment(a, j);
#pragma unroll
                for (int m = 0; m < M; ++m) a.t[(long)m * a.ldt + sgm * a.rank + j] = acc[c][m];
                continue;
            }
        }
#pragma unroll
        for (int m = 0; m < M; ++m) {
            float v;
            if constexpr (PAIR) {
                const float gt = acc[c][m], up = acc[2 + c][m];
                v = gt / (1.0f + __expf(-gt)) * up;
            } else {
                v = acc[c][m];
            }
            if (a.res) v += (float)a.res[(long)m * a.ldr + n];
            if (a.out_f32) ((float*)a.out)[(long)m * a.ldo + n] = v;
            else ((bf16*)a.out)[(long)m * a.ldo + n] = (bf16)v;
        }
    }
}

template <bool PAIR> static void wg_llama_gemv_launch(const GemvArgs& a, int M, unsigned blocks, hipStream_t st) {
    switch (M) {
        case 1: hipLaunchKernelGGL((wg_llama_gemv_kernel<1, PAIR>), dim3(blocks), dim3(256), 0, st, a); break;
        case 2: hipLaunchKernelGGL((wg_llama_gemv_kernel<2, PAIR>), dim3(blocks), dim3(256), 0, st, a); break;
        case 3: hipLaunchKernelGGL((wg_llama_gemv_kernel<3, PAIR>), dim3(blocks), dim3(256), 0, st, a); break;
        case 4: hipLaunchKernelGGL((wg_llama_gemv_kernel<4, PAIR>), dim3(blocks), dim3(256), 0, st, a); break;
        case 5: hipLaunchKernelGGL((wg_llama_gemv_kernel<5, PAIR>), dim3(blocks), dim3(256), 0, st, a); break;
        case 6: hipLaunchKernelGGL((wg_llama_gemv_kernel<6, PAIR>), dim3(blocks), dim3(256), 0, st, a); break;
        case 7: hipLaunchKernelGGL((wg_llama_gemv_kernel<7, PAIR>), dim3(blocks), dim3(256), 0, st, a); break;
        default: hipLaunchKernelGGL((wg_llama_gemv_kernel<8, PAIR>), dim3(blocks), dim3(256), 0, st, a); break;
    }
}

template <int M> static void wg_llama_gemv_lora_launch_m(const GemvLoraArgs& a, unsigned blocks, hipStream_t st) {
    hipLaunchKernelGGL((wg_llama_gemv_kernel<M, false, true>), dim3(blocks), dim3(256), 0, st, a);
}

static int wg_llama_gemv_check(const char* word, const void* x, long ldx, const void* w0, int n0, const void* w1, int n1, const void* w2, int n2,
                               int K, const void* gamma, const void* residual, long ldr, const void* out, long ldo, int pair, int M) {
    WG_REQUIRE(x && w0 && out, "%s: null operand", word);
    WG_REQUIRE(M >= 1 && M <= 8, "%s: M = %d rows (1 .. 8)", word, M);
    WG_REQUIRE(K > 0 && K % 128 == 0, "%s: K = %d must be a positive multiple of 128", word, K);
    WG_REQUIRE(n0 >= 1 && n1 >= 0 && n2 >= 0 && (w1 || n1 == 0) && (w2 || n2 == 0) && (n1 > 0 || n2 == 0), "%s: bad weight segments", word);
    WG_REQUIRE(!pair || (w1 && n1 == n0 && n2 == 0), "%s: pair mode takes two segments of equal N", word);
    const long ntot = pair ? n0 : (long)n0 + n1 + n2;
    WG_REQUIRE(ntot < (1L << 30), "%s: too many output columns", word);
    WG_REQUIRE(ldx >= K && ldx % 8 == 0 && ldo >= ntot && (!residual || ldr >= ntot), "%s: leading dimensions too small (or ldx not a multiple of 8)", word);
    WG_REQUIRE((((uintptr_t)x | (uintptr_t)w0 | (uintptr_t)w1 | (uintptr_t)w2 | (uintptr_t)gamma) & 15) == 0, "%s: misaligned operand", word);
    return 0;
}

extern "C" int wg_llama_gemv_bf16(const void* x, long ldx, const void* w0, int n0, const void* w1, int n1, const void* w2, int n2, int K,
                                  const void* gamma, float eps, const void* residual, long ldr, void* out, long ldo, int out_f32, int pair, int M,
                                  void* stream) {
    if (const int rc = wg_llama_gemv_check("llama_gemv", x, ldx, w0, n0, w1, n1, w2, n2, K, gamma, residual, ldr, out, ldo, pair, M)) return rc;
    const long ntot = pair ? n0 : (long)n0 + n1 + n2;
    GemvArgs a{(const bf16*)x, ldx, {(const bf16*)w0, (const bf16*)w1, (const bf16*)w2}, {n0, n1, n2}, K, (const bf16*)gamma, eps,
               (const bf16*)residual, ldr, out, ldo, out_f32};
    const int per_block = 4 * (pair ? 2 : 4);
    const unsigned blocks = (unsigned)((ntot + per_block - 1) / per_block);
    if (pair) wg_llama_gemv_launch<true>(a, M, blocks, (hipStream_t)stream);
    else wg_llama_gemv_launch<false>(a, M, blocks, (hipStream_t)stream);
    return wg_check_launch("wg_llama_gemv_bf16");
}

extern "C" int wg_llama_gemv_lora_bf16(const void* x, long ldx, const void* w0, int n0, const void* w1, int n1, const void* w2, int n2, int K,
                                       const void* gamma, float eps, const void* residual, long ldr, void* out, long ldo, int out_f32, int pair,
                                       int M, const void* a0, const void* a1, const void* a2, int rank, float* t, long ldt, void* stream) {
    if (const int rc = wg_llama_gemv_check("llama_gemv_lora", x, ldx, w0, n0, w1, n1, w2, n2, K, gamma, residual, ldr, out, ldo, pair, M)) return rc;
    WG_REQUIRE(rank >= 8 && rank <= 64 && rank % 8 == 0, "llama_gemv_lora: rank %d must be a multiple of 8, at most 64", rank);
    WG_REQUIRE(!pair, "llama_gemv_lora: pair mode takes no adapters");
    WG_REQUIRE((!a1 || n1 > 0) && (!a2 || n2 > 0), "llama_gemv_lora: an adapter on a segment that is not there");
    if (a0 || a1 || a2) {
        WG_REQUIRE(t, "llama_gemv_lora: null operand (t, with an adapter given)");
        WG_REQUIRE(ldt >= 3L * rank && ldt % 4 == 0, "llama_gemv_lora: ldt %ld too small for [M, 3 rank] (or not a multiple of 4)", ldt);
        WG_REQUIRE((((uintptr_t)a0 | (uintptr_t)a1 | (uintptr_t)a2 | (uintptr_t)t) & 15) == 0, "llama_gemv_lora: misaligned A / t");
    }
    GemvLoraArgs a{{(const bf16*)x, ldx, {(const bf16*)w0, (const bf16*)w1, (const bf16*)w2}, {n0, n1, n2}, K, (const bf16*)gamma, eps,
                    (const bf16*)residual, ldr, out, ldo, out_f32}, {(const bf16*)a0, (const bf16*)a1, (const bf16*)a2}, rank, t, ldt};
    const long ntot = (long)n0 + n1 + n2 + (long)((a0 != nullptr) + (a1 != nullptr) + (a2 != nullptr)) * rank;
    const unsigned blocks = (unsigned)((ntot + 15) / 16);
    const hipStream_t st = (hipStream_t)stream;
    switch (M) {
        case 1: wg_llama_gemv_lora_launch_m<1>(a, blocks, st); break;
        case 2: wg_llama_gemv_lora_launch_m<2>(a, blocks, st); break;
        case 3: wg_llama_gemv_lora_launch_m<3>(a, blocks, st); break;
        case 4: wg_llama_gemv_lora_launch_m<4>(a, blocks, st); break;
        case 5: wg_llama_gemv_lora_launch_m<5>(a, blocks, st); break;
        case 6: wg_llama_gemv_lora_launch_m<6>(a, blocks, st); break;
        case 7: wg_llama_gemv_lora_launch_m<7>(a, blocks, st); break;
        default: wg_llama_gemv_lora_launch_m<8>(a, blocks, st); break;
    }
    return wg_check_launch("wg_llama_gemv_lora_bf16");
}

// ---- e2. e4m3 weight-only decode (W8A16) ----------------------------------------------------------------------------------------------
// The projection weights as OCP e4m3 bytes with one power-of-two scale per output row; activations bf16, arithmetic fp32.
// Format, for W [N, K] bf16 and row n with amax = max_k |W[n][k]|:  e[n] = the smallest integer with amax <= 448 * 2^e, clamped to
// [-126, 127] (an all-zero row: e = 0);  scale[n] = 2^e[n] (fp32);  q[n][k] = W[n][k] / scale[n] rounded to e4m3, nearest-even.
// W' = q * scale is exactly a bf16 value (4 significant bits times a power of two), so the quantised model is an ordinary model with
// the weights W', and the prefill runs the bf16 GEMMs on W'.  e is found on the bf16 bits: amax = m * 2^x with m in [0.5, 1) gives
// e = x - 9 for m <= 0.875 and x - 8 above.  The quantiser and the dequantiser work on the bit fields alone (no float multiply sees
// a subnormal, whatever the kernel's denormal mode), which is what makes them exact for every finite input; a non-finite weight is
// outside the contract (it gives some byte, never an access outside the buffers).

// |v| = (1 + mm / 128) * 2^(eb - 127) for the non-zero bf16 magnitude bits `a` (15 bits): a normal value as it stands, a subnormal normalised
__device__ __forceinline__ void wg_bf16_fields(unsigned a, int& eb, unsigned& mm) {
    eb = (int)(a >> 7);
    mm = a & 0x7fu;
    if (eb == 0) {                          // subnormal: mm * 2^-133, mm in 1 .. 127
        const int s = __builtin_clz(mm) - 24;       // shifts that bring the leading one to bit 7
        mm = (mm << s) & 0x7fu;
        eb = 1 - s;
    }
}

// the e4m3 byte of bf16 bits `h` divided by 2^e, round to nearest even
__device__ __forceinline__ unsigned wg_e4m3_of_bf16_scaled(unsigned h, int e) {
    const unsigned sign = (h >> 8) & 0x80u, a = h & 0x7fffu;
    if (a == 0) return sign;
    int eb;
    unsigned mm;
    wg_bf16_fields(a, eb, mm);
    int ue = eb - 127 - e;                  // the quotient is sig * 2^(ue - 7), sig in 128 .. 255
    const unsigned sig = 128u | mm;
    if (ue >= -6) {                         // an e4m3 normal: 4 of the 8 significant bits stay
        unsigned q = sig >> 4;
        const unsigned rem = sig & 15u;
        if (rem > 8u || (rem == 8u && (q & 1u))) ++q;
        if (q == 16u) { q = 8u; ++ue; }
        const unsigned byte = ((unsigned)(ue + 7) << 3) | (q & 7u);
        return sign | (byte > 0x7eu ? 0x7eu : byte);          // (not reached by a row's own scale: nothing exceeds 448)
    }
    const int sh = -(ue + 2);               // an e4m3 subnormal, in units of 2^-9: sig >> sh, sh >= 5
    if (sh > 9) return sign;                // below half a unit
    const unsigned q = sig >> sh, rem = sig & ((1u << sh) - 1u), half = 1u << (sh - 1);
    return sign | (q + ((rem > half || (rem == half && (q & 1u))) ? 1u : 0u));      // (8 units are the smallest normal, 0x08)
}

// the bf16 bits of e4m3 byte `b` times 2^e: exact for every (q, scale) the quantiser leaves
__device__ __forceinline__ unsigned wg_bf16_of_e4m3_scaled(unsigned b, int e) {
    const unsigned sign = (b & 0x80u) << 8;
    int ef = (int)((b >> 3) & 15u);
    unsigned f = b & 7u;
    if (ef == 0) {
        if (f == 0) return sign;
        const int s = __builtin_clz(f) - 28;        // shifts that bring the leading one to bit 3
        f = (f << s) & 7u;
        ef = 1 - s;
    }
    const int eb = ef - 7 + e + 127;
    const unsigned m7 = f << 4;
    if (eb >= 255) return sign | 0x7f80u;
    if (eb >= 1) return sign | ((unsigned)eb << 7) | m7;
    const int sh = 1 - eb;                  // a bf16 subnormal: the bits that leave are zeros for a quantiser's (q, scale)
    return sign | (sh > 8 ? 0u : ((128u | m7) >> sh));
}

// One 256-thread block per row; the row maximum is taken on the magnitude bits (integers: exact and the same in any order).
__global__ __launch_bounds__(256) void wg_llama_quantize_e4m3_kernel(const unsigned short* w, unsigned char* q, float* scale, int K) {
    __shared__ unsigned red[4];
    const int tid = threadIdx.x;
    const long row = blockIdx.x;
    const unsigned short* wr = w + row * K;
    unsigned amax = 0;
    for (int k = tid * 16; k < K; k += 4096) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const u32x4 t = *(const u32x4*)(wr + k + 8 * h);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const unsigned lo = t[c] & 0x7fffu, hi = (t[c] >> 16) & 0x7fffu;
                amax = amax > lo ? amax : lo;
                amax = amax > hi ? amax : hi;
            }
        }
    }
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)amax, s, 64);
        amax = amax > o ? amax : o;
    }
    if ((tid & 63) == 0) red[tid >> 6] = amax;
    __syncthreads();
    amax = red[0] > red[1] ? red[0] : red[1];
    amax = amax > red[2] ? amax : red[2];
    amax = amax > red[3] ? amax : red[3];
    int e = 0;
    if (amax != 0) {
        int eb;
        unsigned mm;
        wg_bf16_fields(amax, eb, mm);
        e = eb - 126 - (mm <= 96u ? 9 : 8);           // amax = m * 2^x: x = eb - 126, m = (1 + mm / 128) / 2 <= 0.875 is mm <= 96
        e = wg_clampi(e, -126, 127);
    }
    if (tid == 0) scale[row] = __builtin_bit_cast(float, (unsigned)(e + 127) << 23);
    unsigned char* qr = q + row * K;
    for (int k = tid * 16; k < K; k += 4096) {
        u32x4 o;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const u32x4 t = *(const u32x4*)(wr + k + 8 * h);
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                unsigned v = 0;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const unsigned d = t[2 * c + j];
                    v |= (wg_e4m3_of_bf16_scaled(d & 0xffffu, e) | (wg_e4m3_of_bf16_scaled(d >> 16, e) << 8)) << (16 * j);
                }
                o[2 * h + c] = v;
            }
        }
        *(u32x4*)(qr + k) = o;
    }
}

extern "C" int wg_llama_quantize_weight_e4m3(const void* w, void* q, float* scale, int N, int K, void* stream) {
    WG_REQUIRE(w && q && scale, "llama_quantize_weight_e4m3: null operand");
    WG_REQUIRE(N > 0 && K > 0 && K % 16 == 0, "llama_quantize_weight_e4m3: bad shape (N %d, K %d; K must be a multiple of 16)", N, K);
    WG_REQUIRE((((uintptr_t)w | (uintptr_t)q) & 15) == 0 && ((uintptr_t)scale & 3) == 0, "llama_quantize_weight_e4m3: misaligned operand");
    hipLaunchKernelGGL(wg_llama_quantize_e4m3_kernel, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)w,
                       (unsigned char*)q, scale, K);
    return wg_check_launch("wg_llama_quantize_weight_e4m3");
}

// One thread per 16 weights: W'[n][k] = q[n][k] * scale[n] as bf16, exact.  The scale's exponent field is all that is read of it.
__global__ __launch_bounds__(256) void wg_llama_dequantize_bf16_kernel(const unsigned char* q, const float* scale, unsigned short* w, long total, int K) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long row = i / (K / 16);
    const int e = (int)((__builtin_bit_cast(unsigned, scale[row]) >> 23) & 0xffu) - 127;
    const u32x4 t = *(const u32x4*)(q + i * 16);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        u32x4 o;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const unsigned d = t[2 * h + (c >> 1)] >> (16 * (c & 1));
            o[c] = wg_bf16_of_e4m3_scaled(d & 0xffu, e) | (wg_bf16_of_e4m3_scaled((d >> 8) & 0xffu, e) << 16);
        }
        *(u32x4*)(w + i * 16 + 8 * h) = o;
    }
}

extern "C" int wg_llama_dequantize_weight_bf16(const void* q, const float* scale, void* w, int N, int K, void* stream) {
    WG_REQUIRE(q && scale && w, "llama_dequantize_weight_bf16: null operand");
    WG_REQUIRE(N > 0 && K > 0 && K % 16 == 0, "llama_dequantize_weight_bf16: bad shape (N %d, K %d; K must be a multiple of 16)", N, K);
    WG_REQUIRE((((uintptr_t)w | (uintptr_t)q) & 15) == 0 && ((uintptr_t)scale & 3) == 0, "llama_dequantize_weight_bf16: misaligned operand");
    const long total = (long)N * (K / 16);
    WG_REQUIRE((total + 255) / 256 < (1L << 31), "llama_dequantize_weight_bf16: too many elements");
    hipLaunchKernelGGL(wg_llama_dequantize_bf16_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned char*)q, scale, (unsigned short*)w, total, K);
    return wg_check_launch("wg_llama_dequantize_weight_bf16");
}

// The decode GEMV on byte weights: out[m][n] = scale[n] * sum_k xh[m][k] q[n][k], wg_llama_gemv_bf16's contract otherwise (segments, norm,
// residual, pair, out_f32).  A wave owns 4 weight rows as there; lane l takes the 16-byte pieces l, l + 64, ... of each row (16 weights a
// load, a sweep of the wave covers 1024 of K: K = 128 keeps 8 lanes busy, K = 11008 ends in a sweep of 48), converts them with
// v_cvt_pk_f32_fp8 (OCP on gfx950, exact) and adds its K / 64 products one after the other in element order, 8 elements of the 4 rows at a
// time; the wave adds the lane sums by the same butterfly.  The scale multiplies the wave's sum -- a power of two, so exact -- before
// SiLU and the residual.
//   lora   (wg_llama_gemv_lora_e4m3) the adapter rows stay bf16 and take waves of their own, so a wave holds rows of one kind: the first
//          waves of the launch (an adapter wave streams twice the bytes of a W wave, so it starts with the grid and not behind it;
//          measured on the 7B q | k | v launch, first or last made no difference: 21.3 / 20.7 us).  They are summed as
//          wg_llama_gemv_lora_bf16 sums them (8-element pieces) and leave as fp32 into t.
struct GemvQArgs : GemvArgs {
    const float* s[3];
};
struct GemvQLoraArgs : GemvQArgs {
    const bf16* la[3]; int rank;
    float* t; long ldt;
};

// xf[m][e] = the normalised input elements k .. k + 7 of the M rows
template <int M, class A>
__device__ __forceinline__ void wg_gemv_x8(const A& a, const float* rstd, int k, float (&xf)[M][8]) {
    float g[8];
    if (a.gamma) {
        const bf16x8 t = *(const bf16x8*)(a.gamma + k);
#pragma unroll
        for (int e = 0; e < 8; ++e) g[e] = (float)t[e];
    }
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const bf16x8 t = *(const bf16x8*)(a.x + (long)m * a.ldx + k);
#pragma unroll
        for (int e = 0; e < 8; ++e) xf[m][e] = a.gamma ? (float)t[e] * rstd[m] * g[e] : (float)t[e];
    }
}

template <int M, bool PAIR, bool LORA = false>
__global__ __launch_bounds__(256) void wg_llama_gemv_e4m3_kernel(std::conditional_t<LORA, GemvQLoraArgs, GemvQArgs> a) {
    static_assert(!(PAIR && LORA), "pair mode takes no adapters");
    constexpr int R = 4;
    constexpr int RO = PAIR ? 2 : 4;
    __shared__ float red[4][8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = a.K;
    float rstd[M];
#pragma unroll
    for (int m = 0; m < M; ++m) rstd[m] = 1.f;
    if (a.gamma) {
        float ss[M];
#pragma unroll
        for (int m = 0; m < M; ++m) ss[m] = 0.f;
        for (int k = tid * 8; k < K; k += 2048) {
#pragma unroll
            for (int m = 0; m < M; ++m) {
                const bf16x8 t = *(const bf16x8*)(a.x + (long)m * a.ldx + k);
#pragma unroll
                for (int e = 0; e < 8; ++e) ss[m] += (float)t[e] * (float)t[e];
            }
        }
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const float t = wg_wave_sum(ss[m]);
            if (lane == 0) red[wave][m] = t;
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < M; ++m) rstd[m] = 1.0f / sqrtf(((red[0][m] + red[1][m]) + (red[2][m] + red[3][m])) / (float)K + a.eps);
    }
    const int nw = PAIR ? a.n[0] : a.n[0] + a.n[1] + a.n[2];
    const int wi = blockIdx.x * 4 + wave;       // (every return is after the only barrier)
    float acc[R][M];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int m = 0; m < M; ++m) acc[r][m] = 0.f;
    int l_waves = 0;                            // the launch's first waves take the adapter rows
    if constexpr (LORA) {
        const int nl = ((a.la[0] != nullptr) + (a.la[1] != nullptr) + (a.la[2] != nullptr)) * a.rank;
        l_waves = (nl + R - 1) / R;
        if (wi < l_waves) {                     // a wave of adapter rows: bf16, wg_llama_gemv_kernel's loop
            const int j0 = wi * R;
            const bf16* wp[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                int j = j0 + r < nl ? j0 + r : nl - 1;
                int sgm = 0;
                if (!a.la[0] || j >= a.rank) {
                    if (a.la[0]) j -= a.rank;
                    sgm = 1;
                    if (!a.la[1] || j >= a.rank) {
                        if (a.la[1]) j -= a.rank;
                        sgm = 2;
                    }
                }
                wp[r] = a.la[sgm] + (long)j * K;
            }
#pragma unroll 2
            for (int k = lane * 8; k < K; k += 512) {
                u32x4 wv[R];
#pragma unroll
                for (int r = 0; r < R; ++r) wv[r] = __builtin_nontemporal_load((const u32x4*)(wp[r] + k));
                float xf[M][8];
                wg_gemv_x8<M>(a, rstd, k, xf);
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const bf16x8 wb = __builtin_bit_cast(bf16x8, wv[r]);
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float wf = (float)wb[e];
#pragma unroll
                        for (int m = 0; m < M; ++m) acc[r][m] += xf[m][e] * wf;
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int m = 0; m < M; ++m) acc[r][m] = wg_wave_sum(acc[r][m]);
            if (lane != 0) return;
#pragma unroll
            for (int c = 0; c < R; ++c) {
                int j = j0 + c;
                if (j >= nl) break;
                int sgm = 0;
                if (!a.la[0] || j >= a.rank) {
                    if (a.la[0]) j -= a.rank;
                    sgm = 1;
                    if (!a.la[1] || j >= a.rank) {
                        if (a.la[1]) j -= a.rank;
                        sgm = 2;
                    }
                }
#pragma unroll
                for (int m = 0; m < M; ++m) a.t[(long)m * a.ldt + sgm * a.rank + j] = acc[c][m];
            }
            return;
        }
    }
    const int n0 = (wi - l_waves) * RO;
    if (n0 >= nw) return;
    const unsigned char* wp[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if constexpr (PAIR) {
            const int n = n0 + (r & 1) < nw ? n0 + (r & 1) : nw - 1;
            wp[r] = (const unsigned char*)a.w[r >> 1] + (long)n * K;
        } else {
            int n = n0 + r < nw ? n0 + r : nw - 1;
            int sgm = 0;
            if (n >= a.n[0]) { n -= a.n[0]; sgm = 1; if (n >= a.n[1]) { n -= a.n[1]; sgm = 2; } }
            wp[r] = (const unsigned char*)a.w[sgm] + (long)n * K;
        }
    }
#pragma unroll 2
    for (int k = lane * 16; k < K; k += 1024) {
        u32x4 wv[R];
#pragma unroll
        for (int r = 0; r < R; ++r) wv[r] = __builtin_nontemporal_load((const u32x4*)(wp[r] + k));
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            float xf[M][8];
            wg_gemv_x8<M>(a, rstd, k + 8 * h, xf);
#pragma unroll
            for (int r = 0; r < R; ++r) {
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const int d = (int)wv[r][2 * h + c];
                    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(d, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8(d, true);
                    const float wf[4] = {lo[0], lo[1], hi[0], hi[1]};
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int m = 0; m < M; ++m) acc[r][m] += xf[m][4 * c + e] * wf[e];
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int m = 0; m < M; ++m) acc[r][m] = wg_wave_sum(acc[r][m]);
    if (lane != 0) return;
#pragma unroll
    for (int c = 0; c < RO; ++c) {
        const int n = n0 + c;
        if (n >= nw) break;
        float sc0, sc1 = 0.f;
        if constexpr (PAIR) {
            sc0 = a.s[0][n];
            sc1 = a.s[1][n];
        } else {
            int j = n, sgm = 0;
            if (j >= a.n[0]) { j -= a.n[0]; sgm = 1; if (j >= a.n[1]) { j -= a.n[1]; sgm = 2; } }
            sc0 = a.s[sgm][j];
        }
#pragma unroll
        for (int m = 0; m < M; ++m) {
            float v;
            if constexpr (PAIR) {
                const float gt = acc[c][m] * sc0, up = acc[2 + c][m] * sc1;
                v = gt / (1.0f + __expf(-gt)) * up;
            } else {
                v = acc[c][m] * sc0;
            }
            if (a.res) v += (float)a.res[(long)m * a.ldr + n];
            if (a.out_f32) ((float*)a.out)[(long)m * a.ldo + n] = v;
            else ((bf16*)a.out)[(long)m * a.ldo + n] = (bf16)v;
        }
    }
}

template <bool PAIR> static void wg_llama_gemv_e4m3_launch(const GemvQArgs& a, int M, unsigned blocks, hipStream_t st) {
    switch (M) {
        case 1: hipLaunchKernelGGL((wg_llama_gemv_e4m3_kernel<1, PAIR>), dim3(blocks), dim3(256), 0, st, a); break;
        case 2: hipLaunchKernelGGL((wg_llama_gemv_e4m3_kernel<2, PAIR>), dim3(blocks), dim3(256), 0, st, a); break;
        case 3: hipLaunchKernelGGL((wg_llama_gemv_e4m3_kernel<3, PAIR>), dim3(blocks), dim3(256), 0, st, a); break;
        case 4: hipLaunchKernelGGL((wg_llama_gemv_e4m3_kernel<4, PAIR>), dim3(blocks), dim3(256), 0, st, a); break;
        case 5: hipLaunchKernelGGL((wg_llama_gemv_e4m3_kernel<5, PAIR>), dim3(blocks), dim3(256), 0, st, a); break;
        case 6: hipLaunchKernelGGL((wg_llama_gemv_e4m3_kernel<6, PAIR>), dim3(blocks), dim3(256), 0, st, a); break;
        case 7: hipLaunchKernelGGL((wg_llama_gemv_e4m3_kernel<7, PAIR>), dim3(blocks), dim3(256), 0, st, a); break;
        default: hipLaunchKernelGGL((wg_llama_gemv_e4m3_kernel<8, PAIR>), dim3(blocks), dim3(256), 0, st, a); break;
    }
}

template <int M> static void wg_llama_gemv_lora_e4m3_launch_m(const GemvQLoraArgs& a, unsigned blocks, hipStream_t st) {
    hipLaunchKernelGGL((wg_llama_gemv_e4m3_kernel<M, false, true>), dim3(blocks), dim3(256), 0, st, a);
}

// the scales of the segments that are there: not null, 4-byte aligned
static int wg_llama_gemv_scale_check(const char* word, const float* s0, const float* s1, int n1, const float* s2, int n2) {
    WG_REQUIRE(s0 && (s1 || n1 == 0) && (s2 || n2 == 0), "%s: null scale", word);
    WG_REQUIRE((((uintptr_t)s0 | (uintptr_t)s1 | (uintptr_t)s2) & 3) == 0, "%s: misaligned scale", word);
    return 0;
}

extern "C" int wg_llama_gemv_e4m3(const void* x, long ldx, const void* w0, const float* s0, int n0, const void* w1, const float* s1, int n1,
                                  const void* w2, const float* s2, int n2, int K, const void* gamma, float eps, const void* residual, long ldr,
                                  void* out, long ldo, int out_f32, int pair, int M, void* stream) {
    if (const int rc = wg_llama_gemv_check("llama_gemv_e4m3", x, ldx, w0, n0, w1, n1, w2, n2, K, gamma, residual, ldr, out, ldo, pair, M)) return rc;
    if (const int rc = wg_llama_gemv_scale_check("llama_gemv_e4m3", s0, s1, n1, s2, n2)) return rc;
    const long ntot = pair ? n0 : (long)n0 + n1 + n2;
    GemvQArgs a{{(const bf16*)x, ldx, {(const bf16*)w0, (const bf16*)w1, (const bf16*)w2}, {n0, n1, n2}, K, (const bf16*)gamma, eps,
                 (const bf16*)residual, ldr, out, ldo, out_f32}, {s0, s1, s2}};
    const int per_block = 4 * (pair ? 2 : 4);
    const unsigned blocks = (unsigned)((ntot + per_block - 1) / per_block);
    if (pair) wg_llama_gemv_e4m3_launch<true>(a, M, blocks, (hipStream_t)stream);
    else wg_llama_gemv_e4m3_launch<false>(a, M, blocks, (hipStream_t)stream);
    return wg_check_launch("wg_llama_gemv_e4m3");
}

extern "C" int wg_llama_gemv_lora_e4m3(const void* x, long ldx, const void* w0, const float* s0, int n0, const void* w1, const float* s1, int n1,
                                       const void* w2, const float* s2, int n2, int K, const void* gamma, float eps, const void* residual,
                                       long ldr, void* out, long ldo, int out_f32, int pair, int M, const void* a0, const void* a1,
                                       const void* a2, int rank, float* t, long ldt, void* stream) {
    if (const int rc = wg_llama_gemv_check("llama_gemv_lora_e4m3", x, ldx, w0, n0, w1, n1, w2, n2, K, gamma, residual, ldr, out, ldo, pair, M)) return rc;
    if (const int rc = wg_llama_gemv_scale_check("llama_gemv_lora_e4m3", s0, s1, n1, s2, n2)) return rc;
    WG_REQUIRE(rank >= 8 && rank <= 64 && rank % 8 == 0, "llama_gemv_lora_e4m3: rank %d must be a multiple of 8, at most 64", rank);
    WG_REQUIRE(!pair, "llama_gemv_lora_e4m3: pair mode takes no adapters");
    WG_REQUIRE((!a1 || n1 > 0) && (!a2 || n2 > 0), "llama_gemv_lora_e4m3: an adapter on a segment that is not there");
    if (a0 || a1 || a2) {
        WG_REQUIRE(t, "llama_gemv_lora_e4m3: null operand (t, with an adapter given)");
        WG_REQUIRE(ldt >= 3L * rank && ldt % 4 == 0, "llama_gemv_lora_e4m3: ldt %ld too small for [M, 3 rank] (or not a multiple of 4)", ldt);
        WG_REQUIRE((((uintptr_t)a0 | (uintptr_t)a1 | (uintptr_t)a2 | (uintptr_t)t) & 15) == 0, "llama_gemv_lora_e4m3: misaligned A / t");
    }
    GemvQLoraArgs a{{{(const bf16*)x, ldx, {(const bf16*)w0, (const bf16*)w1, (const bf16*)w2}, {n0, n1, n2}, K, (const bf16*)gamma, eps,
                      (const bf16*)residual, ldr, out, ldo, out_f32}, {s0, s1, s2}}, {(const bf16*)a0, (const bf16*)a1, (const bf16*)a2}, rank, t, ldt};
    const long w_waves = ((long)n0 + n1 + n2 + 3) / 4;
    const long l_waves = ((long)((a0 != nullptr) + (a1 != nullptr) + (a2 != nullptr)) * rank + 3) / 4;
    const unsigned blocks = (unsigned)((w_waves + l_waves + 3) / 4);
    const hipStream_t st = (hipStream_t)stream;
    switch (M) {
        case 1: wg_llama_gemv_lora_e4m3_launch_m<1>(a, blocks, st); break;
        case 2: wg_llama_gemv_lora_e4m3_launch_m<2>(a, blocks, st); break;
        case 3: wg_llama_gemv_lora_e4m3_launch_m<3>(a, blocks, st); break;
        case 4: wg_llama_gemv_lora_e4m3_launch_m<4>(a, blocks, st); break;
        case 5: wg_llama_gemv_lora_e4m3_launch_m<5>(a, blocks, st); break;
        case 6: wg_llama_gemv_lora_e4m3_launch_m<6>(a, blocks, st); break;
        case 7: wg_llama_gemv_lora_e4m3_launch_m<7>(a, blocks, st); break;
        default: wg_llama_gemv_lora_e4m3_launch_m<8>(a, blocks, st); break;
    }
    return wg_check_launch("wg_llama_gemv_lora_e4m3");
}

// ---- SiLU(gate) * up on a [M, 2 I] buffer (gate | up), the prefill's MLP middle ------------------------------------------------------
__global__ __launch_bounds__(256) void wg_llama_silu_mul_kernel(const bf16* gu, long ldgu, bf16* out, long ldo, int M, int I) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int per = I / 8;
    if (i >= (long)M * per) return;
    const int m = (int)(i / per), c = (int)(i % per) * 8;
    const bf16x8 g = *(const bf16x8*)(gu + (long)m * ldgu + c), u = *(const bf16x8*)(gu + (long)m * ldgu + I + c);
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float gt = (float)g[e];
        o[e] = (bf16)(gt / (1.0f + __expf(-gt)) * (float)u[e]);
    }
    *(bf16x8*)(out + (long)m * ldo + c) = o;
}

extern "C" int wg_llama_silu_mul_bf16(const void* gate_up, long ldgu, void* out, long ldo, int M, int I, void* stream) {
    WG_REQUIRE(gate_up && out, "llama_silu_mul: null operand");
    WG_REQUIRE(M > 0 && I > 0 && I % 8 == 0, "llama_silu_mul: bad shape (M %d, I %d; I must be a multiple of 8)", M, I);
    WG_REQUIRE(ldgu >= 2L * I && ldo >= I && ldgu % 8 == 0 && ldo % 8 == 0, "llama_silu_mul: leading dimensions too small or not multiples of 8");
    WG_REQUIRE((((uintptr_t)gate_up | (uintptr_t)out) & 15) == 0, "llama_silu_mul: misaligned operand");
    const long total = (long)M * (I / 8);
    hipLaunchKernelGGL(wg_llama_silu_mul_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const bf16*)gate_up, ldgu,
                       (bf16*)out, ldo, M, I);
    return wg_check_launch("wg_llama_silu_mul_bf16");
}

// ---- f. token pick ------------------------------------------------------------------------------------------------------------------
// One 1024-thread block (the rows share the state words, so one block owns them).  Per row: argmax of the fp32 logits, lowest index on
// a tie; a finished row emits pad, finished |= (token == eos) (eos < 0: no eos, no pad substitution); tokens[row][n_new] = token; the
// token's embedding row -> x_next[row]; mask[row][past_len + 1] = 1.  Then past_len and n_new move on by one -- past_len not beyond
// cap - 1, n_new not beyond tok_cap (a token that has no slot is not written).
struct PickArgs {
    const float* logits; long ldl;
    const bf16* embed; int n_embed;
    bf16* x_next; long ldx;
    long long* tokens; int tok_cap;
    int* finished;
    unsigned char* mask;
    int* state;               // {past_len, n_new}
    int eos, pad;
    int rows, V, H, cap;
};

__global__ __launch_bounds__(1024) void wg_llama_pick_token_kernel(PickArgs a) {
    __shared__ float bv[1024];
    __shared__ int bi[1024];
    __shared__ int tok[8];
    const int tid = threadIdx.x;
    const int past = a.state[0], nn = a.state[1];
    for (int row = 0; row < a.rows; ++row) {
        const float* lg = a.logits + (long)row * a.ldl;
        float best = -INFINITY;
        int idx = 0x7fffffff;
        for (int i = tid; i < a.V; i += 1024) {
            const float v = lg[i];
            if (v > best || idx == 0x7fffffff) { best = v; idx = i; }     // strictly greater: the lowest index of a thread's run wins
        }
        bv[tid] = best;
        bi[tid] = idx;
        __syncthreads();
        for (int w = 512; w > 0; w >>= 1) {
            if (tid < w) {
                const float v2 = bv[tid + w];
                const int i2 = bi[tid + w];
                if (i2 != 0x7fffffff && (bi[tid] == 0x7fffffff || v2 > bv[tid] || (v2 == bv[tid] && i2 < bi[tid]))) { bv[tid] = v2; bi[tid] = i2; }
            }
            __syncthreads();
        }
        if (tid == 0) {
            int t = wg_clampi(bi[0], 0, a.V - 1);
            if (a.eos >= 0) {
                int fin = a.finished[row];
                if (fin) t = a.pad;
                fin |= (t == a.eos);
                a.finished[row] = fin;
            }
            tok[row] = t;
            if (nn >= 0 && nn < a.tok_cap) a.tokens[(long)row * a.tok_cap + nn] = t;
            if (past >= -1 && past < a.cap - 1) a.mask[(long)row * a.cap + past + 1] = 1;
        }
        __syncthreads();
    }
    for (int row = 0; row < a.rows; ++row) {
        const bf16* src = a.embed + (long)wg_clampi(tok[row], 0, a.n_embed - 1) * a.H;
        for (int k = tid * 8; k < a.H; k += 8192) *(bf16x8*)(a.x_next + (long)row * a.ldx + k) = *(const bf16x8*)(src + k);
    }
    if (tid == 0) {
        if (past >= -1 && past < a.cap - 1) a.state[0] = past + 1;
        if (nn >= 0 && nn < a.tok_cap) a.state[1] = nn + 1;
    }
}

extern "C" int wg_llama_pick_token(const float* logits, long ldl, const void* embed, int n_embed, void* x_next, long ldx, long long* tokens,
                                   int tok_cap, int* finished, unsigned char* mask, int* state, int eos, int pad, int rows, int V, int H, int cap,
                                   void* stream) {
    WG_REQUIRE(logits && embed && x_next && tokens && finished && mask && state, "llama_pick_token: null operand");
    WG_REQUIRE(rows >= 1 && rows <= 8, "llama_pick_token: rows = %d (1 .. 8)", rows);
    WG_REQUIRE(V >= 1 && n_embed >= V && H > 0 && H % 8 == 0 && tok_cap >= 1, "llama_pick_token: bad shape (V %d, embedding rows %d, H %d)", V, n_embed, H);
    WG_REQUIRE(cap > 0 && cap % 64 == 0, "llama_pick_token: cache capacity %d must be a positive multiple of 64", cap);
    WG_REQUIRE(ldl >= V && ldx >= H && ldx % 8 == 0, "llama_pick_token: leading dimensions too small");
    WG_REQUIRE(eos < 0 || (pad >= 0 && pad < n_embed), "llama_pick_token: pad id %d outside the embedding table", pad);
    WG_REQUIRE((((uintptr_t)embed | (uintptr_t)x_next) & 15) == 0, "llama_pick_token: misaligned operand");
    PickArgs a{logits, ldl, (const bf16*)embed, n_embed, (bf16*)x_next, ldx, tokens, tok_cap, finished, mask, state, eos, pad, rows, V, H, cap};
    hipLaunchKernelGGL(wg_llama_pick_token_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, a);
    return wg_check_launch("wg_llama_pick_token");
}
