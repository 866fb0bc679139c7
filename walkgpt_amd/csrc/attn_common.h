// Shared by attn.hip, attn_window_unit.hip and attn_pipe.hip: argument block, LDS swizzles of the K / V tiles, tile geometry and LDS layouts,
// the asm form of the transposed LDS read, the few device pieces the kernels share.
#pragma once
#include "wg_common.h"

#define LOG2E 1.4426950408889634f
#define NEG_BIG (-1.0e30f)

struct AttnArgs {
    const bf16* Q; const bf16* K; const bf16* V; bf16* O;
    long ldq, ldk, ldv, ldo;     // row strides (elements)
    long q_bs, k_bs, o_bs;       // rows per batch item (plain mode)
    const bf16* padK; const bf16* padV;  // grid mode: bias rows used for zero-padded window positions
    const bf16* rel_h; const bf16* rel_w;  // [2S-1, HD]
    const float* key_bias;       // plain mode: [B, Lk] additive, may be null
    int B, heads, Lq, Lk;
    int Hg;                      // grid mode: tokens per image side
    int nW;                      // windows per side
    int qchunks;                 // workgroups per (batch, window, head)
    float scale;
    // fp8 chain (grid mode, head_dim 64): the output leaves as e4m3 bytes + one E8M0 scale per (row, 32 columns) -- the A operand of the
    // MX GEMM behind the attention (gemm.hip GemmArgs::mx_a layout: rows r, r + 16, .. of a 128-row group adjacent) -- instead of bf16
    unsigned char* Oq; long ldoq; unsigned char* Omx; long mx_pitch;
};

template <int HD> __device__ __forceinline__ int swzK(int row) {
    if (HD == 16) return (row >> 2) & 3;   // stored as 64-byte rows like head_dim 32
    if (HD == 80) return 0;   // 208-byte padded rows (SAM ViT-H): the row pitch itself spreads the banks
    if (HD == 128) return row & 15;
    if (HD == 64) return (row >> 1) & 7;
    return (row >> 2) & 3;  // HD == 32
}
template <int HD> __device__ __forceinline__ int swzV(int row) {
    if (HD == 80) return 0;
    if (HD == 128) return (row & 3) << 2;
    if (HD == 64) return ((row >> 1) & 1) << 2;
    return 0;
}

// ---- tile geometry: stated once for the kernels of attn.hip / attn_window_unit.hip and their launchers -------------------------------
// S == 0: plain attention; S > 0: the side of a SAM window or (S == 64) of the global grid.
template <int HD, int S> struct AttnGeom {
    static constexpr int HDP = (HD == 80) ? 96 : (HD == 16 ? 32 : HD);  // head dim padded to a multiple of 32 inside LDS
    // head_dim 80: rows padded once more to 13 chunks = 52 dwords, a pitch that sends 16 consecutive rows to 16 different bank
    // quads (the K fragment reads of 192-byte rows were 4-way conflicted: rows r and r + 4 shared their banks); the 13th chunk of
    // a row is never read
    static constexpr int ROWB = (HD == 80) ? 208 : HDP * 2;   // bytes per K row
    // V rows of head_dim 80 keep the natural 192-byte pitch (12 chunks): four consecutive rows x 16 dwords then fall on disjoint bank
    // ranges for the transposed reads (pitch 48 dwords: 0, 48, 32, 16 mod 64), which the 208-byte pitch of the K rows (0, 52, 40, 28: rows
    // r and r + 1 overlap by four banks, a 2-way conflict) does not give; K keeps 208 for its ds_read_b128 pattern
    static constexpr int ROWBV = (HD == 80) ? 192 : ROWB;     // bytes per V row
    static constexpr int TILE = 64 * ROWB;        // bytes per K tile
    static constexpr int TILEV = 64 * ROWBV;      // bytes per V tile
    static constexpr int TILE2 = TILE + TILEV;    // one buffer = K tile | V tile
    static constexpr int KSTEPS = HD / 16;        // QK^T runs over the real head dim only
    static constexpr int DB = HDP / 32;           // PV d-blocks; columns >= HD hold don't-care data and are never stored
    // Grid mode key order: window rows padded to RP slots (16 / 32 / 64), RPT rows per 64-key tile.  A key slot's
    // column (kw) then depends only on the accumulator register, its row (kh) only on (tile, register): the width term
    // of the rel-pos bias is RP/2 registers per lane, the height term RPT LDS reads per tile, and padding slots are
    // masked by -inf entries in those two tables instead of per-element tests.  (S == 64: a tile is exactly one grid row.)
    static constexpr int RP = S <= 16 ? 16 : (S <= 32 ? 32 : 64);
    static constexpr int RPT = 64 / RP;
    static constexpr int NTG = S > 0 ? (S + RPT - 1) / RPT : 0;   // key tiles per window
    static constexpr int SP = S > 0 ? NTG * RPT + 1 : 1;          // relh table row (fp32 words, odd => conflict-free)
    static constexpr int NRW = S > 0 ? RP / 2 : 1;                // width-bias registers per lane
    static constexpr int RELROWS = 2 * S - 1;                     // rows of a rel-pos table
};

// ---- dynamic LDS of each kernel: section offsets (bytes) and the total.  The kernel carves its pointers from it, the launcher requests
// `total` -- the two cannot disagree.
// wg_attn_kernel<HD, S, NW, KB>:  kv [2 buffers][K tile | V tile] | tab (grid: per-wave rel-pos table; plain: the key bias row, whole tiles of Lk)
struct AttnLds { size_t kv, tab, total; };
template <int HD, int S> constexpr AttnLds wg_attn_lds(int nw, int Lk) {
    using G = AttnGeom<HD, S>;
    const size_t tab = 2 * G::TILE2;
    return {0, tab, tab + (S > 0 ? (size_t)nw * 32 * G::SP * 4 : (size_t)((Lk + 63) / 64) * 64 * 4)};
}
// wg_attn_window_kernel<HD, S, NW>:  kv | tab (per-wave rel-pos table in key space) | rels (rel_w | rel_h rows [2][RELROWS][HD]) |
// qslab (per wave: the next unit's query fragments, KSTEPS x 1 KiB) | relw (head_dim 80: a lane-private row of the width term, 80-byte pitch)
struct AttnWindowLds { size_t kv, tab, rels, qslab, relw, total; };
template <int HD, int S> constexpr AttnWindowLds wg_attn_window_lds(int nw) {
    using G = AttnGeom<HD, S>;
    const size_t tab = 2 * G::TILE2, rels = tab + (size_t)nw * 32 * G::SP * 4, qslab = rels + 2 * G::RELROWS * HD * 2;
    const size_t relw = qslab + (size_t)nw * G::KSTEPS * 1024;
    return {0, tab, rels, qslab, relw, relw + (HD == 80 ? (size_t)nw * 64 * 80 : 0)};
}
// wg_attn_window_unit_kernel<HD, S, NW>:  kv [2 units][NTG tiles][K tile | V tile] | tab | rels
struct AttnWindowUnitLds { size_t kv, tab, rels, total; };
template <int HD, int S> constexpr AttnWindowUnitLds wg_attn_window_unit_lds(int nw) {
    using G = AttnGeom<HD, S>;
    const size_t tab = 2 * G::NTG * G::TILE2, rels = tab + (size_t)nw * 32 * G::SP * 4;
    return {0, tab, rels, rels + 2 * G::RELROWS * HD * 2};
}
// the bytes each compiled combination requests (occupancy follows from them: a change here is a change of a launch)
static_assert(wg_attn_window_lds<64, 14>(4).total == 64768 && wg_attn_window_lds<64, 32>(8).total == 115456 && wg_attn_window_lds<32, 14>(7).total == 49408 &&
              wg_attn_window_lds<32, 28>(5).total == 52224 && wg_attn_window_lds<80, 14>(7).total == 146752, "window kernel LDS");
static_assert(wg_attn_lds<64, 64>(8, 0).total == 99328 && wg_attn_lds<80, 64>(8, 0).total == 117760, "global kernel LDS");
static_assert(wg_attn_lds<16, 0>(1, 1025).total == 20736 && wg_attn_lds<32, 0>(4, 1025).total == 20736 && wg_attn_lds<64, 0>(4, 1025).total == 37120 &&
              wg_attn_lds<128, 0>(8, 1025).total == 69888, "plain kernel LDS: two buffers + four bytes per key of the whole tiles");
static_assert(wg_attn_window_unit_lds<64, 14>(7).total == 153216, "unit kernel LDS");

// raw v_exp_f32: exp2f() adds a denormal-range fix-up (compare, select, ldexp) around it that triples the cost of the
// one instruction softmax cannot avoid; arguments here are <= RESCALE_THR and results below 2^-126 may flush to zero.
__device__ __forceinline__ float wg_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// ds_read_b64_tr_b16 through inline asm.  The builtin form makes hipcc park an `s_waitcnt vmcnt(0)` in front of the
// first transposed read (it cannot tell the V tile being read from the LDS-DMA still writing the NEXT tile), which
// drains the prefetch in the middle of every tile.  The asm form is invisible to that pass; the matching wait is
// wg_tr_wait() below (cdna_hip_programming.md §5.7: own wait + sched_barrier before the consumers).
template <int OFF> __device__ __forceinline__ u32x2 wg_ds_read_tr(unsigned lds_addr) {
    u32x2 v;
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(lds_addr), "i"(OFF));
    return v;
}


// ---- device pieces the kernels of attn.hip and attn_window_unit.hip have in common --------------------------------------------------------
// Only these two: hipcc's register allocation of these kernels shifts when their code is reshaped, and moving the unit decode, the staging
// set-up, the V^T address set-up, the rel-pos pass or the epilogue store out of the kernels changed their instruction streams
// (tools/isa_fingerprint.py against the commit before tells); those stay written out in each kernel.

// this lane's query row as the B operand of the S^T MFMAs: its half (hi) of every 16 head dims
template <int KSTEPS>
__device__ __forceinline__ void wg_attn_load_q(const AttnArgs& a, long qrow, int hcol, int hi, bf16x8 (&q)[KSTEPS]) {
    const bf16* qp = a.Q + qrow * a.ldq + hcol + 8 * hi;
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) q[s] = *(const bf16x8*)(qp + 16 * s);
}

// the two transposed reads (key rows 16 ks + .. and + 8) of k-step ks behind a lane's V^T address, i.e. the operands of one P.V MFMA
// (the offset must be an immediate: switch on the unrolled ks)
template <int ROWBV> __device__ __forceinline__ void wg_attn_vt_pair(int ks, unsigned ad, u32x2 (&v)[2]) {
    switch (ks) {
        case 0: v[0] = wg_ds_read_tr<0 * 16 * ROWBV>(ad); v[1] = wg_ds_read_tr<0 * 16 * ROWBV + 8 * ROWBV>(ad); break;
        case 1: v[0] = wg_ds_read_tr<1 * 16 * ROWBV>(ad); v[1] = wg_ds_read_tr<1 * 16 * ROWBV + 8 * ROWBV>(ad); break;
        case 2: v[0] = wg_ds_read_tr<2 * 16 * ROWBV>(ad); v[1] = wg_ds_read_tr<2 * 16 * ROWBV + 8 * ROWBV>(ad); break;
        default: v[0] = wg_ds_read_tr<3 * 16 * ROWBV>(ad); v[1] = wg_ds_read_tr<3 * 16 * ROWBV + 8 * ROWBV>(ad); break;
    }
}

// attn_pipe.hip: the software-pipelined kernel for head_dim 64 (SAM global attention, CLIP without a key mask)
bool wg_attn_pipe_takes(const AttnArgs& a, int head_dim, int S, int nw);
int wg_attn_pipe_launch(const AttnArgs& a, int S, int nw, hipStream_t st);

// attn_window_unit.hip: SAM's 14 x 14 windows at head_dim 64 with a whole (window, head) of K / V staged ahead
bool wg_attn_window_unit_takes(const AttnArgs& a);
int wg_attn_window_unit_launch(AttnArgs a, int groups, hipStream_t st);

// The epilogue of a head_dim-64 attention kernel in its fp8 form: lane (query, hi) holds rows 8 g4 + 4 hi + e of the two 32-row blocks of O^T,
// i.e. 16 of the 32 columns of the MX block (query row, head, d); its partner lane ^ 32 holds the other 16.  The rule is wg_quantize_mx_fp8's on
// the bf16-ROUNDED output (what the quantisation pass used to read back): scale = the power of two at or above max|block| / 448.
template <int DB>
__device__ __forceinline__ void wg_attn_store_mx(const f32x16 (&ot)[DB], float inv_l, bool valid, long row, int hcol, int hi, const AttnArgs& a) {
    const long r = row % 128;
    const long spos = (row - r) + (r % 16) * 8 + r / 16;
#pragma unroll
    for (int d = 0; d < DB; ++d) {
        float v[16], am = 0x1p-100f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            v[i] = (float)(bf16)(ot[d][i] * inv_l);
            am = fmaxf(am, fabsf(v[i]));
        }
        am = wg_xor32_max(am);
        const unsigned bits = __builtin_bit_cast(unsigned, am * (1.0f / 448.0f));
        unsigned e8 = (bits >> 23) + ((bits & 0x7FFFFFu) ? 1u : 0u);
        e8 = e8 > 253u ? 253u : e8;
        const float s = __builtin_bit_cast(float, (254u - e8) << 23);
        if (valid) {
            unsigned char* qp = a.Oq + row * a.ldoq + hcol + 32 * d + 4 * hi;
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                int w = 0;
                w = __builtin_amdgcn_cvt_pk_fp8_f32(v[4 * g4] * s, v[4 * g4 + 1] * s, w, false);
                w = __builtin_amdgcn_cvt_pk_fp8_f32(v[4 * g4 + 2] * s, v[4 * g4 + 3] * s, w, true);
                *(unsigned*)(qp + 8 * g4) = (unsigned)w;
            }
            if (hi == 0) a.Omx[(long)((hcol + 32 * d) >> 5) * a.mx_pitch + spos] = (unsigned char)e8;
        }
    }
}
