// attention_extend.hip -- the attention of one LATER TURN of a conversation: ONE sequence, a block of R new rows at positions
// p .. p + R - 1 (p a host value: the number of rows the session's cache already holds) over that cache, fused like vcla_attn_verify:
//   RoPE(q), RoPE(k_new) for all R rows  ->  append the R new K / V rows to the cache  ->  row j attends over keys [0, p + j].
//
// The shape is a SHORT block over a LONG cache (a follow-up question is 10 - 60 tokens, the conversation hundreds to ~2000), which neither
// existing kernel is laid out for: the causal prefill kernel (attention_mfma.hip) launches ceil(R / 128) x H workgroups -- 32 on a 256-CU
// part at H = 32, each walking its head's whole cache alone, behind a separate RoPE / append launch -- and vcla_attn_verify stops at 16
// rows and multiplies on the VALU.  Here:
//   grid      (key split, q-tile, head).  A q-tile is NW waves x 32 query rows (NW = 2 up to 64 rows: such a block is ONE q-tile, so every
//             cached row of a head is read once per pass; NW = 4 above).  The key tiles a q-tile may see, [0, p + its last row], are cut
//             into S contiguous splits; S is chosen on the host from p + R so that the launch is about two workgroups per CU, each
//             with at least two key tiles.
//   products  both on v_mfma_f32_16x16x32_bf16 in the swapped form of attention_mfma.hip (S^T = K Q^T, O^T = V^T P^T: a softmax row lives
//             in one lane column, P never moves between lanes, V^T fragments by ds_read_b64_tr_b16 from the row-major tile); online
//             softmax per wave in the log2 domain; the next tile's rows are in flight in registers under this tile's MFMAs.
//   new rows  keys >= p never come from the cache: the staging threads take them from `qkv` and rotate K on the way into LDS, so no
//             workgroup reads a row another one writes.  Workgroup (split 0, q-tile 0) of each head writes the R new rows to the cache,
//             through the same function (rope_pair: the arithmetic and roundings of vcla_rope_kv_append's bf16 kernel).
//   merge     S = 1: the wave normalises and stores.  S > 1: per-split (o, m, l) go to scratch and attn_extend_merge_kernel combines them
//             (attention_verify.hip's form, one more grid dimension).
// bf16, head dim 128 or 64, no key mask (a session refuses masked prompts).
//
// Second entry, vcla_attn_extend_rows (at the end of the file): the same tile code (ax_block) for the blocks of SEVERAL sequences of a slots
// cache in one launch -- the ragged admission pass of generate_many(share_prefix=True).  Only the mapping from workgroups to work differs:
// a 1-D work list of (sequence, q-tile, key split) built on the host, the splits chosen from the total work (rule stated there).
//
// PAGED (vcla_attn_extend_rows_paged): the cache is the pool [H][n_blocks * 16][d] of attention_decode.hip's paged form and logical row j of
// slot b lives at physical row table[b * ld + (j >> 4)] * 16 + (j & 15) of the head's slab.  Only two address computations change -- the
// cached-row loads of load_tile and the append -- so a paged call is bit for bit the contiguous one over the same rows.
#include "vcla_common.h"
#include <vector>

namespace {
constexpr int XKV = 64;            // keys per tile
constexpr int X_MAX_SPLITS = 16;
constexpr int X_TARGET_WGS = 512;  // about two workgroups per CU of the 256-CU part

// LDS images of a tile, as attention_mfma.hip lays them out: K rows with their 16-byte chunks XOR-swizzled (conflict-free ds_read_b128
// fragments), V rows with 32-byte column blocks XOR-swizzled for the transpose reads
template <int D> __device__ __forceinline__ int ax_k_off(int key, int ch) {
    if (D == 128) return key * 256 + ((ch ^ (key & 15)) << 4);
    return key * 128 + ((ch ^ ((key >> 1) & 7)) << 4);
}
template <int D> __device__ __forceinline__ int ax_v_off(int key, int d) {
    constexpr int CB = D / 16;
    const int f = D == 128 ? key : key >> 1;
    return key * (D * 2) + ((((d >> 4) ^ f) & (CB - 1)) << 5) + ((d & 15) << 1);
}
typedef __attribute__((ext_vector_type(4))) short ax_s16x4_t;
typedef __attribute__((address_space(3))) ax_s16x4_t* ax_lds_v4_t;

// RoPE of 8 (x[i], x[i + d/2]) pairs at one position: bf16-rounded cos / sin, fp32 products, one rounding of each result -- the body
// of rope_kv_vec_kernel (embed.hip), so that an appended K row is bitwise what vcla_rope_kv_append writes
__device__ __forceinline__ void rope_pair(const uint4& lo, const uint4& hi, const float* __restrict__ cs, const float* __restrict__ sn, uint4& olo,
                                          uint4& ohi) {
    float c[8], s_[8], a[8], b_[8], r0[8], r1[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { c[e] = Act<bf16_t>::rnd(cs[e]); s_[e] = Act<bf16_t>::rnd(sn[e]); }
    bf8_to_f32(lo, a); bf8_to_f32(hi, b_);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        // a c - b s and b c + a s as that kernel's compiled code forms them: one product rounded, the other fused into the sum
        r0[e] = __builtin_fmaf(a[e], c[e], -(b_[e] * s_[e]));
        r1[e] = __builtin_fmaf(a[e], s_[e], b_[e] * c[e]);
    }
    olo = make_uint4(pack_bf2(r0[0], r0[1]), pack_bf2(r0[2], r0[3]), pack_bf2(r0[4], r0[5]), pack_bf2(r0[6], r0[7]));
    ohi = make_uint4(pack_bf2(r1[0], r1[1]), pack_bf2(r1[2], r1[3]), pack_bf2(r1[4], r1[5]), pack_bf2(r1[6], r1[7]));
}
__device__ __forceinline__ u32x4_t as_v4(const uint4& t) { return u32x4_t{t.x, t.y, t.z, t.w}; }

// element (row m, column k) of the fragment-major layout of vcla_gemm_args.A_frag with MT 16-row tiles
__device__ __forceinline__ int64_t ax_frag_index(int m, int k, int MT) {
    return ((((int64_t)(k >> 5) * MT + (m >> 4)) * 64 + ((k & 31) >> 3) * 16 + (m & 15)) << 3) + (k & 7);
}

// PAGED: the block table of the launch by value; the contiguous instantiations take an empty struct in its place
template <bool PAGED> struct AxPages {};
template <> struct AxPages<true> { const int32_t* table; int ld; int n_blocks; };
// The table is never written by a kernel that reads it: through the constant address space a load at a wave-uniform index is a scalar load
typedef const __attribute__((address_space(4))) int32_t* ax_table_p;

struct ExtendPlan { int nw, qb, nqt, S; };
inline ExtendPlan extend_plan(int R, int H, int p) {
    ExtendPlan e;
    e.nw = R <= 64 ? 2 : 4;
    e.qb = e.nw * 32;
    e.nqt = (R + e.qb - 1) / e.qb;
    const int ntiles = (p + R + XKV - 1) / XKV;
    int S = X_TARGET_WGS / (H * e.nqt);
    S = S < 1 ? 1 : (S > X_MAX_SPLITS ? X_MAX_SPLITS : S);
    const int cap = ntiles / 2 > 1 ? ntiles / 2 : 1;       // at least two key tiles per split: a split's partials cost as much as a tile
    e.S = S < cap ? S : cap;
    return e;
}
}  // namespace

// One work item of one head: the query rows [qt_idx * QB, ...) of a block of R new rows at positions p .. p + R - 1 against split `split` of S
// of the key tiles they may see.  qkv: the block's first row; kb / vb: the head's K / V rows of the block's sequence ([ctx_max][D]); out_row0:
// the block's first row in `out` (0 for a single sequence, its first packed row in vcla_attn_extend_rows); pw0: the [QB][D + 4] fp32 partials
// of this work item (S > 1); append: this work item writes the head's R new K / V rows.  Shared by both kernels below, which differ only in
// how a workgroup finds these values.
// PAGED: kb / vb are the head's slab of the pool, trow the slot's row of the block table, n_blocks the pool's size.  A table word outside
// [0, n_blocks) is never turned into an address: the cached keys of such a block are staged as zeros and masked, an append through it is
// skipped.  Words are read only for blocks [0, (p - 1) >> 4] (cached keys) and [p >> 4, (p + R - 1) >> 4] (the append): the blocks the
// sequence owns, because a key clamped to Tk - 1 >= p comes from qkv, never through the table.
template <int D, int NW, bool PAGED = false>
__device__ __forceinline__ void ax_block(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ kb, bf16_t* __restrict__ vb,
                                         const float* __restrict__ cos_tab, const float* __restrict__ sin_tab, bf16_t* __restrict__ out, int out_row0,
                                         float* __restrict__ pw0, int R, int H, int p, float scale, int out_mt, int split, int S, int qt_idx, int h,
                                         bool append, const int32_t* __restrict__ trow = nullptr, int n_blocks = 0) {
    constexpr int QB = NW * 32, NT = NW * 64;
    constexpr int HALF = D / 2;
    constexpr int KST = D / 32;         // MFMA k-steps over the head dim (Q K^T)
    constexpr int DT = D / 16;          // 16-wide output d tiles (P V)
    constexpr int CH = D / 8;           // 16-byte chunks per K/V row
    constexpr int NLD = XKV * CH / NT;  // staging loads per thread per operand
    static_assert(XKV * CH % NT == 0, "whole staging rounds");
    __shared__ __attribute__((aligned(16))) unsigned char lds_all[2 * XKV * D * 2];      // [K tile | V tile]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int HD = H * D;
    const int q0 = qt_idx * QB;                  // first query row of this workgroup
    const int qw = q0 + wave * 32;               // first query row of this wave
    const int Tk = p + R;
    const bf16_t* qh = qkv + h * D;              // row r: q at qh + r*3HD, k at + HD, v at + 2HD
    const int ql = lane & 15, g = lane >> 4;
    const bool wave_active = qw < R;             // waves past the end only help staging

    // ---- the R new rows enter the cache: one workgroup per head writes them, none reads them back
    if (append) {
        for (int idx = tid; idx < R * (CH / 2); idx += NT) {
            const int r = idx / (CH / 2), i = (idx % (CH / 2)) * 8;
            [[maybe_unused]] int64_t arow = 0;
            if constexpr (PAGED) {
                const int word = trow[(p + r) >> 4];
                if ((unsigned)word >= (unsigned)n_blocks) continue;      // no block behind this row: nothing is written
                arow = (int64_t)word * VCLA_KV_BLOCK_ROWS + ((p + r) & (VCLA_KV_BLOCK_ROWS - 1));
            }
            const bf16_t* krow = qh + (int64_t)r * 3 * HD + HD;
            uint4 lo, hi;
            rope_pair(*reinterpret_cast<const uint4*>(krow + i), *reinterpret_cast<const uint4*>(krow + i + HALF),
                      cos_tab + (int64_t)(p + r) * HALF + i, sin_tab + (int64_t)(p + r) * HALF + i, lo, hi);
            if constexpr (PAGED) {
                *reinterpret_cast<uint4*>(kb + arow * D + i) = lo;
                *reinterpret_cast<uint4*>(kb + arow * D + i + HALF) = hi;
            } else {
                *reinterpret_cast<uint4*>(kb + (int64_t)(p + r) * D + i) = lo;
                *reinterpret_cast<uint4*>(kb + (int64_t)(p + r) * D + i + HALF) = hi;
            }
        }
        for (int idx = tid; idx < R * CH; idx += NT) {
            const int r = idx / CH, i = (idx % CH) * 8;
            if constexpr (PAGED) {
                const int word = trow[(p + r) >> 4];
                if ((unsigned)word >= (unsigned)n_blocks) continue;
                const int64_t arow = (int64_t)word * VCLA_KV_BLOCK_ROWS + ((p + r) & (VCLA_KV_BLOCK_ROWS - 1));
                *reinterpret_cast<uint4*>(vb + arow * D + i) = *reinterpret_cast<const uint4*>(qh + (int64_t)r * 3 * HD + 2 * HD + i);
            } else {
                *reinterpret_cast<uint4*>(vb + (int64_t)(p + r) * D + i) = *reinterpret_cast<const uint4*>(qh + (int64_t)r * 3 * HD + 2 * HD + i);
            }
        }
    }

    // ---- Q fragments (B port), rotated: lane (q = ql, g) holds Q[q][s*32 + g*8 .. +8]; the RoPE partner of chunk s is chunk s + KST/2 of
    // the same lane
    bf16x8_t qf[2][KST];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        int qr = qw + qt * 16 + ql;
        if (qr >= R) qr = R - 1;
        const bf16_t* qrow = qh + (int64_t)qr * 3 * HD;
#pragma unroll
        for (int s = 0; s < KST / 2; ++s) {
            const int i = s * 32 + g * 8;
            uint4 lo, hi;
            rope_pair(*reinterpret_cast<const uint4*>(qrow + i), *reinterpret_cast<const uint4*>(qrow + i + HALF),
                      cos_tab + (int64_t)(p + qr) * HALF + i, sin_tab + (int64_t)(p + qr) * HALF + i, lo, hi);
            qf[qt][s] = __builtin_bit_cast(bf16x8_t, lo);
            qf[qt][s + KST / 2] = __builtin_bit_cast(bf16x8_t, hi);
        }
    }

    f32x4_t o[2][DT];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt)
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) o[qt][dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    float m_run[2] = {-INFINITY, -INFINITY}, l_run[2] = {0.f, 0.f};
    const float sl2 = scale * 1.44269504088896340736f;  // scores are kept in the log2 domain

    // ---- this split's share of the key tiles the q-tile may see (causal: up to its last row)
    const int last_q = (q0 + QB < R ? q0 + QB : R) - 1;
    const int kv_end = p + last_q + 1;
    const int ntiles = (kv_end + XKV - 1) / XKV;
    const int per = (ntiles + S - 1) / S;
    const int t_lo = split * per, t_hi = t_lo + per < ntiles ? t_lo + per : ntiles;

    // ---- staging: cached rows from the cache, new rows (keys >= p) from qkv with K rotated on the way
    u32x4_t rk[NLD], rv[NLD];
    // PAGED: the four table words of a 64-key tile (key group t of the tile is logical block tile * 4 + t) as scalar loads: the staging
    // lanes of one wave and load cover 64 / CH keys aligned to that count, inside ONE 16-row block, so the word a lane needs is
    // wave-uniform.  The words are fetched at the TOP of the loop trip whose load_tile forms addresses from them (fetch_words), in front
    // of the barriers around store_tile: the barrier's wait covers them, so no scalar load is outstanding while tile_body reads LDS (a
    // scalar load in flight would turn its counted LDS waits into waits for everything).  Blocks behind the last cached key are
    // clamped to it (their keys are >= p and never go through the table).  ok_next / ok_cur: bit t = word t of the tile in flight / in
    // LDS names a pool block.
    constexpr int GID = CH * VCLA_KV_BLOCK_ROWS;                     // staging ids per 16-row block
    static_assert(!PAGED || (XKV == 4 * VCLA_KV_BLOCK_ROWS && (NT <= GID ? GID % NT == 0 : NT % GID == 0)), "a wave's keys of one load sit in one block");
    [[maybe_unused]] int ok_next = 0, ok_cur = 0;
    [[maybe_unused]] const int q_wave = NT > GID ? __builtin_amdgcn_readfirstlane(tid / GID) : 0;
    [[maybe_unused]] int tw[4] = {0, 0, 0, 0};                       // the words of the tile the NEXT load_tile call stages
    auto fetch_words = [&](int tile) {
        if constexpr (PAGED) {
            const ax_table_p ct = (ax_table_p)(uintptr_t)trow;
            const int lastb = p > 0 ? (p - 1) >> 4 : 0;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int b = tile * 4 + t;
                tw[t] = ct[b < lastb ? b : lastb];
            }
        }
    };
    auto load_tile = [&](int tile) {
        if constexpr (PAGED) {
            ok_next = 0;
#pragma unroll
            for (int t = 0; t < 4; ++t) ok_next |= (int)((unsigned)tw[t] < (unsigned)n_blocks) << t;
        }
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int id = i * NT + tid, key = id / CH, ch = id % CH;
            int kg = tile * XKV + key;
            if (kg >= Tk) kg = Tk - 1;           // clamp; masked below
            if (kg < p) {
                if constexpr (PAGED) {
                    const int q = (i * NT) / GID + q_wave;           // = key >> 4, wave-uniform
                    const int word = q == 0 ? tw[0] : q == 1 ? tw[1] : q == 2 ? tw[2] : tw[3];
                    if ((unsigned)word < (unsigned)n_blocks) {
                        const int64_t row = (int64_t)word * VCLA_KV_BLOCK_ROWS + (kg & (VCLA_KV_BLOCK_ROWS - 1));
                        rk[i] = *reinterpret_cast<const u32x4_t*>(kb + row * D + ch * 8);
                        rv[i] = *reinterpret_cast<const u32x4_t*>(vb + row * D + ch * 8);
                    } else {                                        // no block: zeros (finite under the mask of tile_body), no load
                        rk[i] = u32x4_t{0u, 0u, 0u, 0u};
                        rv[i] = u32x4_t{0u, 0u, 0u, 0u};
                    }
                } else {
                    rk[i] = *reinterpret_cast<const u32x4_t*>(kb + (int64_t)kg * D + ch * 8);
                    rv[i] = *reinterpret_cast<const u32x4_t*>(vb + (int64_t)kg * D + ch * 8);
                }
            } else {
                const bf16_t* row = qh + (int64_t)(kg - p) * 3 * HD;
                const int cl = (ch % (CH / 2)) * 8;
                uint4 lo, hi;
                rope_pair(*reinterpret_cast<const uint4*>(row + HD + cl), *reinterpret_cast<const uint4*>(row + HD + cl + HALF),
                          cos_tab + (int64_t)kg * HALF + cl, sin_tab + (int64_t)kg * HALF + cl, lo, hi);
                rk[i] = ch < CH / 2 ? as_v4(lo) : as_v4(hi);
                rv[i] = *reinterpret_cast<const u32x4_t*>(row + 2 * HD + ch * 8);
            }
        }
    };
    auto store_tile = [&]() {
        if constexpr (PAGED) ok_cur = ok_next;
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int id = i * NT + tid, key = id / CH, ch = id % CH;
            *reinterpret_cast<u32x4_t*>(lds_all + ax_k_off<D>(key, ch)) = rk[i];
            *reinterpret_cast<u32x4_t*>(lds_all + XKV * D * 2 + ax_v_off<D>(key, ch * 8)) = rv[i];
        }
    };

    // ---- one key tile of 64 keys against the wave's 32 query rows
    auto tile_body = [&](int kv0) {
        constexpr int NTK = 4, NS = 2;
        const unsigned char* ks = lds_all;
        const auto v_lds = (__attribute__((address_space(3))) unsigned char*)lds_all + XKV * D * 2;
        f32x4_t sacc[2][NTK];
#pragma unroll
        for (int qt = 0; qt < 2; ++qt)
#pragma unroll
            for (int t = 0; t < NTK; ++t) sacc[qt][t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KST; ++s) {
#pragma unroll
            for (int t = 0; t < NTK; ++t) {
                const bf16x8_t kf = *reinterpret_cast<const bf16x8_t*>(ks + ax_k_off<D>(t * 16 + ql, s * 4 + g));
                sacc[0][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[0][s], sacc[0][t], 0, 0, 0);
                sacc[1][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[1][s], sacc[1][t], 0, 0, 0);
            }
        }
        if constexpr (PAGED) {
            if (ok_cur != 15) {                  // a cached key group without a block (never under a validated table): its keys are masked
#pragma unroll
                for (int qt = 0; qt < 2; ++qt)
#pragma unroll
                    for (int t = 0; t < NTK; ++t)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (!((ok_cur >> t) & 1) && kv0 + t * 16 + g * 4 + r < p) sacc[qt][t][r] = -INFINITY;
            }
        }
        // lane holds keys kv0 + t*16 + g*4 + r of query rows qw + qt*16 + ql; row j sees keys <= p + j (wave-uniform test first)
        if (kv0 + XKV - 1 > qw + p) {
#pragma unroll
            for (int qt = 0; qt < 2; ++qt) {
                const int klim = p + qw + qt * 16 + ql;          // last visible key (rows >= R are never stored)
#pragma unroll
                for (int t = 0; t < NTK; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int key = kv0 + t * 16 + g * 4 + r;
                        sacc[qt][t][r] = (key <= klim && key < Tk) ? sacc[qt][t][r] : -INFINITY;
                    }
            }
        }
        bf16x8_t pf[2][NS];
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
            float mx = -INFINITY;
#pragma unroll
            for (int t = 0; t < NTK; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) mx = fmaxf(mx, sacc[qt][t][r]);
            mx *= sl2;                                   // log2 domain (-inf stays -inf)
            mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float m_new = fmaxf(m_run[qt], mx);
            const float m_use = (m_new == -INFINITY) ? 0.f : m_new;  // nothing visible so far: keep everything at 0
            const float alpha = exp2f(m_run[qt] - m_use);             // exp2(-inf) = 0 on the first tile
            m_run[qt] = m_new;
            float ps = 0.f;
            float pv[NTK * 4];
#pragma unroll
            for (int t = 0; t < NTK; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float pp = __builtin_amdgcn_exp2f(__builtin_fmaf(sacc[qt][t][r], sl2, -m_use));
                    pv[t * 4 + r] = pp;
                    ps += pp;
                }
            l_run[qt] = l_run[qt] * alpha + ps;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) o[qt][dt] *= alpha;
            // P^T fragments: key-step s takes S tiles (2s, 2s+1): slots j<4 from tile 2s, j>=4 from tile 2s+1
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                uint4 u;
                u.x = pack_bf2(pv[(2 * s) * 4 + 0], pv[(2 * s) * 4 + 1]);
                u.y = pack_bf2(pv[(2 * s) * 4 + 2], pv[(2 * s) * 4 + 3]);
                u.z = pack_bf2(pv[(2 * s + 1) * 4 + 0], pv[(2 * s + 1) * 4 + 1]);
                u.w = pack_bf2(pv[(2 * s + 1) * 4 + 2], pv[(2 * s + 1) * 4 + 3]);
                pf[qt][s] = __builtin_bit_cast(bf16x8_t, u);
            }
        }
        // ---- O^T += V^T P^T
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                // lane (ql, g): piece (key row ql / 4, 8 bytes ql % 4) of the 4-key x 16-d blocks of S tiles 2s and 2s + 1
                const int kr = g * 4 + (ql >> 2), dc = dt * 16 + (ql & 3) * 4;
                const ax_s16x4_t v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ax_lds_v4_t)(v_lds + ax_v_off<D>((2 * s) * 16 + kr, dc)));
                const ax_s16x4_t v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ax_lds_v4_t)(v_lds + ax_v_off<D>((2 * s + 1) * 16 + kr, dc)));
                const bf16x8_t vf = __builtin_bit_cast(bf16x8_t, __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7));
                o[0][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[0][s], o[0][dt], 0, 0, 0);
                o[1][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[1][s], o[1][dt], 0, 0, 0);
            }
        }
    };

    if (t_lo < t_hi) {
        if constexpr (PAGED) fetch_words(t_lo);
        load_tile(t_lo);
    }
    for (int tile = t_lo; tile < t_hi; ++tile) {
        if constexpr (PAGED) fetch_words(tile + 1 < t_hi ? tile + 1 : tile);      // the tile this trip's load_tile stages
        __syncthreads();          // previous tile fully consumed
        store_tile();
        __syncthreads();
        load_tile(tile + 1 < t_hi ? tile + 1 : tile);      // unconditional (the last one is a harmless re-load): keeps the prefetch
                                                           // registers out of the private segment
        const int kv0 = tile * XKV;
        // a wave whose rows all precede this tile has nothing to do here
        if (wave_active && kv0 <= (qw + 31 < R ? qw + 31 : R - 1) + p) tile_body(kv0);
    }
    if (!wave_active) return;

    // ---- epilogue: lane holds d = dt*16 + g*4 + r of query row qw + qt*16 + ql
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        float l = l_run[qt];
        l += __shfl_xor(l, 16, 64);
        l += __shfl_xor(l, 32, 64);
        const int qrow = qw + qt * 16 + ql;
        if (qrow >= R) continue;
        if (S == 1) {
            const float inv = l > 0.f ? 1.0f / l : 0.f;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                float v[4] = {o[qt][dt][0] * inv, o[qt][dt][1] * inv, o[qt][dt][2] * inv, o[qt][dt][3] * inv};
                const int k = h * D + dt * 16 + g * 4;
                Act<bf16_t>::st4(out_mt > 0 ? out + ax_frag_index(out_row0 + qrow, k, out_mt) : out + (int64_t)(out_row0 + qrow) * HD + k, v);
            }
        } else {
            float* pw = pw0 + (int64_t)(qrow - q0) * (D + 4);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) *reinterpret_cast<f32x4_t*>(pw + dt * 16 + g * 4) = o[qt][dt];
            if (g == 0) { pw[D] = m_run[qt]; pw[D + 1] = l; }
        }
    }
}

// grid (key split, q-tile, head) of ONE sequence
template <int D, int NW>
__global__ __launch_bounds__(NW * 64) void attn_extend_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ kc, bf16_t* __restrict__ vc,
                                                              const float* __restrict__ cos_tab, const float* __restrict__ sin_tab,
                                                              bf16_t* __restrict__ out, float* __restrict__ part, int R, int H, int ctx_max, int p,
                                                              float scale, int out_mt) {
    constexpr int QB = NW * 32;
    const int split = blockIdx.x, S = gridDim.x, qt_idx = blockIdx.y, nqt = gridDim.y, h = blockIdx.z;
    ax_block<D, NW>(qkv, kc + (int64_t)h * ctx_max * D, vc + (int64_t)h * ctx_max * D, cos_tab, sin_tab, out, 0,
                    part + (((int64_t)h * nqt + qt_idx) * S + split) * QB * (D + 4), R, H, p, scale, out_mt, split, S, qt_idx, h,
                    split == 0 && qt_idx == 0);
}

// S > 1: out[r, h, :] = sum_s o_s 2^(m_s - m) / sum_s l_s 2^(m_s - m).  A thread owns 4 consecutive d of one row, a workgroup 256 / (D / 4)
// rows of one head: the grid is as wide as the block has rows, so the partials are read at the device's rate, not at 32 workgroups'
template <int D>
__global__ __launch_bounds__(256) void attn_extend_merge_kernel(const float* __restrict__ part, bf16_t* __restrict__ out, int R, int H, int S, int QB,
                                                               int nqt, int out_mt) {
    constexpr int LPR = D / 4, RPB = 256 / LPR;              // lanes per row, rows per workgroup
    const int h = blockIdx.y, row = blockIdx.x * RPB + threadIdx.x / LPR, dd = (threadIdx.x % LPR) * 4;
    if (row >= R) return;
    const int qt_idx = row / QB, r = row % QB;
    const float* base = part + ((((int64_t)h * nqt + qt_idx) * S) * QB + r) * (D + 4);
    const int64_t ss = (int64_t)QB * (D + 4);                // stride between the splits of one row
    float mf = -INFINITY;
    for (int s = 0; s < S; ++s) mf = fmaxf(mf, base[s * ss + D]);
    const float mu = mf == -INFINITY ? 0.f : mf;
    float lf = 0.f;
    f32x4_t of = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int s = 0; s < S; ++s) {
        const float* pw = base + s * ss;
        const float a = exp2f(pw[D] - mu);
        lf += pw[D + 1] * a;
        of += *reinterpret_cast<const f32x4_t*>(pw + dd) * a;
    }
    const float inv = lf > 0.f ? 1.0f / lf : 0.f;
    float v[4] = {of[0] * inv, of[1] * inv, of[2] * inv, of[3] * inv};
    const int k = h * D + dd;
    Act<bf16_t>::st4(out_mt > 0 ? out + ax_frag_index(row, k, out_mt) : out + (int64_t)row * H * D + k, v);
}

extern "C" size_t vcla_attn_extend_scratch_bytes(int R, int H, int d, int p) {
    if (R <= 0 || R > VCLA_EXTEND_MAX_ROWS || H <= 0 || d <= 0 || p < 0) return 0;
    const ExtendPlan e = extend_plan(R, H, p);
    return e.S > 1 ? (size_t)H * e.nqt * e.S * e.qb * (d + 4) * sizeof(float) : 0;
}

template <int D, int NW>
static int launch_extend(const void* qkv, void* kc, void* vc, const float* cos_tab, const float* sin_tab, void* out, int R, int H, int ctx_max, int p,
                         float scale, int out_mt, const ExtendPlan& e, float* scratch, hipStream_t s) {
    attn_extend_kernel<D, NW><<<dim3(e.S, e.nqt, H), NW * 64, 0, s>>>((const bf16_t*)qkv, (bf16_t*)kc, (bf16_t*)vc, cos_tab, sin_tab, (bf16_t*)out,
                                                                     scratch, R, H, ctx_max, p, scale, out_mt);
    VCLA_CHECK_LAUNCH("attn_extend_kernel");
    if (e.S > 1) {
        constexpr int RPB = 256 / (D / 4);
        attn_extend_merge_kernel<D><<<dim3((R + RPB - 1) / RPB, H), 256, 0, s>>>(scratch, (bf16_t*)out, R, H, e.S, e.qb, e.nqt, out_mt);
        VCLA_CHECK_LAUNCH("attn_extend_merge_kernel");
    }
    return VCLA_OK;
}

extern "C" int vcla_attn_extend(const void* qkv, void* k_cache, void* v_cache, const float* cos_tab, const float* sin_tab, void* out, int R, int H,
                                int d, int ctx_max, int p, float scale, int dtype, int out_frag, void* scratch, size_t scratch_bytes, void* stream) {
    VCLA_REQUIRE(dtype == VCLA_BF16, VCLA_ERR_BAD_DTYPE, "attn_extend: bad dtype %d (bf16 rows and a bf16 cache only)", dtype);
    VCLA_REQUIRE(d == 64 || d == 128, VCLA_ERR_BAD_SHAPE, "attn_extend: head dim %d not in {64,128}", d);
    VCLA_REQUIRE(R >= 1 && R <= VCLA_EXTEND_MAX_ROWS && H > 0 && ctx_max > 0 && p >= 0 && p + R <= ctx_max, VCLA_ERR_BAD_SHAPE,
                 "attn_extend: R=%d (1..%d) H=%d ctx_max=%d p=%d", R, VCLA_EXTEND_MAX_ROWS, H, ctx_max, p);
    VCLA_REQUIRE(qkv && k_cache && v_cache && cos_tab && sin_tab && out, VCLA_ERR_BAD_ARG, "attn_extend: null pointer");
    VCLA_REQUIRE(vcla_aligned(qkv, 16) && vcla_aligned(k_cache, 16) && vcla_aligned(v_cache, 16) && vcla_aligned(out, 16), VCLA_ERR_BAD_ARG,
                 "attn_extend: qkv, the caches and out must be 16-byte aligned");
    VCLA_REQUIRE(!out_frag || (R <= 64 && (H * d) % 32 == 0), VCLA_ERR_BAD_ARG, "attn_extend: out_frag needs R <= 64 (got %d) and H*d %% 32 == 0", R);
    const ExtendPlan e = extend_plan(R, H, p);
    const size_t need = vcla_attn_extend_scratch_bytes(R, H, d, p);
    VCLA_REQUIRE(scratch_bytes >= need && (need == 0 || (scratch && vcla_aligned(scratch, 16))), VCLA_ERR_WORKSPACE,
                 "attn_extend: scratch %zu < %zu bytes", scratch_bytes, need);
    const int out_mt = out_frag ? (R + 15) / 16 : 0;
    hipStream_t s = (hipStream_t)stream;
#define XT_CASE(DD, NN) return launch_extend<DD, NN>(qkv, k_cache, v_cache, cos_tab, sin_tab, out, R, H, ctx_max, p, scale, out_mt, e, (float*)scratch, s)
    if (d == 64) {
        if (e.nw == 2) XT_CASE(64, 2);
        XT_CASE(64, 4);
    }
    if (e.nw == 2) XT_CASE(128, 2);
    XT_CASE(128, 4);
#undef XT_CASE
}

// ------------------------------------------------------------------ vcla_attn_extend_rows: the blocks of SEVERAL sequences in one launch
// n_seqs blocks of new rows packed back to back in qkv [M, 3 H d], block i = R_i rows at positions p_i .. of slot b_i of a slots cache
// [B_slots][H][ctx_max][d].  Per block exactly what attn_extend_kernel does for its one sequence (the same ax_block); what differs is how a
// workgroup finds its work.  The host flattens (sequence, q-tile, key split) into a 1-D WORK LIST, grid (n_work, H):
//   q-tiles   one NW for the launch: 2 waves (64-row q-tiles) when every block has R <= 64, else 4 waves (128-row q-tiles).
//   splits    chosen from the TOTAL work.  A q-tile sees nt key tiles; NT = the sum over all q-tiles; the launch should be about
//             X_TARGET_WGS workgroups, i.e. budget = max(1, X_TARGET_WGS / H) work items, so a work item should walk
//             tpw = max(2, ceil(NT / budget)) key tiles, and q-tile t gets S_t = min(ceil(nt_t / tpw), X_MAX_SPLITS, max(1, nt_t / 2)) splits:
//             64 short blocks get one split each (they fill the device by their number), one long block gets what attn_extend_kernel
//             gives it.  Work items with S > 1 number at most 2 * budget, which bounds the partials whatever the table.
//   merge     one entry per q-tile with S > 1 ({first partial, S, first packed row, rows}); attn_extend_rows_merge_kernel, grid
//             (entries * QB / rows-per-workgroup, H).
// The two lists live at the head of the caller's scratch, in front of the partials; the host writes them there (one copy per call, or none
// when the caller says the scratch still holds the lists of the same table: the 32 layers of one decoder pass).
namespace {
struct AxWork { int32_t slot, p, R, m0, qt, split, S, part; };      // part: index of the work item's partials (S > 1)
struct AxMerge { int32_t part0, S, row0, rows; };
struct RowsPlan {
    int nw = 2, qb = 64, n_parts = 0;
    std::vector<AxWork> work;
    std::vector<AxMerge> merge;
};
inline size_t ax_up256(size_t x) { return (x + 255) & ~(size_t)255; }

inline void rows_plan(const vcla_extend_seq* seqs, int n_seqs, int H, RowsPlan& pl) {
    pl.work.clear(); pl.merge.clear(); pl.n_parts = 0;
    int max_r = 0;
    for (int i = 0; i < n_seqs; ++i) max_r = seqs[i].rows > max_r ? seqs[i].rows : max_r;
    pl.nw = max_r <= 64 ? 2 : 4;
    pl.qb = pl.nw * 32;
    auto tiles_of = [&](const vcla_extend_seq& q, int qt) {
        const int last_q = ((qt + 1) * pl.qb < q.rows ? (qt + 1) * pl.qb : q.rows) - 1;
        return (q.pos + last_q + 1 + XKV - 1) / XKV;
    };
    int64_t total = 0;
    for (int i = 0; i < n_seqs; ++i)
        for (int qt = 0; qt * pl.qb < seqs[i].rows; ++qt) total += tiles_of(seqs[i], qt);
    const int budget = X_TARGET_WGS / H > 1 ? X_TARGET_WGS / H : 1;
    int tpw = (int)((total + budget - 1) / budget);
    tpw = tpw < 2 ? 2 : tpw;
    for (int i = 0; i < n_seqs; ++i)
        for (int qt = 0; qt * pl.qb < seqs[i].rows; ++qt) {
            const int nt = tiles_of(seqs[i], qt);
            int S = (nt + tpw - 1) / tpw;
            S = S > X_MAX_SPLITS ? X_MAX_SPLITS : S;
            const int cap = nt / 2 > 1 ? nt / 2 : 1;
            S = S < cap ? S : cap;
            if (S > 1) {
                const int rows = seqs[i].rows - qt * pl.qb < pl.qb ? seqs[i].rows - qt * pl.qb : pl.qb;
                pl.merge.push_back(AxMerge{pl.n_parts, S, seqs[i].row0 + qt * pl.qb, rows});
            }
            for (int sp = 0; sp < S; ++sp)
                pl.work.push_back(AxWork{seqs[i].slot, seqs[i].pos, seqs[i].rows, seqs[i].row0, qt, sp, S, S > 1 ? pl.n_parts + sp : 0});
            if (S > 1) pl.n_parts += S;
        }
}
inline size_t rows_lists_bytes(size_t n_work, size_t n_merge) { return ax_up256(n_work * sizeof(AxWork)) + ax_up256(n_merge * sizeof(AxMerge)); }
thread_local RowsPlan g_rows_plan;       // (thread_local: the lists outlive the call that copies them to the device)
}  // namespace

template <int D, int NW, bool PAGED = false>
__global__ __launch_bounds__(NW * 64) void attn_extend_rows_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ kc, bf16_t* __restrict__ vc,
                                                                   const float* __restrict__ cos_tab, const float* __restrict__ sin_tab,
                                                                   bf16_t* __restrict__ out, float* __restrict__ part, const AxWork* __restrict__ work,
                                                                   int H, int ctx_max, float scale, int out_mt, AxPages<PAGED> pg) {
    constexpr int QB = NW * 32;
    const AxWork w = work[blockIdx.x];           // workgroup-uniform: scalar loads, no vector register held for it
    const int h = blockIdx.y;
    if constexpr (PAGED) {
        // the pool is ONE sequence of n_blocks * 16 rows per head; the slot enters through its row of the table
        const int64_t head = (int64_t)h * pg.n_blocks * VCLA_KV_BLOCK_ROWS * D;
        ax_block<D, NW, true>(qkv + (int64_t)w.m0 * 3 * H * D, kc + head, vc + head, cos_tab, sin_tab, out, w.m0,
                              part + ((int64_t)w.part * H + h) * QB * (D + 4), w.R, H, w.p, scale, out_mt, w.split, w.S, w.qt, h,
                              w.split == 0 && w.qt == 0, pg.table + (int64_t)w.slot * pg.ld, pg.n_blocks);
    } else {
        const int64_t head = ((int64_t)w.slot * H + h) * ctx_max * D;
        ax_block<D, NW>(qkv + (int64_t)w.m0 * 3 * H * D, kc + head, vc + head, cos_tab, sin_tab, out, w.m0,
                        part + ((int64_t)w.part * H + h) * QB * (D + 4), w.R, H, w.p, scale, out_mt, w.split, w.S, w.qt, h, w.split == 0 && w.qt == 0);
    }
}

// the merge of attn_extend_merge_kernel per list entry: partials [part][H][QB][D + 4]
template <int D>
__global__ __launch_bounds__(256) void attn_extend_rows_merge_kernel(const float* __restrict__ part, bf16_t* __restrict__ out,
                                                                    const AxMerge* __restrict__ merge, int H, int QB, int out_mt) {
    constexpr int LPR = D / 4, RPB = 256 / LPR;
    const int per = QB / RPB;
    const AxMerge e = merge[blockIdx.x / per];
    const int h = blockIdx.y, r = (blockIdx.x % per) * RPB + threadIdx.x / LPR, dd = (threadIdx.x % LPR) * 4;
    if (r >= e.rows) return;
    const float* base = part + (((int64_t)e.part0 * H + h) * QB + r) * (D + 4);
    const int64_t ss = (int64_t)H * QB * (D + 4);
    float mf = -INFINITY;
    for (int s = 0; s < e.S; ++s) mf = fmaxf(mf, base[s * ss + D]);
    const float mu = mf == -INFINITY ? 0.f : mf;
    float lf = 0.f;
    f32x4_t of = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int s = 0; s < e.S; ++s) {
        const float* pw = base + s * ss;
        const float a = exp2f(pw[D] - mu);
        lf += pw[D + 1] * a;
        of += *reinterpret_cast<const f32x4_t*>(pw + dd) * a;
    }
    const float inv = lf > 0.f ? 1.0f / lf : 0.f;
    float v[4] = {of[0] * inv, of[1] * inv, of[2] * inv, of[3] * inv};
    const int row = e.row0 + r, k = h * D + dd;
    Act<bf16_t>::st4(out_mt > 0 ? out + ax_frag_index(row, k, out_mt) : out + (int64_t)row * H * D + k, v);
}

extern "C" size_t vcla_attn_extend_rows_scratch_bytes(const vcla_extend_seq* seqs, int n_seqs, int H, int d) {
    if (!seqs || n_seqs <= 0 || H <= 0 || d <= 0) return 0;
    RowsPlan pl;
    rows_plan(seqs, n_seqs, H, pl);
    return rows_lists_bytes(pl.work.size(), pl.merge.size()) + (size_t)pl.n_parts * H * pl.qb * (d + 4) * sizeof(float);
}

// the most any table of n_seqs blocks with M rows in all can need (what a workspace is sized by before the tables are known)
extern "C" size_t vcla_attn_extend_rows_scratch_bound(int M, int n_seqs, int H, int d) {
    if (M <= 0 || n_seqs <= 0 || H <= 0 || d <= 0) return 0;
    const size_t budget = X_TARGET_WGS / H > 1 ? X_TARGET_WGS / H : 1;
    const size_t n_qt = (size_t)n_seqs + M / 64;                       // q-tiles: ceil(R_i / 64) <= R_i / 64 + 1 each
    const size_t n_work = n_qt + 2 * budget;                           // one item per q-tile with S = 1, at most 2 * budget items with S > 1
    return rows_lists_bytes(n_work, n_qt) + 2 * budget * H * 128 * (d + 4) * sizeof(float);
}

template <int D, int NW>
static int launch_extend_rows(const void* qkv, void* kc, void* vc, const float* cos_tab, const float* sin_tab, void* out, int H, int ctx_max, float scale,
                              int out_mt, const RowsPlan& pl, const AxWork* work, const AxMerge* merge, float* part, hipStream_t s,
                              const vcla_kv_pages* pages = nullptr) {
    if (pages) {
        attn_extend_rows_kernel<D, NW, true><<<dim3((unsigned)pl.work.size(), H), NW * 64, 0, s>>>(
            (const bf16_t*)qkv, (bf16_t*)kc, (bf16_t*)vc, cos_tab, sin_tab, (bf16_t*)out, part, work, H, ctx_max, scale, out_mt,
            AxPages<true>{pages->table, pages->ld, pages->n_blocks});
        VCLA_CHECK_LAUNCH(D == 128 ? (NW == 2 ? "attn_extend_rows_kernel<D=128,NW=2,PAGED=true>" : "attn_extend_rows_kernel<D=128,NW=4,PAGED=true>")
                                   : (NW == 2 ? "attn_extend_rows_kernel<D=64,NW=2,PAGED=true>" : "attn_extend_rows_kernel<D=64,NW=4,PAGED=true>"));
    } else {
        attn_extend_rows_kernel<D, NW><<<dim3((unsigned)pl.work.size(), H), NW * 64, 0, s>>>((const bf16_t*)qkv, (bf16_t*)kc, (bf16_t*)vc, cos_tab, sin_tab,
                                                                                            (bf16_t*)out, part, work, H, ctx_max, scale, out_mt, AxPages<false>{});
        VCLA_CHECK_LAUNCH("attn_extend_rows_kernel");
    }
    if (!pl.merge.empty()) {
        constexpr int RPB = 256 / (D / 4);
        attn_extend_rows_merge_kernel<D><<<dim3((unsigned)pl.merge.size() * (NW * 32 / RPB), H), 256, 0, s>>>(part, (bf16_t*)out, merge, H, NW * 32, out_mt);
        VCLA_CHECK_LAUNCH("attn_extend_rows_merge_kernel");
    }
    return VCLA_OK;
}

// pages: the paged entry (checked there); NULL: the contiguous slots cache
static int attn_extend_rows_impl(const void* qkv, void* k_cache, void* v_cache, const float* cos_tab, const float* sin_tab, void* out,
                                 const vcla_extend_seq* seqs, int n_seqs, int M, int B_slots, int H, int d, int ctx_max, float scale, int dtype,
                                 int out_frag, int lists_ready, void* scratch, size_t scratch_bytes, void* stream, const vcla_kv_pages* pages) {
    VCLA_REQUIRE(dtype == VCLA_BF16, VCLA_ERR_BAD_DTYPE, "attn_extend_rows: bad dtype %d (bf16 rows and a bf16 cache only)", dtype);
    VCLA_REQUIRE(d == 64 || d == 128, VCLA_ERR_BAD_SHAPE, "attn_extend_rows: head dim %d not in {64,128}", d);
    VCLA_REQUIRE(seqs && n_seqs >= 1 && M >= 1 && B_slots >= 1 && n_seqs <= B_slots && H > 0 && ctx_max > 0, VCLA_ERR_BAD_SHAPE,
                 "attn_extend_rows: n_seqs=%d M=%d B_slots=%d H=%d ctx_max=%d", n_seqs, M, B_slots, H, ctx_max);
    VCLA_REQUIRE(qkv && k_cache && v_cache && cos_tab && sin_tab && out, VCLA_ERR_BAD_ARG, "attn_extend_rows: null pointer");
    VCLA_REQUIRE(vcla_aligned(qkv, 16) && vcla_aligned(k_cache, 16) && vcla_aligned(v_cache, 16) && vcla_aligned(out, 16), VCLA_ERR_BAD_ARG,
                 "attn_extend_rows: qkv, the caches and out must be 16-byte aligned");
    VCLA_REQUIRE(!out_frag || (M <= 64 && (H * d) % 32 == 0), VCLA_ERR_BAD_ARG, "attn_extend_rows: out_frag needs M <= 64 (got %d) and H*d %% 32 == 0", M);
    RowsPlan& pl = g_rows_plan;
    if (!lists_ready) {
        // the table: blocks packed back to back, inside their slots, every slot once -- checked before anything is written
        std::vector<char> seen((size_t)B_slots, 0);
        int next = 0;
        for (int i = 0; i < n_seqs; ++i) {
            const vcla_extend_seq& q = seqs[i];
            VCLA_REQUIRE(q.rows >= 1 && q.rows <= VCLA_EXTEND_MAX_ROWS && q.pos >= 0 && q.pos + q.rows <= ctx_max && q.row0 == next, VCLA_ERR_BAD_SHAPE,
                         "attn_extend_rows: block %d: rows=%d (1..%d) pos=%d ctx_max=%d row0=%d (expected %d)", i, q.rows, VCLA_EXTEND_MAX_ROWS, q.pos, ctx_max,
                         q.row0, next);
            VCLA_REQUIRE(q.slot >= 0 && q.slot < B_slots && !seen[q.slot], VCLA_ERR_BAD_ARG, "attn_extend_rows: block %d: slot %d outside 0..%d or named twice", i,
                         q.slot, B_slots - 1);
            seen[q.slot] = 1;
            next += q.rows;
        }
        VCLA_REQUIRE(next == M, VCLA_ERR_BAD_SHAPE, "attn_extend_rows: the blocks hold %d rows, M=%d", next, M);
        rows_plan(seqs, n_seqs, H, pl);
    }
    // lists_ready: the caller vouches that table, H and scratch are those of this thread's previous call; its plan and its checks stand
    VCLA_REQUIRE(!pl.work.empty(), VCLA_ERR_BAD_ARG, "attn_extend_rows: lists_ready without a previous call on this thread");
    const size_t wl = ax_up256(pl.work.size() * sizeof(AxWork)), lists = rows_lists_bytes(pl.work.size(), pl.merge.size());
    const size_t need = lists + (size_t)pl.n_parts * H * pl.qb * (d + 4) * sizeof(float);
    VCLA_REQUIRE(scratch && vcla_aligned(scratch, 16) && scratch_bytes >= need, VCLA_ERR_WORKSPACE, "attn_extend_rows: scratch %zu < %zu bytes", scratch_bytes,
                 need);
    hipStream_t s = (hipStream_t)stream;
    const AxWork* work = (const AxWork*)scratch;
    const AxMerge* merge = (const AxMerge*)((char*)scratch + wl);
    float* part = (float*)((char*)scratch + lists);
    if (!lists_ready) {
        VCLA_CHECK_HIP(hipMemcpyAsync((void*)work, pl.work.data(), pl.work.size() * sizeof(AxWork), hipMemcpyHostToDevice, s));
        if (!pl.merge.empty())
            VCLA_CHECK_HIP(hipMemcpyAsync((void*)merge, pl.merge.data(), pl.merge.size() * sizeof(AxMerge), hipMemcpyHostToDevice, s));
    }
    const int out_mt = out_frag ? (M + 15) / 16 : 0;
    void *kc = k_cache, *vc = v_cache;
#define XR_CASE(DD, NN) return launch_extend_rows<DD, NN>(qkv, kc, vc, cos_tab, sin_tab, out, H, ctx_max, scale, out_mt, pl, work, merge, part, s, pages)
    if (d == 64) {
        if (pl.nw == 2) XR_CASE(64, 2);
        XR_CASE(64, 4);
    }
    if (pl.nw == 2) XR_CASE(128, 2);
    XR_CASE(128, 4);
#undef XR_CASE
}

extern "C" int vcla_attn_extend_rows(const void* qkv, void* k_cache, void* v_cache, const float* cos_tab, const float* sin_tab, void* out,
                                     const vcla_extend_seq* seqs, int n_seqs, int M, int B_slots, int H, int d, int ctx_max, float scale, int dtype,
                                     int out_frag, int lists_ready, void* scratch, size_t scratch_bytes, void* stream) {
    return attn_extend_rows_impl(qkv, k_cache, v_cache, cos_tab, sin_tab, out, seqs, n_seqs, M, B_slots, H, d, ctx_max, scale, dtype, out_frag, lists_ready,
                                 scratch, scratch_bytes, stream, nullptr);
}

// The same launch over a pool of 16-row blocks [H][n_blocks * 16][d] behind the block table `pages` (device memory, [B_slots][ld], -1 = none):
// ctx_max is the logical cap of a slot, only addresses take the pool.  The caller validates the table (a block with several holders is
// only ever read: every holder's pos lies at or behind its end); the kernel never forms an address from an entry outside [0, n_blocks).
extern "C" int vcla_attn_extend_rows_paged(const void* qkv, void* k_pool, void* v_pool, const float* cos_tab, const float* sin_tab, void* out,
                                           const vcla_extend_seq* seqs, int n_seqs, int M, int B_slots, int H, int d, int ctx_max, float scale, int dtype,
                                           int out_frag, int lists_ready, void* scratch, size_t scratch_bytes, const vcla_kv_pages* pages, void* stream) {
    VCLA_REQUIRE(pages && pages->table && pages->n_blocks >= 1, VCLA_ERR_BAD_ARG, "attn_extend_rows_paged: a null block table, or an empty pool");
    VCLA_REQUIRE(d == 64 || d == 128, VCLA_ERR_BAD_SHAPE, "attn_extend_rows_paged: head dim %d not in {64,128}", d);
    VCLA_REQUIRE(ctx_max > 0 && (int64_t)pages->ld * VCLA_KV_BLOCK_ROWS >= ctx_max, VCLA_ERR_BAD_SHAPE,
                 "attn_extend_rows_paged: a table row of %d blocks does not cover ctx_max %d", pages->ld, ctx_max);
    // (row * d elements of 2 bytes stay a 32-bit offset inside a head's slab, as in vcla_attn_decode_paged)
    VCLA_REQUIRE((int64_t)pages->n_blocks * VCLA_KV_BLOCK_ROWS * d * 2 < ((int64_t)1 << 32), VCLA_ERR_BAD_SHAPE,
                 "attn_extend_rows_paged: n_blocks=%d: a head's slab must stay below 4 GiB", pages->n_blocks);
    return attn_extend_rows_impl(qkv, k_pool, v_pool, cos_tab, sin_tab, out, seqs, n_seqs, M, B_slots, H, d, ctx_max, scale, dtype, out_frag, lists_ready,
                                 scratch, scratch_bytes, stream, pages);
}
