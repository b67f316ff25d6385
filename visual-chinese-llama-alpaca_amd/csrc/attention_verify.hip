// attention_verify.hip -- the attention of one prompt-lookup verify pass: ONE sequence, R = k + 1 <= 16 query rows at positions
// p .. p + R - 1 (p = pos0 + *pos_dev, read from device memory so that the launch replays from a hipGraph), fused like
// vcla_attn_decode_fused:
//   RoPE(q), RoPE(k_new) for all R rows  ->  append the R new K / V rows to the cache  ->  row j attends over keys [0, p + j].
//
// The point of the kernel: every cached K / V row of a head is read from HBM ONCE per pass for all R queries, so verifying k drafts
// costs about what decoding one token costs.  Workgroup = (head, split), 256 threads.  The keys [0, p + R) are cut into S contiguous
// splits (S from ctx_max, so the grid is fixed for graph replay; S > 1 once ctx_max > 256 keys); each walks its share in tiles of
// KT = 32 keys:
//   stage  the tile's K / V rows (fp32 in LDS; the NEXT tile's rows are already in flight in registers while this one is computed);
//          keys >= p are the new rows, taken from LDS -- only split 0 writes them to the cache, so no workgroup reads a row another
//          one writes;
//   scores thread (key, row group) forms q_r . k for two query rows per K fetch from LDS (R x 32 per tile);
//   softmax 16 lanes per query row: online max / sum, probabilities back to LDS (transposed, so a P V thread reads 8 rows at once);
//   P V    thread (dim, row group) accumulates D/16 query rows of one output dim, one V read from LDS per key.
// S = 1: the workgroup normalises and stores.  S > 1: per-split (o, m, l) go to the scratch buffer and attn_verify_merge_kernel
// combines them (the long-context split of the decode engine, as a second launch).
// Scores are VALU dot products: at R <= 16 rows the MFMA tile would be mostly padding for small k, and the pass is bound by streaming
// the K / V rows, not by the R x 32 x D multiply-adds per tile (cdna_hip_programming.md section 3, 5).
#include "vcla_common.h"

namespace {
constexpr int VR = 16;     // max query rows
constexpr int KT = 32;     // keys per tile
constexpr int NT = 256;    // threads

// 16-byte loads of a cache row chunk, kept raw until committed to LDS (lets the next tile's loads overlap this tile's math)
template <typename T> struct Raw16;
template <> struct Raw16<float> {
    static constexpr int EL = 4;
    float4 t;
    __device__ __forceinline__ void load(const float* p) { t = *reinterpret_cast<const float4*>(p); }
    __device__ __forceinline__ void get(float* v) const { v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
};
template <> struct Raw16<bf16_t> {
    static constexpr int EL = 8;
    uint4 t;
    __device__ __forceinline__ void load(const bf16_t* p) { t = *reinterpret_cast<const uint4*>(p); }
    __device__ __forceinline__ void get(float* v) const { bf8_to_f32(t, v); }
};

__device__ __forceinline__ int64_t frag_index(int r, int k) {   // fragment-major element (row r < 16, column k), one 16-row tile
    return ((((int64_t)(k >> 5)) * 64 + ((k & 31) >> 3) * 16 + (r & 15)) << 3) + (k & 7);
}
}  // namespace

template <typename T, int D>
__global__ __launch_bounds__(NT) void attn_verify_kernel(const T* __restrict__ qkv, T* __restrict__ kc, T* __restrict__ vc,
                                                        const float* __restrict__ cos_tab, const float* __restrict__ sin_tab,
                                                        T* __restrict__ out, float* __restrict__ part, int R, int H, int ctx_max, int pos0,
                                                        const int32_t* __restrict__ pos_dev, const int32_t* __restrict__ key_mask,
                                                        float scale, int out_frag) {
    constexpr int HALF = D / 2, KLD = D + 4;                  // padded K tile rows: the score threads read 32 rows at once
    constexpr int EL = Raw16<T>::EL, CPR = D / EL;            // 16-byte chunks per row
    constexpr int NLD = (KT * CPR + NT - 1) / NT;             // chunk loads per thread per tile and matrix
    constexpr int RG = NT / D, RPG = VR / RG;                 // P V: row groups, rows per group (= D / 16)
    __shared__ __attribute__((aligned(16))) float qs[VR * D];
    __shared__ __attribute__((aligned(16))) float knw[VR * D];
    __shared__ __attribute__((aligned(16))) float vnw[VR * D];
    __shared__ __attribute__((aligned(16))) float Kt[KT * KLD];
    __shared__ __attribute__((aligned(16))) float Vt[KT * D];
    __shared__ __attribute__((aligned(16))) float pT[KT * VR];   // probabilities, [key][row]
    __shared__ float alph[VR], lrow[VR], mrow[VR];

    const int tid = threadIdx.x, h = blockIdx.x, sidx = blockIdx.y, S = gridDim.y;
    const int p = pos0 + (pos_dev ? *pos_dev : 0);
    const int HD = H * D;
    T* kbase = kc + (int64_t)h * ctx_max * D;
    T* vbase = vc + (int64_t)h * ctx_max * D;

    // ---- RoPE of q / k for all R rows, values staged; split 0 appends the rows to the cache (the same roundings as the decode kernels,
    // so the cache holds what R sequential decode steps would have written)
    for (int i = tid; i < VR * HALF; i += NT) {
        const int r = i / HALF, c = i % HALF;
        if (r >= R) continue;
        const int pr = min(p + r, ctx_max - 1);          // rows past the cache are never attended to or stored
        const T* row = qkv + (int64_t)r * 3 * HD + h * D;
        const float cr = Act<T>::rnd(cos_tab[(int64_t)pr * HALF + c]), sr = Act<T>::rnd(sin_tab[(int64_t)pr * HALF + c]);
        const float q0 = Act<T>::ld(row + c), q1 = Act<T>::ld(row + c + HALF);
        qs[r * D + c] = Act<T>::rnd(q0 * cr - q1 * sr);
        qs[r * D + c + HALF] = Act<T>::rnd(q1 * cr + q0 * sr);
        const float k0 = Act<T>::ld(row + HD + c), k1 = Act<T>::ld(row + HD + c + HALF);
        const float r0 = Act<T>::rnd(k0 * cr - k1 * sr), r1 = Act<T>::rnd(k1 * cr + k0 * sr);
        knw[r * D + c] = r0; knw[r * D + c + HALF] = r1;
        if (sidx == 0 && p + r < ctx_max) {
            Act<T>::st(kbase + (int64_t)(p + r) * D + c, r0);
            Act<T>::st(kbase + (int64_t)(p + r) * D + c + HALF, r1);
        }
    }
    for (int i = tid; i < VR * D; i += NT) {
        const int r = i / D, c = i % D;
        if (r >= R) continue;
        const float v = Act<T>::ld(qkv + (int64_t)r * 3 * HD + 2 * HD + h * D + c);
        vnw[r * D + c] = v;
        if (sidx == 0 && p + r < ctx_max) Act<T>::st(vbase + (int64_t)(p + r) * D + c, v);
    }

    // ---- this split's share of the keys [0, N)
    const int N = min(p + R, ctx_max);
    const int chunk = ((N + S - 1) / S + KT - 1) / KT * KT;
    const int lo = sidx * chunk, hi = min(N, lo + chunk);

    // score phase: key jj = tid % 32 of the tile, query rows g and g + 8; softmax phase: row tid / 16, keys (tid % 16) and +16
    const int sj = tid & (KT - 1), sg = tid >> 5;
    const int xr = tid >> 4, xl = tid & 15;
    // P V phase: output dim od, query rows og * RPG .. + RPG - 1
    const int od = tid % D, og = tid / D;
    float m_run = -INFINITY, l_run = 0.f;
    float o[RPG];
#pragma unroll
    for (int i = 0; i < RPG; ++i) o[i] = 0.f;

    Raw16<T> rk[NLD], rv[NLD];
    auto fetch = [&](int t0) {
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int idx = tid + i * NT, jj = idx / CPR, c = idx % CPR, j = t0 + jj;
            if (idx < KT * CPR && j < hi && j < p) {
                rk[i].load(kbase + (int64_t)j * D + c * EL);
                rv[i].load(vbase + (int64_t)j * D + c * EL);
            }
        }
    };
    if (lo < hi) fetch(lo);
    __syncthreads();      // qs / knw / vnw complete

    for (int t0 = lo; t0 < hi; t0 += KT) {
        // ---- commit the fetched rows (or the new rows from LDS, or zeros past the split) to the tile
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int idx = tid + i * NT, jj = idx / CPR, c = idx % CPR, j = t0 + jj;
            if (idx < KT * CPR) {
                float kv[EL], vv[EL];
                if (j < hi && j < p) {
                    rk[i].get(kv);
                    rv[i].get(vv);
                } else if (j < hi) {
#pragma unroll
                    for (int e = 0; e < EL; ++e) { kv[e] = knw[(j - p) * D + c * EL + e]; vv[e] = vnw[(j - p) * D + c * EL + e]; }
                } else {
#pragma unroll
                    for (int e = 0; e < EL; ++e) { kv[e] = 0.f; vv[e] = 0.f; }
                }
#pragma unroll
                for (int e = 0; e < EL; ++e) { Kt[jj * KLD + c * EL + e] = kv[e]; Vt[jj * D + c * EL + e] = vv[e]; }
            }
        }
        __syncthreads();
        if (t0 + KT < hi) fetch(t0 + KT);                 // next tile in flight during this one's math

        // ---- scores, two query rows per K read
        {
            const int j = t0 + sj;
            const int r0 = sg, r1 = sg + 8;
            float a0 = 0.f, a1 = 0.f;
            const float* kr = Kt + sj * KLD;
#pragma unroll 8
            for (int c = 0; c < D; c += 4) {
                const float4 kk = *reinterpret_cast<const float4*>(kr + c);
                const float4 x0 = *reinterpret_cast<const float4*>(qs + r0 * D + c);
                const float4 x1 = *reinterpret_cast<const float4*>(qs + r1 * D + c);
                a0 += x0.x * kk.x + x0.y * kk.y + x0.z * kk.z + x0.w * kk.w;
                a1 += x1.x * kk.x + x1.y * kk.y + x1.z * kk.z + x1.w * kk.w;
            }
            const bool vis = j < hi && (!key_mask || key_mask[j] != 0);
            pT[sj * VR + r0] = (vis && r0 < R && j <= p + r0) ? a0 * scale : -INFINITY;
            pT[sj * VR + r1] = (vis && r1 < R && j <= p + r1) ? a1 * scale : -INFINITY;
        }
        __syncthreads();
        // ---- online softmax, 16 lanes per query row (xor offsets < 16 stay inside the row's lanes)
        {
            const float s0 = pT[xl * VR + xr], s1 = pT[(xl + 16) * VR + xr];
            float tm = fmaxf(s0, s1);
#pragma unroll
            for (int off = 8; off >= 1; off >>= 1) tm = fmaxf(tm, __shfl_xor(tm, off, 64));
            const float mn = fmaxf(m_run, tm);
            float al = 1.f, p0 = 0.f, p1 = 0.f;
            if (mn > -INFINITY) {
                al = __expf(m_run - mn);                 // m_run = -inf: 0 (nothing accumulated yet)
                p0 = __expf(s0 - mn);
                p1 = __expf(s1 - mn);
            }
            float ps = p0 + p1;
#pragma unroll
            for (int off = 8; off >= 1; off >>= 1) ps += __shfl_xor(ps, off, 64);
            l_run = l_run * al + ps;
            m_run = mn;
            pT[xl * VR + xr] = p0;
            pT[(xl + 16) * VR + xr] = p1;
            if (xl == 0) alph[xr] = al;
        }
        __syncthreads();
        // ---- P V
        {
            float acc[RPG];
#pragma unroll
            for (int i = 0; i < RPG; ++i) acc[i] = o[i] * alph[og * RPG + i];
#pragma unroll 4
            for (int jj = 0; jj < KT; ++jj) {
                const float v = Vt[jj * D + od];
                const float* pr = pT + jj * VR + og * RPG;
#pragma unroll
                for (int i = 0; i < RPG; ++i) acc[i] = __builtin_fmaf(pr[i], v, acc[i]);
            }
#pragma unroll
            for (int i = 0; i < RPG; ++i) o[i] = acc[i];
        }
        __syncthreads();      // the tile buffers are rewritten next trip
    }
    if (xl == 0) { lrow[xr] = l_run; mrow[xr] = m_run; }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < RPG; ++i) {
        const int r = og * RPG + i;
        if (r >= R) continue;
        if (S == 1) {
            const float l = lrow[r];
            const float v = l > 0.f ? o[i] / l : 0.f;
            if (out_frag) Act<T>::st(out + frag_index(r, h * D + od), v);
            else Act<T>::st(out + (int64_t)r * HD + h * D + od, v);
        } else {
            float* pw = part + (((int64_t)h * S + sidx) * VR + r) * (D + 2);
            pw[od] = o[i];
            if (od == 0) { pw[D] = mrow[r]; pw[D + 1] = lrow[r]; }
        }
    }
}

// S > 1: out[r, h, :] = sum_s o_s exp(m_s - m) / sum_s l_s exp(m_s - m)
template <typename T, int D>
__global__ __launch_bounds__(NT) void attn_verify_merge_kernel(const float* __restrict__ part, T* __restrict__ out, int R, int H, int S,
                                                              int out_frag) {
    const int h = blockIdx.x;
    for (int e = threadIdx.x; e < R * D; e += NT) {
        const int r = e / D, dd = e % D;
        float mf = -INFINITY;
        for (int s = 0; s < S; ++s) mf = fmaxf(mf, part[(((int64_t)h * S + s) * VR + r) * (D + 2) + D]);
        const float mu = mf == -INFINITY ? 0.f : mf;
        float lf = 0.f, of = 0.f;
        for (int s = 0; s < S; ++s) {
            const float* pw = part + (((int64_t)h * S + s) * VR + r) * (D + 2);
            const float a = __expf(pw[D] - mu);
            lf += pw[D + 1] * a;
            of += pw[dd] * a;
        }
        const float v = lf > 0.f ? of / lf : 0.f;
        if (out_frag) Act<T>::st(out + frag_index(r, h * D + dd), v);
        else Act<T>::st(out + (int64_t)r * H * D + h * D + dd, v);
    }
}

static int verify_splits(int ctx_max) {
    const int s = (ctx_max + 255) / 256;
    return s < 1 ? 1 : (s > 8 ? 8 : s);
}

extern "C" size_t vcla_attn_verify_scratch_bytes(int H, int d, int ctx_max) {
    if (H <= 0 || d <= 0 || ctx_max <= 0) return 0;
    const int S = verify_splits(ctx_max);
    return S > 1 ? (size_t)H * S * VR * (d + 2) * sizeof(float) : 0;
}

template <typename T, int D>
static int launch_verify(const void* qkv, void* kc, void* vc, const float* cos_tab, const float* sin_tab, void* out, int R, int H, int ctx_max,
                         int pos0, const int32_t* pos_dev, const int32_t* key_mask, float scale, int out_frag, float* scratch, hipStream_t s) {
    const int S = verify_splits(ctx_max);
    attn_verify_kernel<T, D><<<dim3(H, S), NT, 0, s>>>((const T*)qkv, (T*)kc, (T*)vc, cos_tab, sin_tab, (T*)out, scratch, R, H, ctx_max, pos0,
                                                       pos_dev, key_mask, scale, out_frag);
    VCLA_CHECK_LAUNCH(S > 1 ? "attn_verify_kernel<split>" : "attn_verify_kernel<S=1>");
    if (S > 1) {
        attn_verify_merge_kernel<T, D><<<H, NT, 0, s>>>(scratch, (T*)out, R, H, S, out_frag);
        VCLA_CHECK_LAUNCH("attn_verify_merge_kernel");      // (runs only behind attn_verify_kernel<split>)
    }
    return VCLA_OK;
}

extern "C" int vcla_attn_verify(const void* qkv, void* k_cache, void* v_cache, const float* cos_tab, const float* sin_tab, void* out, int R, int H,
                                int d, int ctx_max, int pos0, const int32_t* pos_dev, const int32_t* key_mask, float scale, int dtype, int out_frag,
                                void* scratch, size_t scratch_bytes, void* stream) {
    VCLA_REQUIRE(dtype == VCLA_F32 || dtype == VCLA_BF16, VCLA_ERR_BAD_DTYPE, "attn_verify: bad dtype %d (the e4m3 cache is not supported)", dtype);
    VCLA_REQUIRE(d == 32 || d == 64 || d == 128, VCLA_ERR_BAD_SHAPE, "attn_verify: head dim %d not in {32,64,128}", d);
    VCLA_REQUIRE(R >= 1 && R <= VR && H > 0 && ctx_max > 0 && pos0 >= 0 && (pos_dev || pos0 + R <= ctx_max), VCLA_ERR_BAD_SHAPE,
                 "attn_verify: R=%d (1..%d) H=%d ctx_max=%d pos0=%d", R, VR, H, ctx_max, pos0);
    VCLA_REQUIRE(qkv && k_cache && v_cache && cos_tab && sin_tab && out, VCLA_ERR_BAD_ARG, "attn_verify: null pointer");
    VCLA_REQUIRE(vcla_aligned(k_cache, 16) && vcla_aligned(v_cache, 16), VCLA_ERR_BAD_ARG, "attn_verify: the caches must be 16-byte aligned");
    VCLA_REQUIRE(!out_frag || (dtype == VCLA_BF16 && (H * d) % 32 == 0), VCLA_ERR_BAD_ARG, "attn_verify: out_frag needs bf16 and H*d %% 32 == 0");
    const size_t need = vcla_attn_verify_scratch_bytes(H, d, ctx_max);
    VCLA_REQUIRE(scratch_bytes >= need && (need == 0 || (scratch && vcla_aligned(scratch, 16))), VCLA_ERR_WORKSPACE,
                 "attn_verify: scratch %zu < %zu bytes", scratch_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    float* sc = (float*)scratch;
#define VF_CASE(TT, DD) return launch_verify<TT, DD>(qkv, k_cache, v_cache, cos_tab, sin_tab, out, R, H, ctx_max, pos0, pos_dev, key_mask, scale, out_frag, sc, s)
    if (dtype == VCLA_F32) {
        if (d == 32) VF_CASE(float, 32);
        if (d == 64) VF_CASE(float, 64);
        VF_CASE(float, 128);
    } else {
        if (d == 32) VF_CASE(bf16_t, 32);
        if (d == 64) VF_CASE(bf16_t, 64);
        VF_CASE(bf16_t, 128);
    }
#undef VF_CASE
}
