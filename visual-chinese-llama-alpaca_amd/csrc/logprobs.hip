// logprobs.hip -- per-token log-probabilities of a slots step.  HF returns them from the scores a generate() call collects
// (hf:generation/utils.py `output_logits` / compute_transition_scores, reached from models/visualcla/modeling_visualcla.py:382-391):
// log_softmax of the [B, V] logits of every step, gathered at the token taken.  Here two launches around the selector of a step:
//   logprob_rows_kernel (BEFORE the selector, on the raw fp32 logits): one 1024-thread workgroup per row, the row read ONCE into
//     registers (52 values per thread, as sample.hip).  lse = max + log(sum exp(x - max)); the k most likely tokens as k block-wide
//     max-reductions over (value desc, id asc) packed into one 64-bit key; optionally the copy of the row that the sampler then
//     consumes (the sampler writes penalties and -inf bans into its input, and the gather below needs the raw row).
//   logprob_pick_kernel (AFTER the selector): one lane per row; a forced id replaces the selected one, and the raw logit of the id
//     taken minus lse is its log-probability.
// Both write at [n_hist_rows[b]][b] of step-major buffers (the layout of vcla_slot_args.history) and skip rows whose length is negative.
#include "vcla_common.h"

#define LP_THREADS 1024
#define LP_PER_THREAD 52   // V <= 53248 = VCLA_SAMPLE_MAX_VOCAB
#define LP_WAVES (LP_THREADS / 64)

static_assert(LP_THREADS * LP_PER_THREAD == VCLA_SAMPLE_MAX_VOCAB, "register slice must cover the largest vocabulary");

// order-preserving float -> unsigned key (ascending), as sample.hip; -0 is keyed as +0, the two are one value to a sort
__device__ __forceinline__ unsigned lp_fkey(float x) {
    const unsigned u = __float_as_uint(x + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// (value, id) -> one key whose maximum is the larger value and, among equal values, the LOWER id (the tie rule of vcla_argmax)
__device__ __forceinline__ unsigned long long lp_pack(float x, int id) { return ((unsigned long long)lp_fkey(x) << 32) | (unsigned)(0xffffffffu - (unsigned)id); }

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned hi = __shfl_xor((unsigned)(v >> 32), o, 64), lo = __shfl_xor((unsigned)v, o, 64);
        const unsigned long long w = ((unsigned long long)hi << 32) | lo;
        v = w > v ? w : v;
    }
    return v;
}

__global__ __launch_bounds__(LP_THREADS) void logprob_rows_kernel(const float* __restrict__ logits, int64_t ld, int V, int B,
                                                                  const int32_t* __restrict__ n_hist_rows, int hist_cap, int k,
                                                                  int64_t* __restrict__ top_ids, float* __restrict__ top_logprobs,
                                                                  float* __restrict__ lse_out, float* __restrict__ copy, int64_t copy_ld) {
    __shared__ float s_f[2][LP_WAVES];
    __shared__ unsigned long long s_k[2][LP_WAVES];
    const int tid = threadIdx.x, b = blockIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = n_hist_rows[b];
    if (h < 0) return;   // workgroup-uniform, ahead of every barrier
    const float* x = logits + (int64_t)b * ld;
    float v[LP_PER_THREAD];
#pragma unroll
    for (int j = 0; j < LP_PER_THREAD; ++j) {
        const int i = tid + j * LP_THREADS;
        v[j] = i < V ? x[i] : -INFINITY;   // columns at or behind V are never read
    }
    if (copy) {
        float* c = copy + (int64_t)b * copy_ld;
#pragma unroll
        for (int j = 0; j < LP_PER_THREAD; ++j) {
            const int i = tid + j * LP_THREADS;
            if (i < V) c[i] = v[j];
        }
    }
    // ---- lse = max + log(sum exp(x - max))
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < LP_PER_THREAD; ++j) m = fmaxf(m, v[j]);
    m = wave_max(m);
    if (lane == 0) s_f[0][wave] = m;
    __syncthreads();
    m = s_f[0][0];
#pragma unroll
    for (int w = 1; w < LP_WAVES; ++w) m = fmaxf(m, s_f[0][w]);
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < LP_PER_THREAD; ++j) sum += expf(v[j] - m);   // a column behind V holds -inf: it adds exp(-inf) = 0
    sum = wave_sum(sum);
    if (lane == 0) s_f[1][wave] = sum;
    __syncthreads();
    sum = 0.f;
#pragma unroll
    for (int w = 0; w < LP_WAVES; ++w) sum += s_f[1][w];
    const float lse = m + logf(sum);
    if (tid == 0) lse_out[b] = lse;
    if (k <= 0 || h >= hist_cap) return;   // uniform
    // ---- the k largest (value desc, id asc): pick t is the largest key strictly below pick t - 1, so nothing is removed from the
    //      registers; a thread re-scans its 52 values only when its own best was the one taken (one thread of the block per pick)
    const int kk = k < V ? k : V;
    //      (a column behind V holds -inf under an id >= V: it ranks behind every real column, and only kk <= V picks are made).
    //      Inside a thread the ids rise with j, so a scan in j order with a strict compare keeps the lowest id of equal values.
    unsigned key[LP_PER_THREAD];
#pragma unroll
    for (int j = 0; j < LP_PER_THREAD; ++j) key[j] = lp_fkey(v[j]);
    unsigned bkey = 0u, bid = 0u;
#pragma unroll
    for (int j = 0; j < LP_PER_THREAD; ++j)
        if (key[j] > bkey) { bkey = key[j]; bid = (unsigned)(tid + j * LP_THREADS); }
    unsigned long long best = ((unsigned long long)bkey << 32) | (0xffffffffu - bid);
    const int64_t o = ((int64_t)h * B + b) * k;
    for (int t = 0; t < kk; ++t) {
        const unsigned long long wbest = wave_max_u64(best);
        if (lane == 0) s_k[t & 1][wave] = wbest;   // the buffer of pick t - 2: every reader of it has passed the barrier of pick t - 1
        __syncthreads();
        unsigned long long win = s_k[t & 1][0];
#pragma unroll
        for (int w = 1; w < LP_WAVES; ++w) { const unsigned long long q = s_k[t & 1][w]; win = q > win ? q : win; }
        if (tid == 0) {
            const unsigned kv = (unsigned)(win >> 32);
            const float val = __uint_as_float((kv & 0x80000000u) ? (kv & 0x7fffffffu) : ~kv);
            top_ids[o + t] = (int64_t)(0xffffffffu - (unsigned)win);
            top_logprobs[o + t] = val - lse;
        }
        if (best == win) {   // this thread's best was taken: its next one is the largest (key, id) behind the winner
            const unsigned wkey = (unsigned)(win >> 32), wid = 0xffffffffu - (unsigned)win;
            bkey = 0u; bid = 0u;
#pragma unroll
            for (int j = 0; j < LP_PER_THREAD; ++j) {
                const unsigned id = (unsigned)(tid + j * LP_THREADS);
                const bool behind = key[j] < wkey || (key[j] == wkey && id > wid);
                if (behind && key[j] > bkey) { bkey = key[j]; bid = id; }
            }
            best = bkey ? ((unsigned long long)bkey << 32) | (0xffffffffu - bid) : 0ull;   // every key of a column is > 0
        }
    }
    if (tid == 0)
        for (int t = kk; t < k; ++t) { top_ids[o + t] = -1; top_logprobs[o + t] = -INFINITY; }   // k > V: nothing is left to rank
}

__global__ void logprob_pick_kernel(const float* __restrict__ logits, int64_t ld, int V, int B, const int32_t* __restrict__ n_hist_rows,
                                    int hist_cap, const int64_t* __restrict__ forced, float* __restrict__ token_logprob,
                                    const float* __restrict__ lse, int64_t* __restrict__ ids) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int h = n_hist_rows[b];
    if (h < 0 || h >= hist_cap) return;
    int64_t id = ids[b];
    if (forced) {
        const int64_t f = forced[(int64_t)h * B + b];
        if (f >= 0 && f < V) { id = f; ids[b] = f; }   // (an id outside the vocabulary is checked by the caller; it never indexes the row)
    }
    token_logprob[(int64_t)h * B + b] = (id >= 0 && id < V) ? logits[(int64_t)b * ld + id] - lse[b] : -INFINITY;
}

static int logprob_args_check(const vcla_logprob_args* a, const char* who) {
    VCLA_REQUIRE(a && a->token_logprob, VCLA_ERR_BAD_ARG, "%s: null pointer in the logprob arguments", who);
    VCLA_REQUIRE(a->k >= 0 && a->k <= VCLA_LOGPROB_MAX_K, VCLA_ERR_BAD_ARG, "%s: k=%d outside [0, %d]", who, a->k, VCLA_LOGPROB_MAX_K);
    VCLA_REQUIRE(a->k == 0 || (a->top_ids && a->top_logprobs), VCLA_ERR_BAD_ARG, "%s: k=%d needs top_ids and top_logprobs", who, a->k);
    return VCLA_OK;
}

extern "C" size_t vcla_logprob_scratch_bytes(int B, int V, int with_copy) {
    if (B < 1 || V < 1) return 0;
    const size_t lse = ((size_t)B * sizeof(float) + 255) / 256 * 256;
    return 256 + lse + (with_copy ? (size_t)B * (size_t)V * sizeof(float) : 0);
}

extern "C" int vcla_logprob_rows(const float* logits, int64_t ld, int B, int V, const int32_t* n_hist_rows, int hist_cap,
                                 const vcla_logprob_args* args, float* lse, float* copy, int64_t copy_ld, void* stream) {
    int rc = logprob_args_check(args, "logprob_rows");
    if (rc) return rc;
    VCLA_REQUIRE(logits && n_hist_rows && lse, VCLA_ERR_BAD_ARG, "logprob_rows: null pointer");
    VCLA_REQUIRE(B >= 0 && V > 0 && V <= VCLA_SAMPLE_MAX_VOCAB && ld >= V && hist_cap >= 1 && (!copy || copy_ld >= V), VCLA_ERR_BAD_SHAPE,
                 "logprob_rows: B=%d V=%d (the row is held in registers: max %d) ld=%lld hist_cap=%d copy_ld=%lld", B, V, VCLA_SAMPLE_MAX_VOCAB,
                 (long long)ld, hist_cap, (long long)copy_ld);
    if (B == 0) return VCLA_OK;
    logprob_rows_kernel<<<B, LP_THREADS, 0, (hipStream_t)stream>>>(logits, ld, V, B, n_hist_rows, hist_cap, args->k, args->top_ids, args->top_logprobs,
                                                                   lse, copy, copy_ld);
    VCLA_CHECK_LAUNCH("logprob_rows_kernel");
    return VCLA_OK;
}

extern "C" int vcla_logprob_pick(const float* logits, int64_t ld, int B, int V, const int32_t* n_hist_rows, int hist_cap,
                                 const vcla_logprob_args* args, const float* lse, int64_t* ids, void* stream) {
    int rc = logprob_args_check(args, "logprob_pick");
    if (rc) return rc;
    VCLA_REQUIRE(logits && n_hist_rows && lse && ids, VCLA_ERR_BAD_ARG, "logprob_pick: null pointer");
    VCLA_REQUIRE(B >= 0 && V > 0 && ld >= V && hist_cap >= 1, VCLA_ERR_BAD_SHAPE, "logprob_pick: B=%d V=%d ld=%lld hist_cap=%d", B, V, (long long)ld,
                 hist_cap);
    if (B == 0) return VCLA_OK;
    logprob_pick_kernel<<<(B + 63) / 64, 64, 0, (hipStream_t)stream>>>(logits, ld, V, B, n_hist_rows, hist_cap, args->forced, args->token_logprob, lse, ids);
    VCLA_CHECK_LAUNCH("logprob_pick_kernel");
    return VCLA_OK;
}
