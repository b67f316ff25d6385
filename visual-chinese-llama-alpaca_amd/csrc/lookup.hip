// lookup.hip -- the bookkeeping launch of one prompt-lookup verify iteration (hf generation/utils.py _assisted_decoding, greedy branch, with
// transformers/generation/candidate_generator.py PromptLookupCandidateGenerator.get_candidates as the draft source), one workgroup:
//   1. acceptance: n = number of leading drafts row[1 + i] equal to the argmax of the row before them (HF's n_matches);
//   2. emit argmax[0 .. n], cut at the first eos and at the token budget, into out[] and the history; *pos_dev advances by the number emitted;
//   3. done flag once the budget is used up or an eos was emitted: later replays change nothing (no output, no position advance);
//   4. the next input row: the last emitted token, then k drafts from the history (padded with the filler id).
// Everything lives in device memory, so the launch replays from the same hipGraph as the verify pass in front of it.
#include "vcla_common.h"

__device__ __forceinline__ bool lk_is_eos(const vcla_lookup_args& a, int64_t t) {
    for (int i = 0; i < a.n_eos; ++i)
        if (t == (int64_t)a.eos_ids[i]) return true;
    return false;
}

__global__ __launch_bounds__(256) void lookup_step_kernel(const int64_t* __restrict__ am, vcla_lookup_args a, int32_t* __restrict__ pos_dev) {
    __shared__ int s_done, s_best;
    int32_t* st = a.state;
    const int tid = threadIdx.x;
    if (tid == 0) {
        int done = st[VCLA_LOOKUP_DONE];
        if (am && !done) {
            int n = 0;
            while (n < a.k && a.row[n + 1] == am[n]) ++n;
            int cnt = st[VCLA_LOOKUP_COUNT], nh = st[VCLA_LOOKUP_NHIST], e = 0;
            for (int i = 0; i <= n; ++i) {
                if (cnt >= a.budget) { done = 1; break; }
                const int64_t t = am[i];
                a.out[cnt++] = t;
                if (nh < a.hist_cap) a.history[nh++] = t;
                ++e;
                if (lk_is_eos(a, t)) { done = 1; break; }
            }
            if (cnt >= a.budget) done = 1;
            st[VCLA_LOOKUP_NHIST] = nh;
            st[VCLA_LOOKUP_COUNT] = cnt;
            st[VCLA_LOOKUP_DONE] = done;
            st[VCLA_LOOKUP_ITERS] += 1;
            st[VCLA_LOOKUP_ACCEPTED] += e > 0 ? e - 1 : 0;
            *pos_dev += e;
        }
        s_done = am ? done : 0;
        s_best = 0x7fffffff;
    }
    __syncthreads();
    if (s_done) return;
    // ---- drafts: the longest tail n-gram (max_matching_ngram_size .. 1) with an EARLIER occurrence whose continuation is non-empty; the
    // earliest such occurrence; up to k continuation tokens, cut before the first eos.  A match whose cut leaves nothing proposes nothing.
    const int L = st[VCLA_LOOKUP_NHIST];
    const int64_t* hs = a.history;
    const int64_t last = L > 0 ? hs[L - 1] : 0;
    int n_found = 0;
    for (int n = min(a.ngram_max, L - 1); n >= 1; --n) {
        for (int idx = tid; idx < L - n; idx += 256) {
            bool eq = true;
            for (int t = 0; t < n && eq; ++t) eq = hs[idx + t] == hs[L - n + t];
            if (eq) atomicMin(&s_best, idx);
        }
        __syncthreads();
        if (s_best != 0x7fffffff) { n_found = n; break; }
        __syncthreads();
    }
    if (tid == 0) {
        int nd = 0;
        if (n_found) {
            const int start = s_best + n_found, end = min(start + a.k, L);
            for (int j = start; j < end && !lk_is_eos(a, hs[j]); ++j) a.row[1 + nd++] = hs[j];
        }
        a.row[0] = last;
        const int64_t fill = a.filler >= 0 ? a.filler : last;
        for (int i = nd; i < a.k; ++i) a.row[1 + i] = fill;
        st[VCLA_LOOKUP_DRAFTS] = nd;
    }
}

extern "C" int vcla_lookup_step(const int64_t* argmax_ids, const vcla_lookup_args* args, int32_t* pos_dev, void* stream) {
    VCLA_REQUIRE(args && args->row && args->history && args->out && args->state && (pos_dev || !argmax_ids), VCLA_ERR_BAD_ARG,
                 "lookup_step: null pointer");
    VCLA_REQUIRE(args->k >= 1 && args->k + 1 <= VCLA_LOOKUP_MAX_ROWS && args->ngram_max >= 1 && args->budget >= 1 && args->hist_cap >= 1 &&
                     args->n_eos >= 0 && args->n_eos <= VCLA_LOOKUP_MAX_EOS, VCLA_ERR_BAD_ARG,
                 "lookup_step: k=%d (1..%d) ngram_max=%d budget=%d hist_cap=%d n_eos=%d", args->k, VCLA_LOOKUP_MAX_ROWS - 1, args->ngram_max,
                 args->budget, args->hist_cap, args->n_eos);
    lookup_step_kernel<<<1, 256, 0, (hipStream_t)stream>>>(argmax_ids, *args, pos_dev);
    VCLA_CHECK_LAUNCH("lookup_step_kernel");
    return VCLA_OK;
}
