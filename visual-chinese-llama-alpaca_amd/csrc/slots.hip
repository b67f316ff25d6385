// slots.hip -- the bookkeeping launch of one in-flight-batching decode step (the slots analogue of post_select_kernel and
// vcla_lookup_step): every batch row is a SLOT that holds one request of a queue at its own position.  Workgroup b, given the id
// selected for slot b this step:
//   active slot (row_pos[b] >= 0): history[count[b]][b] = id, count[b] += 1, row_pos[b] += 1; an eos id or count[b] >= budget[b]
//   finishes the slot (row_pos[b] = -1: position and activity in one word; hist_len[b] = -1), otherwise hist_len[b] = count[b];
//   cur[b] = id and the id's embedding becomes row b of the next step's decoder input.
//   inactive slot: its state is left alone (its input row is re-embedded from cur[b], so the row stays an ordinary embedding).
// The last workgroup to arrive publishes the number of slots still active.  All state lives in device memory, so one captured step
// serves a whole queue.
// STOPS (vcla_slot_step_stops): slot b also finishes when the tail of its generated ids, this step's included, equals one of the up to
// VCLA_SLOT_MAX_STOPS sequences of its row of the stop table.  The first wave decides it before thread 0's update, one lane per
// (sequence, offset); the STOPS = false instantiation is the kernel without any of it.
#include "vcla_common.h"

static_assert(VCLA_SLOT_MAX_STOPS * VCLA_SLOT_MAX_STOP_LEN == 64 && VCLA_SLOT_MAX_STOP_LEN == 16, "one lane of a wave per (sequence, offset)");

template <typename T, bool STOPS>
__global__ __launch_bounds__(256) void slot_step_kernel(const int64_t* __restrict__ ids, vcla_slot_args a, const int32_t* __restrict__ eos_rows,
                                                        const int32_t* __restrict__ stops, const bf16_t* __restrict__ table, T* __restrict__ x,
                                                        int D, int V) {
    __shared__ int64_t s_id;
    const int b = blockIdx.x;
    bool stop_hit = false;   // wave-uniform in the first wave, which holds thread 0
    if constexpr (STOPS) {
        if (threadIdx.x < 64 && a.row_pos[b] >= 0) {   // both conditions are wave-uniform: all 64 lanes take part in the ballots
            const int lane = threadIdx.x, s = lane >> 4, j = lane & 15;
            const int e = stops[(int64_t)b * 64 + lane];   // seqs[b][s][j]: left-aligned, -1 padded
            const int len = __popcll((__ballot(e >= 0) >> (s * 16)) & 0xffffull);
            // lane j < len: is token c - j (c: this step's, earlier ones from the history) the sequence's entry len - 1 - j ?
            const int want = __shfl(e, (s << 4) + (j < len ? len - 1 - j : 0), 64);
            const int c = a.count[b];
            bool ok = true;
            if (j < len) {
                const int t = c - j;
                ok = j == 0 ? ids[b] == (int64_t)want : (t >= 0 && t < a.hist_cap && a.history[(int64_t)t * a.B + b] == (int64_t)want);
            }
            const unsigned long long agree = __ballot(ok);
            stop_hit = len >= 1 && ((agree >> (s * 16)) & 0xffffull) == 0xffffull;
            stop_hit = __ballot(stop_hit) != 0ull;
        }
    }
    if (threadIdx.x == 0) {
        const int pos = a.row_pos[b];
        int64_t id = a.cur[b];
        int active = 0;
        if (pos >= 0) {
            id = ids[b];
            const int c = a.count[b];
            if (c < a.hist_cap) a.history[(int64_t)c * a.B + b] = id;
            bool fin = c + 1 >= a.budget[b];
            if (eos_rows) {   // vcla_slot_step_rows: the slot's own list, -1 padded
                for (int i = 0; i < VCLA_SLOT_MAX_EOS; ++i) {
                    const int e = eos_rows[(int64_t)b * VCLA_SLOT_MAX_EOS + i];
                    fin = fin || (e >= 0 && id == (int64_t)e);
                }
            } else {
                for (int i = 0; i < a.n_eos; ++i) fin = fin || id == (int64_t)a.eos_ids[i];
            }
            if constexpr (STOPS) fin = fin || stop_hit;
            a.count[b] = c + 1;
            a.row_pos[b] = fin ? -1 : pos + 1;
            if (a.hist_len) a.hist_len[b] = fin ? -1 : c + 1;
            a.cur[b] = id;
            active = fin ? 0 : 1;
        }
        s_id = id;
        // ONE returning atomic carries both the arrival (low half) and this slot's activity (high half): the last workgroup to arrive
        // holds the whole sum, publishes it and re-arms the word (B <= 32767, checked by the launcher)
        const int old = atomicAdd(&a.summary[1], 1 + (active << 16));
        if ((old & 0xffff) == a.B - 1) {
            a.summary[0] = (old >> 16) + active;
            a.summary[1] = 0;
        }
    }
    __syncthreads();
    int64_t id = s_id;
    if (id < 0 || id >= V) id = 0;          // as embed_splice_kernel: stay in bounds
    const bf16_t* src = table + id * D;
    T* o = x + (int64_t)b * D;
    if constexpr (sizeof(T) == 2) {
        for (int c = threadIdx.x * 8; c < D; c += 256 * 8) *reinterpret_cast<uint4*>(o + c) = *reinterpret_cast<const uint4*>(src + c);   // D % 8 == 0 (checked by the launcher)
    } else {
        for (int c = threadIdx.x; c < D; c += 256) Act<T>::st(o + c, bf2f(src[c]));
    }
}

int slot_args_check(const vcla_slot_args* a, const char* who) {
    VCLA_REQUIRE(a && a->row_pos && a->count && a->budget && a->history && a->cur && a->summary, VCLA_ERR_BAD_ARG, "%s: null pointer in the slot state", who);
    VCLA_REQUIRE(a->B >= 1 && a->B <= 32767 && a->hist_cap >= 1 && a->n_eos >= 0 && a->n_eos <= VCLA_SLOT_MAX_EOS, VCLA_ERR_BAD_ARG,
                 "%s: slots B=%d (1..32767) hist_cap=%d n_eos=%d (max %d)", who, a->B, a->hist_cap, a->n_eos, VCLA_SLOT_MAX_EOS);
    return VCLA_OK;
}

extern "C" int vcla_slot_step_stops(const int64_t* ids, const vcla_slot_args* args, const int32_t* eos_rows, const vcla_stop_args* stops,
                                    const void* embed_table, void* x, int D, int V, int dtype, void* stream) {
    int rc = slot_args_check(args, "slot_step");
    if (rc) return rc;
    VCLA_REQUIRE(ids && embed_table && x && D > 0 && V > 0, VCLA_ERR_BAD_ARG, "slot_step: null pointer, or D=%d V=%d", D, V);
    VCLA_REQUIRE(dtype == VCLA_F32 || dtype == VCLA_BF16, VCLA_ERR_BAD_DTYPE, "slot_step: bad dtype %d", dtype);
    VCLA_REQUIRE(dtype == VCLA_F32 || (D % 8 == 0 && vcla_aligned(x, 16) && vcla_aligned(embed_table, 16)), VCLA_ERR_BAD_SHAPE,
                 "slot_step: bf16 rows need D %% 8 == 0 (got %d) and 16-byte aligned buffers", D);
    VCLA_REQUIRE(!stops || stops->seqs, VCLA_ERR_BAD_ARG, "slot_step_stops: a null stop table");
    hipStream_t s = (hipStream_t)stream;
    const bf16_t* tb = (const bf16_t*)embed_table;
    if (stops) {
        if (dtype == VCLA_BF16) slot_step_kernel<bf16_t, true><<<args->B, 256, 0, s>>>(ids, *args, eos_rows, stops->seqs, tb, (bf16_t*)x, D, V);
        else slot_step_kernel<float, true><<<args->B, 256, 0, s>>>(ids, *args, eos_rows, stops->seqs, tb, (float*)x, D, V);
    } else {
        if (dtype == VCLA_BF16) slot_step_kernel<bf16_t, false><<<args->B, 256, 0, s>>>(ids, *args, eos_rows, nullptr, tb, (bf16_t*)x, D, V);
        else slot_step_kernel<float, false><<<args->B, 256, 0, s>>>(ids, *args, eos_rows, nullptr, tb, (float*)x, D, V);
    }
    VCLA_CHECK_LAUNCH("slot_step_kernel");
    return VCLA_OK;
}

extern "C" int vcla_slot_step_rows(const int64_t* ids, const vcla_slot_args* args, const int32_t* eos_rows, const void* embed_table, void* x, int D,
                                   int V, int dtype, void* stream) {
    return vcla_slot_step_stops(ids, args, eos_rows, nullptr, embed_table, x, D, V, dtype, stream);
}

extern "C" int vcla_slot_step(const int64_t* ids, const vcla_slot_args* args, const void* embed_table, void* x, int D, int V, int dtype, void* stream) {
    return vcla_slot_step_rows(ids, args, nullptr, embed_table, x, D, V, dtype, stream);
}
