// constrain.hip -- per-request token constraints of a slots step, decided on the device.  HF restricts what a request may generate with
// PrefixConstrainedLogitsProcessor (prefix_allowed_tokens_fn, a host callback per step and row) and SuppressTokensLogitsProcessor
// (hf:generation/logits_process.py, reached from models/visualcla/modeling_visualcla.py:382-391).  Almost every such callback is static
// data -- an allow list, a ban list, a trie of candidate answers -- so here it is a token automaton in device memory (built by
// visualcla/constraints.py): nodes {edge0, n_edges, deny}, edges {token, next} sorted by token inside a node, one int32 state per row.
// Two launches around the selector of a step:
//   constrain_rows_kernel (BEFORE the selector, on the fp32 row the selector then reads): one 1024-thread workgroup per row.  The node's
//     token set becomes a bitmask of ceil(V / 32) words in LDS (zero, barrier, one atomicOr per edge, barrier); then every column whose
//     bit says "not kept" is written -inf.  x[j] = keep(j) ? x[j] : -inf needs no read of the row: a kept column is simply not written.
//   constrain_advance_kernel (AFTER the selector): one lane per row, a binary search of the id taken among the node's edges; a hit on an
//     allow node moves the state, a miss (the id 0 of an all -inf row) and a deny node leave it.
// Both skip rows whose history length is negative (as logprobs.hip) and rows whose state is negative (an unconstrained request).
#include "vcla_common.h"

#define CS_THREADS 1024

__global__ __launch_bounds__(CS_THREADS) void constrain_rows_kernel(float* __restrict__ logits, int64_t ld, int V, const int32_t* __restrict__ n_hist_rows,
                                                                    const vcla_cs_node* __restrict__ nodes, const vcla_cs_edge* __restrict__ edges,
                                                                    const int32_t* __restrict__ state, int n_nodes, int n_edges) {
    extern __shared__ unsigned s_bits[];   // ceil(V / 32) words
    const int tid = threadIdx.x, b = blockIdx.x;
    const int s = state[b];
    if (s < 0 || s >= n_nodes || n_hist_rows[b] < 0) return;   // workgroup-uniform, ahead of every barrier
    const vcla_cs_node nd = nodes[s];
    const int words = (V + 31) >> 5;
    for (int w = tid; w < words; w += CS_THREADS) s_bits[w] = 0u;
    __syncthreads();
    // (the table is validated on the host before the upload; an edge outside it or a token outside the row is skipped, never followed)
    const int e0 = nd.edge0 < 0 ? 0 : nd.edge0;
    const int e1 = (nd.n_edges < 0 || e0 > n_edges) ? e0 : (nd.n_edges > n_edges - e0 ? n_edges : e0 + nd.n_edges);
    for (int e = e0 + tid; e < e1; e += CS_THREADS) {
        const int tok = edges[e].token;
        if (tok >= 0 && tok < V) atomicOr(&s_bits[tok >> 5], 1u << (tok & 31));
    }
    __syncthreads();
    const unsigned flip = nd.deny ? 0u : 0xffffffffu;           // drop = the bit on a deny node, its complement on an allow node
    float* x = logits + (int64_t)b * ld;                        // plain 4-byte stores: with ld = V = 49958 only every other row base is 8-byte aligned
    for (int j = tid; j < V; j += CS_THREADS)                   // columns at or behind V are never touched
        if (((s_bits[j >> 5] ^ flip) >> (j & 31)) & 1u) x[j] = -INFINITY;
}

__global__ void constrain_advance_kernel(const int64_t* __restrict__ ids, int B, const int32_t* __restrict__ n_hist_rows, const vcla_cs_node* __restrict__ nodes,
                                         const vcla_cs_edge* __restrict__ edges, int32_t* __restrict__ state, int n_nodes, int n_edges) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int s = state[b];
    if (s < 0 || s >= n_nodes || n_hist_rows[b] < 0) return;
    const vcla_cs_node nd = nodes[s];
    if (nd.deny || nd.edge0 < 0 || nd.n_edges <= 0 || nd.edge0 > n_edges - nd.n_edges) return;
    const int64_t id = ids[b];
    int lo = nd.edge0, hi = nd.edge0 + nd.n_edges;              // the first edge whose token is >= id
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if ((int64_t)edges[mid].token < id) lo = mid + 1; else hi = mid;
    }
    if (lo < nd.edge0 + nd.n_edges && (int64_t)edges[lo].token == id) {
        const int nx = edges[lo].next;
        if (nx >= 0 && nx < n_nodes) state[b] = nx;
    }
}

static int constrain_args_check(const vcla_constrain_args* a, const char* who) {
    VCLA_REQUIRE(a && a->nodes && a->edges && a->state, VCLA_ERR_BAD_ARG, "%s: null pointer in the constraint arguments", who);
    VCLA_REQUIRE(a->n_nodes >= 1 && a->n_nodes <= VCLA_CS_MAX_NODES && a->n_edges >= 1 && a->n_edges <= VCLA_CS_MAX_EDGES, VCLA_ERR_BAD_ARG,
                 "%s: n_nodes=%d (1..%d) n_edges=%d (1..%d)", who, a->n_nodes, VCLA_CS_MAX_NODES, a->n_edges, VCLA_CS_MAX_EDGES);
    return VCLA_OK;
}

extern "C" int vcla_constrain_rows(float* logits, int64_t ld, int B, int V, const int32_t* n_hist_rows, const vcla_constrain_args* args, void* stream) {
    int rc = constrain_args_check(args, "constrain_rows");
    if (rc) return rc;
    VCLA_REQUIRE(logits && n_hist_rows, VCLA_ERR_BAD_ARG, "constrain_rows: null pointer");
    VCLA_REQUIRE(B >= 0 && V > 0 && V <= VCLA_CS_MAX_VOCAB && ld >= V, VCLA_ERR_BAD_SHAPE,
                 "constrain_rows: B=%d V=%d (the bitmask of a row lives in 64 KiB of LDS: max %d) ld=%lld", B, V, VCLA_CS_MAX_VOCAB, (long long)ld);
    if (B == 0) return VCLA_OK;
    const size_t lds = (size_t)((V + 31) / 32) * sizeof(unsigned);
    constrain_rows_kernel<<<B, CS_THREADS, lds, (hipStream_t)stream>>>(logits, ld, V, n_hist_rows, args->nodes, args->edges, args->state, args->n_nodes,
                                                                       args->n_edges);
    VCLA_CHECK_LAUNCH("constrain_rows_kernel");
    return VCLA_OK;
}

extern "C" int vcla_constrain_advance(const int64_t* ids, int B, const int32_t* n_hist_rows, const vcla_constrain_args* args, void* stream) {
    int rc = constrain_args_check(args, "constrain_advance");
    if (rc) return rc;
    VCLA_REQUIRE(ids && n_hist_rows && B >= 0, VCLA_ERR_BAD_ARG, "constrain_advance: null pointer or B=%d", B);
    if (B == 0) return VCLA_OK;
    constrain_advance_kernel<<<(B + 63) / 64, 64, 0, (hipStream_t)stream>>>(ids, B, n_hist_rows, args->nodes, args->edges, args->state, args->n_nodes,
                                                                            args->n_edges);
    VCLA_CHECK_LAUNCH("constrain_advance_kernel");
    return VCLA_OK;
}
