// vcla_knobs.h -- the run-time VCLA_* switches of libvisualcla_hip.so, read in ONE place.
//
// Rule: an outermost ABI call (vcla_vision_forward, vcla_llama_prefill, vcla_llama_decode_*, vcla_gemm, vcla_attention, ...) opens a
// VCLA_KNOBS_SCOPE, which reads the environment once into a thread-local snapshot; everything below it -- including the calls engine.hip
// makes into vcla_gemm / vcla_attention -- sees that snapshot unchanged.  A switch flipped between two calls therefore takes effect on the
// next call, and the cached graphs hold the snapshot in their keys, so a graph captured under other switch values is never replayed.
// Every switch but VCLA_MACRO_GRAPH_DEBUG and the VCLA_ENGINE_* test / debug hooks only selects among forms that compute the same function.
#pragma once
#include <stdlib.h>
#include <string.h>
#include <type_traits>

struct vcla_knobs {
    unsigned long long engine_tl;   // VCLA_ENGINE_TL (hex device address, 0): debug, per-workgroup stamps of the decode engine (tools/engine_probe.py --timeline)
    int engine;                     // VCLA_ENGINE (1): 0 = the per-operator launches instead of the persistent B = 1 decode step
    int engine_split;               // VCLA_ENGINE_SPLIT (512): context length from which the engine splits a head's cache walk over its CU group; 0 = never
    int engine_tail;                // VCLA_ENGINE_TAIL (1): 0 = argmax / token record / next embedding as separate launches behind the engine step
    int engine_fault;               // VCLA_ENGINE_FAULT (0): test hook, see decode_engine.h
    int ring;                       // VCLA_RING (1): 0 = the round-4 dispatch (128 x 128 tiles + K slices) for 129 - 256 rows and the fp8 decode rows
    int ring_vit;                   // VCLA_RING_VIT (1): 0 = no ring tiles for one image through the ViT / the resampler's latent rows
    int ring_wf;                    // VCLA_RING_WF (1): 0 = the ring kernel reads row-major bf16 weight pieces even when a fragment-major twin exists
    int ring_c3;                    // VCLA_RING_C3 (1): 0 = 4 double-slab stages instead of 9 single-slab ones for the 64 x 64 bf16 ring tile
    int dstream;                    // VCLA_DSTREAM (1): 0 = split-K panel kernels instead of the streaming decode GEMMs (2 <= B <= 64)
    int ds_defer;                   // VCLA_DS_DEFER (1): 0 = a vcla_rmsnorm_pack launch per norm instead of the deferred RMSNorm
    int ds_qkv_split;               // VCLA_DS_QKV_SPLIT (1): 0 = qkv unsplit instead of two raw K slices summed by the decode attention
    int gemv1x;                     // VCLA_GEMV1X (1): 0 = the runtime-K decode GEMV instead of the compile-time-K one (gemv_decode.hip)
    int gemm_pf;                    // VCLA_GEMM_PF (1): 0 = the 256 x 256 GEMM without the L2 prefetch (and without 257-row tiles)
    int gemm_xr;                    // VCLA_GEMM_XR (1): 0 = 256-row tiles + a tail launch also when M = B * 257
    int mfma128_splitk;             // VCLA_MFMA128_SPLITK (1): 0 = no K slices for the 128 x 128 tile kernel
    int attn_mfma_whole;            // VCLA_ATTN_MFMA_WHOLE (1): 0 = the causal d = 128 prefill attention always tile by tile
    int attn_vit;                   // VCLA_ATTN_VIT (2): ViT self-attention, 0 = tile-by-tile kernel, 1 = register-staged, 2 = direct-to-LDS (257 tokens)
    int macro_graph;                // VCLA_MACRO_GRAPH (1): 0 = the vision stack and the prefill always eager (no cached graphs)
    int macro_graph_debug;          // VCLA_MACRO_GRAPH_DEBUG (0): 1 = log every capture / replay decision of the cached graphs to stderr
    int unused;                     // 0: fills the struct to a multiple of 8 bytes
};
// no padding bytes: the graph keys compare snapshots with memcmp
static_assert(std::has_unique_object_representations_v<vcla_knobs>, "vcla_knobs must have no padding bytes");

// the only place of the library that reads the environment
inline vcla_knobs vcla_read_knobs() {
    auto env = [](const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; };
    vcla_knobs k;
    memset(&k, 0, sizeof k);
    const char* tl = getenv("VCLA_ENGINE_TL");
    k.engine_tl = tl ? strtoull(tl, nullptr, 16) : 0;
    k.engine = env("VCLA_ENGINE", 1);
    k.engine_split = env("VCLA_ENGINE_SPLIT", 512);
    k.engine_tail = env("VCLA_ENGINE_TAIL", 1);
    k.engine_fault = env("VCLA_ENGINE_FAULT", 0);
    k.ring = env("VCLA_RING", 1);
    k.ring_vit = env("VCLA_RING_VIT", 1);
    k.ring_wf = env("VCLA_RING_WF", 1);
    k.ring_c3 = env("VCLA_RING_C3", 1);
    k.dstream = env("VCLA_DSTREAM", 1);
    k.ds_defer = env("VCLA_DS_DEFER", 1);
    k.ds_qkv_split = env("VCLA_DS_QKV_SPLIT", 1);
    k.gemv1x = env("VCLA_GEMV1X", 1);
    k.gemm_pf = env("VCLA_GEMM_PF", 1);
    k.gemm_xr = env("VCLA_GEMM_XR", 1);
    k.mfma128_splitk = env("VCLA_MFMA128_SPLITK", 1);
    k.attn_mfma_whole = env("VCLA_ATTN_MFMA_WHOLE", 1);
    k.attn_vit = env("VCLA_ATTN_VIT", 2);
    k.macro_graph = env("VCLA_MACRO_GRAPH", 1);
    k.macro_graph_debug = env("VCLA_MACRO_GRAPH_DEBUG", 0);
    return k;
}

struct vcla_knobs_tls {
    vcla_knobs k;
    int depth;     // open scopes on this thread
};
inline thread_local vcla_knobs_tls vcla_knobs_state = {};

// RAII guard of an ABI entry point: the outermost one on the thread takes the snapshot, nested ones reuse it
struct vcla_knobs_scope {
    vcla_knobs_scope() { if (vcla_knobs_state.depth++ == 0) vcla_knobs_state.k = vcla_read_knobs(); }
    ~vcla_knobs_scope() { --vcla_knobs_state.depth; }
    vcla_knobs_scope(const vcla_knobs_scope&) = delete;
    vcla_knobs_scope& operator=(const vcla_knobs_scope&) = delete;
};
#define VCLA_KNOBS_SCOPE() vcla_knobs_scope vcla_knobs_scope_ {}

// the snapshot of the running outermost call (reached outside any scope: the environment as it is now)
inline const vcla_knobs& vcla_knobs_get() {
    if (vcla_knobs_state.depth == 0) vcla_knobs_state.k = vcla_read_knobs();
    return vcla_knobs_state.k;
}
