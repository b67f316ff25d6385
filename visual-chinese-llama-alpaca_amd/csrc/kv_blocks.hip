// kv_blocks.hip -- the copies of generate_many's persistent prefix cache (visualcla/prefix_cache.py): a table of
// BLOCKS of 16 consecutive K/V rows moved between a slots cache [L][2][B_slots][H][ctx_max][d] and the pool [n_blocks][L][2][H][16][d],
// one launch per direction.
//
// For one table entry {block, slot, row0} and one (layer, k|v, head) the 16 rows are 16 * d * esz CONTIGUOUS bytes on both sides (a
// PIECE: 4 KiB at the 7B shape in bf16), and in the pool the L * 2 * H pieces of a block lie back to back: a block is ONE contiguous run
// of 16-byte units there, and unit u of it belongs to piece u / (d * esz) of the slots cache.  So the kernel is a streaming copy over
// units with a division on the slots side only; every lane moves 16 bytes per access, a wave 1 KiB per instruction.
//
// Grid: a workgroup of 256 lanes moves KVB_UNITS_PER_WG = 2048 consecutive units (32 KiB) of one entry -- all 8 loads of a lane are
// issued before its first store, which is the ~32 KiB of loads a CU wants in flight to stream from HBM.  One workgroup per piece
// (4 KiB, one access per lane) leaves every CU latency-bound; one workgroup per entry (8 MiB at the 7B shape) leaves 255 of 256 CUs
// idle for a table of one entry.  At the 7B shape an entry is 256 workgroups: one per CU for a single block, and the hardware
// dispatcher balances longer tables.  grid = (ceil(units per block / 2048), n_entries).
//
// The table lives in device memory and cannot be range-checked by the launcher: the caller validates it before the upload
// (_lib.kv_block_table), and the kernel SKIPS an entry that would leave either buffer, so a bad record cannot write out of bounds.
#include "vcla_common.h"

#define KVB_THREADS 256
#define KVB_PER_LANE 8
#define KVB_UNITS_PER_WG (KVB_THREADS * KVB_PER_LANE)

template <bool TO_POOL, bool FULL>
__device__ __forceinline__ void kvb_move(u32x4_t* __restrict__ slots, u32x4_t* __restrict__ pb, uint32_t u0, uint32_t units, uint32_t upp, int upr,
                                         const vcla_kv_block& e, int B_slots, int H, int ctx_max) {
    u32x4_t v[KVB_PER_LANE];
    int64_t so[KVB_PER_LANE];
#pragma unroll
    for (int j = 0; j < KVB_PER_LANE; ++j) {
        const uint32_t u = u0 + j * KVB_THREADS;
        so[j] = -1;
        if (FULL || u < units) {
            const uint32_t piece = u / upp;                 // (layer * 2 + k|v) * H + head
            const uint32_t off = u - piece * upp;
            const uint32_t lk = piece / (uint32_t)H;
            const uint32_t h = piece - lk * H;
            so[j] = ((((int64_t)lk * B_slots + e.slot) * H + h) * ctx_max + e.row0) * upr + off;
            v[j] = TO_POOL ? slots[so[j]] : pb[u];
        }
    }
#pragma unroll
    for (int j = 0; j < KVB_PER_LANE; ++j) {
        if (FULL || so[j] >= 0) {
            if (TO_POOL) pb[u0 + j * KVB_THREADS] = v[j];
            else slots[so[j]] = v[j];
        }
    }
}

template <bool TO_POOL>
__global__ __launch_bounds__(KVB_THREADS, 4) void kv_blocks_copy_kernel(u32x4_t* __restrict__ slots, u32x4_t* __restrict__ pool,
                                                                      const vcla_kv_block* __restrict__ table, int LK, int B_slots, int H,
                                                                      int ctx_max, int n_blocks, int upr /* 16-byte units per row: d * esz / 16 */) {
    const vcla_kv_block e = table[blockIdx.y];
    if (e.block < 0 || e.block >= n_blocks || e.slot < 0 || e.slot >= B_slots || e.row0 < 0 || (e.row0 % VCLA_KV_BLOCK_ROWS) != 0 ||
        e.row0 > ctx_max - VCLA_KV_BLOCK_ROWS)
        return;                                             // (uniform over the workgroup)
    const uint32_t upp = (uint32_t)upr * VCLA_KV_BLOCK_ROWS;        // units per piece
    const uint32_t units = (uint32_t)LK * H * upp;                  // units per block (< 2^31, checked by the launcher: 32-bit divisions)
    u32x4_t* const pb = pool + (int64_t)e.block * units;
    const uint32_t u0 = blockIdx.x * KVB_UNITS_PER_WG + threadIdx.x;
    // every workgroup but the last of a block is full: no lane of it tests its units, so the stores wait for their own load only
    if (blockIdx.x * KVB_UNITS_PER_WG + KVB_UNITS_PER_WG <= units) kvb_move<TO_POOL, true>(slots, pb, u0, units, upp, upr, e, B_slots, H, ctx_max);
    else kvb_move<TO_POOL, false>(slots, pb, u0, units, upp, upr, e, B_slots, H, ctx_max);
}

extern "C" int vcla_kv_blocks_copy(void* kv_slots, void* pool, const vcla_kv_block* table, int n_entries, int L, int B_slots, int H, int ctx_max,
                                   int d, int n_blocks, int dtype, int to_pool, void* stream) {
    VCLA_REQUIRE(dtype == VCLA_F32 || dtype == VCLA_BF16, VCLA_ERR_BAD_DTYPE, "kv_blocks_copy: bad dtype %d", dtype);
    VCLA_REQUIRE(n_entries >= 0 && n_entries <= 65535, VCLA_ERR_BAD_SHAPE, "kv_blocks_copy: n_entries=%d (0..65535)", n_entries);
    if (n_entries == 0) return VCLA_OK;
    VCLA_REQUIRE(kv_slots && pool && table, VCLA_ERR_BAD_ARG, "kv_blocks_copy: null pointer");
    VCLA_REQUIRE(L >= 1 && B_slots >= 1 && H >= 1 && d >= 1 && n_blocks >= 1 && ctx_max >= VCLA_KV_BLOCK_ROWS, VCLA_ERR_BAD_SHAPE,
                 "kv_blocks_copy: L=%d B_slots=%d H=%d d=%d n_blocks=%d ctx_max=%d (at least %d rows)", L, B_slots, H, d, n_blocks, ctx_max,
                 VCLA_KV_BLOCK_ROWS);
    const size_t row_bytes = (size_t)d * vcla_dtype_size(dtype);
    // a block starts at row0 * row_bytes behind the start of its (layer, k|v, slot, head) slab: every slab and every row must be 16-byte aligned
    VCLA_REQUIRE(row_bytes % 16 == 0 && vcla_aligned(kv_slots, 16) && vcla_aligned(pool, 16), VCLA_ERR_BAD_SHAPE,
                 "kv_blocks_copy: rows of %zu bytes (head dim %d) and both buffers must be 16-byte aligned", row_bytes, d);
    const int upr = (int)(row_bytes / 16);
    const int64_t units = (int64_t)L * 2 * H * upr * VCLA_KV_BLOCK_ROWS;
    const int64_t gx = (units + KVB_UNITS_PER_WG - 1) / KVB_UNITS_PER_WG;
    VCLA_REQUIRE(units <= 0x7fffffff, VCLA_ERR_BAD_SHAPE, "kv_blocks_copy: a block of %lld bytes is too large", (long long)units * 16);
    const dim3 grid((unsigned)gx, (unsigned)n_entries);
    hipStream_t s = (hipStream_t)stream;
    if (to_pool) kv_blocks_copy_kernel<true><<<grid, KVB_THREADS, 0, s>>>((u32x4_t*)kv_slots, (u32x4_t*)pool, table, L * 2, B_slots, H, ctx_max, n_blocks, upr);
    else kv_blocks_copy_kernel<false><<<grid, KVB_THREADS, 0, s>>>((u32x4_t*)kv_slots, (u32x4_t*)pool, table, L * 2, B_slots, H, ctx_max, n_blocks, upr);
    VCLA_CHECK_LAUNCH("kv_blocks_copy_kernel");
    return VCLA_OK;
}
