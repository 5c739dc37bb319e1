// kvfork.hip -- [EXT] candidate sets (q3tts_spec.h "candidate sets"): k_kv_fork copies the first n_pages logical KV pages of one sequence
// into the pages of n_dst other sequences of the same paged cache, K and V planes, whole pages.  The physical page ids are read from the
// device page table inside the kernel, so the rows KvPool::ensure uploaded asynchronously on the launching stream are the ones used and the
// host never waits.  A plane page is n_layer * n_kv * 8192 halfs = n_layer * n_kv tiles of 1024 16-byte pieces; one workgroup iteration
// moves one tile: each lane issues its four 16-byte loads (lanes of a wave cover 1 KiB per load), then stores the four pieces to every
// destination -- a piece is read once however many destinations there are.  blockIdx.y = (logical page, plane); blockIdx.x strides over the
// tiles.  Only 16-byte vector loads and stores; no LDS, no atomics, no scratch: the per-destination page id is a uniform (scalar) load.
#include "kernels.h"
#include <algorithm>

namespace q3 {

#define KVF_THREADS 256
#define KVF_UNROLL 4
#define KVF_TILE (KVF_THREADS * KVF_UNROLL) // 16-byte pieces per tile = 8192 halfs: one (layer, kv head) of a plane page

__global__ void __launch_bounds__(KVF_THREADS) k_kv_fork(KvCache kv, int src_seq, const int32_t* __restrict__ dst_seqs, int n_dst) {
    const int logical = (int)blockIdx.y >> 1;
    const uint16_t* plane_c = (blockIdx.y & 1) ? kv.v : kv.k; // plain selects of argument fields
    uint16_t* plane = (blockIdx.y & 1) ? kv.v : kv.k;
    const size_t page_u4 = kv.page_stride() / 8; // 16-byte pieces per plane page
    const int n_tiles = kv.n_layer * kv.n_kv;
    // column `logical` of the page table, read through the constant address space: nothing writes the table while the kernel runs, and the
    // uniform lookups become scalar loads that do not wait for the vector stores in flight
    typedef const __attribute__((address_space(4))) int32_t* ConstI32;
    ConstI32 pt = (ConstI32)(kv.page_table + logical);
    ConstI32 dsts = (ConstI32)dst_seqs;
    const uint4* src = (const uint4*)plane_c + (size_t)pt[(size_t)src_seq * kv.max_pages] * page_u4;
    uint4* base = (uint4*)plane;
    for (int tile = (int)blockIdx.x; tile < n_tiles; tile += (int)gridDim.x) {
        const size_t at = (size_t)tile * KVF_TILE + threadIdx.x;
        const uint4 r0 = src[at], r1 = src[at + KVF_THREADS], r2 = src[at + 2 * KVF_THREADS], r3 = src[at + 3 * KVF_THREADS];
        for (int d = 0; d < n_dst; d++) {
            uint4* dst = base + (size_t)pt[(size_t)dsts[d] * kv.max_pages] * page_u4 + at;
            dst[0] = r0; dst[KVF_THREADS] = r1; dst[2 * KVF_THREADS] = r2; dst[3 * KVF_THREADS] = r3;
        }
    }
}

// Grid: 2 * n_pages rows of at most n_layer * n_kv workgroups, about 2048 workgroups in all (8 per CU); the rest of a row's tiles are strided.
// The talker's page (28 layers x 8 kv heads = 224 tiles a plane page) at 5 pages: 10 x 204; the tiny model's (2 x 2): 4 a row.
void launch_kv_fork(hipStream_t st, const KvCache& kv, int src_seq, const int32_t* dst_seqs, int n_dst, int n_pages) {
    if (n_dst <= 0 || n_pages <= 0) return;
    const int n_tiles = kv.n_layer * kv.n_kv, rows = 2 * n_pages;
    const int gx = std::max(1, std::min(n_tiles, 2048 / rows));
    k_kv_fork<<<dim3((unsigned)gx, (unsigned)rows), KVF_THREADS, 0, st>>>(kv, src_seq, dst_seqs, n_dst);
}

} // namespace q3
