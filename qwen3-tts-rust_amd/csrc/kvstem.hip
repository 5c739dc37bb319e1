// kvstem.hip -- [EXT] prompt stems (q3tts_spec.h "prompt stems"): k_kv_stem copies whole KV pages between stem stores and the paged cache.
// A store is one stem's own allocation: n_pages contiguous plane pages of K, then as many of V, in the pool's page layout.  One launch serves
// a table of jobs {store K / V base, n_pages, first destination, n destinations}:
//   restore (save = 0)  logical page l of the job's store goes into logical page l of every slot in slots[first .. first + n_dst): a store
//                       page is read once in the launch however many slots take it
//   save    (save = 1)  logical page l of slot slots[first] goes into page l of the store (n_dst is 1)
// The access pattern is k_kv_fork's: a plane page is n_layer * n_kv tiles of 1024 16-byte pieces; one workgroup iteration moves one tile: each
// lane issues its four 16-byte loads, then the stores.  The physical page ids are read from the device page table inside the kernel, so the
// rows KvPool::ensure uploaded asynchronously on the launching stream are the ones used and the host never waits.  blockIdx.z = job,
// blockIdx.y = (logical page, plane) -- rows past a job's own page count leave at once -- blockIdx.x strides over the tiles.  Only 16-byte
// vector loads and stores; no LDS, no atomics, no scratch: the job's fields and the per-destination page ids are uniform (scalar) loads.
#include "kernels.h"
#include <algorithm>

namespace q3 {

#define KVS_THREADS 256
#define KVS_UNROLL 4
#define KVS_TILE (KVS_THREADS * KVS_UNROLL) // 16-byte pieces per tile = 8192 halfs: one (layer, kv head) of a plane page

__global__ void __launch_bounds__(KVS_THREADS) k_kv_stem(KvCache kv, const StemJob* __restrict__ jobs, const int32_t* __restrict__ slots, int save) {
    // the job table, the slot list and the page table are read through the constant address space: nothing writes them while the kernel
    // runs, and the uniform lookups become scalar loads that do not wait for the vector stores in flight
    typedef const __attribute__((address_space(4))) StemJob* ConstJob;
    typedef const __attribute__((address_space(4))) int32_t* ConstI32;
    ConstJob job = (ConstJob)jobs + blockIdx.z;
    const int logical = (int)blockIdx.y >> 1;
    if (logical >= job->n_pages) return;
    const bool vplane = (blockIdx.y & 1) != 0;
    uint4* pool = (uint4*)(vplane ? kv.v : kv.k);
    uint4* store = (uint4*)(vplane ? job->v : job->k);
    const size_t page_u4 = kv.page_stride() / 8; // 16-byte pieces per plane page
    const int n_tiles = kv.n_layer * kv.n_kv;
    ConstI32 pt = (ConstI32)(kv.page_table + logical);
    ConstI32 dsts = (ConstI32)slots + job->first;
    const int n_dst = job->n_dst;
    uint4* spage = store + (size_t)logical * page_u4;
    if (save) {
        const uint4* src = pool + (size_t)pt[(size_t)dsts[0] * kv.max_pages] * page_u4;
        for (int tile = (int)blockIdx.x; tile < n_tiles; tile += (int)gridDim.x) {
            const size_t at = (size_t)tile * KVS_TILE + threadIdx.x;
            const uint4 r0 = src[at], r1 = src[at + KVS_THREADS], r2 = src[at + 2 * KVS_THREADS], r3 = src[at + 3 * KVS_THREADS];
            uint4* dst = spage + at;
            dst[0] = r0; dst[KVS_THREADS] = r1; dst[2 * KVS_THREADS] = r2; dst[3 * KVS_THREADS] = r3;
        }
        return;
    }
    for (int tile = (int)blockIdx.x; tile < n_tiles; tile += (int)gridDim.x) {
        const size_t at = (size_t)tile * KVS_TILE + threadIdx.x;
        const uint4* src = spage + at;
        const uint4 r0 = src[0], r1 = src[KVS_THREADS], r2 = src[2 * KVS_THREADS], r3 = src[3 * KVS_THREADS];
        for (int d = 0; d < n_dst; d++) {
            uint4* dst = pool + (size_t)pt[(size_t)dsts[d] * kv.max_pages] * page_u4 + at;
            dst[0] = r0; dst[KVS_THREADS] = r1; dst[2 * KVS_THREADS] = r2; dst[3 * KVS_THREADS] = r3;
        }
    }
}

// Grid: n_jobs layers of 2 * max_pages rows (max_pages: the largest page count among the jobs) of at most n_layer * n_kv workgroups, about
// 2048 workgroups in all, as launch_kv_fork; the rest of a row's tiles are strided.
void launch_kv_stem(hipStream_t st, const KvCache& kv, const StemJob* jobs, int n_jobs, int max_pages, const int32_t* slots, bool save) {
    if (n_jobs <= 0 || max_pages <= 0) return;
    const int n_tiles = kv.n_layer * kv.n_kv, rows = 2 * max_pages;
    const int gx = std::max(1, std::min(n_tiles, 2048 / (rows * n_jobs)));
    k_kv_stem<<<dim3((unsigned)gx, (unsigned)rows, (unsigned)n_jobs), KVS_THREADS, 0, st>>>(kv, jobs, slots, save ? 1 : 0);
}

} // namespace q3
