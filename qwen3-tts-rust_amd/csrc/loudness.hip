// loudness.hip -- [EXT] loudness (q3tts_spec.h "loudness"): the K-weighted block energies and sample peaks of the native chunk, in front of
// the volume stage, at most one launch per decode pass and only when the pass holds a metered stream.  The chunk is read, never written.
//
// k_loudness: grid = G, 128 lanes, one workgroup per stream; a stream that is not metered exits at once.  Lanes own segments of 96 samples: a
// 4-frame chunk is 80 segments, a longer chunk is walked in batches of 128.  Per batch, the three phases of the spec: every lane runs its
// segment from the zero state and leaves z_k in LDS; lane 0 walks the batch ascending, start_{k+1} = M start_k + z_k, and leaves start_k in
// LDS; every lane runs its segment again from start_k and leaves q_k and p_k in LDS; lane 0 adds them ascending into the running block and
// stores a row {energy, peak} wherever a block ends.  The walk's last state and the running block go back to the stream's store.
//
// All arithmetic is float64 through loud_step / loud_carry (loudness.h), the one definition the host shares; the file is compiled without
// contraction.  LDS arrays are [component][lane], so a phase's stores are contiguous across lanes.  No counters, no atomics, no scratch.
#include "out_stages.h"
#include "kdev.h"
#include "loudness.h"

namespace q3 {

#define LOUD_THREADS 128

struct LoudArgs { const float* pcm; int T; const LoudStreamMeta* meta; double* state; unsigned char* out; LoudTables tab; };

__global__ void __launch_bounds__(LOUD_THREADS) k_loudness(LoudArgs a) {
    __shared__ double zend[4][LOUD_THREADS];    // phase 1: z_k; phase 2 overwrites entry k with start_k
    __shared__ double sq[LOUD_THREADS], sp[LOUD_THREADS];
    __shared__ double carry[Q3_LOUD_STATE];     // the walk's state between batches, the running block
    const int g = blockIdx.x, tid = threadIdx.x;
    const LoudStreamMeta mt = a.meta[g];
    if (mt.slot < 0) return;   // uniform: the stream is not metered
    const float* const x = a.pcm + (size_t)g * a.T;
    double* const st = a.state + (size_t)mt.slot * Q3_LOUD_STATE;
    double* const rows = reinterpret_cast<double*>(a.out + mt.out_off);
    const int nseg = a.T / Q3_LOUD_SEG;
    const int64_t seg0 = mt.pos / Q3_LOUD_SEG;   // the chunk's first segment, counted from the stream's reset
    if (tid < Q3_LOUD_STATE) carry[tid] = st[tid];
    __syncthreads();
    for (int base = 0; base < nseg; base += LOUD_THREADS) {
        const int k = base + tid, nb = min(LOUD_THREADS, nseg - base);
        const float4* const xs = reinterpret_cast<const float4*>(x + (size_t)k * Q3_LOUD_SEG);   // 96 floats = 24 vectors, 16-byte aligned
        if (k < nseg) {   // phase 1
            double s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 2
            for (int i = 0; i < Q3_LOUD_SEG / 4; i++) {
                const float4 c = xs[i];
                (void)loud_step(s, (double)c.x, a.tab.coef); (void)loud_step(s, (double)c.y, a.tab.coef);
                (void)loud_step(s, (double)c.z, a.tab.coef); (void)loud_step(s, (double)c.w, a.tab.coef);
            }
            zend[0][tid] = s[0]; zend[1][tid] = s[1]; zend[2][tid] = s[2]; zend[3][tid] = s[3];
        }
        __syncthreads();
        if (tid == 0) {   // phase 2
            double s[4] = {carry[0], carry[1], carry[2], carry[3]};
#pragma unroll 1
            for (int j = 0; j < nb; j++) {
                const double z[4] = {zend[0][j], zend[1][j], zend[2][j], zend[3][j]};
                zend[0][j] = s[0]; zend[1][j] = s[1]; zend[2][j] = s[2]; zend[3][j] = s[3];
                double n[4];
                loud_carry(a.tab.m, s, z, n);
                s[0] = n[0]; s[1] = n[1]; s[2] = n[2]; s[3] = n[3];
            }
            carry[0] = s[0]; carry[1] = s[1]; carry[2] = s[2]; carry[3] = s[3];
        }
        __syncthreads();
        if (k < nseg) {   // phase 3
            double s[4] = {zend[0][tid], zend[1][tid], zend[2][tid], zend[3][tid]};
            double q = 0.0; float pk = 0.0f;
#pragma unroll 2
            for (int i = 0; i < Q3_LOUD_SEG / 4; i++) {
                const float4 c = xs[i];
                const double w0 = loud_step(s, (double)c.x, a.tab.coef); q = q + w0 * w0;
                const double w1 = loud_step(s, (double)c.y, a.tab.coef); q = q + w1 * w1;
                const double w2 = loud_step(s, (double)c.z, a.tab.coef); q = q + w2 * w2;
                const double w3 = loud_step(s, (double)c.w, a.tab.coef); q = q + w3 * w3;
                pk = fmaxf(pk, fmaxf(fmaxf(fabsf(c.x), fabsf(c.y)), fmaxf(fabsf(c.z), fabsf(c.w))));
            }
            sq[tid] = q; sp[tid] = (double)pk;
        }
        __syncthreads();
        if (tid == 0) {   // the blocks
            double e = carry[4], p = carry[5];
#pragma unroll 1
            for (int j = 0; j < nb; j++) {
                e = e + sq[j]; p = fmax(p, sp[j]);
                const int64_t kk = seg0 + base + j + 1;   // segments of the stream behind this one
                if (kk % LOUD_SEGS_PER_BLOCK == 0) {
                    const int64_t row = kk / LOUD_SEGS_PER_BLOCK - 1 - mt.pos / Q3_LOUD_BLOCK;   // in [0, loud_blocks(pos, T))
                    rows[2 * row] = e; rows[2 * row + 1] = p;
                    e = 0.0; p = 0.0;
                }
            }
            carry[4] = e; carry[5] = p;
        }
        __syncthreads();   // the next batch overwrites zend, sq and sp
    }
    if (tid < Q3_LOUD_STATE) st[tid] = carry[tid];
}

LoudnessStage::LoudnessStage(int n_streams_, int max_group_, StageCounters* count_) : StageBase(n_streams_, max_group_, count_, "loudness stage") {
    LoudTables t;
    loud_tables(&t);
    std::copy(t.coef, t.coef + 10, coef); std::copy(t.m, t.m + 16, m);
    state_own.alloc((size_t)n_streams * Q3_LOUD_STATE); state_own.zero();
    state = state_own.p;
    Q3_HIP(hipStreamSynchronize(nullptr)); // the memset ran on the null stream, which the caller's non-blocking streams do not wait for
    ring.alloc(max_group);
}

void LoudnessStage::reset_async(hipStream_t st, int slot) {
    check_slot(slot);
    Q3_HIP(hipMemsetAsync(state + (size_t)slot * Q3_LOUD_STATE, 0, sizeof(double) * Q3_LOUD_STATE, st));
}

void launch_loudness(hipStream_t st, LoudnessStage& s, const float* pcm, int G, int T, const int32_t* streams, const int32_t* metered,
                     const int64_t* pos, void* out, const int64_t* out_off, int64_t* n_out) {
    if (const char* why = loudness_launch_refusal(G, s.max_group, T, streams, s.n_streams, metered, pos)) throw Error(std::string("loudness: ") + why);
    Q3_CHECK(pcm && out && out_off && n_out, "bad buffers");
    Q3_CHECK((reinterpret_cast<uintptr_t>(pcm) & 15u) == 0, "misaligned chunk");   // the segments are read as 16-byte vectors
    bool any = false;
    for (int g = 0; g < G; g++) {
        any = any || metered[g] != 0;
        Q3_CHECK(!metered[g] || (out_off[g] >= 0 && ((reinterpret_cast<uintptr_t>(out) + (uintptr_t)out_off[g]) & 7u) == 0), "bad row offset");
        n_out[g] = 0;
    }
    if (!any) return;   // no stream is metered: nothing to run
    const LoudStreamMeta* dm;
    LoudStreamMeta* hm = s.ring.take(&dm);
    for (int g = 0; g < G; g++) {
        LoudStreamMeta& m = hm[g];
        m.slot = metered[g] ? streams[g] : -1; m.pad = 0;
        m.pos = metered[g] ? pos[g] : 0; m.out_off = metered[g] ? out_off[g] : 0;
        if (m.slot < 0) continue;
        n_out[g] = loud_blocks(pos[g], T);
        s.count->loud_chunks += 1; s.count->loud_blocks += n_out[g];
    }
    s.ring.commit(st, G);
    LoudArgs a;
    a.pcm = pcm; a.T = T; a.meta = dm; a.state = s.state; a.out = static_cast<unsigned char*>(out);
    std::copy(s.coef, s.coef + 10, a.tab.coef); std::copy(s.m, s.m + 16, a.tab.m);
    hipLaunchKernelGGL(k_loudness, dim3((unsigned)G), dim3(LOUD_THREADS), 0, st, a);
    s.ring.launched(st);
}

} // namespace q3
