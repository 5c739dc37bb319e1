// volume.hip -- [EXT] volume (q3tts_spec.h "volume"): a gain with a look-ahead peak limiter behind the output conv, in place on the native
// chunk, at most one launch per decode pass and only when the pass holds a stream with a volume.
//
// k_volume: grid = G, 512 lanes, one workgroup per stream; a stream without a volume exits at once.  The chunk is walked in tiles of 1920
// samples from the end downwards, which makes the rewrite in place safe: tile [a, b) takes v[a - 638 .. b) into LDS -- from the chunk, below
// the chunk's first sample from the stream's store -- before it writes [a, b), and every tile below it reads below a only.  In LDS sample
// a - 638 + j sits at word j + 2, so the tile's own samples start on a 16-byte boundary.  r goes into a second array; the nine min levels
// (offsets 1 .. 256) and the seven sum levels (offsets 1 .. 64) are ping-pong passes between it and a third, 16 passes that end in the
// second; word j is final once j >= 638, which is where the tile's own samples begin.  Lane t < 480 then forms samples a + 4 t .. + 3 and
// stores them as one 16-byte vector.
//
// State: hist [n_streams][638], a stream's last 638 values of v.  The topmost tile, walked first, keeps the chunk's last 638 values in LDS;
// they are stored behind the barriers that follow the lowest tile's read of the store.  No counters, no atomics, no scratch.
#include "out_stages.h"
#include "kdev.h"
#include "volume.h"
#include "wsola.h"

namespace q3 {

#define VOL_THREADS 512
#define VOL_PAD 2                                  // words in front of an LDS array: (VOL_PAD + Q3_VOL_HIST) % 4 == 0
#define VOL_WORDS (VOL_PAD + VOL_SPAN)             // 2560
static_assert((VOL_PAD + Q3_VOL_HIST) % 4 == 0 && VOL_WORDS % 4 == 0, "the tile's own samples start on 16 bytes");
static_assert(VOL_TILE / 4 <= VOL_THREADS, "one vector per lane");
static_assert(Q3_VOL_HOLD == 512 && Q3_VOL_LOOK == 128 && Q3_VOL_DELAY == Q3_VOL_LOOK - 1 && Q3_VOL_HIST == Q3_VOL_HOLD - 1 + Q3_VOL_DELAY, "nine min levels, seven sum levels");

struct VolArgs { float* pcm; int T; const VolStreamMeta* meta; float* hist; float* trace; };

__device__ __forceinline__ float vol_required(float v) {
    const float av = fabsf(v);
    return av <= 1.0f ? 1.0f : 1.0f / av;
}

__global__ void __launch_bounds__(VOL_THREADS) k_volume(VolArgs a) {
    __shared__ __attribute__((aligned(16))) float sv[VOL_WORDS];
    __shared__ __attribute__((aligned(16))) float sp[VOL_WORDS];
    __shared__ __attribute__((aligned(16))) float sq[VOL_WORDS];
    __shared__ float keep[Q3_VOL_HIST];
    const int g = blockIdx.x, tid = threadIdx.x;
    const VolStreamMeta mt = a.meta[g];
    if (mt.slot < 0) return;   // uniform: the stream has no volume
    float* const x = a.pcm + (size_t)g * a.T;
    float* const h = a.hist + (size_t)mt.slot * Q3_VOL_HIST;
    const float G = mt.gain;
    for (int lo = a.T - VOL_TILE; lo >= 0; lo -= VOL_TILE) {
        // v[lo - 638 .. lo + 1920) and r of it
        if (tid < VOL_TILE / 4) {
            const float4 c = reinterpret_cast<const float4*>(x + lo)[tid];
            const float4 v = make_float4(G * c.x, G * c.y, G * c.z, G * c.w);
            reinterpret_cast<float4*>(sv + VOL_PAD + Q3_VOL_HIST)[tid] = v;
            reinterpret_cast<float4*>(sp + VOL_PAD + Q3_VOL_HIST)[tid] = make_float4(vol_required(v.x), vol_required(v.y), vol_required(v.z), vol_required(v.w));
        }
        for (int j = tid; j < Q3_VOL_HIST; j += VOL_THREADS) {
            const int i = lo - Q3_VOL_HIST + j;   // in [-638, lo)
            const float v = i >= 0 ? G * x[i] : h[Q3_VOL_HIST + i];
            sv[VOL_PAD + j] = v;
            sp[VOL_PAD + j] = vol_required(v);
        }
        __syncthreads();
        if (lo == a.T - VOL_TILE)
            for (int j = tid; j < Q3_VOL_HIST; j += VOL_THREADS) keep[j] = sv[VOL_PAD + VOL_TILE + j];   // v[T - 638 .. T)
        float* src = sp; float* dst = sq;
#pragma unroll 1
        for (int lvl = 0; lvl < 16; lvl++) {
            const int off = lvl < 9 ? 1 << lvl : 1 << (lvl - 9);
            for (int j = tid; j < VOL_SPAN; j += VOL_THREADS) {
                const float c = src[VOL_PAD + j];
                float o = c;
                if (j >= off) { const float b = src[VOL_PAD + j - off]; o = lvl < 9 ? fminf(b, c) : b + c; }
                dst[VOL_PAD + j] = o;
            }
            __syncthreads();
            float* t = src; src = dst; dst = t;
        }
        // 16 passes: the sums are back in sp
        if (tid < VOL_TILE / 4) {
            const float4 s = reinterpret_cast<const float4*>(sp + VOL_PAD + Q3_VOL_HIST)[tid];
            const float* vd = sv + VOL_PAD + Q3_VOL_HIST - Q3_VOL_DELAY + 4 * tid;   // v[n - 127]
            const float4 gn = make_float4(0x1p-7f * s.x, 0x1p-7f * s.y, 0x1p-7f * s.z, 0x1p-7f * s.w);
            reinterpret_cast<float4*>(x + lo)[tid] = make_float4(pcm_clamp(gn.x * vd[0]), pcm_clamp(gn.y * vd[1]), pcm_clamp(gn.z * vd[2]), pcm_clamp(gn.w * vd[3]));
            if (a.trace) {
                float* tr = a.trace + mt.trace_off + lo + 4 * tid;
                tr[0] = gn.x; tr[1] = gn.y; tr[2] = gn.z; tr[3] = gn.w;
            }
        }
        __syncthreads();   // the next tile overwrites sv and sp
    }
    for (int j = tid; j < Q3_VOL_HIST; j += VOL_THREADS) h[j] = keep[j];
}

VolumeStage::VolumeStage(int n_streams_, int max_group_, StageCounters* count_) : StageBase(n_streams_, max_group_, count_, "volume stage") {
    hist_own.alloc((size_t)n_streams * Q3_VOL_HIST); hist_own.zero();
    hist = hist_own.p;
    Q3_HIP(hipStreamSynchronize(nullptr)); // the memset ran on the null stream, which the caller's non-blocking streams do not wait for
    ring.alloc(max_group);
}

void VolumeStage::reset_async(hipStream_t st, int slot) {
    check_slot(slot);
    Q3_HIP(hipMemsetAsync(hist + (size_t)slot * Q3_VOL_HIST, 0, sizeof(float) * Q3_VOL_HIST, st));
}

void launch_volume(hipStream_t st, VolumeStage& s, float* pcm, int G, int T, const int32_t* streams, const int32_t* db10, float* trace,
                   const int64_t* trace_off) {
    if (const char* why = volume_launch_refusal(G, s.max_group, T, streams, s.n_streams, db10)) throw Error(std::string("volume: ") + why);
    Q3_CHECK(pcm && (!trace || trace_off), "bad buffers");
    Q3_CHECK((reinterpret_cast<uintptr_t>(pcm) & 15u) == 0, "misaligned chunk");   // the tiles are read and written as 16-byte vectors
    bool any = false;
    for (int g = 0; g < G; g++) {
        any = any || db10[g] != 0;
        Q3_CHECK(!trace || trace_off[g] >= 0, "bad trace offset");
    }
    if (!any) return;   // no stream has a volume: nothing to run
    const VolStreamMeta* dm;
    VolStreamMeta* hm = s.ring.take(&dm);
    for (int g = 0; g < G; g++) {
        VolStreamMeta& m = hm[g];
        m.gain = db10[g] == 0 ? 1.0f : volume_gain(db10[g]);
        m.slot = db10[g] == 0 ? -1 : streams[g];
        m.trace_off = trace ? trace_off[g] : 0;
        if (m.slot < 0) continue;
        s.count->vol_chunks += 1; s.count->vol_samples += T;
    }
    s.ring.commit(st, G);
    VolArgs a{pcm, T, dm, s.hist, trace};
    hipLaunchKernelGGL(k_volume, dim3((unsigned)G), dim3(VOL_THREADS), 0, st, a);
    s.ring.launched(st);
}

} // namespace q3
