// intake.h -- [EXT] reference audio intake (q3tts_spec.h "reference audio intake"): everything the intake decides without a device.  Which
// rates it takes and their ratios, how many samples come out, the prototype filter and its phase-major image (both through pcm_out.h's
// builders: the intake and the output converter share one filter definition), how many outputs a block of the kernel computes per ratio,
// what a clip is refused for, and a WAV header reader that never looks past its buffer.  No HIP, no threads:
// tests/host/intake_logic_main.cpp builds it with plain g++ under the host sanitizers.
#pragma once
#include "pcm_out.h"
#include <cstring>

namespace q3 {

// what k_intake's LDS holds, in floats: the ratio's table, the tile's input window, the tile's outputs (64 KB less the block's flag words)
constexpr int INTAKE_LDS_FLOATS = 16384 - 16;
constexpr int INTAKE_TILE_MAX = 1024, INTAKE_TILE_MIN = 64;

// 24000 / rate = L / M in lowest terms; taps = the most terms one output sums, stride = taps rounded up to whole 16-byte vectors,
// c = the prototype's centre, tile = outputs per block.  24000 Hz has no filter: L = M = 1, no taps, a full tile.
struct IntakePlan { int L = 1, M = 1, n_taps = 0, taps = 0, stride = 0, c = 0, tile = INTAKE_TILE_MAX; };

inline int intake_table_floats(const IntakePlan& p) { return p.L * p.stride; }
// input frames the outputs of one tile reach: j(m) = (m M + c) div L moves by at most ceil((tile - 1) M / L) over a tile, and the first
// output reaches stride - 1 frames back; one more so that rounding the parts separately can never come short
inline int64_t intake_window_floats(const IntakePlan& p, int tile) { return ((int64_t)(tile - 1) * p.M + p.L - 1) / p.L + p.stride + 1; }
inline int64_t intake_lds_floats(const IntakePlan& p, int tile) {
    return intake_table_floats(p) + (intake_window_floats(p, tile) + 3) / 4 * 4 + tile;
}

inline const char* intake_rate_why_not(int rate) {
    if (rate < Q3_INTAKE_MIN_RATE || rate > Q3_INTAKE_MAX_RATE) return "sample rate outside [8000, 192000]";
    int a = rate, b = Q3_PCM_NATIVE_RATE;
    while (b) { const int t = a % b; a = b; b = t; }
    if (rate / a > Q3_INTAKE_MAX_F || Q3_PCM_NATIVE_RATE / a > Q3_INTAKE_MAX_F) return "sample rate has no ratio to 24000 within 320";
    return nullptr;
}
inline bool intake_plan(int rate, IntakePlan* out) {
    if (intake_rate_why_not(rate)) return false;
    int a = rate, b = Q3_PCM_NATIVE_RATE;
    while (b) { const int t = a % b; a = b; b = t; }
    IntakePlan p;
    p.L = Q3_PCM_NATIVE_RATE / a; p.M = rate / a;
    if (rate != Q3_PCM_NATIVE_RATE) {
        const int F = p.L > p.M ? p.L : p.M;
        p.c = Q3_PCM_FILTER_Z * F;
        p.n_taps = 2 * p.c + 1;
        p.taps = (p.n_taps + p.L - 1) / p.L;
        p.stride = (p.taps + PCM_TAPS_ALIGN - 1) / PCM_TAPS_ALIGN * PCM_TAPS_ALIGN;
        p.tile = 0;
        for (int t = INTAKE_TILE_MAX; t >= INTAKE_TILE_MIN; t /= 2)
            if (intake_lds_floats(p, t) <= INTAKE_LDS_FLOATS) { p.tile = t; break; }
        if (p.tile == 0) return false;   // no accepted ratio comes here: 64 outputs need at most 11521 + 768 + 64 floats
    }
    *out = p;
    return true;
}
// ceil(n L / M); -1 for a rate the intake does not take or n < 0
inline int64_t intake_samples(int rate, int64_t n) {
    IntakePlan p;
    if (n < 0 || !intake_plan(rate, &p)) return -1;
    return (n * p.L + p.M - 1) / p.M;
}
inline std::vector<float> intake_filter(int rate) {
    IntakePlan p;
    if (!intake_plan(rate, &p) || p.n_taps == 0) return std::vector<float>();
    return pcm_filter_lm(p.L, p.M);
}
// the phase-major image of h, [L][stride], by the converter's builder
inline std::vector<float> intake_table(const IntakePlan& p, const std::vector<float>& h) {
    PcmPlan q;
    q.L = p.L; q.M = p.M; q.n_taps = p.n_taps; q.taps_per_phase = p.taps;
    return pcm_filter_phase_major(q, h);
}

inline int intake_sample_bytes(int fmt) {
    switch (fmt) {
    case Q3_INTAKE_U8: return 1;
    case Q3_INTAKE_S16: return 2;
    case Q3_INTAKE_S24: return 3;
    case Q3_INTAKE_S32: case Q3_INTAKE_F32: return 4;
    default: return 0;
    }
}
// what a clip is refused for (nullptr = it may run)
inline const char* intake_refusal(const q3tts_intake_clip* c) {
    if (!c) return "null clip";
    if (const char* why = intake_rate_why_not(c->sample_rate)) return why;
    if (c->channels < 1 || c->channels > Q3_INTAKE_MAX_CH) return "channel count outside [1, 8]";
    if (intake_sample_bytes(c->sample_format) == 0) return "unknown sample format";
    if (c->downmix != Q3_INTAKE_FIRST && c->downmix != Q3_INTAKE_MEAN) return "unknown downmix";
    if (c->n_frames < 1) return "clip is empty";
    if (c->n_frames > (int64_t)Q3_INTAKE_MAX_OUT * 8 || intake_samples(c->sample_rate, c->n_frames) > Q3_INTAKE_MAX_OUT) return "clip is longer than 120 s";
    if (!c->data) return "null samples";
    return nullptr;
}

// ---- RIFF/WAVE header.  Reads only bytes below n; nullptr = *out is filled, else why the file is not one the intake reads ----
inline uint32_t wav_u32(const unsigned char* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
inline uint32_t wav_u16(const unsigned char* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
inline const char* wav_probe(const void* bytes, int64_t n, q3tts_wav_info* out) {
    if (!bytes || !out || n < 0) return "null argument";
    const unsigned char* d = (const unsigned char*)bytes;
    if (n < 12 || memcmp(d, "RIFF", 4) != 0 || memcmp(d + 8, "WAVE", 4) != 0) return "no RIFF/WAVE header";
    uint32_t tag = 0, ch = 0, rate = 0, align = 0, bits = 0;
    bool have_fmt = false;
    for (int64_t p = 12; p + 8 <= n;) {
        const int64_t len = (int64_t)wav_u32(d + p + 4), left = n - p - 8, avail = len < left ? len : left;
        const unsigned char* body = d + p + 8;
        if (memcmp(d + p, "fmt ", 4) == 0) {
            if (have_fmt) return "second fmt chunk";
            if (avail < 16) return "fmt chunk shorter than 16 bytes";
            tag = wav_u16(body); ch = wav_u16(body + 2); rate = wav_u32(body + 4); align = wav_u16(body + 12); bits = wav_u16(body + 14);
            if (tag == 0xFFFE) {   // WAVE_FORMAT_EXTENSIBLE: the sub-format's first word is the tag
                if (avail < 40) return "extensible fmt chunk shorter than 40 bytes";
                tag = wav_u16(body + 24);
            }
            if (tag != 1 && tag != 3) return "format tag is neither PCM (1) nor IEEE float (3)";
            if (ch == 0) return "zero channels";
            if (rate == 0 || rate > 0x7fffffffu) return "bad sample rate";
            if (tag == 1 ? (bits != 8 && bits != 16 && bits != 24 && bits != 32) : bits != 32) return "sample width is not 8, 16, 24 or 32 bit PCM or 32 bit float";
            if (align != ch * (bits / 8)) return "block align contradicts channels x bits";
            have_fmt = true;
        } else if (memcmp(d + p, "data", 4) == 0) {
            if (!have_fmt) return "data chunk before fmt chunk";
            out->sample_format = tag == 3 ? Q3_INTAKE_F32 : bits == 8 ? Q3_INTAKE_U8 : bits == 16 ? Q3_INTAKE_S16 : bits == 24 ? Q3_INTAKE_S24 : Q3_INTAKE_S32;
            out->channels = (int32_t)ch; out->sample_rate = (int32_t)rate; out->bits = (int32_t)bits;
            out->data_offset = p + 8; out->n_frames = avail / (int64_t)align;
            return nullptr;
        }
        p += 8 + len + (len & 1);   // chunks are padded to even lengths
    }
    return have_fmt ? "no data chunk" : "no fmt chunk";
}

} // namespace q3
