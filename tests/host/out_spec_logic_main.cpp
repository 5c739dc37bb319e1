// Driver of tests/test_out_spec_logic_cpu.py: the one record of a stream's output settings (OutSpec, csrc/sched_logic.h) against the rules it
// was put together from, alone, plain g++ under the host sanitizers.  It checks everything itself, prints one "name checked" line per group
// and exits 1 at the first disagreement.
#include "../../qwen3-tts-rust_amd/csrc/sched_logic.h"
#include <cstdio>
#include <cstdlib>

using namespace q3;

static const int RATES[] = {49, 50, 100, 125, 200, 201}, PITCHES[] = {49, 50, 80, 100, 200, 201}, VOLS[] = {-401, -400, 0, 200, 201};
static const int ENCS[] = {Q3_PCM_F32, Q3_PCM_S16}, STEPS[] = {1, 24, 4096};

// the chain Engine::take_rate ran before there was a record: the volume's rule, then the pitch's, else the rate's
static const char* chain(const q3tts_pcm_format& f, int pct, int pitch, int vol, int max_steps, int64_t cap, bool codec) {
    if (vol != 0) if (const char* why = volume_submit_refusal(vol, codec)) return why;
    if (pitch != 100) return pitch_submit_refusal(pct, pitch, f, max_steps, cap, codec);
    if (pct == 100) return nullptr;
    return tsm_submit_refusal(pct, f, max_steps, cap, codec);
}
// the expression CodecDecoder::Impl::deliver classified a stream with
static int kind_before(const q3tts_pcm_format& f, int rate, int pitch) { return pitch != 100 ? 3 : rate != 100 ? 2 : !pcm_format_native(f) ? 1 : 0; }
// the bytes decoder_main staged for nf frames more of a request that had been given n native samples, computed its three ways
static int64_t bytes_before(const OutSpec& o, int64_t n, int64_t nf) {
    if (o.rate_pct != 100 || o.pitch_pct != 100) {
        auto made = [&](int64_t k) { return o.pitch_pct != 100 ? pitch_out_samples(o.rate_pct, o.pitch_pct, k, false) : tsm_out_samples(o.rate_pct, k, false); };
        return (made(n + nf * Q3_PCM_FRAME) - made(n)) * (o.fmt.encoding == Q3_PCM_S16 ? 2 : 4);
    }
    return pcm_format_native(o.fmt) ? nf * Q3_PCM_FRAME * 4 : pcm_out_bytes(o.fmt, nf);
}

#define EXPECT(c, ...) do { if (!(c)) { printf("FAILED %s: ", #c); printf(__VA_ARGS__); printf("\n"); return 1; } } while (0)

int main() {
    long n = 0;
    const int64_t caps[] = {(int64_t)24 * Q3_PCM_FRAME * 4, (int64_t)4096 * Q3_PCM_FRAME * 4};
    for (int rate : RATES) for (int pitch : PITCHES) for (int vol : VOLS) for (int ri = 0; ri < PCM_N_RATES; ri++) for (int enc : ENCS) {
        const OutSpec o{{pcm_rates()[ri], enc}, rate, pitch, vol};
        EXPECT((int)out_kind(o) == kind_before(o.fmt, rate, pitch), "rate %d pitch %d format %d/%d", rate, pitch, o.fmt.sample_rate, enc);
        EXPECT(out_sample_bytes(o) == (enc == Q3_PCM_S16 ? 2u : 4u), "encoding %d", enc);
        for (int steps : STEPS) for (int64_t cap : caps) for (int codec = 0; codec < 2; codec++) {
            const char* got = out_submit_refusal(o, steps, cap, codec != 0);
            const char* want = chain(o.fmt, rate, pitch, vol, steps, cap, codec != 0);
            EXPECT(got == want, "rate %d pitch %d vol %d format %d/%d steps %d cap %lld codec %d: '%s' for '%s'", rate, pitch, vol, o.fmt.sample_rate, enc,
                   steps, (long long)cap, codec, got ? got : "(none)", want ? want : "(none)");
            n++;
        }
    }
    printf("refusals %ld\n", n);
    EXPECT((int)out_kind(OutSpec()) == 0 && out_submit_refusal(OutSpec(), 1, 0, false) == nullptr, "the default record is the plain stream");

    // counts: every kind at every one of the eight rates, random whole-frame chunkings of up to 64 frames
    uint64_t lcg = 12345;
    auto rnd = [&](int m) { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return (int)((lcg >> 33) % (uint64_t)m); };
    const int prosody[][2] = {{100, 100}, {50, 100}, {125, 100}, {200, 100}, {100, 50}, {100, 107}, {125, 80}, {100, 200}, {80, 125}};
    n = 0;
    for (int ri = 0; ri < PCM_N_RATES; ri++) for (int enc : ENCS) for (const auto& rp : prosody) for (int rep = 0; rep < 8; rep++) {
        const OutSpec o{{pcm_rates()[ri], enc}, rp[0], rp[1], 0};
        const int total = 1 + rnd(64);
        EXPECT(out_delivered(o, 0, false) == 0, "nothing in, nothing out");
        int64_t given = 0, sum = 0;
        for (int left = total; left > 0;) {
            const int nf = 1 + rnd(left < 9 ? left : 9);
            const int64_t term = out_delivered(o, given + (int64_t)nf * Q3_PCM_FRAME, false) - out_delivered(o, given, false);
            EXPECT(term >= 0, "a chunk takes nothing back");
            EXPECT(term * (int64_t)out_sample_bytes(o) == bytes_before(o, given, nf), "kind %d format %d/%d: %lld samples of %d frames behind %lld",
                   (int)out_kind(o), o.fmt.sample_rate, enc, (long long)term, nf, (long long)given);
            if (out_kind(o) == OUT_CONVERTED) EXPECT(term == pcm_out_samples(o.fmt, nf), "the converter's chunk of %d frames at %d Hz", nf, o.fmt.sample_rate);
            if (out_kind(o) == OUT_NATIVE) EXPECT(term == (int64_t)nf * Q3_PCM_FRAME, "the native chunk of %d frames", nf);
            sum += term; given += (int64_t)nf * Q3_PCM_FRAME; left -= nf;
        }
        EXPECT(sum == out_delivered(o, (int64_t)total * Q3_PCM_FRAME, false), "the chunks of %d frames add up", total);
        EXPECT(out_delivered(o, given, true) >= out_delivered(o, given, false), "a flush takes nothing back");
        if (out_kind(o) < OUT_RATED) EXPECT(out_delivered(o, given, true) == out_delivered(o, given, false), "only a stretched or shifted stream is flushed");
        n++;
    }
    printf("counts %ld\n", n);
    return 0;
}
