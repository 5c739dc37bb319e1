// Driver of tests/test_out_spec_logic_cpu.py: the one record of a stream's output settings (OutSpec, csrc/sched_logic.h) against the rules it
// was put together from, and the routing of a pass's streams behind the output conv (out_route) against the expressions the codec's pass tail
// used before there was one, alone, plain g++ under the host sanitizers.  It checks everything itself, prints one "name checked" line per group
// and exits 1 at the first disagreement.
#include "../../qwen3-tts-rust_amd/csrc/sched_logic.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

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

// what CodecDecoder::Impl::run_loudness, run_volume and deliver worked out for the G streams of a pass before out_route: which launches ran,
// what each launcher was handed per stream, and the source, offset and sample size of each stream's copy.  Arrays a path did not write
// (deliver's on a pass of native streams, all of them under a null `out`) stay unset and are not compared
struct Before {
    bool conv = false, rated = false, pitched = false, volume = false, meter = false, args = false;
    q3tts_pcm_format cf[4]; int32_t pct[4], pr[4], pp[4], enc[4], vol[4], met[4]; int64_t toff[4], loff[4];
    int src[4]; size_t src_off[4], bytes[4];
};
static const char* route_before(const OutSpec* out, int G, int64_t T, size_t region, size_t loud_cap, Before* b) {
    *b = Before();
    if (out) {   // run_loudness, then run_volume
        for (int g = 0; g < G; g++) { b->met[g] = out[g].loud != 0; b->meter = b->meter || b->met[g]; b->loff[g] = (int64_t)((size_t)g * loud_cap * 2 * sizeof(double)); }
        for (int g = 0; g < G; g++) { b->vol[g] = out[g].vol_db10; b->volume = b->volume || b->vol[g] != 0; }
    }
    bool any[4] = {false, false, false, false};   // deliver
    for (int g = 0; out && g < G; g++) any[kind_before(out[g].fmt, out[g].rate_pct, out[g].pitch_pct)] = true;
    if (!any[1] && !any[2] && !any[3]) {
        for (int g = 0; g < G; g++) { b->src[g] = 0; b->src_off[g] = (size_t)g * T; b->bytes[g] = 4; }
        return nullptr;
    }
    b->args = true; b->conv = any[1]; b->rated = any[2]; b->pitched = any[3];
    for (int g = 0; g < G; g++) {
        const int k = kind_before(out[g].fmt, out[g].rate_pct, out[g].pitch_pct);
        b->cf[g] = q3tts_pcm_format{Q3_PCM_NATIVE_RATE, Q3_PCM_F32}; b->pct[g] = b->pr[g] = b->pp[g] = 100; b->enc[g] = Q3_PCM_F32; b->toff[g] = 0;
        if (k == 1) b->cf[g] = out[g].fmt;
        if (k < 2) continue;
        if (out[g].fmt.sample_rate != Q3_PCM_NATIVE_RATE) return "a speech rate or a pitch needs the 24000 Hz output format";
        b->enc[g] = out[g].fmt.encoding;
        if (k == 3) { b->pr[g] = out[g].rate_pct; b->pp[g] = out[g].pitch_pct; }
        else b->pct[g] = out[g].rate_pct;
    }
    if (any[2] || any[3]) {
        if (!(2 * (size_t)T + 3 * Q3_TSM_HOP <= region)) return "chunk too long for the stretcher's buffers";
        for (int g = 0; g < G; g++) b->toff[g] = (int64_t)((size_t)g * region * sizeof(float));
    }
    for (int g = 0; g < G; g++) {
        const int k = kind_before(out[g].fmt, out[g].rate_pct, out[g].pitch_pct);
        b->src[g] = k; b->src_off[g] = k < 2 ? (size_t)g * T : (size_t)g * region;
        b->bytes[g] = out[g].fmt.encoding == Q3_PCM_S16 ? 2 : 4;
    }
    return nullptr;
}
// 0: out_route says of the pass what route_before says
static int route_differs(const OutSpec* out, int G, int64_t T, size_t region, size_t loud_cap, OutRoute* r) {
    Before b;
    const char* want = route_before(out, G, T, region, loud_cap, &b);
    const char* got = out_route(out, G, T, region, loud_cap, r);
    if ((got == nullptr) != (want == nullptr) || (got && strcmp(got, want) != 0)) return 1;
    if (got) return 0;
    if (r->run[OUT_CONVERTED] != b.conv || r->run[OUT_RATED] != b.rated || r->run[OUT_PITCHED] != b.pitched) return 2;
    if (r->any_volume != b.volume || r->any_metered != b.meter || r->all_native() != !b.args) return 3;
    for (int g = 0; g < G; g++) {
        if ((int)r->src[g] != b.src[g] || r->src_off[g] != b.src_off[g] || r->bytes[g] != b.bytes[g]) return 4;
        if (out && (r->vol[g] != b.vol[g] || r->metered[g] != b.met[g] || r->loff[g] != b.loff[g])) return 5;
        if (!out && (r->vol[g] != 0 || r->metered[g] != 0)) return 6;
        if (b.args && (r->cf[g].sample_rate != b.cf[g].sample_rate || r->cf[g].encoding != b.cf[g].encoding || r->pct[g] != b.pct[g] || r->pr[g] != b.pr[g] ||
                       r->pp[g] != b.pp[g] || r->enc[g] != b.enc[g] || r->toff[g] != b.toff[g])) return 7;
        // what a stage that does run is told about a stream that is not its own, also where deliver never got that far
        if (!b.args && (!pcm_format_native(r->cf[g]) || r->pct[g] != 100 || r->pp[g] != 100)) return 8;
    }
    return 0;
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

    // the routing: every single stream, then groups of 2 and 4 drawn from the same grid, at one frame and at three
    const size_t region = 2 * 3 * (size_t)Q3_PCM_FRAME + 8 * Q3_TSM_HOP, loud_cap = 3 * (size_t)Q3_PCM_FRAME / Q3_LOUD_BLOCK + 1;
    OutRoute route(4);
    std::vector<OutSpec> all;
    for (int rate : RATES) for (int pitch : PITCHES) for (int vol : VOLS) for (int ri = 0; ri < PCM_N_RATES; ri++) for (int enc : ENCS) for (int loud = 0; loud < 2; loud++)
        all.push_back(OutSpec{{pcm_rates()[ri], enc}, rate, pitch, vol, loud});
    n = 0;
    long refused = 0;
    for (int64_t T : {(int64_t)Q3_PCM_FRAME, (int64_t)3 * Q3_PCM_FRAME}) {
        for (int G : {1, 2, 4}) for (size_t i = 0; i < (G == 1 ? all.size() : 20000); i++) {
            OutSpec out[4];
            for (int g = 0; g < G; g++) out[g] = G == 1 ? all[i] : all[(size_t)rnd((int)all.size())];
            const int d = route_differs(out, G, T, region, loud_cap, &route);
            EXPECT(d == 0, "difference %d at T %lld G %d draw %zu", d, (long long)T, G, i);
            refused += out_route(out, G, T, region, loud_cap, &route) != nullptr;
            n++;
        }
        for (int G : {1, 2, 4}) {   // a null out; the group of default records: G copies of the native chunk either way
            const OutSpec plain[4];
            EXPECT(route_differs(nullptr, G, T, region, loud_cap, &route) == 0 && route.all_native() && !route.any_volume && !route.any_metered, "null out, G %d", G);
            EXPECT(route_differs(plain, G, T, region, loud_cap, &route) == 0 && route.all_native(), "all-native group, G %d", G);
            for (int g = 0; g < G; g++) EXPECT(route.src[g] == OUT_NATIVE && route.src_off[g] == (size_t)g * T && route.bytes[g] == 4, "native copy %d of %d", g, G);
            n += 2;
        }
    }
    EXPECT(refused > 0, "no drawn group had a rate at a non-native format");
    const OutSpec late[2] = {OutSpec(), OutSpec{{16000, Q3_PCM_S16}, 125, 100, 0, 0}};
    EXPECT(route_differs(late, 2, Q3_PCM_FRAME, region, loud_cap, &route) == 0, "a rate at 16000 Hz");
    EXPECT(!strcmp(out_route(late, 2, Q3_PCM_FRAME, region, loud_cap, &route), "a speech rate or a pitch needs the 24000 Hz output format"), "the refusal's text");
    const OutSpec slow[1] = {OutSpec{{Q3_PCM_NATIVE_RATE, Q3_PCM_F32}, 50, 100, 0, 0}};
    EXPECT(route_differs(slow, 1, 3 * Q3_PCM_FRAME, region / 3, loud_cap, &route) == 0, "a chunk longer than the region");
    EXPECT(!strcmp(out_route(slow, 1, 3 * Q3_PCM_FRAME, region / 3, loud_cap, &route), "chunk too long for the stretcher's buffers"), "the region check's text");
    printf("routes %ld\n", n);
    return 0;
}
