// [EXT] reference audio intake end to end (tests/test_gpu_intake.py): a model directory with test-written encoder graphs is opened by the C++
// mirror of the reference API.  With the intake on, create_voice_file on a 48 kHz stereo s16 WAV must give the codes and the embedding, bit for
// bit, that the default path gives on a 24 kHz mono f32 WAV holding q3tts_wav_intake's output of that file (written by the test, one per
// downmix); with it off the 48 kHz file is refused with the reference's text.  The raw-audio generate path keeps its cache in
// "<stem>.intake.cache" and leaves "<stem>.cache" alone.
#include "../../qwen3-tts-rust_amd/host/tts_engine.hpp"
#include <cstdio>
#include <cstring>
#include <stdexcept>

static bool exists(const std::string& p) { if (FILE* f = fopen(p.c_str(), "rb")) { fclose(f); return true; } return false; }

int main(int argc, char** argv) {
    using namespace q3tts;
    if (argc < 6) { fprintf(stderr, "usage: intake_main <model_dir> <clip48k.wav> <first24k.wav> <mean24k.wav> <ref2_44k.wav>\n"); return 2; }
    try {
        TtsEngine eng = TtsEngine::new_(argv[1], "q8_0");
        if (!eng.has_encoders()) throw std::runtime_error("encoders were not loaded");
        if (eng.reference_intake() != -1) throw std::runtime_error("the intake must be off by default");
        try { eng.create_voice_file(argv[2], "x"); throw std::runtime_error("48 kHz audio should be refused while the intake is off"); }
        catch (const std::runtime_error& e) { if (std::string(e.what()).find("Expected 24000Hz audio, found 48000Hz") == std::string::npos) throw; }
        const int modes[2] = {Q3_INTAKE_FIRST, Q3_INTAKE_MEAN};
        std::vector<int64_t> first_codes;
        for (int k = 0; k < 2; k++) {
            eng.set_reference_intake(-1);
            const VoiceFile want = eng.create_voice_file(argv[3 + k], "reference text");   // the default path on the intake's own output
            eng.set_reference_intake(modes[k]);
            const VoiceFile got = eng.create_voice_file(argv[2], "reference text");
            if (got.audio_codes.empty() || got.audio_codes.size() % 16 != 0 || got.speaker_embedding.size() != 2048) throw std::runtime_error("VoiceFile has the wrong shape");
            if (got.audio_codes != want.audio_codes) throw std::runtime_error("codes differ from the default path on the intake's output");
            if (memcmp(got.speaker_embedding.data(), want.speaker_embedding.data(), 2048 * sizeof(float)) != 0) throw std::runtime_error("embedding differs from the default path on the intake's output");
            const VoiceFile again = eng.create_voice_file(argv[3 + k], "reference text");   // a 24 kHz mono f32 file through the intake: as it is
            if (again.audio_codes != want.audio_codes || memcmp(again.speaker_embedding.data(), want.speaker_embedding.data(), 2048 * sizeof(float)) != 0)
                throw std::runtime_error("a 24 kHz mono f32 file changed on its way through the intake");
            if (k == 0) first_codes = got.audio_codes;
            printf("MODE %d CODES %zu\n", modes[k], got.audio_codes.size());
        }
        // generate from raw reference audio at 44.1 kHz: the intake's own cache file
        SamplerConfig sc; sc.temperature = 0.0f; sc.seed = 42;
        eng.set_sampler_config(sc);
        eng.set_max_steps(6);
        eng.set_reference_intake(Q3_INTAKE_FIRST);
        std::string stem = argv[5];
        stem.resize(stem.find_last_of('.'));
        std::vector<int32_t> ids = {100, 101, 102, 103}, ref_text = {7, 8, 9}, c1, c2;
        AudioSample a = eng.generate_ids(ids, argv[5], ref_text, nullptr, &c1);
        if (!exists(stem + ".intake.cache") || exists(stem + ".cache")) throw std::runtime_error("the intake's cache file is not where it belongs");
        std::vector<int64_t> cc; std::vector<float> ce;
        cache::load_cache(stem + ".intake.cache", cc, ce);
        const VoiceFile v = eng.create_voice_file(argv[5], "x");
        if (ce.size() != 2048 || cc != v.audio_codes || memcmp(ce.data(), v.speaker_embedding.data(), 2048 * sizeof(float)) != 0)
            throw std::runtime_error("the cache does not hold what create_voice_file makes of the same clip");
        AudioSample b = eng.generate_ids(ids, argv[5], ref_text, nullptr, &c2);   // second call: the cache short-cut
        if (c1 != c2 || a.samples != b.samples) throw std::runtime_error("cache-backed generate differs from the encoder-backed one");
        try { eng.set_reference_intake(7); throw std::runtime_error("mode 7 should be refused"); }
        catch (const std::runtime_error& e) { if (std::string(e.what()).find("reference intake mode") == std::string::npos) throw; }
        printf("OK\n");
        return 0;
    } catch (const std::exception& e) { fprintf(stderr, "intake_main: %s\n", e.what()); return 1; }
}
