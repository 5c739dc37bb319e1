// TtsEngine::encode_speaker on clips around the first mel frame (256 samples): below it the mel front end has no frame and the call must throw
// its "audio too short" error instead of feeding the speaker encoder a frame of zeros; from 256 samples on it returns the graph's embedding.
#include "../../qwen3-tts-rust_amd/host/tts_engine.hpp"
#include <cstdio>
#include <stdexcept>

int main(int argc, char** argv) {
    using namespace q3tts;
    if (argc < 2) { fprintf(stderr, "usage: short_clip_main <model_dir>\n"); return 2; }
    try {
        TtsEngine eng = TtsEngine::new_(argv[1], "q8_0");
        for (int n : {0, 1, 100, 255}) {
            std::vector<float> clip((size_t)n, 0.25f);
            try { eng.encode_speaker(clip); throw std::logic_error("a clip of " + std::to_string(n) + " samples was encoded"); }
            catch (const std::runtime_error& e) { if (std::string(e.what()).find("audio too short") == std::string::npos) throw; }
        }
        std::vector<float> clip(256, 0.25f);
        const std::vector<float> emb = eng.encode_speaker(clip);
        if (emb.size() != 2048) throw std::logic_error("a 256-sample clip gives one frame and a 2048-d embedding");
        printf("OK\n");
        return 0;
    } catch (const std::exception& e) { fprintf(stderr, "short_clip_main: %s\n", e.what()); return 1; }
}
