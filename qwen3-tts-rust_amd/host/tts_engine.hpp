// tts_engine.hpp -- C++ mirror of the reference's public Rust API over the C ABI (include/q3tts.h).
// The reference's host language (Rust, edition 2024) has no toolchain in this image, so the host side above the
// C ABI is C++ with the same names, argument meaning and error behaviour:
//   SamplerConfig            /root/reference/src/tts/engine.rs:13-45
//   VoiceFile                /root/reference/src/utils/voice_file.rs:5-62  (JSON, alias spk_emb, unknown keys ignored)
//   AudioSample              /root/reference/src/utils/audio.rs:4-46       (save_wav: i16, x32767 clamp)
//   TtsEngine::{new_, set_max_steps, set_sampler_config, get_sampler_config, load_speakers, get_speaker,
//               generate_with_voice, create_voice_file}   /root/reference/src/tts/engine.rs:84-435
// Text -> token ids (src/utils/tokenizer.rs): <model_dir>/tokenizer/tokenizer.json is read by the engine's own byte-level BPE (q3tts_tokenizer_*,
// SURVEY row f-3) when the file exists; a caller-supplied tokenizer function takes precedence.
#pragma once
#include "../../include/q3tts.h"
#include <functional>
#include <map>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

namespace q3tts {

struct SamplerConfig { // engine.rs:13-45
    float temperature = 0.7f; int top_k = 40; float top_p = 0.9f; std::optional<uint64_t> seed;
};

struct VoiceFile { // voice_file.rs:5-22
    std::string ref_text; std::vector<int64_t> audio_codes; std::vector<float> speaker_embedding;
    std::optional<std::string> name, gender, age, description;
    static VoiceFile load(const std::string& path);   // throws std::runtime_error with the parse error
    void save(const std::string& path) const;
};

// ".cache" files next to reference audio (utils/cache.rs:5-67): "TTSC", u32 version 1, u64 n + n x i64 codes, u64 m + m x f32 embedding,
// little endian.  Errors carry the reference's messages ("Invalid magic bytes", "Unsupported version").
namespace cache {
void save_cache(const std::string& path, const std::vector<int64_t>& codes, const std::vector<float>& emb);
void load_cache(const std::string& path, std::vector<int64_t>& codes, std::vector<float>& emb);
}

struct AudioSample { // audio.rs:4-46
    std::vector<float> samples; uint32_t sample_rate = 24000; uint16_t channels = 1;
    // [EXT] output formats (q3tts_spec.h): encoding 1 = the engine delivered int16 at sample_rate; they are in samples16, as delivered, and
    // samples holds the same values / 32767 for callers that want floats
    int32_t encoding = 0; std::vector<int16_t> samples16;
    static AudioSample load_wav(const std::string& path); // audio.rs:11-23: samples read as i16 / 32768, channel count kept but not de-interleaved
    void save_wav(const std::string& path) const;         // PCM16 at sample_rate; an int16 sample is written as it is
    float duration() const { return (float)samples.size() / (float)sample_rate; }
};

using Tokenizer = std::function<std::vector<int32_t>(const std::string&)>;

class TtsEngine {
public:
    // TtsEngine::new(model_dir, quant) -- engine.rs:84-169 (no downloader: local paths only)
    static TtsEngine new_(const std::string& model_dir, const std::string& quant, Tokenizer tok = nullptr);
    TtsEngine(TtsEngine&&) noexcept; TtsEngine& operator=(TtsEngine&&) noexcept;
    TtsEngine(const TtsEngine&) = delete;
    ~TtsEngine();
    void set_max_steps(size_t steps) { max_steps_ = steps; }                       // :172-174
    // [EXT] output formats: what generate_with_voice_ids_stream and vocode deliver from now on (q3tts_engine_set_output_format; rate 0 =
    // native).  The blocking generate* calls stay native.  The converted audio lags by 16 F / L native samples and loses that much at its end
    void set_output_format(uint32_t sample_rate, int32_t encoding);
    void set_sampler_config(const SamplerConfig& c) { sampler_ = c; }              // :177-179
    const SamplerConfig& get_sampler_config() const { return sampler_; }           // :182-184
    void load_speakers(const std::string& dir);                                    // :187-208
    const VoiceFile& get_speaker(const std::string& id_or_name) const;             // :211-231 (vivian fallback)
    bool has_tokenizer() const { return (bool)tok_; }
    std::vector<int32_t> encode(const std::string& text) const { if (!tok_) throw std::runtime_error("Failed to load tokenizer: no tokenizer/tokenizer.json in the model directory"); return tok_(text); }
    // generate_with_voice -- :390-435; text goes through the pluggable tokenizer
    AudioSample generate_with_voice(const std::string& text, const VoiceFile& voice, const std::optional<std::string>& instruct = std::nullopt);
    AudioSample generate_with_voice_ids(const std::vector<int32_t>& text_ids, const VoiceFile& voice,
                                        const std::vector<int32_t>* instruct_ids = nullptr, const std::vector<int32_t>* ref_text_ids = nullptr,
                                        std::vector<int32_t>* codes_out = nullptr);
    // generate -- engine.rs:243-271: voice cloning from reference audio.  process_reference (:275-301) takes the codes + speaker
    // embedding from "<audio>.cache" when that file exists; otherwise it needs the ONNX encoders and fails with the reference's message.
    AudioSample generate_ids(const std::vector<int32_t>& text_ids, const std::string& ref_audio_path, const std::vector<int32_t>& ref_text_ids,
                             const std::vector<int32_t>* instruct_ids = nullptr, std::vector<int32_t>* codes_out = nullptr);
    AudioSample generate(const std::string& text, const std::string& ref_audio_path, const std::string& ref_text,
                         const std::optional<std::string>& instruct = std::nullopt);
    // Streaming form (the reference keeps its `stream_tx` private and always None, engine.rs:442; SURVEY row f-4 asks for a public
    // one): on_chunk receives every decoded chunk (4 frames = 7680 samples, fewer for the tail) as soon as the codec has produced it.
    using ChunkFn = std::function<void(const float* pcm, size_t n_samples)>;
    AudioSample generate_with_voice_ids_stream(const std::vector<int32_t>& text_ids, const VoiceFile& voice, const ChunkFn& on_chunk,
                                               const std::vector<int32_t>* instruct_ids = nullptr, const std::vector<int32_t>* ref_text_ids = nullptr,
                                               std::vector<int32_t>* codes_out = nullptr);
    // [EXT] decoding given frames (q3tts_submit_decode): the audio of codes [n][16] the caller holds -- a cached utterance, the winner of a
    // codes-only candidate set -- on the engine's own codec.  Throws with the engine's reason when the frames are refused.
    AudioSample vocode(const std::vector<int32_t>& codes);
    // create_voice_file -- :324-387.  The two encoders are ONNX graphs run by the engine's own graph executor (q3tts_onnx_session_*, rows a17 /
    // f-2): <model_dir>/onnx/qwen3_tts_codec_encoder.onnx ("input_values" [1, T] -> "audio_codes") and qwen3_tts_speaker_encoder.onnx ("mels"
    // [1, n, 128] from q3tts_mel -> "spk_emb"), loaded when the files exist (engine.rs:106-127); without them the reference's errors are returned.
    VoiceFile create_voice_file(const std::string& audio_path, const std::string& ref_text);
    // [EXT] reference audio intake (q3tts_wav_intake): -1 = off, the default and the reference's behaviour -- create_voice_file refuses anything
    // but 24000 Hz and generate reads every file as 24000 Hz mono s16.  Q3_INTAKE_FIRST or Q3_INTAKE_MEAN: both read the WAV at any accepted
    // rate, sample format and channel count, resampled to 24000 Hz on the device, and generate keeps its cache in "<stem>.intake.cache", so a
    // ".cache" written from a misread clip is never picked up.  Throws for any other mode
    void set_reference_intake(int mode);
    int reference_intake() const { return intake_; }
    bool has_encoders() const { return enc_ && spk_; }
    std::vector<int64_t> encode_audio(const std::vector<float>& audio) const;       // AudioEncoder::encode, onnx.rs:97-121
    std::vector<float> encode_speaker(const std::vector<float>& audio) const;       // SpeakerEncoder::encode, onnx.rs:140-163
private:
    TtsEngine() = default;
    int build_prompt(const std::vector<int32_t>& text_ids, const VoiceFile& voice, const std::vector<int32_t>* ins, const std::vector<int32_t>* ref_text_ids,
                     std::vector<float>& prompt) const;
    void fill_request(q3tts_request& r, const std::vector<float>& prompt, int n) const;
    q3tts_engine* e_ = nullptr;
    q3tts_onnx_session *enc_ = nullptr, *spk_ = nullptr;
    Tokenizer tok_;
    std::map<std::string, VoiceFile> speakers_;
    size_t max_steps_ = 512;
    SamplerConfig sampler_;
    int intake_ = -1;
    std::vector<float> read_reference(const std::string& path) const;   // the intake's mono 24000 Hz samples of a WAV file (intake_ >= 0)
};

} // namespace q3tts
