// Drop-in for the reference test-to-speech.h (test-to-speech.h:11-123): the same classes,
// nested types, defaults and member functions, so callers (main.cpp, the stream examples,
// stream-to-device) compile unchanged. The implementation (csrc/host/tts.cpp) runs the
// whole path on one MI355X: GGUF tokenizer on the host, the LLM decode step as one
// hipGraph per token with on-device sampling, the MioCodec decoder and the fused iSTFT.
// Config::n_threads / n_gpu_layers are accepted and ignored (everything runs on the GPU);
// Config::device (extension, default -1) picks the GPU (-1: MIO_DEVICE, else LOCAL_RANK,
// else 0).
#pragma once

#include <cstddef>
#include <functional>
#include <memory>
#include <string>
#include <vector>

class istft_cache;

class VoiceModel {
public:
    VoiceModel() = default;

    bool load_from_file(const std::string & path);
    bool is_ready() const;

    const std::vector<float> & embedding() const;
    const std::string & path() const;

private:
    std::string path_;
    std::vector<float> embedding_;
};

class TestToSpeech {
public:
    struct StreamProfile {
        double total_sec = 0.0;
        double llm_sec = 0.0;
        double codec_sec = 0.0;
        double istft_sec = 0.0;
        double callback_sec = 0.0;
        int llm_tokens = 0;
        int decode_calls = 0;
        size_t decoded_codes = 0;
        size_t emitted_samples = 0;
        // (extension) codes whose prenet rows a re-decode took from the previous decode
        // (MIO_CODEC_INCREMENTAL) instead of recomputing them
        size_t prenet_rows_reused = 0;
    };

    // output_sample_rate took the four bytes that were padding at the end of Config, so the size
    // and every earlier offset are unchanged; a program compiled against the earlier header never
    // wrote those bytes. The tag puts the layout into the constructor's mangled name: such a
    // program keeps binding to the untagged constructor, which the library still exports and
    // which reads the rate as 0 (csrc/host/tts.cpp, "earlier entry points").
    struct [[gnu::__abi_tag__("cfg2")]] Config {
        std::string model_path;
        std::string codec_path;
        int n_threads = 4;
        int n_gpu_layers = 0;
        float temperature = 0.8f;
        int max_tokens = 700;
        int device = -1;  // extension: GPU index (-1 = MIO_DEVICE / LOCAL_RANK / 0)
        // extension: the rate of everything written or handed to a callback: 8000, 16000, 22050,
        // 24000, 32000 or 48000 Hz, resampled on the device in the PCM epilogue (mio_hip.h
        // "output rate"); 0 or the codec's own rate = as the codec produces it. Checked with the
        // models: any other rate leaves is_ready() false. sample_rate() reports the rate in use.
        int output_sample_rate = 0;
    };

    // The sampler chain's fields grew Options past the 12 bytes it had. The tag puts the layout
    // into the mangled name of every member function that takes an Options, so a program compiled
    // against this header binds to the entry points that read the new fields, and one compiled
    // against the earlier header keeps binding to the untagged ones, which the library still
    // exports and runs with the neutral values (csrc/host/tts.cpp, "earlier entry points").
    struct [[gnu::abi_tag("opt2")]] Options {
        float temperature = -1.0f; // negative => use Config default
        int max_tokens = -1;       // negative => use Config default
        bool skip_llm = false;     // when true, text is raw <|s_N|> token text
        bool apply_peak_normalization = true;
        // extensions for benchmark harnesses (flagged deviations): sample only the 12,800
        // speech ids / never stop at an end token
        bool speech_only = false;
        bool ignore_eos = false;
        // extensions: the on-device sampler chain (mio_hip.h mio_sampling: penalties -> top-k
        // -> top-p -> min-p before the temperature draw). These defaults are the neutral
        // values: the reference's temp + dist pair, unchanged.
        int top_k = 0;
        float top_p = 1.0f;
        float min_p = 0.0f;
        float repeat_penalty = 1.0f;
        int repeat_last_n = 64;
        float frequency_penalty = 0.0f;
        float presence_penalty = 0.0f;
    };

    using StreamCallback = std::function<bool(const float * samples,
                                              size_t n_samples,
                                              int sample_rate,
                                              bool is_last_chunk)>;

    explicit TestToSpeech(const Config & config);
    ~TestToSpeech();

    TestToSpeech(const TestToSpeech &) = delete;
    TestToSpeech & operator=(const TestToSpeech &) = delete;

    bool is_ready() const;
    int sample_rate() const;

    // (extension) speaking rate: the same voice and pitch, `speed` times as fast (0.5 .. 2.0;
    // default 1 = as generated), by WSOLA time-scale modification on the device between the iSTFT
    // and peak normalisation (mio_hip.h "speaking rate"). Applies to synthesize_to_file,
    // synthesize_to_vector and synthesize_batch_to_files from the next call on; the streaming
    // entry points refuse to run while the speed is not 1. false (and no change) for a value
    // outside the range, a NaN, or an instance without a device.
    bool set_speed(float speed);
    float speed() const;

    // (extension) pitch: the same words in the same time, `semitones` higher or lower (-12 .. 12;
    // default 0 = as generated): WSOLA at speed / 2^(semitones / 12), then an arbitrary-ratio sinc
    // resampler, on the device between the iSTFT and peak normalisation (mio_hip.h "pitch").
    // Formants move with the pitch, so it is meant for a few semitones. Same contract as
    // set_speed: applies to synthesize_to_file, synthesize_to_vector and synthesize_batch_to_files
    // from the next call on; the streaming entry points refuse to run while the pitch is not 0.
    // false (and no change) for a value outside the range, a NaN, an instance without a device,
    // or a combination with the current speed whose time-scale speed / 2^(semitones / 12) leaves
    // 0.5 .. 2.0 (set_speed refuses such a combination likewise).
    bool set_pitch(float semitones);
    float pitch() const;

    bool synthesize_to_file(const VoiceModel & voice,
                            const std::string & text,
                            const std::string & output_path,
                            const Options & options);
    bool synthesize_to_file(const VoiceModel & voice,
                            const std::string & text,
                            const std::string & output_path);

    bool synthesize_to_vector(const VoiceModel & voice,
                              const std::string & text,
                              std::vector<float> & out_audio,
                              const Options & options);
    bool synthesize_to_vector(const VoiceModel & voice,
                              const std::string & text,
                              std::vector<float> & out_audio);

    bool synthesize_stream(const VoiceModel & voice,
                           const std::string & text,
                           const StreamCallback & callback,
                           size_t chunk_samples,
                           const Options & options);
    bool synthesize_stream(const VoiceModel & voice,
                           const std::string & text,
                           const StreamCallback & callback,
                           size_t chunk_samples = 4096);
    bool synthesize_stream_profiled(const VoiceModel & voice,
                                    const std::string & text,
                                    const StreamCallback & callback,
                                    size_t chunk_samples,
                                    const Options & options,
                                    StreamProfile & profile);
    bool generate_token_text(const std::string & text,
                             const Options & options,
                             std::string & out_token_text);

    // (extension) several utterances on this device: their LLM decodes run together (one
    // weight pass per step for all of them, up to 16 at a time; mio_hip_llm_generate_queue: a
    // text starts as soon as an earlier one has ended), then each is written as synthesize_to_file writes it (the same bytes: every utterance
    // samples with the seed synthesize_to_file uses)
    bool synthesize_batch_to_files(const VoiceModel & voice,
                                   const std::vector<std::string> & texts,
                                   const std::vector<std::string> & output_paths,
                                   const Options & options);
    // (extension) the same with one voice per utterance (voices.size() == texts.size()): the
    // codec decodes each group of up to 16 utterances, whatever their lengths and voices, as one
    // packed decode (mio_hip_codec_decode_pcm_packed). Each file has the bytes synthesize_to_file
    // writes with that voice.
    bool synthesize_batch_to_files(const std::vector<VoiceModel> & voices,
                                   const std::vector<std::string> & texts,
                                   const std::vector<std::string> & output_paths,
                                   const Options & options);

    struct Impl;  // GPU handles (device, LLM runner, codec, tokenizer)

private:
    bool batch_to_files(const VoiceModel * voices, bool per_utterance,
                        const std::vector<std::string> & texts,
                        const std::vector<std::string> & output_paths,
                        const Options & options);
    Config config_;
    std::unique_ptr<Impl> impl_;
};
