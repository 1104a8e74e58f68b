// Shared flag parsing of the MI355X CLIs. The flag set, defaults and help text follow the
// reference tools (main.cpp:24-89, examples/stream-benchmark.cpp:20-83,
// examples/stream-compare.cpp:27-98).
#pragma once

#include <cstdio>
#include <cstdlib>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>

#include "test-to-speech.h"

struct CliArgs {
    std::string model_path, codec_path, voice_path, prompt;
    std::string output_path = "output.wav";
    std::string out_offline = "offline.wav", out_stream = "stream_concat.wav";
    std::string batch_file;  // miotts --batch: one prompt per line
    int gpus = 1;            // miotts --gpus: MI355Xs the batch is sharded over
    float temperature = 0.8f;
    int max_tokens = 700, n_threads = 4, n_gpu_layers = 0, device = -1;
    size_t chunk_samples = 4096;
    bool skip_llm = false, dump_tensors = false, speech_only = false, ignore_eos = false;
    // the on-device sampler chain (TestToSpeech::Options; neutral by default)
    int top_k = 0, repeat_last_n = 64;
    float top_p = 1.0f, min_p = 0.0f, repeat_penalty = 1.0f, frequency_penalty = 0.0f, presence_penalty = 0.0f;
};

// The whole of v as a number (std::stof / std::stoi alone accept "0.9x"); throws as they do.
inline float cli_float(const std::string &v) {
    size_t n = 0;
    const float f = std::stof(v, &n);
    if (n != v.size()) throw std::invalid_argument(v);
    return f;
}
inline int cli_int(const std::string &v) {
    size_t n = 0;
    const int i = std::stoi(v, &n);
    if (n != v.size()) throw std::invalid_argument(v);
    return i;
}

struct CliFlag {
    std::vector<std::string> names;
    bool takes_value;
    const char *help;
    std::function<void(CliArgs &, const std::string &)> set;
};

inline std::vector<CliFlag> cli_common_flags() {
    return {
        {{"-m", "--model"}, true, "MioTTS LLM GGUF model path (required unless --skip-llm)",
         [](CliArgs &a, const std::string &v) { a.model_path = v; }},
        {{"-c", "--codec"}, true, "MioCodec GGUF model path (required)",
         [](CliArgs &a, const std::string &v) { a.codec_path = v; }},
        {{"-v", "--voice"}, true, "Voice embedding .emb.gguf path (required)",
         [](CliArgs &a, const std::string &v) { a.voice_path = v; }},
        {{"-p", "--prompt"}, true, "Text to synthesize (required)",
         [](CliArgs &a, const std::string &v) { a.prompt = v; }},
        {{"-t", "--temp"}, true, "Sampling temperature (default: 0.8)",
         [](CliArgs &a, const std::string &v) { a.temperature = std::stof(v); }},
        {{"--max-tokens"}, true, "Max tokens to generate (default: 700)",
         [](CliArgs &a, const std::string &v) { a.max_tokens = std::stoi(v); }},
        {{"--threads"}, true, "Number of CPU threads (default: 4; accepted, unused: the path runs on the GPU)",
         [](CliArgs &a, const std::string &v) { a.n_threads = std::stoi(v); }},
        {{"-ngl"}, true, "Number of GPU layers (default: 0; accepted, unused: every layer runs on the GPU)",
         [](CliArgs &a, const std::string &v) { a.n_gpu_layers = std::stoi(v); }},
        {{"--device"}, true, "MI355X index (default: MIO_DEVICE, else LOCAL_RANK, else 0)",
         [](CliArgs &a, const std::string &v) { a.device = std::stoi(v); }},
        {{"--skip-llm"}, false, "Treat --prompt as raw <|s_N|> token text",
         [](CliArgs &a, const std::string &) { a.skip_llm = true; }},
        {{"--speech-only"}, false, "Benchmark harness: sample only the <|s_N|> speech ids",
         [](CliArgs &a, const std::string &) { a.speech_only = true; }},
        {{"--ignore-eos"}, false, "Benchmark harness: do not stop at <|endoftext|> / <|im_end|>",
         [](CliArgs &a, const std::string &) { a.ignore_eos = true; }},
        {{"--top-k"}, true, "Sample among the k most likely ids (default: 0 = off)",
         [](CliArgs &a, const std::string &v) { a.top_k = cli_int(v); }},
        {{"--top-p"}, true, "Sample among the most likely ids that reach this probability mass (default: 1 = off)",
         [](CliArgs &a, const std::string &v) { a.top_p = cli_float(v); }},
        {{"--min-p"}, true, "Drop ids less likely than this fraction of the most likely one (default: 0 = off)",
         [](CliArgs &a, const std::string &v) { a.min_p = cli_float(v); }},
        {{"--repeat-penalty"}, true, "Penalty on the logits of recently sampled ids (default: 1 = off)",
         [](CliArgs &a, const std::string &v) { a.repeat_penalty = cli_float(v); }},
        {{"--repeat-last-n"}, true, "Sampled tokens the penalties look back on, 0..256 (default: 64)",
         [](CliArgs &a, const std::string &v) { a.repeat_last_n = cli_int(v); }},
        {{"--frequency-penalty"}, true, "Subtracted per recent occurrence of an id (default: 0 = off)",
         [](CliArgs &a, const std::string &v) { a.frequency_penalty = cli_float(v); }},
        {{"--presence-penalty"}, true, "Subtracted once from a recently sampled id (default: 0 = off)",
         [](CliArgs &a, const std::string &v) { a.presence_penalty = cli_float(v); }},
    };
}

inline void cli_usage(const char *prog, const char *what, const std::vector<CliFlag> &flags) {
    std::fprintf(stderr, "Usage: %s [options]\n\n%s%sOptions:\n", prog, what, *what ? "\n\n" : "");
    for (const CliFlag &f : flags) {
        std::string n;
        for (const std::string &s : f.names) n += (n.empty() ? "" : ", ") + s;
        if (f.takes_value) n += f.names.back() == "-ngl" || f.names.back().rfind("--", 0) != 0 ? " N" : " VALUE";
        std::fprintf(stderr, "  %-24s %s\n", n.c_str(), f.help);
    }
    std::fprintf(stderr, "  %-24s %s\n\n", "-h, --help", "Show this help");
}

// false on an unknown flag or a missing value (the reference prints usage and exits 1)
inline bool cli_parse(int argc, char **argv, const std::vector<CliFlag> &flags, CliArgs &a, const char *what) {
    for (int i = 1; i < argc; ++i) {
        const std::string arg = argv[i];
        if (arg == "-h" || arg == "--help") {
            cli_usage(argv[0], what, flags);
            std::exit(0);
        }
        const CliFlag *hit = nullptr;
        for (const CliFlag &f : flags)
            for (const std::string &n : f.names)
                if (n == arg) hit = &f;
        if (!hit) {
            std::fprintf(stderr, "Unknown argument: %s\n", arg.c_str());
            return false;
        }
        if (hit->takes_value && ++i >= argc) return false;
        try {
            hit->set(a, hit->takes_value ? std::string(argv[i]) : std::string());
        } catch (const std::exception &) {  // std::stof / std::stoi: not a number, or out of range
            std::fprintf(stderr, "Invalid value for %s: %s\n", arg.c_str(), argv[i]);
            return false;
        }
    }
    return true;
}

// the reference tools' required-argument checks; returns an error text or empty.
// path_words: main.cpp:109-121 says "--codec path is required" where the examples
// (stream-benchmark.cpp:93-105, stream-compare.cpp:174-186) say "--codec is required".
inline std::string cli_check(const CliArgs &a, bool path_words = false) {
    const std::string p = path_words ? " path" : "";
    if (a.prompt.empty()) return "--prompt is required";
    if (a.codec_path.empty()) return "--codec" + p + " is required";
    if (a.voice_path.empty()) return "--voice" + p + " is required";
    if (!a.skip_llm && a.model_path.empty()) return "--model" + p + " is required (or use --skip-llm)";
    // what the runner would refuse (mio_hip_llm_set_sampling), said before any model is loaded
    for (float v : {a.top_p, a.min_p, a.repeat_penalty, a.frequency_penalty, a.presence_penalty})
        if (v != v) return "a sampling option is NaN";
    if (!(a.repeat_penalty > 0.0f)) return "--repeat-penalty must be > 0";
    if (a.repeat_last_n < 0 || a.repeat_last_n > 256) return "--repeat-last-n must be in 0..256";
    return "";
}

inline TestToSpeech::Config cli_config(const CliArgs &a) {
    TestToSpeech::Config c;
    c.model_path = a.model_path;
    c.codec_path = a.codec_path;
    c.n_threads = a.n_threads;
    c.n_gpu_layers = a.n_gpu_layers;
    c.temperature = a.temperature;
    c.max_tokens = a.max_tokens;
    c.device = a.device;
    return c;
}

inline TestToSpeech::Options cli_options(const CliArgs &a) {
    TestToSpeech::Options o;
    o.temperature = a.temperature;
    o.max_tokens = a.max_tokens;
    o.skip_llm = a.skip_llm;
    o.speech_only = a.speech_only;
    o.ignore_eos = a.ignore_eos;
    o.top_k = a.top_k, o.top_p = a.top_p, o.min_p = a.min_p;
    o.repeat_penalty = a.repeat_penalty, o.repeat_last_n = a.repeat_last_n;
    o.frequency_penalty = a.frequency_penalty, o.presence_penalty = a.presence_penalty;
    return o;
}
