// A caller of the drop-in C++ surface as an earlier version of include/test-to-speech.h shaped it:
// tests/test_old_options_gpu.py compiles this file against a copy of the header WITHOUT the
// chain's fields and the ABI tag of TestToSpeech::Options (12 bytes) and links it to the current
// library, where it binds to the untagged entry points.
// The bytes that follow the Options object are set to argv[6] (0: zeros, as the StreamProfile a
// benchmark keeps beside its Options; 255: ones), which the library must not take for settings.
//   old_options_caller MODEL CODEC VOICE TEXT OUT.wav FILL
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "test-to-speech.h"

int main(int argc, char **argv) {
    if (argc != 7) return 2;
    static_assert(sizeof(TestToSpeech::Options) == 12, "build against the header without the extension");
    TestToSpeech::Config cfg;
    cfg.model_path = argv[1];
    cfg.codec_path = argv[2];
    TestToSpeech tts(cfg);
    VoiceModel voice;
    if (!tts.is_ready() || !voice.load_from_file(argv[3])) return 1;
    struct {
        TestToSpeech::Options opt;
        unsigned char after[64];
    } s;
    std::memset(s.after, std::atoi(argv[6]), sizeof(s.after));
    s.opt.max_tokens = 40;
    s.opt.speech_only = true;
    s.opt.ignore_eos = true;
    if (!tts.synthesize_to_file(voice, argv[4], argv[5], s.opt)) {
        std::fprintf(stderr, "old_options_caller: synthesis failed\n");
        return 1;
    }
    return 0;
}
