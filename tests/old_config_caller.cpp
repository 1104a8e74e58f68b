// A caller compiled against include/test-to-speech.h as it was before Config::output_sample_rate:
// Config then ended in four bytes of padding, set here to argv[5] (0 or 255) before the Config is
// constructed in them. It binds to the library's untagged constructor, which must read no rate there.
//   old_config_caller CODEC VOICE TOKEN_TEXT OUT.wav FILL
#include <cstdlib>
#include <cstring>
#include <new>

#include "test-to-speech.h"

int main(int argc, char **argv) {
    if (argc != 6) return 2;
    alignas(TestToSpeech::Config) static unsigned char raw[sizeof(TestToSpeech::Config)];
    std::memset(raw, std::atoi(argv[5]), sizeof(raw));
    TestToSpeech::Config *cfg = new (raw) TestToSpeech::Config;
    cfg->codec_path = argv[1];
    TestToSpeech tts(*cfg);
    VoiceModel voice;
    TestToSpeech::Options opt;
    opt.skip_llm = true;
    return tts.is_ready() && tts.sample_rate() == 44100 && voice.load_from_file(argv[2]) &&
                   tts.synthesize_to_file(voice, argv[3], argv[4], opt) ? 0 : 1;
}
