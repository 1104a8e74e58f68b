// Internal parity hooks of the codec (csrc/host/codec.cpp) for the test library.
#pragma once

#include <cstddef>
#include <cstdint>

struct mio_hip_codec;

namespace mio {

// mio_hip_codec_decode_stage for a packed batch: runs the packed decode of B utterances (host
// codes, one embedding each) up to `stage`, copies the packed activation [rows][cols] to `out`
// (room for out_cap floats; refused, with nothing written, when rows * cols is more) and the
// B + 1 row offsets of the utterances at that stage to seg_off.
int codec_decode_stage_packed(mio_hip_codec *c, const int32_t *const *codes, const int *n_codes, int B,
                              const float *const *embs, int stage, float *out, size_t out_cap, int *rows, int *cols,
                              int *seg_off);

}  // namespace mio
