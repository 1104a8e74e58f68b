"""The pitch resampler's design quality, on the float64 definition alone (tests/np_pitch.py): a sine
at 0.45 of the Nyquist frequency through the resampler, the wanted tone (at r times the frequency)
against everything else in the output. The figures are quoted in DESIGN 4 ("Pitch")."""
import numpy as np
import pytest

import np_pitch as ref


@pytest.mark.parametrize("semitones", [-12, -1, 1, 12])
def test_tone_to_rest(semitones):
    r = float(np.float32(2.0 ** (semitones / 12.0)))
    w = 2 * np.pi * 0.225  # 0.45 of Nyquist, in radians per sample
    y = ref.pitch(np.sin(w * np.arange(8192)), r)[0][128:-128]  # away from the zeros outside the signal
    j = np.arange(128, 128 + y.size)
    basis = np.stack([np.cos(w * r * j), np.sin(w * r * j)], 1)
    rest = y - basis @ np.linalg.lstsq(basis, y, rcond=None)[0]
    db = 10 * np.log10((y @ y - rest @ rest) / (rest @ rest))
    print(f"{semitones:+d} semitones: tone to rest {db:.1f} dB")
    assert db > 60.0
