// mel.h -- the host-only half of the log-mel front end (mel.hip): the frame count and the two tables.
#pragma once

namespace q3 {

constexpr int MEL_N_FFT = 1024, MEL_HOP = 256, MEL_N_MELS = 128, MEL_N_BINS = MEL_N_FFT / 2 + 1, MEL_PAD = (MEL_N_FFT - MEL_HOP) / 2;

// Frames mel_device writes for n samples: the padded clip has n + 768 samples, frame f covers [256 f, 256 f + 1024), and a frame that
// does not fit is dropped (the reference's `break`), so 0 for n < 256 and n / 256 from there on.
inline int mel_frames(int n) {
    if (n < 0) return 0;
    const long plen = (long)n + 2 * MEL_PAD;
    long f = (plen > MEL_N_FFT ? plen - MEL_N_FFT : 0) / MEL_HOP + 1;
    while (f > 0 && (f - 1) * MEL_HOP + MEL_N_FFT > plen) f--;
    return (int)f;
}

// periodic Hann hann[1024] and the Slaney filterbank fb[128][513], in f32 as the kernel reads them (defined in mel.hip)
void mel_tables(float* hann, float* fb);

} // namespace q3
