// What the tracker (track.hip) and the smoother (smooth.hip) share: the key label order, the major scale, a recording's window count.
#pragma once

namespace {

constexpr int kKeys = 24;             // the 24-way label order: 0-11 minor, 12-23 major, tonic = id mod 12
constexpr unsigned kMajorScale = 0xAB5;   // bit d set: d semitones above the major tonic is in the scale {0,2,4,5,7,9,11}

// the windows of recording r that count: counts[r] clamped into 0..W (counts null: all W)
__device__ __forceinline__ int clamped_count(const int* counts, int r, int W) {
    const int n = counts ? counts[r] : W;
    return n < 0 ? 0 : n > W ? W : n;
}

}  // namespace
