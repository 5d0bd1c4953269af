// Internal: what the uint8 augmentation kernels share (augment_affine.hip, augment_elastic.hip): the tile shape, the output descriptors,
// the mean luma from the luma kernel's sum and the gather of one tap pair's bytes.
#pragma once
#include "ctx.h"

namespace mgu {

constexpr int AFF_MAX_SIDE = 8192;
constexpr int AFF_XV = 4;                 // consecutive output x per thread (one 16-byte store per channel on the vector path)
constexpr int AFF_TX = 32, AFF_TY = 32;   // workgroup tile: 8 threads x 4 pixels across, 32 rows (256 threads); see augment.hip

struct AffStrides {
  int64_t b, c, h, w;
};
struct AffNorm {
  float m0, m1, m2, s0, s1, s2;
};

// m = (S + n / 2) / n for S <= 65280 n, n <= 2^26: the double quotient is within one of the integer quotient, then corrected exactly
__device__ __forceinline__ int aff_mean_q8(unsigned long long S, int n) {
  const long long a = (long long)S + n / 2;
  long long q = (long long)((double)a / (double)n);
  const long long r = a - q * n;
  if (r < 0) --q;
  else if (r >= n) ++q;
  return (int)q;
}

struct AffWords {
  unsigned a, b, c;
};
// The six bytes at p (taps (ix, iy) and (ix + 1, iy), three channels each; in0 / in1: the tap lies inside the image) -> r0 = bytes 0..3,
// r1 = bytes 4, 5.  One 12-byte load at the 4-byte aligned address below p where that window lies inside the batch [lo, hi) -- bytes of
// a tap outside the image are then whatever follows in the batch, and the caller replaces them by the fill.  Where the window leaves the
// batch (its first and last bytes) or no tap lies inside, the load goes to `safe` (12 readable bytes: the parameter table) and the taps
// inside are read byte by byte.  Twelve byte gathers per pixel kept the kernel at the rate of the address unit; two wide ones do not.
__device__ __forceinline__ void aff_load_run(const uint8_t* p, const uint8_t* lo, const uint8_t* hi, const uint8_t* safe, bool in0, bool in1,
                                             unsigned& r0, unsigned& r1) {
  const unsigned s = (unsigned)((uintptr_t)p & 3);
  const uint8_t* q = p - s;
  const bool any = in0 || in1, wide = any && q >= lo && q + 12 <= hi;
  const AffWords w = *(const AffWords*)(wide ? q : safe);
  r0 = __builtin_amdgcn_alignbyte(w.b, w.a, s);
  r1 = __builtin_amdgcn_alignbyte(w.c, w.b, s);
  if (__builtin_expect(any && !wide, 0)) {
    r0 = r1 = 0;
    if (in0) r0 = (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16);
    if (in1) r0 |= (unsigned)p[3] << 24, r1 = (unsigned)p[4] | ((unsigned)p[5] << 8);
  }
}

}  // namespace mgu
