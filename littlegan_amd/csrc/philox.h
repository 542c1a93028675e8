// The counter-based generator every draw of the project comes from: Philox4x32-10 (Salmon et al., SC'11), one 128-bit block per
// (counter, key).  Shared by the input side (augment_core.h: noise, augmentation draws) and the dropout masks regenerated inside the
// norm passes (norm.hip); oracle/input_oracle.py restates it in numpy.
#pragma once
#include "lg_common.h"

namespace {

struct u4 { unsigned x, y, z, w; };

__device__ __forceinline__ u4 philox4x32_10(u4 c, unsigned k0, unsigned k1) {
  constexpr unsigned M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(M0, c.x), lo0 = M0 * c.x;
    const unsigned hi1 = __umulhi(M1, c.z), lo1 = M1 * c.z;
    c = u4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
    k0 += W0; k1 += W1;
  }
  return c;
}

}  // namespace
