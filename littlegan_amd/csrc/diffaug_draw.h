// The record of one row of a diff_augment call slot, shared by lg_diffaug_draw (diffaug.hip) and the gated draw of the
// adaptive augmentation probability (ada.hip): both write what diffaug_record returns, the second under a policy that the
// row's own gate words have narrowed.
#pragma once
#include "lg_common.h"
#include "philox.h"

namespace {

// first Philox block of row r of call slot `call` under key_offset: the record reads blocks ctr and ctr + 1 (third counter word 0)
__device__ __forceinline__ unsigned long long diffaug_row_ctr(unsigned long long key_offset, int call, int r) {
  return key_offset + ((((unsigned long long)call << 24) + (unsigned long long)r) << 1);
}

// {p0, p1} = {b, s, c, ty | tx, cy, cx, cut}.  w_j = bits_j >> 8 (24 bits), u_j = w_j 2^-24:
//   b = u0 - 0.5, s = 2 u1, c = u2 + 0.5, ty = (w3 (2M+1) >> 24) - M, tx from w4, cy = w5 (S+1 - cut%2) >> 24, cx from w6; M = S/8, cut = S/2.
// The integers come from integer arithmetic: u n in fp32 can round up to n.  policy: 1 color, 2 translation, 4 cutout; a component
// that is not named gets its identity values.
__device__ __forceinline__ void diffaug_record(unsigned long long seed, unsigned long long ctr, int S, int policy, f32x4& p0, f32x4& p1) {
  const u4 A = philox4x32_10(u4{(unsigned)ctr, (unsigned)(ctr >> 32), 0u, 0u}, (unsigned)seed, (unsigned)(seed >> 32));
  const u4 C = philox4x32_10(u4{(unsigned)(ctr + 1), (unsigned)((ctr + 1) >> 32), 0u, 0u}, (unsigned)seed, (unsigned)(seed >> 32));
  const float k24 = 1.0f / 16777216.0f;
  const int M = S / 8, cut = S / 2;
  const bool color = policy & 1, trans = policy & 2, cutout = policy & 4;
  p0[0] = color ? (float)(A.x >> 8) * k24 - 0.5f : 0.f;
  p0[1] = color ? 2.0f * ((float)(A.y >> 8) * k24) : 1.f;
  p0[2] = color ? (float)(A.z >> 8) * k24 + 0.5f : 1.f;
  p0[3] = trans ? (float)((int)(((unsigned long long)(A.w >> 8) * (unsigned)(2 * M + 1)) >> 24) - M) : 0.f;
  p1[0] = trans ? (float)((int)(((unsigned long long)(C.x >> 8) * (unsigned)(2 * M + 1)) >> 24) - M) : 0.f;
  p1[1] = cutout ? (float)(int)(((unsigned long long)(C.y >> 8) * (unsigned)(S + 1 - cut % 2)) >> 24) : 0.f;
  p1[2] = cutout ? (float)(int)(((unsigned long long)(C.z >> 8) * (unsigned)(S + 1 - cut % 2)) >> 24) : 0.f;
  p1[3] = cutout ? (float)cut : 0.f;
}

}  // namespace
