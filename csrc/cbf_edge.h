// CBF edge helpers shared by cbf.hip (training kernels) and refine.hip (safety filter): the
// layer-1 feature fragment of one edge, the per-edge context and the sizes of the weight images.
// Included inside a translation unit compiled per MFMA precision (csrc/prec.h).
#pragma once
#include "common.h"
#include "state.h"

namespace mb {
namespace MB_PREC {

constexpr int CBF_FWD_FRAGS = 34;  // w1f 2 + w2 16 + w3 16
constexpr int CBF_VEC = 260;       // b2 128 | b3 64 | w4 64 | b4 1 (+3 pad)



// Layer-1 B fragment of one edge (K slots: see layout.cbf_w1_slot): fp32 features split into
// h16 hi (lanes h = 0) and residual lo (lanes h = 1) parts.
template <int D>
DEV h16x8 cbf_edge_frag(const float (&rp)[D], const float (&rv)[D], float eye, float dfeat, bool ok, int h) {
  h16x8 f;
  const h16 z = (h16)0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = z;
  if (!ok) return f;
  h16 hi[2 * D + 1], lo[2 * D + 1];
#pragma unroll
  for (int q = 0; q < D; ++q) {
    split_h16(rp[q], hi[q], lo[q]);
    split_h16(rv[q], hi[D + q], lo[D + q]);
  }
  split_h16(dfeat, hi[2 * D], lo[2 * D]);
  if constexpr (D == 2) {
    if (h == 0) {
      f[0] = hi[0]; f[1] = hi[1]; f[2] = hi[2]; f[3] = hi[3]; f[4] = (h16)eye; f[5] = hi[4]; f[6] = (h16)1.f;
    } else {
      f[0] = lo[0]; f[1] = lo[1]; f[2] = lo[2]; f[3] = lo[3]; f[5] = lo[4];
    }
  } else {
    if (h == 0) {
#pragma unroll
      for (int q = 0; q < 7; ++q) f[q] = hi[q];
      f[7] = (h16)1.f;
    } else {
#pragma unroll
      for (int q = 0; q < 7; ++q) f[q] = lo[q];
      f[7] = (h16)eye;
    }
  }
  return f;
}

template <int D>
struct EdgeCtx {
  bool ok;
  int b, t, i, j;
  float rp[D], rv[D];     // s_i - s_j: positions, velocities
  float eye, d, dfeat;
  bool mask;
};

// LDS row strides (h16 elements) of the row-major W2 [128][WS2], W3 [64][WS3] images (see the bank
// model note at the stage strides in cbf.hip)
constexpr int WS2 = 68, WS3 = 148;
constexpr int RM_W2 = 128 * WS2, RM_W3 = 64 * WS3;  // row-major image sizes (elements)
constexpr int RM_LO = RM_W2 + RM_W3;                // lo plane offset of the images (x3)
constexpr int RMP = (X3 ? 2 : 1) * RM_LO;           // elements of the W2|W3 (+ lo) images

}  // namespace MB_PREC
}  // namespace mb
