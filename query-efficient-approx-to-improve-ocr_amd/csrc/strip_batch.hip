// Minibatch assembly from the device-resident strip store (include/qea_hip.h: qea_strip_batch; datasets/resident.py).
//
// The store keeps every strip of a dataset as 8-bit grey, row-major, packed back to back (strip s: h[s] x w[s] bytes at
// pixels + offset[s]).  One launch writes the whole fp32 batch out[B][OH][OW]: strip idx[b] placed on white (1.0), every byte sent
// through the caller's 256-entry table (p / 255 as the HOST rounds it, so the device compiler's lowering of a division never enters).
//
// strip_batch_kernel: the window gather (csrc/window_gather.h: lanes, reads, store and the bad-table rule) of strip idx[b], centred or
// left-anchored in OH x OW and clipped to it.
#include "window_gather.h"

namespace {

__global__ __launch_bounds__(WG_THREADS) void strip_batch_kernel(const uint8_t* __restrict__ pixels, const int64_t* __restrict__ offset,
                                                                 const int32_t* __restrict__ h, const int32_t* __restrict__ w, int n,
                                                                 const int64_t* __restrict__ idx, int B, int OH, int OW, int anchor,
                                                                 const float* __restrict__ table, float* __restrict__ out) {
  window_gather(pixels, table, out, B, OH, OW, [=](int b) {
    Window win = {};
    const int64_t s = idx[b];
    if (s >= 0 && s < n) {                             // anything else: an all-white image
      const int sw = w[s];
      const int hh = min(max(h[s], 0), OH), ww = min(max(sw, 0), OW);      // the rectangle that is copied: clipped to the output
      const int top = (OH - hh) >> 1;
      const int left = anchor == QEA_STRIP_ANCHOR_LEFT ? 0 : (OW - ww) >> 1;
      win = {offset[s] - ((long long)top * sw + left), sw, left, top, left + ww, top + hh};   // rows 0..hh-1, columns 0..ww-1 of the strip
    }
    return win;
  });
}

}  // namespace

extern "C" int qea_strip_batch(const uint8_t* pixels, const int64_t* offset, const int32_t* h, const int32_t* w, int32_t n,
                               const int64_t* idx, int32_t B, int32_t OH, int32_t OW, int32_t anchor, const float* table, float* out,
                               void* stream) {
  QEA_REQUIRE(pixels && offset && h && w && idx && table && out, "qea_strip_batch: null pointer");
  QEA_REQUIRE(n >= 1, "qea_strip_batch: n=%d strips in the store", n);
  QEA_REQUIRE(B >= 1 && B <= (1 << 24), "qea_strip_batch: B=%d outside 1..2^24", B);
  QEA_REQUIRE(OH >= 1 && OH <= 4096, "qea_strip_batch: OH=%d outside 1..4096", OH);
  QEA_REQUIRE(OW >= 4 && OW <= 16384 && OW % 4 == 0, "qea_strip_batch: OW=%d must be a multiple of 4 in 4..16384", OW);
  QEA_REQUIRE(anchor == QEA_STRIP_ANCHOR_CENTRE || anchor == QEA_STRIP_ANCHOR_LEFT, "qea_strip_batch: unknown anchor %d", anchor);
  QEA_REQUIRE(((uintptr_t)out & 15) == 0, "qea_strip_batch: out must be 16-byte aligned");
  launch_over_quads(strip_batch_kernel, B, OH, OW, stream, pixels, offset, h, w, n, idx, B, OH, OW, anchor, table, out);
  QEA_CHECK_LAUNCH();
  return QEA_OK;
}
