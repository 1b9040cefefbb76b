// Minibatch assembly from the device-resident strip store (include/qea_hip.h: qea_strip_batch; datasets/resident.py).
//
// The store keeps every strip of a dataset as 8-bit grey, row-major, packed back to back (strip s: h[s] x w[s] bytes at
// pixels + offset[s]).  One launch writes the whole fp32 batch out[B][OH][OW]: strip idx[b] placed on white (1.0), every byte sent
// through the caller's 256-entry table (p / 255 as the HOST rounds it, so the device compiler's lowering of a division never enters).
//
// strip_batch_kernel: one lane per four neighbouring output pixels of a row (OW % 4 == 0), one 16-byte store per lane, the lanes of
// a wave on consecutive quads: a wave writes 1 KB contiguously.  grid.x walks the OH * OW / 4 quads of an image, grid.y the images
// (an image per workgroup row, so the strip's words are uniform and the index arithmetic is 32-bit); no output address is visited
// twice and no input byte is shared beyond a cache line, so there is nothing to keep in LDS.  The four source bytes of a
// quad are read one by one, each only when its pixel lies inside the strip's clipped rectangle: strips start at any byte and are
// centred at any column, so a dword read would be unaligned for most quads; the bytes of a wave's quads are neighbours in one or
// two cache lines.
#include "common.h"

namespace {

constexpr int SB_THREADS = 256;

__global__ __launch_bounds__(SB_THREADS) void strip_batch_kernel(const uint8_t* __restrict__ pixels, const int64_t* __restrict__ offset,
                                                                 const int32_t* __restrict__ h, const int32_t* __restrict__ w, int n,
                                                                 const int64_t* __restrict__ idx, int B, int OH, int OW, int anchor,
                                                                 const float* __restrict__ table, float* __restrict__ out) {
  const int qw = OW >> 2;                              // quads per row
  const int q = blockIdx.x * SB_THREADS + threadIdx.x; // quad of the image, row-major
  if (q >= OH * qw) return;
  const int y = q / qw, x0 = (q - y * qw) << 2;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {    // uniform over the workgroup: the strip's words are scalar loads
    f32x4 v = {1.f, 1.f, 1.f, 1.f};
    const int64_t s = idx[b];
    if (s >= 0 && s < n) {                             // anything else: an all-white image
      const int sh = h[s], sw = w[s];
      const int hh = min(max(sh, 0), OH), ww = min(max(sw, 0), OW);        // the rectangle that is copied: clipped to the output
      const int top = (OH - hh) >> 1;
      const int left = anchor == QEA_STRIP_ANCHOR_LEFT ? 0 : (OW - ww) >> 1;
      const int sy = y - top;
      if (sy >= 0 && sy < hh) {
        const uint8_t* src = pixels + offset[s] + (long long)sy * sw;       // row sy of the strip; columns 0..ww-1 are read
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int sx = x0 + k - left;
          if (sx >= 0 && sx < ww) v[k] = table[src[sx]];
        }
      }
    }
    *reinterpret_cast<f32x4*>(out + (((size_t)b * OH * qw + q) << 2)) = v;
  }
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
  const dim3 grid(qea_cdiv((long long)OH * (OW / 4), SB_THREADS), B < 65535 ? B : 65535);   // OH * OW / 4 <= 2^24 quads per image
  hipLaunchKernelGGL(strip_batch_kernel, grid, dim3(SB_THREADS), 0, (hipStream_t)stream, pixels, offset, h, w, n, idx, B, OH, OW, anchor,
                     table, out);
  QEA_CHECK_LAUNCH();
  return QEA_OK;
}
