// The packed page store shared by csrc/page_tiles.hip and csrc/binarize.hip: pages of any sizes back to back, row-major without padding;
// page p is h[p] rows of w[p] elements at element offset[p] of the store (8-bit grey, so pages start at any byte, or fp32).
#pragma once
#include "common.h"

namespace {

struct Page {
  long long off;
  int h, w;     // 0 x 0: no such page
};

// A page that does not lie inside the store (offset < 0 or offset + h * w > store_elems) reads as "no such page": a bad table never
// becomes an access outside the caller's buffers.
__device__ __forceinline__ Page page_of(int p, const int64_t* __restrict__ offset, const int32_t* __restrict__ h, const int32_t* __restrict__ w,
                                        int n_pages, long long store_elems) {
  Page g = {0, 0, 0};
  if (p >= 0 && p < n_pages) {
    const long long off = offset[p];
    const int ph = h[p], pw = w[p];
    if (off >= 0 && ph > 0 && pw > 0 && off <= store_elems && (long long)ph * pw <= store_elems - off) {
      g.off = off;
      g.h = ph;
      g.w = pw;
    }
  }
  return g;
}

// The 8-bit rule of the project (qea/pages.py: quantise_u8): (uint8)(min(max(x, 0), 1) * 255.0f), NaN -> 0
__device__ __forceinline__ uint8_t to_u8(float x) {
  const float c = fminf(fmaxf(x, 0.f), 1.f);           // fmaxf(NaN, 0) = 0
  return (uint8_t)(int)__fmul_rn(c, 255.0f);           // one fp32 multiply, then truncation
}

}  // namespace
