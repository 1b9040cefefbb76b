// Word boxes of a group of pages cut into 32-row CRNN strips, bit for bit the statement tests/word_strips_spec.py (include/qea_hip.h:
// qea_word_strips; qea/reading.py is the product interface, whose host path is the same statement in numpy; DESIGN.md "Word strips").
//
// word_strips_kernel: out[n][32][OW] fp32, the fourth user of the lanes of csrc/window_gather.h: one lane per quad of four neighbouring
// pixels of an output row and one 16-byte store per lane, grid.x walks the 8 OW quads of a strip, grid.y strides over the boxes.  The
// box is uniform over the workgroup: its five words, its page's three and everything derived from them (clip, ch, cw, sw, the placement,
// which of the two cases) sit in scalar registers, and the choice between the cases and between 32- and 64-bit division is a scalar branch.
//   ch <= 32   the crop + pad of footprint(): a pixel is one source element (through value_of and the 256-entry table) or white.
//   ch >  32   the exact area average in units of 1 / 32 source pixel.  Output row oy covers [oy ch, (oy + 1) ch), column j covers
//              [j ch, (j + 1) ch) cut to 32 cw; a lane walks the at most ceil(ch / 32) + 1 source rows and columns of each of its pixels
//              where they lie (L1 / L2 hold them: neighbouring pixels share their edge rows and columns).  A row's sum is at most
//              32767 * 255 < 2^23 and its weighted value < 2^28 (32 bits); the sum over the rows reaches 2.7e11 and is kept in 64 bits;
//              the rounded division runs in 32 bits for ch <= 2048, where 2 S + Area < 2^31, and in 64 bits above.
// Every value is an integer until the table lookup, so no order of summation and no rounding mode enters.  Nothing is staged in LDS, no
// atomics, no synchronisation; ONE launch writes every element of out.
//
// A box whose page index is outside the table, whose page does not lie inside the store or has a side over QEA_WORD_STRIP_MAX_SIDE, or
// which is empty after clipping reads as an all-white strip: a bad table never becomes an access outside the caller's buffers.
#include "page_store.h"
#include "window_gather.h"

namespace {

constexpr int OH = QEA_WORD_STRIP_H;
static_assert(OH == 32, "the statement's unit is 1 / 32 source pixel: the shifts by 5 below");

template <typename T>
__global__ __launch_bounds__(WG_THREADS) void word_strips_kernel(const T* __restrict__ store, const PageStore ps,
                                                                 const int32_t* __restrict__ boxes, int n, int OW,
                                                                 const float* __restrict__ norm, float* __restrict__ out) {
  int q, oy, ox;
  if (!quad_of(OH, OW, q, oy, ox)) return;
  for (int i = blockIdx.y; i < n; i += gridDim.y) {    // uniform over the workgroup: everything up to the pixel loops is scalar
    const int32_t* b = boxes + 5 * (size_t)i;
    Page g = page_of(ps, b[0]);
    if (g.h > QEA_WORD_STRIP_MAX_SIDE || g.w > QEA_WORD_STRIP_MAX_SIDE) g.h = g.w = 0;
    const int x0 = max(b[1], 0), y0 = max(b[2], 0), x1 = min(b[3], g.w), y1 = min(b[4], g.h);
    f32x4 v = {1.f, 1.f, 1.f, 1.f};
    if (x0 < x1 && y0 < y1) {                          // compared, not subtracted: the box words are ANY int32
      const T* const page = store + g.off;
      const int cw = x1 - x0, ch = y1 - y0;            // 1..32767 each
      if (ch <= OH) {
        const Footprint f = footprint(x0, y0, x1, y1, OH, OW);
        const int sy = oy - f.dy;
        if (sy >= f.fy0 && sy < f.fy1) {
          const T* const row = page + (long long)sy * g.w;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int sx = ox + k - f.dx;
            if (sx >= f.fx0 && sx < f.fx1) v[k] = norm[value_of(row[sx])];
          }
        }
      } else {
        const int W32 = 32 * cw, sw = (W32 + ch - 1) / ch, left = qea_floordiv2(OW - sw);
        const int ya = oy * ch, yb = ya + ch;          // <= 32 * 32767
        const int r0 = ya >> 5, r1 = (yb - 1) >> 5;    // r1 <= ch - 1
        const T* const corner = page + (long long)y0 * g.w + x0;
        for (int k = 0; k < 4; ++k) {
          const int j = ox + k - left;
          if (j < 0 || j >= sw) continue;
          const int xa = j * ch, xb = min(xa + ch, W32);   // (sw - 1) ch < 32 cw: never empty
          const int c0 = xa >> 5, c1 = (xb - 1) >> 5;      // c1 <= cw - 1
          unsigned long long S = 0;
          for (int r = r0; r <= r1; ++r) {
            const T* const row = corner + (long long)r * g.w;
            const unsigned wy = (unsigned)(min(32 * r + 32, yb) - max(32 * r, ya));
            unsigned s = 0;
            for (int c = c0; c <= c1; ++c) s += (unsigned)(min(32 * c + 32, xb) - max(32 * c, xa)) * (unsigned)value_of(row[c]);
            S += (unsigned long long)(wy * s);
          }
          const unsigned long long area = (unsigned long long)ch * (unsigned)(xb - xa);
          const unsigned level = ch <= 2048 ? ((unsigned)(2 * S + area)) / ((unsigned)(2 * area)) : (unsigned)((2 * S + area) / (2 * area));
          v[k] = norm[level];
        }
      }
    }
    *reinterpret_cast<f32x4*>(out + quad_element(i, OH, OW, q)) = v;
  }
}

}  // namespace

extern "C" int qea_word_strips(const void* store, int32_t store_is_f32, int64_t store_elems, const int64_t* offset, const int32_t* h,
                               const int32_t* w, int32_t n_pages, const int32_t* boxes, int32_t n, int32_t OW, const float* norm, float* out,
                               void* stream) {
  const char* who = "qea_word_strips";
  const PageStore ps = {(long long)store_elems, n_pages, offset, h, w};
  if (int rc = check_store(who, store, store_is_f32)) return rc;
  if (int rc = check_table(who, ps)) return rc;
  QEA_REQUIRE(boxes && norm && out, "%s: null pointer", who);
  QEA_REQUIRE(n >= 0 && n <= QEA_WORD_STRIP_MAX_BOXES, "%s: n=%d outside 0..2^20", who, n);
  QEA_REQUIRE(OW >= QEA_WORD_STRIP_MIN_W && OW <= QEA_WORD_STRIP_MAX_W && OW % 16 == 0, "%s: OW=%d must be a multiple of 16 in %d..%d", who, OW,
              QEA_WORD_STRIP_MIN_W, QEA_WORD_STRIP_MAX_W);
  QEA_REQUIRE(((uintptr_t)offset & 7) == 0 && (((uintptr_t)h | (uintptr_t)w | (uintptr_t)boxes | (uintptr_t)norm) & 3) == 0,
              "%s: offset must be 8-byte aligned, h / w / boxes / norm 4-byte aligned", who);
  QEA_REQUIRE(((uintptr_t)out & 15) == 0, "%s: out must be 16-byte aligned", who);
  if (n == 0) return QEA_OK;                           // nothing to write
  dispatch_store(store_is_f32, store, [&](auto* typed) {
    launch_over_quads(word_strips_kernel<StoreElem<decltype(typed)>>, n, OH, OW, stream, typed, ps, boxes, n, OW, norm, out);
  });
  QEA_CHECK_LAUNCH();
  return QEA_OK;
}
