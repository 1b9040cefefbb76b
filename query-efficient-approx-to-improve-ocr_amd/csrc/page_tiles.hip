// Whole pages through the eval-mode UNet tile by tile: all tiles of a pass cut out of the packed pages in one launch, and the cores of the
// cleaned tiles pasted into the packed outputs in one launch (include/qea_hip.h: qea_page_tiles_gather / qea_page_tiles_scatter;
// qea/pages.py: clean_pages, whose tiles_gather_spec / tiles_scatter_spec are the specification of the two kernels).
//
// The pages lie in the packed page store of csrc/page_store.h; the outputs are packed the same way with the same offsets.
//
// page_tiles_gather_kernel: out[N][TH][TW] fp32.  Tile t = (page, oy, ox) reads page pixel (oy + y, ox + x); what lies outside the page's
// h x w is white (1.0): the padding to the next multiple of 16 costs nothing.  A window gather (csrc/window_gather.h: lanes, reads, the
// 256-entry table of an 8-bit store, the 16-byte store); the three tile words and the page's words are uniform over the workgroup (scalar
// loads).  Tile origins are any int32: the window is cut to the tile without forming oy + y or h - oy where they overflow, its origin in 64 bits.
//
// page_tiles_scatter_kernel: the same lanes over the same quads, read with one 16-byte load.  Tile t = (page, oy, ox, cy0, cy1, cx0, cx1) owns
// the page pixels of its core [cy0, cy1) x [cx0, cx1) (page coordinates) that lie inside the tile and inside the page; a lane stores those of
// its four pixels, as fp32 and / or as 8-bit (uint8)(min(max(x, 0), 1) * 255.0f): one fp32 multiply, truncation, NaN -> 0.  The cores of a
// page's tiles partition it (qea/pages.py: plan_tiles), so every output element is written exactly once: no atomics, no prior fill.  Output
// rows have any width and start at any element, so the stores are per pixel; a wave's stores are neighbours in a few cache lines.
//
// Both kernels skip a page that does not lie inside the store (offset < 0 or offset + h * w > store_elems): a bad table gives white
// tiles / unwritten outputs, never an access outside the caller's buffers.
#include "page_store.h"
#include "window_gather.h"

namespace {

template <typename T>
__global__ __launch_bounds__(WG_THREADS) void page_tiles_gather_kernel(const T* __restrict__ store, const PageStore ps,
                                                                       const int32_t* __restrict__ tile, int N, int TH, int TW,
                                                                       const float* __restrict__ table, float* __restrict__ out) {
  window_gather(store, table, out, N, TH, TW, [=](int t) {
    const Page g = page_of(ps, tile[3 * t]);
    const int oy = tile[3 * t + 1], ox = tile[3 * t + 2];
    // Tile pixel (x, y) is page pixel (ox + x, oy + y): rows -oy .. h-oy-1 and columns -ox .. w-ox-1 of the tile, cut to it.  Origins are
    // ANY int32, so a - o may not be formed as an int: cut = min(max(a - o, 0), hi) for a >= 0 < hi, where o < a gives 0 < a - o < 2^32
    const auto cut = [](int a, int o, int hi) { return o >= a ? 0 : (int)min((unsigned)a - (unsigned)o, (unsigned)hi); };
    return Window{g.off + (long long)oy * g.w + ox, g.w, cut(0, ox, TW), cut(0, oy, TH), cut(g.w, ox, TW), cut(g.h, oy, TH)};
  });
}

__global__ __launch_bounds__(WG_THREADS) void page_tiles_scatter_kernel(const float* __restrict__ tiles, int N, int TH, int TW,
                                                                        const int32_t* __restrict__ tile, const PageStore ps,
                                                                        float* __restrict__ out_f32, uint8_t* __restrict__ out_u8) {
  int q, ty, tx0;
  if (!quad_of(TH, TW, q, ty, tx0)) return;
  for (int t = blockIdx.y; t < N; t += gridDim.y) {    // uniform over the workgroup
    const int32_t* r = tile + 7 * t;
    const Page g = page_of(ps, r[0]);
    const long long py = (long long)r[1] + ty, px0 = (long long)r[2] + tx0;
    // rows and columns this tile owns: its core, inside the page (the tile itself bounds ty and tx0 + k)
    const long long y0 = max(r[3], 0), y1 = min(r[4], g.h), x0 = max(r[5], 0), x1 = min(r[6], g.w);
    if (py < y0 || py >= y1 || px0 + 3 < x0 || px0 >= x1) continue;
    const f32x4 v = *reinterpret_cast<const f32x4*>(tiles + quad_element(t, TH, TW, q));
    const long long row = g.off + py * g.w;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long long px = px0 + k;
      if (px >= x0 && px < x1) {
        if (out_f32) out_f32[row + px] = v[k];
        if (out_u8) out_u8[row + px] = to_u8(v[k]);
      }
    }
  }
}

int check_common(const char* who, const PageStore& ps, const void* tile, int N, int TH, int TW) {
  if (int rc = check_table(who, ps)) return rc;
  QEA_REQUIRE(tile, "%s: null pointer", who);
  QEA_REQUIRE(N >= 1 && N <= (1 << 24), "%s: N=%d outside 1..2^24", who, N);
  QEA_REQUIRE(TH >= 1 && TH <= 8192, "%s: TH=%d outside 1..8192", who, TH);
  QEA_REQUIRE(TW >= 4 && TW <= 8192 && TW % 4 == 0, "%s: TW=%d must be a multiple of 4 in 4..8192", who, TW);
  return QEA_OK;
}

}  // namespace

extern "C" int qea_page_tiles_gather(const void* store, int32_t store_is_f32, int64_t store_elems, const int64_t* offset, const int32_t* h,
                                     const int32_t* w, int32_t n_pages, const int32_t* tile, int32_t N, int32_t TH, int32_t TW,
                                     const float* table, float* out, void* stream) {
  const char* who = "qea_page_tiles_gather";
  const PageStore ps = {(long long)store_elems, n_pages, offset, h, w};
  if (int rc = check_store(who, store, store_is_f32)) return rc;
  QEA_REQUIRE(out, "%s: null pointer", who);
  if (int rc = check_common(who, ps, tile, N, TH, TW)) return rc;
  QEA_REQUIRE(store_is_f32 || table, "%s: an 8-bit store needs the 256-entry table", who);
  QEA_REQUIRE(((uintptr_t)out & 15) == 0, "%s: out must be 16-byte aligned", who);
  dispatch_store(store_is_f32, store, [&](auto* typed) {
    launch_over_quads(page_tiles_gather_kernel<StoreElem<decltype(typed)>>, N, TH, TW, stream, typed, ps, tile, N, TH, TW, table, out);
  });
  QEA_CHECK_LAUNCH();
  return QEA_OK;
}

extern "C" int qea_page_tiles_scatter(const float* tiles, int32_t N, int32_t TH, int32_t TW, const int32_t* tile, const int64_t* offset,
                                      const int32_t* h, const int32_t* w, int32_t n_pages, int64_t store_elems, float* out_f32, uint8_t* out_u8,
                                      void* stream) {
  const char* who = "qea_page_tiles_scatter";
  const PageStore ps = {(long long)store_elems, n_pages, offset, h, w};
  QEA_REQUIRE(tiles, "%s: null pointer", who);
  if (int rc = check_outputs(who, out_f32, out_u8)) return rc;
  if (int rc = check_common(who, ps, tile, N, TH, TW)) return rc;
  QEA_REQUIRE(((uintptr_t)tiles & 15) == 0, "%s: tiles must be 16-byte aligned", who);
  launch_over_quads(page_tiles_scatter_kernel, N, TH, TW, stream, tiles, N, TH, TW, tile, ps, out_f32, out_u8);
  QEA_CHECK_LAUNCH();
  return QEA_OK;
}
