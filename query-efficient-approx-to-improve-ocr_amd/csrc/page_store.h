// The packed page store, described once for every translation unit that works on it: csrc/page_tiles.hip (tiles for the UNet),
// csrc/binarize.hip (Otsu, Sauvola), csrc/components.hip (labels, despeckle, smear, boxes), csrc/deskew.hip (strip sums, scores, rotation)
// and csrc/word_strips.hip (CRNN strips).  Pages of any sizes lie back to back, row-major without padding: page p is h[p] rows of w[p]
// elements at element offset[p] of the store (8-bit grey, so pages start at any byte, or fp32, read through the 8-bit rule below).  Outputs
// and working buffers "packed like the store" use the same offsets.  qea/pages.py is the Python side of the same object and
// qea/ops.py: page_table builds the tables below.
//
// Device side: PageStore / page_of (the table, by value in a kernel's arguments), page_of_block / tile_of_block (workgroup -> page and
// tile through a prefix table), value_of / ink_of (an element as the 8-bit value every statement reads), put_ink (the two packed
// outputs of a binariser).  Host side: the checks the entry points share and dispatch_store, which turns store_is_f32 into the element type.
// The per-feature checks (window, k, R, connectivity, gap, A, fill, overlaps) stay with their entry points.
#pragma once
#include <type_traits>
#include "common.h"

namespace {

// The scalars lead: with this order the component kernels' loops land where they run fastest (profiles/page_store_ab.json; the order
// decides how the compiler groups the argument loads, and through the prologue's length where every loop starts).
struct PageStore {
  long long store_elems;
  int n_pages;
  const int64_t* offset;
  const int32_t* h;
  const int32_t* w;
};

struct Page {
  long long off;
  int h, w;     // 0 x 0: no such page
};

// A page that does not lie inside the store (offset < 0 or offset + h * w > store_elems) reads as "no such page": a bad table never
// becomes an access outside the caller's buffers.
__device__ __forceinline__ Page page_of(const PageStore& ps, int p) {
  Page g = {0, 0, 0};
  if (p >= 0 && p < ps.n_pages) {
    const long long off = ps.offset[p];
    const int ph = ps.h[p], pw = ps.w[p];
    if (off >= 0 && ph > 0 && pw > 0 && off <= ps.store_elems && (long long)ph * pw <= ps.store_elems - off) {
      g.off = off;
      g.h = ph;
      g.w = pw;
    }
  }
  return g;
}

// largest p in [0, n_pages) with first[p] <= b (first[0] = 0): uniform over the workgroup when b is
__device__ __forceinline__ int page_of_block(const int32_t* __restrict__ first, int n_pages, int b) {
  int lo = 0, hi = n_pages;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (first[mid] <= b) lo = mid; else hi = mid;
  }
  return lo;
}

struct Tile {
  Page g;
  int page, y0, x0;     // g.h == 0: nothing to do (uniform over the workgroup)
};

// Workgroup blockIdx.x owns one TH x TW tile of one page: tile_first[p] <= b < tile_first[p + 1] names the page, b - tile_first[p] the
// tile, row after row.  A page outside the store or a tile outside its page (tables that disagree with the host's) is "nothing to do".
__device__ __forceinline__ Tile tile_of_block(const PageStore& ps, const int32_t* __restrict__ tile_first, int TH, int TW) {
  Tile t;
  t.page = page_of_block(tile_first, ps.n_pages, blockIdx.x);
  t.g = page_of(ps, t.page);
  t.y0 = t.x0 = 0;
  if (t.g.h == 0) return t;
  const int i = (int)blockIdx.x - tile_first[t.page], tiles_x = (t.g.w + TW - 1) / TW;
  if (i < 0 || i / tiles_x >= (t.g.h + TH - 1) / TH) {
    t.g.h = 0;
    return t;
  }
  t.y0 = i / tiles_x * TH;
  t.x0 = i % tiles_x * TW;
  return t;
}

// The 8-bit rule of the project (qea/pages.py: quantise_u8): (uint8)(min(max(x, 0), 1) * 255.0f), NaN -> 0
__device__ __forceinline__ uint8_t to_u8(float x) {
  const float c = fminf(fmaxf(x, 0.f), 1.f);           // fmaxf(NaN, 0) = 0
  return (uint8_t)(int)__fmul_rn(c, 255.0f);           // one fp32 multiply, then truncation
}

// the 8-bit value of a store element of either kind
__device__ __forceinline__ int value_of(uint8_t v) { return v; }
__device__ __forceinline__ int value_of(float v) { return to_u8(v); }

template <typename T>
__device__ __forceinline__ bool ink_of(const T* __restrict__ s, long long i, int ink_max) { return value_of(s[i]) <= ink_max; }

// Element i of the packed outputs that are given: ink as 0 / 0.0, background as 255 / 1.0.  (The two kernels that write grey values,
// page_tiles_scatter_kernel and rotate_kernel, spell their stores out: one derives the 8-bit form by to_u8, the other the fp32 form from a
// table that is only there with out_f32, and a shared writer changed the first one's register allocation.)
__device__ __forceinline__ void put_ink(float* __restrict__ out_f32, uint8_t* __restrict__ out_u8, long long i, bool ink) {
  if (out_f32) out_f32[i] = ink ? 0.f : 1.f;
  if (out_u8) out_u8[i] = ink ? 0 : 255;
}

// ---- host side: what the entry points check alike.  The order in which the checks of a call fire, which matters only for a call that is
// wrong in more than one way: the store (pointer, store_is_f32, fp32 alignment), the table (pointers, n_pages, store_elems), the host's
// page sizes (pointers, every page, then the 2^31 - 1 bound of each grid that is asked for), and only then the entry point's other
// pointers (its prefix table, tiles, boxes, norm, outputs) and its own parameters.  So a NULL prefix table or output is reported after a
// bad n_pages, qea_page_tiles_gather reports a misaligned fp32 store before a bad tile shape, and qea_deskew_rotate reports too many
// workgroups before a bad slope range, fill or overlap.  Every message and return code is what it was.
int check_store(const char* who, const void* store, int store_is_f32) {
  QEA_REQUIRE(store, "%s: null pointer", who);
  QEA_REQUIRE(store_is_f32 == 0 || store_is_f32 == 1, "%s: store_is_f32=%d is neither 0 nor 1", who, store_is_f32);
  QEA_REQUIRE(!store_is_f32 || ((uintptr_t)store & 3) == 0, "%s: an fp32 store must be 4-byte aligned", who);
  return QEA_OK;
}

int check_table(const char* who, const PageStore& ps) {
  QEA_REQUIRE(ps.offset && ps.h && ps.w, "%s: null pointer", who);
  QEA_REQUIRE(ps.n_pages >= 1 && ps.n_pages <= (1 << 24), "%s: n_pages=%d outside 1..2^24", who, ps.n_pages);
  QEA_REQUIRE(ps.store_elems >= 1, "%s: store_elems=%lld", who, ps.store_elems);
  return QEA_OK;
}

// The host's copy of the page sizes: no empty page, no side over max_side (0: no such bound), at most 2^27 pixels.  -> the pages' 32 x 64
// tiles in *tiles, their chunks of QEA_BINARIZE_CHUNK elements in *chunks (either at most 2^31 - 1: the grid of a launch), the largest h
// in *max_h; an output the caller does not need is NULL.
int check_page_sizes(const char* who, const int32_t* host_h, const int32_t* host_w, int n_pages, int max_side, long long* tiles,
                     long long* chunks, int* max_h) {
  constexpr int TH = QEA_BINARIZE_TILE_H, TW = QEA_BINARIZE_TILE_W, CHUNK = QEA_BINARIZE_CHUNK;
  QEA_REQUIRE(host_h && host_w, "%s: null pointer", who);
  long long n_tiles = 0, n_chunks = 0, top = 0;
  for (int p = 0; p < n_pages; ++p) {
    const long long ph = host_h[p], pw = host_w[p];
    QEA_REQUIRE(ph >= 1 && pw >= 1, "%s: page %d is empty (%lld x %lld)", who, p, ph, pw);
    QEA_REQUIRE(!max_side || (ph <= max_side && pw <= max_side), "%s: page %d is %lld x %lld, a side over %d", who, p, ph, pw, max_side);
    QEA_REQUIRE(ph * pw <= QEA_BINARIZE_MAX_PAGE_PIXELS, "%s: page %d has %lld x %lld pixels, more than 2^27", who, p, ph, pw);
    n_tiles += ((ph + TH - 1) / TH) * ((pw + TW - 1) / TW);
    n_chunks += (ph * pw + CHUNK - 1) / CHUNK;
    top = ph > top ? ph : top;
  }
  QEA_REQUIRE(!tiles || n_tiles <= 0x7fffffffll, "%s: %lld workgroups, more than 2^31 - 1", who, n_tiles);
  QEA_REQUIRE(!chunks || n_chunks <= 0x7fffffffll, "%s: %lld workgroups, more than 2^31 - 1", who, n_chunks);
  if (tiles) *tiles = n_tiles;
  if (chunks) *chunks = n_chunks;
  if (max_h) *max_h = (int)top;
  return QEA_OK;
}

// The three above for an entry point whose workgroups find their page through a prefix table: -> the grid in *blocks, the pages' tiles
// (`first` is tile_first) or chunks (chunk_first).
int check_paged_launch(const char* who, const void* store, int store_is_f32, const PageStore& ps, const int32_t* host_h, const int32_t* host_w,
                       const void* first, bool tiles, long long* blocks) {
  if (int rc = check_store(who, store, store_is_f32)) return rc;
  if (int rc = check_table(who, ps)) return rc;
  if (int rc = check_page_sizes(who, host_h, host_w, ps.n_pages, 0, tiles ? blocks : nullptr, tiles ? nullptr : blocks, nullptr)) return rc;
  QEA_REQUIRE(first, "%s: null pointer", who);
  return QEA_OK;
}

int check_outputs(const char* who, const void* out_f32, const void* out_u8) {
  QEA_REQUIRE(out_f32 || out_u8, "%s: neither an fp32 nor an 8-bit output", who);
  QEA_REQUIRE(((uintptr_t)out_f32 & 3) == 0, "%s: out_f32 must be 4-byte aligned", who);
  return QEA_OK;
}

// f(typed store) for the element type store_is_f32 names, so that a launch is written once: f is a generic lambda over `auto* store`, and
// StoreElem<decltype(store)> names a kernel template's instance where the call alone does not.
template <typename P> using StoreElem = std::remove_const_t<std::remove_pointer_t<P>>;

template <typename F>
auto dispatch_store(int store_is_f32, const void* store, F f) {
  if (store_is_f32) return f(static_cast<const float*>(store));
  return f(static_cast<const uint8_t*>(store));
}

}  // namespace
