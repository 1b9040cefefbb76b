// Connected-component labelling over the packed page store, bit for bit the statement tests/components_spec.py (include/qea_hip.h:
// qea_cc_label, qea_cc_stats, qea_cc_despeckle, qea_cc_smear, qea_cc_boxes; qea/components.py is the product interface, whose host path is
// the same statement in numpy).
//
// A pixel is ink iff its 8-bit value (csrc/page_store.h: ink_of) is <= ink_max, or, when a uint8 ink mask packed like the
// store is given, iff its mask byte is not 0.  The label of an ink pixel is the smallest row-major index y * w + x WITHIN ITS PAGE over the
// pixels of its component, background is -1: one labelling, whatever the order in which workgroups run.  `labels` and `area` are int32
// arrays packed like the store; what lies between the pages is never written.  Every kernel but the border kernel gives workgroup b one
// TH x TW tile of one page through the tile_first prefix table (csrc/page_store.h: tile_of_block; QEA_BINARIZE_TILE_H / _W).
//
// qea_cc_label, three launches:
//   tile_kernel     the tile's pixels become a union-find forest in LDS (L[i] = i for ink, -1 otherwise); every ink pixel is united with
//                   its left / upper (and, at connectivity 8, upper-left / upper-right) neighbour inside the tile; then every pixel writes
//                   the page-relative index of its tile-local root.  A tile-local index orders pixels as the page-relative one does, so
//                   the root is the tile-local minimum.  The kernel also clears the in-page elements of `area` when it is given.
//   border_kernel   one thread per pixel of a tile's bottom row and right column unites it with its neighbours across the edge (the two
//                   diagonals as well at connectivity 8, which also covers both diagonals through a tile corner).  Lock-free min-index
//                   union-find on `labels` (csrc/union_find.h): find both roots, atomicMin the larger root's slot with the smaller; when
//                   the value the atomic returns shows that the slot was no longer a root, go on from that value.
//   flatten_kernel  every ink pixel's label becomes its root.
// The invariant and why no connection is lost are in csrc/union_find.h: labels[x] <= x is a pixel of x's component, the smallest pixel m of
// a component is a root throughout, and when the border kernel has ended every adjacent pair has been united, so that a component has one
// root, m.  Inside the border kernel every access to `labels` is an agent-scope relaxed atomic (the XCDs' L2s are not coherent for plain
// loads within a launch); kernel boundaries order the rest.
//
// Termination: no kernel waits for another workgroup.  Every loop over labels / L moves to a strictly smaller index or exits (find), or
// strictly lowers the larger of its two indices or exits (unite), so its length is bounded by the chain it walks.  A value that is no
// index of the page (a caller's buffer that no labelling filled) ends a walk and is never used as an address.
//
// qea_cc_stats, one launch: a thread merges the runs of equal labels among its eight consecutive pixels, the workgroup counts per distinct
// root in an LDS hash table (2048 slots; a tile holds at most 1024 distinct labels, as no two 4-neighbours differ), and sends ONE atomicAdd
// per distinct root to area[root].  Integer adds commute: the result is exact.  It ADDS to what qea_cc_label cleared.
// qea_cc_despeckle, one launch: out = (label >= 0 && area[label] >= min_area) ? 0 : 255 / 1.0f.
// qea_cc_smear, one launch per direction: the tile with `gap` pixels of halo on both sides of the direction in LDS (0 outside the page); a
// background pixel with ink at distance a before and b after it, a + b - 1 <= gap, becomes ink.  Output: a uint8 mask, 1 / 0.
// qea_cc_boxes, one launch: the same hash table carries x / y minima and maxima per distinct root; a root's rank among the caller's ascending
// list of roots is found by binary search, and one atomicMin / atomicMax per bound and distinct root reaches boxes[rank].
#include "page_store.h"
#include "union_find.h"

namespace {

constexpr int TH = QEA_BINARIZE_TILE_H, TW = QEA_BINARIZE_TILE_W, TILE = TH * TW, THREADS = 256, EDGE_THREADS = 128, SLOTS = 2048;
constexpr int MAX_GAP = QEA_CC_MAX_GAP;
static_assert(TW == 64 && TH == 32 && THREADS == 256, "a wave owns eight rows of the tile and a lane one column; 8 pixels per thread");
static_assert((SLOTS & (SLOTS - 1)) == 0 && SLOTS >= TILE, "the hash table holds every pixel of a tile even if all labels differ");
constexpr int SMEAR_LDS = (TH + 2 * MAX_GAP) * TW > TH * (TW + 2 * MAX_GAP) ? (TH + 2 * MAX_GAP) * TW : TH * (TW + 2 * MAX_GAP);

template <typename T>
__global__ __launch_bounds__(THREADS) void cc_tile_kernel(const T* __restrict__ store, const PageStore ps,
                                                          const int32_t* __restrict__ tile_first, const uint8_t* __restrict__ ink_mask,
                                                          int ink_max, int conn8, int32_t* __restrict__ labels, int32_t* __restrict__ area) {
  __shared__ int L[TILE];
  const Tile t = tile_of_block(ps, tile_first, TH, TW);
  if (t.g.h == 0) return;                                      // uniform
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int px = t.x0 + lane;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int ly = 8 * wave + k, py = t.y0 + ly;
    bool ink = false;
    if (py < t.g.h && px < t.g.w) {
      const long long at = t.g.off + (long long)py * t.g.w + px;
      ink = ink_mask ? ink_mask[at] != 0 : ink_of(store, at, ink_max);
    }
    L[ly * TW + lane] = ink ? ly * TW + lane : -1;
  }
  __syncthreads();
  const LdsForest f = {L};
  for (int k = 0; k < 8; ++k) {
    const int ly = 8 * wave + k, i = ly * TW + lane;
    if (f.load(i) < 0) continue;                               // a label is negative iff the pixel is background, at any time
    if (lane > 0 && f.load(i - 1) >= 0) unite(f, i, i - 1);
    if (ly > 0) {
      if (f.load(i - TW) >= 0) unite(f, i, i - TW);
      if (conn8 && lane > 0 && f.load(i - TW - 1) >= 0) unite(f, i, i - TW - 1);
      if (conn8 && lane < TW - 1 && f.load(i - TW + 1) >= 0) unite(f, i, i - TW + 1);
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int ly = 8 * wave + k, py = t.y0 + ly, i = ly * TW + lane;
    if (py >= t.g.h || px >= t.g.w) continue;
    const long long at = t.g.off + (long long)py * t.g.w + px;
    int label = -1;
    if (L[i] >= 0) {
      const int r = find_root(f, i);
      label = (t.y0 + r / TW) * t.g.w + t.x0 + r % TW;
    }
    labels[at] = label;
    if (area) area[at] = 0;
  }
}

// one workgroup per tile: threads 0..63 own the pixels of its bottom row, threads 64..95 those of its right column
__global__ __launch_bounds__(EDGE_THREADS) void cc_border_kernel(const PageStore ps, const int32_t* __restrict__ tile_first, int conn8,
                                                                 int32_t* labels) {
  const Tile t = tile_of_block(ps, tile_first, TH, TW);
  if (t.g.h == 0) return;
  const int k = threadIdx.x, W = t.g.w, H = t.g.h;
  const PageForest f = {labels + t.g.off};
  if (k < TW) {
    const int y = t.y0 + TH - 1, x = t.x0 + k;
    if (y + 1 >= H || x >= W) return;
    const int i = y * W + x;
    if (f.load(i) < 0) return;
    if (f.load(i + W) >= 0) unite(f, i, i + W);
    if (conn8 && x > 0 && f.load(i + W - 1) >= 0) unite(f, i, i + W - 1);
    if (conn8 && x + 1 < W && f.load(i + W + 1) >= 0) unite(f, i, i + W + 1);
  } else if (k < TW + TH) {
    const int y = t.y0 + k - TW, x = t.x0 + TW - 1;
    if (y >= H || x + 1 >= W) return;
    const int i = y * W + x;
    if (f.load(i) < 0) return;
    if (f.load(i + 1) >= 0) unite(f, i, i + 1);
    if (conn8 && y > 0 && f.load(i - W + 1) >= 0) unite(f, i, i - W + 1);
    if (conn8 && y + 1 < H && f.load(i + W + 1) >= 0) unite(f, i, i + W + 1);
  }
}

__global__ __launch_bounds__(THREADS) void cc_flatten_kernel(const PageStore ps, const int32_t* __restrict__ tile_first, int32_t* labels) {
  const Tile t = tile_of_block(ps, tile_first, TH, TW);
  if (t.g.h == 0) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, px = t.x0 + lane;
  // Other threads of this launch replace labels by their roots meanwhile: a walk meets old parents or new roots, members of the same
  // chain either way, and ends at the one root, which nobody changes.
  const PageForest f = {labels + t.g.off};
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int py = t.y0 + 8 * wave + k;
    if (py >= t.g.h || px >= t.g.w) continue;
    const int i = py * t.g.w + px, p = f.load(i);
    if (p < 0 || p >= i) continue;                             // background, or a root
    const int r = find_root(f, p);
    if (r != p) __hip_atomic_store(f.L + i, r, RLX_AGENT);
  }
}

// ---- per-tile aggregation by distinct label: open addressing, linear probing, never more keys than slots
__device__ __forceinline__ int slot_of(int* keys, int key) {
  int s = (int)(((unsigned)key * 2654435761u) >> 21) & (SLOTS - 1);
  for (int n = 0; n < SLOTS; ++n) {                            // at most SLOTS probes
    const int old = atomicCAS(&keys[s], -1, key);
    if (old == -1 || old == key) return s;
    s = (s + 1) & (SLOTS - 1);
  }
  return -1;
}

// the label of pixel (py, x) if it is an index of the page, else -1
__device__ __forceinline__ int label_at(const int32_t* __restrict__ labels, const Page& g, int py, int x) {
  if (py >= g.h || x >= g.w) return -1;
  const int l = labels[g.off + (long long)py * g.w + x];
  return l >= 0 && l < g.h * g.w ? l : -1;
}

__global__ __launch_bounds__(THREADS) void cc_stats_kernel(const PageStore ps, const int32_t* __restrict__ tile_first,
                                                           const int32_t* __restrict__ labels, int32_t* __restrict__ area) {
  __shared__ int keys[SLOTS], count[SLOTS];
  const Tile t = tile_of_block(ps, tile_first, TH, TW);
  if (t.g.h == 0) return;
  for (int s = threadIdx.x; s < SLOTS; s += THREADS) {
    keys[s] = -1;
    count[s] = 0;
  }
  __syncthreads();
  const int py = t.y0 + (int)threadIdx.x / 8, x0 = t.x0 + (int)threadIdx.x % 8 * 8;
  int cur = -1, n = 0;
  for (int k = 0; k <= 8; ++k) {
    const int l = k < 8 ? label_at(labels, t.g, py, x0 + k) : -1;
    if (l == cur) {
      ++n;
      continue;
    }
    if (cur >= 0) {
      const int s = slot_of(keys, cur);
      if (s >= 0) atomicAdd(&count[s], n);
    }
    cur = l;
    n = 1;
  }
  __syncthreads();
  for (int s = threadIdx.x; s < SLOTS; s += THREADS)
    if (keys[s] >= 0) atomicAdd(&area[t.g.off + keys[s]], count[s]);
}

__global__ __launch_bounds__(THREADS) void cc_despeckle_kernel(const PageStore ps, const int32_t* __restrict__ tile_first,
                                                               const int32_t* __restrict__ labels, const int32_t* __restrict__ area,
                                                               int min_area, float* __restrict__ out_f32, uint8_t* __restrict__ out_u8) {
  const Tile t = tile_of_block(ps, tile_first, TH, TW);
  if (t.g.h == 0) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, px = t.x0 + lane;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int py = t.y0 + 8 * wave + k;
    if (py >= t.g.h || px >= t.g.w) continue;
    const int l = label_at(labels, t.g, py, px);
    const bool keep = l >= 0 && area[t.g.off + l] >= min_area;
    put_ink(out_f32, out_u8, t.g.off + (long long)py * t.g.w + px, keep);
  }
}

template <typename T>
__global__ __launch_bounds__(THREADS) void cc_smear_kernel(const T* __restrict__ store, const PageStore ps,
                                                           const int32_t* __restrict__ tile_first, const uint8_t* __restrict__ in_mask,
                                                           int ink_max, int gap, int vertical, uint8_t* __restrict__ out_mask) {
  __shared__ uint8_t px[SMEAR_LDS];
  const Tile t = tile_of_block(ps, tile_first, TH, TW);
  if (t.g.h == 0) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int gy = vertical ? gap : 0, gx = vertical ? 0 : gap, SH = TH + 2 * gy, SW = TW + 2 * gx;     // SH * SW <= SMEAR_LDS
  for (int sy = wave; sy < SH; sy += 4) {
    const int py = t.y0 - gy + sy;
    const bool row_in = py >= 0 && py < t.g.h;
    for (int sx = lane; sx < SW; sx += 64) {
      const int qx = t.x0 - gx + sx;
      bool ink = false;
      if (row_in && qx >= 0 && qx < t.g.w) {
        const long long at = t.g.off + (long long)py * t.g.w + qx;
        ink = in_mask ? in_mask[at] != 0 : ink_of(store, at, ink_max);
      }
      px[sy * SW + sx] = ink;
    }
  }
  __syncthreads();
  const int step = vertical ? SW : 1;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int ly = 8 * wave + k, py = t.y0 + ly, qx = t.x0 + lane;
    if (py >= t.g.h || qx >= t.g.w) continue;
    const uint8_t* c = px + (ly + gy) * SW + lane + gx;
    bool ink = *c != 0;
    if (!ink) {
      int a = 0, b = 0;
      for (int d = 1; d <= gap; ++d)
        if (c[-d * step]) {
          a = d;
          break;
        }
      if (a)
        for (int d = 1; d <= gap + 1 - a; ++d)
          if (c[d * step]) {
            b = d;
            break;
          }
      ink = a && b;
    }
    out_mask[t.g.off + (long long)py * t.g.w + qx] = ink;
  }
}

__global__ __launch_bounds__(THREADS) void cc_boxes_kernel(const PageStore ps, const int32_t* __restrict__ tile_first,
                                                           const int32_t* __restrict__ labels, const int32_t* __restrict__ roots,
                                                           const int32_t* __restrict__ root_first, int n_roots, int32_t* __restrict__ boxes) {
  __shared__ int keys[SLOTS], lo_x[SLOTS], lo_y[SLOTS], hi_x[SLOTS], hi_y[SLOTS];
  const Tile t = tile_of_block(ps, tile_first, TH, TW);
  if (t.g.h == 0) return;
  for (int s = threadIdx.x; s < SLOTS; s += THREADS) {
    keys[s] = -1;
    lo_x[s] = lo_y[s] = 0x7fffffff;
    hi_x[s] = hi_y[s] = -1;
  }
  __syncthreads();
  const int py = t.y0 + (int)threadIdx.x / 8, x0 = t.x0 + (int)threadIdx.x % 8 * 8;
  int cur = -1, from = 0;
  for (int k = 0; k <= 8; ++k) {
    const int l = k < 8 ? label_at(labels, t.g, py, x0 + k) : -1;
    if (l == cur) continue;
    if (cur >= 0) {
      const int s = slot_of(keys, cur);
      if (s >= 0) {
        atomicMin(&lo_x[s], x0 + from);
        atomicMax(&hi_x[s], x0 + k - 1);
        atomicMin(&lo_y[s], py);
        atomicMax(&hi_y[s], py);
      }
    }
    cur = l;
    from = k;
  }
  __syncthreads();
  int lo = root_first[t.page], end = root_first[t.page + 1];
  lo = max(lo, 0);
  end = min(end, n_roots);
  for (int s = threadIdx.x; s < SLOTS; s += THREADS) {
    const int key = keys[s];
    if (key < 0) continue;
    int a = lo, b = end;                                       // the first rank in [lo, end) whose root is >= key
    while (a < b) {
      const int mid = (a + b) >> 1;
      if (roots[mid] < key) a = mid + 1; else b = mid;
    }
    if (a >= end || roots[a] != key) continue;                 // a component the caller did not list
    atomicMin(&boxes[4 * (long long)a + 0], lo_x[s]);
    atomicMin(&boxes[4 * (long long)a + 1], lo_y[s]);
    atomicMax(&boxes[4 * (long long)a + 2], hi_x[s]);
    atomicMax(&boxes[4 * (long long)a + 3], hi_y[s]);
  }
}

int check_words(const char* who, const char* name, const void* p, bool required) {
  QEA_REQUIRE(p || !required, "%s: %s is NULL", who, name);
  QEA_REQUIRE(((uintptr_t)p & 3) == 0, "%s: %s must be 4-byte aligned", who, name);
  return QEA_OK;
}

}  // namespace

extern "C" int qea_cc_label(const void* store, int32_t store_is_f32, int64_t store_elems, const int64_t* offset, const int32_t* h,
                            const int32_t* w, int32_t n_pages, const int32_t* host_h, const int32_t* host_w, const int32_t* tile_first,
                            const uint8_t* ink_mask, int32_t ink_max, int32_t connectivity, int32_t* labels, int32_t* area, void* stream) {
  const char* who = "qea_cc_label";
  const PageStore ps = {(long long)store_elems, n_pages, offset, h, w};
  long long blocks = 0;
  if (int rc = check_paged_launch(who, store, store_is_f32, ps, host_h, host_w, tile_first, true, &blocks)) return rc;
  if (int rc = check_words(who, "labels", labels, true)) return rc;
  if (int rc = check_words(who, "area", area, false)) return rc;
  QEA_REQUIRE(connectivity == 4 || connectivity == 8, "%s: connectivity=%d is neither 4 nor 8", who, connectivity);
  QEA_REQUIRE(ink_max >= 0 && ink_max <= 254, "%s: ink_max=%d outside 0..254", who, ink_max);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)blocks);
  const int conn8 = connectivity == 8;
  dispatch_store(store_is_f32, store, [&](auto* typed) {
    cc_tile_kernel<<<grid, dim3(THREADS), 0, s>>>(typed, ps, tile_first, ink_mask, ink_max, conn8, labels, area);
  });
  QEA_CHECK_LAUNCH();
  cc_border_kernel<<<grid, dim3(EDGE_THREADS), 0, s>>>(ps, tile_first, conn8, labels);
  QEA_CHECK_LAUNCH();
  cc_flatten_kernel<<<grid, dim3(THREADS), 0, s>>>(ps, tile_first, labels);
  QEA_CHECK_LAUNCH();
  return QEA_OK;
}

extern "C" int qea_cc_stats(const void* store, int32_t store_is_f32, int64_t store_elems, const int64_t* offset, const int32_t* h,
                            const int32_t* w, int32_t n_pages, const int32_t* host_h, const int32_t* host_w, const int32_t* tile_first,
                            const int32_t* labels, int32_t* area, void* stream) {
  const char* who = "qea_cc_stats";
  const PageStore ps = {(long long)store_elems, n_pages, offset, h, w};
  long long blocks = 0;
  if (int rc = check_paged_launch(who, store, store_is_f32, ps, host_h, host_w, tile_first, true, &blocks)) return rc;
  if (int rc = check_words(who, "labels", labels, true)) return rc;
  if (int rc = check_words(who, "area", area, true)) return rc;
  cc_stats_kernel<<<dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream>>>(ps, tile_first, labels, area);
  QEA_CHECK_LAUNCH();
  return QEA_OK;
}

extern "C" int qea_cc_despeckle(const void* store, int32_t store_is_f32, int64_t store_elems, const int64_t* offset, const int32_t* h,
                                const int32_t* w, int32_t n_pages, const int32_t* host_h, const int32_t* host_w, const int32_t* tile_first,
                                const int32_t* labels, const int32_t* area, int32_t min_area, float* out_f32, uint8_t* out_u8, void* stream) {
  const char* who = "qea_cc_despeckle";
  const PageStore ps = {(long long)store_elems, n_pages, offset, h, w};
  long long blocks = 0;
  if (int rc = check_paged_launch(who, store, store_is_f32, ps, host_h, host_w, tile_first, true, &blocks)) return rc;
  if (int rc = check_words(who, "labels", labels, true)) return rc;
  if (int rc = check_words(who, "area", area, true)) return rc;
  if (int rc = check_outputs(who, out_f32, out_u8)) return rc;
  QEA_REQUIRE(min_area >= 1, "%s: min_area=%d must be at least 1", who, min_area);
  cc_despeckle_kernel<<<dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream>>>(ps, tile_first, labels, area, min_area, out_f32,
                                                                                         out_u8);
  QEA_CHECK_LAUNCH();
  return QEA_OK;
}

extern "C" int qea_cc_smear(const void* store, int32_t store_is_f32, int64_t store_elems, const int64_t* offset, const int32_t* h,
                            const int32_t* w, int32_t n_pages, const int32_t* host_h, const int32_t* host_w, const int32_t* tile_first,
                            const uint8_t* in_mask, int32_t ink_max, int32_t gap, int32_t vertical, uint8_t* out_mask, void* stream) {
  const char* who = "qea_cc_smear";
  const PageStore ps = {(long long)store_elems, n_pages, offset, h, w};
  long long blocks = 0;
  if (int rc = check_paged_launch(who, store, store_is_f32, ps, host_h, host_w, tile_first, true, &blocks)) return rc;
  QEA_REQUIRE(out_mask, "%s: out_mask is NULL", who);
  QEA_REQUIRE(out_mask != in_mask, "%s: a pass cannot run in place", who);
  QEA_REQUIRE(ink_max >= 0 && ink_max <= 254, "%s: ink_max=%d outside 0..254", who, ink_max);
  QEA_REQUIRE(gap >= 0 && gap <= MAX_GAP, "%s: gap=%d outside 0..%d", who, gap, MAX_GAP);
  QEA_REQUIRE(vertical == 0 || vertical == 1, "%s: vertical=%d is neither 0 nor 1", who, vertical);
  dispatch_store(store_is_f32, store, [&](auto* typed) {
    cc_smear_kernel<<<dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream>>>(typed, ps, tile_first, in_mask, ink_max, gap, vertical,
                                                                                       out_mask);
  });
  QEA_CHECK_LAUNCH();
  return QEA_OK;
}

extern "C" int qea_cc_boxes(const void* store, int32_t store_is_f32, int64_t store_elems, const int64_t* offset, const int32_t* h,
                            const int32_t* w, int32_t n_pages, const int32_t* host_h, const int32_t* host_w, const int32_t* tile_first,
                            const int32_t* labels, const int32_t* roots, const int32_t* root_first, int32_t n_roots, int32_t* boxes,
                            void* stream) {
  const char* who = "qea_cc_boxes";
  const PageStore ps = {(long long)store_elems, n_pages, offset, h, w};
  long long blocks = 0;
  if (int rc = check_paged_launch(who, store, store_is_f32, ps, host_h, host_w, tile_first, true, &blocks)) return rc;
  if (int rc = check_words(who, "labels", labels, true)) return rc;
  if (int rc = check_words(who, "roots", roots, true)) return rc;
  if (int rc = check_words(who, "root_first", root_first, true)) return rc;
  if (int rc = check_words(who, "boxes", boxes, true)) return rc;
  QEA_REQUIRE(n_roots >= 0, "%s: n_roots=%d is negative", who, n_roots);
  cc_boxes_kernel<<<dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream>>>(ps, tile_first, labels, roots, root_first, n_roots, boxes);
  QEA_CHECK_LAUNCH();
  return QEA_OK;
}
