// Page skew estimation and deskew over the packed page store, bit for bit the statement tests/deskew_spec.py (include/qea_hip.h:
// qea_skew_strip_sums, qea_skew_scores, qea_skew_pick, qea_deskew_rotate; qea/deskew.py is the product interface, whose host path is the
// same statement in numpy).  Every value is an integer, so no order of summation and no rounding mode enters.
//
// strip_sums_kernel   ONE pass over the pixels.  Workgroup b owns rows [32 rb, 32 rb + 32) of page b / blocks (rb = b % blocks, blocks =
//                     ceil(largest h / 32): a shorter page's surplus workgroups leave at once, so no block-to-page table is needed).  It walks
//                     the strips eight at a time: thread t reads the 32 pixels of (row t / 8, strip t % 8) — eight neighbouring lanes read
//                     256 consecutive pixels — as aligned 16-byte chunks.  Pages start at any byte, so a strip is cut out of the chunks that
//                     cover it: one bit per pixel (v <= ink_max) is gathered into a 64-bit word, shifted by the misalignment, masked to the
//                     strip's width and counted by one popcount.  A chunk that is not wholly inside the store is read element by element
//                     under a bounds check.  The counts cross an LDS buffer so that the stores run along y: 32 consecutive bytes per strip.
// scores_kernel       Workgroup b owns rows [63 c, 63 c + 63) of a page (c = b % blocks, blocks = ceil(largest h / 63)); lane l owns row
//                     63 c + l, and lane 63 only supplies its P to lane 62 (a chunk needs its neighbour row for the difference).  blockIdx.y
//                     names a group of 32 candidates, of which wave i takes the i-th, (i + 4)-th, ... (the chunks alone would leave most
//                     SIMDs without a wave on a batch of a few large pages).  The shift d(j, a) is uniform, so every read of C is 64
//                     consecutive bytes.  The squared differences are summed over the wave in int64 and reach scores[p][a + A] by one
//                     integer atomic per wave and candidate: exact, whatever the order.  C is read where it lies: it is 1 / 32 of the page and a chunk rereads its
//                     ns x (63 + shifts) bytes 2 A + 1 times from L1 / L2; an LDS copy of the chunk and its margin (up to 2 x 4096 rows at
//                     A = 256 and w = 32767) would not fit for the widest pages and was not kept.
// pick_kernel         One wave per page: every lane keeps the best of its candidates under the total order (larger S, then smaller |a|,
//                     then smaller a), a butterfly merges them, lane 0 applies the gain gate.
// rotate_kernel       ONE launch for all pages.  Workgroup b owns one 32 x 64 tile of one page through the tile_first table
//                     (csrc/page_store.h: tile_of_block); lane = column, a wave owns eight rows.  X and Y are int64 products for a thread's first row and advance
//                     by -2 S16 / +2 C16 per row, which are the same integers.  The four taps are
//                     read where they lie: at slopes of a few degrees the source rows of a tile are the tile's own rows plus a few, which
//                     L1 holds; an LDS copy of the footprint would be read once per tap all the same.
//
// All four skip a page that does not lie inside the store: tables that disagree with the host's give unwritten outputs, never an access
// outside the caller's buffers.
#include "page_store.h"

namespace {

constexpr int TH = QEA_BINARIZE_TILE_H, TW = QEA_BINARIZE_TILE_W, THREADS = 256;
constexpr int SUM_ROWS = 32, SUM_STRIPS = 8, SCORE_ROWS = 63, SCORE_CANDIDATES = 32;
static_assert(TW == 64 && TH == 32 && THREADS == 256 && SUM_ROWS * SUM_STRIPS == THREADS, "a wave owns eight rows of a tile and a lane one column");

struct alignas(16) Bytes16 { uint8_t v[16]; };
struct alignas(16) Floats4 { float v[4]; };
template <typename T> struct ChunkOf;
template <> struct ChunkOf<uint8_t> { typedef Bytes16 type; };
template <> struct ChunkOf<float> { typedef Floats4 type; };

// the number of pixels <= ink_max among the n <= 32 elements store[e .. e + n): 0 <= e, e + n <= store_elems
template <typename T>
__device__ __forceinline__ int strip_count(const T* __restrict__ store, long long store_elems, long long e, int n, int ink_max) {
  constexpr int K = 16 / (int)sizeof(T);                                      // elements per 16-byte chunk
  typedef typename ChunkOf<T>::type Chunk;
  const int mis = (int)(((uintptr_t)store / sizeof(T) + (unsigned long long)e) % K);
  const long long e0 = e - mis;                                               // the first element of the aligned chunk that holds e
  unsigned long long bits = 0;
#pragma unroll
  for (int c = 0; c <= 32 / K; ++c) {
    const long long at = e0 + (long long)c * K;
    if (at >= e + n) break;
    if (at >= 0 && at + K <= store_elems) {
      const Chunk q = *reinterpret_cast<const Chunk*>(store + at);
#pragma unroll
      for (int i = 0; i < K; ++i) bits |= (unsigned long long)(value_of(q.v[i]) <= ink_max) << (c * K + i);
    } else {
      for (int i = 0; i < K; ++i)
        if (at + i >= e && at + i < e + n) bits |= (unsigned long long)(value_of(store[at + i]) <= ink_max) << (c * K + i);
    }
  }
  return __popcll((bits >> mis) & (0xffffffffull >> (32 - n)));
}

template <typename T>
__global__ __launch_bounds__(THREADS) void strip_sums_kernel(const T* __restrict__ store, const PageStore ps, int blocks,
                                                             const int32_t* __restrict__ ink_max_dev, int ink_max, uint8_t* __restrict__ C) {
  __shared__ uint8_t cnt[SUM_STRIPS][SUM_ROWS + 1];
  const int p = (int)(blockIdx.x / (unsigned)blocks), y0 = (int)(blockIdx.x % (unsigned)blocks) * SUM_ROWS;
  const Page g = page_of(ps, p);
  if (g.h == 0 || y0 >= g.h) return;                                          // uniform
  if (ink_max_dev) ink_max = ink_max_dev[p];
  const int ns = (g.w + 31) >> 5;
  const int ry = threadIdx.x >> 3, rj = threadIdx.x & 7;                      // the element this thread counts
  const int wy = threadIdx.x & 31, wj = threadIdx.x >> 5;                     // the element this thread stores
  for (int j0 = 0; j0 < ns; j0 += SUM_STRIPS) {
    const int j = j0 + rj, y = y0 + ry;
    if (j < ns && y < g.h)
      cnt[rj][ry] = (uint8_t)strip_count(store, ps.store_elems, g.off + (long long)y * g.w + 32 * j, min(32, g.w - 32 * j), ink_max);
    __syncthreads();
    if (j0 + wj < ns && y0 + wy < g.h) C[g.off + (long long)(j0 + wj) * g.h + y0 + wy] = cnt[wj][wy];
    __syncthreads();
  }
}

__global__ __launch_bounds__(THREADS) void scores_kernel(const uint8_t* __restrict__ C, const PageStore ps, int blocks, int A,
                                                         unsigned long long* __restrict__ scores) {
  const int p = (int)(blockIdx.x / (unsigned)blocks), r0 = (int)(blockIdx.x % (unsigned)blocks) * SCORE_ROWS;
  const Page g = page_of(ps, p);
  if (g.h == 0 || r0 >= g.h) return;                                          // uniform
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = r0 + lane, ns = (g.w + 31) >> 5, half = g.w >> 1;
  const uint8_t* const Cp = C + g.off;
  const int k_end = min(2 * A + 1, ((int)blockIdx.y + 1) * SCORE_CANDIDATES);
  for (int k = (int)blockIdx.y * SCORE_CANDIDATES + wave; k < k_end; k += THREADS / 64) {
    const int a = k - A;
    int P = 0;
#pragma unroll 4
    for (int j = 0; j < ns; ++j) {
      const int rr = r + ((a * (32 * j + 16 - half) + 512) >> 10);            // an arithmetic shift: the true floor; |a (..)| < 2^24
      if (rr >= 0 && rr < g.h) P += Cp[(long long)j * g.h + rr];
    }
    const int next = __shfl_down(P, 1, 64);
    long long s = 0;
    if (lane < SCORE_ROWS && r + 1 < g.h) s = (long long)(next - P) * (next - P);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0 && s) atomicAdd(&scores[(long long)p * (2 * A + 1) + k], (unsigned long long)s);
  }
}

// the statement's order: a larger score wins, then the smaller |a|, then the negative a
__device__ __forceinline__ bool better(long long s, int a, long long t, int b) {
  if (s != t) return s > t;
  if (abs(a) != abs(b)) return abs(a) < abs(b);
  return a < b;
}

__global__ __launch_bounds__(64) void pick_kernel(const long long* __restrict__ scores, int A, int gain, int32_t* __restrict__ slopes) {
  const long long* const S = scores + (long long)blockIdx.x * (2 * A + 1);
  const int lane = threadIdx.x;
  int a = 0;                                                                  // every lane starts at candidate 0, which always exists
  long long s = S[A];
  for (int k = lane; k <= 2 * A; k += 64) {
    const long long t = S[k];
    if (better(t, k - A, s, a)) {
      s = t;
      a = k - A;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const long long t = __shfl_xor(s, o, 64);
    const int b = __shfl_xor(a, o, 64);
    if (better(t, b, s, a)) {
      s = t;
      a = b;
    }
  }
  if (lane == 0) slopes[blockIdx.x] = 100 * (s - S[A]) >= (long long)gain * S[A] ? a : 0;
}

template <typename T>
__device__ __forceinline__ int tap(const T* __restrict__ page, int h, int w, long long y, long long x, int fill) {
  return y >= 0 && y < h && x >= 0 && x < w ? value_of(page[y * w + x]) : fill;
}

template <typename T>
__global__ __launch_bounds__(THREADS) void rotate_kernel(const T* __restrict__ store, const PageStore ps, const int32_t* __restrict__ tile_first,
                                                         const int32_t* __restrict__ slopes, const int32_t* __restrict__ table, int A,
                                                         int nearest, int fill, const float* __restrict__ norm, float* __restrict__ out_f32,
                                                         uint8_t* __restrict__ out_u8) {
  const Tile t = tile_of_block(ps, tile_first, TH, TW);
  if (t.g.h == 0) return;                                                     // uniform
  const Page g = t.g;
  const int a = slopes[t.page];
  if (a < -A || a > A) return;                                                // uniform
  const long long C16 = table[2 * (a + A)], S16 = table[2 * (a + A) + 1];
  const int x = t.x0 + (threadIdx.x & 63), y0 = t.y0 + 8 * (threadIdx.x >> 6);
  if (x >= g.w) return;
  const T* const page = store + g.off;
  const long long dx2 = 2ll * x - (g.w - 1), dy2 = 2ll * y0 - (g.h - 1);
  long long X = C16 * dx2 - S16 * dy2 + 65536ll * (g.w - 1), Y = S16 * dx2 + C16 * dy2 + 65536ll * (g.h - 1);
  for (int y = y0; y < min(y0 + 8, g.h); ++y, X -= 2 * S16, Y += 2 * C16) {       // dy2 grows by 2 per row: the same integers as the products
    int v;
    if (nearest) {
      v = tap(page, g.h, g.w, (Y + 65536) >> 17, (X + 65536) >> 17, fill);
    } else {
      const long long sx = X >> 17, sy = Y >> 17;
      const int fx = (int)((X >> 9) & 255), fy = (int)((Y >> 9) & 255);
      v = ((256 - fx) * (256 - fy) * tap(page, g.h, g.w, sy, sx, fill) + fx * (256 - fy) * tap(page, g.h, g.w, sy, sx + 1, fill) +
           (256 - fx) * fy * tap(page, g.h, g.w, sy + 1, sx, fill) + fx * fy * tap(page, g.h, g.w, sy + 1, sx + 1, fill) + 32768) >> 16;
    }
    const long long i = g.off + (long long)y * g.w + x;
    if (out_u8) out_u8[i] = (uint8_t)v;
    if (out_f32) out_f32[i] = norm[v];
  }
}

int check_slope_range(const char* who, int A) {
  QEA_REQUIRE(A >= 0 && A <= QEA_DESKEW_MAX_SLOPE, "%s: A=%d outside 0..%d", who, A, QEA_DESKEW_MAX_SLOPE);
  return QEA_OK;
}

bool overlap(const void* a, unsigned long long na, const void* b, unsigned long long nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return a && b && x < y + nb && y < x + na;
}

}  // namespace

extern "C" int qea_skew_strip_sums(const void* store, int32_t store_is_f32, int64_t store_elems, const int64_t* offset, const int32_t* h,
                                   const int32_t* w, int32_t n_pages, const int32_t* host_h, const int32_t* host_w, const int32_t* ink_max_dev,
                                   int32_t ink_max, uint8_t* C, void* stream) {
  const char* who = "qea_skew_strip_sums";
  const PageStore ps = {(long long)store_elems, n_pages, offset, h, w};
  int max_h = 0;
  if (int rc = check_store(who, store, store_is_f32)) return rc;
  if (int rc = check_table(who, ps)) return rc;
  if (int rc = check_page_sizes(who, host_h, host_w, n_pages, QEA_DESKEW_MAX_SIDE, nullptr, nullptr, &max_h)) return rc;
  QEA_REQUIRE(C, "%s: C is NULL", who);
  QEA_REQUIRE(((uintptr_t)ink_max_dev & 3) == 0, "%s: ink_max_dev must be 4-byte aligned", who);
  QEA_REQUIRE(ink_max_dev || (ink_max >= 0 && ink_max <= 254), "%s: ink_max=%d outside 0..254", who, ink_max);
  QEA_REQUIRE(!overlap(store, (unsigned long long)store_elems * (store_is_f32 ? 4 : 1), C, (unsigned long long)store_elems),
              "%s: C overlaps the store", who);
  const long long blocks = (max_h + SUM_ROWS - 1) / SUM_ROWS, grid = blocks * n_pages;
  QEA_REQUIRE(grid <= 0x7fffffffll, "%s: %lld workgroups, more than 2^31 - 1", who, grid);
  dispatch_store(store_is_f32, store, [&](auto* typed) {
    strip_sums_kernel<<<dim3((unsigned)grid), dim3(THREADS), 0, (hipStream_t)stream>>>(typed, ps, (int)blocks, ink_max_dev, ink_max, C);
  });
  QEA_CHECK_LAUNCH();
  return QEA_OK;
}

extern "C" int qea_skew_scores(const uint8_t* C, int64_t store_elems, const int64_t* offset, const int32_t* h, const int32_t* w, int32_t n_pages,
                               const int32_t* host_h, const int32_t* host_w, int32_t A, int64_t* scores, void* stream) {
  const char* who = "qea_skew_scores";
  const PageStore ps = {(long long)store_elems, n_pages, offset, h, w};
  int max_h = 0;
  QEA_REQUIRE(C, "%s: C is NULL", who);
  if (int rc = check_table(who, ps)) return rc;
  if (int rc = check_page_sizes(who, host_h, host_w, n_pages, QEA_DESKEW_MAX_SIDE, nullptr, nullptr, &max_h)) return rc;
  if (int rc = check_slope_range(who, A)) return rc;
  QEA_REQUIRE(scores && ((uintptr_t)scores & 7) == 0, "%s: scores must be an 8-byte aligned table of n_pages x (2 A + 1) values", who);
  const long long blocks = (max_h + SCORE_ROWS - 1) / SCORE_ROWS, grid = blocks * n_pages;
  QEA_REQUIRE(grid <= 0x7fffffffll, "%s: %lld workgroups, more than 2^31 - 1", who, grid);
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(scores, 0, (size_t)n_pages * (2 * A + 1) * sizeof(int64_t), s) != hipSuccess) {
    qea_set_error("%s: cannot zero the scores", who);
    return QEA_ERR_LAUNCH;
  }
  scores_kernel<<<dim3((unsigned)grid, (unsigned)((2 * A + SCORE_CANDIDATES) / SCORE_CANDIDATES)), dim3(THREADS), 0, s>>>(
      C, ps, (int)blocks, A, (unsigned long long*)scores);
  QEA_CHECK_LAUNCH();
  return QEA_OK;
}

extern "C" int qea_skew_pick(const int64_t* scores, int32_t n_pages, int32_t A, int32_t g, int32_t* slopes, void* stream) {
  const char* who = "qea_skew_pick";
  QEA_REQUIRE(n_pages >= 1 && n_pages <= (1 << 24), "%s: n_pages=%d outside 1..2^24", who, n_pages);
  if (int rc = check_slope_range(who, A)) return rc;
  QEA_REQUIRE(g >= 0 && g <= QEA_DESKEW_MAX_GAIN, "%s: g=%d outside 0..%d", who, g, QEA_DESKEW_MAX_GAIN);
  QEA_REQUIRE(scores && ((uintptr_t)scores & 7) == 0, "%s: scores must be an 8-byte aligned table of n_pages x (2 A + 1) values", who);
  QEA_REQUIRE(slopes && ((uintptr_t)slopes & 3) == 0, "%s: slopes must be a 4-byte aligned array of n_pages values", who);
  pick_kernel<<<dim3((unsigned)n_pages), dim3(64), 0, (hipStream_t)stream>>>((const long long*)scores, A, g, slopes);
  QEA_CHECK_LAUNCH();
  return QEA_OK;
}

extern "C" int qea_deskew_rotate(const void* store, int32_t store_is_f32, int64_t store_elems, const int64_t* offset, const int32_t* h,
                                 const int32_t* w, int32_t n_pages, const int32_t* host_h, const int32_t* host_w, const int32_t* tile_first,
                                 const int32_t* slopes, const int32_t* table, int32_t A, int32_t nearest, int32_t fill, const float* norm,
                                 float* out_f32, uint8_t* out_u8, void* stream) {
  const char* who = "qea_deskew_rotate";
  const PageStore ps = {(long long)store_elems, n_pages, offset, h, w};
  long long tiles = 0;
  if (int rc = check_store(who, store, store_is_f32)) return rc;
  if (int rc = check_table(who, ps)) return rc;
  if (int rc = check_page_sizes(who, host_h, host_w, n_pages, QEA_DESKEW_MAX_SIDE, &tiles, nullptr, nullptr)) return rc;
  if (int rc = check_slope_range(who, A)) return rc;
  QEA_REQUIRE(tile_first, "%s: null pointer", who);
  QEA_REQUIRE(slopes && ((uintptr_t)slopes & 3) == 0, "%s: slopes must be a 4-byte aligned array of n_pages values", who);
  QEA_REQUIRE(table && ((uintptr_t)table & 3) == 0, "%s: table must be a 4-byte aligned array of (2 A + 1) x 2 values", who);
  QEA_REQUIRE(nearest == 0 || nearest == 1, "%s: nearest=%d is neither 0 nor 1", who, nearest);
  QEA_REQUIRE(fill >= 0 && fill <= 255, "%s: fill=%d outside 0..255", who, fill);
  if (int rc = check_outputs(who, out_f32, out_u8)) return rc;
  QEA_REQUIRE(!out_f32 || (norm && ((uintptr_t)norm & 3) == 0), "%s: out_f32 needs the 4-byte aligned table norm of 256 values", who);
  const unsigned long long bytes = (unsigned long long)store_elems * (store_is_f32 ? 4 : 1);
  QEA_REQUIRE(!overlap(store, bytes, out_u8, (unsigned long long)store_elems) && !overlap(store, bytes, out_f32, 4ull * store_elems),
              "%s: an output overlaps the store (the rotation reads pixels that other workgroups write)", who);
  dispatch_store(store_is_f32, store, [&](auto* typed) {
    rotate_kernel<<<dim3((unsigned)tiles), dim3(THREADS), 0, (hipStream_t)stream>>>(typed, ps, tile_first, slopes, table, A, nearest, fill, norm,
                                                                                    out_f32, out_u8);
  });
  QEA_CHECK_LAUNCH();
  return QEA_OK;
}
