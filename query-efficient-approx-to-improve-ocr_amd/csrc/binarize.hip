// Classic binarisers over the packed page store, bit for bit the statement tests/binarize_spec.py (include/qea_hip.h: qea_binarize_sauvola,
// qea_otsu_histogram, qea_binarize_otsu; qea/binarize.py: binarize_pages, whose host path is the same statement in numpy).
//
// A pixel is its 8-bit value v (csrc/page_store.h: value_of); ink is foreground and is written as 0 / 0.0, background as 255 / 1.0, into
// outputs packed like the store (put_ink).  Every sum is an integer, so no order of summation
// matters; the two decisions are fp64 products and one subtraction, compiled without fused multiply-adds.
//
// sauvola_kernel: ONE launch for all pages.  Workgroup b owns one TH x TW output tile of one page (csrc/page_store.h: tile_of_block).
// With r = win / 2 the LDS plan is
//     px  [TH + 2r][PB] bytes       the tile and its halo, 0 outside the page; PB = the row length rounded up to 4 with PB / 4 odd
//     H1  [TH + 2r][TW + 1] uint32  sums of v over the win columns around each of the tile's columns (<= 127 * 255)
//     H2  [TH + 2r][TW + 1] uint32  sums of v * v (<= 127 * 65025)
// 30968 + 2 * 41080 = 113128 B at win = 127 (one workgroup per CU), 34272 B at win = 25 (four).  Staging: wave i takes rows i, i + 4, ..., lane l
// columns l, l + 64, ...: byte loads of consecutive addresses.  Row pass: wave i owns the tile's columns 16 i .. 16 i + 15 and lane l rows
// l, l + 64, ...: a window sum of win bytes, then 15 steps of +1 byte -1 byte.  The lanes of a wave differ in the row only, and both pitches are
// an odd number of words, so neither the byte reads nor the H stores meet on a bank.  Column pass: thread (column l, row group i) sums win rows
// of H1 / H2 for output row 8 i and slides down seven times; a wave reads 64 consecutive words.  S2 <= 127 * 127 * 65025 < 2^32; n * S2 is
// formed in 64 bits.  n, the window's pixel count inside the page, is the product of the two clipped extents.
//
// otsu_histogram_kernel / otsu_apply_kernel: a page is one contiguous run of h * w elements, so both walk it in chunks of QEA_BINARIZE_CHUNK
// elements; workgroup b owns chunk b - chunk_first[p] of page p.  The first counts its chunk into four LDS histograms (one per wave) and adds
// the non-zero bins to hist[p][256] with integer atomics: the table is the same whatever the order.  The second reads the page's 256 bins,
// forms w0 / s0 by an LDS scan, num / den per threshold in parallel, and lets ONE thread walk the replace-if-greater chain in ascending t —
// rounded fp64 products need not be transitive, so the chain is the statement's, not a tournament — then thresholds its chunk.  The workgroup
// of chunk 0 also writes t* (or -1) to thresholds[p].
//
// All three skip a page that does not lie inside the store and a tile / chunk that does not lie inside its page: tables that disagree
// with the host's give unwritten outputs, never an access outside the caller's buffers.
#include "page_store.h"

namespace {

constexpr int TH = QEA_BINARIZE_TILE_H, TW = QEA_BINARIZE_TILE_W, HP = TW + 1, THREADS = 256, CHUNK = QEA_BINARIZE_CHUNK;
static_assert(TW == 64 && TH == 32 && THREADS == 256, "the passes below give a wave 16 columns / 8 rows of the tile and a lane one column");

__host__ __device__ constexpr int byte_pitch(int win) { return (((TW + win - 1 + 3) / 4) | 1) * 4; }
__host__ __device__ constexpr int sauvola_lds_bytes(int win) { return (TH + win - 1) * (byte_pitch(win) + 2 * HP * 4); }
static_assert(sauvola_lds_bytes(QEA_BINARIZE_MAX_WINDOW) <= 160 * 1024, "the plan must fit the CU's LDS at the largest window");

// The statement's rule: foreground iff v <= m (1 + k (s / R - 1)), without sqrt or division, every operation rounded as written.
__device__ __forceinline__ bool sauvola_foreground(int n, int v, unsigned S1, unsigned S2, double k, double R) {
#pragma clang fp contract(off)
  const long long Q = (long long)n * (long long)S2 - (long long)S1 * (long long)S1;
  const double A = (double)(n * v) - (double)S1 * (1.0 - k);
  if (A <= 0.0) return true;
  const double L = A * (R * (double)n), G = k * (double)S1;
  return L * L <= (G * G) * (double)Q;
}

template <typename T>
__global__ __launch_bounds__(THREADS) void sauvola_kernel(const T* __restrict__ store, const PageStore ps,
                                                          const int32_t* __restrict__ tile_first, int win, double k, double R,
                                                          float* __restrict__ out_f32, uint8_t* __restrict__ out_u8) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int r = win >> 1, SH = TH + 2 * r, SW = TW + 2 * r, PB = byte_pitch(win);
  unsigned char* const px = lds;
  unsigned* const H1 = reinterpret_cast<unsigned*>(lds + SH * PB);        // SH * PB is a multiple of 4
  unsigned* const H2 = H1 + SH * HP;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

  const Tile t = tile_of_block(ps, tile_first, TH, TW);
  if (t.g.h == 0) return;                                      // uniform
  const Page g = t.g;
  const int ty0 = t.y0, tx0 = t.x0;

  for (int sy = wave; sy < SH; sy += 4) {
    const int py = ty0 - r + sy;
    const bool row_in = py >= 0 && py < g.h;
    for (int sx = lane; sx < SW; sx += 64) {
      const int qx = tx0 - r + sx;
      px[sy * PB + sx] = row_in && qx >= 0 && qx < g.w ? (uint8_t)value_of(store[g.off + (long long)py * g.w + qx]) : (uint8_t)0;
    }
  }
  __syncthreads();

  for (int sy = lane; sy < SH; sy += 64) {
    const unsigned char* row = px + sy * PB + 16 * wave;       // the window of tile column c is row[c .. c + win - 1]
    unsigned s1 = 0, s2 = 0;
    for (int j = 0; j < win; ++j) {
      const unsigned b = row[j];
      s1 += b;
      s2 += b * b;
    }
    unsigned* o1 = H1 + sy * HP + 16 * wave;
    unsigned* o2 = H2 + sy * HP + 16 * wave;
    o1[0] = s1;
    o2[0] = s2;
#pragma unroll
    for (int c = 1; c < 16; ++c) {
      const unsigned a = row[c + win - 1], d = row[c - 1];
      s1 += a - d;
      s2 += a * a - d * d;                                     // modulo 2^32; the sum itself never leaves 0 .. 127 * 65025
      o1[c] = s1;
      o2[c] = s2;
    }
  }
  __syncthreads();

  const int y0 = 8 * wave, qx = tx0 + lane;
  unsigned S1 = 0, S2 = 0;
  for (int j = 0; j < win; ++j) {
    S1 += H1[(y0 + j) * HP + lane];
    S2 += H2[(y0 + j) * HP + lane];
  }
  const int nx = min(qx + r, g.w - 1) - max(qx - r, 0) + 1;
  for (int y = y0;; ++y) {
    const int py = ty0 + y;
    if (py < g.h && qx < g.w) {
      const int n = nx * (min(py + r, g.h - 1) - max(py - r, 0) + 1);
      put_ink(out_f32, out_u8, g.off + (long long)py * g.w + qx, sauvola_foreground(n, px[(y + r) * PB + lane + r], S1, S2, k, R));
    }
    if (y == y0 + 7) break;
    S1 += H1[(y + win) * HP + lane] - H1[y * HP + lane];
    S2 += H2[(y + win) * HP + lane] - H2[y * HP + lane];
  }
}

struct Chunk {
  Page g;
  int page;
  long long begin, end;      // elements of the page this workgroup owns; begin >= end: nothing
};

__device__ __forceinline__ Chunk chunk_of_block(const PageStore& ps, const int32_t* __restrict__ chunk_first) {
  Chunk c;
  c.page = page_of_block(chunk_first, ps.n_pages, blockIdx.x);
  c.g = page_of(ps, c.page);
  const long long size = (long long)c.g.h * c.g.w, at = (long long)((int)blockIdx.x - chunk_first[c.page]) * CHUNK;
  c.begin = at < 0 ? size : at;
  c.end = min(size, c.begin + CHUNK);
  return c;
}

template <typename T>
__global__ __launch_bounds__(THREADS) void otsu_histogram_kernel(const T* __restrict__ store, const PageStore ps,
                                                                 const int32_t* __restrict__ chunk_first, unsigned* __restrict__ hist) {
  __shared__ unsigned bins[4][256];
  const Chunk c = chunk_of_block(ps, chunk_first);
  if (c.begin >= c.end) return;                                // uniform
  for (int i = threadIdx.x; i < 4 * 256; i += THREADS) (&bins[0][0])[i] = 0;
  __syncthreads();
  unsigned* mine = bins[threadIdx.x >> 6];
  for (long long i = c.begin + threadIdx.x; i < c.end; i += THREADS) atomicAdd(&mine[value_of(store[c.g.off + i])], 1u);
  __syncthreads();
  const unsigned n = bins[0][threadIdx.x] + bins[1][threadIdx.x] + bins[2][threadIdx.x] + bins[3][threadIdx.x];
  if (n) atomicAdd(&hist[(long long)c.page * 256 + threadIdx.x], n);
}

// t* of 256 bins by the statement: the first valid t starts the chain, a later one replaces the best iff num * den_best > num_best * den.
// Every thread of the workgroup calls this with its bin; every thread returns t* (-1: a single grey level).
__device__ __forceinline__ int otsu_threshold(unsigned bin) {
#pragma clang fp contract(off)
  __shared__ unsigned w0s[2][256];
  __shared__ long long s0s[2][256];
  __shared__ double nums[256], dens[256];
  __shared__ int best;
  const int t = threadIdx.x;
  int cur = 0;
  w0s[0][t] = bin;
  s0s[0][t] = (long long)t * bin;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1, cur ^= 1) {                // inclusive scan: w0[t] = sum hist[..t], s0[t] = sum v hist[v]
    w0s[cur ^ 1][t] = w0s[cur][t] + (t >= d ? w0s[cur][t - d] : 0u);
    s0s[cur ^ 1][t] = s0s[cur][t] + (t >= d ? s0s[cur][t - d] : 0ll);
    __syncthreads();
  }
  const long long N = w0s[cur][255], S = s0s[cur][255], w0 = w0s[cur][t], w1 = N - w0;
  const long long d = s0s[cur][t] * N - S * w0;                // |d| <= 255 N^2 < 2^63 for N <= 2^27
  nums[t] = (double)d * (double)d;
  dens[t] = w0 > 0 && w1 > 0 ? (double)w0 * (double)w1 : 0.0;  // 0: not a valid threshold
  __syncthreads();
  if (t == 0) {
    int b = -1;
    double nb = 0.0, db = 0.0;
    for (int u = 0; u < 255; ++u) {
      const double nu = nums[u], du = dens[u];
      if (du > 0.0 && (b < 0 || nu * db > nb * du)) {
        b = u;
        nb = nu;
        db = du;
      }
    }
    best = b;
  }
  __syncthreads();
  return best;
}

template <typename T>
__global__ __launch_bounds__(THREADS) void otsu_apply_kernel(const T* __restrict__ store, const PageStore ps,
                                                             const int32_t* __restrict__ chunk_first, const unsigned* __restrict__ hist,
                                                             float* __restrict__ out_f32, uint8_t* __restrict__ out_u8,
                                                             int32_t* __restrict__ thresholds) {
  const Chunk c = chunk_of_block(ps, chunk_first);
  if (c.begin >= c.end) return;                                // uniform
  const int ts = otsu_threshold(hist[(long long)c.page * 256 + threadIdx.x]);
  if (c.begin == 0 && threadIdx.x == 0) thresholds[c.page] = ts;
  for (long long i = c.begin + threadIdx.x; i < c.end; i += THREADS)
    put_ink(out_f32, out_u8, c.g.off + i, value_of(store[c.g.off + i]) <= ts);
}

}  // namespace

extern "C" int qea_binarize_sauvola(const void* store, int32_t store_is_f32, int64_t store_elems, const int64_t* offset, const int32_t* h,
                                    const int32_t* w, int32_t n_pages, const int32_t* host_h, const int32_t* host_w, const int32_t* tile_first,
                                    int32_t win, double k, double R, float* out_f32, uint8_t* out_u8, void* stream) {
  const char* who = "qea_binarize_sauvola";
  const PageStore ps = {(long long)store_elems, n_pages, offset, h, w};
  long long blocks = 0;
  if (int rc = check_paged_launch(who, store, store_is_f32, ps, host_h, host_w, tile_first, true, &blocks)) return rc;
  if (int rc = check_outputs(who, out_f32, out_u8)) return rc;
  QEA_REQUIRE(win >= 3 && win <= QEA_BINARIZE_MAX_WINDOW && win % 2 == 1, "%s: window %d must be odd and in 3..%d", who, win,
              QEA_BINARIZE_MAX_WINDOW);
  QEA_REQUIRE(k > 0.0 && k < 1.0, "%s: k=%g must lie strictly between 0 and 1", who, k);       // false for NaN
  QEA_REQUIRE(R > 0.0 && R <= 1.7976931348623157e308, "%s: R=%g must be positive and finite", who, R);
  const int reserved = dispatch_store(store_is_f32, store, [&](auto* typed) {
    // reserve_lds takes the kernel as a template argument, so the instance needs a constant name: the call alone would not pick it
    constexpr auto kernel = sauvola_kernel<StoreElem<decltype(typed)>>;
    const int rc = reserve_lds<kernel>(who, sauvola_lds_bytes(QEA_BINARIZE_MAX_WINDOW));
    if (rc == QEA_OK)
      kernel<<<dim3((unsigned)blocks), dim3(THREADS), sauvola_lds_bytes(win), (hipStream_t)stream>>>(typed, ps, tile_first, win, k, R, out_f32,
                                                                                                    out_u8);
    return rc;
  });
  if (reserved != QEA_OK) return reserved;
  QEA_CHECK_LAUNCH();
  return QEA_OK;
}

extern "C" int qea_otsu_histogram(const void* store, int32_t store_is_f32, int64_t store_elems, const int64_t* offset, const int32_t* h,
                                  const int32_t* w, int32_t n_pages, const int32_t* host_h, const int32_t* host_w, const int32_t* chunk_first,
                                  uint32_t* hist, void* stream) {
  const char* who = "qea_otsu_histogram";
  const PageStore ps = {(long long)store_elems, n_pages, offset, h, w};
  long long blocks = 0;
  if (int rc = check_paged_launch(who, store, store_is_f32, ps, host_h, host_w, chunk_first, false, &blocks)) return rc;
  QEA_REQUIRE(hist && ((uintptr_t)hist & 3) == 0, "%s: hist must be a 4-byte aligned table of n_pages x 256 counts", who);
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(hist, 0, (size_t)n_pages * 256 * sizeof(uint32_t), s) != hipSuccess) {
    qea_set_error("%s: cannot zero the histogram table", who);
    return QEA_ERR_LAUNCH;
  }
  dispatch_store(store_is_f32, store, [&](auto* typed) {
    otsu_histogram_kernel<<<dim3((unsigned)blocks), dim3(THREADS), 0, s>>>(typed, ps, chunk_first, hist);
  });
  QEA_CHECK_LAUNCH();
  return QEA_OK;
}

extern "C" int qea_binarize_otsu(const void* store, int32_t store_is_f32, int64_t store_elems, const int64_t* offset, const int32_t* h,
                                 const int32_t* w, int32_t n_pages, const int32_t* host_h, const int32_t* host_w, const int32_t* chunk_first,
                                 const uint32_t* hist, float* out_f32, uint8_t* out_u8, int32_t* thresholds, void* stream) {
  const char* who = "qea_binarize_otsu";
  const PageStore ps = {(long long)store_elems, n_pages, offset, h, w};
  long long blocks = 0;
  if (int rc = check_paged_launch(who, store, store_is_f32, ps, host_h, host_w, chunk_first, false, &blocks)) return rc;
  if (int rc = check_outputs(who, out_f32, out_u8)) return rc;
  QEA_REQUIRE(hist && ((uintptr_t)hist & 3) == 0, "%s: hist must be the 4-byte aligned table qea_otsu_histogram filled", who);
  QEA_REQUIRE(thresholds && ((uintptr_t)thresholds & 3) == 0, "%s: thresholds must be a 4-byte aligned array of n_pages values", who);
  dispatch_store(store_is_f32, store, [&](auto* typed) {
    otsu_apply_kernel<<<dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream>>>(typed, ps, chunk_first, hist, out_f32, out_u8,
                                                                                         thresholds);
  });
  QEA_CHECK_LAUNCH();
  return QEA_OK;
}
