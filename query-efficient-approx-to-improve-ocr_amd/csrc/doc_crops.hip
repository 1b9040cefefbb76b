// All text strips of a training step cut out of its documents in one launch, and their gradient put back in one launch
// (include/qea_hip.h: qea_doc_crops_gather / qea_doc_crops_scatter; datasets/resident.py: ResidentDocuments.crops).
//
// The resident document store keeps the clipped word boxes of every document in one table (box[total][4] = x0, y0, x1, y1; the boxes
// of document d are rows box_first[d] .. box_first[d+1]-1).  A step works on N documents, image n being store row doc[n]; its strips
// are all boxes of its documents, document after document and box after box: strip s belongs to the image n with
// strip_first[n] <= s < strip_first[n+1] and is box s - strip_first[n] of that document.
//
// doc_crops_gather_kernel: the values of crop_pad_gather_kernel (csrc/misc.hip) for that image and box, the white ground and the
// floor division of an oversize crop included, as a window gather (csrc/window_gather.h: lanes, reads, store and the bad-table rule).
// The strip is uniform over the workgroup: its image number (a binary search in strip_first) and its four box words are scalar loads.
//
// doc_crops_scatter_kernel: the backward in GATHER form.  Each lane owns four neighbouring pixels of dimg[N][H][W] (W % 4 == 0), a
// workgroup a 16 x 64 tile of one image.  The workgroup first culls the document's boxes against its tile: 256 boxes at a time, a
// lane per box, the survivors compacted into an LDS list IN ASCENDING BOX ORDER (ballot + prefix count inside a wave, the four wave
// totals through LDS); a document with more boxes goes through the list in several chunks.  Every lane then walks the list (all lanes
// read the same LDS words: a broadcast, no bank conflict) and adds the dout element of every box that covers its pixel, lowest box
// first, starting from 0.  Each pixel is written once: the sum, or with `accumulate` dimg + sum; a pixel no box covers gets 0.  No
// atomics: the result is fixed by the inputs, and for boxes that do not overlap it is 0 + dout = what memset + crop_pad_scatter_kernel
// leave.  Index arithmetic inside an image or a strip is 32-bit.
#include "window_gather.h"

namespace {

constexpr int DC_THREADS = 256;
constexpr int DC_TILE_W = 64, DC_TILE_H = 16;          // pixels of dimg per workgroup: 16 quads x 16 rows = 256 lanes
constexpr int DC_LIST = DC_THREADS;                    // boxes culled per chunk, a lane each

// image n of strip s: the last n in 0..N-1 with strip_first[n] <= s (uniform: scalar loads)
__device__ __forceinline__ int image_of(const int32_t* __restrict__ strip_first, int N, int s) {
  int lo = 0, hi = N;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (strip_first[mid] <= s) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(WG_THREADS) void doc_crops_gather_kernel(const float* __restrict__ imgs, int N, int H, int W,
                                                                      const int32_t* __restrict__ box, const int32_t* __restrict__ box_first,
                                                                      int n_docs, int n_boxes, const int64_t* __restrict__ doc,
                                                                      const int32_t* __restrict__ strip_first, int S, int OH, int OW,
                                                                      float* __restrict__ out) {
  window_gather(imgs, (const float*)nullptr, out, S, OH, OW, [=](int s) {
    Window win = {};
    const int n = image_of(strip_first, N, s);
    const int j = s - strip_first[n];
    const int64_t d = doc[n];
    if (j >= 0 && d >= 0 && d < n_docs) {              // anything else: an all-white strip
      const int first = box_first[d], bi = first + j;
      if (first >= 0 && bi < box_first[d + 1] && bi < n_boxes) {
        const Footprint f = footprint(box + 4 * bi, H, W, OH, OW);
        win = {(long long)n * H * W - (f.dy * W + f.dx), W, f.fx0 + f.dx, f.fy0 + f.dy, f.fx1 + f.dx, f.fy1 + f.dy};
      }
    }
    return win;
  });
}

struct Culled {
  int fx0, fy0, fx1, fy1;
  int off;      // dout element of image pixel (px, py), relative to the strip: off + py * OW + px
  int strip;
};

__global__ __launch_bounds__(DC_THREADS) void doc_crops_scatter_kernel(const float* __restrict__ dout, int S, int OH, int OW,
                                                                       const int32_t* __restrict__ box, const int32_t* __restrict__ box_first,
                                                                       int n_docs, int n_boxes, const int64_t* __restrict__ doc,
                                                                       const int32_t* __restrict__ strip_first, float* __restrict__ dimg, int N,
                                                                       int H, int W, int tiles_x, int accumulate) {
  __shared__ Culled list[DC_LIST];
  __shared__ int wave_count[DC_THREADS / QEA_WAVE];
  const int tid = threadIdx.x, lane = tid & (QEA_WAVE - 1), wave = tid / QEA_WAVE;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int tile_x0 = tx * DC_TILE_W, tile_y0 = ty * DC_TILE_H;
  const int tile_x1 = min(tile_x0 + DC_TILE_W, W), tile_y1 = min(tile_y0 + DC_TILE_H, H);
  const int px0 = tile_x0 + ((tid & 15) << 2), py = tile_y0 + (tid >> 4);       // this lane's four pixels: a wave covers 4 rows x 256 B
  const bool mine = px0 < W && py < H;                                          // W % 4 == 0: a quad is inside the row or outside it
  const size_t strip_el = (size_t)OH * OW;
  for (int n = blockIdx.y; n < N; n += gridDim.y) {                             // uniform over the workgroup
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const int64_t d = doc[n];
    int first = 0, nb = 0;
    const int s0 = strip_first[n];
    if (d >= 0 && d < n_docs && s0 >= 0) {
      first = box_first[d];
      nb = min(box_first[d + 1] - first, strip_first[n + 1] - s0);
      if (first < 0) nb = 0;
      nb = min(nb, min(n_boxes - first, S - s0));                               // every box and every strip read below exists
    }
    for (int c0 = 0; c0 < nb; c0 += DC_LIST) {
      // ---- cull boxes c0 .. c0 + 255 against the tile, a lane per box
      const int j = c0 + tid;
      Culled e;
      bool hit = false;
      if (j < nb) {
        const Footprint f = footprint(box + 4 * (first + j), H, W, OH, OW);
        hit = f.fx0 < f.fx1 && f.fy0 < f.fy1 && f.fx0 < tile_x1 && f.fx1 > tile_x0 && f.fy0 < tile_y1 && f.fy1 > tile_y0;
        e.fx0 = f.fx0; e.fy0 = f.fy0; e.fx1 = f.fx1; e.fy1 = f.fy1;
        e.off = f.dy * OW + f.dx;
        e.strip = s0 + j;
      }
      const unsigned long long votes = __ballot(hit);
      if (lane == 0) wave_count[wave] = __popcll(votes);
      __syncthreads();
      int before = __popcll(votes & ((1ull << lane) - 1ull)), count = 0;
#pragma unroll
      for (int w = 0; w < DC_THREADS / QEA_WAVE; ++w) {
        const int c = wave_count[w];
        if (w < wave) before += c;
        count += c;
      }
      if (hit) list[before] = e;                                                // ascending box order: waves, then lanes
      __syncthreads();
      // ---- every lane adds what the surviving boxes give its pixels, lowest box first
      if (mine) {
        for (int i = 0; i < count; ++i) {
          const Culled b = list[i];
          if (py >= b.fy0 && py < b.fy1) {
            const float* src = dout + (size_t)b.strip * strip_el + (b.off + py * OW);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const int px = px0 + k;
              if (px >= b.fx0 && px < b.fx1) acc[k] += src[px];
            }
          }
        }
      }
      __syncthreads();                                                          // the list and the counts are rewritten by the next chunk
    }
    if (mine) {
      f32x4* dst = reinterpret_cast<f32x4*>(dimg + (size_t)n * H * W + (py * W + px0));
      if (accumulate) {
        const f32x4 old = *dst;
        acc = old + acc;
      }
      *dst = acc;
    }
  }
}

int check_tables(const char* who, const void* box, const void* box_first, const void* doc, const void* strip_first, int n_docs, int n_boxes, int N,
                 int H, int W, int S, int OH, int OW) {
  QEA_REQUIRE(box && box_first && doc && strip_first, "%s: null pointer", who);
  QEA_REQUIRE(n_docs >= 1 && n_boxes >= 1, "%s: %d documents with %d boxes in the store", who, n_docs, n_boxes);
  QEA_REQUIRE(N >= 1 && N <= (1 << 16), "%s: N=%d outside 1..2^16", who, N);
  QEA_REQUIRE(H >= 1 && H <= 8192, "%s: H=%d outside 1..8192", who, H);
  QEA_REQUIRE(W >= 4 && W <= 8192 && W % 4 == 0, "%s: W=%d must be a multiple of 4 in 4..8192", who, W);
  QEA_REQUIRE(S >= 1 && S <= (1 << 24), "%s: S=%d outside 1..2^24", who, S);
  QEA_REQUIRE(OH >= 1 && OH <= 4096, "%s: OH=%d outside 1..4096", who, OH);
  QEA_REQUIRE(OW >= 4 && OW <= 8192 && OW % 4 == 0, "%s: OW=%d must be a multiple of 4 in 4..8192", who, OW);
  return QEA_OK;
}

}  // namespace

extern "C" int qea_doc_crops_gather(const float* imgs, int32_t N, int32_t H, int32_t W, const int32_t* box, const int32_t* box_first,
                                    int32_t n_docs, int32_t n_boxes, const int64_t* doc, const int32_t* strip_first, int32_t S, int32_t OH,
                                    int32_t OW, float* out, void* stream) {
  QEA_REQUIRE(imgs && out, "qea_doc_crops_gather: null pointer");
  if (int rc = check_tables("qea_doc_crops_gather", box, box_first, doc, strip_first, n_docs, n_boxes, N, H, W, S, OH, OW)) return rc;
  QEA_REQUIRE(((uintptr_t)out & 15) == 0, "qea_doc_crops_gather: out must be 16-byte aligned");
  launch_over_quads(doc_crops_gather_kernel, S, OH, OW, stream, imgs, N, H, W, box, box_first, n_docs, n_boxes, doc, strip_first, S, OH, OW, out);
  QEA_CHECK_LAUNCH();
  return QEA_OK;
}

extern "C" int qea_doc_crops_scatter(const float* dout, int32_t S, int32_t OH, int32_t OW, const int32_t* box, const int32_t* box_first,
                                     int32_t n_docs, int32_t n_boxes, const int64_t* doc, const int32_t* strip_first, float* dimg, int32_t N,
                                     int32_t H, int32_t W, int32_t accumulate, void* stream) {
  QEA_REQUIRE(dout && dimg, "qea_doc_crops_scatter: null pointer");
  if (int rc = check_tables("qea_doc_crops_scatter", box, box_first, doc, strip_first, n_docs, n_boxes, N, H, W, S, OH, OW)) return rc;
  QEA_REQUIRE(accumulate == 0 || accumulate == 1, "qea_doc_crops_scatter: accumulate=%d is neither 0 nor 1", accumulate);
  QEA_REQUIRE(((uintptr_t)dimg & 15) == 0, "qea_doc_crops_scatter: dimg must be 16-byte aligned");
  const int tiles_x = qea_cdiv(W, DC_TILE_W), tiles_y = qea_cdiv(H, DC_TILE_H);            // at most 128 x 512 tiles per image
  const dim3 grid(tiles_x * tiles_y, N < 65535 ? N : 65535);
  hipLaunchKernelGGL(doc_crops_scatter_kernel, grid, dim3(DC_THREADS), 0, (hipStream_t)stream, dout, S, OH, OW, box, box_first, n_docs, n_boxes,
                     doc, strip_first, dimg, N, H, W, tiles_x, accumulate);
  QEA_CHECK_LAUNCH();
  return QEA_OK;
}
