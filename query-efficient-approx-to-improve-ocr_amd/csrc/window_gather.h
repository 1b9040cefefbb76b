// The window gather: a rectangle of a source image copied into a fixed-size fp32 image on a white (1.0) ground.  strip_batch_kernel
// (strip_batch.hip), doc_crops_gather_kernel (doc_crops.hip) and page_tiles_gather_kernel (page_tiles.hip) are this body behind three
// resolvers; the crop geometry they share with the crop_pad kernels (misc.hip) and doc_crops_scatter_kernel is here as well.
//
//
// The contract ("The window gather", has the reasons): ONE launch writes every element of out[n][OH][OW]
// (OW % 4 == 0).  One lane per quad of four neighbouring pixels of an output row and one 16-byte store per lane; grid.x walks the
// OH * OW / 4 quads of an image, grid.y strides over the images.  The image is uniform over the workgroup: the resolver gets the image
// number alone, never anything of the lane, so its table reads are scalar loads and the Window it returns sits in scalar registers.
// The four source elements of a quad are read one by one, each only inside the window; bytes go through the caller's 256-entry
// table (p / 255 as the HOST rounds it), fp32 is copied.  Nothing is staged in LDS.  A bad table resolves to the EMPTY window: an
// all-white image, never an access outside the caller's buffers.
#pragma once
#include "common.h"

constexpr int WG_THREADS = 256;

// ---- the lanes: quad q of an OH x OW image, row-major -> its row y and first column x; false past the last quad
__device__ __forceinline__ bool quad_of(int OH, int OW, int& q, int& y, int& x) {
  const int qw = OW >> 2;                              // quads per row
  q = blockIdx.x * WG_THREADS + threadIdx.x;
  if (q >= OH * qw) return false;
  y = q / qw;
  x = (q - y * qw) << 2;
  return true;
}
// element of quad q of image i in an [n][OH][OW] array
__device__ __forceinline__ size_t quad_element(int i, int OH, int OW, int q) { return ((size_t)i * OH * (OW >> 2) + q) << 2; }

// ---- what an output image shows of its source, uniform over the workgroup: output pixel (x, y) with x0 <= x < x1 and y0 <= y < y1 is
// source element origin + y * pitch + x (the shift from output to source coordinates is folded into the origin, in 64 bits), every
// other pixel is white.  The rectangle lies inside the output; an empty one is an all-white image.
struct Window {
  long long origin;
  int pitch;
  int x0, y0, x1, y1;
};

template <typename T, typename Resolve>
__device__ __forceinline__ void window_gather(const T* __restrict__ src, const float* __restrict__ table, float* __restrict__ out, int n, int OH,
                                              int OW, Resolve resolve) {
  int q, y, x;
  if (!quad_of(OH, OW, q, y, x)) return;
  for (int i = blockIdx.y; i < n; i += gridDim.y) {    // uniform over the workgroup: the resolver's loads are scalar loads
    const Window win = resolve(i);
    f32x4 v = {1.f, 1.f, 1.f, 1.f};
    if (y >= win.y0 && y < win.y1) {
      const T* row = src + (win.origin + (long long)y * win.pitch);   // columns x0..x1-1 of it are read
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (x + k >= win.x0 && x + k < win.x1) {
          if constexpr (sizeof(T) == 1) v[k] = table[row[x + k]];
          else v[k] = row[x + k];
        }
      }
    }
    *reinterpret_cast<f32x4*>(out + quad_element(i, OH, OW, q)) = v;
  }
}

// the launch of a kernel that walks the quads of n images of OH x OW: OH * OW / 4 <= 2^24 quads per image
template <typename Kernel, typename... Args>
static inline void launch_over_quads(Kernel kernel, int n, int OH, int OW, void* stream, Args... args) {
  const dim3 grid(qea_cdiv((long long)OH * (OW / 4), WG_THREADS), n < 65535 ? n : 65535);
  hipLaunchKernelGGL(kernel, grid, dim3(WG_THREADS), 0, (hipStream_t)stream, args...);
}

// ---- crop + pad geometry (padder of utils.py): a box centred in an OH x OW target
// Python floor division: a crop larger than the target by an odd amount loses the EXTRA pixel on the left/top (negative padding), where
// C's truncation would take it from the right/bottom
__device__ __forceinline__ int qea_floordiv2(int d) { return d >= 0 ? d / 2 : -((-d + 1) / 2); }

// What a strip reads of its image: the box cut to what an OH x OW target keeps of it.  Output element (ox, oy) of the strip is image
// pixel (ox - dx, oy - dy) where that lies in [fx0, fx1) x [fy0, fy1), white elsewhere.
struct Footprint {
  int fx0, fy0, fx1, fy1, dx, dy;
};

__device__ __forceinline__ Footprint footprint(int x0, int y0, int x1, int y1, int OH, int OW) {
  const int cw = x1 - x0, ch = y1 - y0;
  const int left = qea_floordiv2(OW - cw), top = qea_floordiv2(OH - ch);
  Footprint f;
  f.fx0 = x0 + max(0, -left);
  f.fx1 = x0 + min(cw, OW - left);
  f.fy0 = y0 + max(0, -top);
  f.fy1 = y0 + min(ch, OH - top);
  f.dx = left - x0;
  f.dy = top - y0;
  return f;
}
// the box words clipped to the H x W image first: in bounds whatever they hold
__device__ __forceinline__ Footprint footprint(const int32_t* __restrict__ b, int H, int W, int OH, int OW) {
  return footprint(max(b[0], 0), max(b[1], 0), min(b[2], W), min(b[3], H), OH, OW);
}
