// Word boxes grouped into text lines and put into reading order, bit for bit the statement tests/lines_spec.py (include/qea_hip.h:
// qea_line_group; qea/lines.py is the product interface, whose host path is the same statement in numpy; DESIGN.md "Text lines").
//
// ONE launch, ONE workgroup of 1024 threads per page, whatever the pages hold; thread t owns the boxes t, t + 1024, ... of its page (at
// most four: QEA_LINE_MAX_BOXES = 4096) and keeps them in registers.  Everything is an integer and every product is 64-bit, so nothing
// depends on an order of evaluation.  The steps, a barrier between each:
//   median     m = the number of non-empty boxes (one LDS counter); a non-empty box's rank among the heights is the number of non-empty
//              boxes j with (h_j, j) < (h_i, i), counted in one scan over the page; the box of rank (m - 1) div 2 publishes med.
//   neighbours one scan over the page per box: among the linkable boxes j in its height band, the smallest key (x_min_j, j) above its own
//              is succ, the largest below it is pred; the gap rule then keeps or drops each of the two links.
//   lines      every box is united with its succ and its pred in a min-index union-find in LDS (csrc/union_find.h): no round loop, every
//              walk moves to a strictly smaller index.  A line's root is its smallest box index, as the statement asks.
//   line boxes four LDS atomics per box into its root's row.
//   line order a root's rank among the roots under (y_min + y_max, x_min, root), counted in one scan over the roots in LDS.
//   box order  a box's rank under (line, x_min, y_min, index), counted in one scan over the page.
// The page's boxes are staged in LDS once: a scan reads box j at an address that is the same in every lane, a broadcast (out of L2 every
// step of a scan waited for a load of its own: 0.2 us, which was the whole cost of a small page).  LDS per box: the box (16 B), the
// line box (16 B; succ and pred live there until the lines are known, the line ranks after the line boxes are written) and the forest
// (4 B): 36 B, 144 KB at 4096 boxes, sized by the caller's max_boxes.
//
// What the kernel does not trust: box_first is the caller's device table.  A page whose range does not lie inside [0, n_boxes] or runs
// backwards touches none of the per-box outputs; a page of more than max_boxes boxes gets -1 in all of its outputs (its rows exist: they
// are sized by the real counts).  Both report n_lines = med = -1.
#include "common.h"
#include "union_find.h"

namespace {

constexpr int THREADS = 1024, OWN = QEA_LINE_MAX_BOXES / THREADS, LDS_PER_BOX = 36;
static_assert(OWN * THREADS == QEA_LINE_MAX_BOXES, "a thread owns OWN boxes of the largest page");

struct Size {
  long long h, w;
  __device__ __forceinline__ bool some() const { return h > 0 && w > 0; }
};
__device__ __forceinline__ Size size_of(const int4 b) { return {(long long)b.w - b.y + 1, (long long)b.z - b.x + 1}; }

__global__ __launch_bounds__(THREADS) void line_group_kernel(const int4* __restrict__ boxes, const int32_t* __restrict__ box_first, int n_boxes,
                                                             int cap, int overlap, int tall, int gap, int32_t* __restrict__ line,
                                                             int32_t* __restrict__ pos, int32_t* __restrict__ order,
                                                             int4* __restrict__ line_box, int32_t* __restrict__ n_lines,
                                                             long long* __restrict__ med_out) {
  extern __shared__ int4 lds[];
  int4* B = lds;                                               // [cap]: the page's boxes
  int4* lbox = lds + cap;                                      // [cap]
  int* forest = (int*)(lds + 2 * cap);                         // [cap]: parent, then root, then line
  int* succ = (int*)lbox;                                      // [cap] each, until the lines are known
  int* pred = succ + cap;
  int* rank = succ;                                            // [cap]: the line number, at a line's root, once the line boxes are written
  __shared__ long long s_med;
  __shared__ int s_some, s_lines;

  const int page = blockIdx.x, tid = threadIdx.x;
  const long long first = box_first[page], end = box_first[page + 1];
  if (first < 0 || end < first || end > n_boxes) {             // uniform: no row of this page is known to exist
    if (tid == 0) {
      n_lines[page] = -1;
      med_out[page] = -1;
    }
    return;
  }
  if (end - first > cap) {                                     // uniform: the rows exist, the tables do not hold them
    for (long long i = first + tid; i < end; i += THREADS) {
      line[i] = pos[i] = order[i] = -1;
      line_box[i] = make_int4(-1, -1, -1, -1);
    }
    if (tid == 0) {
      n_lines[page] = -1;
      med_out[page] = -1;
    }
    return;
  }
  const int n = (int)(end - first);
  if (tid == 0) {
    s_med = 0;
    s_some = s_lines = 0;
  }
  __syncthreads();

  int4 b[OWN];
  Size sz[OWN];
  bool own[OWN], some[OWN];
  int mine = 0;
#pragma unroll
  for (int k = 0; k < OWN; ++k) {
    const int i = tid + k * THREADS;
    own[k] = i < n;
    b[k] = own[k] ? boxes[first + i] : make_int4(0, 0, -1, -1);
    if (own[k]) B[i] = b[k];
    sz[k] = size_of(b[k]);
    some[k] = own[k] && sz[k].some();
    mine += some[k];
  }
  if (mine) atomicAdd(&s_some, mine);
  __syncthreads();

  // ---- the median height of the non-empty boxes
  if (mine) {
    const int want = (s_some - 1) / 2;
    int below[OWN] = {};
    for (int j = 0; j < n; ++j) {
      const Size sj = size_of(B[j]);
      if (!sj.some()) continue;                                // uniform
#pragma unroll
      for (int k = 0; k < OWN; ++k) below[k] += sj.h < sz[k].h || (sj.h == sz[k].h && j < tid + k * THREADS);
    }
#pragma unroll
    for (int k = 0; k < OWN; ++k)
      if (some[k] && below[k] == want) s_med = sz[k].h;        // the ranks are distinct: one writer
  }
  __syncthreads();
  const long long med = s_med, tallest = (long long)tall * med, widest = (long long)gap * med;

  // ---- succ and pred: the nearest boxes of the same height band along x, kept where the gap rule links them
  bool linkable[OWN];
  bool any = false;
#pragma unroll
  for (int k = 0; k < OWN; ++k) any |= linkable[k] = some[k] && sz[k].h <= tallest;
  int sj[OWN], pj[OWN], s_x[OWN], p_x[OWN], p_xmax[OWN];
#pragma unroll
  for (int k = 0; k < OWN; ++k) sj[k] = pj[k] = -1, s_x[k] = p_x[k] = p_xmax[k] = 0;
  if (any) {
    for (int j = 0; j < n; ++j) {
      const int4 c = B[j];
      const Size sc = size_of(c);
      if (!sc.some() || sc.h > tallest) continue;              // uniform
#pragma unroll
      for (int k = 0; k < OWN; ++k) {
        const int i = tid + k * THREADS;
        if (!linkable[k] || j == i) continue;
        const long long ov = (long long)min(b[k].w, c.w) - max(b[k].y, c.y) + 1;
        if (100 * ov < (long long)overlap * min(sz[k].h, sc.h)) continue;
        if (c.x > b[k].x || (c.x == b[k].x && j > i)) {        // j ascends: of equal x_min the first seen is the smallest key
          if (sj[k] < 0 || c.x < s_x[k]) sj[k] = j, s_x[k] = c.x;
        } else if (pj[k] < 0 || c.x >= p_x[k]) {               // and the last seen the largest
          pj[k] = j, p_x[k] = c.x, p_xmax[k] = c.z;
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < OWN; ++k) {
    if (!own[k]) continue;
    const int i = tid + k * THREADS;
    const bool s_ok = sj[k] >= 0 && (gap == 0 || (long long)s_x[k] - b[k].z - 1 <= widest);
    const bool p_ok = pj[k] >= 0 && (gap == 0 || (long long)b[k].x - p_xmax[k] - 1 <= widest);
    succ[i] = s_ok ? sj[k] : -1;
    pred[i] = p_ok ? pj[k] : -1;
    forest[i] = i;
  }
  __syncthreads();

  // ---- lines: the components of the links
  const LdsForest f = {forest};
#pragma unroll
  for (int k = 0; k < OWN; ++k) {
    if (!own[k]) continue;
    const int i = tid + k * THREADS;
    if (succ[i] >= 0) unite(f, i, succ[i]);
    if (pred[i] >= 0) unite(f, i, pred[i]);
  }
  __syncthreads();                                             // succ and pred are dead: their words become the line boxes
  int root[OWN];
#pragma unroll
  for (int k = 0; k < OWN; ++k) {
    if (!own[k]) continue;
    const int i = tid + k * THREADS;
    root[k] = find_root(f, i);
    lbox[i] = make_int4(0x7fffffff, 0x7fffffff, -0x7fffffff - 1, -0x7fffffff - 1);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < OWN; ++k) {
    if (!own[k]) continue;
    const int i = tid + k * THREADS;
    forest[i] = root[k];
    atomicMin(&lbox[root[k]].x, b[k].x);
    atomicMin(&lbox[root[k]].y, b[k].y);
    atomicMax(&lbox[root[k]].z, b[k].z);
    atomicMax(&lbox[root[k]].w, b[k].w);
    if (root[k] == i) atomicAdd(&s_lines, 1);
  }
  __syncthreads();

  // ---- line order: a root's rank under (y_min + y_max, x_min, root)
  const int L = s_lines;
  bool is_root[OWN];
  bool any_root = false;
#pragma unroll
  for (int k = 0; k < OWN; ++k) any_root |= is_root[k] = own[k] && root[k] == tid + k * THREADS;
  int before_line[OWN] = {};
  if (any_root) {
    int4 lb[OWN];
    int before[OWN] = {};
#pragma unroll
    for (int k = 0; k < OWN; ++k) lb[k] = is_root[k] ? lbox[tid + k * THREADS] : make_int4(0, 0, 0, 0);
    for (int s = 0; s < n; ++s) {
      if (forest[s] != s) continue;                            // uniform
      const int4 c = lbox[s];
      const long long cy = (long long)c.y + c.w;
#pragma unroll
      for (int k = 0; k < OWN; ++k) {
        const long long y = (long long)lb[k].y + lb[k].w;
        before[k] += cy < y || (cy == y && (c.x < lb[k].x || (c.x == lb[k].x && s < tid + k * THREADS)));
      }
    }
#pragma unroll
    for (int k = 0; k < OWN; ++k)
      if (is_root[k]) {
        before_line[k] = before[k];
        line_box[first + before[k]] = lb[k];
      }
  }
  __syncthreads();                                             // the line boxes are dead: their words become the line ranks
#pragma unroll
  for (int k = 0; k < OWN; ++k)
    if (is_root[k]) rank[tid + k * THREADS] = before_line[k];
  __syncthreads();
  int ln[OWN];
#pragma unroll
  for (int k = 0; k < OWN; ++k) {
    if (!own[k]) continue;
    const int i = tid + k * THREADS;
    ln[k] = rank[root[k]];
    forest[i] = ln[k];                                         // nobody reads a root from here on
    line[first + i] = ln[k];
    if (i >= L) line_box[first + i] = make_int4(-1, -1, -1, -1);
  }
  __syncthreads();

  // ---- box order: a box's rank under (line, x_min, y_min, index)
  if (own[0]) {
    int before[OWN] = {};
    for (int j = 0; j < n; ++j) {
      const int lj = forest[j];
      const int4 c = B[j];
#pragma unroll
      for (int k = 0; k < OWN; ++k)
        before[k] += lj < ln[k] ||
                     (lj == ln[k] && (c.x < b[k].x || (c.x == b[k].x && (c.y < b[k].y || (c.y == b[k].y && j < tid + k * THREADS)))));
    }
#pragma unroll
    for (int k = 0; k < OWN; ++k) {
      if (!own[k]) continue;
      pos[first + tid + k * THREADS] = before[k];
      order[first + before[k]] = tid + k * THREADS;
    }
  }
  if (tid == 0) {
    n_lines[page] = L;
    med_out[page] = med;
  }
}

}  // namespace

extern "C" int qea_line_group(const int32_t* boxes, const int32_t* box_first, int32_t n_pages, int32_t n_boxes, int32_t max_boxes,
                              int32_t overlap, int32_t tall, int32_t gap, int32_t* line, int32_t* pos, int32_t* order, int32_t* line_box,
                              int32_t* n_lines, int64_t* med, void* stream) {
  const char* who = "qea_line_group";
  QEA_REQUIRE(n_pages >= 0, "%s: n_pages=%d is negative", who, n_pages);
  QEA_REQUIRE(n_boxes >= 0, "%s: n_boxes=%d is negative", who, n_boxes);
  QEA_REQUIRE(max_boxes >= 0 && max_boxes <= QEA_LINE_MAX_BOXES, "%s: max_boxes=%d outside 0..%d", who, max_boxes, QEA_LINE_MAX_BOXES);
  QEA_REQUIRE(overlap >= 1 && overlap <= 100, "%s: overlap=%d outside 1..100", who, overlap);
  QEA_REQUIRE(tall >= 1 && tall <= QEA_LINE_MAX_TALL, "%s: tall=%d outside 1..%d", who, tall, QEA_LINE_MAX_TALL);
  QEA_REQUIRE(gap >= 0 && gap <= QEA_LINE_MAX_GAP, "%s: gap=%d outside 0..%d", who, gap, QEA_LINE_MAX_GAP);
  QEA_REQUIRE(n_pages > 0 || n_boxes == 0, "%s: %d boxes and no page to hold them", who, n_boxes);
  if (n_pages == 0) return QEA_OK;
  QEA_REQUIRE(box_first && n_lines && med, "%s: box_first, n_lines or med is NULL", who);
  QEA_REQUIRE(((uintptr_t)box_first & 3) == 0 && ((uintptr_t)n_lines & 3) == 0 && ((uintptr_t)med & 7) == 0,
              "%s: box_first / n_lines must be 4-byte and med 8-byte aligned", who);
  hipStream_t s = (hipStream_t)stream;
  if (n_boxes == 0) {                                          // every page is empty: no line, med 0, and no kernel
    if (hipMemsetAsync(n_lines, 0, sizeof(int32_t) * (size_t)n_pages, s) != hipSuccess ||
        hipMemsetAsync(med, 0, sizeof(int64_t) * (size_t)n_pages, s) != hipSuccess) {
      qea_set_error("%s: hipMemsetAsync failed", who);
      return QEA_ERR_LAUNCH;
    }
    return QEA_OK;
  }
  QEA_REQUIRE(boxes && line && pos && order && line_box, "%s: boxes, line, pos, order or line_box is NULL", who);
  QEA_REQUIRE(((uintptr_t)boxes & 15) == 0 && ((uintptr_t)line_box & 15) == 0, "%s: boxes and line_box must be 16-byte aligned", who);
  QEA_REQUIRE((((uintptr_t)line | (uintptr_t)pos | (uintptr_t)order) & 3) == 0, "%s: line, pos and order must be 4-byte aligned", who);
  if (int rc = reserve_lds<line_group_kernel>(who, (size_t)LDS_PER_BOX * QEA_LINE_MAX_BOXES)) return rc;
  line_group_kernel<<<dim3((unsigned)n_pages), dim3(THREADS), (size_t)LDS_PER_BOX * max_boxes, s>>>(
      (const int4*)boxes, box_first, n_boxes, max_boxes, overlap, tall, gap, line, pos, order, (int4*)line_box, n_lines, (long long*)med);
  QEA_CHECK_LAUNCH();
  return QEA_OK;
}
