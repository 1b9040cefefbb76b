// The derived FILTER forms: after every optimiser step each 3x3 layer needs its filter as fp16 fragment planes (forward) and its
// flip-transposed filter as fragment planes (input gradient), each 1x1 / GEMM layer its fragment planes — about 110 forms of a few
// microseconds each per training step (a tenth of a B = 32 step when each had a launch of its own).  This file owns them: every form
// has ONE device body, a grid-stride function of (first item, stride), and its layout is written down once, next to that body.
// qea_weight_forms_multi runs a table of jobs (<= 64, in the kernel arguments; blockIdx.y = job) through the bodies in one launch;
// the single entry points of the flip and the fp16 planes are that launch with one job, and the bf16 planes (qea_pack_frag_planes,
// no job kind) are a kernel of their own over the same 32-row index map.  The bytes of every form, single and multi, are pinned by
// tests/golden/weight_form_digests.json (tests/test_kernels_gpu.py::test_weight_forms_multi_equals_the_single_launches).
#include "common.h"
#include "../../include/qea_hip.h"

namespace {

constexpr int MAXJ = 64;
struct JobTable {
  qea_wform_job j[MAXJ];
};

// ---- which shapes a form takes and how many items (one lane's 8 channels of one fragment; one element of the flip) it has: the
// entry points check with these, the bodies loop over them
__host__ __device__ inline bool flip_shape(int Co, int Ci, int KH, int KW) { return Co > 0 && Ci > 0 && KH > 0 && KW > 0; }
__host__ __device__ inline long long flip_items(int Co, int Ci, int KH, int KW) { return (long long)Co * KH * KW * Ci; }
__host__ __device__ inline bool planes3_shape(int N, int Cin) {
  return (N == 32 || N == 64 || (N > 0 && N % 128 == 0)) && (Cin == 32 || (Cin % 64 == 0 && Cin <= 512));
}
__host__ __device__ inline bool planes3_rows16(int Cin) { return Cin % 64 == 0; }     // fp16 planes only: which of the two orders
__host__ __device__ inline long long rows32_items(int N, int Cin) { return 9LL * (Cin / 16) * (N / 32) * 64; }
__host__ __device__ inline long long rows16_items(int N, int Cin) { return 9LL * (Cin / 32) * (N / 16) * 64; }
__host__ __device__ inline bool planes1_shape(int N, int K) {
  return N > 0 && N % 128 == 0 && K > 0 && K % 64 == 0 && (long long)N * K * 4 < 0x7fffffffLL;
}
__host__ __device__ inline long long planes1_items(int N, int K) { return (long long)(N / 128) * (K / 64) * 4 * 4 * 64; }

// ---- flip-transpose: conv weight [Co][KH][KW][Ci] -> input-gradient filter [Ci][KH][KW][Co] with the taps flipped
__device__ __forceinline__ void flip_body(const float* __restrict__ w, float* __restrict__ wt, int Co, int Ci, int KH, int KW, long long i0,
                                          long long stride) {
  const long long n = flip_items(Co, Ci, KH, KW);
  for (long long i = i0; i < n; i += stride) {                  // i indexes wt: (ci, kh', kw', co), co fastest
    const int co = (int)(i % Co);
    long long r = i / Co;
    const int kw2 = (int)(r % KW);
    r /= KW;
    const int kh2 = (int)(r % KH);
    const int ci = (int)(r / KH);
    wt[i] = w[(((size_t)co * KH + (KH - 1 - kh2)) * KW + (KW - 1 - kw2)) * Ci + ci];
  }
}

// ---- fragment planes.  An item is one lane of one MFMA B fragment: 8 consecutive channels of one filter row, split into `planes`
// 8-value vectors.  The index maps below give, in elements: where the 8 floats sit in the filter, where the first plane's vector
// goes, and the distance from one plane's vector to the next.
struct Frag {
  size_t src, dst, plane;
};

// 3x3, 32-row order (conv3x3_halo_bf3_kernel, 32x32x16 MFMA): w [N][9][Cin] -> [n-block][chunk][step = tap * KS + cs][plane][nj][lane][8],
// n-block = min(N, 128) output channels (one workgroup column), chunk width CW = 32 (Cin = 32) or 64 channels, KS = CW / 16: lane
// (n = nj * 32 + (lane & 31), half = lane >> 5) holds channels chunk * CW + cs * 16 + 8 * half + 0..7 of filter row n at `tap`
__device__ __forceinline__ Frag rows32_frag(int i, int N, int Cin, int planes) {
  const int NB = N > 128 ? 128 : N, CW = Cin == 32 ? 32 : 64;
  const int KSr = CW / 16, WNr = NB / 32, chunks = Cin / CW;
  const int lane = i & 63, nj = (i >> 6) % WNr;
  const int gst = (i >> 6) / WNr;                               // (n-block, chunk, step) flattened
  const int nbk = gst / (chunks * 9 * KSr);
  const int chunk = (gst / (9 * KSr)) % chunks, st = gst % (9 * KSr);
  const int tap = st / KSr, cs = st % KSr;
  const int n = nbk * NB + nj * 32 + (lane & 31);
  return {((size_t)n * 9 + tap) * Cin + chunk * CW + cs * 16 + 8 * (lane >> 5), ((((size_t)gst * planes) * WNr + nj) * 64 + lane) * 8,
          (size_t)WNr * 64 * 8};
}

// 3x3, 16-row order (conv3x3_halo_m16_kernel, 16x16x32 MFMA; Cin % 64 == 0): [n-block][chunk][step = tap * 2 + ks][plane][16-channel
// group][lane][8]: lane l of group g holds filter row n-block * NB + g * 16 + (l & 15), channels chunk * 64 + ks * 32 + 8 (l >> 4) + 0..7
__device__ __forceinline__ Frag rows16_frag(int i, int N, int Cin) {
  const int NB = N > 128 ? 128 : N;
  const int NGr = NB / 16, chunks = Cin / 64;
  const int lane = i & 63, ng = (i >> 6) % NGr;
  const int gst = (i >> 6) / NGr;                               // (n-block, chunk, step) flattened
  const int nbk = gst / (chunks * 18);
  const int chunk = (gst / 18) % chunks, st = gst % 18;
  const int tap = st / 2, ks = st % 2;
  const int n = nbk * NB + ng * 16 + (lane & 15);
  return {((size_t)n * 9 + tap) * Cin + chunk * 64 + ks * 32 + 8 * (lane >> 4), ((((size_t)gst * 2) * NGr + ng) * 64 + lane) * 8,
          (size_t)NGr * 64 * 8};
}

// 1x1 (gemm1x1_f16_kernel): w [N][K] -> [128-column block][chunk][cs][plane][nj4][lane][8]: lane (n = 32 nj + (lane & 31),
// half = lane >> 5) holds channels 64 chunk + 16 cs + 8 half + 0..7 of filter row n
__device__ __forceinline__ Frag gemm_frag(int i, int K) {
  const int chunks = K / 64;
  const int lane = i & 63, nj = (i >> 6) & 3;
  const int gst = i >> 8;                                       // (column block, chunk, cs) flattened
  const int nbk = gst / (chunks * 4);
  const int chunk = (gst >> 2) % chunks, cs = gst & 3;
  const int n = nbk * 128 + nj * 32 + (lane & 31);
  return {(size_t)n * K + chunk * 64 + cs * 16 + 8 * (lane >> 5), ((((size_t)gst * 2) * 4 + nj) * 64 + lane) * 8, (size_t)4 * 64 * 8};
}

// The fp16 forms: two planes (h, l) of the filter SCALED by s_w (qea_f16_scale of the abs-max `amax`), followed — at element
// offset 2 * elems, elems the filter's size — by one float: 1 / s_w.  `at`: item -> Frag.
template <class Map>
__device__ __forceinline__ void planes_f16_body(const float* __restrict__ w, _Float16* __restrict__ dst, size_t elems, const float* __restrict__ amax,
                                                long long total, long long i0, long long stride, Map at) {
  float sw, inv;
  qea_f16_scale(amax[0], sw, inv);
  if (i0 == 0) reinterpret_cast<float*>(dst + elems * 2)[0] = inv;
  for (long long i = i0; i < total; i += stride) {
    const Frag f = at((int)i);
    const f32x4 v0 = *reinterpret_cast<const f32x4*>(w + f.src), v1 = *reinterpret_cast<const f32x4*>(w + f.src + 4);
    f16x4 h0, l0, h1, l1;
    qea_split2_f16(v0, sw, h0, l0);
    qea_split2_f16(v1, sw, h1, l1);
    f16x8 ph, pl;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      ph[k] = h0[k]; ph[k + 4] = h1[k];
      pl[k] = l0[k]; pl[k + 4] = l1[k];
    }
    *reinterpret_cast<f16x8*>(dst + f.dst) = ph;
    *reinterpret_cast<f16x8*>(dst + f.dst + f.plane) = pl;
  }
}

// The bf16 form of the 32-row order: three planes (h, m, l: qea_split3), unscaled, nothing behind them.
__device__ __forceinline__ void planes_bf16_body(const float* __restrict__ w, __bf16* __restrict__ dst, int N, int Cin, long long i0, long long stride) {
  const long long total = rows32_items(N, Cin);
  for (long long i = i0; i < total; i += stride) {
    const Frag f = rows32_frag((int)i, N, Cin, 3);
    const f32x4 v0 = *reinterpret_cast<const f32x4*>(w + f.src), v1 = *reinterpret_cast<const f32x4*>(w + f.src + 4);
    bf16x4 h0, m0, l0, h1, m1, l1;
    qea_split3(v0, h0, m0, l0);
    qea_split3(v1, h1, m1, l1);
    bf16x8 pl[3];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      pl[0][k] = h0[k]; pl[0][k + 4] = h1[k];
      pl[1][k] = m0[k]; pl[1][k + 4] = m1[k];
      pl[2][k] = l0[k]; pl[2][k + 4] = l1[k];
    }
#pragma unroll
    for (int p = 0; p < 3; ++p) *reinterpret_cast<bf16x8*>(dst + f.dst + p * f.plane) = pl[p];
  }
}

__global__ __launch_bounds__(256) void weight_forms_kernel(const JobTable t) {
  const qea_wform_job& jb = t.j[blockIdx.y];
  const long long stride = (long long)gridDim.x * 256;
  const long long i0 = (long long)blockIdx.x * 256 + threadIdx.x;
  const int a = jb.a, b = jb.b;
  if (jb.kind == 0) {
    flip_body(jb.src, (float*)jb.dst, a, b, jb.c, jb.d, i0, stride);
  } else if (jb.kind == 2) {
    planes_f16_body(jb.src, (_Float16*)jb.dst, (size_t)a * b, jb.amax, planes1_items(a, b), i0, stride, [=](int i) { return gemm_frag(i, b); });
  } else if (planes3_rows16(b)) {
    planes_f16_body(jb.src, (_Float16*)jb.dst, (size_t)a * 9 * b, jb.amax, rows16_items(a, b), i0, stride, [=](int i) { return rows16_frag(i, a, b); });
  } else {
    planes_f16_body(jb.src, (_Float16*)jb.dst, (size_t)a * 9 * b, jb.amax, rows32_items(a, b), i0, stride, [=](int i) { return rows32_frag(i, a, b, 2); });
  }
}

__global__ __launch_bounds__(256) void pack_frag_planes_kernel(const float* __restrict__ w, __bf16* __restrict__ dst, int N, int Cin) {
  planes_bf16_body(w, dst, N, Cin, (long long)blockIdx.x * 256 + threadIdx.x, (long long)gridDim.x * 256);
}

// items of a job whose kind and shape the entry point has accepted
long long job_items(const qea_wform_job& j) {
  if (j.kind == 0) return flip_items(j.a, j.b, j.c, j.d);
  if (j.kind == 2) return planes1_items(j.a, j.b);
  return planes3_rows16(j.b) ? rows16_items(j.a, j.b) : rows32_items(j.a, j.b);
}

// n jobs of at most `most` items each; at most `cap` workgroups per job, grid-stride beyond
int launch_forms(const JobTable& t, int n, long long most, int cap, void* stream) {
  hipLaunchKernelGGL(weight_forms_kernel, dim3((unsigned)qea_grid_for(most, cap), (unsigned)n), dim3(256), 0, (hipStream_t)stream, t);
  QEA_CHECK_LAUNCH();
  return QEA_OK;
}

// a single entry point's launch: the chip is this job's alone, so up to 4096 workgroups
int launch_one(const qea_wform_job& j, void* stream) {
  JobTable t = {};
  t.j[0] = j;
  return launch_forms(t, 1, job_items(j), 4096, stream);
}

}  // namespace

extern "C" int qea_weight_forms_multi(const qea_wform_job* jobs, int32_t n, void* stream) {
  QEA_REQUIRE(jobs && n > 0 && n <= MAXJ, "qea_weight_forms_multi: 1 to 64 jobs");
  JobTable t;
  long long most = 0;
  for (int i = 0; i < n; ++i) {
    const qea_wform_job& j = jobs[i];
    QEA_REQUIRE(j.src && j.dst && j.kind >= 0 && j.kind <= 2 && (j.kind == 0 || j.amax), "qea_weight_forms_multi: null pointer or unknown kind in a job");
    QEA_REQUIRE(((uintptr_t)j.src & 15) == 0 && ((uintptr_t)j.dst & 15) == 0, "qea_weight_forms_multi: pointers must be 16-byte aligned");
    if (j.kind == 0)
      QEA_REQUIRE(flip_shape(j.a, j.b, j.c, j.d), "qea_weight_forms_multi: bad flip-transpose shape");
    else if (j.kind == 1)
      QEA_REQUIRE(j.b > 0 && planes3_shape(j.a, j.b), "qea_weight_forms_multi: 3x3 planes need N in {32, 64, 128k}, Cin = 32 or a multiple of 64 up to 512");
    else
      QEA_REQUIRE(planes1_shape(j.a, j.b), "qea_weight_forms_multi: 1x1 planes need N a multiple of 128, K a multiple of 64");
    const long long items = job_items(j);
    QEA_REQUIRE(items < 0x7fffffffLL, "qea_weight_forms_multi: a job is too large");
    if (items > most) most = items;
    t.j[i] = j;
  }
  return launch_forms(t, n, most, 512, stream);                 // 512 x n workgroups fill the chip anyway
}

extern "C" int qea_filter_flip_transpose(const float* w, float* wt, int32_t Co, int32_t Ci, int32_t KH, int32_t KW, void* stream) {
  QEA_REQUIRE(w && wt && flip_shape(Co, Ci, KH, KW), "qea_filter_flip_transpose: bad arguments");
  return launch_one({w, wt, nullptr, 0, Co, Ci, KH, KW}, stream);
}

extern "C" size_t qea_pack_frag_planes_bytes(int32_t N, int32_t Cin) { return (size_t)N * 9 * Cin * 6; }

extern "C" int qea_pack_frag_planes(const float* w, int32_t N, int32_t Cin, void* planes, void* stream) {
  QEA_REQUIRE(w && planes && planes3_shape(N, Cin), "qea_pack_frag_planes: N in {32, 64, 128k}, Cin = 32 or a multiple of 64 up to 512");
  hipLaunchKernelGGL(pack_frag_planes_kernel, dim3(qea_grid_for(rows32_items(N, Cin))), dim3(256), 0, (hipStream_t)stream, w, (__bf16*)planes, N, Cin);
  QEA_CHECK_LAUNCH();
  return QEA_OK;
}

extern "C" size_t qea_pack_frag_planes_f16_bytes(int32_t N, int32_t Cin) { return (size_t)N * 9 * Cin * 4 + 16; }

extern "C" int qea_pack_frag_planes_f16(const float* w, int32_t N, int32_t Cin, const float* wmax, void* planes, void* stream) {
  QEA_REQUIRE(w && planes && wmax && planes3_shape(N, Cin), "qea_pack_frag_planes_f16: N in {32, 64, 128k}, Cin = 32 or a multiple of 64 up to 512");
  return launch_one({w, planes, wmax, 1, N, Cin, 0, 0}, stream);
}

extern "C" size_t qea_pack_frag_planes_f16_1x1_bytes(int32_t N, int32_t K) { return (size_t)N * K * 4 + 16; }

extern "C" int qea_pack_frag_planes_f16_1x1(const float* w, int32_t N, int32_t K, const float* wmax, void* planes, void* stream) {
  QEA_REQUIRE(w && planes && wmax && planes1_shape(N, K), "qea_pack_frag_planes_f16_1x1: N a multiple of 128, K a multiple of 64");
  QEA_REQUIRE(((uintptr_t)w & 15) == 0 && ((uintptr_t)planes & 15) == 0, "qea_pack_frag_planes_f16_1x1: pointers must be 16-byte aligned");
  return launch_one({w, planes, wmax, 2, N, K, 0, 0}, stream);
}
