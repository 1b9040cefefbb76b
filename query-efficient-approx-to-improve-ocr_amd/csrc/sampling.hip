// The two minibatch samplers that pick on estimates (include/qea_hip.h: qea_spread_pick, qea_seq_entropy).
//
// spread_pick_kernel: the range sampling of selection_utils.py (k serial nearest-estimate picks without replacement) as ONE
// workgroup.  The loop over the k points cannot be split, so the kernel makes one pass cheap: the private copy `left` sits in
// LDS (or, above QEA_SPREAD_LDS_MAX_N, in the caller's workspace) padded with NaN to whole 16-byte chunks, thread t scans chunks
// t, t + T, ... and keeps (distance, index) with a strict `<`, so the lowest index of equal distances survives inside a thread (its
// indices ascend); the threads meet in a lexicographic (distance, index) butterfly.  A NaN distance (padding) never passes `<`.
// With more than one wave the wave winners meet in a double-buffered LDS slot behind ONE barrier per pick.  The thread that scans
// chunk j / 4 is the one that writes left[j] = 100, so the only reader of an overwritten element is its writer: no fence, and the
// one-wave form has no barrier inside the loop at all.  The next point is loaded one pick ahead of its use.
// Routing by n.  Measured on an MI355X with tools/bench_samplers.py (device events, k = 256), time per pick in us, linear in n:
//   one wave        0.63 + 0.27 n / 1024    (0.76 at n = 512, 1.18 at 2048: no barrier, the scan is one wave's)
//   four waves      0.93 + 0.07 n / 1024    (1.14 at 2049, 1.49 at 8192: one per SIMD, one barrier per pick)
//   sixteen waves   1.89 + 0.03 n / 1024    (2.15 at 8193, 2.92 at 32768: sixteen slots to read behind the barrier)
// The lines cross at n = 1.5 k and n = 25.7 k:
//   n <= QEA_SPREAD_WAVE_MAX_N (1536)    one wave
//   n <= QEA_SPREAD_LDS4_MAX_N (24576)   four waves
//   n <= QEA_SPREAD_LDS_MAX_N (32768)    sixteen waves, left still in LDS (128 KiB)
//   above                                sixteen waves, left in the workspace (3.2 us per pick at 32769, 4.5 at 65536: L2-resident)
//
// seq_entropy_kernel: one wave per strip b walks the T * C log-probs of lp[:, b, :] (element e = t * C + c, lane-strided), adds
// -p log(p + 1e-6) in fp64 and rounds mean_t / log(num_classes) once.  exp(-inf) = 0 and 0 * log(1e-6) = 0: no NaN.
#include "common.h"
#include <math.h>

namespace {

constexpr int SP_CAP = QEA_SPREAD_LDS_MAX_N;           // floats of dynamic LDS the sixteen-wave form may ask for
constexpr int SE_THREADS = 256;

template <int NW, bool IN_WORKSPACE>
__global__ __launch_bounds__(NW * QEA_WAVE) void spread_pick_kernel(const float* __restrict__ est, int n, const float* __restrict__ pts, int k,
                                                                   int64_t* __restrict__ idx, float* __restrict__ ws) {
#pragma clang fp contract(off)
  extern __shared__ f32x4 sp_left[];
  __shared__ float slot_d[2][NW];
  __shared__ int slot_i[2][NW];
  constexpr int T = NW * QEA_WAVE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n4 = (n + 3) >> 2;
  float* left = IN_WORKSPACE ? ws : reinterpret_cast<float*>(sp_left);
  const f32x4* left4 = reinterpret_cast<const f32x4*>(left);
  for (int j = tid; j < n4 * 4; j += T) left[j] = j < n ? est[j] : __builtin_nanf("");
  __syncthreads();
  float p_next = pts[0];
  for (int i = 0; i < k; ++i) {
    const float p = p_next;
    p_next = pts[i + 1 < k ? i + 1 : i];
    float bd = INFINITY;
    int bi = tid * 4;                                   // thread 0 answers 0 when every distance is +inf, as argmin does
    for (int q = tid; q < n4; q += T) {
      const f32x4 v = left4[q];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float d = fabsf(p - v[c]);
        if (d < bd) {
          bd = d;
          bi = q * 4 + c;
        }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float d2 = __shfl_xor(bd, o, 64);
      const int i2 = __shfl_xor(bi, o, 64);
      if (d2 < bd || (d2 == bd && i2 < bi)) {
        bd = d2;
        bi = i2;
      }
    }
    if constexpr (NW > 1) {
      const int par = i & 1;                            // a wave two picks ahead has passed the barrier every reader of this slot reaches after reading
      if (lane == 0) {
        slot_d[par][wave] = bd;
        slot_i[par][wave] = bi;
      }
      __syncthreads();
      bd = slot_d[par][0];
      bi = slot_i[par][0];
#pragma unroll
      for (int w = 1; w < NW; ++w) {
        const float d2 = slot_d[par][w];
        const int i2 = slot_i[par][w];
        if (d2 < bd || (d2 == bd && i2 < bi)) {
          bd = d2;
          bi = i2;
        }
      }
    }
    const int j = bi < n ? bi : 0;                      // (bi is always a real index; the clamp keeps the store below in bounds regardless)
    if (tid == 0) idx[i] = (int64_t)j;
    if (tid == ((j >> 2) % T)) left[j] = 100.0f;
  }
}

__global__ __launch_bounds__(SE_THREADS) void seq_entropy_kernel(const float* __restrict__ lp, long long ld_t, long long ld_n, int T, int B, int C,
                                                                 int num_classes, float* __restrict__ out) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * (SE_THREADS / QEA_WAVE) + (threadIdx.x >> 6);
  if (b >= B) return;                                   // whole waves leave together
  const float* base = lp + (size_t)b * ld_n;
  double acc = 0.0;
  const int E = T * C;
  for (int e = lane; e < E; e += QEA_WAVE) {
    const int t = e / C, c = e - t * C;
    const double p = exp((double)base[(size_t)t * ld_t + c]);
    acc -= p * log(p + 0.000001);
  }
  acc = qea_wave_sum_d(acc);
  if (lane == 0) out[b] = (float)((acc / (double)T) / log((double)num_classes));
}

template <int NW, bool IN_WORKSPACE>
int launch_spread(const float* est, int n, const float* pts, int k, int64_t* idx, float* ws, hipStream_t s) {
  const size_t lds = IN_WORKSPACE ? 0 : (size_t)((n + 3) / 4) * 16;
  if (lds > 48 * 1024) {
    const int rc = reserve_lds<spread_pick_kernel<NW, IN_WORKSPACE>>("qea_spread_pick", (size_t)SP_CAP * 4);
    if (rc != QEA_OK) return rc;
  }
  hipLaunchKernelGGL((spread_pick_kernel<NW, IN_WORKSPACE>), dim3(1), dim3(NW * QEA_WAVE), lds, s, est, n, pts, k, idx, ws);
  QEA_CHECK_LAUNCH();
  return QEA_OK;
}

}  // namespace

extern "C" size_t qea_spread_pick_workspace_bytes(int32_t n) {
  if (n <= QEA_SPREAD_LDS_MAX_N || n > QEA_SPREAD_MAX_N) return 0;
  return (size_t)((n + 3) / 4) * 16;
}

extern "C" int qea_spread_pick(const float* est, int32_t n, const float* pts, int32_t k, int64_t* idx, void* workspace, void* stream) {
  QEA_REQUIRE(est && pts && idx, "qea_spread_pick: null pointer");
  QEA_REQUIRE(n >= 1 && n <= QEA_SPREAD_MAX_N, "qea_spread_pick: n=%d outside 1..%d", n, QEA_SPREAD_MAX_N);
  QEA_REQUIRE(k >= 1 && k <= QEA_SPREAD_MAX_N, "qea_spread_pick: k=%d outside 1..%d", k, QEA_SPREAD_MAX_N);
  hipStream_t s = (hipStream_t)stream;
  // thresholds: include/qea_hip.h (measured, profiles/samplers.json)
  if (n <= QEA_SPREAD_WAVE_MAX_N) return launch_spread<1, false>(est, n, pts, k, idx, nullptr, s);
  if (n <= QEA_SPREAD_LDS4_MAX_N) return launch_spread<4, false>(est, n, pts, k, idx, nullptr, s);
  if (n <= QEA_SPREAD_LDS_MAX_N) return launch_spread<16, false>(est, n, pts, k, idx, nullptr, s);
  QEA_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0, "qea_spread_pick: n=%d needs a 16-byte aligned workspace of %zu bytes", n,
              qea_spread_pick_workspace_bytes(n));
  return launch_spread<16, true>(est, n, pts, k, idx, (float*)workspace, s);
}

extern "C" int qea_seq_entropy(const float* lp, int64_t ld_t, int64_t ld_n, int32_t T, int32_t B, int32_t C, int32_t num_classes, float* out,
                               void* stream) {
  QEA_REQUIRE(lp && out, "qea_seq_entropy: null pointer");
  QEA_REQUIRE(T >= 1 && T <= 65535 && B >= 1 && B <= (1 << 24) && C >= 1 && C <= 65535, "qea_seq_entropy: T=%d B=%d C=%d out of range", T, B, C);
  QEA_REQUIRE((long long)T * C <= (1ll << 30), "qea_seq_entropy: T * C = %lld exceeds 2^30", (long long)T * C);
  QEA_REQUIRE(num_classes >= 2, "qea_seq_entropy: num_classes=%d must be at least 2", num_classes);
  QEA_REQUIRE(ld_t >= 0 && ld_n >= 0, "qea_seq_entropy: negative stride");
  hipLaunchKernelGGL(seq_entropy_kernel, dim3(qea_cdiv(B, SE_THREADS / QEA_WAVE)), dim3(SE_THREADS), 0, (hipStream_t)stream, lp,
                     (long long)ld_t, (long long)ld_n, T, B, C, num_classes, out);
  QEA_CHECK_LAUNCH();
  return QEA_OK;
}
