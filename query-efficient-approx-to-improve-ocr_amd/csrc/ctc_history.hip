// Label-history weighted CTC loss (tracking_utils.py:59-75) in one device pass: include/qea_hip.h: qea_ctc_history_loss.
//
// A strip n carries up to W problems, one per history depth i, which all read the same log-prob rows lp[:, n, :]:
//   loss        = sum_{n,i present} coef[n,i] * nll[n,i]
//   grad[t,n,c] = sum_i coef[n,i] * (exp(lp) - exp(lse_{s: l'_s = c}(alpha+beta) + nll - lp))
// with coef = w / depth_n (sample-wise weights) or w / (depth_n * max(len,1)) (decaying weights).  Three launches whatever W:
//   1. ctc_history_scan_kernel    grid (N, W, pass): the alpha / beta recursion of problem (n, i): ctc_core.h's ctc_scan, the one
//                                 ctc.hip's ctc_alpha_beta_kernel runs (one thread per extended-label state, one barrier per time
//                                 step, fp64), absent depths exit at once.  alpha, beta [N][W][T][S_max] and nll [N][W] go to the workspace.
//   2. ctc_history_coef_kernel    one workgroup: coef[n,i] in fp64, the fp32 nll table, and the loss by a fixed-order tree.
//   3. ctc_history_grad_kernel    grid (N, T): stages alpha+beta and l' of every present depth in LDS (W * S_max * 12 bytes), then
//                                 thread c sums the depths in ascending order in fp64 and writes grad[t,n,c] ONCE, rounded once.
// No atomics, no zero-fill, no [T, n_i, C] intermediate: bit-reproducible.  The recursion, the gradient's inner loop and the tree sum are
// ctc_core.h's, shared with ctc.hip: at W = 1 the two entry points agree bit for bit (tests/test_history_ctc_gpu.py pins it).
// Bytes: 2 * T*N*C*4 (lp in, grad out) + 2 * 2 * N*W*T*S_max*8 (alpha/beta written once, read once).  Latency-bound scan.
#include "ctc_core.h"

namespace {

constexpr int HW_MAX = QEA_HISTORY_MAX_WINDOW;
constexpr int GRAD_THREADS = 128;

// alpha (blockIdx.z == 0) and beta (blockIdx.z == 1) of problem (n, i) = (blockIdx.x, blockIdx.y); one thread per state
__global__ __launch_bounds__(CTC_MAX_S) void ctc_history_scan_kernel(const float* __restrict__ lp, int ld_t, int ld_n,
                                                                      const int* __restrict__ in_len, const int* __restrict__ lens,
                                                                      const int* __restrict__ offs, const int* __restrict__ chars, int T,
                                                                      int W, int blank, double* __restrict__ alpha,
                                                                      double* __restrict__ beta, double* __restrict__ nll64, int S_max) {
  __shared__ double prev[2][CTC_MAX_S + 2];
  const int n = blockIdx.x;
  const size_t p = (size_t)n * W + blockIdx.y;   // problem index
  const int L = lens[p];
  if (L < 0) return;                             // no label at this depth
  const bool is_beta = blockIdx.z == 1;
  const double v = ctc_scan(lp + (size_t)n * ld_n, ld_t, chars + offs[p], L, min(in_len[n], T), blank, S_max, is_beta,
                            (is_beta ? beta : alpha) + p * T * S_max, prev);
  if (!is_beta && threadIdx.x == 0) nll64[p] = v;
}

// coef[n,i] (0 where the depth is absent), nll [N][W] in fp32 (0 where absent), loss = sum coef * nll in a fixed order
__global__ __launch_bounds__(256) void ctc_history_coef_kernel(const int* __restrict__ lens, const int* __restrict__ depth_n,
                                                                const float* __restrict__ w, int w_stride_n, int w_stride_i,
                                                                int mean_by_length, int N, int W, const double* __restrict__ nll64,
                                                                double* __restrict__ coef, float* __restrict__ nll,
                                                                float* __restrict__ loss) {
  double acc = 0;
  const long long total = (long long)N * W;
  for (long long p = threadIdx.x; p < total; p += 256) {
    const int n = (int)(p / W), i = (int)(p % W);
    const int L = lens[p];
    double cf = 0, nl = 0;
    if (L >= 0) {
      double den = (double)max(depth_n[i], 1);
      if (mean_by_length) den *= (double)max(L, 1);
      cf = (double)w[(long long)n * w_stride_n + (long long)i * w_stride_i] / den;
      nl = nll64[p];
      acc += cf * nl;
    }
    coef[p] = cf;
    nll[p] = (float)nl;
  }
  const double sum = ctc_tree_sum_256(acc);
  if (threadIdx.x == 0) loss[0] = (float)sum;
}

// grad row (t, n): the depths present are staged in LDS, thread c then scans the states carrying character c depth by depth
__global__ __launch_bounds__(GRAD_THREADS) void ctc_history_grad_kernel(const float* __restrict__ lp, int ld_t, int ld_n,
                                                                         const int* __restrict__ in_len, const int* __restrict__ lens,
                                                                         const int* __restrict__ offs, const int* __restrict__ chars,
                                                                         int T, int C, int W, int blank, const double* __restrict__ alpha,
                                                                         const double* __restrict__ beta, const double* __restrict__ nll64,
                                                                         const double* __restrict__ coef, float* __restrict__ grad,
                                                                         int gld_t, int gld_n, int S_max) {
  extern __shared__ double dyn[];                 // ab [W][S_max] fp64, then ext [W][S_max] int32
  __shared__ int sS[HW_MAX];                      // states of depth i, 0 = absent (or longer than S_max: contributes nothing)
  __shared__ double sNll[HW_MAX], sCoef[HW_MAX];
  double* ab = dyn;
  int* ext = (int*)(dyn + (size_t)W * S_max);
  const int n = blockIdx.x, t = blockIdx.y;
  const int Tn = min(in_len[n], T);
  float* grow = grad + (size_t)n * gld_n + (size_t)t * gld_t;
  if (t >= Tn) {
    for (int c = threadIdx.x; c < C; c += GRAD_THREADS) grow[c] = 0.f;
    return;
  }
  if (threadIdx.x < W) {
    const size_t p = (size_t)n * W + threadIdx.x;
    const int L = lens[p];
    const int S = 2 * L + 1;
    sS[threadIdx.x] = (L >= 0 && S <= S_max) ? S : 0;
    sNll[threadIdx.x] = nll64[p];
    sCoef[threadIdx.x] = coef[p];
  }
  __syncthreads();
  for (int i = 0; i < W; ++i) {
    const int S = sS[i];
    const size_t p = (size_t)n * W + i;
    ctc_stage_row(alpha + (p * T + t) * S_max, beta + (p * T + t) * S_max, chars + offs[p], S, blank, ab + i * S_max, ext + i * S_max,
                  GRAD_THREADS);
  }
  __syncthreads();
  const float* lpr = lp + (size_t)n * ld_n + (size_t)t * ld_t;
  for (int c = threadIdx.x; c < C; c += GRAD_THREADS) {
    const double l = (double)lpr[c];
    const double e = exp(l);
    double acc = 0;
    for (int i = 0; i < W; ++i) {
      const int S = sS[i];
      if (S == 0) continue;
      const double res = ctc_lse_char(ab + i * S_max, ext + i * S_max, S, c);
      acc += sCoef[i] * (e - exp(res + sNll[i] - l));
    }
    grow[c] = (float)acc;
  }
}

}  // namespace

extern "C" size_t qea_ctc_history_workspace_bytes(int32_t T, int32_t N, int32_t W, int32_t S_max) {
  if (T <= 0 || N <= 0 || W <= 0 || S_max <= 0) return 0;
  return ((size_t)2 * T * S_max + 2) * (size_t)N * W * sizeof(double);
}

extern "C" int qea_ctc_history_loss(const float* lp, int32_t ld_t, int32_t ld_n, const int32_t* input_lengths, const int32_t* lens,
                                    const int32_t* offs, const int32_t* chars, const int32_t* depth_n, const float* weights,
                                    int32_t w_stride_n, int32_t w_stride_i, int32_t mean_by_length, int32_t T, int32_t N, int32_t C,
                                    int32_t W, int32_t blank, int32_t S_max, float* loss, float* grad, int32_t gld_t, int32_t gld_n,
                                    float* nll, void* workspace, size_t workspace_bytes, void* stream) {
  QEA_REQUIRE(lp && input_lengths && lens && offs && chars && depth_n && weights && loss && nll, "qea_ctc_history_loss: null pointer");
  QEA_REQUIRE(T > 0 && T <= 65535 && N > 0 && C > 0 && blank >= 0 && blank < C, "qea_ctc_history_loss: bad dimensions");
  QEA_REQUIRE(W >= 1 && W <= HW_MAX, "qea_ctc_history_loss: W=%d must be in [1,%d]", W, HW_MAX);
  if (const int rc = ctc_check_s_max("qea_ctc_history_loss", S_max)) return rc;
  QEA_REQUIRE(w_stride_n >= 0 && w_stride_i >= 0, "qea_ctc_history_loss: negative weight stride");
  QEA_REQUIRE(workspace && workspace_bytes >= qea_ctc_history_workspace_bytes(T, N, W, S_max), "qea_ctc_history_loss: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const size_t P = (size_t)N * W;
  double* alpha = (double*)workspace;
  double* beta = alpha + P * T * S_max;
  double* nll64 = beta + P * T * S_max;
  double* coef = nll64 + P;
  hipLaunchKernelGGL(ctc_history_scan_kernel, dim3(N, W, grad ? 2 : 1), dim3(ctc_scan_threads(S_max)), 0, s, lp, ld_t, ld_n, input_lengths, lens,
                     offs, chars, T, W, blank, alpha, beta, nll64, S_max);
  hipLaunchKernelGGL(ctc_history_coef_kernel, dim3(1), dim3(256), 0, s, lens, depth_n, weights, w_stride_n, w_stride_i, mean_by_length, N, W,
                     (const double*)nll64, coef, nll, loss);
  if (grad) {
    const size_t lds = (size_t)W * S_max * (sizeof(double) + sizeof(int));
    hipLaunchKernelGGL(ctc_history_grad_kernel, dim3(N, T), dim3(GRAD_THREADS), lds, s, lp, ld_t, ld_n, input_lengths, lens, offs, chars, T, C,
                       W, blank, (const double*)alpha, (const double*)beta, (const double*)nll64, (const double*)coef, grad, gld_t, gld_n,
                       S_max);
  }
  QEA_CHECK_LAUNCH();
  return QEA_OK;
}
