// Label-history weighted CTC loss (tracking_utils.py:59-75) in one device pass: include/qea_hip.h: qea_ctc_history_loss.
//
// A strip n carries up to W problems, one per history depth i, which all read the same log-prob rows lp[:, n, :]:
//   loss        = sum_{n,i present} coef[n,i] * nll[n,i]
//   grad[t,n,c] = sum_i coef[n,i] * (exp(lp) - exp(lse_{s: l'_s = c}(alpha+beta) + nll - lp))
// with coef = w / depth_n (sample-wise weights) or w / (depth_n * max(len,1)) (decaying weights).  Three launches whatever W:
//   1. ctc_history_scan_kernel    grid (N, W, pass): the alpha / beta recursion of problem (n, i) exactly as ctc.hip's
//                                 ctc_alpha_beta_kernel runs it (one thread per extended-label state, one barrier per time step,
//                                 fp64), absent depths exit at once.  alpha, beta [N][W][T][S_max] and nll [N][W] go to the workspace.
//   2. ctc_history_coef_kernel    one workgroup: coef[n,i] in fp64, the fp32 nll table, and the loss by a fixed-order tree.
//   3. ctc_history_grad_kernel    grid (N, T): stages alpha+beta and l' of every present depth in LDS (W * S_max * 12 bytes), then
//                                 thread c sums the depths in ascending order in fp64 and writes grad[t,n,c] ONCE, rounded once.
// No atomics, no zero-fill, no [T, n_i, C] intermediate: bit-reproducible.  The recursion below repeats ctc.hip's on purpose: that
// file's kernels and entry points are left exactly as they are.
// Bytes: 2 * T*N*C*4 (lp in, grad out) + 2 * 2 * N*W*T*S_max*8 (alpha/beta written once, read once).  Latency-bound scan.
#include "common.h"

namespace {

constexpr int CTC_MAX_S = 256;
constexpr int HW_MAX = QEA_HISTORY_MAX_WINDOW;
constexpr int GRAD_THREADS = 128;

#define NEG_INF_D (-(double)INFINITY)
__device__ __forceinline__ double lse3(double a, double b, double c) {
  const double m = fmax(fmax(a, b), c);
  if (m == NEG_INF_D) return NEG_INF_D;
  return m + log(exp(a - m) + exp(b - m) + exp(c - m));
}
__device__ __forceinline__ double lse2(double a, double b) {
  const double m = fmax(a, b);
  if (m == NEG_INF_D) return NEG_INF_D;
  return m + log(exp(a - m) + exp(b - m));
}

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
  const int s = threadIdx.x;
  const int Tn = min(in_len[n], T);
  const int S = 2 * L + 1;
  const int* tg = chars + offs[p];
  const float* lpn = lp + (size_t)n * ld_n;
  double* out = (is_beta ? beta : alpha) + p * T * S_max;

  int ch = blank;      // l'_s
  bool skip = false;   // alpha: may come from s-2 ; beta: may go to s+2
  if (s < S && (s & 1)) {
    ch = tg[s >> 1];
    if (!is_beta) skip = (s >= 2) && (tg[(s >> 1) - 1] != ch);
    else skip = (s + 2 < S) && (tg[(s >> 1) + 1] != ch);
  }
  if (Tn <= 0 || S > S_max) {  // degenerate / longer than the caller sized for: infeasible
    if (!is_beta && s == 0) nll64[p] = (double)INFINITY;
    return;
  }

  // prev rows are padded by 2 on the side the recursion reaches into
  double cur = NEG_INF_D;
  if (!is_beta) {
    if (s == 0) cur = (double)lpn[blank];
    else if (s == 1 && S > 1) cur = (double)lpn[ch];
  } else {
    const float* lpt = lpn + (size_t)(Tn - 1) * ld_t;
    if (s == S - 1) cur = (double)lpt[blank];
    else if (s == S - 2 && S > 1) cur = (double)lpt[ch];
  }
  int buf = 0;
  if (s < 2) {
    prev[0][is_beta ? CTC_MAX_S + s : s] = NEG_INF_D;  // padding cells
    prev[1][is_beta ? CTC_MAX_S + s : s] = NEG_INF_D;
  }
  // storage index: alpha uses prev[.][s+2] (reads s+1, s), beta uses prev[.][s] (reads s+1, s+2)
  const int off = is_beta ? 0 : 2;
  if (s < S) out[(size_t)(is_beta ? Tn - 1 : 0) * S_max + s] = cur;
  prev[buf][s + off] = (s < S) ? cur : NEG_INF_D;
  __syncthreads();
  for (int step = 1; step < Tn; ++step) {
    const int t = is_beta ? Tn - 1 - step : step;
    double v = NEG_INF_D;
    if (s < S) {
      double a0, a1, a2;
      if (!is_beta) {
        a0 = prev[buf][s + 2];
        a1 = prev[buf][s + 1];
        a2 = skip ? prev[buf][s] : NEG_INF_D;
      } else {
        a0 = prev[buf][s];
        a1 = (s + 1 < S) ? prev[buf][s + 1] : NEG_INF_D;
        a2 = skip ? prev[buf][s + 2] : NEG_INF_D;
      }
      v = lse3(a0, a1, a2) + (double)lpn[(size_t)t * ld_t + ch];
      out[(size_t)t * S_max + s] = v;
    }
    buf ^= 1;
    prev[buf][s + off] = v;
    __syncthreads();
  }
  if (!is_beta && s == 0) {
    // prev[buf] holds alpha_{Tn-1}
    const double a = prev[buf][(S - 1) + 2];
    const double b = (S > 1) ? prev[buf][(S - 2) + 2] : NEG_INF_D;
    nll64[p] = -lse2(a, b);
  }
}

// coef[n,i] (0 where the depth is absent), nll [N][W] in fp32 (0 where absent), loss = sum coef * nll in a fixed order
__global__ __launch_bounds__(256) void ctc_history_coef_kernel(const int* __restrict__ lens, const int* __restrict__ depth_n,
                                                                const float* __restrict__ w, int w_stride_n, int w_stride_i,
                                                                int mean_by_length, int N, int W, const double* __restrict__ nll64,
                                                                double* __restrict__ coef, float* __restrict__ nll,
                                                                float* __restrict__ loss) {
  __shared__ double sred[256];
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
  sred[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) sred[threadIdx.x] += sred[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = (float)sred[0];
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
    const int* tg = chars + offs[p];
    const double* al = alpha + (p * T + t) * S_max;
    const double* be = beta + (p * T + t) * S_max;
    for (int s = threadIdx.x; s < S; s += GRAD_THREADS) {
      ab[i * S_max + s] = al[s] + be[s];
      ext[i * S_max + s] = (s & 1) ? tg[s >> 1] : blank;
    }
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
      double res = NEG_INF_D;
      for (int s = 0; s < S; ++s)
        if (ext[i * S_max + s] == c) res = lse2(res, ab[i * S_max + s]);
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
  QEA_REQUIRE(S_max >= 1 && S_max <= CTC_MAX_S, "qea_ctc_history_loss: S_max=%d must be in [1,%d] (targets up to %d chars)", S_max,
              CTC_MAX_S, (CTC_MAX_S - 1) / 2);
  QEA_REQUIRE(w_stride_n >= 0 && w_stride_i >= 0, "qea_ctc_history_loss: negative weight stride");
  QEA_REQUIRE(workspace && workspace_bytes >= qea_ctc_history_workspace_bytes(T, N, W, S_max), "qea_ctc_history_loss: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const size_t P = (size_t)N * W;
  double* alpha = (double*)workspace;
  double* beta = alpha + P * T * S_max;
  double* nll64 = beta + P * T * S_max;
  double* coef = nll64 + P;
  const int threads = ((S_max + 63) / 64) * 64;
  hipLaunchKernelGGL(ctc_history_scan_kernel, dim3(N, W, grad ? 2 : 1), dim3(threads), 0, s, lp, ld_t, ld_n, input_lengths, lens, offs, chars,
                     T, W, blank, alpha, beta, nll64, S_max);
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
