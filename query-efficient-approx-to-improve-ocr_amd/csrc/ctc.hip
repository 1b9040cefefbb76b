// log_softmax (+ backward with the reference's NaN scrub) and the CTC loss / gradient.
//
// CTC follows ATen's native recursion (Graves 2006 eq. 6-16 in log space).  The recursion, the
// per-sample nll and the gradient formula run in fp64 (inputs/outputs fp32): with |log-likelihood|
// ~ 1e2 an fp32 recursion carries ~1e-5 absolute error into exp(alpha+beta+nll-lp), i.e. a 1e-5..1e-4
// RELATIVE error common to every (t,c) of a sample, which per-channel sums downstream amplify
// (measured: bias gradients 4-7x further from the exact value than ATen's fp32 path).  fp64 costs
// nothing here (latency-bound scan, 2*T*S values per sample).
//   alpha_t(s) = lse(alpha_{t-1}(s), alpha_{t-1}(s-1), [alpha_{t-1}(s-2)]) + lp[t, l'_s]
// one workgroup per sample, one thread per extended-label state (S = 2L+1 <= 256),
// one barrier per time step; alpha and beta go to a caller-owned workspace and a second kernel
// forms   grad[t,n,c] = (exp(lp) - exp(lse_{s: l'_s = c}(alpha+beta) + nll - lp)) * grad_out[n]
// exactly as ATen does (reference call sites: train_nn_patch.py:143,178,294).
// Latency-bound (31-step scan); bytes: 2 * T*N*C*4 in/out + 2 * N*T*S*4 workspace.
// The recursion, the gradient's inner loop and the tree sum live in ctc_core.h, shared with ctc_history.hip.
#include "ctc_core.h"

namespace {

// one wave per row
__global__ __launch_bounds__(256) void log_softmax_fwd_kernel(const float* __restrict__ x, int ldx, float* __restrict__ y, int ldy, long long M,
                                                              int C) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const float* xr = x + row * ldx;
  float mx = -INFINITY;
  for (int c = lane; c < C; c += 64) mx = fmaxf(mx, xr[c]);
  mx = qea_wave_max(mx);
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += expf(xr[c] - mx);
  s = qea_wave_sum(s);
  // (x - mx) - log s, not x - (mx + log s): the latter rounds at the size of mx, which a common offset of the logits makes arbitrarily
  // larger than the result
  const float ls = logf(s);
  for (int c = lane; c < C; c += 64) y[row * ldy + c] = (xr[c] - mx) - ls;
}

// dx = g - exp(lp) * sum_c g ; optional NaN -> 0 (models/model_crnn.py:30-32); pad columns -> 0
__global__ __launch_bounds__(256) void log_softmax_bwd_kernel(const float* __restrict__ g, int ldg, const float* __restrict__ lp, int ldlp,
                                                              float* __restrict__ dx, int lddx, long long M, int C, int Cpad, int scrub) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  // the row sum and the product with it in fp64: an fp32 sum's rounding, times the row's largest probability, would be the largest
  // term of the error (a row is C <= a few hundred values: the fp64 adds cost nothing next to the loads)
  double s = 0.0;
  for (int c = lane; c < C; c += 64) s += (double)g[row * ldg + c];
  s = qea_wave_sum_d(s);
  for (int c = lane; c < Cpad; c += 64) {
    float v = 0.f;
    if (c < C) {
      v = (float)((double)g[row * ldg + c] - (double)expf(lp[row * ldlp + c]) * s);
      if (scrub && v != v) v = 0.f;
    }
    dx[row * lddx + c] = v;
  }
}

// alpha (blockIdx.y == 0) and beta (blockIdx.y == 1) recursions: one workgroup per (sample, pass), one thread per state
__global__ __launch_bounds__(CTC_MAX_S) void ctc_alpha_beta_kernel(const float* __restrict__ lp, int ld_t, int ld_n,
                                                                    const int* __restrict__ targets, const long long* __restrict__ tg_off,
                                                                    const int* __restrict__ in_len, const int* __restrict__ tg_len, int T,
                                                                    int blank, double* __restrict__ alpha, double* __restrict__ beta,
                                                                    float* __restrict__ nll, double* __restrict__ nll64, int S_max) {
  __shared__ double prev[2][CTC_MAX_S + 2];
  const int n = blockIdx.x;
  const bool is_beta = blockIdx.y == 1;
  const double v = ctc_scan(lp + (size_t)n * ld_n, ld_t, targets + tg_off[n], tg_len[n], min(in_len[n], T), blank, S_max, is_beta,
                            (is_beta ? beta : alpha) + (size_t)n * T * S_max, prev);
  if (!is_beta && threadIdx.x == 0) {
    nll64[n] = v;
    nll[n] = (float)v;
  }
}

// grad for one (n, t) row: thread c scans the states carrying character c
__global__ __launch_bounds__(128) void ctc_grad_kernel(const float* __restrict__ lp, int ld_t, int ld_n, const int* __restrict__ targets,
                                                       const long long* __restrict__ tg_off, const int* __restrict__ in_len,
                                                       const int* __restrict__ tg_len, int T, int C, int blank,
                                                       const double* __restrict__ alpha, const double* __restrict__ beta,
                                                       const double* __restrict__ nll, const float* __restrict__ grad_out,
                                                       float* __restrict__ grad, int gld_t, int gld_n, int S_max) {
  __shared__ double ab[CTC_MAX_S];
  __shared__ int ext[CTC_MAX_S];
  const int n = blockIdx.x, t = blockIdx.y;
  const int L = tg_len[n], Tn = min(in_len[n], T);
  const int S = 2 * L + 1;
  float* grow = grad + (size_t)n * gld_n + (size_t)t * gld_t;
  if (t >= Tn || S > S_max) {
    for (int c = threadIdx.x; c < C; c += blockDim.x) grow[c] = 0.f;
    return;
  }
  const int* tg = targets + tg_off[n];
  const double* al = alpha + ((size_t)n * T + t) * S_max;
  const double* be = beta + ((size_t)n * T + t) * S_max;
  ctc_stage_row(al, be, tg, S, blank, ab, ext, blockDim.x);
  __syncthreads();
  const double nl = nll[n];
  const double go = (double)grad_out[n];
  const float* lpr = lp + (size_t)n * ld_n + (size_t)t * ld_t;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    const double res = ctc_lse_char(ab, ext, S, c);
    const double l = (double)lpr[c];
    grow[c] = (float)((exp(l) - exp(res + nl - l)) * go);
  }
}

__global__ void ctc_reduce_kernel(const double* __restrict__ nll, const int* __restrict__ tg_len, int N, int reduction, float scale_in,
                                  float* __restrict__ loss, float* __restrict__ grad_out) {
  // reduction 1 = mean: loss = mean_n(nll_n / max(len_n,1)), grad_out_n = scale_in / (N * max(len_n,1))
  // reduction 0 = none: grad_out_n = scale_in (caller multiplies by its own upstream gradient)
  double acc = 0;
  for (int n = threadIdx.x; n < N; n += blockDim.x) {
    const float tl = (float)max(tg_len[n], 1);
    if (reduction == 1) {
      acc += nll[n] / (double)tl;
      grad_out[n] = scale_in / ((float)N * tl);
    } else {
      acc += nll[n];
      grad_out[n] = scale_in;
    }
  }
  const double sum = ctc_tree_sum_256(acc);
  if (threadIdx.x == 0) loss[0] = (reduction == 1) ? (float)(sum / (double)N) : (float)sum;
}

}  // namespace

extern "C" int qea_log_softmax_fwd(const float* x, int32_t ldx, float* y, int32_t ldy, int64_t M, int32_t C, void* stream) {
  QEA_REQUIRE(x && y && M > 0 && C > 0, "qea_log_softmax_fwd: bad arguments");
  hipLaunchKernelGGL(log_softmax_fwd_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, ldx, y, ldy, (long long)M, C);
  QEA_CHECK_LAUNCH();
  return QEA_OK;
}

extern "C" int qea_log_softmax_bwd(const float* g, int32_t ldg, const float* lp, int32_t ldlp, float* dx, int32_t lddx, int64_t M, int32_t C,
                                   int32_t Cpad, int32_t nan_scrub, void* stream) {
  QEA_REQUIRE(g && lp && dx && M > 0 && C > 0 && Cpad >= C && lddx >= Cpad, "qea_log_softmax_bwd: bad arguments");
  hipLaunchKernelGGL(log_softmax_bwd_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, (hipStream_t)stream, g, ldg, lp, ldlp, dx, lddx,
                     (long long)M, C, Cpad, nan_scrub);
  QEA_CHECK_LAUNCH();
  return QEA_OK;
}

extern "C" size_t qea_ctc_workspace_bytes(int32_t T, int32_t N, int32_t S_max) {
  if (T <= 0 || N <= 0 || S_max <= 0) return 0;
  return (size_t)2 * N * T * S_max * sizeof(double) + (size_t)N * sizeof(double) + (size_t)N * sizeof(float);
}

extern "C" int qea_ctc_loss(const float* lp, int32_t ld_t, int32_t ld_n, const int32_t* targets, const int64_t* target_offsets,
                            const int32_t* input_lengths, const int32_t* target_lengths, int32_t T, int32_t N, int32_t C, int32_t blank,
                            int32_t S_max, int32_t reduction, float grad_scale, float* nll, float* loss, float* grad, int32_t gld_t,
                            int32_t gld_n, void* workspace, size_t workspace_bytes, void* stream) {
  QEA_REQUIRE(lp && targets && target_offsets && input_lengths && target_lengths && nll && loss, "qea_ctc_loss: null pointer");
  QEA_REQUIRE(T > 0 && N > 0 && C > 0 && blank >= 0 && blank < C, "qea_ctc_loss: bad dimensions");
  if (const int rc = ctc_check_s_max("qea_ctc_loss", S_max)) return rc;
  QEA_REQUIRE(workspace && workspace_bytes >= qea_ctc_workspace_bytes(T, N, S_max), "qea_ctc_loss: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  double* alpha = (double*)workspace;
  double* beta = alpha + (size_t)N * T * S_max;
  double* nll64 = beta + (size_t)N * T * S_max;
  float* gout = (float*)(nll64 + N);
  hipLaunchKernelGGL(ctc_alpha_beta_kernel, dim3(N, grad ? 2 : 1), dim3(ctc_scan_threads(S_max)), 0, s, lp, ld_t, ld_n, targets,
                     (const long long*)target_offsets, input_lengths, target_lengths, T, blank, alpha, beta, nll, nll64, S_max);
  hipLaunchKernelGGL(ctc_reduce_kernel, dim3(1), dim3(256), 0, s, (const double*)nll64, target_lengths, N, reduction, grad_scale, loss, gout);
  if (grad) {
    hipLaunchKernelGGL(ctc_grad_kernel, dim3(N, T), dim3(128), 0, s, lp, ld_t, ld_n, targets, (const long long*)target_offsets, input_lengths,
                       target_lengths, T, C, blank, (const double*)alpha, (const double*)beta, (const double*)nll64, (const float*)gout, grad,
                       gld_t, gld_n, S_max);
  }
  QEA_CHECK_LAUNCH();
  return QEA_OK;
}
