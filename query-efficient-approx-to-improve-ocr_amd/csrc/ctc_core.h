// The CTC recursion shared by ctc.hip (one problem per sample) and ctc_history.hip (up to W problems per strip): the alpha / beta
// scan of ONE problem, the two pieces of the gradient's inner loop, the fixed-order fp64 tree sum, and the two host-side lines
// (S_max check, thread count) that both launchers need.  ctc_align.hip, the max-product member of the family, shares the states
// (ctc_state), the thread count and the bound check.  fp64 on purpose.  An infeasible label gives nll = +inf and
// NaN gradient rows; CRNN's NaN scrub depends on that convention.
#pragma once
#include "common.h"

constexpr int CTC_MAX_S = 256;

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

// host side of the scan: S_max is the caller's bound on 2L+1 (QEA_OK or QEA_ERR_INVALID with the message set), one thread per state
// in whole waves
static inline int ctc_check_s_max(const char* fn, int S_max) {
  QEA_REQUIRE(S_max >= 1 && S_max <= CTC_MAX_S, "%s: S_max=%d must be in [1,%d] (targets up to %d chars)", fn, S_max, CTC_MAX_S,
              (CTC_MAX_S - 1) / 2);
  return QEA_OK;
}
static inline int ctc_scan_threads(int S_max) { return ((S_max + 63) / 64) * 64; }
// the same check for a caller that bounds the label length instead (ctc_align.hip): S_max = 2 L_max + 1
constexpr int CTC_MAX_L = (CTC_MAX_S - 1) / 2;
static inline int ctc_check_l_max(const char* fn, int L_max) {
  QEA_REQUIRE(L_max >= 0 && L_max <= CTC_MAX_L, "%s: L_max=%d must be in [0,%d] (%d extended states)", fn, L_max, CTC_MAX_L, CTC_MAX_S);
  return QEA_OK;
}

// state s of the extended label of tg[0..L), S = 2L + 1: its class l'_s (blank for even s and for s >= S) and whether the recursion may
// skip into it: from s - 2 going forward, to s + 2 going backward (is_beta)
__device__ __forceinline__ void ctc_state(const int* __restrict__ tg, int s, int S, int blank, bool is_beta, int& ch, bool& skip) {
  ch = blank;
  skip = false;
  if (s < S && (s & 1)) {
    ch = tg[s >> 1];
    if (!is_beta) skip = (s >= 2) && (tg[(s >> 1) - 1] != ch);
    else skip = (s + 2 < S) && (tg[(s >> 1) + 1] != ch);
  }
}

// alpha (is_beta false) or beta recursion of one problem by one workgroup, one thread per extended-label state:
//   alpha_t(s) = lse(alpha_{t-1}(s), alpha_{t-1}(s-1), [alpha_{t-1}(s-2)]) + lp[t, l'_s]
// lpn: the sample's log-probs (row t at lpn + t * ld_t), tg: its L characters, out: its [T][S_max] rows, prev: two LDS rows.
// Thread 0 of the alpha pass gets the nll; a problem with Tn <= 0 or more than S_max states is infeasible: +inf, nothing written.
// That exit is uniform over the workgroup and comes before the first barrier.
__device__ __forceinline__ double ctc_scan(const float* __restrict__ lpn, int ld_t, const int* __restrict__ tg, int L, int Tn, int blank,
                                           int S_max, bool is_beta, double* __restrict__ out, double (*prev)[CTC_MAX_S + 2]) {
  const int s = threadIdx.x;
  const int S = 2 * L + 1;
  int ch;      // l'_s
  bool skip;   // alpha: may come from s-2 ; beta: may go to s+2
  ctc_state(tg, s, S, blank, is_beta, ch, skip);
  if (Tn <= 0 || S > S_max) return (double)INFINITY;

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
  double nl = 0;
  if (!is_beta && s == 0) {
    // prev[buf] holds alpha_{Tn-1}
    const double a = prev[buf][(S - 1) + 2];
    const double b = (S > 1) ? prev[buf][(S - 2) + 2] : NEG_INF_D;
    nl = -lse2(a, b);
  }
  return nl;
}

// gradient row t of one problem: ab[s] = alpha_t(s) + beta_t(s) and ext[s] = l'_s, the workgroup's threads `stride` apart
__device__ __forceinline__ void ctc_stage_row(const double* __restrict__ al, const double* __restrict__ be, const int* __restrict__ tg, int S,
                                              int blank, double* ab, int* ext, int stride) {
  for (int s = threadIdx.x; s < S; s += stride) {
    ab[s] = al[s] + be[s];
    ext[s] = (s & 1) ? tg[s >> 1] : blank;
  }
}

// lse_{s: l'_s = c}(alpha + beta) over a staged row
__device__ __forceinline__ double ctc_lse_char(const double* ab, const int* ext, int S, int c) {
  double res = NEG_INF_D;
  for (int s = 0; s < S; ++s)
    if (ext[s] == c) res = lse2(res, ab[s]);
  return res;
}

// sum of one value per thread in a fixed order.  The workgroup has exactly 256 threads, ALL of them reach this call (it holds
// barriers), and a kernel calls it once (one LDS array).  Every thread gets the sum.
__device__ __forceinline__ double ctc_tree_sum_256(double acc) {
  __shared__ double sred[256];
  sred[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) sred[threadIdx.x] += sred[threadIdx.x + o];
    __syncthreads();
  }
  return sred[0];
}
